"""Llama-8B serving decode: graphed single-token step at B=1 and B=8.

``--int8`` runs the weight-only int8 A/B instead (scripts/_decode_ab.py):
bf16 against ``quantize_linears_`` weights in the same process, B = 1 and 8
at max_seq/prompt 192/128 and 4096/2048, ``--attn-impl`` in both arms.
``--int4`` adds an int4 arm (``bits=4``): bf16, int8 and int4 in one process.

``--prefill-attn`` runs the prefill-attention A/B (scripts/
kbench_prefill_attn.py): time to first token at a 2048-token prompt and
ms/token of speculative decoding, ``TDPA_PREFILL_ATTN`` off against on.

``--chunk-attn`` runs the chunk-attention A/B (scripts/kbench_chunk_attn.py):
ms/token of speculative decoding with k = 8 at context 2048,
``TDPA_CHUNK_ATTN`` off against on.

``--kv-fp8`` runs the fp8 KV cache A/B (scripts/kbench_decode_attn_fp8.py):
bf16 cache against fp8 cache on the hip route, ms/token, time to first token
and resident cache bytes.

``--kv-paged`` runs the paged KV cache A/B (scripts/
kbench_decode_attn_paged.py): contiguous against paged caches (page 16,
permuted table) on the hip route, ms/token at 4096/2048, B = 1 and 8.

``--sample`` runs the sampling A/B (scripts/kbench_sample.py): graphed greedy
against graphed sampled decode (ops.sample_logits inside the graph) and eager
``generate`` with ``sampler="torch"`` against ``"hip"``, ms/token at
4096/2048, B = 1 and 8.

``--fused-decode`` runs the fused decode step A/B (scripts/
kbench_fused_decode.py): ``TDPA_FUSED_DECODE`` off against on, bf16 and int4
weights, graphed ms/token at 4096/2048, B = 1 and 8."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd.inference.generate import GraphedLlamaDecoder
from torchdistpackage_amd.models.llama import LlamaModel, llama3_8b

PROMPT, NEW = 128, 64
dev = torch.device("cuda")
torch.manual_seed(0)
ap = argparse.ArgumentParser()
ap.add_argument("--int8", action="store_true")
ap.add_argument("--int4", action="store_true")
ap.add_argument("--prefill-attn", action="store_true")
ap.add_argument("--chunk-attn", action="store_true")
ap.add_argument("--kv-fp8", action="store_true")
ap.add_argument("--kv-paged", action="store_true")
ap.add_argument("--sample", action="store_true")
ap.add_argument("--fused-decode", action="store_true")
ap.add_argument("--attn-impl", default="hip", choices=("hip", "sdpa"))
args = ap.parse_args()
m = LlamaModel(llama3_8b(), device=dev, dtype=torch.bfloat16).eval()

if args.int8 or args.int4:
    from _decode_ab import weights_ab
    weights_ab(m, GraphedLlamaDecoder, 128256, args.attn_impl, "llama-8b",
               bits=(8, 4) if args.int4 else (8,))
    print(f"LLAMA DECODE INT{4 if args.int4 else 8} AB OK")
    sys.exit(0)

if args.prefill_attn:
    from kbench_prefill_attn import end_to_end
    end_to_end(m)
    print("LLAMA PREFILL ATTN AB OK")
    sys.exit(0)

if args.chunk_attn:
    from kbench_chunk_attn import end_to_end
    end_to_end(m)
    print("LLAMA CHUNK ATTN AB OK")
    sys.exit(0)

if args.kv_fp8:
    from kbench_decode_attn_fp8 import end_to_end
    end_to_end(m)
    print("LLAMA KV FP8 AB OK")
    sys.exit(0)

if args.kv_paged:
    from kbench_decode_attn_paged import end_to_end
    end_to_end(m)
    print("LLAMA KV PAGED AB OK")
    sys.exit(0)

if args.sample:
    from kbench_sample import end_to_end
    end_to_end(m)
    print("LLAMA SAMPLE AB OK")
    sys.exit(0)

if args.fused_decode:
    from kbench_fused_decode import end_to_end
    end_to_end(m)
    print("LLAMA FUSED DECODE AB OK")
    sys.exit(0)

for B in (1, 8):
    idx = torch.randint(0, 128256, (B, PROMPT), device=dev)
    dec = GraphedLlamaDecoder(m, batch=B, max_seq=PROMPT + NEW)
    dec.prefill(idx)
    for _ in range(8):
        dec.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = NEW - 8
    for _ in range(n):
        dec.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"llama-8b graphed decode B={B}: {dt/n*1e3:.2f} ms/step, "
          f"{B*n/dt:.0f} tok/s")
print("LLAMA DECODE OK")
