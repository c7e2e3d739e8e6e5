"""Chunk attention A/P/C: the split-KV MFMA kernel (ops.chunk_attention)
against the two kernels the hip route has for a short chunk of new rows over
a KV cache.

    (A) row-blocked ops.decode_attention, one launch pair per 16 // G query
        positions, each streaming the visible cache again
    (P) ops.prefill_attention, one launch, no split over the keys
    (C) ops.chunk_attention, one launch pair

Op level: one process, the three arms alternating call by call, device
events, median of N calls after warm-up, three repeats; the spread of an arm
is (max - min) / min over its repeats.  The caches rotate through more than
512 MB so no arm is timed out of the Infinity Cache.  (C)'s share of the HBM
bound (the visible K and V bytes read once over the spec peak) is printed
next to its time, and max |C - A| at every point.

End to end (``--e2e-only``, or scripts/bench_decode_llama.py --chunk-attn):
Llama-8B, ``attn_impl="hip"``, ms/token of speculative_generate with k = 8 at
context 2048, ``TDPA_CHUNK_ATTN`` off against on, three alternating repeats.

    python scripts/kbench_chunk_attn.py [--op-only | --e2e-only]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kbench_prefill_attn import (HBM_PEAK, REPEATS, ROTATE_BYTES, _report,
                                 _timed, time_arms)
from torchdistpackage_amd import ops

dev = torch.device("cuda")


@torch.no_grad()
def op_level():
    assert ops.extension_available(), "HIP extension must be built"
    print("## op level, us: (A) row-blocked decode_attention, (P) "
          "prefill_attention, (C) chunk_attention; median of N calls, "
          f"{REPEATS} repeats, spread = (max-min)/min")
    print(f"{'model':>6s} {'B':>2s} {'keys':>5s} {'Sq':>3s} {'rows':>4s} "
          f"{'(A)':>8s} {'(P)':>8s} {'(C)':>8s} {'A/C':>6s} {'P/C':>6s} "
          f"{'sprA%':>6s} {'sprP%':>6s} {'sprC%':>6s} {'%HBM':>5s} "
          f"{'|C-A|':>8s}")
    missed = []
    for name, Hq, Hkv, D in (("llama", 32, 8, 128), ("gpt2", 16, 16, 128)):
        G = Hq // Hkv
        for B in (1, 8):
            for keys in (2048, 8000):
                for rows in (17, 24, 32, 64):
                    Sq = -(-rows // G)          # llama: 20, 24, 32, 64 rows
                    pos0, Smax = keys - Sq, keys
                    kv_bytes = 2 * B * Hkv * Smax * D * 2
                    ncopy = -(-ROTATE_BYTES // kv_bytes)
                    g = torch.Generator(device="cuda").manual_seed(0)

                    def rn(*s):
                        return torch.randn(*s, device=dev, generator=g,
                                           dtype=torch.bfloat16)

                    ks = [rn(B, Hkv, Smax, D) for _ in range(ncopy)]
                    vs = [rn(B, Hkv, Smax, D) for _ in range(ncopy)]
                    q = rn(B, Hq, Sq, D)
                    fa, fp, fc = (
                        lambda i, f=f: f(q, ks[i % ncopy], vs[i % ncopy], pos0)
                        for f in (ops.decode_attention, ops.prefill_attention,
                                  ops.chunk_attention))
                    diff = (fc(0).float() - fa(0).float()).abs().max().item()
                    reps = [time_arms((fa, fp, fc), 50, 3)
                            for _ in range(REPEATS)]
                    ta, tp, tc = (statistics.median(r[a] for r in reps)
                                  for a in range(3))
                    spr = [(max(r[a] for r in reps) - min(r[a] for r in reps))
                           / min(r[a] for r in reps) for a in range(3)]
                    t_hbm = 2 * B * Hkv * keys * D * 2 / HBM_PEAK
                    print(f"{name:>6s} {B:2d} {keys:5d} {Sq:3d} {G * Sq:4d} "
                          f"{ta:8.1f} {tp:8.1f} {tc:8.1f} {ta / tc:6.2f} "
                          f"{tp / tc:6.2f} {100 * spr[0]:6.1f} "
                          f"{100 * spr[1]:6.1f} {100 * spr[2]:6.1f} "
                          f"{100 * t_hbm / (tc * 1e-6):5.1f} {diff:8.4f}",
                          flush=True)
                    if G * Sq in (32, 64):
                        best, sb = min((ta, spr[0]), (tp, spr[1]))
                        if not best / tc - 1 > max(sb, spr[2]):
                            missed.append((name, B, keys, G * Sq))
                    del ks, vs
                    torch.cuda.empty_cache()
    print("bar (a), (C) faster than the better of (A) and (P) by more than "
          "the larger spread at every 32- and 64-row point: "
          + ("MET" if not missed else f"MISSED at {missed}"), flush=True)


@torch.no_grad()
def end_to_end(m=None):
    from torchdistpackage_amd.inference.generate import speculative_generate
    from torchdistpackage_amd.models.llama import (LlamaConfig, LlamaModel,
                                                   llama3_8b)
    print("## end to end: Llama-8B, attn_impl='hip', speculative_generate "
          f"k=8 at context 2048, TDPA_CHUNK_ATTN off against on, {REPEATS} "
          "alternating repeats")
    torch.manual_seed(0)
    if m is None:
        m = LlamaModel(llama3_8b(), device=dev, dtype=torch.bfloat16).eval()
    draft = LlamaModel(LlamaConfig(n_layer=2), device=dev,
                       dtype=torch.bfloat16).eval()
    idx = torch.randint(0, 128256, (1, 2048), device=dev)
    times = {"off": [], "on": []}
    prev = ops.chunk_attention_enabled()
    try:
        for rep in range(REPEATS + 1):              # repeat 0 is the warm-up
            for tag, on in (("off", False), ("on", True)):
                ops.set_chunk_attention(on)
                # the 2048-token prompt is in both calls: their difference
                # is 64 tokens of draft + verification rounds
                t8 = _timed(lambda: speculative_generate(
                    m, draft, idx, 8, k=8, attn_impl="hip"))
                t72 = _timed(lambda: speculative_generate(
                    m, draft, idx, 72, k=8, attn_impl="hip"))
                if rep:
                    times[tag].append((t72 - t8) / 64)
    finally:
        ops.set_chunk_attention(prev)
    met = _report("speculative_generate k=8, context 2048, ms/token", times,
                  "off", "on")
    print("bar (b), knob on faster than off beyond the repeat spread: "
          + ("MET" if met else "MISSED"), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--e2e-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if not args.e2e_only:
        op_level()
    if not args.op_only:
        end_to_end()
    print("KBENCH CHUNK ATTN OK")
