"""fp8 KV cache A/B: decode attention over an fp8 cache (ops.Fp8KV,
csrc/decode_attn_fp8.hip) against the bf16 kernel (csrc/decode_attn.hip).

Op level: (A) bf16 and (B) fp8 decode_attention timed in one process,
alternating call by call, with device events (median of ITERS calls after
warm-up), three repeats per point, spread = (max-min)/min of the medians.
The caches rotate through more than 512 MB.  Rates are valid K+V(+scale)
bytes over time, as a share of the 8.0 TB/s HBM3E peak.  The append launch
is timed against the two ``index_copy_`` calls of the bf16 cache at S = 1.

End to end: Llama-8B GraphedLlamaDecoder, attn_impl="hip", bf16 cache
against fp8 cache, both alive in one process, three alternating repeats;
time to first token and resident cache bytes of both arms.

    python scripts/kbench_decode_attn_fp8.py [--op-only | --e2e-only]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from kbench_decode_attn import HBM_PEAK, ROTATE_BYTES, time_pair

dev = torch.device("cuda")
POINTS = [(B, Hq, Hkv, Smax, lens)
          for (B, Hq, Hkv) in [(1, 32, 8), (8, 32, 8), (16, 16, 16)]
          for Smax, lens in [(2048, (128, 1024, 2047)),
                             (8192, (128, 4096, 8191))]]
POINTS.append((8, 32, 8, 32768, (16384, 32767)))
D = 128


def _spread(v):
    return (max(v) - min(v)) / min(v)


@torch.no_grad()
def op_level():
    assert ops.extension_available(), "HIP extension must be built"
    print("## op level: (A) bf16 decode_attention, (B) fp8; us = median of "
          "3 repeat medians")
    print(f"{'B':>2s} {'Hq':>3s} {'Hkv':>3s} {'Smax':>5s} {'len':>5s} "
          f"{'(A) us':>8s} {'GB/s':>6s} {'%HBM':>5s} {'(B) us':>8s} "
          f"{'GB/s':>6s} {'%HBM':>5s} {'A/B':>5s} {'spread%':>7s} "
          f"{'maxdiff':>8s} bar")
    misses = []
    for (B, Hq, Hkv, Smax, lens) in POINTS:
        kv_bytes = 2 * B * Hkv * Smax * D * 2
        ncopy = max(2, min(64, -(-ROTATE_BYTES // (kv_bytes // 2))))
        g = torch.Generator(device="cuda").manual_seed(0)
        ks, vs, kq, vq = [], [], [], []
        for _ in range(ncopy):
            k = torch.randn(B, Hkv, Smax, D, device=dev, generator=g,
                            dtype=torch.bfloat16)
            v = torch.randn(B, Hkv, Smax, D, device=dev, generator=g,
                            dtype=torch.bfloat16)
            kc, vc = (ops.Fp8KV.zeros(B, Hkv, Smax, D, device=dev)
                      for _ in range(2))
            ops.kv_cache_append(kc, vc, k, v, 0)
            ks.append(k), vs.append(v), kq.append(kc), vq.append(vc)
        q = torch.randn(B, Hq, 1, D, device=dev, generator=g,
                        dtype=torch.bfloat16)
        for length in lens:
            pos_t = torch.tensor([length - 1], device=dev)

            def fa(i):
                return ops.decode_attention(q, ks[i % ncopy], vs[i % ncopy],
                                            pos_t)

            def fb(i):
                return ops.decode_attention(q, kq[i % ncopy], vq[i % ncopy],
                                            pos_t)

            diff = (fa(0).float() - fb(0).float()).abs().max().item()
            ta, tb = [], []
            for _ in range(3):
                a, b = time_pair(fa, fb)
                ta.append(a), tb.append(b)
            ma, mb = statistics.median(ta), statistics.median(tb)
            spread = max(_spread(ta), _spread(tb))
            ra = 2 * B * Hkv * length * D * 2 / (ma * 1e-6)
            rb = 2 * B * Hkv * length * (D + 4) / (mb * 1e-6)
            barred = B >= 8 and length >= 1024
            ok = mb * (1 + spread) < ma
            if barred and not ok:
                misses.append((B, Hq, Hkv, Smax, length))
            print(f"{B:2d} {Hq:3d} {Hkv:3d} {Smax:5d} {length:5d} "
                  f"{ma:8.1f} {ra / 1e9:6.0f} {100 * ra / HBM_PEAK:5.1f} "
                  f"{mb:8.1f} {rb / 1e9:6.0f} {100 * rb / HBM_PEAK:5.1f} "
                  f"{ma / mb:5.2f} {100 * spread:7.1f} {diff:8.4f} "
                  f"{('ok' if ok else 'MISS') if barred else '-'}",
                  flush=True)
        del ks, vs, kq, vq
        torch.cuda.empty_cache()
    print("bar (a), fp8 faster than bf16 beyond the repeat spread at B >= 8, "
          "length >= 1024: " + ("MET" if not misses else f"MISSED at {misses}"),
          flush=True)

    print("## append at S = 1: (A) two index_copy_ into bf16 caches, "
          "(B) one kv_cache_append launch into fp8 caches, us")
    for (B, Hkv, Smax) in [(1, 8, 8192), (8, 8, 8192), (16, 16, 8192)]:
        kc, vc = (torch.zeros(B, Hkv, Smax, D, device=dev,
                              dtype=torch.bfloat16) for _ in range(2))
        kf, vf = (ops.Fp8KV.zeros(B, Hkv, Smax, D, device=dev)
                  for _ in range(2))
        k, v = (torch.randn(B, Hkv, 1, D, device=dev, dtype=torch.bfloat16)
                for _ in range(2))
        pos_t = torch.tensor([4095], device=dev)

        def fa(i):
            kc.index_copy_(2, pos_t, k)
            vc.index_copy_(2, pos_t, v)

        def fb(i):
            ops.kv_cache_append(kf, vf, k, v, pos_t)

        ta, tb = time_pair(fa, fb)
        print(f"B={B} Hkv={Hkv}: (A) {ta:.1f} (B) {tb:.1f}", flush=True)


@torch.no_grad()
def end_to_end(m=None):
    from torchdistpackage_amd.inference.generate import GraphedLlamaDecoder
    from torchdistpackage_amd.models.llama import LlamaModel, llama3_8b
    print("## end to end: Llama-8B GraphedLlamaDecoder attn_impl=hip, "
          "ms/token (3 alternating repeats per cache format)")
    if m is None:
        torch.manual_seed(0)
        cfg = llama3_8b()
        cfg.max_seq = max(cfg.max_seq, 16384)
        m = LlamaModel(cfg, device=dev, dtype=torch.bfloat16).eval()
    misses = []
    for max_seq, prompt, B, steps in ((4096, 2048, 1, 32), (4096, 2048, 8, 32),
                                      (16384, 8192, 8, 32)):
        if max_seq > m.cfg.max_seq:
            print(f"max_seq={max_seq}: beyond the model's max_seq "
                  f"{m.cfg.max_seq}, skipped")
            continue
        prev = ops.set_prefill_attention(prompt > 2048)
        idx = torch.randint(0, 128256, (B, prompt), device=dev)
        decs, ttft, resident = {}, {}, {}
        for kvd in ("bf16", "fp8"):
            d = GraphedLlamaDecoder(m, batch=B, max_seq=max_seq,
                                    attn_impl="hip", kv_dtype=kvd)
            d.prefill(idx)                       # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.prefill(idx)
            torch.cuda.synchronize()
            ttft[kvd] = (time.perf_counter() - t0) * 1e3
            for _ in range(4):
                d.step()
            resident[kvd] = sum(
                c.nbytes() if isinstance(c, ops.Fp8KV)
                else c.numel() * c.element_size()
                for pair in d.caches for c in pair)
            decs[kvd] = d
        ops.set_prefill_attention(prev)
        times = {"bf16": [], "fp8": []}
        for _ in range(3):
            for kvd in ("bf16", "fp8"):
                d = decs[kvd]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    d.step()
                torch.cuda.synchronize()
                times[kvd].append((time.perf_counter() - t0) / steps * 1e3)
        del decs, d
        torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(_spread(v) for v in times.values())
        ok = med["fp8"] * (1 + spread) < med["bf16"]
        if B >= 8 and not ok:
            misses.append((max_seq, prompt, B))
        print(f"max_seq={max_seq} prompt={prompt} B={B}: "
              f"bf16 {[f'{t:.3f}' for t in times['bf16']]} "
              f"fp8 {[f'{t:.3f}' for t in times['fp8']]} "
              f"median bf16 {med['bf16']:.3f} fp8 {med['fp8']:.3f} "
              f"(fp8/bf16 {med['fp8'] / med['bf16']:.3f}, spread "
              f"{100 * spread:.1f}%); ttft ms bf16 {ttft['bf16']:.1f} fp8 "
              f"{ttft['fp8']:.1f}; cache MB bf16 {resident['bf16'] / 2**20:.0f}"
              f" fp8 {resident['fp8'] / 2**20:.0f}", flush=True)
    print("bar (b), ms/token lower with fp8 beyond the repeat spread at "
          "B = 8: " + ("MET" if not misses else f"MISSED at {misses}"),
          flush=True)


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
    print("KBENCH DECODE ATTN FP8 OK")
