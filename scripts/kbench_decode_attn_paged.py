"""Paged KV cache A/B: decode attention through a block table (ops.PagedKV,
csrc/decode_attn_paged.hip) against the contiguous bf16 kernel
(csrc/decode_attn.hip).

Op level: (A) contiguous, (B16) / (B64) paged under a randomly permuted table
at page 16 / 64, (B16i) page 16 under the identity table; all four timed in
one process, alternating call by call, with device events (median of ITERS
calls after warm-up), three repeats per point, spread = (max-min)/min of the
medians.  The caches rotate through more than 512 MB per arm.  Every arm
reads the same K and V values (the paged result is checked bit-equal to
(A)'s wherever the two pick the same chunk length).  One paged append at
S = 1 is timed against the two ``index_copy_`` calls of the dense cache.

End to end: Llama-8B GraphedLlamaDecoder, attn_impl="hip", contiguous against
paged (page 16, permuted table), both alive in one process, three alternating
repeats, ms/token.

    python scripts/kbench_decode_attn_paged.py [--op-only | --e2e-only]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from kbench_decode_attn import HBM_PEAK, ITERS, ROTATE_BYTES, WARM

dev = torch.device("cuda")
POINTS = [(B, Hq, Hkv, Smax, lens)
          for (B, Hq, Hkv) in [(1, 32, 8), (8, 32, 8), (16, 16, 16)]
          for Smax, lens in [(2048, (128, 1024, 2047)),
                             (8192, (128, 4096, 8191))]]
POINTS.append((8, 32, 8, 32768, (16384, 32767)))
D = 128
ARMS = ("A", "B16", "B64", "B16i")


def _spread(v):
    return (max(v) - min(v)) / min(v)


def time_arms(fns, iters=ITERS, warm=WARM):
    """Median device time (us) of each function, alternating call by call."""
    for i in range(warm):
        for f in fns:
            f(i)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(fns))]
          for _ in range(iters)]
    for i in range(iters):
        for a, f in enumerate(fns):
            ev[i][2 * a].record()
            f(i)
            ev[i][2 * a + 1].record()
    torch.cuda.synchronize()
    return [statistics.median(e[2 * a].elapsed_time(e[2 * a + 1])
                              for e in ev) * 1e3 for a in range(len(fns))]


def _paged(k, v, page, permute, g):
    B, Hkv, Smax, _ = k.shape
    nb = Smax // page
    ids = torch.randperm(B * nb, generator=g, device=dev) if permute \
        else torch.arange(B * nb, device=dev)
    table = ids.to(torch.int32).view(B, nb)
    kp = ops.PagedKV.zeros(B, Hkv, Smax, D, page, device=dev,
                           block_table=table)
    vp = ops.PagedKV(torch.zeros_like(kp.pool), table)
    ops.kv_cache_append(kp, vp, k, v, 0)
    return kp, vp


@torch.no_grad()
def op_level():
    assert ops.extension_available(), "HIP extension must be built"
    print("## op level: (A) contiguous decode_attention, (B16)/(B64) paged, "
          "permuted table, (B16i) page 16, identity table; us = median of 3 "
          "repeat medians; %HBM of (A) and (B64)")
    print(f"{'B':>2s} {'Hq':>3s} {'Hkv':>3s} {'Smax':>5s} {'len':>5s} "
          f"{'(A) us':>8s} {'%HBM':>5s} {'(B64) us':>8s} {'%HBM':>5s} "
          f"{'B64/A':>6s} {'(B16) us':>8s} {'B16/A':>6s} {'(B16i)us':>8s} "
          f"{'B16i/A':>6s} {'spread%':>7s} {'equal':>5s} bar")
    misses = []
    for (B, Hq, Hkv, Smax, lens) in POINTS:
        kv_bytes = 2 * B * Hkv * Smax * D * 2
        ncopy = max(2, min(64, -(-ROTATE_BYTES // kv_bytes)))
        g = torch.Generator(device="cuda").manual_seed(0)
        caches = {a: [] for a in ARMS}
        for _ in range(ncopy):
            k = torch.randn(B, Hkv, Smax, D, device=dev, generator=g,
                            dtype=torch.bfloat16)
            v = torch.randn(B, Hkv, Smax, D, device=dev, generator=g,
                            dtype=torch.bfloat16)
            caches["A"].append((k, v))
            caches["B16"].append(_paged(k, v, 16, True, g))
            caches["B64"].append(_paged(k, v, 64, True, g))
            caches["B16i"].append(_paged(k, v, 16, False, g))
        q = torch.randn(B, Hq, 1, D, device=dev, generator=g,
                        dtype=torch.bfloat16)
        for length in lens:
            pos_t = torch.tensor([length - 1], device=dev)

            def arm(a):
                def f(i):
                    kc, vc = caches[a][i % ncopy]
                    return ops.decode_attention(q, kc, vc, pos_t)
                return f

            fns = [arm(a) for a in ARMS]
            equal = all(torch.equal(fns[0](0), f(0)) for f in fns[1:])
            reps = [time_arms(fns) for _ in range(3)]
            t = {a: [r[i] for r in reps] for i, a in enumerate(ARMS)}
            med = {a: statistics.median(t[a]) for a in ARMS}
            spread = max(_spread(t["A"]), _spread(t["B64"]))
            rate = {a: 2 * B * Hkv * length * D * 2 / (med[a] * 1e-6)
                    for a in ARMS}
            barred = B >= 8 and length >= 1024
            ok = med["B64"] <= med["A"] * (1 + spread)
            if barred and not ok:
                misses.append((B, Hq, Hkv, Smax, length))
            print(f"{B:2d} {Hq:3d} {Hkv:3d} {Smax:5d} {length:5d} "
                  f"{med['A']:8.1f} {100 * rate['A'] / HBM_PEAK:5.1f} "
                  f"{med['B64']:8.1f} {100 * rate['B64'] / HBM_PEAK:5.1f} "
                  f"{med['B64'] / med['A']:6.3f} {med['B16']:8.1f} "
                  f"{med['B16'] / med['A']:6.3f} {med['B16i']:8.1f} "
                  f"{med['B16i'] / med['A']:6.3f} {100 * spread:7.1f} "
                  f"{str(equal):>5s} "
                  f"{('ok' if ok else 'MISS') if barred else '-'}",
                  flush=True)
        del caches
        torch.cuda.empty_cache()
    print("bar (a), (B64) not slower than (A) beyond the larger repeat "
          "spread at B >= 8, length >= 1024: "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)

    print("## append at S = 1: (A) two index_copy_ into dense caches, "
          "(B) one kv_cache_append launch into paged caches (page 16, "
          "permuted table), us = median of 3 repeat medians")
    g = torch.Generator(device="cuda").manual_seed(1)
    for (B, Hkv, Smax) in [(1, 8, 8192), (8, 8, 8192), (16, 16, 8192)]:
        kc, vc = (torch.zeros(B, Hkv, Smax, D, device=dev,
                              dtype=torch.bfloat16) for _ in range(2))
        kp, vp = _paged(kc, vc, 16, True, g)
        k, v = (torch.randn(B, Hkv, 1, D, device=dev, dtype=torch.bfloat16)
                for _ in range(2))
        pos_t = torch.tensor([4095], device=dev)

        def fa(i):
            kc.index_copy_(2, pos_t, k)
            vc.index_copy_(2, pos_t, v)

        def fb(i):
            ops.kv_cache_append(kp, vp, k, v, pos_t)

        reps = [time_arms([fa, fb]) for _ in range(3)]
        ta, tb = ([r[i] for r in reps] for i in range(2))
        print(f"B={B} Hkv={Hkv}: (A) {statistics.median(ta):.1f} "
              f"(B) {statistics.median(tb):.1f} (spread "
              f"{100 * max(_spread(ta), _spread(tb)):.1f}%)", flush=True)


@torch.no_grad()
def end_to_end(m=None):
    from torchdistpackage_amd.inference.generate import GraphedLlamaDecoder
    from torchdistpackage_amd.models.llama import LlamaModel, llama3_8b
    print("## end to end: Llama-8B GraphedLlamaDecoder attn_impl=hip, "
          "ms/token (3 alternating repeats per cache layout; paged = page "
          "16, permuted table)")
    if m is None:
        torch.manual_seed(0)
        m = LlamaModel(llama3_8b(), device=dev, dtype=torch.bfloat16).eval()
    misses = []
    g = torch.Generator(device="cuda").manual_seed(2)
    for max_seq, prompt, B, steps in ((4096, 2048, 1, 32),
                                      (4096, 2048, 8, 32)):
        idx = torch.randint(0, 128256, (B, prompt), device=dev)
        decs = {}
        for layout in ("contiguous", "paged"):
            d = GraphedLlamaDecoder(m, batch=B, max_seq=max_seq,
                                    attn_impl="hip", kv_layout=layout,
                                    page_size=16)
            if layout == "paged":
                table = d.caches[0][0].block_table
                table.copy_(torch.randperm(table.numel(), generator=g,
                                           device=dev).view_as(table))
            d.prefill(idx)
            for _ in range(4):
                d.step()
            decs[layout] = d
        times = {k: [] for k in decs}
        for _ in range(3):
            for layout, d in decs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    d.step()
                torch.cuda.synchronize()
                times[layout].append((time.perf_counter() - t0) / steps * 1e3)
        del decs, d
        torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(_spread(v) for v in times.values())
        ok = med["paged"] <= med["contiguous"] * (1 + spread)
        if not ok:
            misses.append((max_seq, prompt, B))
        print(f"max_seq={max_seq} prompt={prompt} B={B}: contiguous "
              f"{[f'{t:.3f}' for t in times['contiguous']]} paged "
              f"{[f'{t:.3f}' for t in times['paged']]} median contiguous "
              f"{med['contiguous']:.3f} paged {med['paged']:.3f} "
              f"(paged/contiguous {med['paged'] / med['contiguous']:.3f}, "
              f"spread {100 * spread:.1f}%)", flush=True)
    print("bar (b), paged ms/token not higher than contiguous beyond the "
          "repeat spread: " + ("MET" if not misses else f"MISSED at {misses}"),
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
    print("KBENCH DECODE ATTN PAGED OK")
