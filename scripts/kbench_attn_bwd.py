"""Head-dim-128 attention backward A/B: the fused dk/dv kernel (default)
against the two-pass dv + dk kernels (knob ``split_dkdv``).

Both versions run in one process, alternating call by call, timed with
device events (median of ITERS calls after warm-up):

  dk/dv stage   ext.attn_bwd_dkdv: the fused kernel alone against the SUM of
                the two passes (both store the dS workspace)
  attn_bwd      the whole backward: delta, dk/dv stage, dq-lite

and, where the profiler is available, the per-kernel device times of one
profiled pass of each version.

    python scripts/kbench_attn_bwd.py [--recompute]
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops

ITERS, WARM = 30, 5
SHAPES = [(16, 16, 1024, 128), (16, 16, 2048, 128)]     # (B, H, S, D)

dev = torch.device("cuda")


def time_pair(fa, fb, iters=ITERS, warm=WARM):
    """Median device time (us) of fa and fb, alternating call by call."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)]
          for _ in range(iters)]
    for i in range(iters):
        ev[i][0].record()
        fa()
        ev[i][1].record()
        ev[i][2].record()
        fb()
        ev[i][3].record()
    torch.cuda.synchronize()
    ta = [e[0].elapsed_time(e[1]) * 1e3 for e in ev]
    tb = [e[2].elapsed_time(e[3]) * 1e3 for e in ev]
    return statistics.median(ta), statistics.median(tb), \
        max(ta) - min(ta), max(tb) - min(tb)


def kernel_table(fn, label):
    """Per-kernel device time of one call of fn (us), if the profiler works."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.count, getattr(e, "device_time_total", None)
                 or getattr(e, "cuda_time_total", 0.0))
                for e in prof.key_averages()]
        rows = [r for r in rows if r[2] > 0]
        print(f"  kernels, {label}:")
        for key, n, t in sorted(rows, key=lambda r: -r[2]):
            print(f"    {t:9.1f} us  x{n}  {key[:100]}")
    except Exception as e:                      # noqa: BLE001
        print(f"  kernels, {label}: profiler unavailable ({e!r})")


@torch.no_grad()
def main(recompute):
    assert ops.extension_available(), "HIP extension must be built"
    e = ops.ext("kbench_attn_bwd")
    base = {"dq_recompute": True} if recompute else {}
    for (B, H, S, D) in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        q, k, v, do = (torch.randn(B, H, S, D, device=dev, generator=g,
                                   dtype=torch.bfloat16) for _ in range(4))
        scale = 1.0 / math.sqrt(D)
        o, lse = e.attn_fwd(q, k, v, torch.empty_like(q), True, scale)
        delta = e.attn_delta(o, do)
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))

        def stage(split):
            def f():
                with ops.attention_route(split_dkdv=split, **base):
                    e.attn_bwd_dkdv(do, q, k, v, lse, delta, dk, dv, True,
                                    scale)
            return f

        def whole(split):
            def f():
                with ops.attention_route(split_dkdv=split, **base):
                    e.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, True, scale)
            return f

        with ops.attention_route(split_dkdv=False, **base):
            r_f = e.attn_bwd_route(B, H, S, D)
        with ops.attention_route(split_dkdv=True, **base):
            r_s = e.attn_bwd_route(B, H, S, D)
        # same bits both ways before anything is timed
        whole(False)()
        ref = [t.clone() for t in (dq, dk, dv)]
        whole(True)()
        same = all(torch.equal(a, b) for a, b in zip(ref, (dq, dk, dv)))
        print(f"## B{B} H{H} S{S} D{D} causal: {r_f} vs {r_s}, "
              f"bit-equal: {same}")
        tf, ts, sf, ss = time_pair(stage(False), stage(True))
        print(f"  dk/dv stage: fused {tf:8.1f} us (spread {sf:.1f})   "
              f"two-pass sum {ts:8.1f} us (spread {ss:.1f})   "
              f"two-pass/fused {ts / tf:.3f}")
        tf, ts, sf, ss = time_pair(whole(False), whole(True))
        print(f"  attn_bwd   : fused {tf:8.1f} us (spread {sf:.1f})   "
              f"two-pass     {ts:8.1f} us (spread {ss:.1f})   "
              f"two-pass/fused {ts / tf:.3f}", flush=True)
        kernel_table(whole(False), "fused")
        kernel_table(whole(True), "two-pass")
        assert same, "fused and two-pass backward differ"
    print("KBENCH ATTN BWD OK")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--recompute", action="store_true",
                    help="the no-workspace route (no dS store, dq recomputed)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(args.recompute)
