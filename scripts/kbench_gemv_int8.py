"""Int8 weight-only GEMV A/B: (A) what bf16 ``linear()`` picks today for the
shape and M (the bf16 GEMV kernel or hipBLASLt), (B) the W8A16 kernel
(csrc/gemv_int8.hip) on the same weight quantised to int8.

Both arms run in the same process, alternating call by call, timed with
device events; a figure is the median of ITERS calls and every (shape, M)
is measured REPEATS times, which gives the repeat spread (max-min)/min.
Each arm rotates its weights through more than 512 MB of copies, so nothing
is served from the 256 MB Infinity Cache (the method of
scripts/kbench_decode_attn.py).  GB/s counts weight bytes only: 2 N K for
(A), N K + 4 N for (B).

Bar: at every shape with M <= 8, (B) is faster than (A) by more than the
repeat spread.  M = 16 and 32 are reported, not barred.

    python scripts/kbench_gemv_int8.py [--iters 200] [--repeats 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.ops.gemm import decode_route, linear
from torchdistpackage_amd.ops.int8 import int8_linear, quantize_int8

ROTATE_BYTES = 512 << 20
WARM = 20
SHAPES = [                      # (model, name, N, K)
    ("gpt2-1.3b", "qkv", 6144, 2048), ("gpt2-1.3b", "proj", 2048, 2048),
    ("gpt2-1.3b", "fc1", 8192, 2048), ("gpt2-1.3b", "fc2", 2048, 8192),
    ("llama-8b", "wq/wo", 4096, 4096), ("llama-8b", "wk/wv", 1024, 4096),
    ("llama-8b", "w1/w3", 14336, 4096), ("llama-8b", "w2", 4096, 14336),
]
MS = [1, 2, 4, 8, 16, 32]

dev = torch.device("cuda")


def time_pair(fa, fb, iters, warm=WARM):
    """Median device time (us) of fa and fb, alternating call by call."""
    for i in range(warm):
        fa(i)
        fb(i)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)]
          for _ in range(iters)]
    for i in range(iters):
        ev[i][0].record()
        fa(i)
        ev[i][1].record()
        ev[i][2].record()
        fb(i)
        ev[i][3].record()
    torch.cuda.synchronize()
    ta = statistics.median(e[0].elapsed_time(e[1]) for e in ev) * 1e3
    tb = statistics.median(e[2].elapsed_time(e[3]) for e in ev) * 1e3
    return ta, tb


@torch.no_grad()
def main(iters, repeats):
    assert ops.extension_available(), "HIP extension must be built"
    print("## (A) bf16 linear() as dispatched today, (B) gemv_w8a16; "
          f"median of {iters}, {repeats} repeats, weights rotated through "
          f"> {ROTATE_BYTES >> 20} MB")
    print(f"{'model':>9s} {'proj':>6s} {'N':>6s} {'K':>6s} {'M':>3s} "
          f"{'(A) is':>9s} {'(A) us':>8s} {'(B) us':>8s} {'A GB/s':>7s} "
          f"{'B GB/s':>7s} {'B/A':>6s} {'spread':>7s} {'maxdiff':>8s}")
    misses = []
    for model, name, N, K in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        na = -(-ROTATE_BYTES // (2 * N * K)) + 1
        nb = -(-ROTATE_BYTES // (N * K)) + 1
        w0 = torch.randn(N, K, device=dev, generator=g) * 0.02
        q0, s0 = quantize_int8(w0)
        wa = [w0.to(torch.bfloat16).clone() for _ in range(na)]
        qb = [q0.clone() for _ in range(nb)]
        for M in MS:
            x = torch.randn(M, K, device=dev, generator=g,
                            dtype=torch.bfloat16)

            def fa(i):
                return linear(x, wa[i % na])

            def fb(i):
                return int8_linear(x, qb[i % nb], s0)

            diff = (fa(0).float() - fb(0).float()).abs().max().item()
            runs = [time_pair(fa, fb, iters) for _ in range(repeats)]
            tas, tbs = [r[0] for r in runs], [r[1] for r in runs]
            ta, tb = statistics.median(tas), statistics.median(tbs)
            spread = max((max(v) - min(v)) / min(v) for v in (tas, tbs))
            what = decode_route(M, N, K)
            print(f"{model:>9s} {name:>6s} {N:6d} {K:6d} {M:3d} {what:>9s} "
                  f"{ta:8.1f} {tb:8.1f} {2 * N * K / ta / 1e3:7.0f} "
                  f"{(N * K + 4 * N) / tb / 1e3:7.0f} {tb / ta:6.3f} "
                  f"{100 * spread:6.1f}% {diff:8.4f}", flush=True)
            if M <= 8 and not tb < ta * (1 - spread):
                misses.append((name, N, K, M))
        del wa, qb
        torch.cuda.empty_cache()
    print("bar (a) (int8 kernel faster than (A) by more than the repeat "
          "spread at every shape with M <= 8): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(args.iters, args.repeats)
    print("KBENCH GEMV INT8 OK")
