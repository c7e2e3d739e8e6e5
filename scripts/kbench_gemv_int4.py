"""Int4 weight-only small-M linear A/B: (A) what bf16 ``linear()`` picks for
the shape and M (the bf16 GEMV kernel or hipBLASLt), (B8) the W8A16 kernel
(csrc/gemv_int8.hip), (B4) the W4A16 kernel (csrc/gemv_int4.hip) as
dispatched, on the same weight.

The method is that of scripts/kbench_gemv_int8.py: the three arms run in one
process, alternating call by call, timed with device events; a figure is the
median of ITERS calls and every (shape, M) is measured REPEATS times, which
gives the repeat spread (max-min)/min.  Each arm rotates its weights through
more than 512 MB of copies.  GB/s counts the (B4) weight bytes,
N K / 2 + 4 N K / 128.

At M <= 4, where both arms of the int4 kernel exist, two more columns time
the MFMA arm and the dot2 arm forced through the binding (``arm=1`` / ``2``);
the crossover constant GEMV4_DOT2_MAX_M in csrc/gemv_int4.hip is set from
them.

Bar (a): at the two large Llama-8B shapes (w1/w3, w2) and every M, (B4) is
faster than (B8) and than (A), each by more than the larger repeat spread of
the two arms compared.  All other points are reported, not barred.

    python scripts/kbench_gemv_int4.py [--iters 200] [--repeats 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.ops.gemm import decode_route, linear
from torchdistpackage_amd.ops.int4 import int4_linear, quantize_int4
from torchdistpackage_amd.ops.int8 import int8_linear, quantize_int8

ROTATE_BYTES = 512 << 20
WARM = 20
SHAPES = [                      # (model, name, N, K)
    ("gpt2-1.3b", "qkv", 6144, 2048), ("gpt2-1.3b", "proj", 2048, 2048),
    ("gpt2-1.3b", "fc1", 8192, 2048), ("gpt2-1.3b", "fc2", 2048, 8192),
    ("llama-8b", "wq/wo", 4096, 4096), ("llama-8b", "wk/wv", 1024, 4096),
    ("llama-8b", "w1/w3", 14336, 4096), ("llama-8b", "w2", 4096, 14336),
]
BARRED = ("w1/w3", "w2")
MS = [1, 2, 4, 8, 16, 32]

dev = torch.device("cuda")


def time_arms(fns, iters, warm=WARM):
    """Median device time (us) of each fn, alternating call by call."""
    for i in range(warm):
        for f in fns:
            f(i)
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True),
            torch.cuda.Event(enable_timing=True)) for _ in fns]
          for _ in range(iters)]
    for i in range(iters):
        for f, (e0, e1) in zip(fns, ev[i]):
            e0.record()
            f(i)
            e1.record()
    torch.cuda.synchronize()
    return [statistics.median(ev[i][a][0].elapsed_time(ev[i][a][1])
                              for i in range(iters)) * 1e3
            for a in range(len(fns))]


def _spread(v):
    return (max(v) - min(v)) / min(v)


@torch.no_grad()
def main(iters, repeats):
    assert ops.extension_available(), "HIP extension must be built"
    print("## (A) bf16 linear() as dispatched, (B8) gemv_w8a16, (B4) "
          f"gemv_w4a16; median of {iters}, {repeats} repeats, weights "
          f"rotated through > {ROTATE_BYTES >> 20} MB")
    print(f"{'model':>9s} {'proj':>6s} {'N':>6s} {'K':>6s} {'M':>3s} "
          f"{'(A) is':>9s} {'(A) us':>8s} {'(B8) us':>8s} {'(B4) us':>8s} "
          f"{'B4 GB/s':>7s} {'B4/A':>6s} {'B4/B8':>6s} {'sprA':>6s} "
          f"{'sprB8':>6s} {'sprB4':>6s} {'maxdiff':>8s} {'mfma us':>8s} "
          f"{'dot2 us':>8s}")
    kern = ops.ext("kbench").gemv_w4a16
    misses = []
    for model, name, N, K in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        w0 = torch.randn(N, K, device=dev, generator=g) * 0.02
        q8, s8 = quantize_int8(w0)
        q4, s4 = quantize_int4(w0)
        b4 = q4.numel() + 4 * s4.numel()
        wa = [w0.to(torch.bfloat16).clone()
              for _ in range(-(-ROTATE_BYTES // (2 * N * K)) + 1)]
        w8 = [q8.clone() for _ in range(-(-ROTATE_BYTES // (N * K)) + 1)]
        w4 = [(q4.clone(), s4.clone())
              for _ in range(-(-ROTATE_BYTES // b4) + 1)]
        for M in MS:
            x = torch.randn(M, K, device=dev, generator=g,
                            dtype=torch.bfloat16)
            fns = [lambda i: linear(x, wa[i % len(wa)]),
                   lambda i: int8_linear(x, w8[i % len(w8)], s8),
                   lambda i: int4_linear(x, *w4[i % len(w4)])]
            if M <= 4:
                fns += [lambda i: kern(x, *w4[i % len(w4)], None, 1),
                        lambda i: kern(x, *w4[i % len(w4)], None, 2)]
            diff = (fns[0](0).float() - fns[2](0).float()).abs().max().item()
            runs = [time_arms(fns, iters) for _ in range(repeats)]
            ts = [[r[a] for r in runs] for a in range(len(fns))]
            ta, t8, t4 = (statistics.median(v) for v in ts[:3])
            sa, sp8, sp4 = (_spread(v) for v in ts[:3])
            arms = "".join(f" {statistics.median(v):8.1f}" for v in ts[3:])
            print(f"{model:>9s} {name:>6s} {N:6d} {K:6d} {M:3d} "
                  f"{decode_route(M, N, K):>9s} {ta:8.1f} {t8:8.1f} "
                  f"{t4:8.1f} {b4 / t4 / 1e3:7.0f} {t4 / ta:6.3f} "
                  f"{t4 / t8:6.3f} {100 * sa:5.1f}% {100 * sp8:5.1f}% "
                  f"{100 * sp4:5.1f}% {diff:8.4f}{arms}", flush=True)
            if name in BARRED and not (
                    t4 < ta * (1 - max(sa, sp4))
                    and t4 < t8 * (1 - max(sp8, sp4))):
                misses.append((name, M))
        del wa, w8, w4
        torch.cuda.empty_cache()
    print("bar (a) ((B4) faster than (B8) and than (A) beyond the repeat "
          "spread at w1/w3 and w2, every M): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(args.iters, args.repeats)
    print("KBENCH GEMV INT4 OK")
