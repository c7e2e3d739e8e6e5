"""Grouped expert GEMM A/B at the moe_8x shapes (dim 1024, hidden 4096, 8
experts, top-2 of 16 x 1024 tokens = 32768 routed rows).

FFN level: forward + backward of ONE MoE layer's expert FFN over a token
buffer already sorted by expert,
  (a) the default path of moe/layer.py: per-expert loop, each segment
      zero-padded to a multiple of 1024 rows (torch.zeros + torch.cat), two
      linear + one bias_gelu per expert, output sliced and joined with
      torch.cat — fills, copies and launches included,
  (b) GroupedExperts: grouped_linear -> bias_gelu -> grouped_linear on the
      buffer in place,
under a balanced routing and a skewed one in which one expert gets half the
rows.  Both paths live in the same process and alternate call by call;
device events, median of ITERS calls after warm-up.  Inputs rotate through
copies that together exceed the 256 MB Infinity Cache (one call's working
set already does).

GEMM level (balanced routing): each grouped entry point against the loop of
per-expert torch.mm calls it replaces, in TFLOP/s.

    python scripts/kbench_grouped_gemm.py [--iters N]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.moe.layer import Expert, GroupedExperts

DIM, MULT, E = 1024, 4, 8
ROWS = 16 * 1024 * 2           # batch 16 x seq 1024 x top-2
NCOPY = 4                      # 4 x (x + dy) x 64 MB = 512 MB > 256 MB
Q = 1024                       # the loop path's row quantum

dev = torch.device("cuda")
BF16 = torch.bfloat16


def time_pair(fa, fb, iters, warm=3):
    """Median device time (ms) of fa and fb, alternating call by call."""
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
    ta = statistics.median(e[0].elapsed_time(e[1]) for e in ev)
    tb = statistics.median(e[2].elapsed_time(e[3]) for e in ev)
    return ta, tb


def loop_ffn(experts, grouped, per_expert):
    """The batched=False branch of ExpertParallelMoE.forward, verbatim."""
    y_parts = []
    off = 0
    for le in range(len(experts)):
        n = per_expert[le]
        if n > 0:
            seg = grouped[off:off + n]
            npad = (n + Q - 1) // Q * Q
            if npad != n:
                pad = torch.zeros(npad - n, seg.shape[1], dtype=seg.dtype,
                                  device=seg.device)
                seg = torch.cat([seg, pad], dim=0)
            y_parts.append(experts[le](seg)[:n])
        off += n
    return torch.cat(y_parts, dim=0) if y_parts else grouped[:0]


def routings():
    bal = [ROWS // E] * E
    rest = ROWS // 2
    skew = [ROWS // 2] + [rest // (E - 1)] * (E - 1)
    skew[-1] += rest - sum(skew[1:])
    assert sum(bal) == sum(skew) == ROWS
    return [("balanced", bal), ("skewed", skew)]


def ffn_level(iters):
    torch.manual_seed(0)
    experts = torch.nn.ModuleList(
        [Expert(DIM, MULT, device=dev, dtype=BF16) for _ in range(E)])
    ge = GroupedExperts(E, DIM, MULT, device=dev, dtype=BF16)
    ge.load_from_experts(experts)
    xs = [torch.randn(ROWS, DIM, device=dev, dtype=BF16) for _ in range(NCOPY)]
    dys = [torch.randn(ROWS, DIM, device=dev, dtype=BF16)
           for _ in range(NCOPY)]
    print(f"## FFN level: forward + backward, {ROWS} rows, dim {DIM}, "
          f"hidden {DIM * MULT}, {E} experts, median of {iters}")
    print(f"{'routing':>9s} {'rows per expert':>44s} {'(a) loop ms':>12s} "
          f"{'(b) grouped ms':>15s} {'a/b':>6s} {'(b) TF/s':>9s} "
          f"{'maxdiff':>8s}")
    flop = 3 * 2 * 2.0 * ROWS * DIM * DIM * MULT      # 2 GEMMs x (fwd+2 bwd)
    for name, counts in routings():
        offs = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)),
                            device=dev)

        def fa(i):
            for p in experts.parameters():
                p.grad = None
            x = xs[i % NCOPY].requires_grad_(True)
            x.grad = None
            loop_ffn(experts, x, counts).backward(dys[i % NCOPY])

        def fb(i):
            for p in ge.parameters():
                p.grad = None
            x = xs[i % NCOPY].requires_grad_(True)
            x.grad = None
            ge(x, offs).backward(dys[i % NCOPY])

        with torch.no_grad():
            diff = (loop_ffn(experts, xs[0], counts).float()
                    - ge(xs[0], offs).float()).abs().max().item()
        ta, tb = time_pair(fa, fb, iters)
        print(f"{name:>9s} {str(counts):>44s} {ta:12.3f} {tb:15.3f} "
              f"{ta / tb:6.2f} {flop / (tb * 1e-3) / 1e12:9.0f} {diff:8.4f}",
              flush=True)


@torch.no_grad()
def gemm_level(iters):
    e = ops.ext("grouped_gemm")
    counts = [ROWS // E] * E
    o = [0]
    for c in counts:
        o.append(o[-1] + c)
    offs = torch.tensor(o, device=dev)
    print(f"## GEMM level, balanced routing ({counts[0]} rows per expert): "
          "grouped kernel vs the per-expert torch.mm loop, TFLOP/s")
    print(f"{'gemm':>6s} {'Dout':>5s} {'Din':>5s} {'loop ms':>9s} "
          f"{'grouped ms':>11s} {'loop TF/s':>10s} {'grouped TF/s':>13s}")
    for Dout, Din in ((DIM * MULT, DIM), (DIM, DIM * MULT)):
        w = torch.randn(E, Dout, Din, device=dev, dtype=BF16) * 0.02
        b = torch.randn(E, Dout, device=dev, dtype=BF16)
        xs = [torch.randn(ROWS, Din, device=dev, dtype=BF16)
              for _ in range(NCOPY)]
        dys = [torch.randn(ROWS, Dout, device=dev, dtype=BF16)
               for _ in range(NCOPY)]
        y = torch.empty(ROWS, Dout, device=dev, dtype=BF16)
        dx = torch.empty(ROWS, Din, device=dev, dtype=BF16)
        dw = torch.empty(E, Dout, Din, device=dev, dtype=BF16)
        segs = [slice(o[i], o[i + 1]) for i in range(E)]
        pairs = {
            "fprop": (
                lambda i: [torch.addmm(b[k], xs[i % NCOPY][s], w[k].t(),
                                       out=y[s]) for k, s in enumerate(segs)],
                lambda i: e.grouped_gemm_fprop(xs[i % NCOPY], w, offs, b)),
            "dgrad": (
                lambda i: [torch.mm(dys[i % NCOPY][s], w[k], out=dx[s])
                           for k, s in enumerate(segs)],
                lambda i: e.grouped_gemm_dgrad(dys[i % NCOPY], w, offs)),
            "wgrad": (
                lambda i: [torch.mm(dys[i % NCOPY][s].t(), xs[i % NCOPY][s],
                                    out=dw[k]) for k, s in enumerate(segs)],
                lambda i: e.grouped_gemm_wgrad(dys[i % NCOPY], xs[i % NCOPY],
                                               offs, False)),
        }
        flop = 2.0 * ROWS * Dout * Din
        for kind, (fa, fb) in pairs.items():
            ta, tb = time_pair(fa, fb, iters)
            print(f"{kind:>6s} {Dout:5d} {Din:5d} {ta:9.3f} {tb:11.3f} "
                  f"{flop / (ta * 1e-3) / 1e12:10.0f} "
                  f"{flop / (tb * 1e-3) / 1e12:13.0f}", flush=True)
        del xs, dys, y, dx, dw, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.extension_available(), "HIP extension must be built"
    assert ops.grouped_gemm_eligible(DIM * MULT, DIM, BF16)
    ffn_level(args.iters)
    gemm_level(args.iters)
    print("KBENCH GROUPED GEMM OK")
