"""MoE token routing A/B at the moe_8x shape (16 x 1024 tokens, top-2 of 8
experts, dim 1024): forward + backward of ONE layer's routing path with an
identity in place of the expert FFN,
  (T) the torch chain of moe/layer.py route="torch" at ep_size == 1: stable
      argsort, bincount, xt[token_of], the repeat_interleave / second argsort
      regroup with its two copies, gate gather, product and index_add_,
  (F) route="fused": ops.moe_route_plan, moe_dispatch, moe_combine,
both with the one counts.cpu() the layer keeps for its split lists, under a
balanced routing and a skewed one (half the entries on one expert).  Both arms
live in one process and alternate call by call; device events, median of
ITERS calls, REPEATS repeats; inputs rotate through copies that together
exceed 512 MB.  For (F) the essential traffic is one read of x, k writes, k
reads and one write per direction, reported against the 8 TB/s spec peak.
The plan alone is timed against argsort + bincount.

    python scripts/kbench_moe_route.py [--iters N]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from torchdistpackage_amd import ops

N, K, E, D = 16 * 1024, 2, 8, 1024
NCOPY = 9                      # 9 x (x + dy) x 32 MB = 576 MB > 512 MB
REPEATS = 3
PEAK = 8e12                    # HBM bytes/s, spec

dev = torch.device("cuda")
BF16 = torch.bfloat16


def time_pair(fa, fb, iters, warm=5):
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
    ta = statistics.median(e[0].elapsed_time(e[1]) for e in ev)
    tb = statistics.median(e[2].elapsed_time(e[3]) for e in ev)
    return ta * 1e3, tb * 1e3


def route_torch(xt, topk_idx, topk_gate):
    """ExpertParallelMoE.forward, route="torch", ep_size == 1, identity
    experts."""
    flat_expert = topk_idx.reshape(-1)
    order = torch.argsort(flat_expert, stable=True)
    token_of = order // K
    sorted_expert = flat_expert[order]                    # noqa: F841
    counts = torch.bincount(flat_expert, minlength=E)
    my_slice = counts.unsqueeze(0)[:, :E]
    my_slice_host = counts.cpu().unsqueeze(0)[:, :E]      # noqa: F841
    received = xt[token_of]
    seg_sizes_dev = my_slice.reshape(-1)
    seg_expert_dev = torch.arange(E, device=dev) % E
    tok_expert = torch.repeat_interleave(seg_expert_dev, seg_sizes_dev)
    order2 = torch.argsort(tok_expert, stable=True)
    grouped = received[order2]
    cnt_dev = my_slice.sum(0)
    offs = F.pad(torch.cumsum(cnt_dev, 0), (1, 0))        # noqa: F841
    y_all = grouped
    outs = torch.empty_like(received)
    outs[order2] = y_all
    gates = topk_gate.reshape(-1)[order].to(outs.dtype)
    combined = torch.zeros_like(xt)
    combined.index_add_(0, token_of, outs * gates.unsqueeze(-1))
    return combined


def route_fused(xt, topk_idx, topk_gate):
    dest, counts, offs = ops.moe_route_plan(topk_idx, E)
    counts.cpu()
    return ops.moe_combine(ops.moe_dispatch(xt, dest), dest, topk_gate)


def routings():
    g = torch.Generator().manual_seed(0)
    bal = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(N)])
    # skewed: slot 0 of every token on expert 0 (half the entries), slot 1
    # spread over the others
    skew = torch.stack([torch.zeros(N, dtype=torch.long),
                        torch.randint(1, E, (N,), generator=g)], 1)
    return [("balanced", bal.to(dev)), ("skewed", skew.to(dev))]


def main(iters):
    torch.manual_seed(0)
    xs = [torch.randn(N, D, device=dev, dtype=BF16).requires_grad_(True)
          for _ in range(NCOPY)]
    dys = [torch.randn(N, D, device=dev, dtype=BF16) for _ in range(NCOPY)]
    gate = torch.rand(N, K, device=dev).requires_grad_(True)
    traffic = 2 * (2 + 2 * K) * N * D * 2      # bytes, forward + backward
    print(f"## routing path, forward + backward: N={N} k={K} E={E} D={D}, "
          f"median of {iters}, {REPEATS} repeats, us")
    verdict = []
    for name, idx in routings():
        def arm(fn):
            def run(i):
                x = xs[i % NCOPY]
                x.grad = None
                gate.grad = None
                fn(x, idx, gate).backward(dys[i % NCOPY])
            return run

        outs = []
        for fn in (route_torch, route_fused):
            arm(fn)(0)
            outs.append((fn(xs[0], idx, gate).detach().float(),
                         xs[0].grad.float(), gate.grad.clone()))
        diffs = [(a - b).abs().max().item() for a, b in zip(*outs)]
        print(f"{name}: counts {torch.bincount(idx.flatten()).tolist()}, "
              f"max |T - F|: out {diffs[0]:.4f} dx {diffs[1]:.4f} "
              f"dgates {diffs[2]:.4f}")
        reps = [time_pair(arm(route_torch), arm(route_fused), iters)
                for _ in range(REPEATS)]
        ts, fs = [r[0] for r in reps], [r[1] for r in reps]
        spread = max(max(ts) - min(ts), max(fs) - min(fs))
        tm, fm = statistics.median(ts), statistics.median(fs)
        print(f"{name}: (T) {' '.join(f'{t:8.1f}' for t in ts)}  "
              f"(F) {' '.join(f'{t:8.1f}' for t in fs)}  spread {spread:.1f}  "
              f"T/F {tm / fm:.2f}  (F) {traffic / (fm * 1e-6) / 1e9:.0f} GB/s "
              f"= {100 * traffic / (fm * 1e-6) / PEAK:.0f}% of {PEAK / 1e12:.0f}"
              " TB/s", flush=True)
        verdict.append(tm - fm > spread)

        def plan_t(i):
            flat = idx.reshape(-1)
            order = torch.argsort(flat, stable=True)
            return order, torch.bincount(flat, minlength=E)

        reps = [time_pair(plan_t, lambda i: ops.moe_route_plan(idx, E), iters)
                for _ in range(REPEATS)]
        print(f"{name}: plan alone: argsort+bincount "
              f"{' '.join(f'{r[0]:7.1f}' for r in reps)}  moe_route_plan "
              f"{' '.join(f'{r[1]:7.1f}' for r in reps)}", flush=True)
    print("bar (a), (F) faster than (T) by more than the repeat spread at "
          f"both routings: {'met' if all(verdict) else 'MISSED'}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.extension_available(), "HIP extension must be built"
    assert ops.moe_route_eligible(D, BF16)
    main(args.iters)
    print("KBENCH MOE ROUTE OK")
