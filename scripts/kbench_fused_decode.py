"""Fused decode-step ops (csrc/fused_decode.hip) against their own
compositions at the Llama-8B decode shapes (dim 4096, ffn 14336, 32/8 heads,
head dim 128, Smax 4096), M = B in {1, 8}:

  swiglu_linear   (A) swiglu(linear(x, w1), linear(x, w3))      3 launches
                  (B) ops.swiglu_linear                         1 launch
                  plus linear(x, w1) alone: gemv_bf16's GB/s beside (B)'s
  rope_kv_append  (A) rope(q), rope(k), two index_copy_         4 launches
                  (B) ops.rope_kv_append, tensor pos0           1 launch
  add_rms_norm    (A) x + y, ops.rms_norm                       2 launches
                  (B) ops.add_rms_norm                          1 launch

Method of the other kbench scripts: one process, the arms alternate call by
call, device events, a figure is the median of ITERS calls, REPEATS repeats,
spread = (max - min) / min of an arm's medians, operands rotated through
more than 512 MB.  Bar (a): no (B) is slower than its (A) beyond the larger
repeat spread of the two.

    python scripts/kbench_fused_decode.py [--iters 200] [--repeats 3]

``end_to_end(model)`` (scripts/bench_decode_llama.py --fused-decode) is the
decode A/B: GraphedDecoder ms/token with the knob off against on, bf16 and
int4 weights, max_seq / prompt 4096 / 2048, B = 1 and 8, both decoders alive
in one process, three alternating repeats of 32 steps.  Bar (b): on is lower
than off by more than the larger repeat spread at all four points.

``--trace on|off`` runs one captured Llama-8B step between two marker
launches (``torch.cumsum``, which the step does not use) for a
``rocprofv3 --kernel-trace --stats`` run; ``--count DIR`` counts the
dispatches between the markers in the trace that run left under DIR.
"""
import argparse
import copy
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.ops.gemm import decode_route, linear

ROTATE_BYTES = 512 << 20
WARM = 20
DIM, FFN, H, HKV, HD, SMAX = 4096, 14336, 32, 8, 128, 4096
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


def _report(name, B, fns, iters, repeats, misses, extra=None):
    assert torch.equal(fns[0](0), fns[1](0)), name
    runs = [time_arms(fns, iters) for _ in range(repeats)]
    ts = [[r[a] for r in runs] for a in range(len(fns))]
    ta, tb = statistics.median(ts[0]), statistics.median(ts[1])
    sa, sb = _spread(ts[0]), _spread(ts[1])
    ok = tb <= ta * (1 + max(sa, sb))
    if not ok:
        misses.append((name, B))
    line = (f"{name:>15s} B={B}: (A) {ta:7.1f} us (spread {100 * sa:4.1f}%) "
            f"(B) {tb:7.1f} us (spread {100 * sb:4.1f}%) B/A {tb / ta:.3f} "
            f"{'ok' if ok else 'MISSED'}")
    if extra:
        line += extra(tb, [statistics.median(v) for v in ts[2:]])
    print(line, flush=True)


@torch.no_grad()
def main(iters, repeats):
    assert ops.extension_available(), "HIP extension must be built"
    print(f"## fused decode ops, (A) composition vs (B) fused; median of "
          f"{iters}, {repeats} repeats, operands rotated through > "
          f"{ROTATE_BYTES >> 20} MB")
    g = torch.Generator(device="cuda").manual_seed(0)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device=dev, generator=g) * scale) \
            .to(torch.bfloat16)

    misses = []
    nw = -(-ROTATE_BYTES // (4 * FFN * DIM)) + 1
    w1 = [rn(FFN, DIM, scale=0.02) for _ in range(nw)]
    w3 = [rn(FFN, DIM, scale=0.02) for _ in range(nw)]
    wbytes = 2 * FFN * DIM
    for B in (1, 8):
        x = rn(1, B, DIM)
        print(f"swiglu_linear B={B}: linear() routes w1 to "
              f"{decode_route(B, FFN, DIM)}")
        _report("swiglu_linear", B, [
            lambda i: ops.swiglu(linear(x, w1[i % nw]), linear(x, w3[i % nw])),
            lambda i: ops.swiglu_linear(x, w1[i % nw], w3[i % nw]),
            lambda i: linear(x, w1[i % nw])], iters, repeats, misses,
            extra=lambda tb, more: (
                f"; weight GB/s (B) {2 * wbytes / tb / 1e3:.0f}, "
                f"linear(x, w1) alone {wbytes / more[0] / 1e3:.0f} "
                f"({more[0]:.1f} us)"))
    del w1, w3
    torch.cuda.empty_cache()

    cos, sin = (torch.rand(SMAX, HD // 2, device=dev, generator=g)
                for _ in range(2))
    pos_t = torch.tensor([2048], device=dev)
    for B in (1, 8):
        nc = -(-ROTATE_BYTES // (4 * B * HKV * SMAX * HD)) + 1
        caches = [(torch.zeros(B, HKV, SMAX, HD, device=dev,
                               dtype=torch.bfloat16),
                   torch.zeros(B, HKV, SMAX, HD, device=dev,
                               dtype=torch.bfloat16)) for _ in range(nc)]

        def v4(heads):
            return rn(1, B, heads * HD).reshape(1, B, heads, HD) \
                .permute(1, 2, 0, 3)

        q, k, v = v4(H), v4(HKV), v4(HKV)

        def rope_a(i):
            kc, vc = caches[i % nc]
            qr = ops.rope_rotate_half(q, cos, sin, pos_t)
            kc.index_copy_(2, pos_t, ops.rope_rotate_half(k, cos, sin, pos_t))
            vc.index_copy_(2, pos_t, v)
            return qr

        def rope_b(i):
            kc, vc = caches[i % nc]
            return ops.rope_kv_append(q, k, v, cos, sin, kc, vc, pos_t)

        _report("rope_kv_append", B, [rope_a, rope_b], iters, repeats, misses)
        del caches
        torch.cuda.empty_cache()

    w = rn(DIM)
    for B in (1, 8):
        n = -(-ROTATE_BYTES // (4 * B * DIM)) + 1
        X, Y = rn(n, B, DIM), rn(n, B, DIM)
        _report("add_rms_norm", B, [
            lambda i: ops.rms_norm(X[i % n] + Y[i % n], w, 1e-5),
            lambda i: ops.add_rms_norm(X[i % n], Y[i % n], w, 1e-5)[1]],
            iters, repeats, misses)
        del X, Y
    print("bar (a) (no fused op slower than its composition beyond the "
          "larger repeat spread, every point): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)


def _decoder(m, B, max_seq, on, idx):
    from torchdistpackage_amd.inference.generate import GraphedDecoder
    prev = ops.set_fused_decode(on)
    try:
        d = GraphedDecoder(m, batch=B, max_seq=max_seq, attn_impl="hip")
        d.prefill(idx)
    finally:
        ops.set_fused_decode(prev)
    return d


@torch.no_grad()
def end_to_end(m, vocab=128256, max_seq=4096, prompt=2048, steps=32,
               repeats=3):
    models = {"bf16": m, "int4": copy.deepcopy(m)}
    ops.quantize_linears_(models["int4"], bits=4)
    print(f"## llama-8b graphed decode, TDPA_FUSED_DECODE off vs on, "
          f"attn_impl=hip, max_seq {max_seq} prompt {prompt}, {steps} steps "
          f"per repeat, {repeats} alternating repeats, ms/token")
    misses = []
    for tag, model in models.items():
        for B in (1, 8):
            idx = torch.randint(0, vocab, (B, prompt), device=dev)
            decs = {on: _decoder(model, B, max_seq, on, idx)
                    for on in (False, True)}
            for d in decs.values():
                for _ in range(4):
                    d.step()
            times = {on: [] for on in decs}
            for _ in range(repeats):
                for on, d in decs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        d.step()
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t0) / steps * 1e3)
            same = torch.equal(decs[False]._logits, decs[True]._logits)
            del decs, d
            torch.cuda.empty_cache()
            off, on = (statistics.median(times[k]) for k in (False, True))
            so, sn = _spread(times[False]), _spread(times[True])
            ok = on < off * (1 - max(so, sn))
            if not ok:
                misses.append((tag, B))
            print(f"{tag} B={B}: off {off:.3f} (spread {100 * so:.1f}%) on "
                  f"{on:.3f} (spread {100 * sn:.1f}%) on/off {on / off:.3f} "
                  f"{'ok' if ok else 'MISSED'}; last logits equal: {same}",
                  flush=True)
    print("bar (b) (knob on lower than off by more than the larger repeat "
          "spread, all four points): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)


@torch.no_grad()
def trace(on):
    from torchdistpackage_amd.models.llama import LlamaModel, llama3_8b
    m = LlamaModel(llama3_8b(), device=dev, dtype=torch.bfloat16).eval()
    d = _decoder(m, 1, 64, on, torch.randint(0, 128256, (1, 16), device=dev))
    d.step()
    marker = torch.ones(64, device=dev)
    torch.cuda.synchronize()
    marker.cumsum(0)
    d._graph.replay()
    marker.cumsum(0)
    torch.cuda.synchronize()
    print(f"TRACE fused_decode={'on' if on else 'off'} OK")


def count(root):
    """Dispatches between the two last cumsum markers of a kernel trace."""
    path = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"),
                     recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)),
                  key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, n in enumerate(names) if "cumsum" in n.lower()
             or "scan" in n.lower()]
    a, b = marks[-2], marks[-1]
    step = names[a + 1:b]
    print(f"{path}: {len(step)} kernels in one captured step")
    for n in sorted(set(step)):
        print(f"  {step.count(n):4d}  {n[:100]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", choices=("on", "off"))
    ap.add_argument("--count")
    args = ap.parse_args()
    if args.count:
        count(args.count)
        sys.exit(0)
    assert torch.cuda.is_available(), "needs a GPU"
    if args.trace:
        trace(args.trace == "on")
        sys.exit(0)
    main(args.iters, args.repeats)
    print("KBENCH FUSED DECODE OK")
