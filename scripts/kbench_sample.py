"""Sampling A/B at the decode shapes: one next-token draw from (B, V) bf16
logits, V in {50257, 128256}, B in {1, 8, 16},
  (A) the torch chain of inference/generate.py:_sample (float, topk,
      masked_fill, softmax, multinomial), extended with the usual sort +
      cumsum mask where top_p is set,
  (B) ops.sample_logits (csrc/sample.hip, one launch) on u = torch.rand(B),
      the draw included in the timed region as generate() pays it.
Both arms live in one process and alternate call by call; device events,
median of ITERS calls, REPEATS repeats, spread = (max - min) / min per arm;
the logits rotate through copies that together exceed 512 MB.  For (B) the
row bytes over the time are reported against the 8 TB/s spec peak together
with the number of passes the kernel makes over a row.

    python scripts/kbench_sample.py [--iters N]

``end_to_end(model)`` (scripts/bench_decode_llama.py --sample) is the decode
A/B: graphed greedy against graphed sampled ms/token, and eager
``generate(sampler="torch")`` against ``"hip"``, at max_seq / prompt 4096 /
2048, B = 1 and 8, ``attn_impl="hip"``, both arms alive in one process and
alternating over REPEATS repeats.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops

REPEATS = 3
PEAK = 8e12                    # HBM bytes/s, spec
T = 0.8
dev = torch.device("cuda")


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


def sample_torch(logits, top_k, top_p):
    logits = logits.float() / max(T, 1e-5)
    if top_k is not None and top_k < logits.shape[-1]:
        kth = logits.topk(top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p is not None:
        srt, order = logits.sort(dim=-1, descending=True)
        cum = torch.softmax(srt, dim=-1).cumsum(-1)
        drop = cum - torch.softmax(srt, dim=-1) >= top_p
        logits = logits.masked_fill(
            torch.zeros_like(drop).scatter_(1, order, drop), float("-inf"))
    return torch.multinomial(torch.softmax(logits, dim=-1), 1).squeeze(-1)


def passes(top_k, top_p):
    """Passes of the bf16 kernel over a row (csrc/sample.hip)."""
    return 2 + (top_k is not None) + (top_p is not None)


def main(iters):
    print(f"## one draw from (B, V) bf16 logits, T={T}, median of {iters}, "
          f"{REPEATS} repeats, us; spread = (max - min) / min")
    verdict = []
    for V in (50257, 128256):
        for B in (1, 8, 16):
            ncopy = (512 << 20) // (B * V * 2) + 1
            g = torch.Generator(device=dev).manual_seed(0)
            xs = [(torch.randn(B, V, device=dev, generator=g) * 4)
                  .to(torch.bfloat16) for _ in range(ncopy)]
            for top_k, top_p in ((None, None), (50, None), (None, 0.9),
                                 (50, 0.9)):
                def arm_a(i):
                    return sample_torch(xs[i % ncopy], top_k, top_p)

                def arm_b(i):
                    u = torch.rand(B, device=dev)
                    return ops.sample_logits(xs[i % ncopy], u, T, top_k,
                                             top_p)

                reps = [time_pair(arm_a, arm_b, iters)
                        for _ in range(REPEATS)]
                ta, tb = [r[0] for r in reps], [r[1] for r in reps]
                sa = (max(ta) - min(ta)) / min(ta)
                sb = (max(tb) - min(tb)) / min(tb)
                ma, mb = statistics.median(ta), statistics.median(tb)
                row = B * V * 2
                line = (f"V={V} B={B} top_k={top_k} top_p={top_p}: "
                        f"(A) {' '.join(f'{t:7.1f}' for t in ta)} "
                        f"spread {sa:.3f}  "
                        f"(B) {' '.join(f'{t:7.1f}' for t in tb)} "
                        f"spread {sb:.3f}  A/B {ma / mb:.2f}  (B) "
                        f"{passes(top_k, top_p)} passes, row bytes / time "
                        f"{row / (mb * 1e-6) / 1e9:.1f} GB/s = "
                        f"{100 * row / (mb * 1e-6) / PEAK:.2f}% of 8 TB/s")
                if top_k == 50:
                    ok = ma / mb - 1 > max(sa, sb)
                    verdict.append(ok)
                    line += f"  bar: {'met' if ok else 'MISSED'}"
                print(line, flush=True)
            del xs
    print("bar, (B) faster than (A) by more than the larger repeat spread at "
          f"every top_k=50 point: {'met' if all(verdict) else 'MISSED'}")


def end_to_end(m, vocab=128256, max_seq=4096, prompt=2048, new=32):
    from torchdistpackage_amd.inference import generate
    from torchdistpackage_amd.inference.generate import GraphedDecoder
    kw = dict(temperature=T, top_k=50, top_p=0.9)
    # the prompt goes through the flash-prefill kernel in every arm
    ops.set_prefill_attention(True)
    print(f"## llama-8b decode, max_seq {max_seq} prompt {prompt}, "
          f"attn_impl=hip, {new} tokens per repeat, {REPEATS} alternating "
          f"repeats, ms/token; sampling: {kw}")
    for B in (1, 8):
        idx = torch.randint(0, vocab, (B, prompt), device=dev)
        decs = [("graphed greedy", GraphedDecoder(m, batch=B, max_seq=max_seq,
                                                  attn_impl="hip")),
                ("graphed sampled", GraphedDecoder(m, batch=B,
                                                   max_seq=max_seq,
                                                   attn_impl="hip", seed=0,
                                                   **kw))]
        for _, d in decs:
            d.prefill(idx)
            for _ in range(4):
                d.step()
        res = {name: [] for name, _ in decs}
        for _ in range(REPEATS):
            for name, d in decs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(new):
                    d.step()
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) / new * 1e3)
        del decs, d
        g = torch.Generator(device=dev).manual_seed(0)

        def eager(sampler, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate(m, idx, n, greedy=False, temperature=T, top_k=50,
                     attn_impl="hip", sampler=sampler, generator=g)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for sampler in ("torch", "hip"):
            eager(sampler, 2)
            res[f"eager {sampler}"] = []
        for _ in range(REPEATS):
            for sampler in ("torch", "hip"):
                dt = eager(sampler, new + 1) - eager(sampler, 1)
                res[f"eager {sampler}"].append(dt / new * 1e3)
        for name, ts in res.items():
            print(f"B={B} {name:16s} {' '.join(f'{t:7.3f}' for t in ts)}  "
                  f"median {statistics.median(ts):.3f}", flush=True)
        med = {n: statistics.median(ts) for n, ts in res.items()}
        print(f"B={B}: sampling over greedy "
              f"{med['graphed sampled'] - med['graphed greedy']:+.3f} ms/token"
              f" ({med['graphed sampled'] / med['graphed greedy']:.3f}x); "
              f"eager torch / hip "
              f"{med['eager torch'] / med['eager hip']:.3f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.extension_available(), "HIP extension must be built"
    main(args.iters)
    print("KBENCH SAMPLE OK")
