"""Prefill attention A/B/S: the flash-prefill HIP kernel
(ops.prefill_attention) against the two routes ``_cached_attention`` has for a
chunk of new rows over a KV cache.

    (A) hip route without the kernel: row-blocked ops.decode_attention, one
        launch pair per 16 // G query positions
    (S) sdpa route: repeat_interleave of the GQA caches, then _cached_sdpa
    (B) ops.prefill_attention, one launch

Op level: one process, the three arms alternating call by call, device
events, median of N calls after warm-up, three repeats; the spread of an arm
is (max - min) / min over its repeats.  The caches rotate through more than
512 MB so no arm is timed out of the Infinity Cache.  (B)'s rate is
4 * D * (visible q-key pairs) over its time, as a share of the bf16 MFMA
spec peak; the other bound, the K/V bytes every workgroup has to read over
the HBM peak, is printed next to it.  The outputs of (B) and (A) are
compared at every timed shape.

End to end (``--e2e-only``, or scripts/bench_decode_llama.py --prefill-attn):
Llama-8B, ``attn_impl="hip"`` with the knob off against on, three alternating
repeats: time to first token through GraphedLlamaDecoder.prefill (the sdpa
route next to them), and ms/token of speculative_generate with k = 8.

    python scripts/kbench_prefill_attn.py [--op-only | --e2e-only]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.parallel.tensor.attn import _cached_sdpa

MFMA_PEAK = 2.5e15         # FLOP/s, dense bf16 matrix spec peak of the MI355X
HBM_PEAK = 8.0e12          # B/s, HBM3E spec peak
REPEATS = 3
ROTATE_BYTES = 513 << 20   # K+V bytes to cycle through (> Infinity Cache)

dev = torch.device("cuda")


def time_arms(fns, iters, warm):
    """Median device time (us) of every arm, alternating call by call."""
    for i in range(warm):
        for f in fns:
            f(i)
    torch.cuda.synchronize()
    n = len(fns)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * n)]
          for _ in range(iters)]
    for i in range(iters):
        for a, f in enumerate(fns):
            ev[i][2 * a].record()
            f(i)
            ev[i][2 * a + 1].record()
    torch.cuda.synchronize()
    return [statistics.median(e[2 * a].elapsed_time(e[2 * a + 1])
                              for e in ev) * 1e3 for a in range(n)]


def visible_pairs(Sq, pos0):
    """q-key pairs of one head: row i sees pos0 + i + 1 keys."""
    return Sq * pos0 + Sq * (Sq + 1) // 2


@torch.no_grad()
def op_level():
    assert ops.extension_available(), "HIP extension must be built"
    print("## op level, us: (A) row-blocked decode_attention, (S) "
          "repeat_interleave + _cached_sdpa, (B) prefill_attention; "
          f"median of N calls, {REPEATS} repeats, spread = (max-min)/min")
    print(f"{'model':>6s} {'B':>2s} {'Sq':>5s} {'pos0':>5s} {'(A)':>10s} "
          f"{'(S)':>9s} {'(B)':>9s} {'A/B':>7s} {'S/B':>6s} {'sprA%':>6s} "
          f"{'sprS%':>6s} {'sprB%':>6s} {'TFLOP/s':>8s} {'%MFMA':>6s} "
          f"{'%HBM':>5s} {'bound':>5s} {'|B-A|':>8s}")
    miss_a, miss_s = [], []
    # barred: whole prompts and a chunk (Sq >= 128); reported only: the
    # verification chunk (Sq = 8) and the short chunks between, which place
    # the routing threshold of _cached_attention
    points = [(128, 0), (512, 0), (2048, 0), (512, 3584), (8, 2048),
              (8, 8000), (16, 2048), (32, 2048), (64, 2048), (16, 8000),
              (32, 8000), (64, 8000)]
    for name, Hq, Hkv, D in (("llama", 32, 8, 128), ("gpt2", 16, 16, 128)):
        G = Hq // Hkv
        for B in (1, 8):
            for Sq, pos0 in points:
                L = pos0 + Sq
                Smax = max(L, 256)
                kv_bytes = 2 * B * Hkv * Smax * D * 2
                ncopy = -(-ROTATE_BYTES // kv_bytes)
                g = torch.Generator(device="cuda").manual_seed(0)

                def rn(*s):
                    return torch.randn(*s, device=dev, generator=g,
                                       dtype=torch.bfloat16)

                ks = [rn(B, Hkv, Smax, D) for _ in range(ncopy)]
                vs = [rn(B, Hkv, Smax, D) for _ in range(ncopy)]
                q = rn(B, Hq, Sq, D)

                def fa(i):
                    return ops.decode_attention(q, ks[i % ncopy],
                                                vs[i % ncopy], pos0)

                def fs(i):
                    kc, vc = ks[i % ncopy], vs[i % ncopy]
                    if G > 1:
                        kc = kc.repeat_interleave(G, dim=1)
                        vc = vc.repeat_interleave(G, dim=1)
                    return _cached_sdpa(q, kc, vc, pos0, True)

                def fb(i):
                    return ops.prefill_attention(q, ks[i % ncopy],
                                                 vs[i % ncopy], pos0)

                diff = (fb(0).float() - fa(0).float()).abs().max().item()
                # (A) makes Sq*G/16 launch pairs per call: fewer calls there
                iters = 100 if Sq <= 8 else max(10, min(50, 8192 // Sq))
                reps = [time_arms((fa, fs, fb), iters, 2)
                        for _ in range(REPEATS)]
                ta, ts, tb = (statistics.median(r[a] for r in reps)
                              for a in range(3))
                spr = [(max(r[a] for r in reps) - min(r[a] for r in reps))
                       / min(r[a] for r in reps) for a in range(3)]
                flops = 4 * D * visible_pairs(Sq, pos0) * B * Hq
                rate = flops / (tb * 1e-6)
                t_mfma = flops / MFMA_PEAK
                # every (batch, kv head) reads its visible K and V once at
                # the very least
                t_hbm = 2 * B * Hkv * L * D * 2 / HBM_PEAK
                bound = "MFMA" if t_mfma >= t_hbm else "HBM"
                print(f"{name:>6s} {B:2d} {Sq:5d} {pos0:5d} {ta:10.1f} "
                      f"{ts:9.1f} {tb:9.1f} {ta / tb:7.2f} {ts / tb:6.2f} "
                      f"{100 * spr[0]:6.1f} {100 * spr[1]:6.1f} "
                      f"{100 * spr[2]:6.1f} {rate / 1e12:8.1f} "
                      f"{100 * t_mfma / (tb * 1e-6):6.1f} "
                      f"{100 * t_hbm / (tb * 1e-6):5.1f} {bound:>5s} "
                      f"{diff:8.4f}", flush=True)
                if Sq >= 128:
                    if not ta / tb - 1 > max(spr[0], spr[2]):
                        miss_a.append((name, B, Sq, pos0))
                    if not ts / tb - 1 > max(spr[1], spr[2]):
                        miss_s.append((name, B, Sq, pos0))
                del ks, vs
                torch.cuda.empty_cache()
    print("bar (a), (B) faster than (A) by more than the larger spread at "
          "every Sq >= 128: " + ("MET" if not miss_a else
                                 f"MISSED at {miss_a}"))
    print("bar (b), (B) faster than (S) by more than the larger spread at "
          "every Sq >= 128: " + ("MET" if not miss_s else
                                 f"MISSED at {miss_s}"), flush=True)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _report(tag, times, base, new):
    med = {k: statistics.median(v) for k, v in times.items()}
    spr = {k: (max(v) - min(v)) / min(v) for k, v in times.items()}
    gain = med[base] / med[new] - 1
    met = gain > max(spr[base], spr[new])
    print(f"{tag}: " + " ".join(
        f"{k} {[f'{t:.2f}' for t in v]} median {med[k]:.2f} "
        f"(spread {100 * spr[k]:.1f}%)" for k, v in times.items())
        + f" | {base}/{new} {med[base] / med[new]:.3f}: "
        + ("faster beyond the spread" if met else "NOT faster beyond the "
           "spread"), flush=True)
    return met


@torch.no_grad()
def end_to_end(m=None):
    from torchdistpackage_amd.inference.generate import (
        GraphedLlamaDecoder, speculative_generate)
    from torchdistpackage_amd.models.llama import (LlamaConfig, LlamaModel,
                                                   llama3_8b)
    print("## end to end: Llama-8B, attn_impl='hip', TDPA_PREFILL_ATTN off "
          f"against on, ms, {REPEATS} alternating repeats")
    torch.manual_seed(0)
    if m is None:
        m = LlamaModel(llama3_8b(), device=dev, dtype=torch.bfloat16).eval()
    prompt, misses = 2048, []
    prev = ops.prefill_attention_enabled()
    try:
        for B in (1, 8):
            idx = torch.randint(0, 128256, (B, prompt), device=dev)
            decs = {impl: GraphedLlamaDecoder(m, batch=B, max_seq=prompt + 64,
                                              attn_impl=impl)
                    for impl in ("hip", "sdpa")}
            arms = (("off", "hip", False), ("on", "hip", True),
                    ("sdpa", "sdpa", False))
            times = {a[0]: [] for a in arms}
            for rep in range(REPEATS + 1):          # repeat 0 is the warm-up
                for tag, impl, on in arms:
                    ops.set_prefill_attention(on)
                    t = _timed(lambda: decs[impl].prefill(idx))
                    if rep:
                        times[tag].append(t)
            del decs
            torch.cuda.empty_cache()
            if not _report(f"time to first token, prompt {prompt} B={B}",
                           times, "off", "on"):
                misses.append(f"ttft B={B}")

        draft = LlamaModel(LlamaConfig(n_layer=2), device=dev,
                           dtype=torch.bfloat16).eval()
        idx = torch.randint(0, 128256, (1, prompt), device=dev)
        times = {"off": [], "on": []}
        for rep in range(REPEATS + 1):
            for tag, on in (("off", False), ("on", True)):
                ops.set_prefill_attention(on)
                # the 2048-token prompt is in both calls: their difference
                # is 64 tokens of draft + 8-row verification rounds
                t8 = _timed(lambda: speculative_generate(
                    m, draft, idx, 8, k=8, attn_impl="hip"))
                t72 = _timed(lambda: speculative_generate(
                    m, draft, idx, 72, k=8, attn_impl="hip"))
                if rep:
                    times[tag].append((t72 - t8) / 64)
        if not _report("speculative_generate k=8, context 2048, ms/token",
                       times, "off", "on"):
            misses.append("speculative ms/token")
    finally:
        ops.set_prefill_attention(prev)
    print("end-to-end bar (knob on faster than off beyond the repeat "
          "spread): " + ("MET" if not misses else f"MISSED at {misses}"),
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
    print("KBENCH PREFILL ATTN OK")
