"""Decode attention A/B: the split-KV HIP kernel (ops.decode_attention)
against the path the graphed decoders use by default (repeat_interleave of
the GQA caches + full-length masked SDPA).

Op level: both versions are timed in the same process, alternating call by
call, with device events (median of ITERS calls after warm-up).  The K/V
caches rotate through enough copies to exceed the 256 MB Infinity Cache,
so the small shapes are not timed out of cache.  The kernel's rate is its
valid-KV bytes (K and V up to the current length) over its time, as a
share of the 8.0 TB/s HBM3E peak.

End to end: Llama-8B GraphedLlamaDecoder, both attn_impls alive in the same
process, three alternating repeats each; the spread is (max-min)/min.

    python scripts/kbench_decode_attn.py [--op-only | --e2e-only]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from torchdistpackage_amd import ops

HBM_PEAK = 8.0e12          # B/s, HBM3E spec peak of the MI355X
ITERS, WARM = 200, 20
ROTATE_BYTES = 512 << 20   # K+V bytes to cycle through (> Infinity Cache)

dev = torch.device("cuda")


def time_pair(fa, fb, iters=ITERS, warm=WARM):
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
def op_level():
    assert ops.extension_available(), "HIP extension must be built"
    print("## op level: (a) repeat_interleave + full-length masked SDPA, "
          "(b) decode_attention kernel")
    print(f"{'B':>2s} {'Hq':>3s} {'Hkv':>3s} {'D':>3s} {'Smax':>5s} "
          f"{'len':>5s} {'(a) us':>9s} {'(b) us':>9s} {'a/b':>6s} "
          f"{'(b) GB/s':>9s} {'%HBM':>5s} {'maxdiff':>8s}")
    misses = []
    for (B, Hq, Hkv, D) in [(1, 32, 8, 128), (8, 32, 8, 128),
                            (16, 16, 16, 128)]:
        rep = Hq // Hkv
        for Smax in (2048, 8192):
            kv_bytes = 2 * B * Hkv * Smax * D * 2
            ncopy = max(1, min(64, -(-ROTATE_BYTES // kv_bytes)))
            g = torch.Generator(device="cuda").manual_seed(0)
            ks = [torch.randn(B, Hkv, Smax, D, device=dev, generator=g,
                              dtype=torch.bfloat16) for _ in range(ncopy)]
            vs = [torch.randn(B, Hkv, Smax, D, device=dev, generator=g,
                              dtype=torch.bfloat16) for _ in range(ncopy)]
            q = torch.randn(B, Hq, 1, D, device=dev, generator=g,
                            dtype=torch.bfloat16)
            for length in (128, Smax // 2, Smax - 1):
                pos_t = torch.tensor([length - 1], device=dev)
                mask = torch.full((1, 1, 1, Smax), float("-inf"),
                                  dtype=torch.bfloat16, device=dev)
                mask[..., :length] = 0

                def fa(i):
                    kc, vc = ks[i % ncopy], vs[i % ncopy]
                    if rep > 1:
                        kc = kc.repeat_interleave(rep, dim=1)
                        vc = vc.repeat_interleave(rep, dim=1)
                    return F.scaled_dot_product_attention(q, kc, vc,
                                                          attn_mask=mask)

                def fb(i):
                    return ops.decode_attention(q, ks[i % ncopy],
                                                vs[i % ncopy], pos_t)

                diff = (fa(0).float() - fb(0).float()).abs().max().item()
                ta, tb = time_pair(fa, fb)
                valid = 2 * B * Hkv * length * D * 2
                rate = valid / (tb * 1e-6)
                print(f"{B:2d} {Hq:3d} {Hkv:3d} {D:3d} {Smax:5d} {length:5d} "
                      f"{ta:9.1f} {tb:9.1f} {ta / tb:6.2f} {rate / 1e9:9.0f} "
                      f"{100 * rate / HBM_PEAK:5.1f} {diff:8.4f}", flush=True)
                if length >= Smax // 2 and not tb < ta:
                    misses.append((B, Hq, Hkv, D, Smax, length))
            del ks, vs
            torch.cuda.empty_cache()
    print("op-level bar (kernel faster than (a) at every length >= Smax/2): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)


@torch.no_grad()
def end_to_end():
    from torchdistpackage_amd.inference.generate import GraphedLlamaDecoder
    from torchdistpackage_amd.models.llama import LlamaModel, llama3_8b
    print("## end to end: Llama-8B GraphedLlamaDecoder, ms/step "
          "(3 alternating repeats per impl)")
    torch.manual_seed(0)
    m = LlamaModel(llama3_8b(), device=dev, dtype=torch.bfloat16).eval()
    misses = []
    for max_seq, prompt, steps in ((192, 128, 16), (4096, 2048, 32)):
        for B in (1, 8):
            idx = torch.randint(0, 128256, (B, prompt), device=dev)
            decs = {}
            for impl in ("sdpa", "hip"):
                d = GraphedLlamaDecoder(m, batch=B, max_seq=max_seq,
                                        attn_impl=impl)
                d.prefill(idx)
                for _ in range(4):
                    d.step()
                decs[impl] = d
            times = {"sdpa": [], "hip": []}
            for _ in range(3):
                for impl in ("sdpa", "hip"):
                    d = decs[impl]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        d.step()
                    torch.cuda.synchronize()
                    times[impl].append(
                        (time.perf_counter() - t0) / steps * 1e3)
            del decs
            torch.cuda.empty_cache()
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max((max(v) - min(v)) / min(v) for v in times.values())
            slower = med["hip"] / med["sdpa"] - 1
            ok = slower <= spread
            if not ok:
                misses.append((max_seq, prompt, B))
            print(f"max_seq={max_seq} prompt={prompt} B={B}: "
                  f"sdpa {[f'{t:.3f}' for t in times['sdpa']]} "
                  f"hip {[f'{t:.3f}' for t in times['hip']]} "
                  f"median sdpa {med['sdpa']:.3f} hip {med['hip']:.3f} "
                  f"(hip/sdpa {med['hip'] / med['sdpa']:.3f}, "
                  f"spread {100 * spread:.1f}%)",
                  flush=True)
    print("end-to-end bar (hip not slower than sdpa beyond the repeat "
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
    print("KBENCH DECODE ATTN OK")
