"""Same-process A/B of graphed decode, bf16 weights against int8 weights
(ops.quantize_linears_), shared by bench_decode.py and bench_decode_llama.py.

Both decoders are alive in the same process; the arms alternate for three
repeats, a figure is the median ms/token and the spread is the largest
(max-min)/min of an arm.  ``attn_impl`` is the same in both arms."""
import copy
import statistics
import time

import torch

POINTS = [(192, 128, 1), (192, 128, 8), (4096, 2048, 1), (4096, 2048, 8)]
# timed steps per repeat, after WARM warm-up steps: WARM + 3 * steps must fit
# between the prompt and max_seq
STEPS = {192: 16, 4096: 32}
WARM = 4


def linear_bytes(model):
    """Bytes held by the model's Tp/Col/Row/nn.Linear modules."""
    from torchdistpackage_amd.ops.int8 import linear_types
    total = 0
    for m in model.modules():
        if isinstance(m, linear_types()):
            for t in list(m._parameters.values()) + list(m._buffers.values()):
                if t is not None:
                    total += t.numel() * t.element_size()
    return total


def all_bytes(model):
    seen, total = set(), 0
    for t in list(model.parameters()) + list(model.buffers()):
        if t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


@torch.no_grad()
def int8_ab(model, Dec, vocab, attn_impl, label):
    from torchdistpackage_amd.ops import quantize_linears_
    m8 = copy.deepcopy(model)
    n = quantize_linears_(m8)
    print(f"## {label}: graphed decode, bf16 vs int8 weights ({n} linears "
          f"converted), attn_impl={attn_impl}, 3 alternating repeats")
    for tag, m in (("bf16", model), ("int8", m8)):
        print(f"resident {tag}: linears {linear_bytes(m) / 1e9:.3f} GB, "
              f"whole model {all_bytes(m) / 1e9:.3f} GB")
    arms = {"bf16": model, "int8": m8}
    misses = []
    for max_seq, prompt, B in POINTS:
        if max_seq > model.cfg.max_seq:
            print(f"max_seq={max_seq}: beyond the model's max_seq "
                  f"{model.cfg.max_seq}, skipped")
            continue
        idx = torch.randint(0, vocab, (B, prompt), device="cuda")
        decs = {}
        for tag, m in arms.items():
            d = Dec(m, batch=B, max_seq=max_seq, attn_impl=attn_impl)
            d.prefill(idx)
            for _ in range(WARM):
                d.step()
            decs[tag] = d
        steps = STEPS[max_seq]
        assert prompt + WARM + 3 * steps < max_seq
        times = {k: [] for k in arms}
        for _ in range(3):
            for tag, d in decs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    d.step()
                torch.cuda.synchronize()
                times[tag].append((time.perf_counter() - t0) / steps * 1e3)
        del decs
        torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max((max(v) - min(v)) / min(v) for v in times.values())
        ok = med["int8"] < med["bf16"] * (1 - spread)
        if not ok:
            misses.append((max_seq, prompt, B))
        print(f"max_seq={max_seq} prompt={prompt} B={B}: "
              f"bf16 {[f'{t:.3f}' for t in times['bf16']]} "
              f"int8 {[f'{t:.3f}' for t in times['int8']]} "
              f"median bf16 {med['bf16']:.3f} int8 {med['int8']:.3f} ms/token "
              f"(int8/bf16 {med['int8'] / med['bf16']:.3f}, "
              f"spread {100 * spread:.1f}%)", flush=True)
    print(f"{label} bar (b) (int8 ms/token lower than bf16 by more than the "
          "repeat spread at every point): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)
