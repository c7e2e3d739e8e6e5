"""Same-process A/B of graphed decode, bf16 weights against int8 weights
(ops.quantize_linears_), shared by bench_decode.py and bench_decode_llama.py;
``bits=(8, 4)`` adds an int4 arm under the same method.

All decoders are alive in the same process; the arms alternate for three
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
def weights_ab(model, Dec, vocab, attn_impl, label, bits=(8,)):
    """bf16 against one quantised arm per entry of ``bits``, all alive in
    one process.  Bar (b): the last arm's ms/token is lower than the arm
    before it by more than the larger repeat spread of the two."""
    from torchdistpackage_amd.ops import quantize_linears_
    arms = {"bf16": model}
    for b in bits:
        arms[f"int{b}"] = copy.deepcopy(model)
        n = quantize_linears_(arms[f"int{b}"], bits=b)
        print(f"int{b}: {n} linears converted")
    new, old = list(arms)[-1], list(arms)[-2]
    print(f"## {label}: graphed decode, {' vs '.join(arms)} weights, "
          f"attn_impl={attn_impl}, 3 alternating repeats")
    for tag, m in arms.items():
        print(f"resident {tag}: linears {linear_bytes(m) / 1e9:.3f} GB, "
              f"whole model {all_bytes(m) / 1e9:.3f} GB")
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
        spr = {k: (max(v) - min(v)) / min(v) for k, v in times.items()}
        if not med[new] < med[old] * (1 - max(spr[new], spr[old])):
            misses.append((max_seq, prompt, B))
        print(f"max_seq={max_seq} prompt={prompt} B={B}: median ms/token "
              + " ".join(f"{k} {med[k]:.3f} (spread {100 * spr[k]:.1f}%)"
                         for k in arms)
              + "; " + " ".join(f"{new}/{k} {med[new] / med[k]:.3f}"
                                for k in arms if k != new), flush=True)
    print(f"{label} bar (b) ({new} ms/token lower than {old} by more than "
          "the repeat spread at every point): "
          + ("MET" if not misses else f"MISSED at {misses}"), flush=True)
