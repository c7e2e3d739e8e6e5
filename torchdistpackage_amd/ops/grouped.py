"""Grouped linear over ragged expert segments (csrc/grouped_gemm.hip).

``grouped_linear(x, w, offs, bias)`` applies expert ``e``'s weight to rows
``[offs[e], offs[e+1])`` of one token buffer sorted by expert:

    y[offs[e]:offs[e+1]] = x[offs[e]:offs[e+1]] @ w[e].T + bias[e]

Dispatch:
- GPU bf16 with ``Dout`` and ``Din`` multiples of 256
  (``grouped_gemm_eligible``): the HIP kernels, forward, dgrad and wgrad, one
  launch each for all experts.  ``offs`` stays on the device: no host read,
  no ``.item()``, no stream sync, so the op captures into a hipGraph whose
  replay follows the CURRENT contents of ``offs`` (same total row count).
- any other GPU input: a per-segment ``torch.mm`` loop.  It reads ``offs`` on
  the host, i.e. it SYNCS the stream once per call and cannot be captured.
- CPU tensors: the same per-segment loop in plain torch, fp32 math for
  bf16/fp16 inputs and one rounding — the numerics oracle.

The caller guarantees ``offs[0] == 0`` and ``offs[E] == T``; the kernels
clamp every offset into ``[0, T]`` regardless and treat
``offs[e+1] <= offs[e]`` as an empty segment.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ext

# rows per tile of the fprop / dgrad kernels (csrc/grouped_gemm_plan.h GG_BM;
# the extension exports the same number as ``GROUPED_GEMM_BM``)
GROUPED_GEMM_BM = 256


def grouped_gemm_eligible(Dout: int, Din: int, dtype: torch.dtype) -> bool:
    """True when GPU tensors of this shape/dtype run the HIP kernels."""
    return (dtype == torch.bfloat16 and Dout > 0 and Din > 0
            and Dout % 256 == 0 and Din % 256 == 0)


class _GroupedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, offs, bias):
        ctx.save_for_backward(x, w, offs)
        ctx.has_bias = bias is not None
        return ext("grouped_linear").grouped_gemm_fprop(x, w, offs, bias)

    @staticmethod
    def backward(ctx, dy):
        x, w, offs = ctx.saved_tensors
        e = ext("grouped_linear")
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = e.grouped_gemm_dgrad(dy, w, offs)
        if ctx.needs_input_grad[1] or (ctx.has_bias
                                       and ctx.needs_input_grad[3]):
            dw, db = e.grouped_gemm_wgrad(dy, x, offs, ctx.has_bias)
        return dx, dw, None, db


def _grouped_linear_loop(x, w, offs, bias):
    """Per-segment loop in plain differentiable torch ops.  Reads ``offs``
    on the host."""
    T = x.shape[0]
    # T == 0: every segment is empty whatever offs holds — no host read
    o = [min(max(int(v), 0), T) for v in offs.tolist()] if T else \
        [0] * offs.numel()
    low = x.dtype in (torch.bfloat16, torch.float16) and not x.is_cuda
    parts = []
    for e in range(w.shape[0]):
        seg = x[o[e]:max(o[e + 1], o[e])]
        we = w[e]
        be = bias[e] if bias is not None else None
        if low:     # CPU oracle: fp32 math, one rounding
            y = F.linear(seg.float(), we.float(),
                         be.float() if be is not None else None).to(x.dtype)
        else:
            y = F.linear(seg, we, be)
        parts.append(y)
    return torch.cat(parts, dim=0)


def grouped_linear(x: torch.Tensor, w: torch.Tensor, offs: torch.Tensor,
                   bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (T, Din) sorted by expert, w (E, Dout, Din), offs (E+1,) int32 or
    int64 row offsets on x's device, bias (E, Dout) or None -> (T, Dout).
    Differentiable in x, w and bias (see the module docstring for the
    dispatch)."""
    E, Dout, Din = w.shape
    if x.dim() != 2 or x.shape[1] != Din:
        raise ValueError(f"grouped_linear: x {tuple(x.shape)} does not match "
                         f"w {tuple(w.shape)}")
    if offs.dim() != 1 or offs.numel() != E + 1:
        raise ValueError(f"grouped_linear: offs needs {E + 1} entries, got "
                         f"{tuple(offs.shape)}")
    if bias is not None and tuple(bias.shape) != (E, Dout):
        raise ValueError(f"grouped_linear: bias {tuple(bias.shape)} is not "
                         f"({E}, {Dout})")
    if (x.is_cuda and grouped_gemm_eligible(Dout, Din, x.dtype)
            and w.dtype == x.dtype
            and (bias is None or bias.dtype == x.dtype)):
        if offs.dtype not in (torch.int32, torch.int64):
            raise TypeError("grouped_linear: offs must be int32 or int64, "
                            f"got {offs.dtype}")
        # T == 0: the bindings return empty / zero tensors without a launch
        return _GroupedLinearFn.apply(
            x.contiguous(), w.contiguous(), offs.contiguous(),
            bias.contiguous() if bias is not None else None)
    return _grouped_linear_loop(x, w, offs, bias)
