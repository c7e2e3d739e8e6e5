"""Weight-only int8 linear for KV-cache decode ("W8A16").

Single-token decode streams the weights, and the bf16 GEMV (csrc/gemv.hip)
already reads them near HBM rate; the remaining lever is to read fewer
bytes.  Scheme: symmetric per-output-channel int8 weights, bf16 activations
(never quantised), fp32 accumulation::

    y[m, n] = bf16( scale[n] * sum_k q[n, k] * x[m, k] + bias[n] )

with ``q`` int8 (N, K) in [-127, 127] and ``scale`` fp32 (N,).  Inference
only, tp = 1.

Routes of :func:`int8_linear`:

- GPU, bf16 ``x``, M <= 32, K % 16 == 0, contiguous 16-byte aligned ``q``:
  the HIP kernel ``gemv_w8a16`` (csrc/gemv_int8.hip).  There is no library
  int8 x bf16 GEMM, so the kernel serves every M up to 32.
- any other GPU case (prefill chunks, M > 32, odd K): ``q`` is dequantised
  into a TRANSIENT weight of x's dtype, N*K elements, freed after the call,
  and the existing ``linear()`` runs on it.  Prefill is compute-bound, so
  the extra pass over the weight is small beside its GEMM; the resident
  model stays int8.
- CPU: the formula above in fp32, the oracle for the kernel.

``TDPA_INT8_GEMV=0`` forces the dequantise route on GPU (A/B, debugging).
"""

from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import torch
import torch.nn as nn

from . import ext


def _read_env() -> bool:
    return os.environ.get("TDPA_INT8_GEMV", "1") != "0"


_INT8_GEMV = _read_env()        # read once, at import
_MAX_M = 32


def int8_gemv_enabled() -> bool:
    return _INT8_GEMV


def set_int8_gemv(on: bool) -> bool:
    """Switch the int8 GEMV kernel on or off for this process; returns the
    previous setting.  For tests and same-process A/B runs."""
    global _INT8_GEMV
    prev, _INT8_GEMV = _INT8_GEMV, bool(on)
    return prev


def quantize_int8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetric per-row int8: ``scale[n] = max_k |w[n, k]| / 127`` in fp32,
    ``q = clamp(round_half_even(w / scale), -127, 127)``.  An all-zero row
    gets ``q = 0`` and scale 1.  ``w`` (N, K) bf16 or fp32, CPU or GPU."""
    if w.dim() != 2:
        raise ValueError(f"quantize_int8: expected an (N, K) weight, got "
                         f"{tuple(w.shape)}")
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.round(wf / scale[:, None]).clamp_(-127, 127).to(torch.int8)
    return q.contiguous(), scale.contiguous()


def _dequantize(q, scale, dtype):
    return (q.float() * scale[:, None]).to(dtype)


class Int8Weight:
    """Handle on a quantised (N, K) weight: ``q`` int8 and ``scale`` fp32
    (N,).  ``ops.gemm.linear(x, Int8Weight, bias)`` is ``int8_linear``."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        _check_qs(q, scale)
        self.q = q
        self.scale = scale

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    def dequantize(self, dtype=torch.bfloat16) -> torch.Tensor:
        return _dequantize(self.q, self.scale, dtype)

    def nbytes(self) -> int:
        return self.q.numel() * self.q.element_size() + \
            self.scale.numel() * self.scale.element_size()

    def __repr__(self):
        return f"Int8Weight(shape={tuple(self.shape)}, device={self.device})"


def _check_qs(q, scale):
    if not (torch.is_tensor(q) and q.dtype == torch.int8 and q.dim() == 2):
        raise TypeError("int8 weight: q must be a 2-D int8 tensor, got "
                        f"{getattr(q, 'dtype', type(q))} "
                        f"{tuple(getattr(q, 'shape', ()))}")
    if not (torch.is_tensor(scale) and scale.dtype == torch.float32):
        raise TypeError("int8 weight: scale must be an fp32 tensor, got "
                        f"{getattr(scale, 'dtype', type(scale))}")
    if scale.dim() != 1 or scale.numel() != q.shape[0]:
        raise ValueError(f"int8 weight: scale {tuple(scale.shape)} does not "
                         f"hold one value per row of q {tuple(q.shape)}")
    if scale.device != q.device:
        raise ValueError("int8 weight: q and scale live on different devices")


def int8_linear(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x (..., K) -> (..., N)`` with an int8 weight; see the module doc.

    The route is chosen silently.  On the GPU the kernel needs bf16 ``x``,
    M <= 32, K % 16 == 0, contiguous 16-byte aligned ``q``, contiguous
    ``scale`` and a contiguous bf16 ``bias``; miss one (for instance after
    casting the biases to fp32) and EVERY call dequantises a transient
    weight, which is correct but slower than bf16 weights on decode."""
    _check_qs(q, scale)
    N, K = q.shape
    if x.shape[-1] != K:
        raise ValueError(f"int8_linear: x (..., {x.shape[-1]}) against a "
                         f"weight with K = {K}")
    if bias is not None and bias.numel() != N:
        raise ValueError(f"int8_linear: bias has {bias.numel()} elements, "
                         f"the weight {N} rows")
    if torch.is_grad_enabled() and (
            x.requires_grad or (bias is not None and bias.requires_grad)):
        raise RuntimeError(
            "int8_linear is inference-only: it was called with grad enabled "
            "on an input that requires grad; wrap the call in "
            "torch.no_grad()")
    if not x.is_cuda:
        y = (x.float() @ q.float().t()) * scale
        if bias is not None:
            y = y + bias.float()
        return y.to(x.dtype)
    M = x.numel() // K
    if (_INT8_GEMV and x.dtype == torch.bfloat16 and 1 <= M <= _MAX_M
            and K % 16 == 0 and q.is_contiguous() and scale.is_contiguous()
            and q.data_ptr() % 16 == 0
            and (bias is None or (bias.dtype == torch.bfloat16
                                  and bias.is_contiguous()))):
        x2d = x.reshape(M, K)
        if not x2d.is_contiguous() or x2d.data_ptr() % 16 != 0:
            x2d = x2d.clone(memory_format=torch.contiguous_format)
        out = ext("int8_linear").gemv_w8a16(x2d, q, scale, bias)
        return out.reshape(*x.shape[:-1], N)
    from .gemm import linear
    return linear(x, _dequantize(q, scale, x.dtype), bias)


# ---------------------------------------------------------------------------
# converting a model in place
# ---------------------------------------------------------------------------

_INT8_CLASSES = {}


def linear_types():
    """The module classes ``quantize_linears_`` converts (Col/Row-parallel
    linears are ``TpLinear``)."""
    from ..parallel.tensor.tp_utils import TpLinear
    return (TpLinear, nn.Linear)


def _int8_class(base):
    """A cached subclass of ``base`` whose ``weight`` is an
    :class:`Int8Weight` over the ``qweight`` / ``weight_scale`` buffers.  The
    host module survives, so ``bias``, ``skip_bias``, the TP plumbing and
    every call site that reads ``.weight`` keep working."""
    cls = _INT8_CLASSES.get(base)
    if cls is not None:
        return cls

    def weight(self):
        return Int8Weight(self.qweight, self.weight_scale)

    body = {"weight": property(weight), "_tdpa_int8": True,
            "__module__": base.__module__}
    if issubclass(base, nn.Linear):
        def forward(self, x):
            from .gemm import linear
            return linear(x, self.weight, self.bias)
        body["forward"] = forward
    cls = type("Int8" + base.__name__, (base,), body)
    _INT8_CLASSES[base] = cls
    return cls


def is_int8_linear(module: nn.Module) -> bool:
    return getattr(type(module), "_tdpa_int8", False)


def quantize_linears_(model: nn.Module, skip: Iterable[str] = ()) -> int:
    """Quantise every ``TpLinear`` / ``ColParallelLinear`` /
    ``RowParallelLinear`` / ``nn.Linear`` of ``model`` in place and return
    how many were converted.  The ``weight`` Parameter is dropped, int8
    ``qweight`` and fp32 ``weight_scale`` buffers are registered, and the
    module is re-classed so that ``module.weight`` is an :class:`Int8Weight`.

    Left alone: embeddings, the (tied or untied) LM head, norms, MoE experts
    (none of them is one of the four classes, or they sit under an MoE
    layer), modules named in ``skip`` (a name of ``model.named_modules()``;
    it covers the submodules below it), and modules already converted.
    tp = 1 only; the converted model is for inference.

    The re-classed types are made at run time, so ``copy.deepcopy``,
    ``state_dict`` and ``load_state_dict`` (into an equally converted model)
    work, but pickling the whole module (``torch.save(model)``) does not:
    save the state dict."""
    from ..parallel.tensor import get_tp_size
    assert get_tp_size() == 1, "quantize_linears_ supports tp=1 only"
    from ..moe.layer import Expert, ExpertParallelMoE, TopKRouter
    moe_types = (ExpertParallelMoE, Expert, TopKRouter)
    skip = tuple(skip)
    types = linear_types()

    def under(name, roots):
        return any(r == "" or name == r or name.startswith(r + ".")
                   for r in roots)

    moe_roots = [n for n, m in model.named_modules()
                 if isinstance(m, moe_types)]
    count = 0
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, types) or is_int8_linear(mod):
            continue
        if under(name, skip) or under(name, moe_roots):
            continue
        w = mod._parameters.get("weight")
        if w is None or w.dim() != 2:
            continue
        q, scale = quantize_int8(w)
        del mod._parameters["weight"]
        mod.register_buffer("qweight", q)
        mod.register_buffer("weight_scale", scale)
        mod.__class__ = _int8_class(type(mod))
        count += 1
    return count
