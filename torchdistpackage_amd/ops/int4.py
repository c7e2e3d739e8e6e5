"""Weight-only int4 linear for KV-cache decode ("W4A16").

Half the bytes of the int8 format (ops/int8.py) on the weight stream that
bounds single-token decode.  Scheme: symmetric int4 weights with one fp32
scale per output row and group of 128 along K, bf16 activations (never
quantised), fp32 accumulation, one rounding::

    y[m, n] = bf16( sum_g scale[n, g] * sum_{k in g} q[n, k] * x[m, k]
                    + bias[n] )

``q`` is an integer in [-8, 7] (the quantiser produces [-7, 7]), stored two
per byte in a uint8 tensor (N, K/2); ``scale`` is fp32 (N, K/128).
``K % 128 == 0`` is part of the format.  Inference only, tp = 1.

Nibble order: byte ``b`` of a row holds ``q[n, 2b]`` in its low nibble and
``q[n, 2b+1]`` in its high nibble, both two's complement, so the 32 nibbles of
a 16-byte load are 32 consecutive k in ascending bit order.  The kernels
convert with one sign-extending bit-field extract per nibble, int -> fp32 and
one packed bf16 convert per pair (2.5 VALU operations per weight).  An
interleaved order with a mantissa-or conversion was not tried.
:func:`pack_int4`, :func:`unpack_int4` and the kernel (csrc/gemv_int4.hip)
are the only code that knows the order.

Routes of :func:`int4_linear`:

- GPU, bf16 ``x``, 1 <= M <= 32, contiguous 16-byte aligned operands, bf16
  bias if any: the HIP kernel ``gemv_w4a16``: a dot2 arm for M <= 2 and an
  MFMA arm, whose cost per weight does not grow with M, above.
- any other GPU case (prefill chunks, M > 32): the weight is dequantised into
  a TRANSIENT tensor of x's dtype, freed after the call, and the existing
  ``linear()`` runs on it, exactly as int8 does.
- CPU: the formula above in fp32, the oracle for the kernel.

``TDPA_INT4_GEMV=0`` forces the dequantise route on GPU (A/B, debugging).
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import ext

GROUP = 128


def _read_env() -> bool:
    return os.environ.get("TDPA_INT4_GEMV", "1") != "0"


_INT4_GEMV = _read_env()        # read once, at import
_MAX_M = 32


def int4_gemv_enabled() -> bool:
    return _INT4_GEMV


def set_int4_gemv(on: bool) -> bool:
    """Switch the int4 kernel on or off for this process; returns the
    previous setting.  For tests and same-process A/B runs."""
    global _INT4_GEMV
    prev, _INT4_GEMV = _INT4_GEMV, bool(on)
    return prev


def pack_int4(q: torch.Tensor) -> torch.Tensor:
    """int8 (..., K) with values in [-8, 7], K even -> uint8 (..., K/2) in
    the module's nibble order."""
    if q.dtype != torch.int8 or q.shape[-1] % 2 != 0:
        raise TypeError("pack_int4: expected int8 with an even last dim, got "
                        f"{q.dtype} {tuple(q.shape)}")
    u = q.view(torch.uint8)
    return ((u[..., 0::2] & 0xF) | (u[..., 1::2] << 4)).contiguous()


def unpack_int4(packed: torch.Tensor) -> torch.Tensor:
    """uint8 (..., K/2) -> int8 (..., K), the inverse of :func:`pack_int4`."""
    if packed.dtype != torch.uint8:
        raise TypeError(f"unpack_int4: expected uint8, got {packed.dtype}")
    s = packed.view(torch.int8)
    lo = (s << 4) >> 4                  # arithmetic: sign-extends the nibble
    hi = s >> 4
    return torch.stack((lo, hi), dim=-1).reshape(*packed.shape[:-1],
                                                 2 * packed.shape[-1])


def quantize_int4(w: torch.Tensor, group: int = GROUP
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetric group-wise int4: ``scale[n, g] = max_{k in g} |w[n, k]| / 7``
    in fp32, ``q = clamp(round_half_even(w / scale), -7, 7)``.  An all-zero
    group gets ``q = 0`` and scale 1.  ``w`` (N, K) bf16 or fp32, CPU or GPU,
    ``K % 128 == 0``.  Returns ``(packed uint8 (N, K/2), scale (N, K/128))``."""
    if group != GROUP:
        raise ValueError(f"quantize_int4: only group = {GROUP} has a kernel, "
                         f"got {group}")
    if w.dim() != 2:
        raise ValueError(f"quantize_int4: expected an (N, K) weight, got "
                         f"{tuple(w.shape)}")
    N, K = w.shape
    if K == 0 or K % GROUP != 0:
        raise ValueError(f"quantize_int4: K = {K} is not a multiple of "
                         f"{GROUP}")
    wf = w.detach().float().reshape(N, K // GROUP, GROUP)
    amax = wf.abs().amax(dim=2)
    scale = torch.where(amax > 0, amax / 7.0, torch.ones_like(amax))
    q = torch.round(wf / scale[:, :, None]).clamp_(-7, 7).to(torch.int8)
    return pack_int4(q.reshape(N, K)), scale.contiguous()


def _dequantize(packed, scale, dtype):
    N, K2 = packed.shape
    q = unpack_int4(packed).float().reshape(N, -1, GROUP)
    return (q * scale[:, :, None]).reshape(N, 2 * K2).to(dtype)


def _check_qs(packed, scale):
    if not (torch.is_tensor(packed) and packed.dtype == torch.uint8
            and packed.dim() == 2):
        raise TypeError("int4 weight: packed must be a 2-D uint8 tensor, got "
                        f"{getattr(packed, 'dtype', type(packed))} "
                        f"{tuple(getattr(packed, 'shape', ()))}")
    if not (torch.is_tensor(scale) and scale.dtype == torch.float32):
        raise TypeError("int4 weight: scale must be an fp32 tensor, got "
                        f"{getattr(scale, 'dtype', type(scale))}")
    N, K = packed.shape[0], 2 * packed.shape[1]
    if K == 0 or K % GROUP != 0:
        raise ValueError(f"int4 weight: K = {K} is not a multiple of {GROUP}")
    if tuple(scale.shape) != (N, K // GROUP):
        raise ValueError(f"int4 weight: scale {tuple(scale.shape)} is not "
                         f"(N, K/{GROUP}) = {(N, K // GROUP)}")
    if scale.device != packed.device:
        raise ValueError("int4 weight: packed and scale live on different "
                         "devices")


class Int4Weight:
    """Handle on a quantised (N, K) weight: ``packed`` uint8 (N, K/2) and
    ``scale`` fp32 (N, K/128).  ``ops.gemm.linear(x, Int4Weight, bias)`` is
    ``int4_linear``."""

    __slots__ = ("packed", "scale")

    def __init__(self, packed: torch.Tensor, scale: torch.Tensor):
        _check_qs(packed, scale)
        self.packed = packed
        self.scale = scale

    @property
    def shape(self):
        return torch.Size((self.packed.shape[0], 2 * self.packed.shape[1]))

    @property
    def device(self):
        return self.packed.device

    def dequantize(self, dtype=torch.bfloat16) -> torch.Tensor:
        return _dequantize(self.packed, self.scale, dtype)

    def nbytes(self) -> int:
        return self.packed.numel() * self.packed.element_size() + \
            self.scale.numel() * self.scale.element_size()

    def __repr__(self):
        return f"Int4Weight(shape={tuple(self.shape)}, device={self.device})"


def int4_linear(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x (..., K) -> (..., N)`` with an int4 weight; see the module doc.

    The route is chosen silently.  On the GPU the kernel needs bf16 ``x``,
    M <= 32, contiguous 16-byte aligned ``packed``, contiguous ``scale`` and
    a contiguous bf16 ``bias``; miss one and EVERY call dequantises a
    transient weight, which is correct but slower than bf16 weights on
    decode."""
    _check_qs(packed, scale)
    N, K = packed.shape[0], 2 * packed.shape[1]
    if x.shape[-1] != K:
        raise ValueError(f"int4_linear: x (..., {x.shape[-1]}) against a "
                         f"weight with K = {K}")
    if bias is not None and bias.numel() != N:
        raise ValueError(f"int4_linear: bias has {bias.numel()} elements, "
                         f"the weight {N} rows")
    if torch.is_grad_enabled() and (
            x.requires_grad or (bias is not None and bias.requires_grad)):
        raise RuntimeError(
            "int4_linear is inference-only: it was called with grad enabled "
            "on an input that requires grad; wrap the call in "
            "torch.no_grad()")
    if not x.is_cuda:
        xg = x.float().reshape(-1, K // GROUP, GROUP)
        qg = unpack_int4(packed).float().reshape(N, K // GROUP, GROUP)
        y = (torch.einsum("mgk,ngk->mng", xg, qg) * scale).sum(-1)
        if bias is not None:
            y = y + bias.float()
        return y.to(x.dtype).reshape(*x.shape[:-1], N)
    M = x.numel() // K
    if (_INT4_GEMV and x.dtype == torch.bfloat16 and 1 <= M <= _MAX_M
            and packed.is_contiguous() and scale.is_contiguous()
            and packed.data_ptr() % 16 == 0
            and (bias is None or (bias.dtype == torch.bfloat16
                                  and bias.is_contiguous()))):
        x2d = x.reshape(M, K)
        if not x2d.is_contiguous() or x2d.data_ptr() % 16 != 0:
            x2d = x2d.clone(memory_format=torch.contiguous_format)
        out = ext("int4_linear").gemv_w4a16(x2d, packed, scale, bias)
        return out.reshape(*x.shape[:-1], N)
    from .gemm import linear
    return linear(x, _dequantize(packed, scale, x.dtype), bias)


# ---------------------------------------------------------------------------
# converting a model in place (driven by int8.quantize_linears_(bits=4))
# ---------------------------------------------------------------------------

_INT4_CLASSES = {}


def _int4_class(base):
    """The int4 twin of ``int8._int8_class``: a cached subclass of ``base``
    whose ``weight`` is an :class:`Int4Weight` over the ``qweight`` (packed
    uint8) / ``weight_scale`` buffers."""
    cls = _INT4_CLASSES.get(base)
    if cls is not None:
        return cls

    def weight(self):
        return Int4Weight(self.qweight, self.weight_scale)

    body = {"weight": property(weight), "_tdpa_int4": True,
            "__module__": base.__module__}
    if issubclass(base, nn.Linear):
        def forward(self, x):
            from .gemm import linear
            return linear(x, self.weight, self.bias)
        body["forward"] = forward
    cls = type("Int4" + base.__name__, (base,), body)
    _INT4_CLASSES[base] = cls
    return cls


def is_int4_linear(module: nn.Module) -> bool:
    return getattr(type(module), "_tdpa_int4", False)


def convert_linear_(mod: nn.Module) -> bool:
    """Convert one linear in place; False (and untouched) when its K is not
    a multiple of 128."""
    w = mod._parameters["weight"]
    if w.shape[1] == 0 or w.shape[1] % GROUP != 0:
        return False
    packed, scale = quantize_int4(w)
    del mod._parameters["weight"]
    mod.register_buffer("qweight", packed)
    mod.register_buffer("weight_scale", scale)
    mod.__class__ = _int4_class(type(mod))
    return True
