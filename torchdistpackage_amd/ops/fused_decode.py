"""Fused glue ops of the Llama single-token decode step
(csrc/fused_decode.hip; docs/design/inference.md "Fused decode step").

Three ops, each the exact composition of ops that exist, in one launch:

* :func:`swiglu_linear`   ``swiglu(linear(x, w_gate), linear(x, w_up))``
* :func:`rope_kv_append`  RoPE on q and k, rotated k and v into the caches
* :func:`add_rms_norm`    ``x_new = x + y`` and ``rms_norm(x_new)``

The kernels make the roundings of the ops they replace, so results are
bit-identical; whatever a kernel does not cover runs the composition itself.
``TDPA_FUSED_DECODE=1`` (or :func:`set_fused_decode`) makes
models/llama.py's decode path use them; the ops themselves work either way.
"""

from __future__ import annotations

import os

import torch

from . import (Fp8KV, PagedKV, _bf16_rows_ok, _bf16_vecs_ok, ext, rms_norm,
               rope_rotate_half, swiglu)
from .gemm import decode_route, linear

# TDPA_FUSED_DECODE=1 routes the Llama decode step through the fused ops
# (read once, here)
_FUSED_DECODE = os.environ.get("TDPA_FUSED_DECODE", "0") == "1"

_ADD_RMS_MAX_D = 16384      # the RMSNorm kernels' widest row


def fused_decode_enabled() -> bool:
    return _FUSED_DECODE


def set_fused_decode(on: bool) -> bool:
    """Switch the fused Llama decode step on or off for this process;
    returns the previous setting.  A captured graph keeps the step it was
    captured with.  For tests and same-process A/B runs."""
    global _FUSED_DECODE
    prev, _FUSED_DECODE = _FUSED_DECODE, bool(on)
    return prev


def swiglu_linear(x: torch.Tensor, w_gate, w_up) -> torch.Tensor:
    """``swiglu(linear(x, w_gate), linear(x, w_up))``: the gate and up
    projections of a SwiGLU MLP and the activation.

    One HIP launch (``gemv_swiglu_bf16``) when ``linear`` would send both
    projections to the bf16 GEMV: CUDA bf16 ``x`` with grad disabled, both
    weights plain contiguous bf16 tensors of one shape, ``K % 8 == 0`` and
    ``ops.gemm.decode_route(M, N, K) == "gemv"``.  The two (M, N)
    intermediates are then never written, and the result is bit-identical.
    Anything else (``Int8Weight`` / ``Int4Weight``, M > 8, CPU tensors, grad
    enabled) returns the composition through the existing ops."""
    if (torch.is_tensor(w_gate) and torch.is_tensor(w_up) and x.is_cuda
            and not torch.is_grad_enabled()
            and x.dtype == w_gate.dtype == w_up.dtype == torch.bfloat16
            and w_gate.dim() == 2 and w_gate.shape == w_up.shape
            and x.shape[-1] == w_gate.shape[1] and x.numel() > 0
            and w_gate.is_contiguous() and w_up.is_contiguous()
            and w_gate.device == w_up.device == x.device
            and w_gate.data_ptr() % 16 == 0 and w_up.data_ptr() % 16 == 0):
        N, K = w_gate.shape
        M = x.numel() // K
        if K % 8 == 0 and N > 0 and decode_route(M, N, K) == "gemv":
            x2d = x.reshape(M, K)
            if not x2d.is_contiguous() or x2d.data_ptr() % 16 != 0:
                x2d = x2d.clone(memory_format=torch.contiguous_format)
            out = ext("swiglu_linear").gemv_swiglu(x2d, w_gate, w_up)
            return out.reshape(*x.shape[:-1], N)
    return swiglu(linear(x, w_gate), linear(x, w_up))


def rope_kv_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                   cos: torch.Tensor, sin: torch.Tensor,
                   k_cache: torch.Tensor, v_cache: torch.Tensor,
                   pos0) -> torch.Tensor:
    """RoPE (rotate-half) on q and k at positions ``[pos0, pos0+S)`` and both
    cache writes, one launch: returns rotated q, contiguous (B, H, S, D), and
    writes rotated k to ``k_cache[:, :, pos0:pos0+S]`` and v to
    ``v_cache[:, :, pos0:pos0+S]``.

    q (B, H, S, D) and k, v (B, Hkv, S, D) may be permuted views of the
    (S, B, heads*D) projection outputs (D contiguous, other strides free).
    The caches are dense (B, Hkv, Smax, D) tensors, last dim contiguous, other
    strides free.  ``pos0`` is a host int, which must lie in
    ``[0, min(table rows, Smax) - S]`` (it raises otherwise), or a 1-element
    int64 tensor: the kernel reads it on the device (hipGraph-capturable) and
    clamps it to that range before forming any address.

    GPU tensors run the HIP kernel (bf16, head dim 64 or 128; anything else
    raises): values are those of :func:`rope_rotate_half` bit for bit.  CPU
    tensors run ``rope_rotate_half`` and slice assignment.  ``Fp8KV`` and
    ``PagedKV`` caches raise ``TypeError``: they are written by
    ``kv_cache_append``."""
    if isinstance(k_cache, (Fp8KV, PagedKV)) or \
            isinstance(v_cache, (Fp8KV, PagedKV)):
        raise TypeError("rope_kv_append: the kernel writes dense bf16 caches; "
                        "Fp8KV and PagedKV take rope_rotate_half + "
                        "kv_cache_append")
    S = q.shape[2]
    Smax = k_cache.shape[2]
    hi = min(cos.shape[0], Smax) - S
    on_device = torch.is_tensor(pos0)
    if hi < 0:
        raise ValueError(f"rope_kv_append: S={S} exceeds the cos/sin table "
                         f"({cos.shape[0]} rows) or the cache (Smax={Smax})")
    if on_device:
        assert not torch.is_grad_enabled(), \
            "tensor pos0 is the no-grad decode path"
    elif pos0 < 0 or pos0 > hi:
        raise ValueError(f"rope_kv_append: pos0={pos0} with S={S} outside the "
                         f"cos/sin table ({cos.shape[0]} rows) or the cache "
                         f"(Smax={Smax})")
    if q.is_cuda:
        if not (q.dtype == k.dtype == v.dtype == k_cache.dtype
                == v_cache.dtype == torch.bfloat16):
            raise TypeError("rope_kv_append: the GPU kernel is bf16-only, "
                            f"got {q.dtype} into {k_cache.dtype}")
        e = ext("rope_kv_append")
        if on_device:
            return e.rope_kv_append(q, k, v, cos, sin, k_cache, v_cache,
                                    pos0, 0)
        return e.rope_kv_append(q, k, v, cos, sin, k_cache, v_cache, None,
                                int(pos0))
    if v.shape != k.shape or k_cache.shape != v_cache.shape or \
            k_cache.shape[:2] != k.shape[:2] or k_cache.shape[3] != k.shape[3]:
        raise ValueError("rope_kv_append: shape mismatch between "
                         f"k {tuple(k.shape)}, v {tuple(v.shape)} and caches "
                         f"{tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    p = min(max(int(pos0), 0), hi) if on_device else int(pos0)
    k_cache[:, :, p:p + S] = rope_rotate_half(k, cos, sin, p)
    v_cache[:, :, p:p + S] = v
    return rope_rotate_half(q, cos, sin, p)


def add_rms_norm(x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor,
                 eps: float = 1e-6):
    """``x_new = x + y`` and ``h = rms_norm(x_new, weight, eps)`` as
    ``(x_new, h)``: the junction between a branch of a pre-norm block and the
    next norm.  Inference only.  One HIP launch for same-shape contiguous
    16-byte aligned bf16 CUDA rows with ``D % 8 == 0`` under no_grad,
    bit-identical to the two ops; the two ops themselves otherwise."""
    if (not torch.is_grad_enabled() and _bf16_rows_ok(x, y)
            and _bf16_vecs_ok(x, weight)
            and x.shape[-1] <= _ADD_RMS_MAX_D):
        x_new, h = ext("add_rms_norm").add_rmsnorm(x, y, weight, eps)
        return x_new, h
    x_new = x + y
    return x_new, rms_norm(x_new, weight, eps)
