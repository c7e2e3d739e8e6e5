"""fp8 (OCP e4m3) KV cache: the cache type, the quantising append and the
dequantise (csrc/kv_fp8.hip).

Format.  A cache row is one (batch, kv head, position) with ``D`` elements:
``D`` bytes of e4m3 (``torch.float8_e4m3fn`` encoding) in a uint8 tensor
(B, Hkv, Smax, D), and one fp32 scale in a tensor (B, Hkv, Smax).  K and V
each have their own pair.  The scale is per row and a power of two, chosen
when the row is written::

    amax  = max|x| over the row = m * 2^e,  m in [0.5, 1)
    scale = 2^(e-9) if m <= 0.875 else 2^(e-8)     (exponent floored at -64)
    byte  = e4m3_rne(x / scale)

so ``amax/scale`` lies in (224, 448] (448 = 0.875 * 2^9 is the e4m3 maximum)
and the converter's overflow behaviour is never met.  ``x / scale`` and
``fp32(byte) * scale`` are exact, so the only rounding is the one to e4m3.
An all-zero row (and any row with ``amax < 2^-55``) takes the floor scale
2^-64.  Non-finite K/V are out of contract.  Per-row scales need no
calibration, make the cache bytes independent of how a prompt is chunked, and
keep a speculative rollback free (a stale row's scale is overwritten with
its data).  Overhead: 4 bytes per ``D`` (3 % at hd 128, 6 % at hd 64).

GPU tensors run the HIP kernels; CPU tensors run the same rule in torch
(``torch.frexp`` / ``torch.ldexp``, ``.to(torch.float8_e4m3fn)``), which is
the oracle for them.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ext

SCALE_EXP_FLOOR = -64       # smallest scale 2^-64, also the all-zero row's


class Fp8KV:
    """One fp8 cache (K or V): ``data`` uint8 (B, Hkv, Smax, D) and ``scale``
    fp32 (B, Hkv, Smax).  Not a tensor subclass: the models pass it through
    to ``_cached_attention`` untouched, and ops.kv_cache_append /
    ops.decode_attention dispatch on it."""

    def __init__(self, data: torch.Tensor, scale: torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 4:
            raise TypeError("Fp8KV: data must be uint8 (B, Hkv, Smax, D)")
        if scale.dtype != torch.float32 or scale.shape != data.shape[:3]:
            raise TypeError("Fp8KV: scale must be fp32 (B, Hkv, Smax)")
        if not (data.is_contiguous() and scale.is_contiguous()):
            raise ValueError("Fp8KV: data and scale must be contiguous")
        if data.device != scale.device:
            raise ValueError("Fp8KV: data and scale on different devices")
        self.data, self.scale = data, scale

    @classmethod
    def zeros(cls, batch: int, n_kv_head: int, max_seq: int, head_dim: int,
              device=None) -> "Fp8KV":
        """Zeroed storage: zero bytes under the floor scale."""
        data = torch.zeros(batch, n_kv_head, max_seq, head_dim,
                           dtype=torch.uint8, device=device)
        scale = torch.full((batch, n_kv_head, max_seq),
                           2.0 ** SCALE_EXP_FLOOR, dtype=torch.float32,
                           device=device)
        return cls(data, scale)

    @property
    def shape(self) -> torch.Size:
        return self.data.shape

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    def nbytes(self) -> int:
        return self.data.numel() + 4 * self.scale.numel()

    def dequantize(self, dtype: torch.dtype = torch.bfloat16,
                   length: Optional[int] = None) -> torch.Tensor:
        """Dense (B, Hkv, length, D) tensor of the first ``length`` positions
        (default all); exact in bf16 and fp32."""
        Smax = self.shape[2]
        L = Smax if length is None else int(length)
        if L < 0 or L > Smax:
            raise ValueError(f"Fp8KV.dequantize: length={L} outside the "
                             f"cache (Smax={Smax})")
        if self.is_cuda:
            if dtype not in (torch.bfloat16, torch.float32):
                raise TypeError("Fp8KV.dequantize: the GPU kernel writes "
                                f"bf16 or fp32, got {dtype}")
            return ext("kv_fp8_dequant").kv_fp8_dequant(
                self.data, self.scale, L, dtype == torch.bfloat16)
        vals = self.data[:, :, :L].view(torch.float8_e4m3fn).float()
        return (vals * self.scale[:, :, :L, None]).to(dtype)


def quantize_kv_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rule of the module docstring in torch: ``x`` (..., D) of any float
    dtype -> (uint8 bytes (..., D), fp32 scales (...))."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    m, e = torch.frexp(amax)                       # m in [0.5, 1), or 0
    e = e - 9 + (m > 0.875).to(e.dtype)
    e = torch.where(amax > 0, e, torch.full_like(e, SCALE_EXP_FLOOR))
    e = e.clamp_min(SCALE_EXP_FLOOR)
    scale = torch.ldexp(torch.ones_like(amax), e)
    data = (xf / scale[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return data, scale


def _positions(pos0, B: int, Smax: int, S: int, device) -> torch.Tensor:
    """(B,) clamped write positions from either form of ``pos0``."""
    if torch.is_tensor(pos0):
        pos = pos0.reshape(-1).to(device=device, dtype=torch.long)
        if pos.numel() not in (1, B):
            raise ValueError("kv_cache_append: pos0 tensor must have 1 or B "
                             f"elements, got {pos.numel()}")
        pos = pos.expand(B) if pos.numel() == 1 else pos
        return pos.clamp(0, Smax - S)
    if pos0 < 0 or pos0 + S > Smax:
        raise ValueError(f"kv_cache_append: pos0={pos0} with S={S} outside "
                         f"the cache (Smax={Smax})")
    return torch.full((B,), int(pos0), dtype=torch.long, device=device)


def kv_cache_append(k_cache, v_cache, k: torch.Tensor, v: torch.Tensor,
                    pos0) -> None:
    """Write k, v (B, Hkv, S, D) into the caches at positions
    ``[pos0, pos0+S)``.  ``pos0`` is a host int, or an int64 tensor with 1 or
    B elements read on the device (hipGraph-capturable; clamped to
    ``[0, Smax-S]``).

    :class:`Fp8KV` caches quantise on the way in: on the GPU one launch of
    the HIP kernel for K and V together (bf16 sources, head dim 64 or 128,
    last dim contiguous, other strides free); on the CPU the torch rule.
    bf16/fp32 tensor caches take the plain copy (slice-assign for a host
    int, ``index_copy_`` for a 1-element tensor).  Mixing the two raises.
    """
    kq, vq = isinstance(k_cache, Fp8KV), isinstance(v_cache, Fp8KV)
    if kq != vq:
        raise TypeError("kv_cache_append: k_cache and v_cache must both be "
                        "Fp8KV or both be tensors")
    B, Hkv, S, D = k.shape
    if not kq:
        if torch.is_tensor(pos0):
            k_cache.index_copy_(2, pos0, k)
            v_cache.index_copy_(2, pos0, v)
        else:
            k_cache[:, :, pos0:pos0 + S] = k
            v_cache[:, :, pos0:pos0 + S] = v
        return
    if k_cache.shape != v_cache.shape or v.shape != k.shape or \
            k_cache.shape[:2] != (B, Hkv) or k_cache.shape[3] != D:
        raise ValueError("kv_cache_append: shape mismatch between "
                         f"k {tuple(k.shape)}, v {tuple(v.shape)} and caches "
                         f"{tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    Smax = k_cache.shape[2]
    if k.is_cuda:
        if k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
            raise TypeError("kv_cache_append: the GPU kernel quantises bf16, "
                            f"got {k.dtype}")
        if D not in (64, 128):
            raise ValueError("kv_cache_append: the GPU kernel covers head "
                             f"dim 64 and 128, got {D}")
        e = ext("kv_cache_append")
        if torch.is_tensor(pos0):
            e.kv_fp8_append(k_cache.data, k_cache.scale, v_cache.data,
                            v_cache.scale, k, v, pos0, 0)
        else:
            pos0 = int(pos0)
            if pos0 < 0 or pos0 + S > Smax:
                raise ValueError(f"kv_cache_append: pos0={pos0} with S={S} "
                                 f"outside the cache (Smax={Smax})")
            e.kv_fp8_append(k_cache.data, k_cache.scale, v_cache.data,
                            v_cache.scale, k, v, None, pos0)
        return
    pos = _positions(pos0, B, Smax, S, k.device)
    for cache, x in ((k_cache, k), (v_cache, v)):
        data, scale = quantize_kv_rows(x)
        for b in range(B):
            p = int(pos[b])
            cache.data[b, :, p:p + S] = data[b]
            cache.scale[b, :, p:p + S] = scale[b]
