"""Attention and tensor-parallel attention.

Reference parity: /root/reference/torchdistpackage/parallel/tensor_parallel/
attn.py (Attention/TpAttention: fused-QKV 3*dim ColParallel with
heads-per-partition = nh/tp, RowParallel out-proj).  Where the reference runs
naive math attention (attn.py:85-88: q@k^T -> softmax -> @v), this stack runs
the in-tree gfx950 flash-attention kernel (ops.flash_attention; blockwise
online-softmax per the reference spec explore/flash-attn/tile_attn.py).

Layout: activations are sequence-first (S, B, D); SP shards dim 0.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...ops import fused_qkv_attention, resolve_decode_attn_impl
from .tp_utils import (ColParallelLinear, RowParallelLinear, TpLinear,
                       copy_to_tp_region, gather_from_sequence_parallel_region,
                       get_tp_size, is_sequence_parallel)


def _cached_sdpa(q: torch.Tensor, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, pos0: int,
                 causal: bool) -> torch.Tensor:
    """Attention of q (B, H, S_new, hd) against cache positions
    [0, pos0+S_new), with the causal mask aligned so new position i sees
    cached positions <= pos0 + i (torch's ``is_causal`` is top-left
    aligned, wrong for a chunk appended mid-sequence)."""
    S = q.shape[2]
    ka = k_cache[:, :, :pos0 + S]
    va = v_cache[:, :, :pos0 + S]
    if not causal or S == 1:
        return F.scaled_dot_product_attention(q, ka, va)
    if pos0 == 0:
        return F.scaled_dot_product_attention(q, ka, va, is_causal=True)
    mask = torch.arange(pos0 + S, device=q.device)[None, :] <= \
        (pos0 + torch.arange(S, device=q.device))[:, None]
    return F.scaled_dot_product_attention(q, ka, va, attn_mask=mask)


def _cached_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      k_cache: torch.Tensor, v_cache: torch.Tensor, pos0,
                      causal: bool, attn_impl: Optional[str] = None,
                      mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The one KV-cache attention step behind every ``decode_step``.

    q (B, H, S, hd) and k, v (B, Hkv, S, hd), RoPE already applied; writes
    k/v into the caches (B, Hkv, max_seq, hd) at ``pos0`` and returns the
    attention output as (S, B, H*hd).  ``pos0`` has two forms, and each
    keeps its own cache write and SDPA call (other kernels, other bf16
    summation order — do not merge them):

    * host int (eager decode, any S): slice-assign write, then
      :func:`_cached_sdpa` over the valid prefix of the cache;
    * 1-element int64 tensor (hipGraph-captured decode, S == 1): never read
      back to the host; ``index_copy_`` write, then SDPA over the
      full-length cache under the additive ``mask`` (1, 1, 1, max_seq) the
      caller keeps open up to the current position.

    ``attn_impl="hip"`` runs ops.decode_attention on the un-expanded caches
    with either form; the SDPA routes expand K/V heads to Q heads first.
    """
    B, H, S, hd = q.shape
    hip = resolve_decode_attn_impl(attn_impl) == "hip"
    on_device = torch.is_tensor(pos0)
    if on_device:
        if S != 1:
            raise ValueError(f"tensor pos0 is the single-token step, got "
                             f"S={S}")
        if not hip and mask is None:
            raise ValueError("tensor pos0 with attn_impl='sdpa' needs the "
                             "cache visibility mask")
        k_cache.index_copy_(2, pos0, k)
        v_cache.index_copy_(2, pos0, v)
    else:
        k_cache[:, :, pos0:pos0 + S] = k
        v_cache[:, :, pos0:pos0 + S] = v
    if hip:
        assert causal or S == 1, \
            "decode_attention is causal over the new rows"
        o = ops.decode_attention(q, k_cache, v_cache, pos0)
    else:
        rep = H // k_cache.shape[1]
        if rep != 1:
            k_cache = k_cache.repeat_interleave(rep, dim=1)
            v_cache = v_cache.repeat_interleave(rep, dim=1)
        if on_device:
            o = F.scaled_dot_product_attention(q, k_cache, v_cache,
                                               attn_mask=mask)
        else:
            o = _cached_sdpa(q, k_cache, v_cache, pos0, causal)
    return o.permute(2, 0, 1, 3).reshape(S, B, H * hd)


def _sdpa(x_qkv: torch.Tensor, n_head: int, causal: bool) -> torch.Tensor:
    """(S, B, 3*Hl*hd) fused qkv -> (S, B, Hl*hd) attention output.

    Zero-copy path: the flash kernels read/write strided views into the fused
    qkv / output buffers (no permute-contiguous transposes).
    """
    return fused_qkv_attention(x_qkv.contiguous(), n_head, causal=causal)


class Attention(nn.Module):
    """Non-parallel attention (oracle for TP tests)."""

    def __init__(self, dim: int, n_head: int, bias: bool = True,
                 causal: bool = True, device=None, dtype=None):
        super().__init__()
        assert dim % n_head == 0
        self.n_head = n_head
        self.causal = causal
        self.qkv = TpLinear(dim, 3 * dim, bias=bias, device=device, dtype=dtype)
        self.proj = TpLinear(dim, dim, bias=bias, device=device, dtype=dtype)

    def forward(self, x):
        return self.proj(_sdpa(self.qkv(x), self.n_head, self.causal))


class TpAttention(nn.Module):
    """Tensor-parallel attention: heads split over TP ranks.

    qkv is ColParallel over 3*dim (each rank computes its nh/tp heads'
    Q,K,V); out-proj is RowParallel ending in all-reduce (or reduce-scatter
    into SP).  SP-tagged inputs are gathered on entry.
    """

    def __init__(self, dim: int, n_head: int, bias: bool = True,
                 causal: bool = True, sequence_parallel: bool = False,
                 device=None, dtype=None):
        super().__init__()
        tp = get_tp_size()
        assert dim % n_head == 0 and n_head % tp == 0, (dim, n_head, tp)
        self.n_head = n_head
        self.n_head_local = n_head // tp
        self.causal = causal
        self.qkv = ColParallelLinear(dim, 3 * dim, bias=bias,
                                     device=device, dtype=dtype)
        self.proj = RowParallelLinear(dim, dim, bias=bias,
                                      sequence_parallel=sequence_parallel,
                                      device=device, dtype=dtype)

    def forward(self, x, skip_bias: bool = False):
        """``skip_bias``: return the reduced out-projection WITHOUT
        ``proj.bias``; the caller adds it."""
        if is_sequence_parallel(x):
            x = gather_from_sequence_parallel_region(x)
        else:
            x = copy_to_tp_region(x)
        from ...ops.gemm import linear as fast_linear
        qkv = fast_linear(x, self.qkv.weight, self.qkv.bias)
        # qkv layout per rank: [q_local | k_local | v_local] thanks to the
        # interleaved loader (init_qkv_weight_from_full) / native init
        o = _sdpa(qkv, self.n_head_local, self.causal)
        return self.proj(o, skip_bias=skip_bias)

    @torch.no_grad()
    def decode_step(self, x: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, pos0,
                    attn_impl: Optional[str] = None,
                    mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """KV-cache inference step (tp=1 only; see inference/generate.py).

        x (S_new, B, D) — the new tokens' hidden states; writes their K/V
        into ``k_cache``/``v_cache`` (B, H, max_seq, hd) at ``pos0`` and
        attends q against positions [0, pos0+S_new).  ``pos0`` is a host
        int, or a 1-element device tensor with ``mask`` for the graphed
        step (see :func:`_cached_attention`).  ``attn_impl``: ``"sdpa"`` =
        eager SDPA over the cache, ``"hip"`` = the split-KV decode kernel
        (ops.decode_attention); ``None`` reads ``TDPA_DECODE_ATTN``
        (default sdpa).
        """
        from ...ops.gemm import linear as fast_linear
        S, B, D = x.shape
        hl = self.n_head_local
        hd = D // self.n_head
        qkv = fast_linear(x, self.qkv.weight, self.qkv.bias)
        q, k, v = qkv.split(hl * hd, dim=-1)

        def v4(t):
            return t.reshape(S, B, hl, hd).permute(1, 2, 0, 3)

        return self.proj(_cached_attention(v4(q), v4(k), v4(v), k_cache,
                                           v_cache, pos0, self.causal,
                                           attn_impl, mask))

    @torch.no_grad()
    def init_from_full(self, full_attn: Attention):
        self.qkv.init_qkv_weight_from_full(full_attn.qkv.weight,
                                           full_attn.qkv.bias, num_splits=3)
        self.proj.init_weight_from_full(full_attn.proj.weight,
                                        full_attn.proj.bias)
