"""Paged bf16 KV cache: the cache type and the append through the block
table (csrc/decode_attn_paged.hip, which also holds the decode-attention
kernel that reads it).

Format.  One paged cache (K or V) is a ``pool`` (P, Hkv, page, D) and a
``block_table`` (B, NB) int32: entry ``[b, i]`` is the pool page that holds
positions ``[i*page, (i+1)*page)`` of sequence ``b``.  ``page`` is a power of
two in 16..128 and the capacity is ``Smax = NB * page``.  K and V of one
layer share one table (the same tensor); each has its own pool.

Contract on the table: entries for positions at or past the valid length may
hold anything, no kernel dereferences them; every entry a kernel does read is
clamped to ``[0, P-1]`` before an address is formed, so a stale table may
give a wrong answer, never an out-of-range access.  Rows may name the same
page (read-only prefix sharing); appending into a shared page is the
caller's responsibility.  There is no allocator here: the caller owns the
table's contents.

GPU tensors run the HIP kernels; CPU tensors run the same indexing in torch,
which is the oracle for them.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import ext_nopk
from . import kv_fp8

PAGE_SIZES = (16, 32, 64, 128)


class PagedKV:
    """One paged cache (K or V): ``pool`` (P, Hkv, page, D) and
    ``block_table`` int32 (B, NB).  Not a tensor subclass: the models pass it
    through to ``_cached_attention`` untouched, and ops.kv_cache_append /
    ops.decode_attention dispatch on it."""

    def __init__(self, pool: torch.Tensor, block_table: torch.Tensor):
        if pool.dim() != 4 or not pool.is_floating_point():
            raise TypeError("PagedKV: pool must be a float (P, Hkv, page, D) "
                            "tensor")
        if pool.shape[2] not in PAGE_SIZES:
            raise ValueError("PagedKV: page size must be a power of two in "
                             f"16..128, got {pool.shape[2]}")
        if block_table.dtype != torch.int32 or block_table.dim() != 2:
            raise TypeError("PagedKV: block_table must be int32 (B, NB)")
        if not (pool.is_contiguous() and block_table.is_contiguous()):
            raise ValueError("PagedKV: pool and block_table must be "
                             "contiguous")
        if pool.device != block_table.device:
            raise ValueError("PagedKV: pool and block_table on different "
                             "devices")
        if pool.shape[0] < 1 or block_table.shape[1] < 1:
            raise ValueError("PagedKV: empty pool or block_table")
        self.pool, self.block_table = pool, block_table

    @classmethod
    def zeros(cls, batch: int, n_kv_head: int, max_seq: int, head_dim: int,
              page_size: int = 16, dtype: torch.dtype = torch.bfloat16,
              device=None, block_table: Optional[torch.Tensor] = None,
              num_pages: Optional[int] = None) -> "PagedKV":
        """Zeroed pool under ``block_table`` (default: the identity
        ``arange(B*NB).view(B, NB)`` with ``NB = ceil(max_seq / page)``) of
        ``num_pages`` pages (default exactly ``B*NB``)."""
        if page_size not in PAGE_SIZES:
            raise ValueError("PagedKV: page size must be a power of two in "
                             f"16..128, got {page_size}")
        nb = -(-int(max_seq) // page_size)
        if block_table is None:
            block_table = torch.arange(batch * nb, dtype=torch.int32,
                                       device=device).view(batch, nb)
        elif tuple(block_table.shape) != (batch, nb):
            raise ValueError(f"PagedKV: block_table {tuple(block_table.shape)}"
                             f" does not cover ({batch}, {nb}) pages")
        if num_pages is None:
            num_pages = batch * nb
        pool = torch.zeros(num_pages, n_kv_head, page_size, head_dim,
                           dtype=dtype, device=block_table.device)
        return cls(pool, block_table)

    @property
    def page_size(self) -> int:
        return self.pool.shape[2]

    @property
    def shape(self) -> torch.Size:
        B, NB = self.block_table.shape
        _, Hkv, page, D = self.pool.shape
        return torch.Size((B, Hkv, NB * page, D))

    @property
    def device(self) -> torch.device:
        return self.pool.device

    @property
    def is_cuda(self) -> bool:
        return self.pool.is_cuda

    def nbytes(self) -> int:
        return self.pool.numel() * self.pool.element_size() + \
            4 * self.block_table.numel()

    def _ids(self) -> torch.Tensor:
        return self.block_table.long().clamp(0, self.pool.shape[0] - 1)

    def gather(self, length: Optional[int] = None) -> torch.Tensor:
        """Dense (B, Hkv, length, D) copy of the first ``length`` positions
        (default all), built in torch: off the hot path (the CPU oracle, the
        prefill route and tests)."""
        B, Hkv, Smax, D = self.shape
        L = Smax if length is None else int(length)
        if L < 0 or L > Smax:
            raise ValueError(f"PagedKV.gather: length={L} outside the cache "
                             f"(Smax={Smax})")
        page = self.page_size
        nb = -(-L // page)
        pages = self.pool[self._ids()[:, :nb]]        # (B, nb, Hkv, page, D)
        dense = pages.permute(0, 2, 1, 3, 4).reshape(B, Hkv, nb * page, D)
        return dense[:, :, :L]


def _check_pair(k_cache, v_cache, op: str) -> None:
    if not (isinstance(k_cache, PagedKV) and isinstance(v_cache, PagedKV)):
        raise TypeError(f"{op}: k_cache and v_cache must both be PagedKV or "
                        "both be tensors")
    if k_cache.block_table is not v_cache.block_table and not (
            k_cache.block_table.data_ptr() == v_cache.block_table.data_ptr()
            and k_cache.block_table.shape == v_cache.block_table.shape):
        raise ValueError(f"{op}: K and V of one layer share one block table; "
                         "pass the same tensor to both PagedKV")
    if k_cache.pool.shape != v_cache.pool.shape or \
            k_cache.pool.dtype != v_cache.pool.dtype:
        raise ValueError(f"{op}: K and V pools differ: "
                         f"{tuple(k_cache.pool.shape)} {k_cache.pool.dtype}, "
                         f"{tuple(v_cache.pool.shape)} {v_cache.pool.dtype}")


def kv_cache_append(k_cache, v_cache, k: torch.Tensor, v: torch.Tensor,
                    pos0) -> None:
    """Write k, v (B, Hkv, S, D) into the caches at positions
    ``[pos0, pos0+S)``.  ``pos0`` is a host int, or an int64 tensor with 1 or
    B elements read on the device (hipGraph-capturable; clamped to
    ``[0, Smax-S]``).

    :class:`PagedKV` caches are written through their block table: on the
    GPU one launch of the HIP kernel for K and V together (bf16, head dim 64
    or 128, sources with a contiguous last dim, other strides free); on the
    CPU a torch loop.  Anything else is ops.kv_fp8.kv_cache_append
    (:class:`Fp8KV` pairs quantise, tensors take the plain copy).  Mixing
    cache types raises.
    """
    if not (isinstance(k_cache, PagedKV) or isinstance(v_cache, PagedKV)):
        return kv_fp8.kv_cache_append(k_cache, v_cache, k, v, pos0)
    _check_pair(k_cache, v_cache, "kv_cache_append")
    B, Hkv, S, D = k.shape
    Smax = k_cache.shape[2]
    if v.shape != k.shape or k_cache.shape[:2] != (B, Hkv) or \
            k_cache.shape[3] != D:
        raise ValueError("kv_cache_append: shape mismatch between "
                         f"k {tuple(k.shape)}, v {tuple(v.shape)} and caches "
                         f"{tuple(k_cache.shape)}")
    if k.is_cuda:
        if not (k.dtype == v.dtype == k_cache.pool.dtype == torch.bfloat16):
            raise TypeError("kv_cache_append: the GPU kernel moves bf16, got "
                            f"{k.dtype} into {k_cache.pool.dtype}")
        if D not in (64, 128):
            raise ValueError("kv_cache_append: the GPU kernel covers head "
                             f"dim 64 and 128, got {D}")
        e = ext_nopk("kv_cache_append")
        if torch.is_tensor(pos0):
            e.kv_paged_append(k_cache.pool, v_cache.pool,
                              k_cache.block_table, k, v, pos0, 0)
        else:
            pos0 = int(pos0)
            if pos0 < 0 or pos0 + S > Smax:
                raise ValueError(f"kv_cache_append: pos0={pos0} with S={S} "
                                 f"outside the cache (Smax={Smax})")
            e.kv_paged_append(k_cache.pool, v_cache.pool,
                              k_cache.block_table, k, v, None, pos0)
        return
    pos = kv_fp8._positions(pos0, B, Smax, S, k.device)
    page = k_cache.page_size
    ids = k_cache._ids()
    for cache, x in ((k_cache, k), (v_cache, v)):
        x = x.to(cache.pool.dtype)
        for b in range(B):
            for s in range(S):
                p = int(pos[b]) + s
                cache.pool[ids[b, p // page], :, p % page] = x[b, :, s]
