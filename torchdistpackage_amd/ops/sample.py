"""Fused temperature / top-k / top-p sampling (csrc/sample.hip).

``sample_logits(logits, u, temperature, top_k, top_p, out) -> (B,) int64``
draws one token per row of ``logits`` from the uniform numbers ``u`` the
caller supplies: the op holds no random number generator, so it is a pure
function of its inputs.  Per row:

1. ``T = max(temperature, 1e-5)``, ``z = x / T``.
2. top-k: K = the k largest ``x``, ties at the k-th value to the lower index.
3. top-p: K ordered by (``x`` descending, index ascending), ``p`` the softmax
   of ``z`` over K; N = the shortest prefix with mass >= ``top_p`` (at least
   one token).
4. draw: over N in ascending token index, ``C_i`` the running sum of
   ``exp(z_i - z_max)``; the first ``i`` with ``C_i > u * C_last``, or the
   last kept index if there is none.

``top_k`` of None, <= 0 or >= V and ``top_p`` of None or >= 1 keep everything.

Dispatch:
- CPU tensors: exactly the steps above in fp64 torch (the numerics oracle).
- GPU tensors: the HIP kernel, one launch, no host synchronisation; the
  parameters are read from device memory per row, so a captured launch stays
  valid when the host rewrites them between replays.
"""

from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import ext

Param = Union[None, int, float, torch.Tensor]


def _param(v: Param, default, dtype, B, device, name) -> torch.Tensor:
    if v is None:
        v = default
    if not isinstance(v, torch.Tensor):
        return torch.full((B,), v, dtype=dtype, device=device)
    if v.dtype != dtype:
        raise TypeError(f"sample_logits: a {name} tensor must be {dtype}, "
                        f"got {v.dtype}")
    if tuple(v.shape) != (B,) or v.device != device:
        raise ValueError(f"sample_logits: a {name} tensor must be ({B},) on "
                         f"{device}, got {tuple(v.shape)} on {v.device}")
    return v.contiguous()


def _kept_ref(logits, temperature, top_k, top_p) -> Tuple[torch.Tensor,
                                                          torch.Tensor]:
    """(kept (B, V) bool, weights exp(z - z_max) (B, V) fp64): steps 1-3."""
    B, V = logits.shape
    x = logits.double()
    z = x / temperature.double().clamp_min(1e-5)[:, None]
    _, order = torch.sort(x, dim=-1, descending=True, stable=True)
    zs = z.gather(1, order)
    w = torch.exp(z - zs[:, :1])
    k = top_k.long()
    k = torch.where((k <= 0) | (k >= V), torch.full_like(k, V), k)
    rank = torch.arange(V)[None, :]
    ws = torch.where(rank < k[:, None], w.gather(1, order), 0.0)
    cum = ws.cumsum(-1)
    p = top_p.double()
    n = ((cum / cum[:, -1:]) < p[:, None]).sum(-1) + 1
    n = torch.where(p >= 1, k, torch.minimum(n, k))
    kept = torch.zeros(B, V, dtype=torch.bool)
    kept.scatter_(1, order, rank < n[:, None])
    return kept, w


def _sample_ref(logits, u, temperature, top_k, top_p) -> torch.Tensor:
    kept, w = _kept_ref(logits, temperature, top_k, top_p)
    V = logits.shape[1]
    C = torch.where(kept, w, 0.0).cumsum(-1)
    hit = C > u.double()[:, None] * C[:, -1:]
    first = hit.to(torch.uint8).argmax(-1)
    last = V - 1 - kept.flip(-1).to(torch.uint8).argmax(-1)
    return torch.where(hit.any(-1), first, last)


def sample_logits(logits: torch.Tensor, u: torch.Tensor,
                  temperature: Param = 1.0, top_k: Param = None,
                  top_p: Param = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits (B, V) bf16/fp32 with ``stride(-1) == 1`` (any row stride), u
    (B,) fp32 in [0, 1) -> (B,) int64 token ids.  ``temperature`` / ``top_k``
    / ``top_p``: a Python scalar or a (B,) fp32 / int32 / fp32 tensor on the
    logits' device.  ``out``: an optional (B,) or (B, 1) contiguous int64
    tensor to write into (the return value is its (B,) view)."""
    if logits.dim() != 2:
        raise ValueError("sample_logits: logits must be (B, V), got "
                         f"{tuple(logits.shape)}")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("sample_logits: logits must be bf16 or fp32, got "
                        f"{logits.dtype}")
    B, V = logits.shape
    if V < 1 or (V > 1 and logits.stride(1) != 1):
        raise ValueError("sample_logits: logits need V >= 1 and "
                         f"stride(-1) == 1, got strides {logits.stride()}")
    dev = logits.device
    if not isinstance(u, torch.Tensor):
        raise TypeError("sample_logits: u must be a (B,) fp32 tensor")
    u = _param(u, None, torch.float32, B, dev, "u")
    t = _param(temperature, 1.0, torch.float32, B, dev, "temperature")
    k = _param(top_k, 0, torch.int32, B, dev, "top_k")
    p = _param(top_p, 1.0, torch.float32, B, dev, "top_p")
    if out is not None:
        if out.dtype != torch.int64 or out.device != dev or \
                tuple(out.shape) not in ((B,), (B, 1)) or \
                not out.is_contiguous():
            raise ValueError(f"sample_logits: out must be a contiguous ({B},)"
                             f" or ({B}, 1) int64 tensor on {dev}")
        out = out.view(B)
    if logits.is_cuda:
        if out is None:
            out = torch.empty(B, dtype=torch.int64, device=dev)
        return ext("sample_logits").sample_logits(logits.detach(), u, t, k, p,
                                                  out)
    tok = _sample_ref(logits.detach(), u, t, k, p)
    return tok if out is None else out.copy_(tok)
