"""Fused MoE token routing (csrc/moe_route.hip).

Three ops around one index, ``dest[t, j]``: the row of routing entry
``(t, j)`` in the token buffer sorted by expert.

- ``moe_route_plan(topk_idx, num_experts) -> (dest, counts, offs)``: a stable
  counting sort of the (N, k) expert ids.  ``dest.flatten()`` is the inverse
  permutation of ``argsort(topk_idx.flatten(), stable=True)``, ``counts`` is
  the ``bincount`` and ``offs`` the zero-padded ``cumsum``
  (``grouped_linear``'s segment table).
- ``moe_dispatch(x, dest) -> (N*k, D)``: ``out[dest[t, j]] = x[t]``.
- ``moe_combine(y, dest, gates) -> (N, D)``:
  ``out[t] = round(sum_j gates[t, j] * float(y[dest[t, j]]))``, ascending j,
  fp32 accumulation, one rounding.

Dispatch:
- CPU tensors of any float dtype: the plain torch formulas below, fp32 math
  for bf16/fp16 and one rounding (the numerics oracle); the plan is a stable
  ``argsort``.
- GPU bf16 token buffers with ``D % 8 == 0``, 16-byte aligned: the HIP
  kernels.  Nothing reads device data on the host, so all three ops capture
  into a hipGraph.
- any other GPU token buffer: the same torch formulas on the device,
  announced once.  The plan always runs its kernel on the GPU.

Expert ids are clamped to ``[0, E-1]`` and ``dest`` values to
``[0, N*k-1]`` before they index anything: a stale index gives a wrong
answer, never an access outside the buffers.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ext

# routing entries per workgroup of the plan kernels (csrc/moe_route.h; the
# extension exports the same number as ``MOE_PLAN_CHUNK``): N*k at or below
# it takes the single-launch plan
MOE_PLAN_CHUNK = 2048
MOE_ROUTE_MAX_K = 8
MOE_ROUTE_MAX_E = 256


def moe_route_eligible(D: int, dtype: torch.dtype) -> bool:
    """True when GPU token buffers of this width/dtype run the row kernels."""
    return dtype == torch.bfloat16 and D > 0 and D % 8 == 0


def _check_dest(dest, what):
    if dest.dim() != 2 or not 1 <= dest.shape[1] <= MOE_ROUTE_MAX_K:
        raise ValueError(f"{what}: dest must be (N, k) with 1 <= k <= "
                         f"{MOE_ROUTE_MAX_K}, got {tuple(dest.shape)}")
    if dest.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: dest must be int32 or int64, got "
                        f"{dest.dtype}")


def moe_route_plan(topk_idx: torch.Tensor, num_experts: int):
    """topk_idx (N, k) int32/int64 -> (dest (N, k) int32, counts (E,) int64,
    offs (E+1,) int64).  No grad."""
    if topk_idx.dim() != 2 or \
            topk_idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("moe_route_plan: topk_idx must be an (N, k) int32 or "
                         f"int64 tensor, got {tuple(topk_idx.shape)} "
                         f"{topk_idx.dtype}")
    N, k = topk_idx.shape
    E = int(num_experts)
    if not 1 <= k <= MOE_ROUTE_MAX_K:
        raise ValueError(f"moe_route_plan: k={k} outside 1..{MOE_ROUTE_MAX_K}")
    if not 1 <= E <= MOE_ROUTE_MAX_E:
        raise ValueError(f"moe_route_plan: num_experts={E} outside "
                         f"1..{MOE_ROUTE_MAX_E}")
    if N * k >= 2 ** 31:
        raise ValueError(f"moe_route_plan: N*k={N * k} must stay below 2^31")
    topk_idx = topk_idx.detach()
    if topk_idx.is_cuda:
        return ext("moe_route_plan").moe_route_plan(topk_idx.contiguous(), E)
    flat = topk_idx.reshape(-1).long().clamp(0, E - 1)
    order = torch.argsort(flat, stable=True)
    dest = torch.empty(N * k, dtype=torch.int32)
    dest[order] = torch.arange(N * k, dtype=torch.int32)
    counts = torch.bincount(flat, minlength=E)
    return dest.view(N, k), counts, F.pad(torch.cumsum(counts, 0), (1, 0))


# ------------------------------------------------------------ torch formulas

def _ctype(t):
    return torch.float32 if t.dtype in (torch.bfloat16, torch.float16) \
        else t.dtype


def _rows(dest):
    """dest (N, k) clamped into the N*k-row buffer, as int64."""
    return dest.long().clamp(0, max(dest.numel() - 1, 0))


def _scatter_ref(x, dest, gates):
    """out[dest[t, j]] = round(gates[t, j] * x[t])."""
    N, k = dest.shape
    out = torch.empty(N * k, x.shape[1], dtype=x.dtype, device=x.device)
    if gates is None:
        src = x[:, None, :].expand(N, k, x.shape[1])
    else:
        ct = _ctype(x)
        src = (gates.to(ct)[:, :, None] * x.to(ct)[:, None, :]).to(x.dtype)
    out[_rows(dest).reshape(-1)] = src.reshape(N * k, -1)
    return out


def _gather_ref(y, dest, gates):
    """out[t] = round(sum_j gates[t, j] * y[dest[t, j]]), ascending j."""
    ct = _ctype(y)
    rows, yf = _rows(dest), y.to(ct)
    acc = None
    for j in range(dest.shape[1]):
        term = yf[rows[:, j]]
        if gates is not None:
            term = gates[:, j, None].to(ct) * term
        acc = term if acc is None else acc + term
    return acc.to(y.dtype)


def _dgates_ref(dout, y, dest):
    """dgates[t, j] = sum_d dout[t, d] * y[dest[t, j], d]."""
    ct = _ctype(y)
    return (dout.to(ct)[:, None, :] * y.to(ct)[_rows(dest)]).sum(-1)


_announced = set()


def _use_kernels(what, *bufs):
    """True: the HIP row kernels; False: the torch formulas (CPU, or a GPU
    buffer the kernels do not read — announced once per reason)."""
    t0 = bufs[0]
    if not t0.is_cuda:
        return False
    e = ext(what)        # a GPU call without the extension raises
    del e
    if all(moe_route_eligible(t.shape[-1], t.dtype) and
           t.data_ptr() % 16 == 0 for t in bufs):
        return True
    key = (what, t0.dtype, t0.shape[-1] % 8 == 0)
    if key not in _announced:
        _announced.add(key)
        print(f"[tdpa.ops] {what}: no HIP kernel for {t0.dtype} rows of "
              f"width {t0.shape[-1]} (bf16, D % 8 == 0, 16-byte aligned do); "
              "using the torch composition for them")
    return False


def _scatter(x, dest, gates, y, what):
    """(out, dgates or None) on either path."""
    x = x.contiguous()
    bufs = (x,) if y is None else (x, y.contiguous())
    if _use_kernels(what, *bufs):
        return ext(what).moe_route_scatter(
            x, dest.int().contiguous(),
            None if gates is None else gates.float().contiguous(),
            None if y is None else bufs[1])
    dg = None if y is None else _dgates_ref(x, y, dest)
    return _scatter_ref(x, dest, gates), dg


def _gather(y, dest, gates, what):
    y = y.contiguous()
    if _use_kernels(what, y):
        return ext(what).moe_route_gather(
            y, dest.int().contiguous(),
            None if gates is None else gates.float().contiguous())
    return _gather_ref(y, dest, gates)


class _DispatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dest):
        ctx.save_for_backward(dest)
        return _scatter(x, dest, None, None, "moe_dispatch")[0]

    @staticmethod
    def backward(ctx, dout):
        dest, = ctx.saved_tensors
        return _gather(dout, dest, None, "moe_dispatch"), None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, dest, gates):
        ctx.save_for_backward(y, dest, gates)
        return _gather(y, dest, gates, "moe_combine")

    @staticmethod
    def backward(ctx, dout):
        y, dest, gates = ctx.saved_tensors
        want_dg = gates is not None and ctx.needs_input_grad[2]
        dy, dg = _scatter(dout, dest, gates, y if want_dg else None,
                          "moe_combine")
        if not ctx.needs_input_grad[0]:
            dy = None
        return dy, None, dg.to(gates.dtype) if want_dg else None


def _check_rows(buf, rows, dest, what, name):
    if buf.dim() != 2 or buf.shape[0] != rows:
        raise ValueError(f"{what}: {name} must be ({rows}, D) for dest "
                         f"{tuple(dest.shape)}, got {tuple(buf.shape)}")
    if not buf.is_floating_point():
        raise TypeError(f"{what}: {name} must be a float tensor, got "
                        f"{buf.dtype}")
    if dest.device != buf.device:
        raise ValueError(f"{what}: dest is on {dest.device}, {name} on "
                         f"{buf.device}")


def moe_dispatch(x: torch.Tensor, dest: torch.Tensor) -> torch.Tensor:
    """x (N, D), dest (N, k) -> (N*k, D) with ``out[dest[t, j]] = x[t]``.
    Differentiable in x: ``dx[t] = round(sum_j float(dout[dest[t, j]]))``."""
    _check_dest(dest, "moe_dispatch")
    _check_rows(x, dest.shape[0], dest, "moe_dispatch", "x")
    return _DispatchFn.apply(x, dest)


def moe_combine(y: torch.Tensor, dest: torch.Tensor,
                gates: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y (N*k, D), dest (N, k), gates (N, k) fp32 or None (unit gates) ->
    (N, D) with ``out[t] = round(sum_j gates[t, j] * float(y[dest[t, j]]))``.
    Differentiable in y (``dy[dest[t, j]] = round(gates[t, j] *
    float(dout[t]))``) and gates (``dgates[t, j] = dout[t] . y[dest[t, j]]``
    in fp32, formed in the pass that writes dy)."""
    _check_dest(dest, "moe_combine")
    _check_rows(y, dest.numel(), dest, "moe_combine", "y")
    if gates is not None and (tuple(gates.shape) != tuple(dest.shape)
                              or not gates.is_floating_point()):
        raise ValueError(f"moe_combine: gates must be a float "
                         f"{tuple(dest.shape)} tensor, got "
                         f"{tuple(gates.shape)} {gates.dtype}")
    return _CombineFn.apply(y, dest, gates)
