"""Tensor-parallel + Megatron-style sequence-parallel primitives.

Capability parity with the reference tp_utils
(/root/reference/torchdistpackage/parallel/tensor_parallel/tp_utils.py):
module-global TP group get/set, the three collective autograd Functions
(all-reduce fwd / identity bwd; reduce-scatter fwd / all-gather bwd;
all-gather fwd / reduce-scatter bwd), SP tensor tagging
(``tensor.sequence_parallel``), and the Col/Row parallel linear layers with
weight-surgery loaders (incl. interleaved QKV split).

MI355X-first decisions:
- Public collective APIs only: ``all_gather_into_tensor`` /
  ``reduce_scatter_tensor`` (the reference uses torch-private
  ``_all_gather_base``/``_reduce_scatter_base``, tp_utils.py:67,84).
- Weights are stored in nn.Linear orientation (out_features, in_features) and
  GEMMs go through ``torch.nn.functional.linear`` → hipBLASLt picks the
  transpose-free bf16 kernel.  (The reference stores (fin,fout) transposed,
  tp_utils.py:162-174 — an artifact of its x@W formulation, not an API.)
- On gloo (CPU tests) reduce_scatter_tensor is unsupported: collectives fall
  back to all_reduce + local slice, numerics-identical.
- The TP all-reduce in RowParallel backward etc. rides RCCL over xGMI; with
  the 'tensor' axis innermost (adjacent ranks), a TP=2/4/8 group is fully
  connected by direct links.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from ...ops.gemm import linear as fast_linear

_TP_GROUP: Optional[dist.ProcessGroup] = None


def set_tp_group(group: Optional[dist.ProcessGroup]):
    global _TP_GROUP
    _TP_GROUP = group


def get_tp_group() -> Optional[dist.ProcessGroup]:
    global _TP_GROUP
    if _TP_GROUP is None:
        try:
            from ...dist.topo import tpc
            if tpc.is_mode_inited("tensor"):
                _TP_GROUP = tpc.get_group("tensor")
        except Exception:
            pass
    return _TP_GROUP


def get_tp_size() -> int:
    g = get_tp_group()
    return dist.get_world_size(g) if (g is not None and dist.is_initialized()) else 1


def get_tp_rank() -> int:
    g = get_tp_group()
    return dist.get_rank(g) if (g is not None and dist.is_initialized()) else 0


def _backend_is_gloo(group) -> bool:
    try:
        return dist.get_backend(group) == "gloo"
    except Exception:
        return False


# ---------------------------------------------------------------------------
# raw helpers (first-dim sharding, SP convention: dim 0 = sequence)
# ---------------------------------------------------------------------------

def _all_gather_first_dim(x: torch.Tensor) -> torch.Tensor:
    tp = get_tp_size()
    if tp == 1:
        return x
    group = get_tp_group()
    out_shape = list(x.shape)
    out_shape[0] *= tp
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x.contiguous(), group=group)
    return out


def _reduce_scatter_first_dim(x: torch.Tensor) -> torch.Tensor:
    tp = get_tp_size()
    if tp == 1:
        return x
    group = get_tp_group()
    assert x.shape[0] % tp == 0, \
        f"first dim {x.shape[0]} not divisible by tp {tp}"
    out_shape = list(x.shape)
    out_shape[0] //= tp
    x = x.contiguous()
    if _backend_is_gloo(group):
        # clone: all_reduce mutates in place, and backward inputs (incoming
        # grads) must never be mutated — they may be shared by other consumers
        x = x.clone()
        dist.all_reduce(x, group=group)
        r = dist.get_rank(group)
        return x.narrow(0, r * out_shape[0], out_shape[0]).clone()
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    dist.reduce_scatter_tensor(out, x, group=group)
    return out


def _split_first_dim(x: torch.Tensor) -> torch.Tensor:
    tp = get_tp_size()
    if tp == 1:
        return x
    r = get_tp_rank()
    n = x.shape[0] // tp
    return x.narrow(0, r * n, n).contiguous()


def _all_reduce(x: torch.Tensor) -> torch.Tensor:
    if get_tp_size() == 1:
        return x
    dist.all_reduce(x, group=get_tp_group())
    return x


# ---------------------------------------------------------------------------
# autograd collective functions (reference tp_utils.py:39-149)
# ---------------------------------------------------------------------------

class _ReduceFromTp(torch.autograd.Function):
    """fwd: all-reduce over TP; bwd: identity (RowParallel output)."""

    @staticmethod
    def forward(ctx, x):
        # TP size 1: the all-reduce is the identity and nothing is mutated,
        # so the input goes through (a clone here was a pure 2-pass copy of
        # every Row-parallel output)
        if get_tp_size() == 1:
            return x
        return _all_reduce(x.clone())

    @staticmethod
    def backward(ctx, grad):
        return grad


class _CopyToTp(torch.autograd.Function):
    """fwd: identity; bwd: all-reduce (ColParallel input)."""

    @staticmethod
    def forward(ctx, x):
        return x

    @staticmethod
    def backward(ctx, grad):
        if get_tp_size() == 1:
            return grad
        # clone: never mutate the incoming grad in place (all_reduce would)
        return _all_reduce(grad.contiguous().clone())


class _ReduceScatterToSp(torch.autograd.Function):
    """fwd: reduce-scatter along seq(first) dim; bwd: all-gather."""

    @staticmethod
    def forward(ctx, x):
        return _reduce_scatter_first_dim(x)

    @staticmethod
    def backward(ctx, grad):
        return _all_gather_first_dim(grad.contiguous())


class _GatherFromSp(torch.autograd.Function):
    """fwd: all-gather along seq dim; bwd: reduce-scatter (or plain split if
    the forward input was a pure shard copy, tensor_already_summed)."""

    @staticmethod
    def forward(ctx, x, bwd_mode: str = "reduce_scatter"):
        ctx.bwd_mode = bwd_mode
        return _all_gather_first_dim(x)

    @staticmethod
    def backward(ctx, grad):
        grad = grad.contiguous()
        if ctx.bwd_mode == "split":
            return _split_first_dim(grad), None
        return _reduce_scatter_first_dim(grad), None


def reduce_from_tp_region(x):
    return _ReduceFromTp.apply(x)


def copy_to_tp_region(x):
    return _CopyToTp.apply(x)


def reduce_scatter_to_sequence_parallel_region(x):
    out = _ReduceScatterToSp.apply(x)
    set_sequence_parallel_attr(out)
    return out


def gather_from_sequence_parallel_region(x, bwd_mode: str = "reduce_scatter"):
    return _GatherFromSp.apply(x, bwd_mode)


# ---------------------------------------------------------------------------
# SP tagging (reference tp_utils.py:20-35)
# ---------------------------------------------------------------------------

def set_sequence_parallel_attr(t: torch.Tensor):
    t.sequence_parallel = True


def is_sequence_parallel(t: torch.Tensor) -> bool:
    return getattr(t, "sequence_parallel", False)


def maybe_gather_for_sequence_parallel(t: torch.Tensor) -> torch.Tensor:
    if is_sequence_parallel(t):
        return gather_from_sequence_parallel_region(t)
    return t


def maybe_split_into_sequence_parallel(t: torch.Tensor) -> torch.Tensor:
    """Slice the local sequence shard out of a replicated tensor (first SP
    entry point).  Backward = all-gather (handled by autograd fn)."""
    if get_tp_size() == 1 or is_sequence_parallel(t):
        return t
    out = _SplitToSp.apply(t)
    set_sequence_parallel_attr(out)
    return out


class _SplitToSp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _split_first_dim(x)

    @staticmethod
    def backward(ctx, grad):
        return _all_gather_first_dim(grad.contiguous())


class _GatherLastDim(torch.autograd.Function):
    """fwd: all-gather along the LAST dim (ColParallel gather_output);
    bwd: take the local slice."""

    @staticmethod
    def forward(ctx, x):
        tp = get_tp_size()
        if tp == 1:
            return x
        xs = [torch.empty_like(x) for _ in range(tp)]
        dist.all_gather(xs, x.contiguous(), group=get_tp_group())
        return torch.cat(xs, dim=-1)

    @staticmethod
    def backward(ctx, grad):
        tp = get_tp_size()
        if tp == 1:
            return grad
        n = grad.shape[-1] // tp
        return grad.narrow(-1, get_tp_rank() * n, n).contiguous()


# ---------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------

class TpLinear(nn.Module):
    """Plain linear with nn.Linear weight orientation; base for Col/Row."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 device=None, dtype=None):
        super().__init__()
        kw = {"device": device, "dtype": dtype}
        self.in_features = in_features
        self.out_features = out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, **kw))
        self.bias = nn.Parameter(torch.empty(out_features, **kw)) if bias \
            else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.normal_(self.weight, std=0.02)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x):
        return fast_linear(x, self.weight, self.bias)


class ColParallelLinear(TpLinear):
    """Column-parallel: splits out_features over TP; no fwd comm (input is
    replicated or gathered-from-SP); bwd all-reduces the input grad.

    Reference: tp_utils.py:176-216.
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 gather_output: bool = False, device=None, dtype=None):
        tp = get_tp_size()
        assert out_features % tp == 0, (out_features, tp)
        self.full_out_features = out_features
        self.gather_output = gather_output
        super().__init__(in_features, out_features // tp, bias=bias,
                         device=device, dtype=dtype)

    def forward(self, x):
        x = copy_to_tp_region(x)
        out = fast_linear(x, self.weight, self.bias)
        if self.gather_output and get_tp_size() > 1:
            out = _GatherLastDim.apply(out)
        return out

    @torch.no_grad()
    def init_weight_from_full(self, full_weight: torch.Tensor,
                              full_bias: Optional[torch.Tensor] = None):
        """Load this rank's row-slice of a full (out, in) weight."""
        tp, r = get_tp_size(), get_tp_rank()
        shard = full_weight.chunk(tp, dim=0)[r]
        self.weight.copy_(shard)
        if full_bias is not None and self.bias is not None:
            self.bias.copy_(full_bias.chunk(tp, dim=0)[r])

    @torch.no_grad()
    def init_qkv_weight_from_full(self, full_weight: torch.Tensor,
                                  full_bias: Optional[torch.Tensor] = None,
                                  num_splits: int = 3):
        """Load from a full interleaved QKV weight (3*dim, in): each TP rank
        takes its slice of each of Q, K, V so heads stay contiguous per rank.
        Reference: tp_utils.py:195-216."""
        tp, r = get_tp_size(), get_tp_rank()
        chunks = full_weight.chunk(num_splits, dim=0)
        mine = torch.cat([c.chunk(tp, dim=0)[r] for c in chunks], dim=0)
        self.weight.copy_(mine)
        if full_bias is not None and self.bias is not None:
            bchunks = full_bias.chunk(num_splits, dim=0)
            self.bias.copy_(
                torch.cat([c.chunk(tp, dim=0)[r] for c in bchunks], dim=0))


class RowParallelLinear(TpLinear):
    """Row-parallel: splits in_features over TP; fwd ends in all-reduce (or
    reduce-scatter into SP when ``sequence_parallel``).

    Reference: tp_utils.py:218-248.
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 sequence_parallel: bool = False, device=None, dtype=None):
        tp = get_tp_size()
        assert in_features % tp == 0, (in_features, tp)
        self.full_in_features = in_features
        self.sequence_parallel = sequence_parallel
        super().__init__(in_features // tp, out_features, bias=bias,
                         device=device, dtype=dtype)

    def forward(self, x, skip_bias: bool = False):
        # bias added once, after the reduction (not per-rank!); with
        # ``skip_bias`` the caller adds it (ParallelBlock folds it into the
        # residual kernel that reads this output next)
        out = fast_linear(x, self.weight)
        if self.sequence_parallel and get_tp_size() > 1:
            out = reduce_scatter_to_sequence_parallel_region(out)
        else:
            out = reduce_from_tp_region(out)
        if self.bias is not None and not skip_bias:
            out = out + self.bias
        return out

    @torch.no_grad()
    def init_weight_from_full(self, full_weight: torch.Tensor,
                              full_bias: Optional[torch.Tensor] = None):
        tp, r = get_tp_size(), get_tp_rank()
        shard = full_weight.chunk(tp, dim=1)[r]
        self.weight.copy_(shard)
        if full_bias is not None and self.bias is not None:
            self.bias.copy_(full_bias)


def mark_sequence_parallel_params(module: "nn.Module"):
    """Tag a module's params as SP-region params (grads computed from the
    local sequence shard only -> need an all-reduce over TP)."""
    for p in module.parameters():
        p.sequence_parallel_param = True


def allreduce_sequence_parallel_grads(module: "nn.Module"):
    """All-reduce the grads of SP-region params (LayerNorm weights/biases
    inside ParallelBlock) over the TP group.  Must be called once per
    iteration after backward when sequence_parallel is on — Megatron-SP
    semantics the reference does not implement (its transformer tolerates
    rtol=1e-1, test_transformer.py:33-39)."""
    if get_tp_size() == 1:
        return
    group = get_tp_group()
    grads = [p.grad for p in module.parameters()
             if getattr(p, "sequence_parallel_param", False)
             and p.grad is not None]
    if not grads:
        return
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, group=group)
    off = 0
    for g in grads:
        g.copy_(flat[off:off + g.numel()].view_as(g))
        off += g.numel()


# --------------------------------------------------------------------------
# Migration aliases for users of the reference package (tp_utils.py there
# exposes these names; ``is_squence_parallel_tensor`` keeps the reference's
# spelling so ported code imports unchanged).
# --------------------------------------------------------------------------

get_tensor_model_parallel_world_size = get_tp_size
maybe_gather_from_sequence_parallel = maybe_gather_for_sequence_parallel
is_squence_parallel_tensor = is_sequence_parallel
