"""Fused MoE token routing on the CPU: the reference ops (the oracle of
tests/test_moe_route_gpu.py) against the torch chain they replace, the layer
with route="fused" against route="torch", and the MoEConfig.route_impl
switch.
"""

import copy

import pytest
import torch
import torch.nn.functional as F

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh
from tests.dist_helpers import run_distributed
from torchdistpackage_amd.moe import ExpertParallelMoE


def _ids(N, k, E, tag):
    g = nh._gen("moe-route-ids", tag, N, k, E)
    return torch.stack([torch.randperm(E, generator=g)[:k]
                        for _ in range(N)])


@pytest.mark.parametrize("N,k,E,dtype", [(1, 1, 3, torch.int64),
                                         (37, 2, 8, torch.int32),
                                         (300, 4, 8, torch.int64)])
def test_plan_ref_vs_argsort(N, k, E, dtype):
    idx = _ids(N, k, E, "plan").to(dtype)
    dest, counts, offs = ops.moe_route_plan(idx, E)
    order = torch.argsort(idx.flatten().long(), stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(N * k)
    assert dest.dtype == torch.int32 and dest.shape == (N, k)
    assert torch.equal(dest.flatten().long(), inv)
    want = torch.bincount(idx.flatten().long(), minlength=E)
    assert counts.dtype == offs.dtype == torch.int64
    assert torch.equal(counts, want)
    assert torch.equal(offs, F.pad(torch.cumsum(want, 0), (1, 0)))


def test_plan_limits_and_clamp():
    idx = torch.zeros(4, 2, dtype=torch.int64)
    for bad_k in (0, 9):
        with pytest.raises(ValueError):
            ops.moe_route_plan(torch.zeros(4, bad_k, dtype=torch.int64), 4)
    for bad_e in (0, 257):
        with pytest.raises(ValueError):
            ops.moe_route_plan(idx, bad_e)
    with pytest.raises(ValueError):
        ops.moe_route_plan(idx.float(), 4)
    # ids outside [0, E-1] are clamped, not indexed with
    _, counts, _ = ops.moe_route_plan(torch.tensor([[-5, 99]]), 4)
    assert counts.tolist() == [1, 0, 0, 1]


def torch_chain(x, y, gates, order, k, dout_d, dout_c, dt, device):
    """The chain the ops replace, forward and backward in dtype ``dt``:
    [x[token_of], index_add_ of y * gates, dx, dy, dgates (if gates)]."""
    def leaf(t, dtype):
        return t.detach().to(device=device, dtype=dtype).clone() \
            .requires_grad_(True)
    order = order.to(device)
    token_of = order // k
    x, y = leaf(x, dt), leaf(y, dt)
    ins = [x, y]
    disp = x[token_of]
    prod = y
    if gates is not None:
        gates = leaf(gates, gates.dtype)
        ins.append(gates)
        prod = y * gates.reshape(-1)[order].to(dt).unsqueeze(-1)
    comb = torch.zeros_like(x).index_add_(0, token_of, prod)
    disp.backward(dout_d.to(device=device, dtype=dt))
    comb.backward(dout_c.to(device=device, dtype=dt))
    return [disp.detach(), comb.detach()] + [i.grad for i in ins]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gated", [True, False])
def test_dispatch_combine_ref_vs_torch_chain(dtype, gated):
    """fp32: bit-equal to xt[token_of] / index_add_ at k = 2 (two addends
    commute).  bf16: fp32 accumulation and one rounding, so the yardstick
    against fp64 with the bf16 chain as the library arm."""
    N, k, E, D = 33, 2, 4, 24
    g = nh._gen("moe-route-ref", dtype, gated)
    idx = _ids(N, k, E, "ref")
    dest, _, _ = ops.moe_route_plan(idx, E)
    order = torch.argsort(idx.flatten(), stable=True)
    x = nh._randn((N, D), g).to(dtype)
    y = nh._randn((N * k, D), g).to(dtype)
    gates = torch.rand((N, k), generator=g) if gated else None
    dout_d = nh._randn((N * k, D), g).to(dtype)
    dout_c = nh._randn((N, D), g).to(dtype)

    def chain(dt):
        return torch_chain(x, y, gates, order, k, dout_d, dout_c, dt, "cpu")

    x1 = x.clone().requires_grad_(True)
    y1 = y.clone().requires_grad_(True)
    g1 = gates.clone().requires_grad_(True) if gated else None
    disp = ops.moe_dispatch(x1, dest)
    comb = ops.moe_combine(y1, dest, g1)
    disp.backward(dout_d)
    comb.backward(dout_c)
    got = [disp.detach(), comb.detach(), x1.grad, y1.grad] + \
        ([g1.grad] if gated else [])
    names = ["dispatch", "combine", "dx", "dy", "dgates"]
    lib = chain(dtype)
    nh.check_equal(got[0], lib[0], "dispatch")
    if dtype == torch.float32:
        for n, a, b in zip(names, got, lib):
            nh.check_equal(a, b, n)
        return
    ref = chain(torch.float64)
    f_fwd, f_grad = nh.floors(dtype)
    for n, a, r, b in zip(names[1:], got[1:], ref[1:], lib[1:]):
        nh.yardstick(a, r, b, f_fwd if n == "combine" else f_grad,
                     what=f"ref {n}")


def _layers(k, grouped, seed=21, dim=32, E=4):
    """(route="torch" layer, route="fused" layer) with the same weights."""
    torch.manual_seed(seed)
    a = ExpertParallelMoE(dim, E, k, 2, ep_group=None, grouped=grouped)
    b = ExpertParallelMoE(dim, E, k, 2, ep_group=None, grouped=grouped,
                          route="fused")
    b.load_state_dict(a.state_dict())
    return a, b


def _run(layer, x, dy):
    x = x.detach().clone().requires_grad_(True)
    y = layer(x)
    y.backward(dy.to(y.dtype))
    return [y.detach(), x.grad] + [
        p.grad if p.grad is not None else torch.zeros_like(p)
        for p in layer.parameters()]


@pytest.mark.parametrize("grouped", [False, True], ids=["loop", "grouped"])
def test_layer_fused_equals_torch_k2(grouped):
    a, b = _layers(2, grouped)
    assert a.route == "torch" and b.route == "fused"
    g = nh._gen("moe-route-layer", grouped)
    x = nh._randn((5, 9, 32), g).float()
    dy = nh._randn((5, 9, 32), g).float()
    for i, (p, q) in enumerate(zip(_run(a, x, dy), _run(b, x, dy))):
        nh.check_equal(q, p, f"k=2 fused vs torch, tensor {i}")


def test_layer_k4_vs_fp64():
    a, b = _layers(4, True, E=8)
    ref = copy.deepcopy(a)
    ref.experts_g.double()            # the router is fp32 in every run
    g = nh._gen("moe-route-layer-k4")
    x = nh._randn((40, 32), g).float()
    dy = nh._randn((40, 32), g).float()
    r_ref = _run(ref, x.double(), dy)
    r_a, r_b = _run(a, x, dy), _run(b, x, dy)
    floor = nh.floors(torch.float32)[0]
    for i, (r, p, q) in enumerate(zip(r_ref, r_a, r_b)):
        # each route with the other as the library arm
        nh.yardstick(q, r, p, floor, what=f"k=4 fused, tensor {i}")
        nh.yardstick(p, r, q, floor, what=f"k=4 torch, tensor {i}")


def _fused_ep2(rank, world_size):
    from torchdistpackage_amd.dist.topo import tpc

    tpc.setup_process_groups([("data", world_size)])
    tpc.build_moe_groups(moe_dp_size=1, moe_ep_size=world_size)
    group = tpc.get_group("moe_ep")
    for grouped in (False, True):
        torch.manual_seed(3)
        a = ExpertParallelMoE(32, 4, 2, 2, ep_group=group, grouped=grouped)
        b = ExpertParallelMoE(32, 4, 2, 2, ep_group=group, grouped=grouped,
                              route="fused")
        b.load_state_dict(a.state_dict())
        assert a.ep_size == 2 and b.num_local == 2
        g = nh._gen("moe-route-ep2", rank)
        x = nh._randn((11, 32), g).float()
        dy = nh._randn((11, 32), g).float()
        for i, (p, q) in enumerate(zip(_run(a, x, dy), _run(b, x, dy))):
            nh.check_equal(q, p, f"EP=2 rank {rank} grouped={grouped}, "
                                 f"tensor {i}")
    return True


def test_layer_fused_equals_torch_ep2():
    run_distributed(_fused_ep2, world_size=2)


def test_route_impl_config(monkeypatch):
    from torchdistpackage_amd.models.moe_model import MoEConfig, MoEModel

    monkeypatch.delenv("TDPA_MOE_ROUTE", raising=False)
    assert MoEConfig().route_impl == "torch"
    monkeypatch.setenv("TDPA_MOE_ROUTE", "fused")
    assert MoEConfig().route_impl == "fused"
    assert MoEConfig(route_impl="torch").route_impl == "torch"
    monkeypatch.setenv("TDPA_MOE_ROUTE", "nonsense")
    with pytest.raises(ValueError):
        MoEConfig()
    with pytest.raises(ValueError):
        ExpertParallelMoE(16, 4, ep_group=None, route="nonsense")

    kw = dict(vocab_size=128, n_layer=1, n_head=2, dim=32, max_seq=16,
              num_experts=4, top_k=2, hidden_mult=2)
    x = torch.randint(0, 128, (2, 16), generator=nh._gen("route-cfg"))
    for impl in ("loop", "batched", "grouped"):
        m = MoEModel(MoEConfig(expert_impl=impl, route_impl="fused", **kw))
        assert m.blocks[0].moe.route == "fused"
        out = m(x, labels=x)
        out["loss"].backward()
        assert torch.isfinite(out["loss"])
        for p in m.expert_parameters():
            assert p.grad is not None
