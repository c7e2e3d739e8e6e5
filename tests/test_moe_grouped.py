"""ExpertParallelMoE(grouped=True) on the CPU: parity with the per-expert
loop path, empty experts, expert parallelism over gloo, and the
MoEConfig.expert_impl switch.  The GPU kernels behind grouped=True are
covered by tests/test_grouped_gemm_gpu.py and tests/test_moe_grouped_gpu.py.
"""

import pytest
import torch

from tests.dist_helpers import run_distributed
from tests.test_moe import _dense_oracle
from torchdistpackage_amd.moe import ExpertParallelMoE, GroupedExperts
from torchdistpackage_amd.moe.layer import Expert


def _pair(dim=32, E=4, top_k=2, mult=2, seed=13):
    """(loop layer, grouped layer) with identical weights and router."""
    torch.manual_seed(seed)
    a = ExpertParallelMoE(dim, num_experts=E, top_k=top_k, hidden_mult=mult,
                          ep_group=None, grouped=False)
    b = ExpertParallelMoE(dim, num_experts=E, top_k=top_k, hidden_mult=mult,
                          ep_group=None, grouped=True)
    with torch.no_grad():
        for ex in a.experts:         # non-zero biases: the epilogue bias path
            ex.fc1.bias.normal_(std=0.1)
            ex.fc2.bias.normal_(std=0.1)
        b.router.gate.weight.copy_(a.router.gate.weight)
    b.experts_g.load_from_experts(a.experts)
    return a, b


def _check_expert_grads(a, b, atol):
    eg = b.experts_g
    for e, ex in enumerate(a.experts):
        pairs = [(eg.w1.grad[e], ex.fc1.weight.grad),
                 (eg.b1.grad[e], ex.fc1.bias.grad),
                 (eg.w2.grad[e], ex.fc2.weight.grad),
                 (eg.b2.grad[e], ex.fc2.bias.grad)]
        for got, want in pairs:
            if want is None:         # the loop path skips an empty expert
                assert not got.any(), e
            else:
                assert torch.allclose(got, want, atol=atol), \
                    (e, (got - want).abs().max().item())


def test_grouped_experts_parity():
    """grouped=True vs the per-expert ModuleList path in fp32, at the
    tolerance of test_batched_experts_parity."""
    a, b = _pair()
    assert b.grouped and not b.batched and not hasattr(b, "experts")
    x = torch.randn(6, 5, 32, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    ya, yb = a(x), b(x2)
    assert torch.allclose(ya, yb, atol=1e-5), (ya - yb).abs().max()
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    assert torch.allclose(x.grad, x2.grad, atol=1e-5)
    _check_expert_grads(a, b, 1e-5)
    for p in b.experts_g.parameters():
        assert p.expert_parallel


def test_grouped_empty_expert():
    """Routing that leaves the LAST expert without tokens (its offset sits
    at the end of the buffer), and no tokens at all."""
    a, b = _pair(seed=17)
    with torch.no_grad():
        for m in (a, b):
            m.router.gate.weight[3, 0] = -50.0
    x = torch.randn(20, 32)
    x[:, 0] = 4.0
    idx, _, _ = a.router(x)
    assert not (idx == 3).any()
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    ya, yb = a(x1), b(x2)
    assert torch.allclose(ya, yb, atol=1e-5)
    ya.sum().backward()
    yb.sum().backward()
    assert torch.allclose(x1.grad, x2.grad, atol=1e-5)
    _check_expert_grads(a, b, 1e-5)
    for p in b.experts_g.parameters():
        assert not p.grad[3].any()

    ge = GroupedExperts(num_local=4, dim=16, hidden_mult=2)
    y0 = ge(torch.randn(0, 16), torch.zeros(5, dtype=torch.long))
    assert y0.shape == (0, 16)
    y1 = ge(torch.randn(10, 16), torch.tensor([0, 4, 10, 10, 10]))
    assert y1.shape == (10, 16) and torch.isfinite(y1).all()


def test_grouped_and_batched_are_exclusive():
    with pytest.raises(ValueError):
        ExpertParallelMoE(16, 4, ep_group=None, batched=True, grouped=True)


def _moe_grouped_ep2(rank, world_size):
    """tests/test_moe.py::_moe_ep2 with grouped=True, forward and backward:
    the EP dispatch must equal the dense oracle over all experts."""
    from torchdistpackage_amd.dist.topo import tpc

    tpc.setup_process_groups([("data", world_size)])
    tpc.build_moe_groups(moe_dp_size=1, moe_ep_size=world_size)

    dim, E = 32, 4
    torch.manual_seed(0)  # same router everywhere
    moe = ExpertParallelMoE(dim, num_experts=E, top_k=2, hidden_mult=2,
                            ep_group=tpc.get_group("moe_ep"), grouped=True)
    assert moe.num_local == E // world_size
    torch.manual_seed(100)
    all_experts = [Expert(dim, 2) for _ in range(E)]
    with torch.no_grad():
        for ex in all_experts:
            ex.fc1.bias.normal_(std=0.1)
            ex.fc2.bias.normal_(std=0.1)
    lo = moe.ep_rank * moe.num_local
    moe.experts_g.load_from_experts(all_experts[lo:lo + moe.num_local])

    torch.manual_seed(5 + rank)   # different tokens per rank
    x = torch.randn(8, dim, requires_grad=True)
    out = moe(x)
    out.pow(2).sum().backward()

    xs = []
    for r in range(world_size):
        torch.manual_seed(5 + r)
        xs.append(torch.randn(8, dim))
    x_all = torch.cat(xs).requires_grad_(True)
    ref = _dense_oracle(all_experts, moe.router(x_all), x_all)
    ref.pow(2).sum().backward()

    mine = slice(rank * 8, (rank + 1) * 8)
    assert torch.allclose(out, ref[mine], atol=1e-5), \
        (out - ref[mine]).abs().max().item()
    assert torch.allclose(x.grad, x_all.grad[mine], atol=1e-4)
    for i in range(moe.num_local):
        ge = all_experts[lo + i]
        want1 = ge.fc1.weight.grad
        want2 = ge.fc2.bias.grad
        got1, got2 = moe.experts_g.w1.grad[i], moe.experts_g.b2.grad[i]
        if want1 is None:
            assert not got1.any() and not got2.any()
        else:
            assert torch.allclose(got1, want1, atol=1e-4), \
                (got1 - want1).abs().max().item()
            assert torch.allclose(got2, want2, atol=1e-4)
    return True


def test_moe_grouped_ep2():
    run_distributed(_moe_grouped_ep2, world_size=2)


def test_expert_impl_config(monkeypatch):
    from torchdistpackage_amd.models.moe_model import MoEConfig, MoEModel
    from torchdistpackage_amd.moe.layer import BatchedExperts

    monkeypatch.delenv("TDPA_MOE_EXPERTS", raising=False)
    assert MoEConfig().expert_impl == "loop"
    monkeypatch.setenv("TDPA_MOE_EXPERTS", "grouped")
    assert MoEConfig().expert_impl == "grouped"
    assert MoEConfig(expert_impl="batched").expert_impl == "batched"
    with pytest.raises(ValueError):
        MoEConfig(expert_impl="fused")
    monkeypatch.setenv("TDPA_MOE_EXPERTS", "nonsense")
    with pytest.raises(ValueError):
        MoEConfig()

    kw = dict(vocab_size=128, n_layer=1, n_head=2, dim=32, max_seq=16,
              num_experts=4, top_k=2, hidden_mult=2)
    torch.manual_seed(0)
    x = torch.randint(0, 128, (2, 16))
    for impl, attr, cls in (("loop", "experts", torch.nn.ModuleList),
                            ("batched", "experts_b", BatchedExperts),
                            ("grouped", "experts_g", GroupedExperts)):
        m = MoEModel(MoEConfig(expert_impl=impl, **kw))
        assert type(getattr(m.blocks[0].moe, attr)) is cls
        out = m(x, labels=x)
        out["loss"].backward()
        assert torch.isfinite(out["loss"])
        assert sum(1 for _ in m.expert_parameters()) > 0
        for p in m.expert_parameters():
            assert p.grad is not None
