"""ExpertParallelMoE(grouped=True) on the GPU: the grouped HIP GEMM path
against an fp64 CPU run of the same layer, with the existing per-expert loop
path (grouped=False, bf16, same device) as the library yardstick.

dim=256, hidden_mult=2 keeps both expert GEMMs on the kernels (256 and 512
wide); 4 experts, top-2, 64 to 200 tokens.  One case routes nothing to the
last expert: its weight gradients must be exactly zero.

Run on MI355X via: pytest tests/test_moe_grouped_gpu.py -m gpu -q
"""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.moe import ExpertParallelMoE
from tests import numerics_helpers as nh

BF16 = torch.bfloat16
DIM, MULT, E, TOPK = 256, 2, 4, 2


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"


def _round_bf16_(t):
    t.copy_(t.to(BF16).to(t.dtype))


def _build(tokens, empty_expert):
    """(master fp32 CPU loop layer with bf16-valued expert weights, x, dy).
    ``empty_expert``: column 0 of x is a constant 4 and the router's last
    row weighs it by -8, so the last expert's logit trails by ~32 and top-2
    never picks it."""
    g = nh._gen("moe-grouped", tokens, empty_expert)
    torch.manual_seed(1234 + tokens)
    master = ExpertParallelMoE(DIM, E, TOPK, MULT, ep_group=None)
    with torch.no_grad():
        for ex in master.experts:
            ex.fc1.bias.copy_(0.1 * nh._randn(ex.fc1.bias.shape, g))
            ex.fc2.bias.copy_(0.1 * nh._randn(ex.fc2.bias.shape, g))
            for p in ex.parameters():
                _round_bf16_(p)
        if empty_expert:
            master.router.gate.weight[E - 1, 0] = -8.0
    x = nh._randn((tokens, DIM), g)
    if empty_expert:
        x[:, 0] = 4.0
    x = x.to(BF16)
    dy = nh._randn((tokens, DIM), g).to(BF16)
    return master, x, dy


def _run(layer, x, dy):
    x = x.detach().clone().requires_grad_(True)
    y = layer(x)
    y.backward(dy)
    with torch.no_grad():
        idx, _, _ = layer.router(x.reshape(-1, DIM))
    return y.detach(), x.grad.detach(), idx.cpu()


def _expert_grads(layer):
    """{name: (E, ...) stacked gradient} for either expert container."""
    if getattr(layer, "grouped", False):
        eg = layer.experts_g
        return {"w1": eg.w1.grad, "b1": eg.b1.grad, "w2": eg.w2.grad,
                "b2": eg.b2.grad}
    ex = layer.experts

    def stack(get):
        return torch.stack([
            get(e).grad if get(e).grad is not None
            else torch.zeros_like(get(e)) for e in ex])
    return {"w1": stack(lambda e: e.fc1.weight),
            "b1": stack(lambda e: e.fc1.bias),
            "w2": stack(lambda e: e.fc2.weight),
            "b2": stack(lambda e: e.fc2.bias)}


@pytest.mark.parametrize("tokens,empty_expert",
                         [(64, False), (200, False), (150, True)],
                         ids=["64tok", "200tok", "150tok-empty_expert"])
def test_grouped_moe_vs_loop_and_fp64(tokens, empty_expert):
    assert ops.grouped_gemm_eligible(DIM * MULT, DIM, BF16)
    assert ops.grouped_gemm_eligible(DIM, DIM * MULT, BF16)
    master, x, dy = _build(tokens, empty_expert)

    # fp64 CPU reference: the loop layer, experts in fp64 (the router is
    # fp32 in every run)
    ref = copy.deepcopy(master)
    ref.experts.double()
    y_ref, dx_ref, idx_ref = _run(ref, x.double(), dy.double())
    g_ref = _expert_grads(ref)

    # library: the existing loop path in bf16 on the device
    lib = copy.deepcopy(master)
    lib.experts.to(BF16)
    lib.to(_dev())
    y_lib, dx_lib, idx_lib = _run(lib, x.to(_dev()), dy.to(_dev()))
    g_lib = _expert_grads(lib)

    # under test: grouped=True with the same weights and router
    got = ExpertParallelMoE(DIM, E, TOPK, MULT, ep_group=None, grouped=True)
    got.experts_g.load_from_experts(master.experts)
    with torch.no_grad():
        got.router.gate.weight.copy_(master.router.gate.weight)
    got.experts_g.to(BF16)
    got.to(_dev())
    y, dx, idx = _run(got, x.to(_dev()), dy.to(_dev()))
    g_got = _expert_grads(got)

    # the three runs must have routed alike, or they are not comparable
    assert torch.equal(idx, idx_ref) and torch.equal(idx_lib, idx_ref)
    counts = torch.bincount(idx_ref.flatten(), minlength=E)
    if empty_expert:
        assert counts[E - 1] == 0 and (counts[:E - 1] > 0).all(), counts

    what = f"moe grouped {tokens} tok"
    f_fwd, f_grad = nh.floors(BF16)
    assert y.dtype == BF16 and y.is_cuda and got.experts_g.w1.is_cuda
    nh.yardstick(y, y_ref, y_lib, f_fwd, what=f"{what} y")
    nh.yardstick(dx, dx_ref, dx_lib, f_grad, what=f"{what} dx")
    for n in ("w1", "b1", "w2", "b2"):
        assert g_got[n].dtype == BF16
        nh.yardstick(g_got[n], g_ref[n], g_lib[n], f_grad,
                     what=f"{what} d{n}")
        if empty_expert:
            assert not g_got[n][E - 1].any(), \
                f"{what}: d{n} of the empty expert is not exactly zero"
