"""Fused MoE token routing on the GPU (csrc/moe_route.hip): the counting-sort
plan against a stable argsort, the dispatch and combine kernels forward and
backward against fp64 with the torch chain in bf16 as the library arm, and
ExpertParallelMoE(route="fused") against the fp64 CPU layer.

Run on MI355X via: pytest tests/test_moe_route_gpu.py -m gpu -q
"""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.moe import ExpertParallelMoE
from tests import numerics_helpers as nh
from tests.test_moe_grouped_gpu import (DIM, E, MULT, TOPK, _build,
                                        _expert_grads, _run)
from tests.test_moe_route import torch_chain

BF16 = torch.bfloat16
CHUNK = ops.MOE_PLAN_CHUNK


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"
        assert ops.ext().MOE_PLAN_CHUNK == CHUNK


def _plan_ids(N, k, E_, kind):
    g = nh._gen("moe-plan", N, k, E_, kind)
    if kind == "one_expert":
        return torch.full((N, k), E_ - 2)
    if kind == "sparse":          # E = 256 with most experts empty
        live = torch.tensor([0, 17, 200, 255])
        return live[torch.randint(0, 4, (N, k), generator=g)]
    # "rand": iid ids, so rows name the same expert twice when k > 1
    return torch.randint(0, E_, (N, k), generator=g)


PLAN_CASES = [             # (N, k, E, ids)
    (1, 1, 3, "rand"),                       # one entry
    (5, 2, 8, "rand"),                       # fewer entries than a wave
    (50, 2, 8, "rand"),                      # 100: not a multiple of 64
    (CHUNK // 8, 8, 256, "sparse"),          # exactly one chunk, one launch
    (3 * CHUNK + 37, 1, 8, "rand"),          # three launches, ragged tail
    ((3 * CHUNK + 37) // 7, 7, 3, "rand"),   # the same count at k = 7, E = 3
    (CHUNK + 5, 2, 8, "one_expert"),         # every entry on one expert
    (CHUNK, 2, 256, "sparse"),               # two full chunks, 8 id bits
]


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64],
                         ids=["int32", "int64"])
@pytest.mark.parametrize("N,k,E_,kind", PLAN_CASES)
def test_plan_vs_stable_argsort(N, k, E_, kind, idtype):
    idx = _plan_ids(N, k, E_, kind)
    order = torch.argsort(idx.flatten(), stable=True)
    inv = torch.empty(N * k, dtype=torch.int32)
    inv[order] = torch.arange(N * k, dtype=torch.int32)
    want_counts = torch.bincount(idx.flatten(), minlength=E_)
    dest, counts, offs = ops.moe_route_plan(idx.to(_dev(), idtype), E_)
    assert dest.is_cuda and dest.shape == (N, k)
    nh.check_equal(dest.flatten(), inv, "dest")
    nh.check_equal(counts, want_counts, "counts")
    nh.check_equal(offs, F.pad(torch.cumsum(want_counts, 0), (1, 0)), "offs")


@pytest.mark.parametrize("gated", [True, False], ids=["gates", "unit"])
@pytest.mark.parametrize("N", [3, 130])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("D", [8, 520, 1024])
def test_dispatch_combine_vs_fp64(D, k, N, gated):
    assert ops.moe_route_eligible(D, BF16)
    g = nh._gen("moe-route-rows", D, k, N, gated)
    idx = torch.stack([torch.randperm(4, generator=g)[:k] for _ in range(N)])
    order = torch.argsort(idx.flatten(), stable=True)
    x = nh._randn((N, D), g).to(BF16)
    y = nh._randn((N * k, D), g).to(BF16)
    gates = torch.rand((N, k), generator=g) if gated else None
    dout_d = nh._randn((N * k, D), g).to(BF16)
    dout_c = nh._randn((N, D), g).to(BF16)
    ref = torch_chain(x, y, gates, order, k, dout_d, dout_c, torch.float64,
                      "cpu")
    lib = torch_chain(x, y, gates, order, k, dout_d, dout_c, BF16, _dev())

    dest, _, _ = ops.moe_route_plan(idx.to(_dev()), 4)
    x1 = x.to(_dev()).requires_grad_(True)
    y1 = y.to(_dev()).requires_grad_(True)
    g1 = gates.to(_dev()).requires_grad_(True) if gated else None
    disp = ops.moe_dispatch(x1, dest)
    comb = ops.moe_combine(y1, dest, g1)
    disp.backward(dout_d.to(_dev()))
    comb.backward(dout_c.to(_dev()))
    got = [disp.detach(), comb.detach(), x1.grad, y1.grad] + \
        ([g1.grad] if gated else [])

    what = f"D={D} k={k} N={N}"
    nh.check_equal(got[0], ref[0].to(BF16), f"{what} dispatch")
    f_fwd, f_grad = nh.floors(BF16)
    for n, a, r, b in zip(["combine", "dx", "dy", "dgates"], got[1:],
                          ref[1:], lib[1:]):
        assert a.dtype == (torch.float32 if n == "dgates" else BF16)
        floor = f_fwd if n == "combine" else \
            nh.floors(torch.float32)[1] if n == "dgates" else f_grad
        nh.yardstick(a, r, b, floor, what=f"{what} {n}")


@pytest.mark.parametrize("tokens,empty_expert",
                         [(64, False), (200, False), (150, True)],
                         ids=["64tok", "200tok", "150tok-empty_expert"])
def test_fused_route_layer_vs_torch_route_and_fp64(tokens, empty_expert):
    master, x, dy = _build(tokens, empty_expert)

    ref = copy.deepcopy(master)       # fp64 CPU loop layer, fp32 router
    ref.experts.double()
    y_ref, dx_ref, idx_ref = _run(ref, x.double(), dy.double())
    g_ref = _expert_grads(ref)

    runs = {}
    for route in ("torch", "fused"):
        m = ExpertParallelMoE(DIM, E, TOPK, MULT, ep_group=None,
                              grouped=True, route=route)
        m.experts_g.load_from_experts(master.experts)
        with torch.no_grad():
            m.router.gate.weight.copy_(master.router.gate.weight)
        m.experts_g.to(BF16)
        m.to(_dev())
        y, dx, idx = _run(m, x.to(_dev()), dy.to(_dev()))
        assert torch.equal(idx, idx_ref), f"{route}: routing differs"
        runs[route] = (y, dx, _expert_grads(m), m.router.gate.weight.grad)
    y, dx, g_got, dr = runs["fused"]
    y_lib, dx_lib, g_lib, dr_lib = runs["torch"]

    what = f"moe fused route {tokens} tok"
    f_fwd, f_grad = nh.floors(BF16)
    assert y.dtype == BF16 and y.is_cuda
    nh.yardstick(y, y_ref, y_lib, f_fwd, what=f"{what} y")
    nh.yardstick(dx, dx_ref, dx_lib, f_grad, what=f"{what} dx")
    nh.yardstick(dr, ref.router.gate.weight.grad, dr_lib, f_grad,
                 what=f"{what} drouter")
    for n in ("w1", "b1", "w2", "b2"):
        nh.yardstick(g_got[n], g_ref[n], g_lib[n], f_grad,
                     what=f"{what} d{n}")
        if empty_expert:
            assert not g_got[n][E - 1].any(), \
                f"{what}: d{n} of the empty expert is not exactly zero"
