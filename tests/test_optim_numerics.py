"""AdamW on hard inputs against fp64, CPU paths: ``ops.fused_adamw_`` and
``FusedAdamW`` run every family of tests/numerics_helpers.py, and two
deliberately wrong emulations of the HIP kernels' arithmetic show that the
bound has teeth.  tests/test_optim_numerics_gpu.py holds the HIP kernels to
the same bound."""

import math

import pytest
import torch

import numerics_helpers as H
import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.ops.optim import FusedAdamW

N = 1031
HY = H.OPT_HYPER
CASES = [(f, s, b) for f in H.OPT_FAMILIES for s in H.OPT_STEPS
         for b in H.OPT_BETAS]
IDS = [f"{f}-t{s}-b{b[1]}" for f, s, b in CASES]


def _args(step, betas):
    return (step, HY["lr"], betas, HY["eps"], HY["weight_decay"])


def _misses(got, ins, step, betas):
    """Names of the outputs of ``got`` that miss the bound."""
    a = _args(step, betas)
    e = H.optim_err(got, ins, *a)
    el = H.optim_err(H.adamw_lib(*ins, *a), ins, *a)
    return {k for k in e if not e[k] <= max(H.MARGIN * el[k], H.FLOOR_OPT)}


@pytest.mark.parametrize("family,step,betas", CASES, ids=IDS)
def test_fused_adamw_cpu(family, step, betas):
    ins = H.opt_input(family, N, step, betas)
    p, g, m, v = (t.clone() for t in ins)
    ops.fused_adamw_(p, g, m, v, step, HY["lr"], betas[0], betas[1],
                     HY["eps"], HY["weight_decay"])
    assert torch.equal(g, ins[1]), "the grad must not be written"
    H.optim_check((p, m, v), ins, step, HY, betas, "cpu",
                  f"fused_adamw_ cpu {family} t={step} b2={betas[1]}")


def _preload(opt, step, m, v):
    """Put (step-1, m, v) into a one-flat FusedAdamW through its own
    state_dict / load_state_dict."""
    sd = opt.state_dict()
    assert isinstance(sd["step"], int) and sd["step"] == 0
    sd["step"] = step - 1
    fsd = sd["groups"][0][0]
    sd["groups"][0][0] = {"master": fsd["master"],
                          "exp_avg": m.clone().to(fsd["exp_avg"].device),
                          "exp_avg_sq": v.clone().to(fsd["exp_avg"].device)}
    opt.load_state_dict(sd)


@pytest.mark.parametrize("family,step,betas", CASES, ids=IDS)
def test_fused_adamw_optimizer_cpu(family, step, betas):
    ins = H.opt_input(family, N, step, betas)
    p = torch.nn.Parameter(ins[0].clone())
    opt = FusedAdamW([p], lr=HY["lr"], betas=betas, eps=HY["eps"],
                     weight_decay=HY["weight_decay"])
    _preload(opt, step, ins[2], ins[3])
    p.grad = ins[1].clone()
    opt.step()
    sd = opt.state_dict()
    assert isinstance(sd["step"], int) and sd["step"] == step
    fg = opt.param_groups[0]["_flats"][0]
    assert torch.equal(p.detach(), fg.master)
    H.optim_check((fg.master, fg.exp_avg, fg.exp_avg_sq), ins, step, HY,
                  betas, "cpu",
                  f"FusedAdamW cpu {family} t={step} b2={betas[1]}")


@pytest.mark.parametrize("family,step,betas", CASES, ids=IDS)
def test_kernel_arithmetic_emulation_meets_bound(family, step, betas):
    """The arithmetic the HIP kernels use (fp32, coefficients from double)."""
    ins = H.opt_input(family, N, step, betas)
    got = H.adamw_emulate(*ins, *_args(step, betas))
    H.optim_check(got, ins, step, HY, betas, "cpu",
                  f"emulation {family} t={step} b2={betas[1]}")


@pytest.mark.parametrize("step", [1, 2, 10])
@pytest.mark.parametrize("family", [f for f in H.OPT_FAMILIES
                                    if f != "zero_grad"])
def test_teeth_fp32_coefficients_miss(family, step):
    """1.f - beta2 formed in fp32 is 1.3e-5 off at beta2 = 0.999: v', and
    p' from step 2 on, must miss the bound."""
    betas = (0.9, 0.999)
    ins = H.opt_input(family, N, step, betas)
    got = H.adamw_emulate(*ins, *_args(step, betas), coef="fp32")
    missed = _misses(got, ins, step, betas)
    assert "v" in missed, missed
    if step >= 2 and family in ("randn", "small_p"):
        assert "p" in missed, missed


@pytest.mark.parametrize("betas", H.OPT_BETAS)
@pytest.mark.parametrize("step", H.OPT_STEPS)
def test_teeth_eps_inside_sqrt_misses(step, betas):
    """sqrt(v/bc2 + eps) for sqrt(v/bc2) + eps must miss in eps_scale."""
    ins = H.opt_input("eps_scale", N, step, betas)
    got = H.adamw_emulate(*ins, *_args(step, betas), eps_inside=True)
    assert "p" in _misses(got, ins, step, betas)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_fused_adamw_cpu_nonfinite_grad(bad):
    step, betas = 10, (0.9, 0.999)
    ins = list(H.opt_input("randn", N, step, betas))
    ins[1] = ins[1].clone()
    ins[1][517] = bad
    p, g, m, v = (t.clone() for t in ins)
    ops.fused_adamw_(p, g, m, v, step, HY["lr"], betas[0], betas[1],
                     HY["eps"], HY["weight_decay"])
    lib = H.adamw_lib(*ins, *_args(step, betas))
    for got, want, name in zip((p, m, v), lib, "pmv"):
        assert torch.equal(torch.isfinite(got), torch.isfinite(want)), name
        assert not torch.isfinite(got[517]), name
    keep = torch.ones(N, dtype=torch.bool)
    keep[517] = False
    H.optim_check((p, m, v), ins, step, HY, betas, "cpu",
                  f"fused_adamw_ cpu grad={bad}", keep=keep, lib=lib)


def test_zero_grad_elements_see_pure_decay():
    step, betas = 10, (0.9, 0.999)
    ins = H.opt_input("zero_grad", N, step, betas)
    p, g, m, v = (t.clone() for t in ins)
    ops.fused_adamw_(p, g, m, v, step, HY["lr"], betas[0], betas[1],
                     HY["eps"], HY["weight_decay"])
    want = (ins[0][::2].double() * (1 - HY["lr"] * HY["weight_decay"]))
    assert torch.isfinite(p).all()
    assert (p[::2].double() - want).abs().max() <= \
        2.0 ** -23 * want.abs().max()
    assert (m[::2] == 0).all() and (v[::2] == 0).all()


def test_opt_input_moments_are_stationary():
    """The generator's own contract: zero state at step 1, and moments of
    the stated size later."""
    p, g, m, v = H.opt_input("randn", 4096, 1, (0.9, 0.999))
    assert (m == 0).all() and (v == 0).all()
    p, g, m, v = H.opt_input("big_grad", 4096, 1000, (0.9, 0.999))
    assert 0.5e24 * (1 - 0.999 ** 999) <= v.min().item()
    assert v.max().item() <= 1.5e24
    want = 1e12 * math.sqrt(0.1 / 1.9)
    assert 0.9 * want < m.std().item() < 1.1 * want
    pb, gb, _, _ = H.opt_input("randn", 64, 2, (0.9, 0.95), torch.bfloat16)
    assert torch.equal(pb, pb.bfloat16().float())
    assert torch.equal(gb, gb.bfloat16().float())
