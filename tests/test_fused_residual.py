"""CPU side of the fused residual path: off the GPU the fused entry points
are the composition of the unfused ops, exactly, and ParallelBlock computes
the same thing with the fusion switched on or off.  The kernels themselves
are covered in tests/test_fused_residual_gpu.py."""

import os
import subprocess
import sys

import pytest
import torch

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

EPS = 1e-5
SHAPES = [(5, 768), (3, 1027), nh.BF16_V8_SHAPE]
DTYPES = [torch.bfloat16, torch.float32]


def _inputs(shape, dtype, with_bias=True):
    x, w, b, dh = nh.norm_input("randn", *shape, dtype)
    y = nh.act_other("frc_y", shape, dtype)
    lb = nh.act_other("frc_lb", (shape[1],), dtype) if with_bias else None
    gx = nh.act_other("frc_gx", shape, dtype)
    return y, lb, x, w, b, dh, gx


def _leaves(*ts):
    return [None if t is None else t.detach().clone().requires_grad_(True)
            for t in ts]


def _unfused(y, lb, x, w, b):
    x_new = x + (y if lb is None else y + lb)
    return x_new, ops.layer_norm(x_new, w, b, EPS)


@pytest.mark.parametrize("dtype", DTYPES, ids=nh.dtype_name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_bias_residual_layer_norm_cpu(shape, dtype, with_bias):
    y, lb, x, w, b, dh, gx = _inputs(shape, dtype, with_bias)
    fy, flb, fx, fw, fb = _leaves(y, lb, x, w, b)
    xn, h = ops.bias_residual_layer_norm(fy, flb, fx, fw, fb, EPS)
    torch.autograd.backward([xn, h], [gx, dh])
    ry, rlb, rx, rw, rb = _leaves(y, lb, x, w, b)
    xr, hr = _unfused(ry, rlb, rx, rw, rb)
    torch.autograd.backward([xr, hr], [gx, dh])
    nh.check_equal(xn, xr, "x_new")
    nh.check_equal(h, hr, "h")
    pairs = [("dy", fy, ry), ("dx", fx, rx), ("dw", fw, rw), ("db", fb, rb)]
    if with_bias:
        pairs.append(("dbias", flb, rlb))
    for name, f, r in pairs:
        nh.check_equal(f.grad, r.grad, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=nh.dtype_name)
def test_layer_norm_fork_and_add_cpu(dtype):
    y, lb, x, w, b, dh, gx = _inputs((5, 768), dtype)
    fx, fw, fb = _leaves(x, w, b)
    x_out, h = ops.layer_norm_fork(fx, fw, fb, EPS)
    assert x_out is fx
    nh.check_equal(h, ops.layer_norm(x, w, b, EPS), "fork h")
    nh.check_equal(ops.bias_residual_add(y, lb, x), x + (y + lb), "add")
    nh.check_equal(ops.bias_residual_add(y, None, x), x + y, "add, no bias")


def test_noncontiguous_input_cpu():
    y, lb, x, w, b, _, _ = _inputs((5, 768), torch.float32)
    wide = nh.act_other("frc_wide", (5, 1536), torch.float32)
    yv = wide[:, ::2]
    xn, h = ops.bias_residual_layer_norm(yv, lb, x, w, b, EPS)
    xr, hr = _unfused(yv, lb, x, w, b)
    nh.check_equal(xn, xr, "x_new")
    nh.check_equal(h, hr, "h")


def _block_run(blk, x, dout, fused):
    prev = ops.set_fused_residual(fused)
    try:
        for p in blk.parameters():
            p.grad = None
        xin = x.detach().clone().requires_grad_(True)
        out = blk(xin)
        out.backward(dout)
    finally:
        ops.set_fused_residual(prev)
    return out.detach(), xin.grad, \
        {n: p.grad.clone() for n, p in blk.named_parameters()}


@pytest.mark.parametrize("dtype", DTYPES, ids=nh.dtype_name)
def test_parallel_block_same_with_switch_on_and_off_cpu(dtype):
    from torchdistpackage_amd.parallel.tensor.transformer import ParallelBlock
    torch.manual_seed(3)
    blk = ParallelBlock(64, 2, dtype=dtype)
    x = nh.act_other("frc_blk_x", (16, 2, 64), dtype)
    dout = nh.act_other("frc_blk_d", (16, 2, 64), dtype)
    out_f, dx_f, g_f = _block_run(blk, x, dout, True)
    out_u, dx_u, g_u = _block_run(blk, x, dout, False)
    nh.check_equal(out_f, out_u, "out")
    nh.check_equal(dx_f, dx_u, "dx")
    for n in g_u:
        nh.check_equal(g_f[n], g_u[n], "d" + n)


def test_training_dropout_takes_the_unfused_block():
    from torchdistpackage_amd.parallel.tensor.transformer import ParallelBlock
    blk = ParallelBlock(64, 2, dropout=0.1)
    called = []
    blk._forward_fused = lambda x: called.append(1)
    blk.train()
    blk(torch.randn(8, 1, 64))
    assert not called
    blk.eval()
    blk(torch.randn(8, 1, 64))
    assert called


def test_skip_bias_leaves_only_the_bias_out():
    from torchdistpackage_amd.parallel.tensor.tp_utils import \
        RowParallelLinear
    torch.manual_seed(5)
    lin = RowParallelLinear(32, 16)
    with torch.no_grad():
        lin.bias.normal_()
    x = torch.randn(4, 32)
    nh.check_equal(lin(x, skip_bias=True) + lin.bias, lin(x), "row linear")


def test_switch_is_read_from_the_environment_at_import():
    code = ("import torchdistpackage_amd.ops as o; "
            "print(o.fused_residual_enabled())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for val in ("0", None):
        env = dict(os.environ)
        env.pop("TDPA_FUSED_RESIDUAL", None)
        if val is not None:
            env["TDPA_FUSED_RESIDUAL"] = val
        outs.append(subprocess.run(
            [sys.executable, "-c", code], cwd=root, env=env, check=True,
            capture_output=True, text=True).stdout.strip())
    assert outs == ["False", "True"]
