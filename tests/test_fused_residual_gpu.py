"""Fused residual-stream kernels against the unfused composition they
replace (docs/design/kernels.md, "Fused residual kernels").

Everything but the bias grads must match the unfused ops BIT FOR BIT: the
kernels make the same bf16 roundings in the same order.  The bias grads
(column sums) differ in fp32 summation order only and are held to the
yardstick of tests/numerics_helpers.py against the fp64 column sum of the same
bf16 addends, with torch's own bf16 ``.sum(0)`` as the library; exact-integer
cases pin them bit for bit as well.

Run on MI355X via: pytest tests/test_fused_residual_gpu.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

BF16 = torch.bfloat16
EPS = 1e-5
FAMILIES = ["randn", "shift30", "outlier_last", "zero_var", "huge"]
# the register-path entries of NORM_SHAPES
REG_SHAPES = [(3, 64), (5, 768), (2, 2056), (2, 6144), (2, 8192), (2050, 64)]
assert all(s in nh.NORM_SHAPES for s in REG_SHAPES)


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"
        # the kernels are tested whatever TDPA_FUSED_RESIDUAL the suite
        # runs under
        module._prev_switch = ops.set_fused_residual(True)


def teardown_module(module):
    if hasattr(module, "_prev_switch"):
        ops.set_fused_residual(module._prev_switch)


def _junction_input(family, shape, with_bias):
    """(y, lin_bias or None, x_res, w, b, dh, gx) on the device, bf16.
    x_res is the norm family's x; for zero_var the rows that family makes
    constant get y = 0, so that without a bias they stay constant."""
    x, w, b, dh = nh.norm_input(family, *shape, BF16)
    y = nh.act_other("fr_y", shape, BF16)
    if family == "zero_var":
        y[:2] = 0.0
    lb = nh.act_other("fr_lb", (shape[1],), BF16) if with_bias else None
    gx = nh.act_other("fr_gx", shape, BF16)
    d = _dev()
    return (y.to(d), lb.to(d) if with_bias else None, x.to(d), w.to(d),
            b.to(d), dh.to(d), gx.to(d))


def _unfused_junction(y, lb, x, w, b):
    x_new = x + (y if lb is None else y + lb)
    return x_new, ops.layer_norm(x_new, w, b, EPS)


def _leaves(*ts):
    return [None if t is None else t.detach().clone().requires_grad_(True)
            for t in ts]


def _colsum_check(got, addends, what):
    """Bias grad ``got`` against the fp64 column sum of the bf16 addends."""
    a2 = addends.reshape(-1, addends.shape[-1])
    assert got.dtype == a2.dtype == BF16
    nh.yardstick(got, a2.double().sum(0).cpu(), a2.sum(0),
                 nh.FLOOR_BF16_GRAD, what=what)


def _cases():
    for fam in FAMILIES:
        for shape in REG_SHAPES:
            for wb in (True, False):
                yield pytest.param(
                    fam, shape, wb,
                    id=f"{fam}-{shape[0]}x{shape[1]}-"
                       f"{'bias' if wb else 'nobias'}")


# ------------------------------------------------ 1. junction: bit equality

@pytest.mark.parametrize("family,shape,with_bias", list(_cases()))
def test_bias_residual_layer_norm_matches_unfused(family, shape, with_bias):
    y, lb, x, w, b, dh, gx = _junction_input(family, shape, with_bias)
    what = f"brln[{family} {shape} bias={with_bias}]"

    # forward, statistics included, straight from the kernel
    x_new, h, mean, rstd = ops.ext("layer_norm").bias_residual_layernorm_fwd(
        y, lb, x, w, b, EPS)
    x_ref, h_ref = _unfused_junction(y, lb, x, w, b)
    _, mean_ref, rstd_ref = ops.ext("layer_norm").layernorm_fwd(
        x_ref, w, b, EPS)
    nh.check_equal(x_new, x_ref, what + " x_new")
    nh.check_equal(h, h_ref, what + " h")
    nh.check_equal(mean, mean_ref, what + " mean")
    nh.check_equal(rstd, rstd_ref, what + " rstd")

    # backward through the public op against autograd through the unfused ops
    fy, flb, fx, fw, fb = _leaves(y, lb, x, w, b)
    xn, hh = ops.bias_residual_layer_norm(fy, flb, fx, fw, fb, EPS)
    assert "BiasResidualLayerNorm" in type(xn.grad_fn).__name__, \
        "the fused path must be taken for this shape"
    nh.check_equal(xn, x_ref, what + " x_new (op)")
    nh.check_equal(hh, h_ref, what + " h (op)")
    torch.autograd.backward([xn, hh], [gx, dh])

    ry, rlb, rx, rw, rb = _leaves(y, lb, x, w, b)
    xr, hr = _unfused_junction(ry, rlb, rx, rw, rb)
    torch.autograd.backward([xr, hr], [gx, dh])

    nh.check_equal(fy.grad, ry.grad, what + " dy")
    nh.check_equal(fx.grad, rx.grad, what + " dx_res")
    nh.check_equal(fw.grad, rw.grad, what + " ln dw")
    nh.check_equal(fb.grad, rb.grad, what + " ln db")
    if with_bias:
        _colsum_check(flb.grad, fy.grad, what + " dbias")


@pytest.mark.parametrize("family,shape",
                         [pytest.param(f, s, id=f"{f}-{s[0]}x{s[1]}")
                          for f in FAMILIES for s in REG_SHAPES])
def test_layer_norm_fork_matches_unfused(family, shape):
    _, _, x, w, b, dh, gx = _junction_input(family, shape, False)
    what = f"fork[{family} {shape}]"
    fx, fw, fb = _leaves(x, w, b)
    x_out, h = ops.layer_norm_fork(fx, fw, fb, EPS)
    assert "LayerNormFork" in type(h.grad_fn).__name__
    nh.check_equal(x_out, x, what + " x")
    torch.autograd.backward([x_out, h], [gx, dh])

    rx, rw, rb = _leaves(x, w, b)
    h_ref = ops.layer_norm(rx, rw, rb, EPS)
    nh.check_equal(h, h_ref, what + " h")
    torch.autograd.backward([rx * 1, h_ref], [gx, dh])
    nh.check_equal(fx.grad, rx.grad, what + " dx")
    nh.check_equal(fw.grad, rw.grad, what + " dw")
    nh.check_equal(fb.grad, rb.grad, what + " db")


def test_junction_backward_with_a_missing_grad():
    """Either incoming grad may be None: the plain pieces take over."""
    y, lb, x, w, b, dh, gx = _junction_input("randn", (5, 768), True)
    for use_h, use_x in ((True, False), (False, True)):
        fy, flb, fx, fw, fb = _leaves(y, lb, x, w, b)
        xn, hh = ops.bias_residual_layer_norm(fy, flb, fx, fw, fb, EPS)
        ry, rlb, rx, rw, rb = _leaves(y, lb, x, w, b)
        xr, hr = _unfused_junction(ry, rlb, rx, rw, rb)
        if use_h:
            hh.backward(dh)
            hr.backward(dh)
        else:
            xn.backward(gx)
            xr.backward(gx)
        what = f"missing grad (h={use_h}, x={use_x})"
        nh.check_equal(fy.grad, ry.grad, what + " dy")
        nh.check_equal(fx.grad, rx.grad, what + " dx_res")
        nh.check_equal(flb.grad, rlb.grad, what + " dbias")
        if use_h:
            nh.check_equal(fw.grad, rw.grad, what + " dw")
            nh.check_equal(fb.grad, rb.grad, what + " db")
        else:
            assert fw.grad is None and fb.grad is None


ADD_SHAPES = REG_SHAPES + [(2056, 2056)]    # the last: > 2048 blocks of 2048


@pytest.mark.parametrize("family,shape,with_bias", [
    pytest.param(f, s, wb, id=f"{f}-{s[0]}x{s[1]}-{'bias' if wb else 'nobias'}")
    for f in FAMILIES for s in ADD_SHAPES for wb in (True, False)
    if s != (2056, 2056) or f == "randn"])
def test_bias_residual_add_matches_unfused(family, shape, with_bias):
    y, lb, x, _, _, _, gx = _junction_input(family, shape, with_bias)
    what = f"bias_residual_add[{family} {shape} bias={with_bias}]"
    fy, flb, fx = _leaves(y, lb, x)
    out = ops.bias_residual_add(fy, flb, fx)
    assert "BiasResidualAdd" in type(out.grad_fn).__name__
    nh.check_equal(out, x + (y if lb is None else y + lb), what)
    out.backward(gx)
    nh.check_equal(fy.grad, gx, what + " dy")
    nh.check_equal(fx.grad, gx, what + " dx_res")
    if with_bias:
        _colsum_check(flb.grad, gx, what + " dbias")


# (1030, 8192): 512 row lanes for 1030 rows, the row loop strides
GELU_SHAPES = [(7, 512), (257, 2056), (2050, 64), (1030, 8192)]


@pytest.mark.parametrize("family,shape", [
    pytest.param(f, s, id=f"{f}-{s[0]}x{s[1]}")
    for f in nh.ACT_FAMILIES for s in GELU_SHAPES])
def test_bias_gelu_bwd_colsum(family, shape):
    d = _dev()
    x = nh.act_input(family, shape, BF16).to(d)
    bias = nh.act_bias("fr_gelu", (shape[1],), BF16).to(d)
    dy = nh.act_other("fr_gelu_dy", shape, BF16).to(d)
    what = f"bias_gelu_bwd_colsum[{family} {shape}]"
    e = ops.ext("bias_gelu")
    dx, partial = e.bias_gelu_bwd_colsum(dy, x, bias)
    nh.check_equal(dx, e.bias_gelu_bwd(dy, x, bias), what + " dx")
    assert partial.dtype == torch.float32 and partial.shape[1] == shape[1]
    _colsum_check(partial.sum(0).to(BF16), dx, what + " dbias")

    # and through autograd: same dx, the kernel's bias grad
    fx, fb = _leaves(x, bias)
    ops.bias_gelu(fx, fb).backward(dy)
    nh.check_equal(fx.grad, dx, what + " dx (op)")
    nh.check_equal(fb.grad, partial.sum(0).to(BF16), what + " dbias (op)")


# ------------------------------------------------- 2. bias grads, exact cases
#
# Addends are integers in [-4, 4] and there are at most 2050 rows: every
# partial sum is an integer below 2**24, exact in fp32 in any order, so the
# result is the fp64 sum rounded once to bf16.

@pytest.mark.parametrize("shape", [(2050, 64), (5, 768), (33, 2056)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_layer_norm_bias_grad_exact(shape):
    """dh = 0 makes the LayerNorm term exactly zero: g = g_res."""
    d = _dev()
    x, w, b, _ = (t.to(d) for t in nh.norm_input("randn", *shape, BF16))
    g_res = nh.int_mat("fr_ln_exact", shape).to(d)
    dh = torch.zeros_like(x)
    mean, rstd = ops.ext("layer_norm").layernorm_fwd(x, w, b, EPS)[1:]
    g, partial = ops.ext("layer_norm").layernorm_bwd_residual(
        dh, x, w, mean, rstd, g_res, True)
    nh.check_equal(g, g_res, "exact ln g")
    sums = partial.sum(1)
    want = g_res.double().sum(0).to(BF16)
    nh.check_equal(sums[2].to(BF16), want, "exact ln colsum")
    assert not sums[0].any() and not sums[1].any(), "dw, db of dh = 0"


@pytest.mark.parametrize("shape", [(2050, 64), (7, 512), (1030, 8192)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_bias_gelu_bias_grad_exact(shape):
    """x = 20 with bias 0: gelu_df is exactly 1 in the kernel's own formula
    (tanh saturates to 1.f), so dx = dy."""
    d = _dev()
    x = torch.full(shape, 20.0, dtype=BF16, device=d)
    bias = torch.zeros(shape[1], dtype=BF16, device=d)
    dy = nh.int_mat("fr_gelu_exact", shape).to(d)
    dx, partial = ops.ext("bias_gelu").bias_gelu_bwd_colsum(dy, x, bias)
    nh.check_equal(dx, dy, "exact gelu dx")
    nh.check_equal(partial.sum(0).to(BF16), dy.double().sum(0).to(BF16),
                   "exact gelu colsum")


# ------------------------------------------------------------- 3. fallbacks

def _fallback_inputs(kind):
    d = _dev()
    if kind == "odd_width":
        shape, dtype = (3, 1027), BF16
    elif kind == "too_wide":
        shape, dtype = nh.BF16_V8_SHAPE, BF16
    elif kind == "fp32":
        shape, dtype = (5, 768), torch.float32
    else:
        assert kind == "noncontig"
        shape, dtype = (5, 768), BF16
    x, w, b, dh = (t.to(d) for t in nh.norm_input("randn", *shape, dtype))
    y = nh.act_other("fr_fb_y", shape, dtype).to(d)
    if kind == "noncontig":
        wide = nh.act_other("fr_fb_y2", (shape[0], 2 * shape[1]), dtype).to(d)
        y = wide[:, ::2]
        assert not y.is_contiguous()
    lb = nh.act_other("fr_fb_lb", (shape[1],), dtype).to(d)
    gx = nh.act_other("fr_fb_gx", shape, dtype).to(d)
    return y, lb, x, w, b, dh, gx


@pytest.mark.parametrize("kind", ["odd_width", "too_wide", "fp32",
                                  "noncontig"])
def test_fallbacks_are_the_composition(kind):
    y, lb, x, w, b, dh, gx = _fallback_inputs(kind)

    def y_leaf():
        """(leaf, the y the op sees): clone() would make y contiguous."""
        if kind != "noncontig":
            leaf = y.detach().clone().requires_grad_(True)
            return leaf, leaf
        leaf = y._base.detach().clone().requires_grad_(True)
        view = leaf[:, ::2]
        assert not view.is_contiguous() and torch.equal(view, y)
        return leaf, view

    fy, fy_in = y_leaf()
    flb, fx, fw, fb = _leaves(lb, x, w, b)
    xn, hh = ops.bias_residual_layer_norm(fy_in, flb, fx, fw, fb, EPS)
    assert "BiasResidual" not in type(xn.grad_fn).__name__
    torch.autograd.backward([xn, hh], [gx, dh])
    ry, ry_in = y_leaf()
    rlb, rx, rw, rb = _leaves(lb, x, w, b)
    xr, hr = _unfused_junction(ry_in, rlb, rx, rw, rb)
    torch.autograd.backward([xr, hr], [gx, dh])
    nh.check_equal(xn, xr, kind + " x_new")
    nh.check_equal(hh, hr, kind + " h")
    for name, f, r in (("dy", fy, ry), ("dbias", flb, rlb), ("dx", fx, rx),
                       ("dw", fw, rw), ("db", fb, rb)):
        nh.check_equal(f.grad, r.grad, f"{kind} {name}")

    out = ops.bias_residual_add(y, lb, x)
    nh.check_equal(out, x + (y + lb), kind + " bias_residual_add")

    if kind != "noncontig":         # the fork takes x alone
        gx_, gw_, gb_ = _leaves(x, w, b)
        x_out, h = ops.layer_norm_fork(gx_, gw_, gb_, EPS)
        assert x_out is gx_, "fallback hands x through untouched"
        assert "Fork" not in type(h.grad_fn).__name__
        nh.check_equal(h, ops.layer_norm(x, w, b, EPS), kind + " fork h")


def test_switch_off_is_the_composition():
    y, lb, x, w, b, dh, gx = _junction_input("randn", (5, 768), True)
    prev = ops.set_fused_residual(False)
    try:
        fy, flb, fx, fw, fb = _leaves(y, lb, x, w, b)
        xn, _ = ops.bias_residual_layer_norm(fy, flb, fx, fw, fb, EPS)
        assert "BiasResidual" not in type(xn.grad_fn).__name__
        out = ops.bias_residual_add(fy, flb, fx)
        assert "BiasResidual" not in type(out.grad_fn).__name__
        x_out, _ = ops.layer_norm_fork(fx, fw, fb, EPS)
        assert x_out is fx
    finally:
        ops.set_fused_residual(prev)


# ------------------------------------------------------------ 4. attn_delta

def _delta_views(B, H, S, D, layout, o, do):
    """o, do given as (B, H, S, D) values; returns device views in
    ``layout``."""
    d = _dev()
    if layout == "contiguous":
        return o.to(d), do.to(d)
    assert layout == "sbhd"
    def conv(t):
        buf = t.permute(2, 0, 1, 3).reshape(S, B, H * D).contiguous().to(d)
        return buf.view(S, B, H, D).permute(1, 2, 0, 3)
    return conv(o), conv(do)


DELTA_SHAPES = [(1, 3, 37), (2, 2, 192)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("bhs", DELTA_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", ["contiguous", "sbhd"])
def test_attn_delta(D, bhs, layout):
    B, H, S = bhs
    o = nh.act_other("fr_delta_o", (B, H, S, D), BF16)
    do = nh.act_other("fr_delta_do", (B, H, S, D), BF16)
    ov, dov = _delta_views(B, H, S, D, layout, o, do)
    got = ops.ext("attn_delta").attn_delta(ov, dov)
    assert got.shape == (B, H, S) and got.dtype == torch.float32
    ref = (o.double() * do.double()).sum(-1)
    lib = (ov.float() * dov.float()).sum(-1)
    nh.yardstick(got, ref, lib, nh.FLOOR_FP32,
                 what=f"attn_delta[D{D} {bhs} {layout}]")


@pytest.mark.parametrize("D,bhs", [(64, (1, 3, 37)), (128, (2, 2, 192)),
                                   # more rows than one pass of the capped
                                   # grid: 2048 blocks x 16 (D128) / 32 (D64)
                                   (128, (2, 17, 1000)), (64, (2, 33, 1000))],
                         ids=["D64", "D128", "D128-gridstride",
                              "D64-gridstride"])
@pytest.mark.parametrize("layout", ["contiguous", "sbhd"])
def test_attn_delta_exact(D, bhs, layout):
    """Integers in [-4, 4]: every product and partial sum is an integer of
    at most 16 * 128, exact in fp32 in any order."""
    B, H, S = bhs
    o = nh.int_mat("fr_delta_io", (B, H, S, D))
    do = nh.int_mat("fr_delta_ido", (B, H, S, D))
    ov, dov = _delta_views(B, H, S, D, layout, o, do)
    got = ops.ext("attn_delta").attn_delta(ov, dov)
    nh.check_equal(got, (o.double() * do.double()).sum(-1).float(),
                   f"attn_delta exact[D{D} {bhs} {layout}]")


# ------------------------------------------------------------ 5. block level

DIM, HEADS, SEQ, BATCH = 256, 2, 64, 2
ROW_BIASES = ("attn.proj.bias", "mlp.fc2.bias")


def _make_block():
    from torchdistpackage_amd.parallel.tensor.transformer import ParallelBlock
    torch.manual_seed(7)
    blk = ParallelBlock(DIM, HEADS, device=_dev(), dtype=BF16)
    with torch.no_grad():           # biases and LN params off their inits
        for n, p in blk.named_parameters():
            if p.dim() == 1:
                p.add_(nh.act_other("fr_blk_" + n, tuple(p.shape), BF16)
                       .to(_dev()) * 0.5)
    x = nh.act_other("fr_blk_x", (SEQ, BATCH, DIM), BF16).to(_dev())
    dout = nh.act_other("fr_blk_dout", (SEQ, BATCH, DIM), BF16).to(_dev())
    return blk, x, dout


def _run_block(blk, x, dout, fused, wrap=None):
    """(out, dx, {param: grad}, grad of the attention output)."""
    prev = ops.set_fused_residual(fused)
    seen = {}

    def grab_grad(module, args, out):       # returns None: output unchanged
        out.register_hook(
            lambda g: seen.__setitem__("attn_out_grad", g.detach().clone()))

    hook = blk.attn.register_forward_hook(grab_grad)
    try:
        for p in blk.parameters():
            p.grad = None
        xin = x.detach().clone().requires_grad_(True)
        out = wrap(blk, xin) if wrap else blk(xin)
        out.backward(dout)
    finally:
        hook.remove()
        ops.set_fused_residual(prev)
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    return out.detach(), xin.grad.detach(), grads, seen["attn_out_grad"]


_BLOCK_REF = {}


def _block_ref():
    """The unfused run, computed once and shared."""
    if not _BLOCK_REF:
        blk, x, dout = _make_block()
        _BLOCK_REF.update(blk=blk, x=x, dout=dout,
                          ref=_run_block(blk, x, dout, fused=False))
    return _BLOCK_REF


def _compare_block(got, ref, dout, what, bias_exact):
    out, dx, grads, ga = got
    out_r, dx_r, grads_r, ga_r = ref
    nh.check_equal(out, out_r, what + " out")
    nh.check_equal(dx, dx_r, what + " dx")
    nh.check_equal(ga, ga_r, what + " attention output grad")
    assert set(grads) == set(grads_r)
    addends = {"attn.proj.bias": ga, "mlp.fc2.bias": dout}
    for n in grads:
        if n in ROW_BIASES and not bias_exact:
            _colsum_check(grads[n], addends[n], f"{what} d{n}")
        else:
            nh.check_equal(grads[n], grads_r[n], f"{what} d{n}")


def test_block_fused_matches_unfused():
    r = _block_ref()
    got = _run_block(r["blk"], r["x"], r["dout"], fused=True)
    _compare_block(got, r["ref"], r["dout"], "block", bias_exact=False)


def test_block_fused_under_checkpoint():
    from torch.utils.checkpoint import checkpoint
    r = _block_ref()
    plain = _run_block(r["blk"], r["x"], r["dout"], fused=True)
    ck = _run_block(r["blk"], r["x"], r["dout"], fused=True,
                    wrap=lambda b, xin: checkpoint(b, xin,
                                                   use_reentrant=False))
    _compare_block(ck, plain, r["dout"], "checkpointed block",
                   bias_exact=True)
    _compare_block(ck, r["ref"], r["dout"], "checkpointed block vs unfused",
                   bias_exact=False)


def test_block_fused_in_graphed_step():
    """Captured into a hipGraph, the fused block replays to the eager
    result: nothing in it syncs with the host."""
    from torchdistpackage_amd.utils_graph import GraphedStep
    r = _block_ref()
    eager = _run_block(r["blk"], r["x"], r["dout"], fused=True)
    blk, dout = r["blk"], r["dout"]
    assert ops.fused_residual_enabled()
    xin = r["x"].detach().clone().requires_grad_(True)
    box = {}

    def step():
        for t in [xin, *blk.parameters()]:
            if t.grad is not None:
                t.grad.zero_()
        out = blk(xin)
        out.backward(dout)
        box["out"] = out.detach()

    for p in blk.parameters():
        p.grad = None
    gs = GraphedStep(step, warmup=2)
    for _ in range(2):
        gs.replay()
    torch.cuda.synchronize()
    out_e, dx_e, grads_e, _ = eager
    nh.check_equal(box["out"], out_e, "graphed out")
    nh.check_equal(xin.grad, dx_e, "graphed dx")
    for n, p in blk.named_parameters():
        nh.check_equal(p.grad, grads_e[n], f"graphed d{n}")
