"""HIP kernels on hard inputs vs fp64, with torch's own op in the same dtype
as the yardstick.  Families, shapes, floors and the yardstick live in
tests/numerics_helpers.py; docs/design/kernels.md ("Numerics on hard
inputs") has the table and the measured errors.

Run on MI355X via: pytest tests/test_ops_numerics_gpu.py -m gpu -q
"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

DTYPES = [torch.bfloat16, torch.float32]
EPS_LN, EPS_RMS = 1e-5, 1e-6


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"


def _norm_cases(extra_bf16_shape=None):
    for dtype in DTYPES:
        shapes = list(nh.NORM_SHAPES)
        if extra_bf16_shape and dtype == torch.bfloat16:
            shapes.append(extra_bf16_shape)
        for fam in nh.norm_families(dtype):
            for shape in shapes:
                yield pytest.param(fam, shape, dtype,
                                   id=f"{fam}-{shape[0]}x{shape[1]}-"
                                      f"{nh.dtype_name(dtype)}")


# ------------------------------------------------------------------- norms

@pytest.mark.parametrize("family,shape,dtype",
                         list(_norm_cases(nh.BF16_V8_SHAPE)))
def test_layer_norm(family, shape, dtype):
    x, w, b, dy = nh.norm_input(family, *shape, dtype)
    D = shape[1]
    what = f"layer_norm[{family} {shape} {nh.dtype_name(dtype)}]"

    # saved statistics straight from the kernel
    xd, wd, bd = (t.to(_dev()) for t in (x, w, b))
    _, mean, rstd = ops.ext("layer_norm").layernorm_fwd(xd, wd, bd, EPS_LN)
    mean_ref, rstd_ref = nh.layer_norm_stats_ref(x, EPS_LN)
    mean_lib, rstd_lib = nh.layer_norm_stats_two_pass_fp32(xd, EPS_LN)
    nh.yardstick(mean, mean_ref, mean_lib, nh.FLOOR_STATS,
                 what=what + " mean")
    nh.yardstick(rstd, rstd_ref, rstd_lib, nh.FLOOR_STATS,
                 what=what + " rstd")

    nh.check_fwd_bwd(
        lambda x, w, b: ops.layer_norm(x, w, b, EPS_LN),
        lambda x, w, b: F.layer_norm(x, (D,), w, b, EPS_LN),
        lambda x, w, b: F.layer_norm(x, (D,), w, b, EPS_LN),
        (x, w, b), dy, "xwb", dtype, _dev(), dtype, what)


@pytest.mark.parametrize("family,shape,dtype",
                         list(_norm_cases(nh.BF16_V8_SHAPE)))
def test_rms_norm(family, shape, dtype):
    x, w, _, dy = nh.norm_input(family, *shape, dtype)
    D = shape[1]
    what = f"rms_norm[{family} {shape} {nh.dtype_name(dtype)}]"

    xd, wd = x.to(_dev()), w.to(_dev())
    _, rstd = ops.ext("rms_norm").rmsnorm_fwd(xd, wd, EPS_RMS)
    rstd_ref = torch.rsqrt(x.double().pow(2).mean(-1) + EPS_RMS)
    rstd_lib = torch.rsqrt(xd.float().pow(2).mean(-1) + EPS_RMS)
    nh.yardstick(rstd, rstd_ref, rstd_lib, nh.FLOOR_STATS,
                 what=what + " rstd")

    nh.check_fwd_bwd(
        lambda x, w: ops.rms_norm(x, w, EPS_RMS),
        lambda x, w: F.rms_norm(x, (D,), w, EPS_RMS),
        lambda x, w: nh.rms_norm_formula(x, w, EPS_RMS),
        (x, w), dy, "xw", dtype, _dev(), dtype, what)


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (2050, 64)),
                                         (torch.bfloat16, (2050, 68))],
                         ids=["fp32-2050x64", "bf16-2050x68"])
def test_norm_backward_dw_is_deterministic(dtype, shape):
    """Outside the bf16 register path dw and db are summed in a fixed order
    (they once went through 2048-deep fp32 atomics and moved from run to
    run): repeated calls must agree in every bit."""
    x, w, _, dy = nh.norm_input("outlier_last", *shape, dtype)
    x, w, dy = (t.to(_dev()) for t in (x, w, dy))
    e = ops.ext("norms")
    mean = x.float().mean(-1)
    rstd = torch.rsqrt(x.float().var(-1, unbiased=False) + EPS_LN)
    first = None
    for _ in range(4):
        got = e.rmsnorm_bwd(dy, x, w, rstd)[1:] + \
            e.layernorm_bwd(dy, x, w, mean, rstd)[1:]
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert torch.equal(a, b)


# ------------------------------------------------------------- activations

@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=nh.dtype_name)
def test_bias_gelu_with_bias(family, dtype):
    shape = (7, 512)
    x = nh.act_input(family, shape, dtype)
    bias = nh.act_bias("gelu", (shape[1],), dtype)
    dy = nh.act_other("dy", shape, dtype)
    fn = lambda x, b: nh.gelu_tanh(x + b)  # noqa: E731
    nh.check_fwd_bwd(ops.bias_gelu, fn, fn, (x, bias), dy, ("x", "bias"),
                     dtype, _dev(), dtype,
                     f"bias_gelu[{family} {shape} {nh.dtype_name(dtype)}]")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=nh.dtype_name)
def test_bias_gelu_no_bias_tail(family, dtype):
    """numel % 8 != 0: the scalar tail of the bf16 kernels."""
    shape = (3, 1001)
    x = nh.act_input(family, shape, dtype)
    dy = nh.act_other("dy", shape, dtype)
    nh.check_fwd_bwd(ops.bias_gelu, nh.gelu_tanh, nh.gelu_tanh, (x,), dy,
                     ("x",), dtype, _dev(), dtype,
                     f"bias_gelu[{family} {shape} {nh.dtype_name(dtype)} "
                     f"no bias]")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
def test_bias_gelu_no_bias_above_grid_cap(family):
    """4104 x 1024 bf16 elements is just above the 2048 * 256 * 8 one pass
    of the capped grid covers, so the stride loop runs.  The op is
    elementwise: the first, a middle and the last row are compared."""
    shape, dtype = (4104, 1024), torch.bfloat16
    assert shape[0] * shape[1] > 2048 * 256 * 8
    rows = [0, shape[0] // 2, shape[0] - 1]
    x = nh.act_input(family, shape, dtype)
    dy = nh.act_other("dy", shape, dtype)
    y, (dx,) = nh.fwd_bwd(ops.bias_gelu, (x,), dy, dtype, _dev())
    y_ref, (dx_ref,) = nh.fwd_bwd(nh.gelu_tanh, (x[rows],), dy[rows],
                                  torch.float64, "cpu")
    y_lib, (dx_lib,) = nh.fwd_bwd(nh.gelu_tanh, (x[rows],), dy[rows],
                                  dtype, _dev())
    what = f"bias_gelu[{family} {shape} bf16 no bias]"
    f_fwd, f_grad = nh.floors(dtype)
    nh.yardstick(y[rows], y_ref, y_lib, f_fwd, what=what + " y")
    nh.yardstick(dx[rows], dx_ref, dx_lib, f_grad, what=what + " dx")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
def test_batched_bias_gelu(family):
    E, N, H = 3, 5, 72
    dtype = torch.bfloat16
    x = nh.act_input(family, (E, N, H), dtype)
    bias = nh.act_bias("bgelu", (E, H), dtype)
    dy = nh.act_other("dy", (E, N, H), dtype)
    fn = lambda x, b: nh.gelu_tanh(x + b.unsqueeze(1))  # noqa: E731
    nh.check_fwd_bwd(ops.batched_bias_gelu, fn, fn, (x, bias), dy,
                     ("x", "bias"), dtype, _dev(), dtype,
                     f"batched_bias_gelu[{family} {(E, N, H)}]")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
def test_swiglu(family):
    shape, dtype = (5, 264), torch.bfloat16
    a = nh.act_input(family, shape, dtype)
    b = nh.act_other("gate", shape, dtype)
    dy = nh.act_other("dy", shape, dtype)
    fn = lambda a, b: F.silu(a) * b  # noqa: E731
    nh.check_fwd_bwd(ops.swiglu, fn, fn, (a, b), dy, "ab", dtype, _dev(),
                     dtype, f"swiglu[{family} {shape}]")


# ----------------------------------------------------------- cross-entropy

@pytest.mark.parametrize("family", nh.CE_FAMILIES)
@pytest.mark.parametrize("shape", nh.CE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy(family, shape):
    x, t, masked = nh.ce_input(family, *shape)
    what = f"cross_entropy[{family} {shape}]"
    loss_ref, dl_ref, lse_ref = nh.ce_ref(x, t)
    td = t.to(_dev())
    one = torch.tensor(1.0)

    loss, (dl,) = nh.fwd_bwd(lambda l: ops.cross_entropy_loss(l, td), (x,),
                             one, torch.bfloat16, _dev())
    loss_lib, (dl_lib,) = nh.fwd_bwd(
        lambda l: F.cross_entropy(l.float(), td), (x,), one, torch.bfloat16,
        _dev())
    nh.yardstick(loss, loss_ref, loss_lib, nh.FLOOR_CE_LOSS, absolute=True,
                 what=what + " loss")
    nh.yardstick(dl, dl_ref, dl_lib, nh.FLOOR_BF16_GRAD,
                 what=what + " dlogits")
    assert (dl.cpu()[masked] == 0).all(), \
        f"{what}: gradient at a -inf logit"

    # per-row lse of the fused forward
    xd = x.to(_dev())
    lse_lib = torch.logsumexp(xd.float(), -1)
    _, lse = ops.ext("cross_entropy").ce_fwd(xd, td)
    nh.yardstick(lse, lse_ref, lse_lib, nh.FLOOR_LSE, absolute=True,
                 what=what + " lse")

    # vocab-parallel primitive: half the targets live on another shard
    tp = t.clone()
    tp[::2] = -1
    lse_p, tgt_p = ops.ext("ce_partial").ce_partial_fwd(xd, tp.to(_dev()))
    nh.yardstick(lse_p, lse_ref, lse_lib, nh.FLOOR_LSE, absolute=True,
                 what=what + " partial lse")
    picked = x.double().gather(-1, tp.clamp_min(0).unsqueeze(-1)).squeeze(-1)
    tgt_ref = torch.where(tp >= 0, picked, torch.zeros_like(picked))
    nh.yardstick(tgt_p, tgt_ref, tgt_ref.float().to(_dev()), nh.FLOOR_LSE,
                 absolute=True, what=what + " partial target logit")


# --------------------------------------------------------------- attention

# Cases the head-dim-128 backward misses and that were not fixed with the
# tests (docs/design/kernels.md, "Numerics on hard inputs").  Figures are
# e(got) / e(lib) measured on MI355X; the bound is 2.5 * e(lib).
_ATTN_XFAIL = {
    ("dominant_key", (1, 2, 2, 100, 128), True):
        "dk e(got)=1.153e-02 vs e(lib)=4.414e-03 (bound 1.104e-02); "
        "dq 1.651e-02 vs 7.012e-03 passes",
    ("dominant_key", (1, 2, 2, 100, 128), False):
        "dq e(got)=1.890e-02 vs e(lib)=6.154e-03 (bound 1.539e-02)",
}


def _attn_cases():
    for causal in (True, False):
        for shape in nh.ATTN_SHAPES:
            for fam in nh.ATTN_FAMILIES:
                reason = _ATTN_XFAIL.get((fam, shape, causal))
                marks = [pytest.mark.xfail(strict=True, reason=reason)] \
                    if reason else []
                yield pytest.param(
                    fam, shape, causal, marks=marks,
                    id=f"{'causal' if causal else 'full'}-"
                       f"{'x'.join(map(str, shape))}-{fam}")


@pytest.mark.parametrize("family,shape,causal", list(_attn_cases()))
def test_flash_attention(family, shape, causal):
    q, k, v, do = nh.attn_input(family, *shape)
    scale = 1.0 / math.sqrt(shape[-1])
    what = f"flash_attention[{family} {shape} causal={causal}]"

    # lse: the kernel accumulates q.k in fp32, so the yardstick is fp32 math
    qd, kd, vd = (t.to(_dev()) for t in (q, k, v))
    _, lse = ops.ext("flash_attention").attn_fwd(
        qd, kd, vd, torch.empty_like(qd), causal, scale)
    lse_ref = nh.attn_lse(q.double(), k.double(), causal, scale)
    lse_lib = nh.attn_lse(qd.float(), kd.float(), causal, scale)
    nh.yardstick(lse, lse_ref, lse_lib, nh.FLOOR_LSE, absolute=True,
                 what=what + " lse")

    tiny = None
    if family == "uniform":     # exact dq is 0: see attn_dq_cancel_scale
        tiny = {"q": nh.attn_dq_cancel_scale(q, k, v, do, causal, scale)}
    fn = lambda q, k, v: nh.attn_chain(q, k, v, causal, scale)  # noqa: E731
    nh.check_fwd_bwd(
        lambda q, k, v: ops.flash_attention(q, k, v, causal=causal),
        fn, fn, (q, k, v), do, "qkv", torch.bfloat16, _dev(),
        torch.bfloat16, what, tiny=tiny)
