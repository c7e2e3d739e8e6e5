"""CPU side of the hard-input numerics suite.

Runs every input family of tests/numerics_helpers.py through the CPU paths
of ``ops.*`` with the same yardstick the GPU file uses (fp64 reference,
torch's fp32 CPU op as ``lib``).  That proves the families and floors can
be met by a correct implementation, and guards the CPU oracles themselves.
The teeth check at the end keeps the floors honest: the one-pass LayerNorm
variance, applied to every row as the HIP kernels once did, must fail them.
"""

import math

import pytest
import torch
import torch.nn.functional as F

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

CPU = "cpu"
DTYPES = [torch.bfloat16, torch.float32]
EPS_LN, EPS_RMS = 1e-5, 1e-6


def _norm_cases():
    for dtype in DTYPES:
        for fam in nh.norm_families(dtype):
            for shape in nh.NORM_SHAPES:
                yield pytest.param(fam, shape, dtype,
                                   id=f"{fam}-{shape[0]}x{shape[1]}-"
                                      f"{nh.dtype_name(dtype)}")


@pytest.mark.parametrize("family,shape,dtype", list(_norm_cases()))
def test_layer_norm_cpu(family, shape, dtype):
    x, w, b, dy = nh.norm_input(family, *shape, dtype)
    D = shape[1]
    nh.check_fwd_bwd(
        lambda x, w, b: ops.layer_norm(x, w, b, EPS_LN),
        lambda x, w, b: F.layer_norm(x, (D,), w, b, EPS_LN),
        lambda x, w, b: F.layer_norm(x, (D,), w, b, EPS_LN),
        (x, w, b), dy, "xwb", dtype, CPU, torch.float32,
        f"layer_norm[{family} {shape} {nh.dtype_name(dtype)}]")


@pytest.mark.parametrize("family,shape,dtype", list(_norm_cases()))
def test_rms_norm_cpu(family, shape, dtype):
    x, w, _, dy = nh.norm_input(family, *shape, dtype)
    nh.check_fwd_bwd(
        lambda x, w: ops.rms_norm(x, w, EPS_RMS),
        lambda x, w: nh.rms_norm_formula(x, w, EPS_RMS),
        lambda x, w: nh.rms_norm_formula(x, w, EPS_RMS),
        (x, w), dy, "xw", dtype, CPU, torch.float32,
        f"rms_norm[{family} {shape} {nh.dtype_name(dtype)}]")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=nh.dtype_name)
def test_bias_gelu_cpu(family, dtype):
    shape = (7, 512)
    x = nh.act_input(family, shape, dtype)
    bias = nh.act_bias("gelu", (shape[1],), dtype)
    dy = nh.act_other("dy", shape, dtype)
    what = f"bias_gelu[{family} {nh.dtype_name(dtype)}]"
    nh.check_fwd_bwd(ops.bias_gelu, lambda x, b: nh.gelu_tanh(x + b),
                     lambda x, b: nh.gelu_tanh(x + b), (x, bias), dy,
                     ("x", "bias"), dtype, CPU, torch.float32, what)
    shape = (3, 1001)
    x = nh.act_input(family, shape, dtype)
    dy = nh.act_other("dy", shape, dtype)
    nh.check_fwd_bwd(ops.bias_gelu, nh.gelu_tanh, nh.gelu_tanh, (x,), dy,
                     ("x",), dtype, CPU, torch.float32, what + " no bias")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
def test_batched_bias_gelu_cpu(family):
    E, N, H = 3, 5, 72
    dtype = torch.bfloat16
    x = nh.act_input(family, (E, N, H), dtype)
    bias = nh.act_bias("bgelu", (E, H), dtype)
    dy = nh.act_other("dy", (E, N, H), dtype)
    fn = lambda x, b: nh.gelu_tanh(x + b.unsqueeze(1))  # noqa: E731
    nh.check_fwd_bwd(ops.batched_bias_gelu, fn, fn, (x, bias), dy,
                     ("x", "bias"), dtype, CPU, torch.float32,
                     f"batched_bias_gelu[{family}]")


@pytest.mark.parametrize("family", nh.ACT_FAMILIES)
def test_swiglu_cpu(family):
    shape = (5, 264)
    dtype = torch.bfloat16
    a = nh.act_input(family, shape, dtype)
    b = nh.act_other("gate", shape, dtype)
    dy = nh.act_other("dy", shape, dtype)
    fn = lambda a, b: F.silu(a) * b  # noqa: E731
    nh.check_fwd_bwd(ops.swiglu, fn, fn, (a, b), dy, "ab", dtype, CPU,
                     torch.float32, f"swiglu[{family}]")


@pytest.mark.parametrize("family", nh.CE_FAMILIES)
@pytest.mark.parametrize("shape", nh.CE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy_cpu(family, shape):
    x, t, masked = nh.ce_input(family, *shape)
    what = f"cross_entropy[{family} {shape}]"
    loss_ref, dl_ref, _ = nh.ce_ref(x, t)
    one = torch.tensor(1.0)
    loss, (dl,) = nh.fwd_bwd(lambda l: ops.cross_entropy_loss(l, t), (x,),
                             one, torch.bfloat16, CPU)
    loss_lib, (dl_lib,) = nh.fwd_bwd(lambda l: F.cross_entropy(l, t), (x,),
                                     one, torch.float32, CPU)
    nh.yardstick(loss, loss_ref, loss_lib, nh.FLOOR_CE_LOSS, absolute=True,
                 what=what + " loss")
    nh.yardstick(dl, dl_ref, dl_lib, nh.FLOOR_BF16_GRAD,
                 what=what + " dlogits")
    assert (dl[masked] == 0).all(), f"{what}: gradient at a -inf logit"


@pytest.mark.parametrize("family", nh.ATTN_FAMILIES)
@pytest.mark.parametrize("shape", nh.ATTN_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_flash_attention_cpu(family, shape, causal):
    q, k, v, do = nh.attn_input(family, *shape)
    scale = 1.0 / math.sqrt(shape[-1])
    tiny = None
    if family == "uniform":     # exact dq is 0: see attn_dq_cancel_scale
        tiny = {"q": nh.attn_dq_cancel_scale(q, k, v, do, causal, scale)}
    fn = lambda q, k, v: nh.attn_chain(q, k, v, causal, scale)  # noqa: E731
    nh.check_fwd_bwd(
        lambda q, k, v: ops.flash_attention(q, k, v, causal=causal),
        fn, fn, (q, k, v), do, "qkv", torch.bfloat16, CPU, torch.float32,
        f"flash_attention[{family} {shape} causal={causal}]", tiny=tiny)


def test_layer_norm_cpu_centred_rows_keep_one_pass_bits():
    """Rows with mean^2 <= var keep the plain mean / var(): the refinement
    must not move a single bit of y or of the saved statistics there."""
    x, w, b, _ = nh.norm_input("randn", 5, 768, torch.float32)
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    assert (mean * mean <= var).all()
    want = (x - mean) * torch.rsqrt(var + EPS_LN) * w + b
    assert torch.equal(ops.layer_norm(x, w, b, EPS_LN), want)


# ------------------------------------------------------------- teeth check

def _one_pass_yardstick(family, shape):
    dtype = torch.float32
    x, w, b, _ = nh.norm_input(family, *shape, dtype)
    D = shape[1]
    ref = F.layer_norm(x.double(), (D,), w.double(), b.double(), EPS_LN)
    lib = F.layer_norm(x, (D,), w, b, EPS_LN)
    got = nh.layer_norm_one_pass_fp32(x, w, b, EPS_LN)
    nh.yardstick(got, ref, lib, nh.FLOOR_FP32,
                 what=f"one-pass layer_norm[{family} {shape}]")


@pytest.mark.parametrize("shape", [(5, 768), (3, 1027)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_pass_variance_fails_the_yardstick(shape):
    """var = E[x^2] - E[x]^2 in fp32 passes on centred rows and must FAIL on
    the two off-centre families; if it ever passes, a floor was loosened."""
    _one_pass_yardstick("randn", shape)
    for family in ("shift1000", "near_const"):
        with pytest.raises(AssertionError):
            _one_pass_yardstick(family, shape)
