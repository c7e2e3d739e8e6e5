"""The W8A16 GEMV kernel (csrc/gemv_int8.hip), its dispatch (ops/int8.py) and
int8-converted models on the GPU.

- exact family: integer x, full-range q, power-of-two scales and integer
  bias make every fp32 operation exact, so the output must equal the fp64
  value rounded once to bf16, bit for bit, through every MT arm and K edge
- selection: one-hot x rows return scale * q columns exactly, which pins the
  byte order of the int8 unpack across a 16-byte load
- locality and bounds: a NaN stays in its row / column; operands carved out
  of NaN-margined allocations give unchanged, finite results
- precision: per-element error against torch's fp32 matmul on the
  dequantised weight
- dispatch: kernel route, dequantise route, the TDPA_INT8_GEMV switch
- models: decode logits against the dequantised-bf16 twin, graphed against
  eager generation, resident bytes

Run on MI355X via: pytest tests/test_int8_linear_gpu.py -m gpu -q
"""

import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.ops import int8 as int8_ops
from torchdistpackage_amd.ops.gemm import linear
from torchdistpackage_amd.ops.int8 import (Int8Weight, int8_linear,
                                           is_int8_linear, quantize_int8,
                                           quantize_linears_)
from torchdistpackage_amd.parallel.tensor.tp_utils import TpLinear

from tests import numerics_helpers as nh

BF16 = torch.bfloat16
LINEAR_TYPES = (TpLinear, nn.Linear)


def _dev():
    return torch.device("cuda")


def _kernel(x, q, scale, bias=None):
    return ops.ext("gemv_w8a16").gemv_w8a16(x, q, scale, bias)


# ------------------------------------------------------------ exact family
#
# q uniform over [-127, 127], x integers in [-4, 4], scale[n] = 2**-k with k
# in 0..6, bias integers in [-4, 4], K <= 8192.  |sum| <= 127 * 4 * 8192
# < 2**22 and |sum + bias * 2**k| < 2**24 are integers, so fp32 accumulation
# is exact in any order, the power-of-two scale is exact, and the only
# rounding is the final fp32 -> bf16.
#
# (M, N, K).  MT arms 1, 2, 4 (M=3 padded), 8 (M=5 padded), 16 (M=9 padded),
# 32 (M=17 padded).  A lane's 16-byte load carries 16 weights, so a wave
# covers 1024 of K per load ("chunk"); the x tile is KT = 2048 for MT <= 16
# (two chunks per lane and tile) and 1024 for MT = 32 (one).  1024 / 1040 sit
# on and 16 past the chunk edge (for MT = 32 also the tile edge), 2048 / 2064
# / 4112 on and 16 past a tile edge for MT <= 16 (2064 = two tiles and one
# chunk past for MT = 32); K = 16 and 32 leave all but one or two lanes idle;
# 8192 is the largest exact K.  Odd N ends on the ``n0 + 1 == N`` wave, N = 1
# is that wave alone, N = 1000 is many blocks.
EXACT_MAX_K = 8192
INT8_GEMV_SHAPES = [
    (1, 1, 16), (1, 7, 2048), (1, 1000, 2064), (1, 9, 1040),
    (2, 9, 32), (2, 8, 2048), (2, 7, 4112), (2, 3, 1024),
    (3, 1, 2064), (3, 9, 2048), (4, 1000, 4112), (4, 2, 1024), (4, 7, 1040),
    (5, 7, 2048), (8, 9, 2064), (8, 1, 16), (8, 1000, 1040), (8, 2, 8192),
    (9, 7, 2064), (9, 8, 2048), (16, 9, 4112), (16, 1, 32), (16, 7, 1040),
    (17, 9, 1024), (17, 7, 1040), (32, 9, 1040), (32, 1, 1024),
    (32, 1000, 2064), (32, 2, 16),
]


def _exact_operands(M, N, K):
    assert K <= EXACT_MAX_K
    g = nh._gen("int8-exact", M, N, K)
    q = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
    if N * K >= 254:                    # the extremes are really there
        q.view(-1)[0], q.view(-1)[-1] = 127, -127
    x = nh.int_mat("int8-x", (M, K))
    scale = 2.0 ** -torch.randint(0, 7, (N,), generator=g).float()
    bias = nh.int_mat("int8-b", (N,))
    return x, q, scale, bias


def exact_w8a16_ref(x, q, scale, bias=None):
    """bf16( scale * (x @ q^T) [+ bias] ) from fp64, rounded once: the
    construction of ``nh.exact_mm_ref``."""
    r = (x.double().cpu() @ q.double().cpu().t()) * scale.double().cpu()
    if bias is not None:
        r = r + bias.double().cpu()
    return r.to(BF16)


@pytest.mark.parametrize("shape", INT8_GEMV_SHAPES, ids=nh.gemv_id)
def test_exact_w8a16(shape):
    x, q, scale, bias = _exact_operands(*shape)
    xd, qd, sd, bd = (t.to(_dev()) for t in (x, q, scale, bias))
    nh.check_equal(_kernel(xd, qd, sd), exact_w8a16_ref(x, q, scale),
                   f"w8a16 {shape}")
    nh.check_equal(_kernel(xd, qd, sd, bd),
                   exact_w8a16_ref(x, q, scale, bias), f"w8a16 {shape} +bias")


# --------------------------------------------------------------- selection

# K = 16 / 32 with M = K: every byte of a 16-byte load is selected once
SELECTION = [(16, 7, 16), (32, 9, 32), (8, 9, 2064), (32, 5, 1040)]


@pytest.mark.parametrize("M,N,K", SELECTION)
def test_selection_returns_scaled_columns_of_q(M, N, K):
    x, idx = nh.selection_matrix("int8", M, K)
    g = nh._gen("int8-sel", M, N, K)
    w = torch.randn(N, K, generator=g)
    q, scale = quantize_int8(w)
    # distinct values along K, so that a swapped byte cannot go unnoticed
    q[0] = ((torch.arange(K) * 37) % 255 - 127).to(torch.int8)
    got = _kernel(x.to(_dev()), q.to(_dev()), scale.to(_dev()))
    want = (scale[:, None] * q.float()).t()[idx].to(BF16).contiguous()
    nh.check_equal(got, want, f"w8a16 selection {(M, N, K)}")


# --------------------------------------------------- locality and bounds

def test_nan_in_x_row_stays_in_that_row():
    M, N, K = 5, 9, 2064
    x, q, scale, bias = _exact_operands(M, N, K)
    ref = exact_w8a16_ref(x, q, scale, bias)
    x = x.clone()
    x[3, K - 1] = float("nan")
    got = _kernel(*(t.to(_dev()) for t in (x, q, scale, bias))).cpu()
    assert torch.isnan(got[3]).all()
    keep = torch.arange(M) != 3
    nh.check_equal(got[keep], ref[keep], "w8a16 NaN in x row 3, other rows")


def test_nan_in_scale_stays_in_that_column():
    M, N, K = 5, 9, 2064
    x, q, scale, bias = _exact_operands(M, N, K)
    ref = exact_w8a16_ref(x, q, scale, bias)
    scale = scale.clone()
    scale[4] = float("nan")
    got = _kernel(*(t.to(_dev()) for t in (x, q, scale, bias))).cpu()
    assert torch.isnan(got[:, 4]).all()
    keep = torch.arange(N) != 4
    nh.check_equal(got[:, keep].contiguous(), ref[:, keep].contiguous(),
                   "w8a16 NaN in scale[4], other columns")


@pytest.mark.parametrize("shape", [(5, 9, 2064), (32, 7, 1040), (1, 1, 16)],
                         ids=nh.gemv_id)
def test_operands_carved_from_nan_margins(shape):
    """x, q, scale and bias sit in the middle of larger allocations whose
    margins are NaN (q: 127, which a stray read would multiply with the NaN
    that follows x's last row)."""
    M, N, K = shape
    x, q, scale, bias = _exact_operands(M, N, K)
    ref = exact_w8a16_ref(x, q, scale, bias)
    nan = float("nan")
    xb = torch.full((M * K + 4096,), nan, dtype=BF16, device=_dev())
    qb = torch.full((N * K + 8192,), 127, dtype=torch.int8, device=_dev())
    sb = torch.full((N + 64,), nan, dtype=torch.float32, device=_dev())
    bb = torch.full((N + 64,), nan, dtype=BF16, device=_dev())
    xd = xb[2048:2048 + M * K].view(M, K)          # 16-byte aligned offsets
    qd = qb[4096:4096 + N * K].view(N, K)
    sd, bd = sb[31:31 + N], bb[33:33 + N]
    xd.copy_(x), qd.copy_(q), sd.copy_(scale), bd.copy_(bias)
    got = _kernel(xd, qd, sd, bd)
    assert torch.isfinite(got).all()
    nh.check_equal(got, ref, f"w8a16 carved {shape}")
    assert torch.isnan(xb[:2048]).all() and torch.isnan(xb[2048 + M * K:]).all()
    assert (qb[:4096] == 127).all() and (qb[4096 + N * K:] == 127).all()


# ---------------------------------------------------------------- precision

PRECISION = [(1, 1000, 4112), (4, 9, 8192), (8, 1000, 2064), (32, 9, 1040)]


@functools.lru_cache(maxsize=None)
def _quantised(wfam, N, K):
    """int8 weight from randn rows or rows with scales 2**-6 .. 2**6."""
    _, B = nh.mm_input(wfam, 1, N, K)
    return quantize_int8(B.float())


def _oracle(x, q, scale, bias=None):
    """fp64 (ref, mag) from x and the exact q * scale."""
    w64 = q.double().cpu() * scale.double().cpu()[:, None]
    x64 = x.double().cpu().reshape(-1, x.shape[-1])
    ref, mag = x64 @ w64.t(), x64.abs() @ w64.abs().t()
    if bias is not None:
        ref = ref + bias.double().cpu()
        mag = mag + bias.double().cpu().abs()
    return ref, mag


@pytest.mark.parametrize("wfam", ["randn", "wide"])
@pytest.mark.parametrize("xfam", ["randn", "shift", "wide"])
@pytest.mark.parametrize("M,N,K", PRECISION)
def test_precision_vs_fp32_matmul(M, N, K, xfam, wfam):
    x, _ = nh.mm_input(xfam, M, 1, K)
    q, scale = _quantised(wfam, N, K)
    ref, mag = _oracle(x, q, scale)
    xd, qd, sd = x.to(_dev()), q.to(_dev()), scale.to(_dev())
    lib = (xd.float() @ (qd.float() * sd[:, None]).t()).to(BF16)
    got = _kernel(xd, qd, sd)
    nh.mm_check(got, lib, ref, mag, f"w8a16[x {xfam}, w {wfam} {M}x{N}x{K}]")


# ----------------------------------------------------------------- dispatch

@pytest.mark.parametrize("M", [1, 6, 32])
def test_linear_takes_the_kernel_up_to_m32(M):
    N, K = 1000, 2064
    x, _ = nh.mm_input("randn", M, 1, K)
    q, scale = _quantised("randn", N, K)
    b = nh.act_other("int8-bias", (N,), BF16)
    xd, qd, sd, bd = (t.to(_dev()) for t in (x, q, scale, b))
    W = Int8Weight(qd, sd)
    with torch.no_grad():
        nh.check_equal(linear(xd, W, bd), _kernel(xd, qd, sd, bd),
                       f"linear(Int8Weight) M={M} +bias")
        nh.check_equal(linear(xd, W), _kernel(xd, qd, sd),
                       f"linear(Int8Weight) M={M}")
        if M % 2 == 0:
            y = linear(xd.view(2, M // 2, K), W, bd)
            nh.check_equal(y, _kernel(xd, qd, sd, bd).view(2, M // 2, N),
                           f"linear(Int8Weight) 3-D M={M}")


@pytest.mark.parametrize("M,N,K", [(33, 40, 2064), (256, 256, 1024),
                                   (4, 24, 40)])
def test_dequantise_route(M, N, K, monkeypatch):
    """M > 32 and K % 16 != 0 never reach the kernel."""
    def no_kernel(*a, **k):
        raise AssertionError("the int8 kernel was called")

    x, _ = nh.mm_input("randn", M, 1, K)
    q, scale = _quantised("randn", N, K)
    b = nh.act_other("int8-bias", (N,), BF16)
    ref, mag = _oracle(x, q, scale, b)
    xd, qd, sd, bd = (t.to(_dev()) for t in (x, q, scale, b))
    W = Int8Weight(qd, sd)
    lib = F.linear(xd, W.dequantize(BF16), bd)
    monkeypatch.setattr(int8_ops, "ext", lambda *_: type(
        "NoExt", (), {"gemv_w8a16": staticmethod(no_kernel)}))
    with torch.no_grad():
        got = linear(xd, W, bd)
    assert got.dtype == BF16 and got.shape == (M, N)
    nh.mm_check(got, lib, ref, mag, f"int8 dequantise route {M}x{N}x{K}")


def test_switch_forces_the_dequantise_route():
    M, N, K = 4, 1000, 2064
    x, _ = nh.mm_input("randn", M, 1, K)
    q, scale = _quantised("randn", N, K)
    xd, qd, sd = x.to(_dev()), q.to(_dev()), scale.to(_dev())
    W = Int8Weight(qd, sd)
    with torch.no_grad():
        want = linear(xd, W.dequantize(BF16))
        kern = linear(xd, W)
        prev = int8_ops.set_int8_gemv(False)
        try:
            assert not int8_ops.int8_gemv_enabled()
            off = linear(xd, W)
        finally:
            int8_ops.set_int8_gemv(prev)
        again = linear(xd, W)
    nh.check_equal(off, want, "TDPA_INT8_GEMV=0: the bf16 route on q*scale")
    nh.check_equal(again, kern, "switch restored")
    nh.check_equal(kern, _kernel(xd, qd, sd), "switch on: the kernel")
    # the two routes round differently (bf16 weight vs exact q * scale)
    assert not torch.equal(off, kern)


def test_launcher_argument_checks():
    x, q, scale, bias = (t.to(_dev()) for t in _exact_operands(2, 8, 32))
    bad = [
        (x.float(), q, scale, None),                       # x dtype
        (x, q.to(torch.int16), scale, None),               # q dtype
        (x, q, scale.double(), None),                      # scale dtype
        (x, q, scale[:-1], None),                          # scale numel
        (x, q, scale, bias.float()),                       # bias dtype
        (x, q, scale, bias[:-1]),                          # bias numel
        (x[:, ::2], q[:, ::2], scale, None),               # not contiguous
        (x[:, :24].contiguous(), q[:, :24].contiguous(), scale, None),  # K
        (x.repeat(17, 1), q, scale, None),                 # M = 34
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            _kernel(*args)


# ------------------------------------------------------------------- models

def _linears(model):
    return [(n, m) for n, m in model.named_modules()
            if isinstance(m, LINEAR_TYPES)]


def _randomise_biases(model):
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, LINEAR_TYPES) and m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))


@functools.lru_cache(maxsize=None)
def _models(family):
    """(converted model, twin whose linears hold the dequantised bf16
    weights), tiny bf16 configs of tests/test_generate_gpu.py."""
    torch.manual_seed(0)
    if family == "gpt2":
        from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
        cfg = GPT2Config(vocab_size=50304, n_layer=4, n_head=8, dim=512,
                         max_seq=64)
        m = GPT2Model(cfg, device="cuda", dtype=BF16).eval()
    else:
        from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel
        cfg = LlamaConfig(vocab_size=2048, n_layer=3, n_head=8, n_kv_head=2,
                          dim=512, ffn_dim=1024, max_seq=64)
        m = LlamaModel(cfg, device="cuda", dtype=BF16).eval()
    _randomise_biases(m)
    twin = copy.deepcopy(m)
    n = quantize_linears_(m)
    assert n == len(_linears(twin)) > 0
    with torch.no_grad():
        for (_, a), (_, b) in zip(_linears(m), _linears(twin)):
            b.weight.copy_(a.weight.dequantize(BF16))
    return m, twin


def _decode_logits(model, toks):
    from torchdistpackage_amd.inference.generate import (_alloc_caches,
                                                         decode_forward)
    B, T = toks.shape
    caches = _alloc_caches(model, B, T)
    out = [decode_forward(model, toks[:, :8], caches, 0).float()]
    for p in range(8, T):
        out.append(decode_forward(model, toks[:, p:p + 1], caches,
                                  p).float())
    return out


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_decode_logits_match_dequantised_twin(family):
    m, twin = _models(family)
    toks = torch.randint(0, m.cfg.vocab_size, (2, 24), device="cuda",
                         generator=torch.Generator("cuda").manual_seed(1))
    worst = 0.0
    for p, (a, b) in enumerate(zip(_decode_logits(m, toks),
                                   _decode_logits(twin, toks))):
        assert torch.isfinite(a).all()
        diff = (a - b).abs().max().item()
        worst = max(worst, diff)
        assert diff < 0.25, (p, diff)     # bf16 logits, two orders
    print(f"NUMERICS int8 {family} decode logits vs twin: max diff "
          f"{worst:.4f} (bound 0.25)")


@pytest.mark.parametrize("attn_impl", ["hip", "sdpa"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_graphed_decoder_vs_eager_on_converted_model(family, attn_impl):
    from torchdistpackage_amd.inference import (GraphedGPT2Decoder,
                                                GraphedLlamaDecoder, generate)
    m, _ = _models(family)
    Dec = GraphedGPT2Decoder if family == "gpt2" else GraphedLlamaDecoder
    idx = torch.randint(0, m.cfg.vocab_size, (2, 8), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(2))
    dec = Dec(m, batch=2, max_seq=48, attn_impl=attn_impl)
    out_g = dec.generate(idx, 24)
    out_e = generate(m, idx, 24, attn_impl=attn_impl)
    assert out_g.shape == out_e.shape == (2, 32)
    assert torch.equal(out_g[:, :12], out_e[:, :12])
    agree = (out_g == out_e).float().mean().item()
    assert agree >= 0.8, agree


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_converted_linears_hold_int8_bytes(family):
    m, twin = _models(family)
    for (name, a), (_, b) in zip(_linears(m), _linears(twin)):
        assert is_int8_linear(a), name
        N, K = b.weight.shape
        held = sum(t.numel() * t.element_size()
                   for k, t in a._buffers.items()
                   if k in ("qweight", "weight_scale"))
        assert held == N * K + 4 * N, name
        assert "weight" not in a._parameters
        assert a.weight.nbytes() == held
        assert a.qweight.is_cuda and a.weight_scale.is_cuda
