"""The W4A16 kernel, both arms (csrc/gemv_int4.hip), its dispatch (ops/int4.py) and
int4-converted models on the GPU: exact-integer family, one-hot selection,
NaN locality and bounds, precision, dispatch, models.

Run on MI355X via: pytest tests/test_int4_linear_gpu.py -m gpu -q
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.ops import int4 as int4_ops
from torchdistpackage_amd.ops.gemm import linear
from torchdistpackage_amd.ops.int4 import (Int4Weight, pack_int4,
                                           quantize_int4, unpack_int4)
from torchdistpackage_amd.ops.int8 import quantize_linears_
from torchdistpackage_amd.parallel.tensor.tp_utils import TpLinear

from tests import numerics_helpers as nh

BF16 = torch.bfloat16
LINEAR_TYPES = (TpLinear, nn.Linear)
DEV = "cuda"


def _kernel(x, packed, scale, bias=None, arm=0):
    return ops.ext("gemv_w4a16").gemv_w4a16(x, packed, scale, bias, arm)


# Exact family: q uniform over [-7, 7] with a -8 and a 7 planted, x integers
# in [-4, 4], scale[n, g] = 2**-k with k in 0..4, bias integers in [-4, 4],
# K <= 8192.  The conversion carries no offset.  The scaled sums are multiples
# of 2**-4 with |sum| <= 8 * 4 * 8192 = 2**18, below 2**22 units, so every
# fp32 partial (inside the MFMA or dot2, across groups, lanes and waves, plus
# bias) is exact in any order and the only rounding is the final fp32 -> bf16.
#
# (M, N, K); M <= 4 runs on BOTH arms through the binding (the crossover is
# M <= 2 -> dot2).  MFMA arm: 16 rows per workgroup (N = 7 below, 17 / 33 one
# past a multiple, 1 alone); 8 waves per workgroup below 512 workgroups, 4
# from there (N = 8200: 513); an instantiation for M <= 16 and one for
# M <= 32 (3, 5, 9, 17 padded); each wave takes one 128-k group per pass, so a
# pass is 1024 k at 8 waves and 512 k at 4; the x tile is 2048 k for M <= 16
# and 1024 k above.  The N = 8200 shapes take the 4-wave kernels through all
# four unrolled steps (K = 2048) and into a second and third tile.  dot2 arm:
# 2 rows per wave, 8 per workgroup (odd N, N = 1), 2048 k per wave load,
# x tile 4096 k, instantiations 1, 2, 4 (M = 3 padded).  Every K edge appears
# on and one group past: 512 / 640, 1024 / 1152, 2048 / 2176, 4096 / 4224.
INT4_SHAPES = [
    (1, 1, 128), (1, 7, 2048), (1, 1000, 2176), (1, 8200, 2048), (1, 9, 4224),
    (2, 17, 4096), (2, 7, 512), (2, 33, 4224), (2, 9, 8192),
    (3, 1, 2176), (3, 33, 2048), (4, 1000, 4224),
    (5, 7, 640), (5, 8200, 2176), (5, 17, 8192), (9, 7, 2176), (9, 16, 1024),
    (16, 17, 4224), (16, 1, 256), (16, 7, 1152),
    (17, 17, 1024), (17, 8200, 1152), (17, 1, 128), (17, 33, 2176),
    (32, 7, 128), (32, 1000, 2176), (32, 8200, 2176), (32, 16, 8192),
]


@functools.lru_cache(maxsize=None)
def _exact_operands(M, N, K):
    """(x, packed, scale, bias, bf16 reference with bias); read-only."""
    assert K <= 8192
    g = nh._gen("int4-exact", M, N, K)
    q = torch.randint(-7, 8, (N, K), generator=g).to(torch.int8)
    q.view(-1)[0], q.view(-1)[-1] = -8, 7
    x = nh.int_mat("int4-x", (M, K))
    scale = 2.0 ** -torch.randint(0, 5, (N, K // 128), generator=g).float()
    p, b = pack_int4(q), nh.int_mat("int4-b", (N,))
    return x, p, scale, b, _ref64(x, p, scale, b)[0].to(BF16)


def _ref64(x, packed, scale, bias=None):
    """fp64 (ref, mag) of the module formula from the torch unpack."""
    w = unpack_int4(packed.cpu()).double() * \
        scale.double().cpu().repeat_interleave(128, 1)
    x64 = x.double().cpu().reshape(-1, x.shape[-1])
    ref, mag = x64 @ w.t(), x64.abs() @ w.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double().cpu(), mag + bias.double().cpu().abs()
    return ref, mag


def _on_dev(*ts):
    return tuple(t.to(DEV) for t in ts)


@pytest.mark.parametrize("shape", INT4_SHAPES, ids=nh.gemv_id)
def test_exact_w4a16(shape):
    x, p, s, b, ref = _exact_operands(*shape)
    xd, pd, sd, bd = _on_dev(x, p, s, b)
    for arm in ((1, 2) if shape[0] <= 4 else (1,)):
        nh.check_equal(_kernel(xd, pd, sd, None, arm),
                       _ref64(x, p, s)[0].to(BF16), f"w4a16 {shape} arm {arm}")
        nh.check_equal(_kernel(xd, pd, sd, bd, arm), ref,
                       f"w4a16 {shape} arm {arm} +bias")


# (128, 9, 128): a permutation of all 128 k in four calls of M = 32 (MFMA arm)
# or 64 calls of M = 2 (dot2 arm), so every nibble of every lane's 16-byte
# load is selected once
@pytest.mark.parametrize("M,N,K,step", [(128, 9, 128, 32), (128, 9, 128, 2),
                                        (8, 9, 2176, 8), (2, 9, 4224, 2),
                                        (32, 5, 1152, 32)])
def test_selection_returns_scaled_nibbles(M, N, K, step):
    x, idx = nh.selection_matrix("int4", M, K)
    p, s = quantize_int4(torch.randn(N, K,
                                     generator=nh._gen("int4-sel", M, N, K)))
    q = unpack_int4(p)
    q[0] = ((torch.arange(K) * 5) % 16 - 8).to(torch.int8)   # distinct along K
    p = pack_int4(q)
    pd, sd = _on_dev(p, s)
    want = Int4Weight(p, s).dequantize(torch.float32).t()[idx].to(BF16)
    for r0 in range(0, M, step):
        got = _kernel(x[r0:r0 + step].contiguous().to(DEV), pd, sd)
        nh.check_equal(got, want[r0:r0 + step].contiguous(),
                       f"w4a16 selection {(M, N, K)} rows {r0}+")


@pytest.mark.parametrize("M", [2, 5])            # dot2 arm, MFMA arm
def test_nan_in_x_row_or_scale_stays_local(M):
    N, K = 17, 2176
    x, p, s, b, ref = _exact_operands(M, N, K)
    x2, s2 = x.clone(), s.clone()
    x2[1, K - 1] = s2[4, 9] = float("nan")
    got = _kernel(*_on_dev(x2, p, s, b)).cpu()
    keep = torch.arange(M) != 1
    assert torch.isnan(got[1]).all()
    nh.check_equal(got[keep], ref[keep], "w4a16 NaN in x row 1, other rows")
    got = _kernel(*_on_dev(x, p, s2, b)).cpu()
    keep = torch.arange(N) != 4
    assert torch.isnan(got[:, 4]).all()
    nh.check_equal(got[:, keep].contiguous(), ref[:, keep].contiguous(),
                   "w4a16 NaN in scale[4, 9], other columns")


@pytest.mark.parametrize("shape", [(5, 17, 2176), (32, 7, 1152), (1, 1, 128),
                                   (2, 9, 4224)],
                         ids=nh.gemv_id)
def test_operands_carved_from_nan_margins(shape):
    """x, q, scale and bias sit in the middle of larger allocations whose
    margins are NaN (q: 0xFF bytes)."""
    M, N, K = shape
    x, p, s, b, ref = _exact_operands(M, N, K)
    nan = float("nan")
    xb = torch.full((M * K + 4096,), nan, dtype=BF16, device=DEV)
    pb = torch.full((N * K // 2 + 8192,), 0xFF, dtype=torch.uint8, device=DEV)
    sb = torch.full((s.numel() + 64,), nan, dtype=torch.float32, device=DEV)
    bb = torch.full((N + 64,), nan, dtype=BF16, device=DEV)
    xd = xb[2048:2048 + M * K].view(M, K)          # 16-byte aligned offsets
    pd = pb[4096:4096 + N * K // 2].view(N, K // 2)
    sd, bd = sb[31:31 + s.numel()].view(s.shape), bb[33:33 + N]
    xd.copy_(x), pd.copy_(p), sd.copy_(s), bd.copy_(b)
    got = _kernel(xd, pd, sd, bd)
    assert torch.isfinite(got).all()
    nh.check_equal(got, ref, f"w4a16 carved {shape}")


@functools.lru_cache(maxsize=None)
def _quantised(wfam, N, K):
    return quantize_int4(nh.mm_input(wfam, 1, N, K)[1].float())


@pytest.mark.parametrize("wfam", ["randn", "wide"])
@pytest.mark.parametrize("xfam", ["randn", "shift", "wide"])
@pytest.mark.parametrize("M,N,K", [(1, 1000, 4224), (4, 9, 8192),
                                   (8, 8200, 2176), (32, 17, 1152)])
def test_precision_vs_fp32_matmul(M, N, K, xfam, wfam):
    x, _ = nh.mm_input(xfam, M, 1, K)
    p, s = _quantised(wfam, N, K)
    ref, mag = _ref64(x, p, s)
    xd, pd, sd = _on_dev(x, p, s)
    lib = (xd.float() @ Int4Weight(pd, sd).dequantize(torch.float32).t()) \
        .to(BF16)
    nh.mm_check(_kernel(xd, pd, sd), lib, ref, mag,
                f"w4a16[x {xfam}, w {wfam} {M}x{N}x{K}]")


@pytest.mark.parametrize("M", [1, 6, 32])
def test_linear_takes_the_kernel_up_to_m32(M):
    N, K = 1000, 2176
    x, _ = nh.mm_input("randn", M, 1, K)
    p, s = _quantised("randn", N, K)
    xd, pd, sd, bd = _on_dev(x, p, s, nh.act_other("int4-bias", (N,), BF16))
    W = Int4Weight(pd, sd)
    with torch.no_grad():
        nh.check_equal(linear(xd, W, bd), _kernel(xd, pd, sd, bd),
                       f"linear(Int4Weight) M={M} +bias")
        nh.check_equal(linear(xd, W), _kernel(xd, pd, sd),
                       f"linear(Int4Weight) M={M}")
        if M % 2 == 0:
            nh.check_equal(linear(xd.view(2, M // 2, K), W, bd),
                           _kernel(xd, pd, sd, bd).view(2, M // 2, N),
                           f"linear(Int4Weight) 3-D M={M}")


def test_m33_takes_the_dequantise_route(monkeypatch):
    def no_kernel(*a, **k):
        raise AssertionError("the int4 kernel was called")

    M, N, K = 33, 40, 2176
    x, _ = nh.mm_input("randn", M, 1, K)
    p, s = _quantised("randn", N, K)
    b = nh.act_other("int4-bias", (N,), BF16)
    ref, mag = _ref64(x, p, s, b)
    xd, pd, sd, bd = _on_dev(x, p, s, b)
    W = Int4Weight(pd, sd)
    lib = F.linear(xd, W.dequantize(BF16), bd)
    monkeypatch.setattr(int4_ops, "ext", lambda *_: type(
        "NoExt", (), {"gemv_w4a16": staticmethod(no_kernel)}))
    with torch.no_grad():
        got = linear(xd, W, bd)
    assert got.dtype == BF16 and got.shape == (M, N)
    nh.mm_check(got, lib, ref, mag, f"int4 dequantise route {M}x{N}x{K}")


def test_switch_forces_the_dequantise_route():
    x, _ = nh.mm_input("randn", 4, 1, 2176)
    xd, pd, sd = _on_dev(x, *_quantised("randn", 1000, 2176))
    W = Int4Weight(pd, sd)
    with torch.no_grad():
        want, kern = linear(xd, W.dequantize(BF16)), linear(xd, W)
        prev = int4_ops.set_int4_gemv(False)
        try:
            assert not int4_ops.int4_gemv_enabled()
            off = linear(xd, W)
        finally:
            int4_ops.set_int4_gemv(prev)
        again = linear(xd, W)
    nh.check_equal(off, want, "TDPA_INT4_GEMV=0: the bf16 route on q*scale")
    nh.check_equal(again, kern, "switch restored")
    nh.check_equal(kern, _kernel(xd, pd, sd), "switch on: the kernel")
    # the two routes round differently (bf16 weight vs exact q * scale)
    assert not torch.equal(off, kern)


def test_launcher_argument_checks():
    x, p, s, b = _on_dev(*_exact_operands(2, 17, 256)[:4])
    bad = [
        (x.float(), p, s, None),                           # x dtype
        (x, p.to(torch.int8), s, None),                    # q dtype
        (x, p, s.double(), None),                          # scale dtype
        (x, p, s[:, :1].contiguous(), None),               # scale shape
        (x, p, s, b.float()),                              # bias dtype
        (x, p[:, ::2], s, None),                           # not contiguous
        (x[:, :192].contiguous(), p[:, :96].contiguous(),
         s[:, :1].contiguous(), None),                     # K % 128 != 0
        (x.repeat(17, 1)[:33], p, s, None),                # M = 33
        (x.repeat(3, 1), p, s, None, 2),                   # dot2 arm, M = 6
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            _kernel(*args)


def _linears(model):
    return [m for m in model.modules() if isinstance(m, LINEAR_TYPES)]


@functools.lru_cache(maxsize=None)
def _models(family):
    """(converted model, twin whose linears hold the dequantised bf16
    weights), the tiny bf16 configs of tests/test_int8_linear_gpu.py."""
    torch.manual_seed(0)
    if family == "gpt2":
        from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
        m = GPT2Model(GPT2Config(vocab_size=50304, n_layer=4, n_head=8,
                                 dim=512, max_seq=64), device=DEV, dtype=BF16)
    else:
        from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel
        m = LlamaModel(LlamaConfig(vocab_size=2048, n_layer=3, n_head=8,
                                   n_kv_head=2, dim=512, ffn_dim=1024,
                                   max_seq=64), device=DEV, dtype=BF16)
    m.eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for lin in _linears(m):
            if lin.bias is not None:
                lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
    twin = copy.deepcopy(m)
    assert quantize_linears_(m, bits=4) == len(_linears(twin)) > 0
    with torch.no_grad():
        for a, b in zip(_linears(m), _linears(twin)):
            assert a.qweight.is_cuda and a.qweight.dtype == torch.uint8
            b.weight.copy_(a.weight.dequantize(BF16))
    return m, twin


def _decode_logits(model, toks):
    from torchdistpackage_amd.inference.generate import (_alloc_caches,
                                                         decode_forward)
    caches = _alloc_caches(model, *toks.shape)
    out = [decode_forward(model, toks[:, :8], caches, 0).float()]
    for p in range(8, toks.shape[1]):
        out.append(decode_forward(model, toks[:, p:p + 1], caches, p).float())
    return out


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_decode_logits_match_dequantised_twin(family):
    m, twin = _models(family)
    toks = torch.randint(0, m.cfg.vocab_size, (2, 24), device=DEV,
                         generator=torch.Generator(DEV).manual_seed(1))
    diffs = [(a - b).abs().max().item() for a, b in
             zip(_decode_logits(m, toks), _decode_logits(twin, toks))]
    print(f"NUMERICS int4 {family} decode logits vs twin: max diff "
          f"{max(diffs):.4f} (bound 0.25)")
    assert max(diffs) < 0.25, diffs       # bf16 logits, two orders; NaN fails


@pytest.mark.parametrize("attn_impl", ["hip", "sdpa"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_graphed_decoder_vs_eager_on_converted_model(family, attn_impl):
    from torchdistpackage_amd.inference import (GraphedGPT2Decoder,
                                                GraphedLlamaDecoder, generate)
    m, _ = _models(family)
    Dec = GraphedGPT2Decoder if family == "gpt2" else GraphedLlamaDecoder
    idx = torch.randint(0, m.cfg.vocab_size, (2, 8), device=DEV,
                        generator=torch.Generator(DEV).manual_seed(2))
    out_g = Dec(m, batch=2, max_seq=48, attn_impl=attn_impl).generate(idx, 24)
    out_e = generate(m, idx, 24, attn_impl=attn_impl)
    assert out_g.shape == out_e.shape == (2, 32)
    assert torch.equal(out_g[:, :12], out_e[:, :12])
    assert (out_g == out_e).float().mean().item() >= 0.8
