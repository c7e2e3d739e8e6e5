"""Weight-only int8 linear (ops/int8.py) on the CPU: the quantiser, the fp32
oracle route of ``int8_linear``, the ``linear(x, Int8Weight)`` branch, the
in-place model conversion with its state dict, and the argument errors.

The HIP kernel is covered by tests/test_int8_linear_gpu.py."""
import copy

import pytest
import torch
import torch.nn as nn

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.inference.generate import (_alloc_caches,
                                                     decode_forward)
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny
from torchdistpackage_amd.ops.gemm import linear
from torchdistpackage_amd.ops.int8 import (Int8Weight, int8_linear,
                                           is_int8_linear, quantize_int8,
                                           quantize_linears_)
from torchdistpackage_amd.parallel.tensor.tp_utils import TpLinear
from torchdistpackage_amd.tools.module_replace import replace_linear_by_int8

LINEAR_TYPES = (TpLinear, nn.Linear)     # Col/RowParallelLinear are TpLinear


# ------------------------------------------------------------- 1. quantiser

def _quantiser_rows():
    g = torch.Generator().manual_seed(11)
    K = 96
    randn = torch.randn(6, K, generator=g)
    wide = torch.randn(13, K, generator=g) * \
        (2.0 ** torch.arange(-6, 7, dtype=torch.float32))[:, None]
    neg = -torch.rand(1, K, generator=g) - 0.5       # maximum is negative
    neg[0, 7] = -3.0
    zero = torch.zeros(1, K)
    return torch.cat([randn, wide, neg, zero], 0)    # zero row last


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_int8(dtype):
    w = _quantiser_rows().to(dtype)
    q, scale = quantize_int8(w)
    assert q.dtype == torch.int8 and q.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    assert q.abs().max().item() <= 127
    assert (q[:-1].abs().amax(1) == 127).all(), "a non-zero row misses +-127"
    assert (q[-1] == 0).all()
    assert torch.isfinite(scale).all() and (scale != 0).all()
    # half a step plus the fp32 rounding of the quotient at |q| <= 127
    w64, s64 = w.double(), scale.double()[:, None]
    err = (w64 - q.double() * s64).abs()
    assert (err <= s64 * (0.5 + 2.0 ** -16)).all(), \
        (err / s64).max().item()
    # the row whose entries are all negative reaches -127 at its extreme
    assert q[-2, 7].item() == -127
    assert torch.equal(scale[:-1], w.float().abs().amax(1)[:-1] / 127.0)


def test_quantize_int8_bf16_equals_fp32_upcast():
    w = _quantiser_rows().bfloat16()
    q16, s16 = quantize_int8(w)
    q32, s32 = quantize_int8(w.float())
    assert torch.equal(q16, q32) and torch.equal(s16, s32)


# ---------------------------------------------------------------- 2. oracle

def _oracle_case(N=37, K=48):
    g = torch.Generator().manual_seed(5)
    q, scale = quantize_int8(torch.randn(N, K, generator=g))
    bias = torch.randn(N, generator=g)
    return q, scale, bias, g


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("xshape", [(5, 48), (2, 3, 48)])
def test_cpu_int8_linear_is_the_fp64_formula(xshape, with_bias):
    q, scale, bias, g = _oracle_case()
    x = torch.randn(*xshape, generator=g)
    b = bias if with_bias else None
    got = int8_linear(x, q, scale, b)
    ref = (x.double() @ q.double().t()) * scale.double()
    mag = (x.double().abs() @ q.double().abs().t()) * scale.double()
    if with_bias:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    assert got.dtype == x.dtype and got.shape == xshape[:-1] + (37,)
    # fp32 rounding: K + 2 roundings of half an ulp of the terms' magnitude
    assert ((got.double() - ref).abs() <= (48 + 2) * 2.0 ** -24 * mag).all()
    same = linear(x, Int8Weight(q, scale), b)
    assert torch.equal(same, got)


def test_int8_weight_handle():
    q, scale, _, _ = _oracle_case()
    w = Int8Weight(q, scale)
    assert tuple(w.shape) == (37, 48) and w.device == q.device
    d = w.dequantize(torch.float32)
    assert d.dtype == torch.float32
    assert torch.equal(d, q.float() * scale[:, None])
    assert w.dequantize(torch.bfloat16).dtype == torch.bfloat16
    assert w.nbytes() == 37 * 48 + 4 * 37


# ------------------------------------------------------ 3. model conversion

def _gpt2():
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_layer=2, n_head=4, dim=128,
                     max_seq=64)
    return GPT2Model(cfg).eval()


def _llama():
    torch.manual_seed(0)
    return LlamaModel(llama_tiny()).eval()          # n_head 4, n_kv_head 2


def _randomise_biases(model):
    """Linear biases start at zero; make them count."""
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, LINEAR_TYPES) and m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))


def _linears(model):
    return [(n, m) for n, m in model.named_modules()
            if isinstance(m, LINEAR_TYPES)]


def _oracle_twin(model):
    """Deep copy of the unconverted model, each linear's weight overwritten
    by q * scale in fp32."""
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for _, m in _linears(twin):
            q, s = quantize_int8(m.weight)
            m.weight.copy_(q.float() * s[:, None])
    return twin


def _decode_logits(model, idx):
    B, T = idx.shape
    caches = _alloc_caches(model, B, T)
    out = [decode_forward(model, idx[:, :4], caches, 0)]    # prefill, steps
    for p in range(4, T):
        out.append(decode_forward(model, idx[:, p:p + 1], caches, p))
    return torch.stack(out, 1)


MODELS = {"gpt2": _gpt2, "llama": _llama}


@pytest.mark.parametrize("family", sorted(MODELS))
@pytest.mark.parametrize("entry", ["ops", "tools"])
def test_convert_model_in_place(family, entry):
    model = MODELS[family]()
    _randomise_biases(model)
    twin = _oracle_twin(model)
    n_lin = len(_linears(model))
    assert n_lin > 0
    head_w, emb = model.head.weight, list(model.embed.parameters())
    convert = quantize_linears_ if entry == "ops" else replace_linear_by_int8
    assert convert(model) == n_lin
    assert model.head.weight is head_w
    assert isinstance(model.head.weight, nn.Parameter)
    for a, b in zip(emb, model.embed.parameters()):
        assert a is b
    for name, m in _linears(model):
        assert is_int8_linear(m), name
        assert "weight" not in m._parameters, name
        assert isinstance(m.weight, Int8Weight), name
        assert m.qweight.dtype == torch.int8
        assert m.weight_scale.dtype == torch.float32
    assert not any(n.endswith(".weight") and p.dim() == 2
                   and not n.startswith(("embed.", "head."))
                   for n, p in model.named_parameters())

    idx = torch.randint(0, model.cfg.vocab_size, (2, 9),
                        generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        got, want = model(idx)["logits"], twin(idx)["logits"]
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
        got, want = _decode_logits(model, idx), _decode_logits(twin, idx)
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)


def test_convert_honours_skip():
    model = _llama()
    names = [n for n, _ in _linears(model)]
    skip = ("blocks.0.attn", "blocks.1.mlp.w2")
    left = [n for n in names
            if n.startswith("blocks.0.attn.") or n == "blocks.1.mlp.w2"]
    assert len(left) == 5               # wq wk wv wo of block 0, one w2
    assert quantize_linears_(model, skip=skip) == len(names) - len(left)
    for n, m in _linears(model):
        assert is_int8_linear(m) == (n not in left), n
        if n in left:
            assert isinstance(m.weight, nn.Parameter)


def test_convert_bare_nn_linear():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(32, 24), nn.Tanh(), nn.Linear(24, 8,
                                                                bias=False))
    twin = _oracle_twin(net)
    assert quantize_linears_(net) == 2
    x = torch.randn(5, 32)
    with torch.no_grad():
        torch.testing.assert_close(net(x), twin(x), rtol=1e-4, atol=1e-5)


def test_convert_leaves_moe_experts():
    from torchdistpackage_amd.moe.layer import Expert
    torch.manual_seed(0)
    net = nn.ModuleDict({"ex": Expert(16), "lin": nn.Linear(16, 16)})
    assert quantize_linears_(net) == 1
    assert isinstance(net["ex"].fc1.weight, nn.Parameter)
    assert isinstance(net["ex"].fc2.weight, nn.Parameter)
    assert is_int8_linear(net["lin"])


# ------------------------------------------------------------ 4. state dict

@pytest.mark.parametrize("family", sorted(MODELS))
def test_state_dict_round_trip(family):
    a = MODELS[family]()
    _randomise_biases(a)
    quantize_linears_(a)
    sd = a.state_dict()
    lin_names = [n for n, _ in _linears(a)]
    for n in lin_names:
        assert n + ".qweight" in sd and n + ".weight_scale" in sd
        assert n + ".weight" not in sd
    assert sd[lin_names[0] + ".qweight"].dtype == torch.int8

    torch.manual_seed(123)                     # a different initialisation
    b = type(a)(a.cfg).eval()
    quantize_linears_(b)
    idx = torch.randint(0, a.cfg.vocab_size, (2, 6),
                        generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        assert not torch.equal(a(idx)["logits"], b(idx)["logits"])
        b.load_state_dict(sd)
        assert torch.equal(a(idx)["logits"], b(idx)["logits"])
    for n, m in _linears(b):
        assert torch.equal(m.qweight, sd[n + ".qweight"])
        assert torch.equal(m.weight_scale, sd[n + ".weight_scale"])


# ---------------------------------------------------------------- 5. errors

def test_grad_enabled_call_raises():
    q, scale, bias, g = _oracle_case()
    x = torch.randn(3, 48, generator=g)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference-only"):
            int8_linear(x.clone().requires_grad_(True), q, scale)
        with pytest.raises(RuntimeError, match="inference-only"):
            linear(x, Int8Weight(q, scale),
                   bias.clone().requires_grad_(True))
        int8_linear(x, q, scale, bias)          # nothing requires grad: fine
    with torch.no_grad():
        int8_linear(x.clone().requires_grad_(True), q, scale)


def test_wrong_dtypes_and_shapes_raise():
    q, scale, bias, g = _oracle_case()
    x = torch.randn(3, 48, generator=g)
    with pytest.raises(TypeError):
        int8_linear(x, q.to(torch.int16), scale)
    with pytest.raises(TypeError):
        int8_linear(x, q.float(), scale)
    with pytest.raises(TypeError):
        int8_linear(x, q, scale.double())
    with pytest.raises(TypeError):
        int8_linear(x, q.reshape(-1), scale)
    with pytest.raises(ValueError):
        int8_linear(x, q, scale[:-1])
    with pytest.raises(ValueError):
        int8_linear(x, q, scale[:, None])
    with pytest.raises(ValueError):
        int8_linear(x[:, :-1], q, scale)
    with pytest.raises(ValueError):
        int8_linear(x, q, scale, bias[:-1])
    with pytest.raises(TypeError):
        Int8Weight(q.float(), scale)
    with pytest.raises(ValueError):
        quantize_int8(torch.zeros(4))


def test_converting_twice_is_a_no_op():
    model = _gpt2()
    n = quantize_linears_(model)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert n > 0 and quantize_linears_(model) == 0
    assert replace_linear_by_int8(model) == 0
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_env_switch_value(monkeypatch):
    from torchdistpackage_amd.ops import int8 as int8_ops
    monkeypatch.delenv("TDPA_INT8_GEMV", raising=False)
    assert int8_ops._read_env() is True
    monkeypatch.setenv("TDPA_INT8_GEMV", "0")
    assert int8_ops._read_env() is False
    monkeypatch.setenv("TDPA_INT8_GEMV", "1")
    assert int8_ops._read_env() is True
    prev = int8_ops.set_int8_gemv(False)
    try:
        assert int8_ops.int8_gemv_enabled() is False
    finally:
        int8_ops.set_int8_gemv(prev)
    assert int8_ops.int8_gemv_enabled() is prev
