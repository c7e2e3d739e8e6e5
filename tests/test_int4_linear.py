"""Weight-only int4 linear (ops/int4.py) on the CPU: the nibble packing, the
group-wise quantiser, the fp32 oracle route of ``int4_linear`` and the
in-place model conversion (``quantize_linears_(bits=4)``) with its state dict.

The HIP kernel is covered by tests/test_int4_linear_gpu.py."""
import pytest
import torch
import torch.nn as nn

from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny
from torchdistpackage_amd.ops.gemm import linear
from torchdistpackage_amd.ops.int4 import (Int4Weight, int4_linear,
                                           is_int4_linear, pack_int4,
                                           quantize_int4, unpack_int4)
from torchdistpackage_amd.ops.int8 import is_int8_linear, quantize_linears_
from torchdistpackage_amd.parallel.tensor.tp_utils import TpLinear
from torchdistpackage_amd.tools.module_replace import replace_linear_by_int4

LINEAR_TYPES = (TpLinear, nn.Linear)


def test_pack_round_trip_every_value_at_every_position():
    # row (v, p): value v - 8 at position p of a 32-nibble (16-byte) block,
    # a different value everywhere else
    v, p = torch.meshgrid(torch.arange(16), torch.arange(32), indexing="ij")
    q = ((v + 5) % 16 - 8)[:, :, None].repeat(1, 1, 32)
    q[v, p, p] = v - 8
    q = q.reshape(16 * 32, 32).to(torch.int8)
    packed = pack_int4(q)
    assert packed.dtype == torch.uint8 and packed.shape == (512, 16)
    assert torch.equal(unpack_int4(packed), q)
    # the documented order: low nibble = even k, two's complement
    one = pack_int4(torch.tensor([[-8, 7]], dtype=torch.int8))
    assert one.item() == 0x78


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_int4(dtype):
    g = torch.Generator().manual_seed(11)
    w = torch.randn(9, 384, generator=g) * \
        (2.0 ** torch.arange(-4, 5, dtype=torch.float32))[:, None]
    w[3, 128:256] = 0                           # an all-zero group
    w = w.to(dtype)
    packed, scale = quantize_int4(w)
    assert packed.dtype == torch.uint8 and packed.shape == (9, 192)
    assert scale.dtype == torch.float32 and scale.shape == (9, 3)
    q = unpack_int4(packed)
    assert q.abs().max().item() == 7
    assert (q[3, 128:256] == 0).all() and scale[3, 1].item() == 1.0
    s64 = scale.double().repeat_interleave(128, 1)
    err = (w.double() - q.double() * s64).abs()
    # half a step plus the fp32 rounding of the quotient at |q| <= 7
    assert (err <= s64 * (0.5 + 2.0 ** -20)).all(), (err / s64).max().item()
    W = Int4Weight(packed, scale)
    assert tuple(W.shape) == (9, 384) and W.nbytes() == 9 * 192 + 4 * 9 * 3
    assert torch.equal(W.dequantize(torch.float32), (q.double() * s64).float())
    with pytest.raises(ValueError):
        quantize_int4(torch.zeros(4, 192))      # K % 128 != 0
    with pytest.raises(ValueError):
        quantize_int4(w, group=64)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("xshape", [(5, 256), (2, 3, 256)])
def test_cpu_int4_linear_is_the_fp64_formula(xshape, with_bias):
    g = torch.Generator().manual_seed(5)
    N, K = 37, 256
    packed, scale = quantize_int4(torch.randn(N, K, generator=g))
    bias = torch.randn(N, generator=g) if with_bias else None
    x = torch.randn(*xshape, generator=g)
    got = int4_linear(x, packed, scale, bias)
    w64 = unpack_int4(packed).double() * scale.double().repeat_interleave(128, 1)
    ref, mag = x.double() @ w64.t(), x.double().abs() @ w64.abs().t()
    if with_bias:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    assert got.dtype == x.dtype and got.shape == xshape[:-1] + (N,)
    # fp32 rounding: K + 4 roundings of half an ulp of the terms' magnitude
    assert ((got.double() - ref).abs() <= (K + 4) * 2.0 ** -24 * mag).all()
    assert torch.equal(linear(x, Int4Weight(packed, scale), bias), got)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="inference"):
        int4_linear(x.clone().requires_grad_(True), packed, scale)


def _gpt2():
    torch.manual_seed(0)
    return GPT2Model(GPT2Config(vocab_size=512, n_layer=2, n_head=4, dim=128,
                                max_seq=64)).eval()


def _llama():
    torch.manual_seed(0)
    return LlamaModel(llama_tiny()).eval()          # n_head 4, n_kv_head 2


def _linears(model):
    return [(n, m) for n, m in model.named_modules()
            if isinstance(m, LINEAR_TYPES)]


@pytest.mark.parametrize("make", [_gpt2, _llama])
def test_convert_model_to_int4_and_reload(make):
    a = make()
    shapes = {n: tuple(m.weight.shape) for n, m in _linears(a)}
    ref8 = make()
    assert quantize_linears_(ref8) == len(shapes)           # bits=8, as ever
    assert all(is_int8_linear(m) and m.qweight.dtype == torch.int8
               and m.weight_scale.shape == (shapes[n][0],)
               for n, m in _linears(ref8))
    assert replace_linear_by_int4(a) == len(shapes) > 0
    assert quantize_linears_(a, bits=4) == 0                # already converted
    assert isinstance(a.head.weight, nn.Parameter)
    for n, m in _linears(a):
        N, K = shapes[n]
        assert is_int4_linear(m) and not is_int8_linear(m), n
        assert "weight" not in m._parameters and isinstance(m.weight, Int4Weight)
        assert m.qweight.dtype == torch.uint8 and m.qweight.shape == (N, K // 2)
        assert m.weight_scale.shape == (N, K // 128)
        assert m.weight.nbytes() == N * K // 2 + 4 * N * K // 128
    sd = a.state_dict()
    torch.manual_seed(123)                     # a different initialisation
    b = type(a)(a.cfg).eval()
    quantize_linears_(b, bits=4)
    idx = torch.randint(0, a.cfg.vocab_size, (2, 6),
                        generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        assert not torch.equal(a(idx)["logits"], b(idx)["logits"])
        b.load_state_dict(sd)
        assert torch.equal(a(idx)["logits"], b(idx)["logits"])


def test_linear_with_k_off_the_group_stays_bf16():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(256, 192), nn.Tanh(), nn.Linear(192, 8))
    assert quantize_linears_(net, bits=4) == 1
    assert is_int4_linear(net[0]) and not is_int4_linear(net[2])
    assert isinstance(net[2].weight, nn.Parameter)
    with torch.no_grad():
        assert net(torch.randn(3, 256)).shape == (3, 8)
    with pytest.raises(ValueError):
        quantize_linears_(net, bits=3)
