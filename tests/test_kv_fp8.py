"""fp8 (e4m3) KV cache on the CPU: the reference quantiser (ops/kv_fp8.py),
cache contents under chunked prefill, and generation and routing with
``kv_dtype="fp8"`` (fp32 tiny models, tp=1; the hip route is the fp32 oracle
on CPU tensors)."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.inference.generate import (_alloc_caches,
                                                     decode_forward,
                                                     speculative_generate)
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny


def _gpt2(n_layer=2, n_head=4, dim=128):
    torch.manual_seed(0)
    return GPT2Model(GPT2Config(vocab_size=512, n_layer=n_layer,
                                n_head=n_head, dim=dim, max_seq=64)).eval()


def test_reference_quantiser_properties():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 128, generator=g).bfloat16()
    x *= torch.logspace(-6, 4.5, 64)[:, None].bfloat16()   # 1e-6 .. 3e4
    x[0] = 0                                               # all-zero row
    x[1, 3:] = 0                                           # one live element
    x[2, 0], x[3, 0] = 448 * 2.0 ** 5, 450 * 2.0 ** 5      # amax at / above
    x[4] = 0
    x[4, 0] = 2.0 ** -80                                   # under the floor
    data, scale = ops.quantize_kv_rows(x)
    assert data.dtype == torch.uint8 and scale.dtype == torch.float32
    amax = x.float().abs().amax(-1)
    ratio = (amax / scale)[amax > 2.0 ** -55]
    assert (ratio > 224).all() and (ratio <= 448).all()
    assert torch.equal(torch.frexp(scale)[0], torch.full_like(scale, 0.5))
    assert scale[0] == scale[4] == 2.0 ** -64 and not data[0].any()
    assert scale[2] * 2 == scale[3]
    # round trip: half an e4m3 ulp (2^-4 relative) on every normal element
    back = data.view(torch.float8_e4m3fn).float() * scale[:, None]
    xf = x.float()
    normal = xf.abs() >= scale[:, None] * 2.0 ** -6
    assert ((back - xf).abs() <= xf.abs() * 2.0 ** -4)[normal].all()
    assert ((back - xf).abs() <= scale[:, None] * 2.0 ** -10)[~normal].all()


def test_fp8kv_type_append_and_dequantize():
    kc, vc = ops.Fp8KV.zeros(2, 3, 16, 32), ops.Fp8KV.zeros(2, 3, 16, 32)
    assert kc.shape == (2, 3, 16, 32) and kc.device.type == "cpu"
    assert not kc.dequantize(torch.float32).any()
    g = torch.Generator().manual_seed(1)
    k, v = torch.randn(2, 3, 5, 32, generator=g), torch.randn(2, 3, 5, 32,
                                                              generator=g)
    ops.kv_cache_append(kc, vc, k, v, torch.tensor([2, 11]))  # per-row pos
    data, scale = ops.quantize_kv_rows(v)
    assert torch.equal(vc.data[0, :, 2:7], data[0])
    assert torch.equal(vc.scale[1, :, 11:16], scale[1])
    assert not vc.data[1, :, :11].any() and not kc.data[0, :, 7:].any()
    got = kc.dequantize(torch.float32, length=7)
    assert got.shape == (2, 3, 7, 32)
    assert (got[0, :, 2:] - k[0]).abs().max() <= k[0].abs().max() * 2.0 ** -4
    with pytest.raises(ValueError, match="outside the cache"):
        ops.kv_cache_append(kc, vc, k, v, 12)


def test_cache_bytes_independent_of_prefill_chunking():
    m = _gpt2()
    toks = torch.randint(0, 512, (2, 23))
    one = _alloc_caches(m, 2, 32, kv_dtype="fp8")
    chunked = _alloc_caches(m, 2, 32, kv_dtype="fp8")
    want = decode_forward(m, toks, one, 0, attn_impl="hip")
    pos0 = 0
    for n in (7, 1, 10, 5):
        got = decode_forward(m, toks[:, pos0:pos0 + n], chunked, pos0,
                             attn_impl="hip")
        pos0 += n
    for pair_a, pair_b in zip(one, chunked):
        for a, b in zip(pair_a, pair_b):
            assert torch.equal(a.data, b.data)
            assert torch.equal(a.scale, b.scale)
    assert (got - want).abs().max() < 1e-4      # same values, other order


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_and_speculative_fp8(family):
    if family == "gpt2":
        target, draft = _gpt2(), _gpt2(n_layer=1, n_head=2, dim=64)
    else:
        torch.manual_seed(0)
        target = LlamaModel(llama_tiny()).eval()
        draft = LlamaModel(llama_tiny()).eval()
    idx = torch.randint(0, 512, (1, 6))
    want = generate(target, idx, 12, attn_impl="hip", kv_dtype="fp8")
    assert want.shape == (1, 18) and torch.equal(want[:, :6], idx)
    for k in (1, 4):
        got = speculative_generate(target, draft, idx, 12, k=k,
                                   attn_impl="hip", kv_dtype="fp8")
        assert torch.equal(got, want), k


def test_kv_dtype_knob_and_routing_errors(monkeypatch):
    m = _gpt2()
    monkeypatch.setenv("TDPA_KV_DTYPE", "fp8")
    assert isinstance(_alloc_caches(m, 1, 8)[0][0], ops.Fp8KV)
    monkeypatch.delenv("TDPA_KV_DTYPE")
    assert torch.is_tensor(_alloc_caches(m, 1, 8)[0][0])
    with pytest.raises(ValueError, match="kv_dtype"):
        _alloc_caches(m, 1, 8, kv_dtype="int4")
    idx = torch.randint(0, 512, (1, 4))
    with pytest.raises(ValueError, match="attn_impl='hip'"):
        generate(m, idx, 2, attn_impl="sdpa", kv_dtype="fp8")
    kq = ops.Fp8KV.zeros(1, 2, 8, 32)
    kt = torch.zeros(1, 2, 8, 32)
    x = torch.zeros(1, 2, 1, 32)
    with pytest.raises(TypeError, match="both"):
        ops.kv_cache_append(kq, kt, x, x, 0)
    with pytest.raises(TypeError, match="both"):
        ops.decode_attention(x, kt, kq, 0)
