"""ops.decode_attention on CPU (the fp32 oracle of the GPU kernel) and the
``attn_impl`` wiring through every decode path (fp32 CPU, tp=1)."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.inference.generate import speculative_generate
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny
from torchdistpackage_amd.parallel.tensor.attn import _cached_sdpa

B, HKV, SMAX, D = 2, 2, 12, 16


def _inputs(G, Sq, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, HKV * G, Sq, D, generator=g)
    k = torch.randn(B, HKV, SMAX, D, generator=g)
    v = torch.randn(B, HKV, SMAX, D, generator=g)
    return q, k, v


def _sdpa_ref(q, k, v, pos0, G):
    """The path the models use today: expanded caches + _cached_sdpa."""
    return _cached_sdpa(q, k.repeat_interleave(G, 1),
                        v.repeat_interleave(G, 1), pos0, True)


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("pos0", [0, 5])
def test_cpu_matches_cached_sdpa(G, Sq, pos0):
    q, k, v = _inputs(G, Sq)
    want = _sdpa_ref(q, k, v, pos0, G)
    got_int = ops.decode_attention(q, k, v, pos0)
    got_t1 = ops.decode_attention(q, k, v, torch.tensor([pos0]))
    assert got_int.shape == want.shape
    torch.testing.assert_close(got_int, want, atol=1e-5, rtol=0)
    torch.testing.assert_close(got_t1, want, atol=1e-5, rtol=0)
    # B-element tensor: a different length per batch row
    pos_b = torch.tensor([pos0, pos0 + 2])
    got_b = ops.decode_attention(q, k, v, pos_b)
    for b in range(B):
        want_b = _sdpa_ref(q[b:b + 1], k[b:b + 1], v[b:b + 1],
                           int(pos_b[b]), G)
        torch.testing.assert_close(got_b[b:b + 1], want_b, atol=1e-5, rtol=0)


def test_output_is_view_of_seq_first_buffer():
    q, k, v = _inputs(4, 3)
    o = ops.decode_attention(q, k, v, 2)
    Hq = q.shape[1]
    flat = o.permute(2, 0, 1, 3).reshape(3, B, Hq * D)
    assert flat.is_contiguous()
    assert flat.data_ptr() == o.data_ptr()          # a view, not a copy


@pytest.mark.parametrize("pos_kind", ["int", "tensor"])
def test_nan_beyond_valid_length_is_not_read(pos_kind):
    G, Sq, pos0 = 4, 3, 4
    q, k, v = _inputs(G, Sq, seed=1)
    want = ops.decode_attention(q, k, v, pos0)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, pos0 + Sq:] = float("nan")
    v2[:, :, pos0 + Sq:] = float("nan")
    pos = pos0 if pos_kind == "int" else torch.tensor([pos0, pos0])
    got = ops.decode_attention(q, k2, v2, pos)
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, want, atol=1e-6, rtol=0)


def test_scale_and_bad_arguments():
    q, k, v = _inputs(1, 1)
    a = ops.decode_attention(q, k, v, 3, scale=0.5)
    want = torch.nn.functional.scaled_dot_product_attention(
        q, k[:, :, :4], v[:, :, :4], scale=0.5)
    torch.testing.assert_close(a, want, atol=1e-5, rtol=0)
    with pytest.raises(ValueError):
        ops.decode_attention(q, k, v, SMAX)         # past the cache
    with pytest.raises(ValueError):
        ops.decode_attention(q[:, :1], k[:, :2], v[:, :2], 0)  # 1 % 2 != 0


def test_env_knob_resolution(monkeypatch):
    monkeypatch.delenv("TDPA_DECODE_ATTN", raising=False)
    assert ops.resolve_decode_attn_impl(None) == "sdpa"
    monkeypatch.setenv("TDPA_DECODE_ATTN", "1")
    assert ops.resolve_decode_attn_impl(None) == "hip"
    assert ops.resolve_decode_attn_impl("sdpa") == "sdpa"
    monkeypatch.setenv("TDPA_DECODE_ATTN", "0")
    assert ops.resolve_decode_attn_impl(None) == "sdpa"
    assert ops.resolve_decode_attn_impl("hip") == "hip"
    with pytest.raises(ValueError):
        ops.resolve_decode_attn_impl("flash")


@pytest.fixture
def gpt2_tiny_model():
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_layer=2, n_head=4, dim=128,
                     max_seq=64)
    return GPT2Model(cfg).eval()


def test_gpt2_generate_hip_equals_default(gpt2_tiny_model):
    torch.manual_seed(1)
    idx = torch.randint(0, 512, (2, 7))
    want = generate(gpt2_tiny_model, idx, 10)
    got = generate(gpt2_tiny_model, idx, 10, attn_impl="hip")
    assert torch.equal(got, want)


def test_llama_generate_hip_equals_default(monkeypatch):
    torch.manual_seed(0)
    m = LlamaModel(llama_tiny()).eval()          # GQA: 4 q heads, 2 kv heads
    torch.manual_seed(2)
    idx = torch.randint(0, 512, (2, 5))
    want = generate(m, idx, 8)
    assert torch.equal(generate(m, idx, 8, attn_impl="hip"), want)
    # the env knob selects the same path when the argument is left unset
    calls = []
    real = ops.decode_attention
    monkeypatch.setattr(ops, "decode_attention",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv("TDPA_DECODE_ATTN", "1")
    assert torch.equal(generate(m, idx, 8), want)
    assert calls, "TDPA_DECODE_ATTN=1 did not reach ops.decode_attention"
    calls.clear()
    monkeypatch.setenv("TDPA_DECODE_ATTN", "0")
    assert torch.equal(generate(m, idx, 8), want)
    assert not calls, "default path must not touch ops.decode_attention"


def test_speculative_hip_equals_greedy(gpt2_tiny_model):
    target = gpt2_tiny_model
    torch.manual_seed(42)
    draft = GPT2Model(GPT2Config(vocab_size=512, n_layer=1, n_head=2,
                                 dim=64, max_seq=64)).eval()
    torch.manual_seed(5)
    idx = torch.randint(0, 512, (1, 6))
    want = generate(target, idx, 12)
    for k in (1, 4, 7):
        got = speculative_generate(target, draft, idx, 12, k=k,
                                   attn_impl="hip")
        assert torch.equal(got, want), k


def test_speculative_llama_hip_equals_greedy():
    # GQA (G=2) with verification chunks of up to 9 rows: G*Sq > 16
    torch.manual_seed(0)
    target = LlamaModel(llama_tiny()).eval()
    torch.manual_seed(9)
    draft = LlamaModel(llama_tiny()).eval()
    idx = torch.randint(0, 512, (1, 5))
    want = generate(target, idx, 14)
    got = speculative_generate(target, draft, idx, 14, k=9, attn_impl="hip")
    assert torch.equal(got, want)
