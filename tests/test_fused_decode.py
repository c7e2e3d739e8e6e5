"""CPU side of the fused decode step: the three ops equal their compositions,
the knob, the deferred-residual restructuring of the Llama decode path, and
``_cached_attention(appended=True)``."""
import pytest
import torch

from tests import numerics_helpers as nh
from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny
from torchdistpackage_amd.ops.gemm import linear
from torchdistpackage_amd.parallel.tensor.attn import _cached_attention


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_equal_their_compositions_on_cpu(dtype):
    g = nh._gen("fused_decode_cpu", dtype)

    def rn(*shape):
        return nh._randn(shape, g).to(dtype)

    x, w1, w3 = rn(3, 64), rn(24, 64), rn(24, 64)
    assert torch.equal(ops.swiglu_linear(x, w1, w3),
                       ops.swiglu(linear(x, w1), linear(x, w3)))
    y, w = rn(3, 64), rn(64)
    x_new, h = ops.add_rms_norm(x, y, w, 1e-5)
    assert torch.equal(x_new, x + y)
    assert torch.equal(h, ops.rms_norm(x + y, w, 1e-5))

    B, H, Hkv, S, D, Smax = 2, 4, 2, 3, 16, 8
    q, k, v = rn(B, H, S, D), rn(B, Hkv, S, D), rn(B, Hkv, S, D)
    cos, sin = nh.rope_tables(Smax, D)
    for pos0 in (5, torch.tensor([5]), torch.tensor([99])):   # 99 clamps to 5
        kc, vc = torch.zeros(B, Hkv, Smax, D, dtype=dtype), \
            torch.zeros(B, Hkv, Smax, D, dtype=dtype)
        with torch.no_grad():
            got = ops.rope_kv_append(q, k, v, cos, sin, kc, vc, pos0)
        assert torch.equal(got, ops.rope_rotate_half(q, cos, sin, 5))
        assert torch.equal(kc[:, :, 5:], ops.rope_rotate_half(k, cos, sin, 5))
        assert torch.equal(vc[:, :, 5:], v)
        assert not kc[:, :, :5].any() and not vc[:, :, :5].any()
    with pytest.raises(ValueError, match="pos0"):
        ops.rope_kv_append(q, k, v, cos, sin, kc, vc, 6)
    f8 = ops.Fp8KV.zeros(B, Hkv, Smax, D)
    with pytest.raises(TypeError, match="kv_cache_append"):
        ops.rope_kv_append(q, k, v, cos, sin, f8, f8, 0)


def test_knob_defaults_off_and_returns_previous():
    assert ops.fused_decode_enabled() is False
    assert ops.set_fused_decode(True) is False
    assert ops.fused_decode_enabled() is True
    assert ops.set_fused_decode(False) is True
    assert ops.fused_decode_enabled() is False


@pytest.mark.parametrize("attn_impl", ["sdpa", "hip"])
def test_llama_generate_knob_on_equals_off(attn_impl):
    torch.manual_seed(0)
    m = LlamaModel(llama_tiny(), dtype=torch.float32).eval()
    idx = torch.randint(0, m.cfg.vocab_size, (2, 5))
    outs = []
    for on in (False, True):
        prev = ops.set_fused_decode(on)
        try:
            outs.append(generate(m, idx, 6, attn_impl=attn_impl))
        finally:
            ops.set_fused_decode(prev)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("attn_impl", ["sdpa", "hip"])
def test_cached_attention_appended_skips_only_the_write(attn_impl):
    g = nh._gen("cached_attention_appended")
    B, H, Hkv, S, D, Smax, pos0 = 2, 4, 2, 3, 16, 12, 4
    q, k, v = (nh._randn(s, g).float() for s in
               ((B, H, S, D), (B, Hkv, S, D), (B, Hkv, S, D)))
    kc, vc = (nh._randn((B, Hkv, Smax, D), g).float() for _ in range(2))
    k1, v1 = kc.clone(), vc.clone()
    want = _cached_attention(q, k, v, k1, v1, pos0, True, attn_impl)
    k2, v2 = k1.clone(), v1.clone()            # pre-written caches
    got = _cached_attention(q, None, None, k2, v2, pos0, True, attn_impl,
                            appended=True)
    assert torch.equal(got, want)
    assert torch.equal(k2, k1) and torch.equal(v2, v1)
    assert not torch.equal(k1, kc)             # the default did write
