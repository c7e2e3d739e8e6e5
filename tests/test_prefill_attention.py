"""ops.prefill_attention on CPU (the shared fp32 oracle) and the
``TDPA_PREFILL_ATTN`` routing in ``_cached_attention`` (fp32 CPU, tp=1)."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny


@pytest.mark.parametrize("pos0", [0, 5, torch.tensor([5]),
                                  torch.tensor([1, 6])])
def test_cpu_equals_decode_attention(pos0):
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 4, 6, 16, generator=g)
    k = torch.randn(2, 2, 12, 16, generator=g)
    v = torch.randn(2, 2, 12, 16, generator=g)
    got = ops.prefill_attention(q, k, v, pos0)
    assert torch.equal(got, ops.decode_attention(q, k, v, pos0))
    flat = got.permute(2, 0, 1, 3).reshape(6, 2, 4 * 16)
    assert flat.is_contiguous() and flat.data_ptr() == got.data_ptr()
    with pytest.raises(ValueError):
        ops.prefill_attention(q, k, v, 7)               # past the cache
    with pytest.raises(ValueError):
        ops.prefill_attention(q[:, :3], k, v, 0)        # 3 % 2 != 0


def test_knob_routes_long_chunks_only(monkeypatch):
    torch.manual_seed(0)
    m = LlamaModel(llama_tiny()).eval()          # GQA: 4 q heads, 2 kv heads
    torch.manual_seed(2)
    idx = torch.randint(0, 512, (2, 40))         # G * S = 80 > 64
    assert not ops.prefill_attention_enabled()   # off unless asked for
    want = generate(m, idx, 4, attn_impl="hip")

    calls = []
    for name in ("prefill_attention", "decode_attention"):
        real = getattr(ops, name)
        monkeypatch.setattr(
            ops, name, lambda q, *a, _n=name, _r=real, **k:
            calls.append((_n, q.shape[2])) or _r(q, *a, **k))
    assert torch.equal(generate(m, idx, 4, attn_impl="hip"), want)
    assert calls and all(n == "decode_attention" for n, _ in calls)

    calls.clear()
    prev = ops.set_prefill_attention(True)
    try:
        assert prev is False
        assert torch.equal(generate(m, idx, 4, attn_impl="hip"), want)
        # every layer's 40-row prompt chunk went to prefill_attention, every
        # single-token step (G * S = 2) stayed on decode_attention
        assert ("prefill_attention", 40) in calls
        assert all((n == "prefill_attention") == (s == 40) for n, s in calls)
        calls.clear()
        generate(m, idx, 4)                      # sdpa route: neither op
        assert not calls
    finally:
        assert ops.set_prefill_attention(prev) is True
