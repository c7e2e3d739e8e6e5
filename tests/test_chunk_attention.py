"""ops.chunk_attention on CPU (the shared fp32 oracle) and the
``TDPA_CHUNK_ATTN`` routing in ``_cached_attention`` (fp32 CPU)."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.parallel.tensor.attn import _cached_attention


@pytest.mark.parametrize("Hq,Hkv,Sq,pos0", [(4, 2, 9, 3),
                                            (3, 1, 20, torch.tensor([0, 4]))])
def test_cpu_equals_decode_attention(Hq, Hkv, Sq, pos0):
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, Hq, Sq, 16, generator=g)
    k = torch.randn(2, Hkv, 24, 16, generator=g)
    v = torch.randn(2, Hkv, 24, 16, generator=g)
    got = ops.chunk_attention(q, k, v, pos0)
    assert torch.equal(got, ops.decode_attention(q, k, v, pos0))
    flat = got.permute(2, 0, 1, 3).reshape(Sq, 2, Hq * 16)
    assert flat.is_contiguous() and flat.data_ptr() == got.data_ptr()


def test_row_cap_raises():
    q, kv = torch.zeros(1, 5, 13, 16), torch.zeros(1, 1, 16, 16)
    with pytest.raises(ValueError, match="prefill_attention"):
        ops.chunk_attention(q, kv, kv, 0)                # 5 * 13 = 65 rows


def test_knob_routes_17_to_64_rows_only(monkeypatch):
    calls = []
    real = ops.chunk_attention
    monkeypatch.setattr(ops, "chunk_attention", lambda q, *a, **k:
                        calls.append(q.shape[2]) or real(q, *a, **k))

    def step(S, pos0=2, G=1):
        g = torch.Generator().manual_seed(S)
        q = torch.randn(1, 2 * G, S, 16, generator=g)
        k = torch.randn(1, 2, S, 16, generator=g)
        v = torch.randn(1, 2, S, 16, generator=g)
        kc, vc = torch.zeros(1, 2, 80, 16), torch.zeros(1, 2, 80, 16)
        return _cached_attention(q, k, v, kc, vc, pos0, True, "hip")

    assert not ops.chunk_attention_enabled()             # off unless asked for
    want = {S: step(S) for S in (17, 64)}
    assert not calls
    prev = ops.set_chunk_attention(True)
    try:
        assert prev is False
        for S in (17, 64):
            assert torch.equal(step(S), want[S])
        assert calls == [17, 64]
        step(32, G=2)                                    # G * S = 64
        assert calls == [17, 64, 32]
        step(16), step(65), step(33, G=2)                # 16, 65, 66 rows
        step(1, pos0=torch.tensor([2]), G=17)            # 17 rows, tensor pos0
        assert calls == [17, 64, 32]
    finally:
        assert ops.set_chunk_attention(prev) is True
