"""Paged KV cache on the CPU (ops/paged_kv.py): append and gather through a
permuted block table, the paged ``"hip"`` route of generate() in fp32, and
the environment knobs."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.inference.generate import resolve_kv_layout
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model


@pytest.mark.parametrize("pos", [14, torch.tensor([14]),
                                 torch.tensor([14, 30])])
def test_append_gather_round_trip(pos):
    g = torch.Generator().manual_seed(0)
    B, Hkv, D, S, page = 2, 2, 8, 20, 16
    table = torch.randperm(B * 4 + 3, generator=g)[:B * 4] \
        .to(torch.int32).view(B, 4)
    k = ops.PagedKV.zeros(B, Hkv, 64, D, page, torch.float32,
                          block_table=table, num_pages=B * 4 + 3)
    v = ops.PagedKV(torch.zeros_like(k.pool), table)
    assert k.shape == (B, Hkv, 64, D) and not k.is_cuda
    assert k.nbytes() == k.pool.numel() * 4 + 4 * table.numel()
    dense_k, dense_v = torch.zeros(k.shape), torch.zeros(k.shape)
    xk = torch.randn(B, Hkv, S, D, generator=g)
    xv = torch.randn(B, Hkv, S, D, generator=g)
    ops.kv_cache_append(k, v, xk, xv, pos)
    rows = [int(pos)] * B if not torch.is_tensor(pos) or pos.numel() == 1 \
        else pos.tolist()
    for b, p in enumerate(rows):
        dense_k[b, :, p:p + S] = xk[b]
        dense_v[b, :, p:p + S] = xv[b]
    assert torch.equal(k.gather(), dense_k)
    assert torch.equal(v.gather(), dense_v)
    assert torch.equal(k.gather(37), dense_k[:, :, :37])


def test_generate_paged_fp32_equals_default():
    torch.manual_seed(0)
    m = GPT2Model(GPT2Config(vocab_size=128, n_layer=2, n_head=4, dim=64,
                             max_seq=64)).eval()
    idx = torch.randint(0, 128, (2, 5))
    assert torch.equal(generate(m, idx, 14, attn_impl="hip",
                                kv_layout="paged"), generate(m, idx, 14))


def test_environment_knobs(monkeypatch):
    monkeypatch.delenv("TDPA_KV_LAYOUT", raising=False)
    monkeypatch.delenv("TDPA_KV_PAGE", raising=False)
    assert resolve_kv_layout() == ("contiguous", 16)
    monkeypatch.setenv("TDPA_KV_LAYOUT", "paged")
    monkeypatch.setenv("TDPA_KV_PAGE", "64")
    assert resolve_kv_layout() == ("paged", 64)
    assert resolve_kv_layout("contiguous", 32) == ("contiguous", 32)
    monkeypatch.setenv("TDPA_KV_PAGE", "24")
    with pytest.raises(ValueError, match="page_size"):
        resolve_kv_layout()
    assert resolve_kv_layout("contiguous")[0] == "contiguous"   # no pages
    monkeypatch.setenv("TDPA_KV_LAYOUT", "ragged")
    with pytest.raises(ValueError, match="kv_layout"):
        resolve_kv_layout()
