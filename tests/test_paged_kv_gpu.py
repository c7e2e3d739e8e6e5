"""Paged KV cache on the GPU (ops/csrc/decode_attn_paged.hip): the paged
decode kernel against the CPU fp32 oracle and, bit for bit, against the
contiguous kernel; the append against the CPU torch loop; the model routes
against the contiguous ``"hip"`` route.

Bound for the kernel: max abs error < 3e-2 with every expected |v| < 8, the
bound of test_decode_attention_gpu.py and its reason.  Every kernel case runs
on a poisoned copy of the cache: spare pool pages, every slot at or past
``pos0+Sq`` and every page a table entry past the valid length names are NaN,
and those entries stay in range, so a wrong kernel shows NaN, not a fault."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.inference.generate import (GraphedDecoder,
                                                     _alloc_caches,
                                                     decode_forward,
                                                     speculative_generate)
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel

pytestmark = pytest.mark.gpu

B, SMAX, SPARE = 2, 256, 8
BOUND = 3e-2
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 200, 256]   # pos0 + Sq
NAN = float("nan")


def _make(page, Hq, Hkv, D, Sq, seed=0):
    """bf16 q and clean K, V PagedKV of capacity SMAX under one seeded
    random permutation table; no row names the pool's last SPARE pages."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nb = SMAX // page
    P = B * nb + SPARE
    table = torch.randperm(B * nb, generator=g, device="cuda") \
        .to(torch.int32).view(B, nb)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device="cuda",
                           dtype=torch.bfloat16)

    return (rn(B, Hq, Sq, D), ops.PagedKV(rn(P, Hkv, page, D), table),
            ops.PagedKV(rn(P, Hkv, page, D), table))


def _check(q, k, v, pos0, split_kv, tag):
    """Kernel on the poisoned copy against the oracle on the clean gathered
    cache, and bit for bit against the contiguous kernel."""
    Sq, page, P = q.shape[2], k.page_size, k.pool.shape[0]
    p = pos0.reshape(-1).tolist() if torch.is_tensor(pos0) else [pos0]
    dead = [x + Sq for x in (p if len(p) == B else p * B)]
    table = k.block_table.clone()
    kp, vp = k.pool.clone(), v.pool.clone()
    for b, n in enumerate(dead):
        if n % page:
            last = int(table[b, n // page])
            kp[last, :, n % page:] = NAN
            vp[last, :, n % page:] = NAN
        table[b, -(-n // page):] = P - 1 - b
    unnamed = torch.ones(P, dtype=torch.bool, device="cuda")
    unnamed[table.reshape(-1).long()] = False
    unnamed[-SPARE:] = True
    kp[unnamed] = NAN
    vp[unnamed] = NAN
    got = ops.decode_attention(q, ops.PagedKV(kp, table),
                               ops.PagedKV(vp, table), pos0,
                               split_kv=split_kv)
    kd, vd = k.gather(), v.gather()
    want = ops.decode_attention(q.float().cpu(), kd.float().cpu(),
                                vd.float().cpu(),
                                pos0.cpu() if torch.is_tensor(pos0) else pos0)
    assert want.abs().max().item() < 8
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    err = (got.float().cpu() - want).abs().max().item()
    print(f"paged decode_attention {tag}: max abs err {err:.3e}")
    assert err < BOUND, (tag, err)           # NaN fails here too
    assert torch.equal(got, ops.decode_attention(q, kd, vd, pos0,
                                                 split_kv=split_kv)), tag


# (Hq, Hkv, Sq): M = G*Sq = 1, 4, 4, 16 and a padded 6
@pytest.mark.parametrize("Hq,Hkv,Sq", [(4, 4, 1), (4, 4, 4), (8, 2, 1),
                                       (8, 2, 4), (4, 2, 3)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("page", [16, 64])
def test_kernel_vs_oracle(page, D, Hq, Hkv, Sq):
    q, k, v = _make(page, Hq, Hkv, D, Sq)
    for n in LENGTHS:
        for split in (64, None):
            _check(q, k, v, max(n - Sq, 0), split,
                   f"page{page} D{D} H{Hq}/{Hkv} Sq{Sq} len{n} split{split}")


def test_kernel_page_128():
    q, k, v = _make(128, 8, 2, 128, 2, seed=1)
    for n in (2, 127, 128, 129, 256):
        _check(q, k, v, n - 2, 128, f"page128 len{n}")


@pytest.mark.parametrize("pos", [[130], [9, 199]])
def test_position_forms_bit_equal_contiguous(pos):
    # _check compares with the contiguous kernel at the same split_kv
    q, k, v = _make(16, 8, 2, 128, 2, seed=2)
    if len(pos) == 1:
        _check(q, k, v, pos[0], 64, "int pos")
    _check(q, k, v, torch.tensor(pos, device="cuda"), 64, f"tensor pos {pos}")


@pytest.mark.parametrize("form", ["int", "one", "per_row"])
@pytest.mark.parametrize("S", [1, 5, 20])
@pytest.mark.parametrize("D", [64, 128])
def test_append_equals_cpu_loop(D, S, form):
    # from 14 (and 30): page edges at 16 and 32 are crossed
    q, k, v = _make(16, 2, 2, D, 1, seed=3)
    g = torch.Generator(device="cuda").manual_seed(4)
    src = torch.randn(2, B, 2, S + 2, 2 * D, generator=g, device="cuda",
                      dtype=torch.bfloat16)[:, :, :, 1:S + 1, D:]
    assert not src[0].is_contiguous()
    pos = {"int": 14, "one": torch.tensor([14]),
           "per_row": torch.tensor([14, 30])}[form]
    kc = ops.PagedKV(k.pool.cpu(), k.block_table.cpu())
    vc = ops.PagedKV(v.pool.cpu(), kc.block_table)
    ops.kv_cache_append(kc, vc, src[0].cpu(), src[1].cpu(), pos)
    ops.kv_cache_append(k, v, src[0], src[1],
                        pos.cuda() if torch.is_tensor(pos) else pos)
    assert torch.equal(k.pool.cpu(), kc.pool)
    assert torch.equal(v.pool.cpu(), vc.pool)


def test_shared_prefix_equals_private_copies():
    q, k, v = _make(16, 8, 2, 64, 1, seed=5)
    k.block_table[1, :2] = k.block_table[0, :2]     # v shares the table
    got = ops.decode_attention(q, k, v, 99, split_kv=64)
    assert torch.equal(got, ops.decode_attention(q, k.gather(), v.gather(),
                                                 99, split_kv=64))


def test_raises():
    q, k, v = _make(16, 4, 4, 64, 1)
    m = _tiny("gpt2")
    with pytest.raises(ValueError, match="hip"):
        generate(m, torch.zeros(1, 4, dtype=torch.long, device="cuda"), 2,
                 attn_impl="sdpa", kv_layout="paged")
    with pytest.raises(ValueError, match="fp8"):
        _alloc_caches(m, 1, 32, kv_dtype="fp8", kv_layout="paged")
    with pytest.raises(ValueError, match="share one block table"):
        ops.decode_attention(
            q, k, ops.PagedKV(v.pool, v.block_table.clone()), 5)
    with pytest.raises(ValueError, match="page size"):
        ops.PagedKV.zeros(1, 2, 48, 64, page_size=24, device="cuda")
    with pytest.raises(TypeError, match="both"):
        ops.decode_attention(q, k, v.gather(), 5)


# ---------------------------------------------------------------------------
# model level: the tiny configs of test_decode_attention_gpu.py, B = 2,
# capacity 48 (three pages of 16), permuted table
# ---------------------------------------------------------------------------

def _tiny(family, n_layer=3):
    torch.manual_seed(0)
    if family == "gpt2":
        return GPT2Model(GPT2Config(vocab_size=50304, n_layer=n_layer,
                                    n_head=8, dim=512, max_seq=64),
                         device="cuda", dtype=torch.bfloat16).eval()
    return LlamaModel(LlamaConfig(vocab_size=2048, n_layer=n_layer, n_head=8,
                                  n_kv_head=2, dim=512, ffn_dim=1024,
                                  max_seq=64),
                      device="cuda", dtype=torch.bfloat16).eval()


def _perm_table():
    return torch.tensor([[4, 1, 3], [0, 5, 2]], dtype=torch.int32,
                        device="cuda")


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_model_logits_equal_contiguous(family):
    m = _tiny(family)
    toks = torch.randint(0, m.cfg.vocab_size, (2, 12), device="cuda")
    dense = _alloc_caches(m, 2, 48)
    paged = _alloc_caches(m, 2, 48, kv_layout="paged",
                          block_table=_perm_table())
    assert paged[0][0].block_table is paged[-1][1].block_table
    for p0, p1 in [(0, 8), (8, 9), (9, 10), (10, 11), (11, 12)]:
        a = decode_forward(m, toks[:, p0:p1], dense, p0, attn_impl="hip")
        b = decode_forward(m, toks[:, p0:p1], paged, p0, attn_impl="hip")
        assert torch.equal(a, b), p0


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_tokens_equal_contiguous(family):
    # generate() builds its own (identity) table; 6 + 30 positions cross two
    # page edges per sequence, and batch row 1 starts at page 3
    m = _tiny(family)
    idx = torch.randint(0, m.cfg.vocab_size, (2, 6), device="cuda")
    assert torch.equal(generate(m, idx, 30, attn_impl="hip",
                                kv_layout="paged"),
                       generate(m, idx, 30, attn_impl="hip"))
    d = _tiny(family, n_layer=1)
    assert torch.equal(
        speculative_generate(m, d, idx[:1], 30, k=4, attn_impl="hip",
                             kv_layout="paged"),
        speculative_generate(m, d, idx[:1], 30, k=4, attn_impl="hip"))


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_graph_follows_rewritten_table(family):
    m = _tiny(family)
    idx = torch.randint(0, m.cfg.vocab_size, (2, 6), device="cuda")
    want = GraphedDecoder(m, batch=2, max_seq=48,
                          attn_impl="hip").generate(idx, 20)
    dec = GraphedDecoder(m, batch=2, max_seq=48, attn_impl="hip",
                         kv_layout="paged")
    dec.caches[0][0].block_table.copy_(_perm_table())
    assert torch.equal(dec.generate(idx, 20), want)


def test_prefill_gather_route_equals_contiguous():
    m = _tiny("llama")                  # G = 4: 24 rows -> 96 per kv head
    toks = torch.randint(0, m.cfg.vocab_size, (2, 24), device="cuda")
    prev = ops.set_prefill_attention(True)
    try:
        a = decode_forward(m, toks, _alloc_caches(m, 2, 48), 0,
                           all_logits=True, attn_impl="hip")
        b = decode_forward(m, toks,
                           _alloc_caches(m, 2, 48, kv_layout="paged",
                                         block_table=_perm_table()), 0,
                           all_logits=True, attn_impl="hip")
    finally:
        ops.set_prefill_attention(prev)
    assert torch.equal(a, b)
