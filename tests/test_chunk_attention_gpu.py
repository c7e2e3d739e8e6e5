"""Split-KV chunk attention kernel (ops/csrc/chunk_attn.hip) against the CPU
fp32 oracle, and the ``TDPA_CHUNK_ATTN`` route of the hip decode path.

Bound for the kernel: max abs error < 3e-2, the project's bound for flash
forward; the oracle runs fp32 math on the same bf16 inputs and every expected
value is asserted |v| < 8.  The kernel's tiles: RT = 1, 2 or 4 16-row tiles
(M = G * Sq up to 16, 32, 64), 32-key wave steps, and a KV chunk that is 64
keys here by default; 128 gives every wave a step and 256 is the single
split that writes bf16 itself."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference.generate import (_alloc_caches,
                                                     decode_forward)

pytestmark = pytest.mark.gpu

B, SMAX = 2, 256
BOUND = 3e-2
NAN = float("nan")


def _make(Hq, Hkv, D, Sq, seed=0):
    """bf16 q and the two larger allocations the caches are views of."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device="cuda",
                           dtype=torch.bfloat16)

    return rn(B, Hq, Sq, D), rn(B, Hkv, SMAX + 32, D), rn(B, Hkv, SMAX + 48, D)


def _views(kb, vb):
    kc, vc = kb.narrow(2, 16, SMAX), vb.narrow(2, 24, SMAX)
    assert not kc.is_contiguous() and not vc.is_contiguous()
    return kc, vc


def _poisoned(kb, vb, first_dead):
    """Copies whose margins, and every slot from ``first_dead[b]`` on, are
    NaN."""
    kb, vb = kb.clone(), vb.clone()
    kc, vc = _views(kb, vb)
    kb[:, :, :16], kb[:, :, 16 + SMAX:] = NAN, NAN
    vb[:, :, :24], vb[:, :, 24 + SMAX:] = NAN, NAN
    for b, n in enumerate(first_dead):
        kc[b, :, n:], vc[b, :, n:] = NAN, NAN
    return kc, vc


def _oracle(q, kc, vc, pos0):
    pos = pos0.cpu() if torch.is_tensor(pos0) else pos0
    want = ops.chunk_attention(q.float().cpu(), kc.float().cpu(),
                               vc.float().cpu(), pos)
    assert want.abs().max().item() < 8
    return want


def _check(q, kb, vb, pos0, tag, splits=(None,)):
    Sq = q.shape[2]
    p = pos0.tolist() if torch.is_tensor(pos0) else [pos0] * B
    k2, v2 = _poisoned(kb, vb, [x + Sq for x in p])
    want = _oracle(q, *_views(kb, vb), pos0)
    for split_kv in splits:
        got = ops.chunk_attention(q, k2, v2, pos0, split_kv=split_kv)
        assert got.shape == q.shape and got.dtype == torch.bfloat16
        gotf = got.float().cpu()
        assert torch.isfinite(gotf).all(), (tag, split_kv)
        err = (gotf - want).abs().max().item()
        print(f"chunk_attention {tag} split {split_kv}: max abs err "
              f"{err:.3e}")
        assert err < BOUND, (tag, split_kv, err)


@pytest.mark.parametrize("Hq,Hkv,Sq", [(4, 4, 17), (8, 2, 5), (8, 2, 8),
                                       (3, 1, 11), (8, 1, 8), (8, 1, 3)])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_vs_oracle(D, Hq, Hkv, Sq):
    # M = 17, 20, 32, 33, 64, 24: every RT, a ragged last row tile, G of 1,
    # 3, 4 and 8; pos0 = 62 puts the frontier across the 64-key split edge,
    # so some rows see nothing of the second split while others do
    q, kb, vb = _make(Hq, Hkv, D, Sq)
    for pos0 in (0, 62, SMAX - Sq):
        _check(q, kb, vb, pos0, f"D{D} H{Hq}/{Hkv} Sq{Sq} pos{pos0}",
               (None, 128, 256))


@pytest.mark.parametrize("Hq,Hkv,D,Sq,pos0", [(8, 2, 128, 8, 62),
                                              (4, 4, 64, 9, 156),
                                              (3, 1, 64, 17, 0),
                                              (8, 1, 128, 5, 251)])
def test_frontier_needle_bit_exact(Hq, Hkv, D, Sq, pos0):
    # consecutive keys score 128 nats apart: every row's fp32 softmax is
    # exactly one-hot on its last visible key, so the output IS that V row
    q = torch.zeros(B, Hq, Sq, D, device="cuda", dtype=torch.bfloat16)
    q[..., 0] = 1024
    kc = torch.zeros(B, Hkv, SMAX, D, device="cuda", dtype=torch.bfloat16)
    kc[..., 0] = torch.arange(SMAX, device="cuda")[None, None]
    vc = torch.randn(B, Hkv, SMAX, D, device="cuda", dtype=torch.bfloat16)
    for pos in (pos0, torch.tensor([9, 150], device="cuda")):
        p = pos if torch.is_tensor(pos) else torch.full((B,), pos,
                                                        device="cuda")
        rows = p[:, None] + torch.arange(Sq, device="cuda")      # (B, Sq)
        want = vc[torch.arange(B, device="cuda")[:, None], :, rows]
        want = want.permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1)
        for split_kv in (None, 256):
            got = ops.chunk_attention(q, kc, vc, pos, split_kv=split_kv)
            assert torch.equal(got, want), (pos, split_kv)


def test_per_row_lengths_tensor_pos_and_capture():
    q, kb, vb = _make(8, 2, 128, 10, seed=1)                 # M = 40
    _check(q, kb, vb, torch.tensor([9, 150], device="cuda"), "per-row pos")
    kc, vc = _views(kb, vb)
    a = ops.chunk_attention(q, kc, vc, 130)
    b = ops.chunk_attention(q, kc, vc, torch.tensor([130], device="cuda"))
    assert torch.equal(a, b)

    q = q[:, :, :8].contiguous()                             # M = 32
    pos_t = torch.tensor([60], device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.chunk_attention(q, kc, vc, pos_t)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.chunk_attention(q, kc, vc, pos_t)
    for p in (60, 61, 62):
        graph.replay()
        torch.cuda.synchronize()
        err = (out.float().cpu() - _oracle(q, kc, vc, p)).abs().max().item()
        assert err < BOUND, (p, err)
        pos_t += 1


def test_output_layout_and_errors():
    q, kb, vb = _make(8, 2, 128, 7, seed=2)
    o = ops.chunk_attention(q, *_views(kb, vb), 100)
    flat = o.permute(2, 0, 1, 3).reshape(7, B, 8 * 128)
    assert flat.is_contiguous() and flat.data_ptr() == o.data_ptr()
    kc, vc = _views(kb, vb)
    with pytest.raises(ValueError, match="prefill_attention"):
        ops.chunk_attention(_make(5, 1, 128, 13)[0], kc[:, :1], vc[:, :1], 0)
    q = torch.zeros(1, 2, 4, 96, device="cuda", dtype=torch.bfloat16)
    kv = torch.zeros(1, 2, 64, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head dim"):
        ops.chunk_attention(q, kv, kv, 0)
    q = torch.zeros(1, 2, 4, 64, device="cuda")
    kv = torch.zeros(1, 2, 64, 64, device="cuda")
    with pytest.raises(TypeError, match="bf16"):
        ops.chunk_attention(q, kv, kv, 0)
    f8 = ops.Fp8KV.zeros(1, 2, 64, 64, device="cuda")
    with pytest.raises(TypeError, match="Fp8KV"):
        ops.chunk_attention(q.bfloat16(), f8, f8, 0)


def test_llama_chunk_route_matches_training_path_and_knob_off():
    from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=2048, n_layer=3, n_head=8, n_kv_head=2,
                      dim=512, ffn_dim=1024, max_seq=64)
    m = LlamaModel(cfg, device="cuda", dtype=torch.bfloat16).eval()
    toks = torch.randint(0, cfg.vocab_size, (2, 32), device="cuda")
    with torch.no_grad():
        full = m(toks)["logits"].float()

    @torch.no_grad()
    def chunk_logits():
        # prefill 24 (96 rows per kv head: not this route), then the 8-token
        # chunk at pos0 = 24 (G * S = 32 rows)
        caches = _alloc_caches(m, 2, 32)
        decode_forward(m, toks[:, :24], caches, 0, attn_impl="hip")
        return decode_forward(m, toks[:, 24:], caches, 24, attn_impl="hip",
                              all_logits=True).float()

    off, off2 = chunk_logits(), chunk_logits()
    assert torch.equal(off, off2)
    prev = ops.set_chunk_attention(True)
    try:
        on = chunk_logits()
    finally:
        ops.set_chunk_attention(prev)
    assert on.shape == full[:, 24:].shape
    assert (on - full[:, 24:]).abs().max().item() < 0.25
    assert (on - off).abs().max().item() < 0.25
