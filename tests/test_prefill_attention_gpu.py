"""Flash-prefill attention kernel (ops/csrc/prefill_attn.hip) against the CPU
fp32 oracle, and the ``TDPA_PREFILL_ATTN`` route of the hip decode path.

Bound for the kernel: max abs error < 3e-2, the project's bound for flash
forward; the oracle runs fp32 math on the same bf16 inputs and every expected
value is asserted |v| < 8.  The kernel's tiles: 16-row wave tiles, 32-key
tiles, and a workgroup position tile of 16 * pos_tile rows (pos_tile <= 16/G;
the automatic choice at these sizes is 1, so each case also forces the
largest, which runs the two-wave-tiles-per-wave arm for G = 3, 4, 8)."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
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
    want = ops.prefill_attention(q.float().cpu(), kc.float().cpu(),
                                 vc.float().cpu(), pos)
    assert want.abs().max().item() < 8
    return want


def _check(q, kb, vb, pos0, tag, pos_tiles=(None,)):
    Sq = q.shape[2]
    p = pos0.tolist() if torch.is_tensor(pos0) else [pos0] * B
    k2, v2 = _poisoned(kb, vb, [x + Sq for x in p])
    want = _oracle(q, *_views(kb, vb), pos0)
    for pos_tile in pos_tiles:
        got = ops.prefill_attention(q, k2, v2, pos0, pos_tile=pos_tile)
        assert got.shape == q.shape and got.dtype == torch.bfloat16
        gotf = got.float().cpu()
        assert torch.isfinite(gotf).all(), (tag, pos_tile)
        err = (gotf - want).abs().max().item()
        print(f"prefill_attention {tag} tile {pos_tile}: max abs err "
              f"{err:.3e}")
        assert err < BOUND, (tag, pos_tile, err)


@pytest.mark.parametrize("Sq", [5, 17, 33, 100])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (8, 1), (3, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_vs_oracle(D, heads, Sq):
    # Sq crosses the 16-row wave tile, the 32-key tile and the forced
    # workgroup position tiles (32 rows at G = 8, 64 at G = 4, 80 at G = 3);
    # pos0 = 62 puts the frontier across the 64-key edge
    Hq, Hkv = heads
    q, kb, vb = _make(Hq, Hkv, D, Sq)
    for pos0 in (0, 62, SMAX - Sq):
        _check(q, kb, vb, pos0, f"D{D} H{Hq}/{Hkv} Sq{Sq} pos{pos0}",
               (None, 16))


@pytest.mark.parametrize("Hq,Hkv,D,Sq,pos0", [(8, 2, 128, 33, 62),
                                              (4, 4, 64, 100, 156),
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
        for pos_tile in (None, 16):
            got = ops.prefill_attention(q, kc, vc, pos, pos_tile=pos_tile)
            assert torch.equal(got, want), (pos, pos_tile)


def test_per_row_lengths_tensor_pos_and_capture():
    q, kb, vb = _make(8, 2, 128, 40, seed=1)
    _check(q, kb, vb, torch.tensor([9, 150], device="cuda"), "per-row pos")
    kc, vc = _views(kb, vb)
    a = ops.prefill_attention(q, kc, vc, 130)
    b = ops.prefill_attention(q, kc, vc, torch.tensor([130], device="cuda"))
    assert torch.equal(a, b)

    q = q[:, :, :24].contiguous()
    pos_t = torch.tensor([40], device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.prefill_attention(q, kc, vc, pos_t)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.prefill_attention(q, kc, vc, pos_t)
    for p in (40, 41, 42):
        graph.replay()
        torch.cuda.synchronize()
        err = (out.float().cpu() - _oracle(q, kc, vc, p)).abs().max().item()
        assert err < BOUND, (p, err)
        pos_t += 1


def test_output_layout_and_errors():
    q, kb, vb = _make(8, 2, 128, 19, seed=2)
    o = ops.prefill_attention(q, *_views(kb, vb), 100)
    flat = o.permute(2, 0, 1, 3).reshape(19, B, 8 * 128)
    assert flat.is_contiguous() and flat.data_ptr() == o.data_ptr()
    q = torch.zeros(1, 2, 4, 96, device="cuda", dtype=torch.bfloat16)
    kv = torch.zeros(1, 2, 64, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head dim"):
        ops.prefill_attention(q, kv, kv, 0)
    q = torch.zeros(1, 2, 4, 64, device="cuda")
    kv = torch.zeros(1, 2, 64, 64, device="cuda")
    with pytest.raises(TypeError, match="bf16"):
        ops.prefill_attention(q, kv, kv, 0)


def test_llama_prefill_route_matches_training_path_and_knob_off():
    from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=2048, n_layer=3, n_head=8, n_kv_head=2,
                      dim=512, ffn_dim=1024, max_seq=64)
    m = LlamaModel(cfg, device="cuda", dtype=torch.bfloat16).eval()
    toks = torch.randint(0, cfg.vocab_size, (2, 24), device="cuda")
    off = generate(m, toks, 24, attn_impl="hip")
    prev = ops.set_prefill_attention(True)
    try:
        with torch.no_grad():
            full = m(toks)["logits"].float()
        logits = decode_forward(m, toks, _alloc_caches(m, 2, 24), 0,
                                attn_impl="hip").float()
        diff = (logits - full[:, -1]).abs().max().item()
        assert diff < 0.25, diff
        on = generate(m, toks, 24, attn_impl="hip")
    finally:
        ops.set_prefill_attention(prev)
    assert on.shape == off.shape == (2, 48)
    assert torch.equal(on[:, :12], off[:, :12])
    agree = (on == off).float().mean().item()
    new = (on[:, 24:] == off[:, 24:]).float().mean().item()
    print(f"knob on vs off: agreement {agree:.3f}, new tokens {new:.3f}")
    assert agree >= 0.8, agree
