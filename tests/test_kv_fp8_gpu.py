"""fp8 (e4m3) KV cache on the GPU: the dequantise and append kernels
(ops/csrc/kv_fp8.hip) against the CPU rule, bit for bit, and the fp8 decode
attention kernel (ops/csrc/decode_attn_fp8.hip) against the CPU fp32 oracle
on the dequantised cache.

Bound for the attention kernel: max abs error < 3e-2, the bound of
test_decode_attention_gpu.py; the quantisation is common to both sides, so
only kernel arithmetic is measured.  Every expected value is asserted
|v| < 8."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.inference.generate import (GraphedDecoder,
                                                     _alloc_caches,
                                                     decode_forward)
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel

pytestmark = pytest.mark.gpu

B, SMAX = 2, 256
BOUND = 3e-2
LENGTHS = [1, 63, 64, 65, 128, 200, 256]   # pos0 + 1, chunk edges at 64


def test_dequantise_all_256_codes():
    """Settles on hardware that the gfx950 converter is OCP e4m3."""
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).float()
    kv = ops.Fp8KV(codes.view(1, 1, 4, 64).cuda(),
                   torch.ones(1, 1, 4, device="cuda"))
    for dtype in (torch.float32, torch.bfloat16):
        got = kv.dequantize(dtype).float().cpu().reshape(256)
        nan = want.isnan()
        assert nan.sum() == 2 and got[nan].isnan().all(), dtype
        assert torch.equal(got[~nan], want[~nan]), dtype


@pytest.mark.parametrize("pos", [7, [7], [7, 250]])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("D", [64, 128])
def test_append_is_byte_exact(D, S, pos):
    Hkv = 2
    g = torch.Generator(device="cuda").manual_seed(S)
    # k and v are strided views of one fused (S, B, 3*Hkv*D) buffer
    buf = torch.randn(S, B, 3 * Hkv * D, generator=g, device="cuda",
                      dtype=torch.bfloat16)
    k, v = (buf.narrow(-1, o * Hkv * D, Hkv * D).view(S, B, Hkv, D)
            .permute(1, 2, 0, 3) for o in (1, 2))
    k[0, 0, 0] = 0                      # all-zero row
    k[0, 1, 0, 0] = 448 * 8             # amax exactly 448 * 2^3 ...
    k[1, 0, 0, 0] = 448 * 8 + 16        # ... and one bf16 step above
    v[0, 0, 0] *= 1e4                   # magnitude ~3e4
    v[1, 1, 0] *= 1e-6
    caches = [ops.Fp8KV(torch.full((B, Hkv, SMAX, D), 0x55, device="cuda",
                                   dtype=torch.uint8),
                        torch.full((B, Hkv, SMAX), 7.0, device="cuda"))
              for _ in range(2)]
    pos0 = pos if isinstance(pos, int) else torch.tensor(pos, device="cuda")
    ops.kv_cache_append(caches[0], caches[1], k, v, pos0)
    rows = [pos] * B if isinstance(pos, int) else pos * (B // len(pos))
    for cache, x in zip(caches, (k, v)):
        data, scale = ops.quantize_kv_rows(x.cpu())        # the CPU rule
        want_d = torch.full((B, Hkv, SMAX, D), 0x55, dtype=torch.uint8)
        want_s = torch.full((B, Hkv, SMAX), 7.0)
        for b, p in enumerate(rows):
            want_d[b, :, p:p + S] = data[b]
            want_s[b, :, p:p + S] = scale[b]
        assert torch.equal(cache.scale.cpu(), want_s)
        assert torch.equal(cache.data.cpu(), want_d)


def _make(Hq, Hkv, D, Sq, seed=0):
    """bf16 q, fp8 caches written by kv_cache_append, and their fp32 values
    on the CPU for the oracle.  Row magnitudes vary by key with coprime
    periods (K x{1/4..4}, V x{1/4..1}), so a wrong scale index fails."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device="cuda",
                           dtype=torch.bfloat16)

    j = torch.arange(SMAX, device="cuda")
    km = torch.tensor([.25, .5, 1, 2, 4], device="cuda")[j % 5]
    vm = torch.tensor([.25, .5, 1], device="cuda")[j % 3]
    k = rn(B, Hkv, SMAX, D) * km[:, None].bfloat16()
    v = rn(B, Hkv, SMAX, D) * vm[:, None].bfloat16()
    kc, vc = (ops.Fp8KV.zeros(B, Hkv, SMAX, D, device="cuda")
              for _ in range(2))
    ops.kv_cache_append(kc, vc, k, v, 0)
    ref = (kc.dequantize(torch.float32).cpu(),
           vc.dequantize(torch.float32).cpu())
    return rn(B, Hq, Sq, D), kc, vc, ref


def _oracle(q, ref, pos0):
    pos = pos0.cpu() if torch.is_tensor(pos0) else pos0
    want = ops.decode_attention(q.float().cpu(), ref[0], ref[1], pos)
    assert want.abs().max().item() < 8
    return want


def _check(q, kc, vc, ref, pos0, split_kv, tag):
    """Kernel on a copy of the caches whose dead slots hold byte 0x7F (NaN)
    under a NaN scale, against the oracle on the clean values."""
    Sq = q.shape[2]
    p = pos0.reshape(-1).tolist() if torch.is_tensor(pos0) else [pos0]
    k2, v2 = (ops.Fp8KV(c.data.clone(), c.scale.clone()) for c in (kc, vc))
    for b, n in enumerate(p * (B // len(p))):
        for c in (k2, v2):
            c.data[b, :, n + Sq:] = 0x7F
            c.scale[b, :, n + Sq:] = float("nan")
    got = ops.decode_attention(q, k2, v2, pos0, split_kv=split_kv)
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    gotf = got.float().cpu()
    assert torch.isfinite(gotf).all(), tag
    err = (gotf - _oracle(q, ref, pos0)).abs().max().item()
    print(f"decode_attention fp8 {tag}: max abs err {err:.3e}")
    assert err < BOUND, (tag, err)
    return got


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (8, 1)])
def test_kernel_vs_oracle_forced_splits(D, heads):
    Hq, Hkv = heads
    made = _make(Hq, Hkv, D, 1)
    for n in LENGTHS:
        _check(*made, n - 1, 64, f"D{D} H{Hq}/{Hkv} len{n}")


@pytest.mark.parametrize("split_kv", [None, 256])
def test_auto_split_and_single_split(split_kv):
    made = _make(8, 2, 128, 1, seed=1)
    for n in (1, 65, 200, 256):
        _check(*made, n - 1, split_kv, f"split{split_kv} len{n}")


@pytest.mark.parametrize("Sq,G", [(1, 1), (2, 1), (4, 1), (2, 4), (4, 4),
                                  (3, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_rows_per_kv_head_and_causal_alignment(Sq, G, D):
    # M = G*Sq hits 1, 2, 4, 8, 16 and a padded 6; pos0 = 62 puts the last
    # visible keys on both sides of a chunk edge
    made = _make(2 * G, 2, D, Sq, seed=2)
    for pos0 in (62, 0, SMAX - Sq):
        _check(*made, pos0, 64, f"Sq{Sq} G{G} D{D} pos{pos0}")


def test_row_blocking_per_row_positions_and_tensor_pos():
    # G*Sq = 20 > 16: the wrapper issues one call per block of 4 rows
    made = _make(8, 2, 64, 5, seed=3)
    _check(*made, 61, 64, "blocked Sq5 G4")
    q, kc, vc, ref = _make(8, 2, 128, 2, seed=5)
    _check(q, kc, vc, ref, torch.tensor([9, 199], device="cuda"), 64,
           "per-row pos [9,199]")
    a = ops.decode_attention(q, kc, vc, 130, split_kv=64)
    b = ops.decode_attention(q, kc, vc, torch.tensor([130], device="cuda"),
                             split_kv=64)
    assert torch.equal(a, b)
    flat = a.permute(2, 0, 1, 3).reshape(2, B, 8 * 128)
    assert flat.is_contiguous() and flat.data_ptr() == a.data_ptr()


def test_graph_holds_append_and_attention():
    q, kc, vc, _ = _make(8, 2, 128, 1, seed=7)
    g = torch.Generator(device="cuda").manual_seed(8)
    k1, v1 = (torch.randn(B, 2, 1, 128, generator=g, device="cuda",
                          dtype=torch.bfloat16) for _ in range(2))
    pos_t = torch.tensor([63], device="cuda")

    def step():
        ops.kv_cache_append(kc, vc, k1, v1, pos_t)
        return ops.decode_attention(q, kc, vc, pos_t, split_kv=64)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    data1, scale1 = ops.quantize_kv_rows(k1.cpu())
    for p in (63, 64, 65):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(kc.data[:, :, p:p + 1].cpu(), data1), p
        assert torch.equal(kc.scale[:, :, p:p + 1].cpu(), scale1), p
        ref = (kc.dequantize(torch.float32).cpu(),
               vc.dequantize(torch.float32).cpu())
        err = (out.float().cpu() - _oracle(q, ref, p)).abs().max().item()
        assert err < BOUND, (p, err)
        pos_t += 1


# ---------------------------------------------------------------------------
# model level: the tiny models and criteria of test_decode_attention_gpu.py
# ---------------------------------------------------------------------------

# Teacher-forced logits against the training stack: 0.25, the bound of the
# hip route on a bf16 cache, plus 2 * q.  q is the quantisation's own effect,
# measured with the reference alone: on the CPU in fp32, same configs, seeds
# and token shapes, the max abs logit difference between the fp8-cache route
# and the exact-cache route (Q_GPT2, Q_LLAMA below; docs/design/inference.md
# "fp8 KV cache" has the runs).  The factor 2: the GPU quantiser sees
# bf16-noisy inputs and may round isolated elements the other way.
# Measured at seed 0: gpt2 0.0909 (seeds 1, 2: 0.0823, 0.0732), llama 0.0687
# (0.0736, 0.0685), on logits of magnitude up to 3.1 and 2.2; the bounds are
# 0.25 + 2 * 0.091 = 0.432 and 0.25 + 2 * 0.069 = 0.388.
Q_GPT2, Q_LLAMA = 0.091, 0.069


def _gpt2(n_head, dim):
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=50304, n_layer=4, n_head=n_head, dim=dim,
                     max_seq=64)
    return GPT2Model(cfg, device="cuda", dtype=torch.bfloat16).eval()


def _tiny_gqa_llama():
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=2048, n_layer=3, n_head=8, n_kv_head=2,
                      dim=512, ffn_dim=1024, max_seq=64)
    return LlamaModel(cfg, device="cuda", dtype=torch.bfloat16).eval()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_decode_logits_fp8_match_training_path(family):
    m, q = (_gpt2(12, 768), Q_GPT2) if family == "gpt2" else \
        (_tiny_gqa_llama(), Q_LLAMA)
    toks = torch.randint(0, m.cfg.vocab_size, (2, 24), device="cuda")
    with torch.no_grad():
        full = m(toks)["logits"].float()        # training stack, (B, T, V)
    caches = _alloc_caches(m, 2, 24, kv_dtype="fp8")
    pos0, chunk, worst = 0, toks[:, :8], 0.0
    while chunk.shape[1] > 0:
        logits = decode_forward(m, chunk, caches, pos0,
                                attn_impl="hip").float()
        pos0 += chunk.shape[1]
        worst = max(worst, (logits - full[:, pos0 - 1]).abs().max().item())
        chunk = toks[:, pos0:pos0 + 1]
    print(f"fp8 kv {family}: max abs logit diff {worst:.4f}")
    assert worst < 0.25 + 2 * q, worst


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_graphed_decoder_fp8_vs_eager_fp8(family):
    m = _gpt2(8, 512) if family == "gpt2" else _tiny_gqa_llama()
    S0, n = (8, 24) if family == "gpt2" else (6, 20)
    idx = torch.randint(0, m.cfg.vocab_size, (2, S0), device="cuda")
    dec = GraphedDecoder(m, batch=2, max_seq=S0 + n + 16, attn_impl="hip",
                         kv_dtype="fp8")
    assert isinstance(dec.caches[0][0], ops.Fp8KV)
    out_g = dec.generate(idx, n)
    out_e = generate(m, idx, n, attn_impl="hip", kv_dtype="fp8")
    assert out_g.shape == out_e.shape == (2, S0 + n)
    assert torch.equal(out_g[:, :12], out_e[:, :12])
    agree = (out_g == out_e).float().mean().item()
    assert agree >= 0.8, agree
