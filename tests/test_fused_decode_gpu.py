"""Fused decode-step kernels (ops/csrc/fused_decode.hip) against fp64 and,
bit for bit, against the compositions they replace; then the Llama decode
path with the knob on against the knob off.

Bounds: a result rounded once to bf16 from an fp32 value that is itself good
to far below a bf16 ulp sits within one bf16 ulp, ``2**-7 * |ref|``, of the
fp64 value (2**-8 for the rounding, the rest for the fp32 sigmoid / rsqrt /
two-term sum)."""
import pytest
import torch

from tests import numerics_helpers as nh
from torchdistpackage_amd import ops
from torchdistpackage_amd.inference.generate import (GraphedDecoder,
                                                     _alloc_caches,
                                                     decode_forward)
from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -7
SENTINEL = 768.0          # finite, exact in bf16, far outside randn


def _cuda(*ts):
    return [t.cuda() for t in ts]


# ------------------------------------------------------------ swiglu_linear

@pytest.mark.parametrize("N,K", [(8, 64), (10, 2112), (7, 4104)])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
def test_swiglu_linear(M, N, K):
    from torchdistpackage_amd.ops.gemm import decode_route, linear
    fused = ops.swiglu_linear
    if decode_route(M, N, K) != "gemv":
        # M > 4 at K = 4104: linear() sends these to hipBLASLt, so the op
        # returns the composition.  The kernel's MT = 8 arm still has to
        # cross two x tiles + 8: it and the GEMV it mirrors run through
        # their bindings here
        assert M > 4 and K > 4096
        fused = ops.ext().gemv_swiglu

        def linear(x, w):
            return ops.ext().gemv_bf16(x, w, None)
    g = nh._gen("swiglu_linear", M, N, K)
    x, w1, w3 = _cuda(*(nh._randn(s, g).to(torch.bfloat16)
                        for s in ((M, K), (N, K), (N, K))))
    # ops.swiglu takes multiples of 8 elements: the composition runs on the
    # weights padded with zero rows to 16 (a GEMV column does not depend on N)
    pad = torch.zeros(16 - N, K, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        got = fused(x, w1, w3)
        want = ops.swiglu(linear(x, torch.cat([w1, pad])),
                          linear(x, torch.cat([w3, pad])))[:, :N]
        nh.check_equal(got, want, "randn vs composition")
        # exact family: integer weights, x in steps of 2**-6: the fp32
        # accumulation is exact, a and b are the dot products rounded once
        w1, w3 = _cuda(nh.int_mat("g", (N, K)), nh.int_mat("u", (N, K)))
        x = (nh.int_mat("x", (M, K)) * 2.0 ** -6).cuda()
        got = fused(x, w1, w3).double().cpu()
    a = nh.exact_mm_ref(x, w1).double()
    b = nh.exact_mm_ref(x, w3).double()
    ref = a * torch.sigmoid(a) * b
    err = (got - ref).abs()
    print(f"swiglu_linear M{M} N{N} K{K}: worst err/ulp "
          f"{(err / (ULP * ref.abs() + 2.0 ** -40)).max().item():.3f}")
    assert (err <= ULP * ref.abs() + 2.0 ** -40).all()


def test_swiglu_linear_fallbacks():
    g = nh._gen("swiglu_linear_fallbacks")
    w1, w3 = _cuda(*(nh._randn((16, 256), g).to(torch.bfloat16)
                     for _ in range(2)))
    x = nh._randn((9, 256), g).to(torch.bfloat16).cuda()
    from torchdistpackage_amd.ops.gemm import linear
    with torch.no_grad():
        nh.check_equal(ops.swiglu_linear(x, w1, w3),
                       ops.swiglu(linear(x, w1), linear(x, w3)), "M = 9")
        q1, q3 = (ops.Int4Weight(*ops.quantize_int4(w)) for w in (w1, w3))
        nh.check_equal(ops.swiglu_linear(x[:2], q1, q3),
                       ops.swiglu(linear(x[:2], q1), linear(x[:2], q3)),
                       "Int4Weight")


# ----------------------------------------------------------- rope_kv_append

RB, SMAX = 2, 24


def _rope_case(D, H, Hkv, S):
    """Permuted views of (S, B, heads*D) buffers, and cache views inside
    larger sentinel-filled allocations."""
    g = nh._gen("rope_kv_append", D, H, Hkv, S)

    def proj(heads):
        t = nh._randn((S, RB, heads * D), g).to(torch.bfloat16).cuda()
        return t.reshape(S, RB, heads, D).permute(1, 2, 0, 3)

    kb = torch.full((RB, Hkv, SMAX + 16, D), SENTINEL, device="cuda",
                    dtype=torch.bfloat16)
    vb = torch.full((RB, Hkv, SMAX + 24, D), SENTINEL, device="cuda",
                    dtype=torch.bfloat16)
    kc, vc = kb.narrow(2, 8, SMAX), vb.narrow(2, 16, SMAX)
    assert not kc.is_contiguous() and not vc.is_contiguous()
    cos, sin = _cuda(*nh.rope_tables(SMAX + 4, D))
    return proj(H), proj(Hkv), proj(Hkv), cos, sin, kb, vb, kc, vc


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_kv_append(D, H, Hkv, S):
    q, k, v, cos, sin, kb, vb, kc, vc = _rope_case(D, H, Hkv, S)
    for p in (0, SMAX - S):
        want_q = ops.rope_rotate_half(q, cos, sin, p)
        want_k = ops.rope_rotate_half(k, cos, sin, p)
        for pos0 in (p, torch.tensor([p], device="cuda")):
            kb.fill_(SENTINEL), vb.fill_(SENTINEL)
            with torch.no_grad():
                got_q = ops.rope_kv_append(q, k, v, cos, sin, kc, vc, pos0)
            assert got_q.is_contiguous()
            nh.check_equal(got_q, want_q, f"q pos {pos0}")
            nh.check_equal(kc[:, :, p:p + S], want_k, f"k rows pos {pos0}")
            nh.check_equal(vc[:, :, p:p + S], v, f"v rows pos {pos0}")
            # nothing else in either allocation was written
            kc[:, :, p:p + S] = SENTINEL
            vc[:, :, p:p + S] = SENTINEL
            assert (kb == SENTINEL).all() and (vb == SENTINEL).all()
        # fp64 RoPE on the same bf16 inputs and fp32 tables: one rounding
        # of a two-term fp32 sum
        for got, x in ((want_q, q), (want_k, k)):
            ref = nh.rope_formula(x.double(), cos.double(), sin.double(), p)
            mag = x[..., :D // 2].double().abs() + x[..., D // 2:].double().abs()
            assert ((got.double() - ref).abs()
                    <= ULP * torch.cat([mag, mag], -1)).all()


def test_rope_kv_append_capture_and_errors():
    q, k, v, cos, sin, kb, vb, kc, vc = _rope_case(128, 4, 2, 1)
    pos_t = torch.tensor([3], device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        ops.rope_kv_append(q, k, v, cos, sin, kc, vc, pos_t)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    kb.fill_(SENTINEL), vb.fill_(SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = ops.rope_kv_append(q, k, v, cos, sin, kc, vc, pos_t)
    kb.fill_(SENTINEL), vb.fill_(SENTINEL)
    for p in (3, 4, 5):
        graph.replay()
        torch.cuda.synchronize()
        nh.check_equal(out, ops.rope_rotate_half(q, cos, sin, p), f"q {p}")
        nh.check_equal(kc[:, :, p:p + 1],
                       ops.rope_rotate_half(k, cos, sin, p), f"k {p}")
        nh.check_equal(vc[:, :, p:p + 1], v, f"v {p}")
        pos_t += 1
    assert (kc[:, :, :3] == SENTINEL).all() and (kc[:, :, 6:] == SENTINEL).all()
    assert (vc[:, :, :3] == SENTINEL).all() and (vc[:, :, 6:] == SENTINEL).all()
    for bad in (-1, SMAX):
        with pytest.raises(ValueError, match="pos0"):
            ops.rope_kv_append(q, k, v, cos, sin, kc, vc, bad)
    f8 = ops.Fp8KV.zeros(RB, 2, SMAX, 128, device="cuda")
    with pytest.raises(TypeError, match="kv_cache_append"):
        ops.rope_kv_append(q, k, v, cos, sin, f8, f8, 0)


# ------------------------------------------------------------- add_rms_norm

@pytest.mark.parametrize("D", [64, 2056, 4096, 8200])
@pytest.mark.parametrize("rows", [1, 3])
def test_add_rms_norm(rows, D):
    eps = 1e-5
    g = nh._gen("add_rms_norm", rows, D)
    x, y, w = _cuda(*(nh._randn(s, g).to(torch.bfloat16)
                      for s in ((rows, D), (rows, D), (D,))))
    with torch.no_grad():
        x_new, h = ops.add_rms_norm(x, y, w, eps)
        nh.check_equal(x_new, x + y, "x_new vs x + y")
        nh.check_equal(h, ops.rms_norm(x + y, w, eps), "h vs rms_norm")
    x64 = (x.double() + y.double()).to(torch.bfloat16)
    nh.check_equal(x_new, x64, "x_new vs fp64 sum rounded once")
    ref = nh.rms_norm_formula(x64.double(), w.double(), eps)
    assert ((h.double() - ref).abs() <= ULP * ref.abs() + 2.0 ** -40).all()


# ------------------------------------------------ model: knob on against off

@pytest.fixture(scope="module")
def llama():
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=2048, n_layer=3, n_head=8, n_kv_head=2,
                      dim=512, ffn_dim=1024, max_seq=64)
    m = LlamaModel(cfg, device="cuda", dtype=torch.bfloat16).eval()
    toks = torch.randint(0, cfg.vocab_size, (2, 10), device="cuda")
    return m, toks


def _run(m, toks, on, attn_impl, **cache_kw):
    """Logits of a 7-token chunk and three single-token steps, and the
    caches they leave."""
    prev = ops.set_fused_decode(on)
    try:
        caches = _alloc_caches(m, 2, 32, **cache_kw)
        out = [decode_forward(m, toks[:, :7], caches, 0, all_logits=True,
                              attn_impl=attn_impl)]
        for p in (7, 8, 9):
            out.append(decode_forward(m, toks[:, p:p + 1], caches, p,
                                      attn_impl=attn_impl))
        return out, caches
    finally:
        ops.set_fused_decode(prev)


def _dense(c):
    if isinstance(c, ops.Fp8KV):
        return c.data
    return c.pool if isinstance(c, ops.PagedKV) else c


@pytest.mark.parametrize("attn_impl,cache_kw,bits", [
    ("sdpa", {}, None), ("hip", {}, None), ("hip", {"kv_dtype": "fp8"}, None),
    ("hip", {"kv_layout": "paged"}, None), ("hip", {}, 4)])
def test_llama_knob_on_equals_off(llama, attn_impl, cache_kw, bits):
    m, toks = llama
    if bits:
        import copy
        m = copy.deepcopy(m)
        assert ops.quantize_linears_(m, bits=bits) > 0
    off, c_off = _run(m, toks, False, attn_impl, **cache_kw)
    on, c_on = _run(m, toks, True, attn_impl, **cache_kw)
    for i, (a, b) in enumerate(zip(on, off)):
        nh.check_equal(a, b, f"logits of call {i}")
    for layer, (a, b) in enumerate(zip(c_on, c_off)):
        for x, y in zip(a, b):
            assert torch.equal(_dense(x), _dense(y)), f"cache, layer {layer}"


def test_graphed_decoder_knob_on_equals_off(llama):
    m, toks = llama
    runs = []
    for on in (False, True):
        prev = ops.set_fused_decode(on)
        try:
            dec = GraphedDecoder(m, batch=2, max_seq=32, attn_impl="hip")
            dec.prefill(toks[:, :7])
            runs.append(torch.stack([dec.step() for _ in range(8)]))
        finally:
            ops.set_fused_decode(prev)
    assert torch.equal(runs[0], runs[1])
