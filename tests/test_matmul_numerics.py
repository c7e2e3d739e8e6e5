"""Matmul-family numerics on the CPU: the generators, fp64 references and
checkers of tests/numerics_helpers.py run through the CPU paths
(``gemm.linear``, ``ops.decode_attention``, ``ops.rope_rotate_half``), and
the TEETH: deliberately wrong fp64 emulations of the GEMM / GEMV / split-K /
split-KV kernels that the same checkers must reject.  The HIP kernels meet
the same checkers in tests/test_matmul_numerics_gpu.py;
docs/design/kernels.md ("Matmul-family numerics") has the table.
"""

import math

import pytest
import torch
import torch.nn.functional as F

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.ops import gemm
from tests import numerics_helpers as nh

CPU = torch.device("cpu")
BF16 = torch.bfloat16


# ------------------------------------------------- exact family, CPU paths

@pytest.mark.parametrize("M,N,K", [(256, 256, 4096), (9, 7, 2056),
                                   (4, 1000, 8)])
def test_exact_reference_matches_torch_bf16_matmul(M, N, K):
    """torch's own bf16 matmul on the CPU reproduces the fp64-rounded-once
    reference bit for bit: the reference is what a correct kernel gives."""
    A = nh.int_mat("A", (M, K))
    B = nh.int_mat("B", (N, K))
    bias = nh.int_mat("bias", (N,))
    nh.check_equal(A @ B.t(), nh.exact_mm_ref(A, B), "A @ B^T")
    nh.check_equal(F.linear(A, B, bias), nh.exact_mm_ref(A, B, bias),
                   "F.linear")


@pytest.mark.parametrize("shape", [(256, 256, 256), (2, 4, 64, 72)],
                         ids=["2d", "4d-input"])
def test_exact_linear_cpu_fwd_bwd(shape):
    """gemm.linear on CPU tensors, forward and backward, against fp64
    autograd rounded once (dy in [-2, 2] keeps db exact)."""
    *lead, K, N = shape
    x = nh.int_mat("x", (*lead, K))
    w = nh.int_mat("w", (N, K))
    b = nh.int_mat("b", (N,))
    dy = nh.int_mat("dy", (*lead, N), -2, 2)
    y, grads = nh.fwd_bwd(gemm.linear, (x, w, b), dy, BF16, CPU)
    y_ref, g_ref = nh.fwd_bwd(F.linear, (x, w, b), dy, torch.float64, CPU)
    nh.check_equal(y, y_ref.to(BF16), "y")
    for n, g, gr in zip(("dx", "dw", "db"), grads, g_ref):
        nh.check_equal(g, gr.to(BF16), n)


def test_selection_matrix_selects_rows():
    A, idx = nh.selection_matrix("cpu", 40, 64)
    B = nh.mm_input("randn", 8, 24, 64)[1]                      # (24, 64)
    nh.check_equal(A @ B.t(), B.t()[idx], "selection")


# ----------------------------------------------------- exact family, teeth

def _slots(K):
    return [slice(s, s + 32) for s in range(0, K, 32)]


@pytest.mark.parametrize("K", [32, 96, 288, 4096])
@pytest.mark.parametrize("fault", ["slot_dropped", "slot_twice"])
def test_teeth_gemm_slot(K, fault):
    """A GEMM whose K loop skips one 32-deep slot, or runs it twice (the
    typical fault of a mis-counted LDS ring)."""
    A = nh.int_mat("A", (256, K))
    B = nh.int_mat("B", (256, K))
    A64, B64 = A.double(), B.double()
    ref = nh.exact_mm_ref(A, B)
    nh.check_equal((A64 @ B64.t()).to(BF16), ref, "sanity")
    for sl in (_slots(K)[0], _slots(K)[-1], _slots(K)[len(_slots(K)) // 2]):
        part = A64[:, sl] @ B64[:, sl].t()
        bad = A64 @ B64.t() + (part if fault == "slot_twice" else -part)
        with pytest.raises(AssertionError, match="elements differ"):
            nh.check_equal(bad.to(BF16), ref, fault)


@pytest.mark.parametrize("shape", [s for s in nh.GEMV_SHAPES if s[2] > 8][::4],
                         ids=nh.gemv_id)
def test_teeth_gemv_without_last_8_columns(shape):
    M, N, K = shape
    x = nh.int_mat("x", (M, K))
    W = nh.int_mat("W", (N, K))
    ref = nh.exact_mm_ref(x, W)
    bad = x.double()[:, :K - 8] @ W.double()[:, :K - 8].t()
    with pytest.raises(AssertionError, match="elements differ"):
        nh.check_equal(bad.to(BF16), ref, "gemv K-8")


@pytest.mark.parametrize("split", [2, 4, 8])
def test_teeth_splitk_loses_a_slab(split):
    T = 128 * split
    dy = nh.int_mat("dy", (256, T))      # logical A (M, K = T)
    x = nh.int_mat("x", (256, T))
    ref = nh.exact_mm_ref(dy, x)
    kper = T // split
    slabs = [dy.double()[:, s * kper:(s + 1) * kper]
             @ x.double()[:, s * kper:(s + 1) * kper].t()
             for s in range(split)]
    nh.check_equal(sum(slabs).to(BF16), ref, "sanity")
    for lost in (0, split - 1):
        bad = sum(s for i, s in enumerate(slabs) if i != lost)
        with pytest.raises(AssertionError, match="elements differ"):
            nh.check_equal(bad.to(BF16), ref, f"slab {lost} lost")


def test_teeth_precision_checker():
    """The per-element error sees what a max-norm bound does not: the
    'cancel' family's result is ~0 next to |A||B|, so a bf16-rounded
    accumulator (error ~2**-9 of the running sum) fails e <= 1 by orders of
    magnitude.  A correctly rounded result has e <= 2 (bf16 unit roundoff
    2**-8 against the 2**-9 in e)."""
    A, B = nh.mm_input("cancel", 64, 64, 2048)
    lib = (A.float() @ B.float().t()).to(BF16)
    ref, mag = nh.mm_ref_mag(A, B)
    e_lib = nh.mm_err(lib, ref, mag)
    assert e_lib <= 2.0, e_lib
    acc = torch.zeros(64, 64, dtype=BF16)
    for sl in _slots(2048):              # partial sums rounded to bf16
        acc = (acc.float() + A[:, sl].float() @ B[:, sl].float().t()).to(BF16)
    with pytest.raises(AssertionError, match="e\\(got\\)"):
        nh.mm_check(acc, lib, ref, mag, "bf16 accumulator")


# --------------------------------------------------- decode needles on CPU

def _split_kv_emulate(q, kc, vc, pos0, chunk, fault=None):
    """fp64 emulation of the split-KV kernel for B = any, Sq = 1: per-split
    online-softmax partials (m, l, acc) and an l-weighted merge, with one
    fault injected:
      drop_first   split 1 skips its first key
      dup_last     split 0 counts its last key twice (in acc and in l)
      equal_merge  the merge gives every valid split the same weight"""
    B, Hq, Sq, D = q.shape
    assert Sq == 1
    Hkv = kc.shape[1]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    out = torch.empty(B, Hkv, G, D, dtype=torch.float64)
    for b in range(B):
        L = pos0[b] + 1
        qb = q[b].double().reshape(Hkv, G, D)
        parts = []
        for si, c0 in enumerate(range(0, L, chunk)):
            keys = list(range(c0, min(c0 + chunk, L)))
            if fault == "drop_first" and si == 1:
                keys = keys[1:]
            if fault == "dup_last" and si == 0:
                keys = keys + keys[-1:]
            if not keys:
                continue
            k = kc[b][:, keys].double()
            v = vc[b][:, keys].double()
            s = qb @ k.transpose(-1, -2) * scale                # (Hkv,G,n)
            m = s.max(-1, keepdim=True).values
            p = torch.exp(s - m)
            parts.append((m, p.sum(-1, keepdim=True), p @ v))
        mx = torch.stack([m for m, _, _ in parts]).max(0).values
        if fault == "equal_merge":
            out[b] = sum(a / l for _, l, a in parts) / len(parts)
        else:
            den = sum(torch.exp(m - mx) * l for m, l, _ in parts)
            out[b] = sum(torch.exp(m - mx) * a for m, _, a in parts) / den
    return out.reshape(B, Hq, 1, D).to(BF16)


def _needle_call(D, heads, Smax, which):
    Hq, Hkv, Sq = heads
    M = Hq // Hkv * Sq
    pos0, needles = nh.needle_grid(Smax, Sq, M)[which]
    q, kb, vb, want = nh.needle_input(which, D, Hq, Hkv, Sq, Smax, pos0,
                                      needles)
    kc, vc = nh.needle_views(kb, vb, Smax)
    return q, kc, vc, pos0, want


@pytest.mark.parametrize(
    "D,heads,Smax",
    [pytest.param(D, h, S, id="D%d-Hq%d-Hkv%d-Sq%d-Smax%d" % (D, *h, S))
     for D in (64, 128) for h in [(2, 2, 1), (6, 2, 2), (8, 2, 4)]
     for S in nh.NEEDLE_SMAX if h[2] <= S])
def test_needles_cpu_path(D, heads, Smax):
    """ops.decode_attention on CPU tensors (exact fp32 math) returns every
    needle's v row bit for bit, for equal and for per-row lengths: the
    generator and its expected values are right."""
    for which in ("full", "ragged"):
        q, kc, vc, pos0, want = _needle_call(D, heads, Smax, which)
        if not pos0:
            continue
        got = ops.decode_attention(q, kc, vc, torch.tensor(pos0))
        nh.check_needles(got, want, f"cpu {which}")
        ref = nh.decode_ref64(q, kc, vc, pos0).to(BF16)
        nh.check_needles(ref, want, f"fp64 {which}")


def test_teeth_needles_dropped_first_key_of_a_chunk():
    q, kc, vc, pos0, want = _needle_call(64, (2, 2, 1), 256, "full")
    good = _split_kv_emulate(q, kc, vc, pos0, 64)
    nh.check_needles(good, want, "sanity")
    bad = _split_kv_emulate(q, kc, vc, pos0, 64, "drop_first")
    with pytest.raises(AssertionError, match="not their needle's v row"):
        nh.check_needles(bad, want, "drop_first")


def test_old_absolute_bound_accepts_a_dropped_key_at_length_256():
    """The gap this file closes: on the unit-variance inputs of
    tests/test_decode_attention_gpu.py (B=2, Hq/Hkv=8/2, D=128, length 256)
    a kernel that drops key 64 in every row stays under max|err| < 3e-2."""
    g = nh._gen("old-bound", 0)
    q = nh._randn((2, 8, 1, 128), g).to(BF16)
    kc = nh._randn((2, 2, 256, 128), g).to(BF16)
    vc = nh._randn((2, 2, 256, 128), g).to(BF16)
    pos0 = [255, 255]
    want = nh.decode_ref64(q, kc, vc, pos0)
    bad = _split_kv_emulate(q, kc, vc, pos0, 64, "drop_first")
    err = (bad.double() - want).abs().max().item()
    print(f"dropped key 64 at length 256: max abs err {err:.3e}")
    assert 1e-3 < err < 3e-2, err


@pytest.mark.parametrize("positions,why", nh.MULTI_NEEDLES,
                         ids=["-".join(map(str, p))
                              for p, _ in nh.MULTI_NEEDLES])
@pytest.mark.parametrize("D", [64, 128])
def test_multi_needles_cpu_path(D, positions, why):
    q, kb, vb, want = nh.multi_needle_input("mn", D, 256, positions, M=2)
    kc, vc = nh.needle_views(kb, vb, 256)
    nh.check_needles(ops.decode_attention(q, kc, vc, 255), want, why)
    nh.check_needles(_split_kv_emulate(q, kc, vc, [255], 64), want, why)


@pytest.mark.parametrize("G,istar", [(1, (2,)), (4, (3, 0, 2, 1))],
                         ids=["G1", "G4"])
def test_causal_needles_cpu_path(G, istar):
    """Sq = 4: rows from istar[g] on return group g's needle exactly; the
    earlier rows do not see it and stay a plain average of v in [1, 2)."""
    q, kb, vb, want, exact = nh.causal_needle_input("causal", 64, G, 4, 200,
                                                    62, istar)
    kc, vc = nh.needle_views(kb, vb, 200)
    got = ops.decode_attention(q, kc, vc, 62)
    nh.check_needles(got[exact], want[exact], "rows that see the needle")
    ref = nh.decode_ref64(q, kc, vc, [62])
    nh.yardstick(got[~exact], ref[~exact], ref[~exact].to(BF16),
                 nh.FLOOR_BF16_FWD, what="earlier rows")


def test_teeth_double_counted_last_key_of_a_chunk():
    """A key counted twice in acc AND l renormalises away when it is the
    only needle (the single-needle checker is blind to it by construction,
    asserted here); with a second needle elsewhere the weights become 2:1
    and the two-needle checker rejects it."""
    q, kc, vc, pos0, want = _needle_call(64, (2, 2, 1), 256, "full")
    bad = _split_kv_emulate(q, kc, vc, pos0, 64, "dup_last")
    nh.check_needles(bad, want, "single needle cannot see a renormalised dup")
    for positions in ((63, 64), (63, 100)):
        q, kb, vb, want = nh.multi_needle_input("mn", 64, 256, positions)
        kc, vc = nh.needle_views(kb, vb, 256)
        bad = _split_kv_emulate(q, kc, vc, [255], 64, "dup_last")
        with pytest.raises(AssertionError, match="not their needle's v row"):
            nh.check_needles(bad, want, "dup_last")


def test_teeth_merge_with_equal_weights():
    for positions in ((63, 100), (3, 12, 20, 100)):
        q, kb, vb, want = nh.multi_needle_input("mn", 64, 256, positions)
        kc, vc = nh.needle_views(kb, vb, 256)
        bad = _split_kv_emulate(q, kc, vc, [255], 64, "equal_merge")
        with pytest.raises(AssertionError, match="not their needle's v row"):
            nh.check_needles(bad, want, "equal_merge")
    # exactly two splits, three needles against one: only the l weights
    # separate right from wrong
    q, kb, vb, want = nh.multi_needle_input("mn2", 64, 128, (3, 12, 20, 100))
    kc, vc = nh.needle_views(kb, vb, 128)
    nh.check_needles(_split_kv_emulate(q, kc, vc, [127], 64), want, "sanity")
    bad = _split_kv_emulate(q, kc, vc, [127], 64, "equal_merge")
    with pytest.raises(AssertionError, match="not their needle's v row"):
        nh.check_needles(bad, want, "equal_merge, two splits")


# -------------------------------------------------------------------- RoPE

@pytest.mark.parametrize("layout", ["contiguous", "permuted"])
@pytest.mark.parametrize("pos0", [0, 8])
@pytest.mark.parametrize("D", nh.ROPE_DIMS)
@pytest.mark.parametrize("family", nh.ROPE_FAMILIES)
def test_rope_cpu_path(family, D, pos0, layout):
    x, dy, cos, sin, view = nh.rope_case(family, D, layout)
    what = f"rope cpu[{family} D{D} pos{pos0} {layout}]"
    nh.check_fwd_bwd(
        lambda t: ops.rope_rotate_half(view(t), cos, sin, pos0),
        lambda t: nh.rope_lib(view(t), cos, sin, pos0),
        lambda t: nh.rope_formula(view(t), cos.double(), sin.double(), pos0),
        (x,), dy, "x", BF16, CPU, BF16, what)
    if pos0 == 0:       # cos = 1, sin = 0: position 0 is the identity
        y = ops.rope_rotate_half(view(x), cos, sin, 0)
        nh.check_equal(y[:, :, 0], view(x)[:, :, 0], what + " row 0")


def test_teeth_rope_rounded_tables_and_products():
    """The CPU fallback once rounded the tables and every product to bf16;
    that formula misses the yardstick the fp32 one passes."""
    # unit-vector pairs: every output is below 1, where bf16's half ulp is
    # smallest relative to max|ref| and the extra roundings show
    x, _ = nh.rope_input("rotation", (4, 8, 64, 128))
    cos, sin = nh.rope_tables(64 + 8, 128)
    ref = nh.rope_formula(x.double(), cos.double(), sin.double(), 8)
    lib = nh.rope_lib(x, cos, sin, 8)
    nh.yardstick(ops.rope_rotate_half(x, cos, sin, 8), ref, lib,
                 nh.FLOOR_BF16_FWD, what="rope fp32 path")
    with pytest.raises(AssertionError, match="e\\(got\\)"):
        nh.yardstick(nh.rope_all_bf16(x, cos, sin, 8), ref, lib,
                     nh.FLOOR_BF16_FWD, what="rope all-bf16 formula")


def test_rope_cpu_rejects_bad_tables():
    x, _, cos, sin, _ = nh.rope_case("randn", 64, "contiguous")
    with pytest.raises(ValueError, match="outside the cos/sin table"):
        ops.rope_rotate_half(x, cos, sin, 9)
    with pytest.raises(ValueError, match="outside the cos/sin table"):
        ops.rope_rotate_half(x, cos, sin, -1)
    with pytest.raises(ValueError, match="shape of cos"):
        ops.rope_rotate_half(x, cos, sin[:-1], 0)
