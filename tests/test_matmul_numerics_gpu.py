"""The matmul-shaped HIP kernels (csrc/gemm.hip, gemv.hip, decode_attn.hip
and the RoPE half of rope_swiglu.hip) against fp64:

- exact family: small-integer operands make fp32 accumulation exact in any
  order, so every result must equal the fp64 product rounded once, bit for
  bit, through every ring depth, tile grid, split-K factor and GEMV arm
- locality family: one NaN taints exactly its row / column; a 0/1 selection
  matrix returns the selected rows exactly
- precision family: per-element error (cancellation included) against
  hipBLASLt's own
- decode needles: one key dominates by > 40 bits, so the output row is that
  key's v row bit for bit, at every key position, length, split and row count
- RoPE: fp64 yardstick forward and backward, argument checks, position clamp

Generators, references and checkers live in tests/numerics_helpers.py, the
CPU twin with the teeth in tests/test_matmul_numerics.py, the table and the
measured errors in docs/design/kernels.md ("Matmul-family numerics").

Run on MI355X via: pytest tests/test_matmul_numerics_gpu.py -m gpu -q
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.ops import gemm
from tests import numerics_helpers as nh

BF16 = torch.bfloat16


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"


# ------------------------------------------------------------ exact family

@functools.lru_cache(maxsize=4)
def _exact_case(M, N, K):
    """Logical integer A (M,K), B (N,K), bias (N,) and the exact results
    without / with bias; shared by the cases that differ only in split-K
    factor or swizzle."""
    A = nh.int_mat("A", (M, K))
    B = nh.int_mat("B", (N, K))
    bias = nh.int_mat("bias", (N,))
    return A, B, bias, nh.exact_mm_ref(A, B), nh.exact_mm_ref(A, B, bias)


def _run_gemm(kind, A, B, bias=None, splitk=1, kswz=False):
    a, b = (t.to(_dev()) for t in nh.gemm_operands(kind, A, B))
    e = ops.ext("gemm")
    if kind == "fprop":
        return e.gemm_fprop(a, b, None if bias is None else bias.to(_dev()))
    if kind == "dgrad":
        return e.gemm_dgrad(a, b, kswz)
    return e.gemm_wgrad(a, b, splitk, kswz)


@pytest.mark.parametrize("K", nh.GEMM_KS, ids=nh.gemm_k_id)
@pytest.mark.parametrize("grid", nh.GEMM_GRIDS_FPROP,
                         ids=lambda g: nh.gemm_grid_id(*g))
def test_exact_gemm_fprop(grid, K):
    M, N = 256 * grid[0], 256 * grid[1]
    A, B, bias, ref, ref_b = _exact_case(M, N, K)
    what = f"gemm_fprop {M}x{N}x{K}"
    nh.check_equal(_run_gemm("fprop", A, B), ref, what)
    nh.check_equal(_run_gemm("fprop", A, B, bias), ref_b, what + " +bias")
    # the library on the same values: must reproduce the reference as well
    lib = F.linear(A.to(_dev()), B.to(_dev()), bias.to(_dev()))
    nh.check_equal(lib, ref_b, what + " F.linear (sanity)")


@pytest.mark.parametrize("K", nh.GEMM_KS, ids=nh.gemm_k_id)
@pytest.mark.parametrize("grid", nh.GEMM_GRIDS_DGRAD,
                         ids=lambda g: nh.gemm_grid_id(*g))
def test_exact_gemm_dgrad(grid, K):
    M, N = 256 * grid[0], 256 * grid[1]
    A, B, _, ref, _ = _exact_case(M, N, K)
    for kswz in (False, True):
        nh.check_equal(_run_gemm("dgrad", A, B, kswz=kswz), ref,
                       f"gemm_dgrad {M}x{N}x{K} kswz={kswz}")


def _wgrad_cases():
    for grid in nh.GEMM_GRIDS_WGRAD:
        for split in (1, 2, 4, 8):
            Ts = [(32 * split, "one_slot_per_slice"), (128 * split, ""),
                  (4096, "")]
            if split == 8 and grid == (1, 1):
                Ts.append((16384, "deep_K_policy_shape"))
            for T, note in Ts:
                yield pytest.param(
                    grid, split, T,
                    id=f"{nh.gemm_grid_id(*grid, split)}-split{split}-T{T}"
                       + (f"-{note}" if note else ""))


@pytest.mark.parametrize("grid,split,T", list(_wgrad_cases()))
def test_exact_gemm_wgrad(grid, split, T):
    M, N = 256 * grid[0], 256 * grid[1]
    A, B, _, ref, _ = _exact_case(M, N, T)
    for kswz in (False, True):
        nh.check_equal(_run_gemm("wgrad", A, B, splitk=split, kswz=kswz),
                       ref, f"gemm_wgrad {M}x{N} T={T} split={split} "
                            f"kswz={kswz}")


@pytest.mark.parametrize("shape", nh.GEMV_SHAPES, ids=nh.gemv_id)
def test_exact_gemv(shape):
    M, N, K = shape
    A, B, bias, ref, ref_b = _exact_case(M, N, K)
    x, W, b = (t.to(_dev()) for t in (A, B, bias))
    e = ops.ext("gemv")
    nh.check_equal(e.gemv_bf16(x, W, None), ref, f"gemv {shape}")
    nh.check_equal(e.gemv_bf16(x, W, b), ref_b, f"gemv {shape} +bias")
    nh.check_equal(F.linear(x, W, b), ref_b, f"F.linear {shape} (sanity)")


# ------------------------------------------- gemm.linear() end to end, exact

MODES = ["1", "all", "0"]


def _linear_fwd_bwd(x, w, b, dy, fn=gemm.linear, ref_fn=F.linear):
    y, grads = nh.fwd_bwd(fn, (x, w, b), dy, BF16, _dev())
    y_ref, g_ref = nh.fwd_bwd(ref_fn, (x, w, b), dy, torch.float64, "cpu")
    return [("y", y, y_ref)] + \
        [(n, g, gr) for n, g, gr in zip(("dx", "dw", "db"), grads, g_ref)]


@pytest.mark.parametrize("M", [1, 4, 8, 9])
@pytest.mark.parametrize("mode", MODES)
def test_exact_linear_decode_arm(mode, M, monkeypatch):
    """no_grad, M = 1 / 4 / 8: the in-tree GEMV (modes "1" and "all");
    M = 9 and mode "0": the library."""
    monkeypatch.setattr(gemm, "_MODE", mode)
    K, N = 1032, 1000
    assert gemm._GEMV
    assert gemm._use_gemv(M, N, K) == (M <= 8)     # the arm this case takes
    A, B, bias, ref, ref_b = _exact_case(M, N, K)
    x, W, b = (t.to(_dev()) for t in (A, B, bias))
    with torch.no_grad():
        nh.check_equal(gemm.linear(x, W, b), ref_b, f"linear M={M} +bias")
        nh.check_equal(gemm.linear(x, W), ref, f"linear M={M}")
        if M % 2 == 0:      # 3-D input
            y = gemm.linear(x.view(2, M // 2, K), W, b)
            nh.check_equal(y, ref_b.view(2, M // 2, N), f"linear 3-D M={M}")


@pytest.mark.parametrize("mode", MODES)
def test_exact_linear_fwd_bwd_deep_wgrad(mode, monkeypatch):
    """(tokens 4096, in 256, out 256): in the default mode "1" this is the
    shape class whose wgrad goes to the in-tree kernel with split-K 8."""
    monkeypatch.setattr(gemm, "_MODE", mode)
    T, K, N = 4096, 256, 256
    # the route, asserted so a policy change cannot silently empty the test
    assert gemm.pick_splitk(N, K, T) == 8
    assert gemm._eligible(T, N, K)
    assert gemm._use_mine("wgrad", N, K, T) == (mode in ("1", "all"))
    assert gemm._use_mine("dgrad", T, K, N) == (mode == "all")
    assert gemm._use_mine("fprop", T, N, K) == (mode == "all")
    x = nh.int_mat("x", (T, K))
    w = nh.int_mat("w", (N, K))
    b = nh.int_mat("b", (N,))
    dy = nh.int_mat("dy", (T, N), -2, 2)       # |db| <= 8192: exact
    for n, g, r in _linear_fwd_bwd(x, w, b, dy):
        nh.check_equal(g, r.to(BF16), f"linear mode={mode} {n}")


def test_exact_linear_fwd_bwd_all_512(monkeypatch):
    monkeypatch.setattr(gemm, "_MODE", "all")
    for kind, a in (("fprop", (512, 512, 512)), ("dgrad", (512, 512, 512)),
                    ("wgrad", (512, 512, 512))):
        assert gemm._use_mine(kind, *a)
    x = nh.int_mat("x", (512, 512))
    w = nh.int_mat("w", (512, 512))
    b = nh.int_mat("b", (512,))
    dy = nh.int_mat("dy", (512, 512), -2, 2)
    for n, g, r in _linear_fwd_bwd(x, w, b, dy):
        nh.check_equal(g, r.to(BF16), f"linear all 512^3 {n}")


@pytest.mark.parametrize("mode", MODES)
def test_exact_linear_3d_input_noncontiguous_weight(mode, monkeypatch):
    monkeypatch.setattr(gemm, "_MODE", mode)
    x = nh.int_mat("x", (2, 2048, 256))
    wt = nh.int_mat("wt", (256, 512))          # weight is wt.t(): (512, 256)
    b = nh.int_mat("b", (512,))
    dy = nh.int_mat("dy", (2, 2048, 512), -2, 2)
    assert gemm._use_mine("wgrad", 512, 256, 4096) == (mode != "0")

    def fn(x, wt, b):
        assert not wt.t().is_contiguous()
        return gemm.linear(x, wt.t(), b)

    for n, g, r in _linear_fwd_bwd(
            x, wt, b, dy, fn, lambda x, wt, b: F.linear(x, wt.t(), b)):
        nh.check_equal(g, r.to(BF16), f"linear 3-D mode={mode} {n}")


# --------------------------------------------------------- locality family

# (kind, M, N, K, splitk): K = 160 and 96 end on clamped tail slots
LOCALITY = [("fprop", 512, 256, 160, 1), ("dgrad", 256, 512, 96, 1),
            ("wgrad", 512, 256, 256, 2), ("gemv", 5, 9, 2056, 1)]


def _run_any(kind, A, B, splitk):
    if kind == "gemv":
        return ops.ext("gemv").gemv_bf16(A.to(_dev()), B.to(_dev()), None)
    return _run_gemm(kind, A, B, splitk=splitk, kswz=(kind != "fprop"))


@pytest.mark.parametrize("where", ["A_row", "B_row"])
@pytest.mark.parametrize("kind,M,N,K,splitk", LOCALITY,
                         ids=[c[0] for c in LOCALITY])
def test_nan_stays_in_its_row_or_column(kind, M, N, K, splitk, where):
    """One NaN in row r of A (row c of B): output row r (column c) is
    non-finite everywhere and every other element is the exact result.  A
    kernel that reads a neighbour's row, or lets a clamped tail slot reach
    an accumulator, spreads it."""
    A, B, _, ref, _ = _exact_case(M, N, K)
    A, B = A.clone(), B.clone()
    r, c = (M * 2) // 3, N // 3
    if where == "A_row":
        A[r, K - 1] = float("nan")
        tainted = torch.zeros(M, N, dtype=torch.bool)
        tainted[r] = True
    else:
        B[c, 0] = float("nan")
        tainted = torch.zeros(M, N, dtype=torch.bool)
        tainted[:, c] = True
    got = _run_any(kind, A, B, splitk).cpu()
    what = f"{kind} NaN in {where}"
    assert not torch.isfinite(got[tainted]).any(), \
        f"{what}: a tainted element is finite"
    clean = torch.where(tainted, torch.zeros_like(got), got)
    nh.check_equal(clean, torch.where(tainted, torch.zeros_like(ref), ref),
                   what + " (elements outside the tainted line)")


SELECTION = [("fprop", 256, 256, 512), ("dgrad", 256, 256, 288),
             ("wgrad", 256, 512, 1024), ("gemv", 8, 9, 2056)]


@pytest.mark.parametrize("kind,M,N,K", SELECTION,
                         ids=[c[0] for c in SELECTION])
def test_selection_matrix_returns_rows_of_b(kind, M, N, K):
    A, idx = nh.selection_matrix(kind, M, K)
    _, B = nh.mm_input("randn", 8, N, K)
    got = _run_any(kind, A, B, 2 if kind == "wgrad" else 1)
    nh.check_equal(got, B.t()[idx].contiguous(), f"{kind} selection")


# -------------------------------------------------------- precision family

@functools.lru_cache(maxsize=2)
def _mm_case(family, M, N, K):
    A, B = nh.mm_input(family, M, N, K)
    ref, mag = nh.mm_ref_mag(A, B)
    lib = A.to(_dev()) @ B.to(_dev()).t()          # hipBLASLt, bf16
    return A, B, ref, mag, lib


# the deep-K policy class at its smallest size
PRECISION = [("wgrad", 256, 256, 16384, 1), ("wgrad", 256, 256, 16384, 4),
             ("wgrad", 256, 256, 16384, 8), ("fprop", 256, 256, 2048, 1),
             ("dgrad", 256, 256, 2048, 1),
             ("gemv", 4, 1000, 4104, 1), ("gemv", 32, 9, 1032, 1)]


@pytest.mark.parametrize(
    "kind,M,N,K,splitk", PRECISION,
    ids=[f"{k}-{M}x{N}x{K}-split{s}" for k, M, N, K, s in PRECISION])
@pytest.mark.parametrize("family", nh.MM_FAMILIES)
def test_precision_vs_hipblaslt(kind, M, N, K, splitk, family):
    A, B, ref, mag, lib = _mm_case(family, M, N, K)
    got = _run_any(kind, A, B, splitk)
    nh.mm_check(got, lib, ref, mag,
                f"{kind}[{family} {M}x{N}x{K} split={splitk}]")


# ------------------------------------------------ decode-attention needles

def _to_dev_views(kb, vb, Smax):
    kc, vc = nh.needle_views(kb.to(_dev()), vb.to(_dev()), Smax)
    return kc, vc


def _needle_run(D, heads, Smax, which, splits):
    Hq, Hkv, Sq = heads
    M = Hq // Hkv * Sq
    pos0, needles = nh.needle_grid(Smax, Sq, M)[which]
    if not pos0:
        return
    q, kb, vb, want = nh.needle_input(which, D, Hq, Hkv, Sq, Smax, pos0,
                                      needles)
    kc, vc = _to_dev_views(kb, vb, Smax)
    qd = q.to(_dev())
    # equal lengths go in as a host int, differing ones as a per-row tensor
    p = pos0[0] if which == "full" else torch.tensor(pos0, device=_dev())
    for skv in splits:
        got = ops.decode_attention(qd, kc, vc, p, split_kv=skv)
        nh.check_needles(got, want,
                         f"decode D{D} heads{heads} Smax{Smax} {which} "
                         f"split_kv={skv}")


@pytest.mark.parametrize(
    "D,heads,Smax",
    [pytest.param(D, h, S,
                  id="D%d-Hq%d-Hkv%d-Sq%d-M%d-Smax%d" % (D, *h,
                                                         h[0] // h[1] * h[2],
                                                         S))
     for D in (64, 128) for h in nh.NEEDLE_HEADS
     for S in nh.NEEDLE_SMAX if h[2] <= S])
def test_decode_needles(D, heads, Smax):
    """Every probed key position of the cache, and every probed length with
    the needle on its last key; split_kv 64 (a split per chunk), 100 (rounded
    up to 128), None (auto) and Smax (one split, no combine launch).
    Smax = 40 is shorter than a chunk, 72 and 200 end in a partial chunk."""
    splits = (64, 100, None, Smax)
    _needle_run(D, heads, Smax, "full", splits)
    _needle_run(D, heads, Smax, "ragged", splits)


@pytest.mark.parametrize("heads", [(1, 1, 1), (4, 1, 1), (2, 1, 2)],
                         ids=lambda h: "Hq%d-Hkv%d-Sq%d" % h)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_needles_65_splits(D, heads):
    """Smax = 4160 with split_kv = 64 at B * Hkv = 1 per row: 65 valid
    splits, i.e. eight full trips of the combine kernel's 8-way unrolled
    loop plus a remainder of one.  Needles on the first / last key of the
    first, a middle and the last (65th) split."""
    Hq, Hkv, Sq = heads
    Smax = 4160
    last = Smax - Sq
    for n in (0, 63, 64, 2047, 2048, 4095, 4096, last):
        M = Hq * Sq
        others = [(n + 97 * (p + 1)) % (last + 1) for p in range(M - 1)]
        q, kb, vb, want = nh.needle_input("65", D, Hq, Hkv, Sq, Smax, [last],
                                          [[n] + others])
        kc, vc = _to_dev_views(kb, vb, Smax)
        for skv in (64, None):
            got = ops.decode_attention(q.to(_dev()), kc, vc, last,
                                       split_kv=skv)
            nh.check_needles(got, want, f"decode 4160 needle {n} "
                                        f"split_kv={skv}")


def _sdpa_lib(q, kc, vc, pos0):
    """bf16 SDPA over the visible cache with the causal-offset mask: the
    library value for the yardstick.  B = 1 or equal lengths."""
    B, Hq, Sq, D = q.shape
    L = pos0 + Sq
    rep = Hq // kc.shape[1]
    k = kc[:, :, :L].repeat_interleave(rep, 1)
    v = vc[:, :, :L].repeat_interleave(rep, 1)
    j = torch.arange(L, device=q.device)
    mask = j[None, :] <= (pos0 + torch.arange(Sq, device=q.device))[:, None]
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask)


@pytest.mark.parametrize("G,istar",
                         [(1, (2,)), (2, (1, 3)), (4, (3, 0, 2, 1))],
                         ids=["G1", "G2", "G4"])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_causal_rows(D, G, istar):
    """Sq = 4 at pos0 = 62: the rows' last visible keys 62..65 straddle the
    chunk edge.  Group g's needle is the key at pos0 + istar[g]: rows from
    istar[g] on return its v row exactly, earlier rows must not see it and
    are held to the fp64 oracle."""
    Sq, Smax, pos0 = 4, 200, 62
    q, kb, vb, want, exact = nh.causal_needle_input("causal", D, G, Sq, Smax,
                                                    pos0, istar)
    kc, vc = _to_dev_views(kb, vb, Smax)
    qd = q.to(_dev())
    k_cpu, v_cpu = nh.needle_views(kb, vb, Smax)
    ref = nh.decode_ref64(q, k_cpu, v_cpu, [pos0])
    lib = _sdpa_lib(qd, kc, vc, pos0)
    for skv in (64, None, Smax):
        got = ops.decode_attention(qd, kc, vc, pos0, split_kv=skv).cpu()
        what = f"decode causal D{D} G{G} split_kv={skv}"
        nh.check_needles(got[exact], want[exact], what + " rows that see it")
        nh.yardstick(got[~exact], ref[~exact], lib.cpu()[~exact],
                     nh.FLOOR_BF16_FWD, what=what + " earlier rows")


@pytest.mark.parametrize("positions,why", nh.MULTI_NEEDLES,
                         ids=["-".join(map(str, p))
                              for p, _ in nh.MULTI_NEEDLES])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_equal_needles_mean(D, positions, why):
    """Equal needles share the weight equally: the output is the exact mean
    of their v rows.  Pins the merge weights of the wave merge, the block
    merge and the combine kernel."""
    for M in (1, 2, 8):
        q, kb, vb, want = nh.multi_needle_input("mn", D, 256, positions, M=M)
        kc, vc = _to_dev_views(kb, vb, 256)
        for skv in (64, None, 256):
            got = ops.decode_attention(q.to(_dev()), kc, vc, 255,
                                       split_kv=skv)
            nh.check_needles(got, want, f"{why} D{D} M{M} split_kv={skv}")


@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("shape", [(1, 2, 2, 192, 64), (1, 4, 2, 192, 128)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", ["dominant_key", "uniform", "peaky"])
def test_decode_hard_inputs(family, shape, Sq):
    """attn_input's dominant key, identical keys and large scores through
    the decode kernel, against fp64 with bf16 SDPA as the yardstick."""
    B, H, Hkv, S, D = shape
    q, k, v, _ = nh.attn_input(family, *shape)
    q = q[:, :, S - Sq:].contiguous()
    pos0 = S - Sq
    ref = nh.decode_ref64(q, k, v, [pos0] * B)
    qd, kd, vd = (t.to(_dev()) for t in (q, k, v))
    lib = _sdpa_lib(qd, kd, vd, pos0)
    for skv in (64, None):
        got = ops.decode_attention(qd, kd, vd, pos0, split_kv=skv)
        nh.yardstick(got, ref, lib, nh.FLOOR_BF16_FWD,
                     what=f"decode[{family} {shape} Sq={Sq} split_kv={skv}]")


# -------------------------------------------------------------------- RoPE

def _tables_dev(cos, sin):
    return cos.to(_dev()), sin.to(_dev())


@pytest.mark.parametrize("layout", ["contiguous", "permuted"])
@pytest.mark.parametrize("pos0", [0, 8])
@pytest.mark.parametrize("D", nh.ROPE_DIMS)
@pytest.mark.parametrize("family", nh.ROPE_FAMILIES)
def test_rope(family, D, pos0, layout):
    x, dy, cos, sin, view = nh.rope_case(family, D, layout)
    cd, sd = _tables_dev(cos, sin)
    what = f"rope[{family} D{D} pos{pos0} {layout}]"
    nh.check_fwd_bwd(
        lambda t: ops.rope_rotate_half(view(t), cd, sd, pos0),
        lambda t: nh.rope_lib(view(t), cd, sd, pos0),
        lambda t: nh.rope_formula(view(t), cos.double(), sin.double(), pos0),
        (x,), dy, "x", BF16, _dev(), BF16, what)
    xd = view(x.to(_dev()))
    assert xd.is_contiguous() == (layout == "contiguous")
    with torch.no_grad():
        host = ops.rope_rotate_half(xd, cd, sd, pos0)
        devp = ops.rope_rotate_half(xd, cd, sd,
                                    torch.tensor([pos0], device=_dev()))
    # device-position variant: the same bits as the host-position one
    nh.check_equal(devp, host, what + " device pos vs host pos")
    if pos0 == 0:       # cos = 1, sin = 0: position 0 is the identity
        nh.check_equal(host[:, :, 0], xd[:, :, 0], what + " row 0")


def test_rope_many_blocks_permuted():
    """More than one block and rows that straddle blocks, Llama layout."""
    x, dy, cos, sin, view = nh.rope_case("randn", 128, "permuted",
                                         B=2, H=5, S=67)
    cd, sd = _tables_dev(cos, sin)
    nh.check_fwd_bwd(
        lambda t: ops.rope_rotate_half(view(t), cd, sd, 8),
        lambda t: nh.rope_lib(view(t), cd, sd, 8),
        lambda t: nh.rope_formula(view(t), cos.double(), sin.double(), 8),
        (x,), dy, "x", BF16, _dev(), BF16, "rope[randn 2x5x67x128 permuted]")


def test_rope_rejects_bad_arguments():
    """Every rejection happens before a launch."""
    B, H, S, D = 2, 3, 5, 64
    x = torch.zeros(B, H, S, D, dtype=BF16, device=_dev())
    cos, sin = nh.rope_tables(S + 8, D)
    cd, sd = _tables_dev(cos, sin)
    e = ops.ext("rope")
    pos = torch.tensor([0], device=_dev())
    for call in (lambda *a: e.rope_apply(*a, 0, True),
                 lambda *a: e.rope_apply_pos(*a, pos, True)):
        with pytest.raises(RuntimeError, match="on x's device"):
            call(x, cos, sd)
        with pytest.raises(RuntimeError, match="on x's device"):
            call(x, cd, sin)
        with pytest.raises(RuntimeError, match="shape of cos"):
            call(x, cd, sd[:-1])
        # x strides that break the 16-byte loads: rows 68 elements apart
        xs = torch.zeros(B, H, S, D + 4, dtype=BF16,
                         device=_dev())[..., :D]
        assert xs.stride(3) == 1 and xs.stride(2) % 8 != 0
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(xs, cd, sd)
        # base pointer 8 bytes into an allocation
        xo = torch.zeros(B * H * S * D + 4, dtype=BF16,
                         device=_dev())[4:].view(B, H, S, D)
        assert xo.data_ptr() % 16 == 8
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(xo, cd, sd)
    with pytest.raises(RuntimeError, match="outside the cos/sin table"):
        e.rope_apply(x, cd, sd, -1, True)
    with pytest.raises(RuntimeError, match="outside the cos/sin table"):
        e.rope_apply(x, cd, sd, 9, True)
    with pytest.raises(RuntimeError, match="exceeds the cos/sin table"):
        e.rope_apply_pos(x, cd[:S - 1], sd[:S - 1], pos, True)
    with pytest.raises(RuntimeError, match="outside the cos/sin table"):
        ops.rope_rotate_half(x, cd, sd, 9)


@pytest.mark.parametrize("D", [16, 128])
def test_rope_device_position_is_clamped(D):
    """The tables are narrowed views of a larger allocation whose margins
    are NaN, so every read stays in owned memory whatever the kernel does.
    At the valid edge rows - S the device position gives the host result;
    beyond either end it is clamped to the edge (no NaN from the margins)."""
    B, H, S, rows, margin = 2, 3, 5, 13, 8
    x, _ = nh.rope_input("randn", (B, H, S, D))
    xd = x.to(_dev())
    cos, sin = nh.rope_tables(rows, D)

    def margined(t):
        big = torch.full((rows + 2 * margin, D // 2), float("nan"),
                         device=_dev())
        big[margin:margin + rows] = t.to(_dev())
        return big.narrow(0, margin, rows)

    cd, sd = margined(cos), margined(sin)
    with torch.no_grad():
        first = ops.rope_rotate_half(xd, cd, sd, 0)
        edge = ops.rope_rotate_half(xd, cd, sd, rows - S)
        for p, want in ((rows - S, edge), (rows - S + 3, edge), (-3, first)):
            got = ops.rope_rotate_half(xd, cd, sd,
                                       torch.tensor([p], device=_dev()))
            nh.check_equal(got, want, f"rope device pos {p}")
    ref = nh.rope_formula(x.double(), cos.double(), sin.double(), rows - S)
    nh.yardstick(edge, ref, nh.rope_lib(x, cos, sin, rows - S),
                 nh.FLOOR_BF16_FWD, what=f"rope D{D} at the table edge")
