"""The grouped expert GEMM (csrc/grouped_gemm.hip) and ops.grouped_linear on
the GPU:

- exact family: integer operands in [-4, 4] make fp32 accumulation exact in
  any order, so y, dx, dw and db must equal the per-segment fp64 product
  rounded once, bit for bit, through aligned, ragged, one-row and empty
  segments, short and long wgrad reductions, int32 and int64 offsets
- locality family: one NaN row at a segment edge taints exactly its own row
  of y / dx and exactly its own expert's dw / db (clamped loads, masked
  stores, zero-sourced reduction tail)
- precision family: normal inputs against fp64, the per-expert torch.mm loop
  as the library yardstick
- plan: the host run of the block -> tile mapping covers every row once,
  never leaves its expert, and fits the launch bound
- capture: a hipGraph of the forward follows new contents of offs
- autograd: ops.grouped_linear against its CPU path in fp64

The kernel tests call the extension bindings directly and assert
grouped_gemm_eligible, so none of them can pass through the fallback loop.

Run on MI355X via: pytest tests/test_grouped_gemm_gpu.py -m gpu -q
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

BF16 = torch.bfloat16
BM = ops.GROUPED_GEMM_BM
E = 4
SHAPES = [(256, 256), (512, 256), (256, 512)]      # (Dout, Din)

SEGMENTS = {
    "aligned": [BM, BM, BM, BM],
    "one_row-empty-tile_plus_1-sub_slot": [1, 0, BM + 1, 31],
    "all_in_last": [0, 0, 0, 2 * BM + 3],
    "all_in_first": [2 * BM + 3, 0, 0, 0],
    "ragged_both_sides": [33, BM - 1, BM + 1, 64],
    # wgrad nslot = 1, 3, 4, 8: ring never fills (twice), empty main loop,
    # first main-loop group with a 5-row tail in the last slot
    "wgrad_ring_depths": [32, 96, 128, 229],
    "T0": [0, 0, 0, 0],
}


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"
        assert ops.ext().GROUPED_GEMM_BM == BM


def _offs(lengths, dtype=torch.int64, device="cpu"):
    o = [0]
    for c in lengths:
        o.append(o[-1] + c)
    return torch.tensor(o, dtype=dtype, device=device)


def _segs(lengths):
    o = _offs(lengths).tolist()
    return [slice(o[e], o[e + 1]) for e in range(len(lengths))]


def _exact_refs(x, dy, w, bias, lengths):
    """Per-segment fp64 products rounded once: (y, dx, dw, db)."""
    T = x.shape[0]
    Eq, Dout, Din = w.shape
    y = torch.empty(T, Dout, dtype=BF16)
    dx = torch.empty(T, Din, dtype=BF16)
    dw = torch.empty(Eq, Dout, Din, dtype=BF16)
    db = torch.empty(Eq, Dout, dtype=BF16)
    for e, s in enumerate(_segs(lengths)):
        y[s] = nh.exact_mm_ref(x[s], w[e], bias[e])
        dx[s] = nh.exact_mm_ref(dy[s], w[e].t())
        dw[e] = nh.exact_mm_ref(dy[s].t(), x[s].t())
        db[e] = dy[s].double().sum(0).to(BF16)
    return y, dx, dw, db


@functools.lru_cache(maxsize=None)
def _exact_case(name, Dout, Din):
    lengths = SEGMENTS[name]
    T = sum(lengths)
    x = nh.int_mat("gx", (T, Din))
    dy = nh.int_mat("gdy", (T, Dout))
    w = nh.int_mat("gw", (E, Dout, Din))
    bias = nh.int_mat("gb", (E, Dout))
    return x, dy, w, bias, _exact_refs(x, dy, w, bias, lengths)


def _run_kernels(x, dy, w, bias, offs):
    """The four results straight from the bindings."""
    e = ops.ext("grouped_gemm")
    xd, dyd, wd, bd, od = (t.to(_dev()) for t in (x, dy, w, bias, offs))
    y = e.grouped_gemm_fprop(xd, wd, od, bd)
    dx = e.grouped_gemm_dgrad(dyd, wd, od)
    dw, db = e.grouped_gemm_wgrad(dyd, xd, od, True)
    torch.cuda.synchronize()
    return y, dx, dw, db


# ------------------------------------------------------------ exact family

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"out{s[0]}-in{s[1]}")
@pytest.mark.parametrize("name", list(SEGMENTS))
def test_exact_grouped_gemm(name, shape):
    Dout, Din = shape
    assert ops.grouped_gemm_eligible(Dout, Din, BF16)
    x, dy, w, bias, refs = _exact_case(name, Dout, Din)
    lengths = SEGMENTS[name]
    for odt in (torch.int64, torch.int32):
        got = _run_kernels(x, dy, w, bias, _offs(lengths, odt))
        for n, g, r in zip(("y", "dx", "dw", "db"), got, refs):
            nh.check_equal(g, r, f"grouped {n} {name} {shape} offs={odt}")


def test_exact_no_bias_and_no_bias_grad():
    Dout, Din = 256, 256
    name = "ragged_both_sides"
    x, dy, w, bias, refs = _exact_case(name, Dout, Din)
    lengths = SEGMENTS[name]
    e = ops.ext("grouped_gemm")
    xd, dyd, wd, od = (t.to(_dev()) for t in (x, dy, w, _offs(lengths)))
    y = e.grouped_gemm_fprop(xd, wd, od, None)
    ref = torch.cat([nh.exact_mm_ref(x[s], w[i])
                     for i, s in enumerate(_segs(lengths))])
    nh.check_equal(y, ref, "grouped y without bias")
    dw, db = e.grouped_gemm_wgrad(dyd, xd, od, False)
    assert db is None
    nh.check_equal(dw, refs[2], "grouped dw without db")


@pytest.mark.parametrize("table,segs", [
    # offsets outside [0, T] are clamped into it
    ([-7, 40, 40, 290, 10 ** 9], [(0, 40), (0, 0), (40, 290), (290, 300)]),
    # offs[1] < offs[0]: expert 0 is empty (rows 0..39 belong to nobody)
    ([50, 40, 60, 290, 300], [(0, 0), (40, 60), (60, 290), (290, 300)]),
], ids=["out_of_range", "descending_pair"])
def test_offsets_are_clamped(table, segs):
    Dout = Din = 256
    T = 300
    x = nh.int_mat("cx", (T, Din))
    w = nh.int_mat("cw", (E, Dout, Din))
    bias = nh.int_mat("cb", (E, Dout))
    dy = nh.int_mat("cdy", (T, Dout))
    offs = torch.tensor(table, dtype=torch.int64)
    y, dx, dw, db = (t.cpu() for t in _run_kernels(x, dy, w, bias, offs))
    for i, (lo, hi) in enumerate(segs):
        s = slice(lo, hi)
        nh.check_equal(y[s], nh.exact_mm_ref(x[s], w[i], bias[i]),
                       f"clamped y expert {i}")
        nh.check_equal(dx[s], nh.exact_mm_ref(dy[s], w[i].t()),
                       f"clamped dx expert {i}")
        nh.check_equal(dw[i], nh.exact_mm_ref(dy[s].t(), x[s].t()),
                       f"clamped dw expert {i}")
        nh.check_equal(db[i], dy[s].double().sum(0).to(BF16),
                       f"clamped db expert {i}")


# --------------------------------------------------------- locality family

LOC_LENGTHS = [33, BM - 1, BM + 1, 64]


@pytest.mark.parametrize("shape", [(256, 256), (512, 256)],
                         ids=lambda s: f"out{s[0]}-in{s[1]}")
@pytest.mark.parametrize("where", ["last_row_of_e", "first_row_of_e_plus_1"])
@pytest.mark.parametrize("e", [0, 1, 2])
def test_nan_row_stays_in_its_segment(e, where, shape):
    Dout, Din = shape
    assert ops.grouped_gemm_eligible(Dout, Din, BF16)
    x, dy, w, bias, refs = _exact_case("ragged_both_sides", Dout, Din)
    assert SEGMENTS["ragged_both_sides"] == LOC_LENGTHS
    o = _offs(LOC_LENGTHS).tolist()
    if where == "last_row_of_e":
        row, owner = o[e + 1] - 1, e
    else:
        row, owner = o[e + 1], e + 1
    x, dy = x.clone(), dy.clone()
    x[row] = float("nan")
    dy[row] = float("nan")
    y, dx, dw, db = (t.cpu() for t in
                     _run_kernels(x, dy, w, bias, _offs(LOC_LENGTHS)))
    keep = torch.ones(x.shape[0], dtype=torch.bool)
    keep[row] = False
    others = [i for i in range(E) if i != owner]
    what = f"NaN row {row} (expert {owner})"
    assert torch.isnan(y[row]).all(), f"{what}: y row not NaN"
    assert torch.isnan(dx[row]).all(), f"{what}: dx row not NaN"
    nh.check_equal(y[keep], refs[0][keep], f"{what}: other rows of y")
    nh.check_equal(dx[keep], refs[1][keep], f"{what}: other rows of dx")
    assert torch.isnan(dw[owner]).all(), f"{what}: dw[{owner}] not all NaN"
    assert torch.isnan(db[owner]).all(), f"{what}: db[{owner}] not all NaN"
    nh.check_equal(dw[others], refs[2][others], f"{what}: other experts' dw")
    nh.check_equal(db[others], refs[3][others], f"{what}: other experts' db")


# -------------------------------------------------------- precision family

def _mm_loop(x, w, bias, lengths):
    """The library: one torch.mm per expert on the device."""
    return torch.cat([
        torch.mm(x[s], w[i].t()) + (bias[i] if bias is not None else 0)
        for i, s in enumerate(_segs(lengths))])


@pytest.mark.parametrize("shape", [(512, 256), (256, 512)],
                         ids=lambda s: f"out{s[0]}-in{s[1]}")
def test_precision_grouped_gemm(shape):
    Dout, Din = shape
    assert ops.grouped_gemm_eligible(Dout, Din, BF16)
    lengths = [33, BM - 1, BM + 1, 64]
    T = sum(lengths)
    g = nh._gen("grouped-prec", shape)
    x = nh._randn((T, Din), g).to(BF16)
    dy = nh._randn((T, Dout), g).to(BF16)
    w = nh._randn((E, Dout, Din), g).to(BF16)
    bias = nh._randn((E, Dout), g).to(BF16)
    y, dx, dw, db = _run_kernels(x, dy, w, bias, _offs(lengths))
    segs = _segs(lengths)
    x64, dy64, w64, b64 = (t.double() for t in (x, dy, w, bias))
    y_ref = torch.cat([x64[s] @ w64[i].t() + b64[i]
                       for i, s in enumerate(segs)])
    dx_ref = torch.cat([dy64[s] @ w64[i] for i, s in enumerate(segs)])
    dw_ref = torch.stack([dy64[s].t() @ x64[s] for s in segs])
    db_ref = torch.stack([dy64[s].sum(0) for s in segs])
    xd, dyd, wd, bd = (t.to(_dev()) for t in (x, dy, w, bias))
    y_lib = torch.cat([torch.addmm(bd[i], xd[s], wd[i].t())
                       for i, s in enumerate(segs)])
    dx_lib = torch.cat([torch.mm(dyd[s], wd[i]) for i, s in enumerate(segs)])
    dw_lib = torch.stack([torch.mm(dyd[s].t(), xd[s]) for s in segs])
    db_lib = torch.stack([dyd[s].sum(0) for s in segs])
    f_fwd, f_grad = nh.floors(BF16)
    nh.yardstick(y, y_ref, y_lib, f_fwd, what=f"grouped y {shape}")
    nh.yardstick(dx, dx_ref, dx_lib, f_grad, what=f"grouped dx {shape}")
    nh.yardstick(dw, dw_ref, dw_lib, f_grad, what=f"grouped dw {shape}")
    nh.yardstick(db, db_ref, db_lib, f_grad, what=f"grouped db {shape}")


# -------------------------------------------------------------------- plan

def _plan_vectors():
    g = nh._gen("grouped-plan")
    out = [
        ("all_zero", [0] * 5),
        ("all_in_one", [0, 0, 7 * BM + 5, 0]),
        ("all_in_last", [0, 0, 0, 3 * BM]),
        ("every_count_1_mod_BM", [1, BM + 1, 2 * BM + 1, 1, 5 * BM + 1, 1]),
        ("all_ones", [1] * 8),
        ("one_expert", [2 * BM + 17]),
        ("BM_minus_1_each", [BM - 1] * 6),
    ]
    for i in range(12):
        n = int(torch.randint(1, 10, (1,), generator=g))
        hi = [4, BM + 2, 4 * BM][i % 3]
        out.append((f"random{i}",
                    torch.randint(0, hi, (n,), generator=g).tolist()))
    return out


@pytest.mark.parametrize("name,counts", _plan_vectors(),
                         ids=[n for n, _ in _plan_vectors()])
def test_plan_covers_every_row_once(name, counts):
    Ex, T = len(counts), sum(counts)
    bound = min(T // BM + Ex, T)
    for odt in (torch.int64, torch.int32):
        offs = _offs(counts, odt)
        plan = ops.ext("grouped_gemm").grouped_gemm_plan(offs, T)
        # every block index below the launch bound is assigned or idle
        assert plan.shape == (bound, 3), (plan.shape, bound)
        owner = torch.full((T,), -1, dtype=torch.long)
        seen_idle = False
        for ex, r0, n in plan.tolist():
            if ex < 0:
                seen_idle = True
                continue
            assert not seen_idle, "an assigned block after an idle one"
            assert 0 <= ex < Ex and 1 <= n <= BM
            # no block covers a row outside its expert
            assert offs[ex] <= r0 and r0 + n <= offs[ex + 1], (ex, r0, n)
            assert (owner[r0:r0 + n] == -1).all(), "a row covered twice"
            owner[r0:r0 + n] = ex
        # every row in [0, T) is covered, by its own expert
        want = torch.repeat_interleave(torch.arange(Ex),
                                       torch.tensor(counts))
        assert torch.equal(owner, want)


def test_plan_clamps_offsets():
    offs = torch.tensor([-5, 10, 3, 10 ** 12], dtype=torch.int64)
    plan = ops.ext("grouped_gemm").grouped_gemm_plan(offs, 20).tolist()
    live = [p for p in plan if p[0] >= 0]
    assert live == [[0, 0, 10], [2, 3, 17]]


# ----------------------------------------------------------------- capture

def test_graph_replay_follows_offs():
    Dout = Din = 256
    assert ops.grouped_gemm_eligible(Dout, Din, BF16)
    la = [33, BM - 1, BM + 1, 64]
    lb = [BM + 40, 0, 97, sum(la) - (BM + 40) - 97]
    assert sum(la) == sum(lb) and min(lb) >= 0
    T = sum(la)
    xa, xb = nh.int_mat("capA", (T, Din)), nh.int_mat("capB", (T, Din))
    w = nh.int_mat("capw", (E, Dout, Din)).to(_dev())
    bias = nh.int_mat("capb", (E, Dout)).to(_dev())
    x = xa.to(_dev())
    offs = _offs(la, device=_dev())
    with torch.no_grad():
        ops.grouped_linear(x, w, offs, bias)          # warm-up, eager
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = ops.grouped_linear(x, w, offs, bias)
        x.copy_(xb.to(_dev()))
        offs.copy_(_offs(lb, device=_dev()))
        graph.replay()
        torch.cuda.synchronize()
        got = y.clone()
        eager = ops.grouped_linear(xb.to(_dev()), w, _offs(lb, device=_dev()),
                                   bias)
    nh.check_equal(got, eager, "graph replay vs eager, new routing")
    ref = torch.cat([nh.exact_mm_ref(xb[s], w[i].cpu(), bias[i].cpu())
                     for i, s in enumerate(_segs(lb))])
    nh.check_equal(got, ref, "graph replay vs exact reference")


# ---------------------------------------------------------------- autograd

def _loop_linear(x, w, b, lengths):
    return torch.cat([F.linear(x[s], w[i], b[i])
                      for i, s in enumerate(_segs(lengths))])


@pytest.mark.parametrize("follow", [False, True],
                         ids=["plain", "through_gelu"])
@pytest.mark.parametrize("shape", [(512, 256), (256, 512)],
                         ids=lambda s: f"out{s[0]}-in{s[1]}")
def test_grouped_linear_autograd(shape, follow):
    Dout, Din = shape
    assert ops.grouped_gemm_eligible(Dout, Din, BF16)
    lengths = [1, 0, BM + 1, 31] if follow else [33, BM - 1, BM + 1, 64]
    T = sum(lengths)
    g = nh._gen("grouped-autograd", shape, follow)
    x = nh._randn((T, Din), g).to(BF16)
    w = (nh._randn((E, Dout, Din), g) / Din ** 0.5).to(BF16)
    b = nh._randn((E, Dout), g).to(BF16)
    dy = nh._randn((T, Dout), g).to(BF16)
    post = nh.gelu_tanh if follow else (lambda t: t)
    offs_dev, offs_cpu = _offs(lengths, device=_dev()), _offs(lengths)
    nh.check_fwd_bwd(
        lambda x_, w_, b_: post(ops.grouped_linear(x_, w_, offs_dev, b_)),
        lambda x_, w_, b_: post(_loop_linear(x_, w_, b_, lengths)),
        lambda x_, w_, b_: post(ops.grouped_linear(x_, w_, offs_cpu, b_)),
        (x, w, b), dy, ("x", "w", "b"), BF16, _dev(), BF16,
        f"grouped_linear {shape} follow={follow}")


def test_grouped_linear_ineligible_gpu_uses_the_loop():
    """fp32 (and a 128-wide bf16) input is not eligible: the per-segment
    loop runs and agrees with the CPU path."""
    lengths = [5, 0, 9, 3]
    T = sum(lengths)
    g = nh._gen("grouped-inel")
    for dtype, Dout, Din in ((torch.float32, 256, 256), (BF16, 128, 256)):
        assert not ops.grouped_gemm_eligible(Dout, Din, dtype)
        x = nh._randn((T, Din), g).to(dtype)
        w = (nh._randn((E, Dout, Din), g) / 16).to(dtype)
        b = nh._randn((E, Dout), g).to(dtype)
        got = ops.grouped_linear(x.to(_dev()), w.to(_dev()),
                                 _offs(lengths, device=_dev()), b.to(_dev()))
        ref = ops.grouped_linear(x.double(), w.double(), _offs(lengths),
                                 b.double())
        lib = _loop_linear(x.to(_dev()), w.to(_dev()), b.to(_dev()), lengths)
        nh.yardstick(got, ref, lib, nh.floors(dtype)[0],
                     what=f"ineligible {dtype}")


def test_t0_returns_empty():
    Dout = Din = 256
    w = nh.int_mat("t0w", (E, Dout, Din)).to(_dev()).requires_grad_(True)
    x = torch.empty(0, Din, dtype=BF16, device=_dev(), requires_grad=True)
    offs = torch.zeros(E + 1, dtype=torch.int64, device=_dev())
    y = ops.grouped_linear(x, w, offs)
    assert y.shape == (0, Dout) and y.dtype == BF16
    y.sum().backward()
    assert x.grad.shape == (0, Din)
    assert w.grad.shape == w.shape and not w.grad.any()
