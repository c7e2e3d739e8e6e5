"""Training attention on the GPU across tiles, layouts and backward routes.

Exact needle / tie inputs and the fp64 yardstick at shapes that cross q-tile
and key-tile edges, through flash_attention in every head-dim-128 route
(nh.ATTN_ROUTES), through the zero-copy layouts of fused_qkv_attention and
gqa_attention, and through ring attention's block math on one GPU; plus the
argument checks of the attn_fwd / attn_bwd bindings.  Generators, checkers
and bounds live in tests/numerics_helpers.py, the CPU twin with the emulated
faults in tests/test_attention_numerics.py, the tables and measured figures
in docs/design/kernels.md ("Training attention: tiles, layouts, routes").

What the needle dv bound found (docs/design/kernels.md): the bf16 MFMA floors
addends that fall below its alignment window, so a dv pass that feeds it
P = e**-45 returned -2**-22 where the sum of do is exactly 0 (2.4e-7 to
9.5e-7 against 2**-24, in every route; torch's own bf16 GEMM does the same).
Both dv passes now hand the MFMA an exact 0 for P < 2**-40.

Run on MI355X via: pytest tests/test_attention_numerics_gpu.py -m gpu -q
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh
from tests.test_ops_numerics_gpu import _ATTN_XFAIL

GEN = {"needle": nh.train_needle_input, "tie": nh.train_tie_input}
FIELDS = ("o", "lse", "dq", "dk", "dv")


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"


def _routes(D):
    return list(nh.ATTN_ROUTES) if D == 128 else ["default"]


def _flash(causal):
    return lambda q, k, v: ops.flash_attention(q, k, v, causal=causal)


def _run_route(route, causal, case, shape):
    """flash_attention forward and backward under a route; asserts the
    backward route the dispatch reports."""
    B, H, _, S, D = shape
    expect = {"default": "v2_workspace", "recompute": "v2_recompute",
              "over_budget": "v2_recompute",
              "no_tr16": "v2_workspace+no_tr16",
              "pstore": "v2_workspace+pstore", "v1": "v1"}[route] \
        if D == 128 else "v1"
    before = ops.attention_knobs()
    with ops.attention_route(**nh.ATTN_ROUTES[route]):
        assert ops.ext().attn_bwd_route(B, H, S, D) == expect
        got = nh.run_attention(_flash(causal), case, _dev())
    assert ops.attention_knobs() == before
    return got


def _assert_bit_equal(a, b, what, fields=FIELDS):
    for n in fields:
        assert a[n].shape == b[n].shape, f"{what} {n}"
        assert torch.equal(a[n].contiguous(), b[n].contiguous()), \
            f"{what}: {n} differs"


@functools.lru_cache(maxsize=None)
def _case(kind, tag, shape, causal):
    case = GEN[kind](tag, *shape, causal)
    ref = nh.attn_ref64(case["q"], case["k"], case["v"], case["do"], causal,
                        1.0 / math.sqrt(shape[-1]))
    return case, ref


def _sid(shape):
    return "x".join(map(str, shape))


# ------------------------------------------- needle and tie, every route

def _exact_cases():
    for kind in GEN:
        for causal in (True, False):
            for S in ([1, 7] if kind == "needle" else []) + nh.TRAIN_S:
                for D in (64, 128):
                    for route in _routes(D):
                        for bh in nh.TRAIN_HEADS:
                            shape = bh + (S, D)
                            yield pytest.param(
                                kind, shape, causal, route,
                                id=f"{kind}-{'causal' if causal else 'full'}"
                                   f"-{_sid(shape)}-{route}")


@pytest.mark.parametrize("kind,shape,causal,route", list(_exact_cases()))
def test_exact_inputs(kind, shape, causal, route):
    """o, lse, dq, dk, dv of flash_attention on an exact input under a
    route."""
    case, ref = _case(kind, "gpu", shape, causal)
    got = _run_route(route, causal, case, shape)
    what = f"{kind}[{shape} causal={causal} {route}]"
    if route == "over_budget":
        _assert_bit_equal(got, _run_route("recompute", causal, case, shape),
                          what + " vs recompute")
    nh.check_train_case(got, case, causal, what, ref=ref)


# ------------------------------------------- yardstick at multi-tile shapes

def _tiled_cases():
    for causal in (True, False):
        for shape in nh.ATTN_SHAPES_TILED:
            for fam in nh.ATTN_FAMILIES:
                for route in _routes(shape[-1]):
                    yield pytest.param(
                        fam, shape, causal, route,
                        id=f"{'causal' if causal else 'full'}-{_sid(shape)}"
                           f"-{fam}-{route}")


def _yardstick_case(family, shape, causal, route):
    """What test_flash_attention does, under a route."""
    q, k, v, do = nh.attn_input(family, *shape)
    scale = 1.0 / math.sqrt(shape[-1])
    what = f"flash_attention[{family} {shape} causal={causal} {route}]"
    with ops.attention_route(**nh.ATTN_ROUTES[route]):
        qd, kd, vd = (t.to(_dev()) for t in (q, k, v))
        _, lse = ops.ext("flash_attention").attn_fwd(
            qd, kd, vd, torch.empty_like(qd), causal, scale)
        lse_ref = nh.attn_lse(q.double(), k.double(), causal, scale)
        lse_lib = nh.attn_lse(qd.float(), kd.float(), causal, scale)
        nh.yardstick(lse, lse_ref, lse_lib, nh.FLOOR_LSE, absolute=True,
                     what=what + " lse")
        tiny = None
        if family == "uniform":     # exact dq is 0: see attn_dq_cancel_scale
            tiny = {"q": nh.attn_dq_cancel_scale(q, k, v, do, causal, scale)}
        fn = lambda q, k, v: nh.attn_chain(q, k, v, causal, scale)  # noqa
        nh.check_fwd_bwd(
            lambda q, k, v: ops.flash_attention(q, k, v, causal=causal),
            fn, fn, (q, k, v), do, "qkv", torch.bfloat16, _dev(),
            torch.bfloat16, what, tiny=tiny)


@pytest.mark.parametrize("family,shape,causal,route", list(_tiled_cases()))
def test_flash_attention_tiled(family, shape, causal, route):
    _yardstick_case(family, shape, causal, route)


# ------------------------------------------------------- zero-copy layouts

LAYOUT_KINDS = ["needle", "tie", "randn", "dominant_key"]


def _layout_input(kind, tag, shape, causal):
    if kind in GEN:
        return _case(kind, tag, shape, causal)
    t = nh.attn_input(kind, *shape)
    return dict(zip(("q", "k", "v", "do"), t)), None


def _layout_check(kind, got, case, ref, causal, what):
    if kind in GEN:
        nh.check_train_case(got, case, causal, what, ref=ref)
        return
    t = tuple(case[n] for n in ("q", "k", "v", "do"))
    scale = 1.0 / math.sqrt(t[0].shape[-1])
    lse_ref = nh.attn_lse(t[0].double(), t[1].double(), causal, scale)
    lse_lib = nh.attn_lse(t[0].to(_dev()).float(), t[1].to(_dev()).float(),
                          causal, scale)
    nh.yardstick(got["lse"], lse_ref, lse_lib, nh.FLOOR_LSE, absolute=True,
                 what=what + " lse")
    nh.attn_yardstick(got, t, causal, _dev(), what)


@pytest.mark.parametrize("kind", LAYOUT_KINDS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", [257, 300])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H", [2, 4])
def test_fused_qkv_layout(kind, causal, S, hd, H):
    shape = (2, H, H, S, hd)
    case, ref = _layout_input(kind, "fused", shape, causal)
    what = f"fused_qkv[{kind} {shape} causal={causal}]"
    got = nh.run_fused_qkv(ops.fused_qkv_attention, case, _dev(), causal)
    # dqkv is an empty_like buffer written only through three strided views:
    # every element must equal the plain-layout gradient, bit for bit
    plain = nh.run_attention(_flash(causal), case, _dev())
    _assert_bit_equal(got, plain, what + " vs contiguous")
    want = torch.cat([nh._sbh(plain[n]) for n in ("dq", "dk", "dv")], -1)
    assert torch.equal(got["dqkv"], want), what + ": dqkv"
    _layout_check(kind, got, case, ref, causal, what)


@pytest.mark.parametrize("kind", LAYOUT_KINDS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", [257, 300])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 2)])
def test_gqa_layout(kind, causal, S, hd, H, Hkv):
    shape = (2, H, Hkv, S, hd)
    case, ref = _layout_input(kind, "gqa", shape, causal)
    what = f"gqa[{kind} {shape} causal={causal}]"
    got = nh.run_gqa(ops.gqa_attention, case, _dev(), causal)
    plain = nh.run_attention(_flash(causal), case, _dev())
    _assert_bit_equal(got, plain, what + " vs contiguous")
    _layout_check(kind, got, case, ref, causal, what)


# ------------------------------------------- ring block math on one GPU

@pytest.mark.parametrize("kind", ["needle", "tie", "randn"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nblk,L", [(2, 64), (3, 64), (2, 300), (3, 300)])
def test_ring_blocks(kind, D, nblk, L):
    """attn_fwd per key block plus the merge, attn_bwd per block with the
    merged o and the GLOBAL lse, as _RingAttention runs them.  lse is merged
    on the host; o, dq, dk and dv are the kernels' and are all asserted."""
    shape = (1, 2, 2, nblk * L, D)
    what = f"ring[{kind} {nblk}x{L} D={D}]"
    if kind == "randn":
        t = nh.attn_input("randn", *shape)
        got = nh.run_ring_blocks(t, nblk, _dev())
        nh.attn_yardstick(got, t, True, _dev(), what)
        return
    case, ref = _case(kind, "ring", shape, True)
    assert nh.rows_reaching_other_blocks(case, L) >= 32
    got = nh.run_ring_blocks(case, nblk, _dev())
    nh.check_train_case(got, case, True, what, ref=ref)


# ------------------------------- the two open head-dim-128 cases, per route

@pytest.mark.parametrize("route", list(nh.ATTN_ROUTES))
@pytest.mark.parametrize("family,shape,causal", sorted(_ATTN_XFAIL))
def test_open_d128_cases_report(family, shape, causal, route):
    """Report only: e(got) / e(lib) of the two strict xfails of
    test_flash_attention in every backward route (the figures are in
    docs/design/kernels.md, "Open: attention backward, head dim 128").
    Asserts that the result is finite and that over_budget == recompute."""
    q, k, v, do = nh.attn_input(family, *shape)
    scale = 1.0 / math.sqrt(shape[-1])
    got = _run_route(route, causal, (q, k, v, do), shape)
    for n in FIELDS:
        assert torch.isfinite(got[n]).all(), n
    if route == "over_budget":
        _assert_bit_equal(got, _run_route("recompute", causal, (q, k, v, do),
                                          shape), "over_budget vs recompute")
    fn = lambda q, k, v: nh.attn_chain(q, k, v, causal, scale)  # noqa: E731
    y_ref, g_ref = nh.fwd_bwd(fn, (q, k, v), do, torch.float64, "cpu")
    y_lib, g_lib = nh.fwd_bwd(fn, (q, k, v), do, torch.bfloat16, _dev())
    for n, g, r, lib in zip(("o", "dq", "dk", "dv"),
                            [got["o"]] + [got[x] for x in ("dq", "dk", "dv")],
                            [y_ref] + g_ref, [y_lib] + g_lib):
        e_got = nh._err(g, r, False, nh.TINY)
        e_lib = nh._err(lib, r, False, nh.TINY)
        print(f"OPEN128 {family} causal={causal} {route} {n}: "
              f"e_got={e_got:.3e} e_lib={e_lib:.3e} "
              f"ratio={e_got / e_lib:.2f}")


# --------------------------------------------------------- argument checks

_B, _H, _HKV, _S, _D = 1, 4, 2, 16, 64


def _good():
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16

    def t(*shape):
        return torch.randn(shape, generator=g).to(bf).to(_dev())

    a = dict(dout=t(_B, _H, _S, _D), q=t(_B, _H, _S, _D),
             k=t(_B, _HKV, _S, _D), v=t(_B, _HKV, _S, _D))
    for n in ("o", "dq", "dk", "dv"):
        a[n] = torch.full((_B, _H, _S, _D), 7.0, dtype=bf, device=_dev())
    a["lse"] = torch.zeros(_B, _H, _S, device=_dev())
    return a


def _like(t, *shape, dtype=None):
    return torch.zeros(shape, dtype=dtype or t.dtype, device=t.device)


def _row_stride(t):          # row stride D + 4: rows 8 bytes off alignment
    buf = _like(t, *t.shape[:-1], t.shape[-1] + 4)
    return buf[..., :t.shape[-1]]


def _misaligned(t):          # base address 8 bytes off 16-byte alignment
    buf = _like(t, t.numel() + 4)
    return buf[4:].view(t.shape)


_BAD_ARGS = [
    # (id, which binding, argument, replacement)
    ("k_heads_differ_from_v", "both", "v",
     lambda a: _like(a["v"], _B, _H, _S, _D)),
    ("k_not_4d", "both", "k", lambda a: a["k"][0]),
    ("v_head_dim_differs", "both", "v",
     lambda a: _like(a["v"], _B, _HKV, _S, 128)),
    ("v_shorter_than_k", "both", "v",
     lambda a: _like(a["v"], _B, _HKV, _S - 1, _D)),
    ("o_wrong_shape", "both", "o",
     lambda a: _like(a["o"], _B, _H, _S - 1, _D)),
    ("o_wrong_dtype", "both", "o",
     lambda a: _like(a["o"], _B, _H, _S, _D, dtype=torch.float16)),
    ("dq_wrong_shape", "bwd", "dq",
     lambda a: _like(a["q"], _B, _H, _S, 2 * _D)),
    ("dk_wrong_dtype", "bwd", "dk",
     lambda a: _like(a["q"], _B, _H, _S, _D, dtype=torch.float32)),
    ("dv_wrong_shape", "bwd", "dv",
     lambda a: _like(a["q"], _B, _H, _S + 1, _D)),
    ("dk_dv_kv_heads_wide", "bwd", "dk",
     lambda a: _like(a["q"], _B, _HKV, _S, _D)),
    ("lse_not_fp32", "bwd", "lse", lambda a: a["lse"].double()),
    ("lse_wrong_shape", "bwd", "lse",
     lambda a: _like(a["lse"], _B, _H, _S + 1)),
    ("lse_not_contiguous", "bwd", "lse",
     lambda a: _like(a["lse"], _B, _S, _H).transpose(1, 2)),
    ("k_on_cpu", "both", "k", lambda a: a["k"].cpu()),
    ("v_not_bf16", "both", "v", lambda a: a["v"].half()),
    ("q_last_stride", "both", "q",
     lambda a: _like(a["q"], _B, _H, _D, _S).transpose(2, 3)),
    ("k_row_stride_unaligned", "both", "k", lambda a: _row_stride(a["k"])),
    ("dout_row_stride_unaligned", "bwd", "dout",
     lambda a: _row_stride(a["dout"])),
    ("v_base_unaligned", "both", "v", lambda a: _misaligned(a["v"])),
    ("dq_base_unaligned", "bwd", "dq", lambda a: _misaligned(a["dq"])),
]


def _call(binding, a):
    e = ops.ext("flash_attention")
    scale = 1.0 / math.sqrt(_D)
    if binding == "fwd":
        return e.attn_fwd(a["q"], a["k"], a["v"], a["o"], True, scale)
    return e.attn_bwd(a["dout"], a["q"], a["k"], a["v"], a["o"], a["lse"],
                      a["dq"], a["dk"], a["dv"], True, scale)


@pytest.mark.parametrize("binding,arg,bad", [
    pytest.param(b, arg, bad, id=f"{b}-{name}")
    for name, which, arg, bad in _BAD_ARGS
    for b in (("fwd", "bwd") if which == "both" else (which,))])
def test_bindings_reject(binding, arg, bad):
    """Each call must raise before anything is launched: the outputs keep
    their fill value."""
    a = _good()
    _call(binding, a)                      # the good arguments are accepted
    a = _good()
    a[arg] = bad(a)
    outs = {n: a[n].clone() for n in ("o", "dq", "dk", "dv")
            if a[n].is_cuda}
    with pytest.raises(RuntimeError, match=f"attn_{binding}"):
        _call(binding, a)
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert torch.equal(a[n], t), f"{n} was written"


@pytest.mark.parametrize("binding", ["fwd", "bwd"])
def test_bindings_reject_empty_sequence(binding):
    a = {n: t[:, :, :0] if t.dim() == 4 else t[:, :, :0].contiguous()
         for n, t in _good().items()}
    with pytest.raises(RuntimeError, match=f"attn_{binding}.*S = 0"):
        _call(binding, a)


def test_attention_route_restores_and_rejects_unknown():
    before = ops.attention_knobs()
    assert set(before) == {"dq_recompute", "no_tr16", "pstore", "force_v1",
                           "max_ds_bytes"}
    with pytest.raises(ZeroDivisionError):
        with ops.attention_route(pstore=True, max_ds_bytes=123):
            assert ops.attention_knobs()["pstore"] is True
            assert ops.attention_knobs()["max_ds_bytes"] == 123
            1 / 0
    assert ops.attention_knobs() == before
    with pytest.raises(TypeError):
        with ops.attention_route(no_such_knob=1):
            pass
    # pstore doubles the workspace estimate: a cap between the two sizes
    # sends only the pstore run to the recompute route
    B, H, S = 1, 2, 300
    ds_bytes = B * H * S * 512 * 2
    with ops.attention_route(max_ds_bytes=ds_bytes):
        assert ops.ext().attn_bwd_route(B, H, S, 128) == "v2_workspace"
    with ops.attention_route(max_ds_bytes=ds_bytes, pstore=True):
        assert ops.ext().attn_bwd_route(B, H, S, 128) == "v2_recompute"
