"""The fused dk/dv kernel of the head-dim-128 backward against the two-pass
kernels it replaces (knob ``split_dkdv``), bit for bit.

The fused kernel keeps the two passes' arithmetic and accumulation order, so
dq, dk and dv must be equal in every bit: on the dS-workspace route (default
knobs against ``split_dkdv``) and on the recompute route (``dq_recompute``
against ``dq_recompute, split_dkdv``), for causal and full masks, at sequence
lengths that give a partial query tile (33), the query-tile edge (64, 65),
exactly one 256-key block (256), one key in the second block (257) and
three key blocks with causal skipping (520), with and without GQA, on random
inputs and on the needle / tie / dominant-key inputs of
tests/numerics_helpers.py, through flash_attention and through the strided
layouts of fused_qkv_attention and gqa_attention.

Run on MI355X via: pytest tests/test_attention_fused_dkdv_gpu.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh
from tests.test_attention_numerics_gpu import _case

D = 128
HEADS = [(1, 2, 2), (2, 4, 2), (1, 4, 1)]          # (B, H, Hkv)
SEQS = [33, 64, 65, 256, 257, 300, 520]
INPUTS = ["randn", "needle", "tie", "dominant_key"]
GRADS = ("dq", "dk", "dv")
# (knobs of the fused run, knobs of its two-pass partner)
PAIRS = {
    "workspace": ({"split_dkdv": False}, {"split_dkdv": True}),
    "recompute": ({"dq_recompute": True, "split_dkdv": False},
                  {"dq_recompute": True, "split_dkdv": True}),
}   # split_dkdv=False is the default, spelled out against TDPA_SPLIT_DKDV


def _dev():
    return torch.device("cuda:0")


def setup_module(module):
    if torch.cuda.is_available():
        assert ops.extension_available(), \
            "HIP extension must be built+loaded on a GPU box"


def _input(kind, shape, causal):
    if kind in ("needle", "tie"):
        return _case(kind, "gpu", shape, causal)[0]
    return nh.attn_input(kind, *shape)


def _assert_equal(a, b, what):
    for n in GRADS:
        nh.check_equal(a[n].contiguous(), b[n].contiguous(), f"{what} {n}")


def _mask_id(causal):
    return "causal" if causal else "full"


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", SEQS)
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "x".join(map(str, h)))
def test_fused_equals_two_pass(heads, S, causal):
    """dq, dk, dv of flash_attention: fused against two-pass, both routes,
    every input family."""
    B, H, _ = heads
    shape = heads + (S, D)
    fn = lambda q, k, v: ops.flash_attention(q, k, v, causal=causal)  # noqa: E731
    for kind in INPUTS:
        case = _input(kind, shape, causal)
        for pair, (fused, split) in PAIRS.items():
            base = "v2_workspace" if pair == "workspace" else "v2_recompute"
            with ops.attention_route(**fused):
                assert ops.ext().attn_bwd_route(B, H, S, D) == base
                a = nh.run_attention(fn, case, _dev())
            with ops.attention_route(**split):
                assert ops.ext().attn_bwd_route(B, H, S, D) == \
                    base + "+split_dkdv"
                b = nh.run_attention(fn, case, _dev())
            _assert_equal(a, b, f"{kind}[{shape} {_mask_id(causal)} {pair}]")


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", SEQS)
def test_fused_equals_two_pass_fused_qkv_layout(S, causal):
    """q, k, v and the gradients as column blocks of one (S, B, 3*H*hd)
    buffer (fused_qkv_attention)."""
    shape = (1, 2, 2, S, D)
    case = _input("randn", shape, causal)
    for pair, (fused, split) in PAIRS.items():
        with ops.attention_route(**fused):
            a = nh.run_fused_qkv(ops.fused_qkv_attention, case, _dev(), causal)
        with ops.attention_route(**split):
            b = nh.run_fused_qkv(ops.fused_qkv_attention, case, _dev(), causal)
        _assert_equal(a, b, f"fused_qkv[{shape} {_mask_id(causal)} {pair}]")
        nh.check_equal(a["dqkv"], b["dqkv"], f"fused_qkv dqkv {pair}")


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", SEQS)
def test_fused_equals_two_pass_gqa_layout(S, causal):
    """GQA with v a strided view of an (S, B, Hkv*hd) buffer: the V^T
    fragments and the K image are staged through non-trivial strides."""
    shape = (2, 4, 2, S, D)
    case = _input("randn", shape, causal)
    for pair, (fused, split) in PAIRS.items():
        with ops.attention_route(**fused):
            a = nh.run_gqa(ops.gqa_attention, case, _dev(), causal)
        with ops.attention_route(**split):
            b = nh.run_gqa(ops.gqa_attention, case, _dev(), causal)
        _assert_equal(a, b, f"gqa[{shape} {_mask_id(causal)} {pair}]")


def test_route_names():
    """The fused kernel changes no existing route name; split_dkdv shows only
    where it alone selects the two-pass kernels; knobs come back on exit."""
    route = lambda: ops.ext().attn_bwd_route(2, 4, 300, D)  # noqa: E731
    before = ops.attention_knobs(extended=True)
    assert "split_dkdv" in before
    assert set(before) - set(ops.attention_knobs()) == {"split_dkdv"}
    with ops.attention_route(split_dkdv=False):
        assert route() == "v2_workspace"
        with ops.attention_route(split_dkdv=True):
            assert ops.attention_knobs(extended=True)["split_dkdv"] is True
            assert route() == "v2_workspace+split_dkdv"
            with ops.attention_route(pstore=True):
                assert route() == "v2_workspace+pstore"
            with ops.attention_route(no_tr16=True):
                assert route() == "v2_workspace+no_tr16"
            with ops.attention_route(dq_recompute=True):
                assert route() == "v2_recompute+split_dkdv"
            with ops.attention_route(force_v1=True):
                assert route() == "v1"
        assert ops.attention_knobs(extended=True)["split_dkdv"] is False
        with ops.attention_route(pstore=True):
            assert route() == "v2_workspace+pstore"
        with ops.attention_route(no_tr16=True):
            assert route() == "v2_workspace+no_tr16"
        with ops.attention_route(dq_recompute=True):
            assert route() == "v2_recompute"
        with ops.attention_route(max_ds_bytes=0):
            assert route() == "v2_recompute"
    assert ops.attention_knobs(extended=True) == before


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
def test_fused_repeatable(causal):
    """Two fused calls on the same inputs agree in every bit."""
    shape = (2, 4, 2, 520, D)
    case = _input("randn", shape, causal)
    fn = lambda q, k, v: ops.flash_attention(q, k, v, causal=causal)  # noqa: E731
    with ops.attention_route(split_dkdv=False):
        a = nh.run_attention(fn, case, _dev())
        b = nh.run_attention(fn, case, _dev())
    _assert_equal(a, b, f"repeat[{shape} {_mask_id(causal)}]")
