"""CPU twin of tests/test_attention_numerics_gpu.py.

The exact-input generators and checkers of tests/numerics_helpers.py
("training attention: exact inputs") run here on the fp32 CPU paths of
flash_attention, fused_qkv_attention, gqa_attention and the ring helpers, and
on a small blockwise attention with one switch per emulated kernel fault:
every fault must be rejected by the checker named for it, and the same code
with no switch set must pass everything.  docs/design/kernels.md ("Training
attention: tiles, layouts, routes") has the derivation of the bounds.
"""

import math

import pytest
import torch

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

GEN = {"needle": nh.train_needle_input, "tie": nh.train_tie_input}


def _flash(causal):
    return lambda q, k, v: ops.flash_attention(q, k, v, causal=causal)


# ------------------------------------------------------- the CPU paths

def _cpu_cases():
    for kind in GEN:
        for causal in (True, False):
            for S in (33, 257, 300):
                for D in (64, 128):
                    for bh in nh.TRAIN_HEADS:
                        yield kind, bh + (S, D), causal
            yield kind, (2, 4, 2, 520, 128), causal


def _id(kind, shape, causal):
    return f"{kind}-{'causal' if causal else 'full'}-" + \
        "x".join(map(str, shape))


@pytest.mark.parametrize("kind,shape,causal", [
    pytest.param(*c, id=_id(*c)) for c in _cpu_cases()])
def test_flash_attention_cpu(kind, shape, causal):
    case = GEN[kind]("cpu", *shape, causal)
    got = nh.run_attention(_flash(causal), case, "cpu")
    nh.check_train_case(got, case, causal, _id(kind, shape, causal))


@pytest.mark.parametrize("kind", list(GEN))
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", [1, 7])
def test_needle_short_cpu(kind, causal, S):
    """A sequence shorter than any tile; the tie input degenerates to single
    needles where no pair fits."""
    case = GEN[kind]("short", 2, 4, 2, S, 64, causal)
    got = nh.run_attention(_flash(causal), case, "cpu")
    nh.check_train_case(got, case, causal, f"{kind} S={S}")


@pytest.mark.parametrize("kind", list(GEN))
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,hd,S", [(2, 64, 257), (4, 128, 300)])
def test_fused_qkv_attention_cpu(kind, causal, H, hd, S):
    case = GEN[kind]("fused", 2, H, H, S, hd, causal)
    got = nh.run_fused_qkv(ops.fused_qkv_attention, case, "cpu", causal)
    assert torch.isfinite(got["dqkv"]).all()
    nh.check_train_case(got, case, causal, f"fused_qkv {kind}")


@pytest.mark.parametrize("kind", list(GEN))
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hkv,hd,S", [(4, 2, 64, 257), (8, 2, 128, 300)])
def test_gqa_attention_cpu(kind, causal, H, Hkv, hd, S):
    case = GEN[kind]("gqa", 2, H, Hkv, S, hd, causal)
    got = nh.run_gqa(ops.gqa_attention, case, "cpu", causal)
    nh.check_train_case(got, case, causal, f"gqa {kind}")


@pytest.mark.parametrize("kind", list(GEN) + ["randn"])
@pytest.mark.parametrize("nblk,L,D", [(2, 64, 64), (3, 64, 128),
                                      (2, 300, 128), (3, 300, 64)])
def test_ring_blocks_cpu(kind, nblk, L, D):
    """lse is merged on the host by the ring, so o, dq, dk, dv are what the
    block math is held to (the merged lse is checked all the same)."""
    S = nblk * L
    what = f"ring {kind} {nblk}x{L} D={D}"
    if kind == "randn":
        t = nh.attn_input("randn", 1, 2, 2, S, D)
        got = nh.run_ring_blocks(t, nblk, "cpu")
        nh.attn_yardstick(got, t, True, "cpu", what)
        return
    case = GEN[kind]("ring", 1, 2, 2, S, D, True)
    assert nh.rows_reaching_other_blocks(case, L) >= 32
    got = nh.run_ring_blocks(case, nblk, "cpu")
    nh.check_train_case(got, case, True, what)


# --------------------------------------------- teeth: emulated kernel faults

FAULTS = {
    # fault: (input, quantity whose check must reject it)
    "skip_tile": ("needle", "o"),          # one key tile skipped for a q-tile
    "diag_unmasked": ("randn", "y"),       # diagonal tile treated as unmasked
    "drop_tail": ("needle", "o"),          # ragged last tile loses its tail key
    "rescale_tie": ("tie", "o"),           # rescale wrong at equal maxima
    "delta_neighbour": ("needle", "dq"),   # delta taken from the next row
    "gqa_missing_head": ("needle", "dv"),  # GQA sum misses one q-head
    "dv_wrong_qtile": ("needle", "dv"),    # dv pairs P with another tile's do
    "ds_scaled": ("tie", "dq"),            # dS scaled by 1.02
}


def blockwise_attention(tensors, causal, fault=None, QT=64, KT=64):
    """Flash attention the way the kernels do it, in torch on the CPU: 64-row
    q-tiles, 64-key tiles, online softmax, whole key tiles above the diagonal
    skipped, P and dS rounded to bf16 before their matmuls, per-q-head dk/dv
    partials rounded to bf16 and summed over the GQA group.  ``fault``
    switches one emulated kernel bug on (``FAULTS``).

    "rescale_tie": swapping the two rescale weights is the identity when the
    maxima are equal (both weights are 1), so the emulated fault is the
    asymmetric one a wrong comparison produces: where a tile's row maximum
    equals the running one, the running sum l is replaced by the tile's
    instead of added to."""
    assert fault is None or fault in FAULTS
    q, k, v, do = (t.float() for t in tensors)
    B, H, S, D = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    scale = 1.0 / math.sqrt(D)
    bf = torch.bfloat16
    rnd = lambda t: t.to(bf).float()                        # noqa: E731
    qts = [(r, min(S, r + QT)) for r in range(0, S, QT)]
    kts = [(c, min(S, c + KT)) for c in range(0, S, KT)]
    skip = (len(qts) - 1, min(1, len(kts) - 1))

    def scores(b, h, qi, ki):
        """Masked scores of a (q-tile, key-tile) pair; None if skipped."""
        (r0, r1), (k0, k1) = qts[qi], kts[ki]
        if causal and k0 > r1 - 1:
            return None
        if fault == "skip_tile" and (qi, ki) == skip:
            return None
        s = q[b, h, r0:r1] @ k[b, h // rep, k0:k1].T * scale
        if causal and k1 - 1 > r0 and fault != "diag_unmasked":
            i = torch.arange(r0, r1)[:, None]
            j = torch.arange(k0, k1)[None, :]
            s = s.masked_fill(j > i, float("-inf"))
        if fault == "drop_tail" and k1 == S and S % KT:
            s[:, -1] = float("-inf")
        return s

    o = torch.empty(B, H, S, D)
    lse = torch.empty(B, H, S)
    for b in range(B):
        for h in range(H):
            for qi, (r0, r1) in enumerate(qts):
                m = torch.full((r1 - r0,), float("-inf"))
                l = torch.zeros(r1 - r0)
                acc = torch.zeros(r1 - r0, D)
                for ki, (k0, k1) in enumerate(kts):
                    s = scores(b, h, qi, ki)
                    if s is None:
                        continue
                    mt = s.max(-1).values
                    m_new = torch.maximum(m, mt)
                    alpha = torch.exp(m - m_new)
                    p = torch.exp(s - m_new[:, None])
                    l_new = l * alpha + p.sum(-1)
                    if fault == "rescale_tie":
                        l_new = torch.where(mt == m, p.sum(-1), l_new)
                    l = l_new
                    acc = acc * alpha[:, None] + \
                        rnd(p) @ v[b, h // rep, k0:k1]
                    m = m_new
                o[b, h, r0:r1] = acc / l[:, None]
                lse[b, h, r0:r1] = m + torch.log(l)
    o = o.to(bf)

    delta = (do * o.float()).sum(-1)
    if fault == "delta_neighbour":
        delta = delta.roll(-1, -1)
    dq = torch.zeros(B, H, S, D)
    dkh = torch.zeros(B, H, S, D)
    dvh = torch.zeros(B, H, S, D)
    for b in range(B):
        for h in range(H):
            for qi, (r0, r1) in enumerate(qts):
                rows = torch.arange(r0, r1)
                do_dv = do[b, h, (rows + QT) % S] \
                    if fault == "dv_wrong_qtile" else do[b, h, r0:r1]
                for ki, (k0, k1) in enumerate(kts):
                    s = scores(b, h, qi, ki)
                    if s is None:
                        continue
                    p = torch.exp(s - lse[b, h, r0:r1, None])
                    dp = do[b, h, r0:r1] @ v[b, h // rep, k0:k1].T
                    ds = p * (dp - delta[b, h, r0:r1, None]) * scale
                    if fault == "ds_scaled":
                        ds = ds * 1.02
                    ds = rnd(ds)
                    dq[b, h, r0:r1] += ds @ k[b, h // rep, k0:k1]
                    dkh[b, h, k0:k1] += ds.T @ q[b, h, r0:r1]
                    dvh[b, h, k0:k1] += rnd(p).T @ do_dv
    heads = rep - 1 if fault == "gqa_missing_head" else rep

    def fold(t):
        t = rnd(t).view(B, Hkv, rep, S, D)
        return t[:, :, :heads].sum(2).to(bf)

    return dict(o=o, lse=lse, dq=dq.to(bf), dk=fold(dkh), dv=fold(dvh))


TEETH_SHAPE = (1, 4, 2, 300, 64)      # 5 tiles, ragged last one, GQA


def _teeth_input(name):
    if name == "randn":
        return nh.attn_input("randn", *TEETH_SHAPE)
    return GEN[name]("teeth", *TEETH_SHAPE, True)


def _teeth_check(name, got, data):
    what = f"emulated {name}"
    if name == "randn":
        nh.attn_yardstick(got, data, True, "cpu", what)
    else:
        nh.check_train_case(got, data, True, what)


def _tensors(data):
    return data if isinstance(data, tuple) else \
        tuple(data[n] for n in ("q", "k", "v", "do"))


@pytest.mark.parametrize("name", ["needle", "tie", "randn"])
def test_clean_blockwise_passes(name):
    data = _teeth_input(name)
    _teeth_check(name, blockwise_attention(_tensors(data), True), data)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_rejected(fault):
    name, field = FAULTS[fault]
    data = _teeth_input(name)
    got = blockwise_attention(_tensors(data), True, fault)
    with pytest.raises(AssertionError, match=rf"emulated {name} {field}:"):
        _teeth_check(name, got, data)


@pytest.mark.parametrize("D", [64, 128])
def test_unmasked_diagonal_is_rejected_by_short_tie(D):
    """At S = 300 the exact inputs cannot see an unmasked diagonal tile: no
    key beyond the diagonal of a 64-key tile carries a row's pattern (the
    pairs are 65 apart), which is why FAULTS names the randn yardstick for
    it.  Below S = 130 the tie pairs are S // 2 apart and share a tile: rows
    16..31 of S = 33 see the first key of the pair (16, 32) and must return
    its v row alone, so letting them see key 32 breaks o.  The GPU file runs
    this shape in every route."""
    data = GEN["tie"]("teeth", 1, 4, 2, 33, D, True)
    t = _tensors(data)
    nh.check_train_case(blockwise_attention(t, True), data, True, "clean")
    got = blockwise_attention(t, True, "diag_unmasked")
    with pytest.raises(AssertionError, match=r"unmasked o:"):
        nh.check_train_case(got, data, True, "unmasked")


def test_absolute_bound_accepts_dropped_tail_key():
    """The bounds tests/test_ops_gpu.py puts on randn (3e-2 forward, 8e-2
    backward, absolute) accept a kernel that drops the last key of a ragged
    tile; the needle input rejects it (test_fault_is_rejected)."""
    t = nh.attn_input("randn", *TEETH_SHAPE)
    got = blockwise_attention(t, True, "drop_tail")
    ref = nh.attn_ref64(*t, True, 1.0 / math.sqrt(TEETH_SHAPE[-1]))
    assert (got["o"].double() - ref["o"]).abs().max() < 3e-2
    for n in ("dq", "dk", "dv"):
        assert (got[n].double() - ref[n]).abs().max() < 8e-2, n
    # ... although the output of the row that lost its key is plainly wrong
    clean = blockwise_attention(t, True)
    assert not torch.equal(got["o"][:, :, -1], clean["o"][:, :, -1])
