"""ops.grouped_linear on CPU tensors (the oracle path of the grouped expert
GEMM) against a hand-written fp64 loop, and the argument checks.  The HIP
kernels are covered by tests/test_grouped_gemm_gpu.py."""

import pytest
import torch

import torchdistpackage_amd.ops as ops
from tests import numerics_helpers as nh

E = 4


def _offs(lengths, dtype=torch.int64):
    o = [0]
    for c in lengths:
        o.append(o[-1] + c)
    return torch.tensor(o, dtype=dtype)


def _ref64(x, w, b, dy, lengths):
    """fp64 forward and gradients, segment by segment, no autograd."""
    x, w, dy = x.double(), w.double(), dy.double()
    o = _offs(lengths).tolist()
    y = torch.empty(x.shape[0], w.shape[1], dtype=torch.float64)
    dx = torch.empty_like(x)
    dw = torch.zeros_like(w)
    db = torch.zeros(w.shape[0], w.shape[1], dtype=torch.float64)
    for e in range(w.shape[0]):
        s = slice(o[e], o[e + 1])
        y[s] = x[s] @ w[e].t() + (b[e].double() if b is not None else 0.0)
        dx[s] = dy[s] @ w[e]
        dw[e] = dy[s].t() @ x[s]
        db[e] = dy[s].sum(0)
    return y, dx, dw, db


def _case(lengths, Dout, Din, dtype, tag):
    T = sum(lengths)
    g = nh._gen("grouped-cpu", tag, lengths, Dout, Din, dtype)
    x = nh._randn((T, Din), g).to(dtype)
    w = (nh._randn((E, Dout, Din), g) / Din ** 0.5).to(dtype)
    b = nh._randn((E, Dout), g).to(dtype)
    dy = nh._randn((T, Dout), g).to(dtype)
    return x, w, b, dy


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=nh.dtype_name)
@pytest.mark.parametrize("lengths", [[5, 3, 9, 2], [4, 0, 7, 0], [0, 0, 0, 6],
                                     [0, 0, 0, 0]],
                         ids=["plain", "empty_segments", "all_in_last", "T0"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_grouped_linear_cpu_vs_fp64(lengths, dtype, with_bias):
    Dout, Din = 24, 16
    x, w, b, dy = _case(lengths, Dout, Din, dtype, "fwd")
    if not with_bias:
        b = None
    tensors = (x, w) + ((b,) if with_bias else ())
    offs = _offs(lengths)
    ins = [t.clone().requires_grad_(True) for t in tensors]
    y = ops.grouped_linear(ins[0], ins[1], offs, ins[2] if with_bias else None)
    assert y.shape == (sum(lengths), Dout) and y.dtype == dtype
    y.backward(dy)
    y_ref, dx_ref, dw_ref, db_ref = _ref64(x, w, b, dy, lengths)
    f_fwd, f_grad = nh.floors(dtype)
    # fp32 math rounded once: one output ulp (the floors) is the whole bound
    def close(got, ref, floor, what):
        assert got.shape == ref.shape and got.dtype == dtype, what
        if ref.numel():
            err = (got.detach().double() - ref).abs().max().item()
            assert err <= floor * max(ref.abs().max().item(), nh.TINY), \
                (what, err)

    close(y, y_ref, f_fwd, "y")
    got = [ins[0].grad, ins[1].grad] + ([ins[2].grad] if with_bias else [])
    for n, g, r in zip(("dx", "dw", "db"), got, (dx_ref, dw_ref, db_ref)):
        close(g, r, f_grad, n)
    # an empty segment's parameters get exactly zero
    for e, c in enumerate(lengths):
        if c == 0:
            assert not ins[1].grad[e].any()
            if with_bias:
                assert not ins[2].grad[e].any()


def test_grouped_linear_int32_offsets_and_matches_linear():
    lengths = [3, 0, 4, 5]
    x, w, b, _ = _case(lengths, 8, 16, torch.float32, "i32")
    y64 = ops.grouped_linear(x, w, _offs(lengths), b)
    y32 = ops.grouped_linear(x, w, _offs(lengths, torch.int32), b)
    assert torch.equal(y64, y32)
    o = _offs(lengths).tolist()
    for e in range(E):
        s = slice(o[e], o[e + 1])
        assert torch.equal(y64[s], torch.nn.functional.linear(x[s], w[e],
                                                              b[e]))


def test_grouped_linear_argument_checks():
    x, w, b, _ = _case([2, 2, 2, 2], 8, 16, torch.float32, "args")
    offs = _offs([2, 2, 2, 2])
    with pytest.raises(ValueError):
        ops.grouped_linear(x[:, :8], w, offs, b)          # Din mismatch
    with pytest.raises(ValueError):
        ops.grouped_linear(x, w, offs[:-1], b)            # E entries only
    with pytest.raises(ValueError):
        ops.grouped_linear(x, w, offs, b[:, :4])          # bias shape


def test_grouped_gemm_eligible():
    bf = torch.bfloat16
    assert ops.grouped_gemm_eligible(256, 256, bf)
    assert ops.grouped_gemm_eligible(4096, 1024, bf)
    assert not ops.grouped_gemm_eligible(256, 256, torch.float32)
    assert not ops.grouped_gemm_eligible(128, 256, bf)
    assert not ops.grouped_gemm_eligible(256, 384, bf)
    assert not ops.grouped_gemm_eligible(0, 256, bf)
    assert ops.GROUPED_GEMM_BM in (64, 128, 256)
