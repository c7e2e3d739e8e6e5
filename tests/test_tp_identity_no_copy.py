"""At tensor-parallel size 1 the TP collectives are identities and must not
copy: reduce_from_tp_region hands its input through, the backward of
copy_to_tp_region hands the incoming grad through, and a ParallelBlock still
computes what a Block with the same weights computes.  (With a TP group of
more than one rank the clone stays: tests/test_tensor_parallel.py.)
"""

import torch

from torchdistpackage_amd.parallel.tensor import (Block, ParallelBlock,
                                                  copy_to_tp_region,
                                                  reduce_from_tp_region)
from torchdistpackage_amd.parallel.tensor.tp_utils import get_tp_size


def test_reduce_from_tp_shares_storage():
    assert get_tp_size() == 1
    x = torch.randn(5, 3, 8)
    y = reduce_from_tp_region(x)
    assert y.data_ptr() == x.data_ptr()
    assert y.shape == x.shape and y.stride() == x.stride()
    assert torch.equal(y, x)
    # under autograd too, and the backward is still the identity
    xg = torch.randn(5, 3, 8, requires_grad=True)
    yg = reduce_from_tp_region(xg)
    assert yg.data_ptr() == xg.data_ptr()
    g = torch.randn_like(yg)
    yg.backward(g)
    assert torch.equal(xg.grad, g)


def test_copy_to_tp_backward_hands_grad_through():
    assert get_tp_size() == 1
    seen = {}

    class Tap(torch.autograd.Function):
        """Records the grad that reaches the op below copy_to_tp_region."""

        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, grad):
            seen["ptr"] = grad.data_ptr()
            seen["strides"] = grad.stride()
            return grad

    x = torch.randn(6, 2, 4, requires_grad=True)
    y = copy_to_tp_region(Tap.apply(x))
    assert torch.equal(y, x)
    # a non-contiguous incoming grad: handed on as it is, not compacted
    g = torch.randn(4, 2, 6).permute(2, 1, 0)
    assert not g.is_contiguous()
    y.backward(g)
    assert seen["ptr"] == g.data_ptr()
    assert seen["strides"] == g.stride()
    assert torch.equal(x.grad, g)


def test_parallel_block_equals_block():
    assert get_tp_size() == 1
    dim, n_head, S, B = 32, 4, 12, 2
    torch.manual_seed(0)
    full = Block(dim, n_head)
    tp = ParallelBlock(dim, n_head, sequence_parallel=False)
    tp.init_from_full(full)

    torch.manual_seed(1)
    x = torch.randn(S, B, dim, requires_grad=True)
    x_ref = x.detach().clone().requires_grad_(True)
    out, ref = tp(x), full(x_ref)
    assert torch.allclose(out, ref, atol=1e-5), \
        f"fwd mismatch {(out - ref).abs().max().item()}"
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g)
    assert torch.allclose(x.grad, x_ref.grad, atol=1e-5)
    pairs = [
        (tp.ln_1.weight, full.ln_1.weight), (tp.ln_1.bias, full.ln_1.bias),
        (tp.ln_2.weight, full.ln_2.weight), (tp.ln_2.bias, full.ln_2.bias),
        (tp.mlp.fc1.weight, full.mlp.fc1.weight),
        (tp.mlp.fc1.bias, full.mlp.fc1.bias),
        (tp.mlp.fc2.weight, full.mlp.fc2.weight),
        (tp.mlp.fc2.bias, full.mlp.fc2.bias),
        (tp.attn.proj.weight, full.attn.proj.weight),
        (tp.attn.proj.bias, full.attn.proj.bias),
    ]
    for a, b in pairs:
        assert a.grad is not None and b.grad is not None
        assert torch.allclose(a.grad, b.grad, atol=1e-5), \
            f"grad mismatch {(a.grad - b.grad).abs().max().item()}"
