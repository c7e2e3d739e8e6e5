"""The sampling kernel (csrc/sample.hip) against the CPU route of
ops.sample_logits (fp64), token for token, and the sampled GraphedDecoder.

Inputs keep every decision away from a boundary in exact arithmetic: ``u``
sits at the fp64 midpoint of the draw interval of a token whose renormalised
probability is >= 1e-3, and a nominal ``top_p`` is replaced by the midpoint of
the two cumulative masses of the sorted list that bracket it, so each decision
has a margin of >= 5e-4 in relative mass.  The kernel sums integers of 2^-40
of the largest weight: its sums are off by below V * 2^-40 plus the fp32
rounding of exp2's argument, orders of magnitude inside that margin.  The
margin is a condition on the inputs; the comparison is exact."""
import functools

import pytest
import torch

import numerics_helpers as nh
from torchdistpackage_amd import ops
from torchdistpackage_amd.inference.generate import GraphedDecoder
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel
from torchdistpackage_amd.ops.sample import _kept_ref

pytestmark = pytest.mark.gpu

B, NU = 3, 8


@functools.lru_cache(maxsize=None)
def logits_of(V, dtype):
    return (torch.randn(B, V, generator=nh._gen("sample", V)) * 4).to(dtype)


@functools.lru_cache(maxsize=None)
def case(V, dtype, T, top_k, top_p):
    """(logits, u, temperature, top_k, top_p, want) on the CPU: each of the B
    rows NU times, with the u of up to NU of its likeliest kept tokens."""
    x = logits_of(V, dtype)
    t = torch.full((B,), T)
    k = torch.full((B,), top_k or 0, dtype=torch.int32)
    p = torch.ones(B)
    if top_p is not None:
        kept, w = _kept_ref(x, t, k, p)
        ws = torch.where(kept, w, 0.0).sort(-1, descending=True).values
        cum = torch.nn.functional.pad(ws.cumsum(-1) / ws.sum(-1, keepdim=True),
                                      (1, 0))
        i = torch.searchsorted(cum[:, 1:].contiguous(),
                               torch.full((B, 1), top_p, dtype=cum.dtype))
        p = ((cum.gather(1, i) + cum.gather(1, i + 1)) / 2)[:, 0].float()
    kept, w = _kept_ref(x, t, k, p)
    w = torch.where(kept, w, 0.0)
    C = w.cumsum(-1)
    prob, tok = (w / C[:, -1:]).topk(NU, -1)
    mid = (C.gather(1, tok) - w.gather(1, tok) / 2) / C[:, -1:]
    mid = torch.where(prob >= 1e-3, mid, mid[:, :1])
    rows = torch.arange(B).repeat_interleave(NU)
    ins = (x[rows], mid.reshape(-1).float(), t[rows], k[rows], p[rows])
    return ins + (ops.sample_logits(*ins),)


def on_gpu(ins):
    return [a.cuda() for a in ins]


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("top_k,top_p", [(None, None), (1, None), (50, None),
                                         (None, 0.9), (50, 0.9), (2048, 0.5)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1000, 50257, 128256])
def test_kernel_matches_oracle(V, dtype, top_k, top_p, T):
    *ins, want = case(V, dtype, T, top_k, top_p)
    got = ops.sample_logits(*on_gpu(ins))
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), (got.cpu(), want)


def test_strided_two_byte_aligned_rows_and_out_buffer():
    V = 50257
    x, u, t, k, p, want = case(V, torch.bfloat16, 0.7, 50, 0.9)
    n = x.shape[0]
    big = torch.zeros(n, 2, V, dtype=torch.bfloat16, device="cuda")
    big[:, -1, :] = x.cuda()
    view = big[:, -1, :]
    assert view.stride() == (2 * V, 1) and view[1].data_ptr() % 16 != 0
    out = torch.full((n, 1), -1, dtype=torch.int64, device="cuda")
    got = ops.sample_logits(view, *on_gpu((u, t, k, p)), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out[:, 0].cpu(), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_dominant_logit_at_the_edges(dtype):
    # rows of an odd V start off the 16-byte grid: the dominant logit at
    # index 0, at V - 1, and at the last element of each row's partial head
    V = 1001
    x = logits_of(V, dtype).cuda()
    per = 16 // x.element_size()
    head = [(-(x[r].data_ptr() % 16 // x.element_size())) % per
            for r in range(B)]
    assert any(head), head
    u = torch.full((B,), 0.5, device="cuda")
    for pos in ([0] * B, [V - 1] * B, [h - 1 if h else per - 1 for h in head]):
        y = x.clone()
        y[torch.arange(B), pos] = 40.0
        got = ops.sample_logits(y, u)
        assert got.tolist() == pos
        assert torch.equal(got.cpu(), ops.sample_logits(y.cpu(), u.cpu()))


def test_per_row_parameters():
    x, u, _, _, _, _ = case(50257, torch.bfloat16, 1.0, None, None)
    x, u = x[:4].cuda(), u[:4].cuda()
    rows = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.6), (0.5, 7, 0.8)]
    t, k, p = (torch.tensor(c, dtype=d, device="cuda") for c, d in
               zip(zip(*rows), (torch.float32, torch.int32, torch.float32)))
    got = ops.sample_logits(x, u, t, k, p)
    for r, (tr, kr, pr) in enumerate(rows):
        one = ops.sample_logits(x[r:r + 1], u[r:r + 1], tr, kr, pr)
        assert one.item() == got[r].item(), r


def test_captured_launch_reads_rewritten_inputs():
    a = on_gpu(case(50257, torch.bfloat16, 0.7, 50, 0.9)[:5])
    b = on_gpu(case(50257, torch.bfloat16, 0.7, 1, None)[:5])
    eager = [ops.sample_logits(*c).clone() for c in (a, b)]
    static = [c.clone() for c in a]
    out = torch.zeros(a[0].shape[0], dtype=torch.int64, device="cuda")
    ops.sample_logits(*static, out=out)                      # warm up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample_logits(*static, out=out)
    for c, want in ((a, eager[0]), (b, eager[1]), (a, eager[0])):
        for s, v in zip(static, c):
            s.copy_(v)
        for _ in range(2):
            out.fill_(-1)
            g.replay()
            assert torch.equal(out, want)


def tiny(family):
    torch.manual_seed(0)
    if family == "gpt2":
        cfg = GPT2Config(vocab_size=2048, n_layer=2, n_head=4, dim=256,
                         max_seq=64)
        return GPT2Model(cfg, device="cuda", dtype=torch.bfloat16).eval()
    cfg = LlamaConfig(vocab_size=2048, n_layer=2, n_head=8, n_kv_head=2,
                      dim=256, ffn_dim=512, max_seq=64)
    return LlamaModel(cfg, device="cuda", dtype=torch.bfloat16).eval()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_graphed_decoder_sampling(family):
    m = tiny(family)
    idx = torch.randint(0, 2048, (2, 6), device="cuda")
    greedy = GraphedDecoder(m, batch=2, max_seq=32).generate(idx, 16)
    assert torch.equal(
        GraphedDecoder(m, batch=2, max_seq=32, top_k=1).generate(idx, 16),
        greedy)

    kw = dict(temperature=0.8, top_k=50, top_p=0.9)
    dec = GraphedDecoder(m, batch=2, max_seq=32, seed=5, **kw)
    toks = dec.generate(idx, 16)
    twin = GraphedDecoder(m, batch=2, max_seq=32, seed=5, **kw)
    assert torch.equal(twin.generate(idx, 16), toks)
    assert not torch.equal(toks, greedy)

    # every token lies in the oracle's kept set of the logits it came from
    par = [torch.full((2,), v, dtype=d) for v, d in
           ((0.8, torch.float32), (50, torch.int32), (0.9, torch.float32))]
    dec.prefill(idx)
    for _ in range(8):
        dec.step()
        kept, _ = _kept_ref(dec._logits.cpu(), *par)
        assert kept.gather(1, dec.in_tok.cpu()).all()

    dec.set_sampling(top_k=1)           # the same graph, now greedy
    assert torch.equal(dec.generate(idx, 16), greedy)
