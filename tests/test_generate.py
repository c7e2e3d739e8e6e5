"""KV-cache generation vs the full-recompute oracle (fp32 CPU, tp=1)."""
import pytest
import torch

from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.inference.generate import (_alloc_caches,
                                                     decode_forward)
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaModel, llama_tiny


def naive_generate(model, idx, n):
    """O(T^2) oracle: full forward every step, greedy."""
    tokens = idx
    for _ in range(n):
        logits = model(tokens)["logits"]
        nxt = logits[:, -1].argmax(-1)
        tokens = torch.cat([tokens, nxt[:, None]], dim=1)
    return tokens


@pytest.fixture
def gpt2_tiny_model():
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_layer=2, n_head=4, dim=128,
                     max_seq=64)
    return GPT2Model(cfg).eval()


def test_gpt2_generate_matches_full_recompute(gpt2_tiny_model):
    m = gpt2_tiny_model
    torch.manual_seed(1)
    idx = torch.randint(0, 512, (2, 7))
    want = naive_generate(m, idx, 10)
    got = generate(m, idx, 10)
    assert torch.equal(got[:, :7], idx)
    assert torch.equal(got, want)


def test_llama_generate_matches_full_recompute():
    torch.manual_seed(0)
    m = LlamaModel(llama_tiny()).eval()
    torch.manual_seed(2)
    idx = torch.randint(0, 512, (2, 5))
    want = naive_generate(m, idx, 8)
    got = generate(m, idx, 8)
    assert torch.equal(got, want)


def test_generate_sampling_shapes_and_range(gpt2_tiny_model):
    m = gpt2_tiny_model
    torch.manual_seed(3)
    idx = torch.randint(0, 512, (3, 4))
    out = generate(m, idx, 6, greedy=False, temperature=0.8, top_k=20)
    assert out.shape == (3, 10)
    assert out.min() >= 0 and out.max() < 512


def test_generate_single_token_prompt(gpt2_tiny_model):
    m = gpt2_tiny_model
    idx = torch.tensor([[5]])
    want = naive_generate(m, idx, 4)
    assert torch.equal(generate(m, idx, 4), want)


def test_speculative_equals_greedy(gpt2_tiny_model):
    """Speculative decode must reproduce the target's greedy output
    EXACTLY, for any draft."""
    from torchdistpackage_amd.inference.generate import speculative_generate
    target = gpt2_tiny_model
    torch.manual_seed(42)
    draft = GPT2Model(GPT2Config(vocab_size=512, n_layer=1, n_head=2,
                                 dim=64, max_seq=64)).eval()
    torch.manual_seed(5)
    idx = torch.randint(0, 512, (1, 6))
    want = generate(target, idx, 12)
    for k in (1, 3, 4, 7):
        got = speculative_generate(target, draft, idx, 12, k=k)
        assert torch.equal(got, want), k
    # draft == target: every proposal accepted, still exact
    got = speculative_generate(target, target, idx, 12, k=4)
    assert torch.equal(got, want)


def test_speculative_llama():
    from torchdistpackage_amd.inference.generate import speculative_generate
    torch.manual_seed(0)
    target = LlamaModel(llama_tiny()).eval()
    torch.manual_seed(9)
    draft = LlamaModel(llama_tiny()).eval()
    idx = torch.randint(0, 512, (1, 5))
    want = generate(target, idx, 10)
    got = speculative_generate(target, draft, idx, 10, k=3)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# the one cached-attention step: host-int pos0 (eager) and 1-element tensor
# pos0 (the form GraphedDecoder captures) drive the same decode_forward
# ---------------------------------------------------------------------------

DEC_B, DEC_PROMPT, DEC_STEPS, DEC_CACHE = 2, 5, 7, 16


def _gpt2_tiny():
    torch.manual_seed(0)
    return GPT2Model(GPT2Config(vocab_size=512, n_layer=2, n_head=4, dim=128,
                                max_seq=64)).eval()


def _llama_tiny():           # n_kv_head=2 < n_head=4: the GQA expand
    torch.manual_seed(0)
    return LlamaModel(llama_tiny()).eval()


DEC_MODELS = {"gpt2": _gpt2_tiny, "llama": _llama_tiny}


def _prefilled(model, attn_impl):
    """(prompt, caches after the prompt, first generated token (B, 1))."""
    idx = torch.randint(0, 512, (DEC_B, DEC_PROMPT),
                        generator=torch.Generator().manual_seed(11))
    caches = _alloc_caches(model, DEC_B, DEC_CACHE)
    logits = decode_forward(model, idx, caches, 0, attn_impl=attn_impl)
    return idx, caches, logits.argmax(-1, keepdim=True)


@pytest.mark.parametrize("family", sorted(DEC_MODELS))
def test_tensor_pos_equals_int_pos_hip(family):
    """attn_impl="hip" (the fp32 oracle on CPU): the tensor-pos0 step and
    the int-pos0 step are the same arithmetic, bit for bit."""
    m = DEC_MODELS[family]()
    _, c_int, tok = _prefilled(m, "hip")
    c_ten = [(k.clone(), v.clone()) for k, v in c_int]
    for pos in range(DEC_PROMPT, DEC_PROMPT + DEC_STEPS):
        a = decode_forward(m, tok, c_int, pos, attn_impl="hip")
        b = decode_forward(m, tok, c_ten, torch.tensor([pos]),
                           attn_impl="hip")
        assert torch.equal(a, b), pos
        tok = a.argmax(-1, keepdim=True)
    for (ka, va), (kb, vb) in zip(c_int, c_ten):
        assert torch.equal(ka, kb) and torch.equal(va, vb)


@pytest.mark.parametrize("family", sorted(DEC_MODELS))
def test_tensor_pos_masked_sdpa_matches_full_recompute(family):
    """attn_impl="sdpa": the tensor-pos0 step over the full-length cache,
    its additive mask opened one slot per step as GraphedDecoder.step does,
    reproduces the full-recompute oracle's tokens.  (Logits are not compared
    bitwise: masked full-length SDPA and sliced SDPA sum in other orders.)"""
    m = DEC_MODELS[family]()
    idx, caches, tok = _prefilled(m, "sdpa")
    mask = torch.full((1, 1, 1, DEC_CACHE), float("-inf"))
    mask[..., :DEC_PROMPT + 1] = 0
    pos, pos_t, toks = DEC_PROMPT, torch.tensor([DEC_PROMPT]), [tok]
    for _ in range(DEC_STEPS):
        logits = decode_forward(m, tok, caches, pos_t, attn_impl="sdpa",
                                mask=mask)
        tok = logits.argmax(-1, keepdim=True)
        toks.append(tok)
        pos += 1
        pos_t += 1
        mask[..., pos] = 0
    got = torch.cat([idx] + toks, dim=1)
    assert torch.equal(got, naive_generate(m, idx, DEC_STEPS + 1))


@pytest.mark.parametrize("family", sorted(DEC_MODELS))
def test_tensor_pos_argument_errors(family):
    m = DEC_MODELS[family]()
    idx, caches, tok = _prefilled(m, "sdpa")
    pos_t = torch.tensor([DEC_PROMPT])
    mask = torch.zeros(1, 1, 1, DEC_CACHE)
    for impl in ("hip", "sdpa"):
        with pytest.raises(ValueError, match="single-token"):
            decode_forward(m, idx[:, :2], caches, pos_t, attn_impl=impl,
                           mask=mask)
    with pytest.raises(ValueError, match="mask"):
        decode_forward(m, tok, caches, pos_t, attn_impl="sdpa")
