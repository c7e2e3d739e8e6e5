"""ops.sample_logits on CPU tensors (the fp64 oracle of csrc/sample.hip): its
rules on hand-made rows, and the ``sampler="hip"`` plumbing of ``generate``."""
import pytest
import torch

from torchdistpackage_amd import ops
from torchdistpackage_amd.inference import generate
from torchdistpackage_amd.models.gpt2 import GPT2Config, GPT2Model
from torchdistpackage_amd.models.llama import LlamaConfig, LlamaModel


def draw(row, u, **kw):
    x = torch.tensor([row], dtype=torch.float32)
    return ops.sample_logits(x, torch.tensor([u], dtype=torch.float32),
                             **kw).item()


@pytest.mark.parametrize("u,want", [(0.0, 1), (0.4, 1), (0.6, 2)])
def test_tie_at_kth_value_goes_to_lower_index(u, want):
    # the three 2.0 tie at the 2nd value: index 1 and 2 are kept, 4 is not
    assert draw([0.0, 2.0, 2.0, 1.0, 2.0], u, top_k=2) == want


@pytest.mark.parametrize("top_p", [0.0, 1e-6, 0.5])
def test_nucleus_keeps_at_least_one_token(top_p):
    # p = (0.09, 0.24, 0.67): any top_p <= 0.67 keeps index 2 alone
    assert draw([0.0, 1.0, 2.0], 0.999, top_p=top_p) == 2


def test_nucleus_prefix_is_shortest_with_mass_at_least_top_p():
    # p = (0.67, 0.24, 0.09): 0.8 keeps two tokens, the draw walks index order
    row = [2.0, 0.0, 1.0]
    assert draw(row, 0.999, top_p=0.8) == 2
    assert draw(row, 0.999, top_p=0.95) == 2
    assert draw(row, 0.75, top_p=0.95) == 1
    assert draw(row, 0.75, top_p=0.8) == 2      # index 1 is outside


@pytest.mark.parametrize("u", [0.0, 0.5, 0.999])
def test_top_k_one_is_argmax_lowest_index(u):
    assert draw([1.0, 3.0, -2.0, 3.0], u, top_k=1, temperature=0.3) == 1


def test_draw_falls_back_to_last_kept_index():
    # u * C_last rounds to C_last in fp64 only at u = 1, which is outside
    # [0, 1) but shows the fallback: no C_i exceeds it, the last kept index
    assert draw([0.0, 5.0, 1.0, -3.0], 1.0, top_k=3) == 2
    assert draw([0.0, 5.0, 1.0, -3.0], 1 - 2.0 ** -24, top_k=3) == 2


def test_errors():
    x = torch.zeros(2, 8)
    u = torch.zeros(2)
    with pytest.raises(TypeError):
        ops.sample_logits(x.half(), u)
    with pytest.raises(ValueError):
        ops.sample_logits(x[0], u)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 16)[:, ::2], u)
    with pytest.raises(ValueError):
        ops.sample_logits(x, torch.zeros(3))
    with pytest.raises(TypeError):
        ops.sample_logits(x, u, top_k=torch.ones(2))


def tiny(family):
    torch.manual_seed(0)
    if family == "gpt2":
        return GPT2Model(GPT2Config(vocab_size=128, n_layer=2, n_head=2,
                                    dim=32, max_seq=32)).eval()
    return LlamaModel(LlamaConfig(vocab_size=128, n_layer=2, n_head=4,
                                  n_kv_head=2, dim=32, ffn_dim=64,
                                  max_seq=32)).eval()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_hip_sampler(family):
    m = tiny(family)
    idx = torch.randint(0, 128, (2, 4))

    def run(seed, **kw):
        g = torch.Generator().manual_seed(seed)
        return generate(m, idx, 8, greedy=False, sampler="hip", generator=g,
                        **kw)

    a = run(1, temperature=0.8, top_k=20, top_p=0.9)
    assert a.shape == (2, 12)
    assert torch.equal(a, run(1, temperature=0.8, top_k=20, top_p=0.9))
    assert not torch.equal(a, run(2, temperature=0.8, top_k=20, top_p=0.9))
    assert torch.equal(run(1, top_k=1), generate(m, idx, 8))


def test_torch_sampler_rejects_top_p(monkeypatch):
    m = tiny("gpt2")
    idx = torch.randint(0, 128, (1, 4))
    monkeypatch.delenv("TDPA_SAMPLER", raising=False)
    with pytest.raises(ValueError, match='sampler="hip"'):
        generate(m, idx, 2, greedy=False, top_p=0.9)
    monkeypatch.setenv("TDPA_SAMPLER", "hip")
    assert generate(m, idx, 2, greedy=False, top_p=0.9).shape == (1, 6)
