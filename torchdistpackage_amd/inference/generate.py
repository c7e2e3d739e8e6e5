"""KV-cache autoregressive generation for the model zoo (single-GPU serving).

The reference has no inference path at all (its ``forward_eval`` pipelines
full forwards, pipeline_sched.py:233-269); this module adds the serving-side
basics: prefill + incremental decode with per-layer K/V caches, greedy and
temperature/top-k sampling.

Scope: tp=1 (single device).  At tp=1 the Col/Row parallel linears, SP
plumbing and vocab-parallel head are all inert, so the training modules'
weights are reused directly by the ``decode_step`` methods
(parallel/tensor/attn.py, models/llama.py).  Decode-shaped attention is
GEMV-like and memory-bound, so the training flash kernel is the wrong tool;
every path here takes ``attn_impl``: ``"sdpa"`` (eager SDPA over the cache,
the default) or ``"hip"`` (the split-KV decode kernel,
ops.decode_attention).  ``None`` reads ``TDPA_DECODE_ATTN``.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ..ops import resolve_decode_attn_impl
from ..parallel.tensor import get_tp_size


def _alloc_caches(model, batch: int,
                  max_seq: int) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Zeroed per-layer (k, v) caches (B, n_kv, max_seq, hd) for ``model``,
    on its parameters' device and dtype."""
    cfg = model.cfg
    p = next(model.parameters())
    shape = (batch, getattr(cfg, "n_kv_head", cfg.n_head), max_seq,
             cfg.dim // cfg.n_head)
    return [(torch.zeros(shape, device=p.device, dtype=p.dtype),
             torch.zeros(shape, device=p.device, dtype=p.dtype))
            for _ in range(cfg.n_layer)]


def _sample(logits: torch.Tensor, greedy: bool, temperature: float,
            top_k: Optional[int]) -> torch.Tensor:
    """logits (B, V) -> next token ids (B,)."""
    if greedy:
        return logits.argmax(dim=-1)
    logits = logits.float() / max(temperature, 1e-5)
    if top_k is not None and top_k < logits.shape[-1]:
        kth = logits.topk(top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, 1).squeeze(-1)


def decode_forward(model, idx: torch.Tensor, caches, pos0,
                   all_logits: bool = False, attn_impl: Optional[str] = None,
                   mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``idx`` (B, S_new) through ``model``'s cached stack at ``pos0``: a
    host int, or a 1-element device tensor for the graphed single-token
    step.  Each model family holds its own ``decode_forward``
    (models/gpt2.py, models/llama.py); the arguments are described there."""
    return model.decode_forward(idx, caches, pos0, all_logits, attn_impl,
                                mask)


# the per-family names this function replaced; code written against them
# (same arguments) keeps importing
_gpt2_decode_forward = _llama_decode_forward = decode_forward


class GraphedDecoder:
    """Greedy single-token decode captured as ONE hipGraph.

    The eager decode step is launch-bound (~330 kernels for 24 layers,
    measured 5.3 ms/step on 1.3B); every shape here is static so the whole
    step — embedding, all blocks over the full-length cache with an
    additive visibility mask, head, argmax fed back into the input buffer —
    replays as a single graph launch (measured 2.5 ms/step, and 2.0 ms
    single-stream with the decode GEMV kernels).  Host work per token:
    advance the position tensor, open one mask slot, replay.  The captured
    step is the model's own ``decode_forward`` with the position as the
    device tensor ``pos_t`` (RoPE and the cache write read it on the
    device; a host int would bake one position into the graph).

    ``attn_impl="hip"`` replaces the full-length masked SDPA with
    ops.decode_attention reading ``pos_t`` on the device: cost follows the
    valid length instead of the cache capacity, GQA caches are read
    un-expanded, and no mask is built or maintained.

    Greedy only (the argmax lives inside the graph).  Works for either
    model family (``GraphedGPT2Decoder`` and ``GraphedLlamaDecoder`` are
    this class); usage::

        dec = GraphedDecoder(model, batch=B, max_seq=T)
        out = dec.generate(prompt, max_new_tokens=n)
    """

    def __init__(self, model, batch: int, max_seq: int, warmup: int = 3,
                 attn_impl: Optional[str] = None):
        assert get_tp_size() == 1
        self.attn_impl = resolve_decode_attn_impl(attn_impl)
        assert torch.cuda.is_available()
        self.model = model
        assert max_seq <= model.cfg.max_seq
        p = next(model.parameters())
        dev, dtype = p.device, p.dtype
        self.max_seq = max_seq
        self.caches = _alloc_caches(model, batch, max_seq)
        self.in_tok = torch.zeros(batch, 1, dtype=torch.long, device=dev)
        self.pos_t = torch.zeros(1, dtype=torch.long, device=dev)
        self.pos = 0
        self.mask = None                # the hip path reads pos_t instead
        # capture with position 0 visible (an all-masked row would NaN);
        # the garbage this warmup writes into cache slot 0 is overwritten
        # by the first prefill()
        if self.attn_impl == "sdpa":
            self.mask = torch.full((1, 1, 1, max_seq), float("-inf"),
                                   dtype=dtype, device=dev)
            self.mask[..., :1] = 0
        self._graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step_static()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        with torch.cuda.graph(self._graph):
            self._step_static()

    @torch.no_grad()
    def _step_static(self):
        logits = decode_forward(self.model, self.in_tok, self.caches,
                                self.pos_t, attn_impl=self.attn_impl,
                                mask=self.mask)             # (B, V)
        self._logits = logits
        self.in_tok.copy_(logits.argmax(-1, keepdim=True))

    @torch.no_grad()
    def prefill(self, idx: torch.Tensor):
        """Run the prompt (B, S0) through the non-graph path into this
        decoder's caches and arm the first decode step."""
        B, S0 = idx.shape
        assert S0 < self.max_seq
        logits = decode_forward(self.model, idx, self.caches, 0,
                                attn_impl=self.attn_impl)
        self.pos = S0
        if self.mask is not None:
            self.mask.fill_(float("-inf"))
            self.mask[..., :S0 + 1] = 0
        self.pos_t.fill_(S0)
        self.in_tok.copy_(logits.argmax(-1, keepdim=True))

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """Emit one token per batch row: (B,) ids.  The returned token is
        the one the PREVIOUS forward predicted; this replay consumes it."""
        assert self.pos < self.max_seq, "decoder cache is full"
        tok = self.in_tok[:, 0].clone()
        self._graph.replay()
        self.pos += 1
        self.pos_t += 1
        if self.mask is not None and self.pos < self.max_seq:
            self.mask[..., self.pos] = 0
        return tok

    @torch.no_grad()
    def generate(self, idx: torch.Tensor,
                 max_new_tokens: int) -> torch.Tensor:
        assert idx.shape[1] + max_new_tokens <= self.max_seq
        self.prefill(idx)
        toks = [self.step() for _ in range(max_new_tokens)]
        return torch.cat([idx, torch.stack(toks, dim=1)], dim=1)


# the names README, docs, scripts and tests construct the decoder by
GraphedGPT2Decoder = GraphedLlamaDecoder = GraphedDecoder


@torch.no_grad()
def generate(model, idx: torch.Tensor, max_new_tokens: int,
             greedy: bool = True, temperature: float = 1.0,
             top_k: Optional[int] = None,
             attn_impl: Optional[str] = None) -> torch.Tensor:
    """Autoregressive generation with KV caches.

    Args:
        model: a GPT2Model or LlamaModel (tp=1).
        idx: prompt token ids (B, S0).
        max_new_tokens: number of tokens to append.
        attn_impl: decode attention, ``"sdpa"`` or ``"hip"``; ``None``
            reads ``TDPA_DECODE_ATTN`` (default sdpa).
    Returns (B, S0 + max_new_tokens) token ids.
    """
    assert get_tp_size() == 1, "generate() supports tp=1 (single device)"
    B, S0 = idx.shape
    total = S0 + max_new_tokens
    assert total <= model.cfg.max_seq, (total, model.cfg.max_seq)
    caches = _alloc_caches(model, B, total)

    tokens = idx
    chunk, pos0 = idx, 0
    for _ in range(max_new_tokens):
        logits = decode_forward(model, chunk, caches, pos0,
                                attn_impl=attn_impl)
        nxt = _sample(logits, greedy, temperature, top_k)
        tokens = torch.cat([tokens, nxt[:, None]], dim=1)
        pos0 += chunk.shape[1]
        chunk = nxt[:, None]
    return tokens


@torch.no_grad()
def speculative_generate(target, draft, idx: torch.Tensor,
                         max_new_tokens: int, k: int = 4,
                         attn_impl: Optional[str] = None) -> torch.Tensor:
    """Greedy speculative decoding: ``draft`` proposes ``k`` tokens per
    round, ``target`` verifies the whole chunk in ONE forward.  Output is
    EXACTLY the target's greedy generation — the draft only changes how
    many target forwards it takes (verified by the differential test).

    Cache bookkeeping: rejected proposals leave stale entries past the
    committed length in both caches; they are overwritten sequentially
    before any later position can attend to them, so a rollback is just a
    smaller next ``pos0``.  B=1 (speculative decode is per-request —
    batched rows would accept different lengths each round).
    """
    assert get_tp_size() == 1
    assert idx.shape[0] == 1, "speculative decode is per-request (B=1)"
    S0 = idx.shape[1]
    cap = S0 + max_new_tokens + k + 1
    assert cap <= target.cfg.max_seq and cap <= draft.cfg.max_seq
    t_caches = _alloc_caches(target, 1, cap)
    d_caches = _alloc_caches(draft, 1, cap)
    attn_impl = resolve_decode_attn_impl(attn_impl)
    lt = decode_forward(target, idx, t_caches, 0, attn_impl=attn_impl)
    decode_forward(draft, idx, d_caches, 0, attn_impl=attn_impl)
    tokens = torch.cat([idx, lt.argmax(-1)[:, None]], dim=1)
    produced = 1
    while produced < max_new_tokens:
        kk = min(k, max_new_tokens - produced)
        base = tokens.shape[1] - 1        # cache-valid length of both models
        # ---- draft proposes kk tokens after the last committed token
        props = []
        cur = tokens[:, -1:]
        for j in range(kk):
            dl = decode_forward(draft, cur, d_caches, base + j,
                                attn_impl=attn_impl)
            cur = dl.argmax(-1)[:, None]
            props.append(cur)
        # ---- target verifies [last_committed, props[:-1]] in one chunk
        chunk = torch.cat([tokens[:, -1:]] + props[:-1], dim=1)  # (1, kk)
        tl = decode_forward(target, chunk, t_caches, base, all_logits=True,
                            attn_impl=attn_impl)
        truth = tl.argmax(-1)             # (1, kk): token after each prefix
        a = 0
        while a < kk - 1 and bool(truth[0, a] == props[a][0, 0]):
            a += 1
        # accept props[0..a-1] (they matched) plus the target's token at a
        accepted = props[:a] + [truth[:, a:a + 1]]
        tokens = torch.cat([tokens] + accepted, dim=1)
        produced += a + 1
    return tokens[:, :S0 + max_new_tokens]
