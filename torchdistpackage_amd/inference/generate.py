"""KV-cache autoregressive generation for the model zoo (single-GPU serving).

The reference has no inference path at all (its ``forward_eval`` pipelines
full forwards, pipeline_sched.py:233-269); this module adds the serving-side
basics: prefill + incremental decode with per-layer K/V caches, greedy and
temperature / top-k / top-p sampling (``sampler="hip"``: ops.sample_logits,
one launch per step, also inside the graphed decoder).

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

import os
from typing import List, Optional, Tuple

import torch

from ..ops import (Fp8KV, PagedKV, resolve_decode_attn_impl,
                   sample_logits)
from ..parallel.tensor import get_tp_size


def resolve_kv_dtype(kv_dtype: Optional[str] = None) -> str:
    """``"bf16"`` (caches in the model's dtype, the default) or ``"fp8"``
    (ops.Fp8KV caches: e4m3 bytes and a power-of-two scale per row; needs
    ``attn_impl="hip"``).  ``None`` reads ``TDPA_KV_DTYPE``."""
    if kv_dtype is None:
        kv_dtype = os.environ.get("TDPA_KV_DTYPE", "bf16")
    if kv_dtype not in ("bf16", "fp8"):
        raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got "
                         f"{kv_dtype!r}")
    return kv_dtype


def resolve_kv_layout(kv_layout: Optional[str] = None,
                      page_size: Optional[int] = None) -> Tuple[str, int]:
    """``("contiguous" | "paged", page size)``.  ``"paged"`` keeps the
    caches as ops.PagedKV (pools of ``page_size`` positions behind one block
    table; needs ``attn_impl="hip"``).  ``None`` reads ``TDPA_KV_LAYOUT``
    (default contiguous) and ``TDPA_KV_PAGE`` (default 16)."""
    if kv_layout is None:
        kv_layout = os.environ.get("TDPA_KV_LAYOUT", "contiguous")
    if kv_layout not in ("contiguous", "paged"):
        raise ValueError(f"kv_layout must be 'contiguous' or 'paged', got "
                         f"{kv_layout!r}")
    if page_size is None:
        env = os.environ.get("TDPA_KV_PAGE", "16")
        page_size = int(env) if env.isdigit() else env
    # a contiguous cache has no pages: a stray value must not break it
    if kv_layout == "paged" and page_size not in (16, 32, 64, 128):
        raise ValueError("page_size must be a power of two in 16..128, got "
                         f"{page_size!r}")
    return kv_layout, page_size


def _alloc_caches(model, batch: int, max_seq: int,
                  kv_dtype: Optional[str] = None,
                  kv_layout: Optional[str] = None,
                  page_size: Optional[int] = None,
                  block_table: Optional[torch.Tensor] = None) -> List[Tuple]:
    """Zeroed per-layer (k, v) caches (B, n_kv, max_seq, hd) for ``model``,
    on its parameters' device: tensors of its dtype, with ``kv_dtype="fp8"``
    pairs of ops.Fp8KV, or with ``kv_layout="paged"`` pairs of ops.PagedKV.
    A paged model has ONE block table (``block_table``, default the
    identity), shared by every layer's K and V; each PagedKV has its own
    pool."""
    cfg = model.cfg
    p = next(model.parameters())
    shape = (batch, getattr(cfg, "n_kv_head", cfg.n_head), max_seq,
             cfg.dim // cfg.n_head)
    kv_layout, page_size = resolve_kv_layout(kv_layout, page_size)
    if kv_layout == "paged":
        if resolve_kv_dtype(kv_dtype) == "fp8":
            raise ValueError("kv_layout='paged' with kv_dtype='fp8': there "
                             "is no paged fp8 cache")
        if block_table is not None and block_table.device != p.device:
            raise ValueError(f"block_table on {block_table.device}, the "
                             f"model on {p.device}")
        first = PagedKV.zeros(*shape, page_size=page_size, dtype=p.dtype,
                              device=p.device, block_table=block_table)
        table = first.block_table

        def one():
            return PagedKV(torch.zeros_like(first.pool), table)
        return [(first if i == 0 else one(), one())
                for i in range(cfg.n_layer)]
    if block_table is not None:
        raise ValueError("block_table needs kv_layout='paged'")
    if resolve_kv_dtype(kv_dtype) == "fp8":
        return [(Fp8KV.zeros(*shape, device=p.device),
                 Fp8KV.zeros(*shape, device=p.device))
                for _ in range(cfg.n_layer)]
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


def resolve_sampler(sampler: Optional[str] = None) -> str:
    """``"torch"`` (``_sample``: topk, masked_fill, softmax, multinomial; no
    top-p) or ``"hip"`` (ops.sample_logits on uniform numbers drawn with
    ``torch.rand``).  ``None`` reads ``TDPA_SAMPLER`` (default torch)."""
    if sampler is None:
        sampler = os.environ.get("TDPA_SAMPLER", "torch")
    if sampler not in ("torch", "hip"):
        raise ValueError(f"sampler must be 'torch' or 'hip', got {sampler!r}")
    return sampler


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

    ``kv_dtype="fp8"`` (hip route only) keeps the caches as ops.Fp8KV; the
    quantising cache write is captured with the step.

    ``kv_layout="paged"`` (hip route only) keeps them as ops.PagedKV behind
    one block table (``self.caches[0][0].block_table``).  The captured step
    reads the table's contents on the device, so the host may rewrite them in
    place between replays.

    Greedy by default (the argmax lives inside the graph).  With any of
    ``temperature`` / ``top_k`` / ``top_p`` / ``seed`` set, the captured step
    ends in ops.sample_logits instead, writing the next token straight into
    the input buffer: the parameters are (B,) device tensors this decoder
    owns (``set_sampling`` rewrites them in place, no recapture) and the
    uniform numbers ``self.u`` are refilled from the decoder's own
    ``torch.Generator`` (seeded with ``seed``) before every replay, one small
    launch outside the graph.  ``top_k=1`` is greedy.  Works for either
    model family (``GraphedGPT2Decoder`` and ``GraphedLlamaDecoder`` are
    this class); usage::

        dec = GraphedDecoder(model, batch=B, max_seq=T)
        out = dec.generate(prompt, max_new_tokens=n)
    """

    def __init__(self, model, batch: int, max_seq: int, warmup: int = 3,
                 attn_impl: Optional[str] = None,
                 kv_dtype: Optional[str] = None,
                 kv_layout: Optional[str] = None,
                 page_size: Optional[int] = None,
                 temperature: Optional[float] = None,
                 top_k: Optional[int] = None,
                 top_p: Optional[float] = None,
                 seed: Optional[int] = None):
        assert get_tp_size() == 1
        self.attn_impl = resolve_decode_attn_impl(attn_impl)
        assert torch.cuda.is_available()
        self.model = model
        assert max_seq <= model.cfg.max_seq
        p = next(model.parameters())
        dev, dtype = p.device, p.dtype
        self.max_seq = max_seq
        self.caches = _alloc_caches(model, batch, max_seq, kv_dtype,
                                    kv_layout, page_size)
        self.in_tok = torch.zeros(batch, 1, dtype=torch.long, device=dev)
        self.pos_t = torch.zeros(1, dtype=torch.long, device=dev)
        self.pos = 0
        self.mask = None                # the hip path reads pos_t instead
        self.sampled = any(v is not None
                           for v in (temperature, top_k, top_p, seed))
        if self.sampled:
            self.u = torch.zeros(batch, dtype=torch.float32, device=dev)
            self.temperature = torch.ones(batch, dtype=torch.float32,
                                          device=dev)
            self.top_k = torch.zeros(batch, dtype=torch.int32, device=dev)
            self.top_p = torch.ones(batch, dtype=torch.float32, device=dev)
            self.set_sampling(temperature, top_k, top_p)
            self.generator = torch.Generator(device=dev)
            if seed is not None:
                self.generator.manual_seed(seed)
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
        self._next_token(logits)

    def _next_token(self, logits):
        if self.sampled:
            sample_logits(logits, self.u, self.temperature, self.top_k,
                          self.top_p, out=self.in_tok)
        else:
            self.in_tok.copy_(logits.argmax(-1, keepdim=True))

    def set_sampling(self, temperature: Optional[float] = None,
                     top_k: Optional[int] = None,
                     top_p: Optional[float] = None):
        """Rewrite the sampling parameters of a sampled decoder in place (a
        scalar, or a (B,) tensor for per-row values); None leaves one as it
        is.  The captured graph reads them on the device."""
        assert self.sampled, "this decoder was captured greedy"
        for buf, v in ((self.temperature, temperature), (self.top_k, top_k),
                       (self.top_p, top_p)):
            if isinstance(v, torch.Tensor):
                buf.copy_(v)
            elif v is not None:
                buf.fill_(v)

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
        if self.sampled:
            self.u.uniform_(generator=self.generator)
        self._next_token(logits)

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """Emit one token per batch row: (B,) ids.  The returned token is
        the one the PREVIOUS forward predicted; this replay consumes it."""
        assert self.pos < self.max_seq, "decoder cache is full"
        tok = self.in_tok[:, 0].clone()
        if self.sampled:
            self.u.uniform_(generator=self.generator)
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
             attn_impl: Optional[str] = None,
             kv_dtype: Optional[str] = None,
             kv_layout: Optional[str] = None,
             page_size: Optional[int] = None,
             top_p: Optional[float] = None,
             sampler: Optional[str] = None,
             generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Autoregressive generation with KV caches.

    Args:
        model: a GPT2Model or LlamaModel (tp=1).
        idx: prompt token ids (B, S0).
        max_new_tokens: number of tokens to append.
        attn_impl: decode attention, ``"sdpa"`` or ``"hip"``; ``None``
            reads ``TDPA_DECODE_ATTN`` (default sdpa).
        kv_dtype: KV cache format, ``"bf16"`` (the model's dtype) or
            ``"fp8"`` (needs ``attn_impl="hip"``); ``None`` reads
            ``TDPA_KV_DTYPE`` (default bf16).
        kv_layout: ``"contiguous"`` or ``"paged"`` (ops.PagedKV caches of
            ``page_size`` positions per page; needs ``attn_impl="hip"``);
            ``None`` reads ``TDPA_KV_LAYOUT`` and ``TDPA_KV_PAGE`` (default
            contiguous, 16).
        top_p: nucleus mass; needs ``sampler="hip"``.
        sampler: with ``greedy=False``, ``"torch"`` (``_sample``) or
            ``"hip"`` (ops.sample_logits on ``torch.rand(B,
            generator=generator)``); ``None`` reads ``TDPA_SAMPLER``
            (default torch).
        generator: the ``torch.Generator`` of the ``"hip"`` sampler's
            uniform numbers, on the logits' device (None: the default one).
    Returns (B, S0 + max_new_tokens) token ids.
    """
    sampler = resolve_sampler(sampler)
    if top_p is not None and sampler == "torch":
        raise ValueError("top_p needs sampler=\"hip\" (the torch sampler "
                         "has no nucleus step)")
    assert get_tp_size() == 1, "generate() supports tp=1 (single device)"
    B, S0 = idx.shape
    total = S0 + max_new_tokens
    assert total <= model.cfg.max_seq, (total, model.cfg.max_seq)
    caches = _alloc_caches(model, B, total, kv_dtype, kv_layout, page_size)

    tokens = idx
    chunk, pos0 = idx, 0
    for _ in range(max_new_tokens):
        logits = decode_forward(model, chunk, caches, pos0,
                                attn_impl=attn_impl)
        if greedy or sampler == "torch":
            nxt = _sample(logits, greedy, temperature, top_k)
        else:
            if logits.dtype not in (torch.bfloat16, torch.float32):
                logits = logits.float()
            u = torch.rand(B, generator=generator, device=logits.device)
            nxt = sample_logits(logits, u, temperature, top_k, top_p)
        tokens = torch.cat([tokens, nxt[:, None]], dim=1)
        pos0 += chunk.shape[1]
        chunk = nxt[:, None]
    return tokens


@torch.no_grad()
def speculative_generate(target, draft, idx: torch.Tensor,
                         max_new_tokens: int, k: int = 4,
                         attn_impl: Optional[str] = None,
                         kv_dtype: Optional[str] = None,
                         kv_layout: Optional[str] = None,
                         page_size: Optional[int] = None) -> torch.Tensor:
    """Greedy speculative decoding: ``draft`` proposes ``k`` tokens per
    round, ``target`` verifies the whole chunk in ONE forward.  Output is
    EXACTLY the target's greedy generation — the draft only changes how
    many target forwards it takes (verified by the differential test).

    Cache bookkeeping: rejected proposals leave stale entries past the
    committed length in both caches; they are overwritten sequentially
    before any later position can attend to them, so a rollback is just a
    smaller next ``pos0`` (with ``kv_dtype="fp8"`` too: a row's scale is
    overwritten with its bytes).  B=1 (speculative decode is per-request —
    batched rows would accept different lengths each round).
    """
    assert get_tp_size() == 1
    assert idx.shape[0] == 1, "speculative decode is per-request (B=1)"
    S0 = idx.shape[1]
    cap = S0 + max_new_tokens + k + 1
    assert cap <= target.cfg.max_seq and cap <= draft.cfg.max_seq
    t_caches = _alloc_caches(target, 1, cap, kv_dtype, kv_layout, page_size)
    d_caches = _alloc_caches(draft, 1, cap, kv_dtype, kv_layout, page_size)
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
