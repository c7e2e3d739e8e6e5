"""FusedAdamW: flat multi-tensor AdamW on the in-tree HIP kernel.

Replaces the reference's stock torch.optim.Adam/AdamW
(/root/reference/torchdistpackage/ddp/zero_optim.py:265, examples) with an
MI355X-shaped update: per param-group, ALL state lives in single contiguous
fp32 flats (master weights, exp_avg, exp_avg_sq, grad buffer), so a step is

    1. one fused foreach-copy of grads into the fp32 grad flat (casts bf16)
    2. ONE adamw kernel pass over the whole flat (4 reads + 3 writes of HBM)
    3. one fused foreach-copy of updated master views back into the params

instead of ~6 kernels x #params.  Profiling of the v0 per-param variant showed
~1900 cast + ~1700 copy kernels per 4 steps dominating step time.

Known difference from stock torch: the optimizer keeps ONE global step count,
where torch.optim.AdamW counts per parameter.  A parameter whose grad first
appears at a late step (it was None until then) is therefore bias-corrected
with the global count, not with 1 as in torch: its first updates are smaller.
"""

from __future__ import annotations

from typing import List

import torch

from . import fused_adamw_


class _FlatGroup:
    CHUNK = 1 << 16  # must match MT_CHUNK in elementwise.hip

    def __init__(self, params: List[torch.Tensor]):
        self.params = params
        n = sum(p.numel() for p in params)
        dev = params[0].device
        dtypes = {p.dtype for p in params}
        self.uniform_dtype = params[0].dtype if len(dtypes) == 1 else None
        self.mt_ready = dev.type == "cuda" and self.uniform_dtype in (
            torch.bfloat16, torch.float32)
        # fp32 params on the multi-tensor path update IN PLACE: no master
        # copy (the ZeRO composition passes fp32 master VIEWS here — a
        # duplicate master + grad32 wasted +64 GB on Llama-8B)
        inplace_fp32 = self.mt_ready and self.uniform_dtype == torch.float32
        offs = []
        off = 0
        for p in params:
            offs.append(off)
            off += p.numel()
        self.offs = offs
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.master_views = []
        self.grad_views = []
        if not inplace_fp32:
            self.master = torch.empty(n, dtype=torch.float32, device=dev)
            for p, o in zip(params, offs):
                mv = self.master.narrow(0, o, p.numel()).view_as(p)
                mv.copy_(p.detach().to(torch.float32))
                self.master_views.append(mv)
        else:
            self.master = None
            self.master_views = [p for p in params]  # aliases
        if not self.mt_ready:
            self.grad32 = torch.empty(n, dtype=torch.float32, device=dev)
            for p, o in zip(params, offs):
                self.grad_views.append(
                    self.grad32.narrow(0, o, p.numel()).view_as(p))
        if self.mt_ready:
            cpid, coff = [], []
            for i, p in enumerate(params):
                for c0 in range(0, p.numel(), self.CHUNK):
                    cpid.append(i)
                    coff.append(c0)
            self.cpid = torch.tensor(cpid, dtype=torch.int32, device=dev)
            self.coff = torch.tensor(coff, dtype=torch.int64, device=dev)
            self.pptrs = torch.tensor([p.data_ptr() for p in params],
                                      dtype=torch.int64, device=dev)
            if inplace_fp32:
                self.mptrs = self.pptrs
            else:
                base = self.master.data_ptr()
                self.mptrs = torch.tensor(
                    [base + o * 4 for o in offs], dtype=torch.int64,
                    device=dev)
            self.moffs = torch.tensor(offs, dtype=torch.int64, device=dev)
            self.numels = torch.tensor([p.numel() for p in params],
                                       dtype=torch.int64, device=dev)


class FusedAdamW(torch.optim.Optimizer):
    """AdamW over flat per-group state, one HIP kernel pass per flat.

    hipGraph capture.  With params on a GPU the step count and every
    group's ``lr`` (and ``weight_decay``) live in device memory.  Each
    ``step()`` launches a one-block prelude kernel that advances the device
    count and writes the group's fp32 coefficients ``1-beta1``, ``1-beta2``,
    ``1-beta2^t``, ``lr/(1-beta1^t)`` and ``1-lr*wd`` (each formed in double,
    rounded once) for the update kernels to read.  The prelude is part of
    ``step()``, so a captured ``step()`` (``utils_graph.GraphedStep``) counts
    and bias-corrects correctly on every replay.

    ``group["lr"]`` / ``group["weight_decay"]`` are uploaded by an eager
    ``step()`` whenever they changed.  A captured ``step()`` records no such
    write (it would put the capture-time value back on every replay), so
    between replays call :meth:`sync_lr` after changing them.  ``betas`` and
    ``eps`` are kernel immediates: a captured graph keeps the values it was
    captured with, and changing them needs a new capture.
    """

    # Bf16ZeroOptimizer may attach a ``_tdpa_grad_override`` tensor to a
    # param instead of materializing a cast-copy into .grad: the
    # multi-tensor kernel reads grads by raw pointer with a dtype flag, so
    # the owner's bf16 reduced-bucket view feeds the fp32 master update
    # directly (saves ~48 GB/step of cast-copy traffic on Llama-8B).
    supports_grad_override = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.95),
                 eps: float = 1e-8, weight_decay: float = 0.01):
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._flats: List[_FlatGroup] = []
        self._step_host = 0      # the count while no flat is on a GPU
        self._dev = None         # device of the GPU flats, if any
        self._built = False

    def _build(self):
        for group in self.param_groups:
            # NOTE: no requires_grad filter — like stock torch optimizers.
            # (Bf16ZeroOptimizer rebinds groups to fp32 master VIEWS whose
            # requires_grad is False; their .grad is assigned manually.)
            ps = list(group["params"])
            # split by dtype so each flat stays multi-tensor-kernel eligible
            # (e.g. fp32 MoE router gates among bf16 params)
            by_dtype = {}
            for p in ps:
                by_dtype.setdefault(p.dtype, []).append(p)
            group["_flats"] = [_FlatGroup(v) for v in by_dtype.values()]
        devs = {fg.exp_avg.device for g in self.param_groups
                for fg in g["_flats"] if fg.exp_avg.device.type == "cuda"}
        if devs:
            assert len(devs) == 1, f"params on several GPUs: {devs}"
            self._dev = devs.pop()
            G = len(self.param_groups)
            self._step_dev = torch.full((1,), self._step_host,
                                        dtype=torch.int64, device=self._dev)
            self._hyp = torch.zeros(G, 4, dtype=torch.float64,
                                    device=self._dev)
            self._coef = torch.zeros(G, 5, dtype=torch.float32,
                                     device=self._dev)
            self._hyp_host = None
        self._built = True

    @property
    def _step(self) -> int:
        """Steps taken so far (reads the device counter: a sync)."""
        if self._dev is not None:
            return int(self._step_dev.item())
        return self._step_host

    def _set_step(self, step: int):
        if self._dev is not None:
            self._step_dev.fill_(int(step))
        else:
            self._step_host = int(step)

    def _host_hyp(self):
        return [[float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                 float(g["weight_decay"])] for g in self.param_groups]

    @torch.no_grad()
    def sync_lr(self):
        """Upload every group's ``lr`` and ``weight_decay`` to the device.
        Eager steps do this themselves; call it between replays of a
        captured ``step()`` after changing ``group["lr"]``.  Not to be
        called while capturing."""
        if not self._built:
            self._build()
        if self._dev is None:
            return
        host = self._host_hyp()
        self._hyp.copy_(torch.tensor(host, dtype=torch.float64))
        self._hyp_host = host

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._built:
            self._build()
        if self._dev is not None:
            from . import ext
            if self._host_hyp() != self._hyp_host:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(
                        "FusedAdamW: lr/betas/weight_decay changed since "
                        "the last eager step; call sync_lr() before "
                        "capturing step()")
                self.sync_lr()
            ext("fused_adamw").adamw_prelude(self._step_dev, self._hyp,
                                             self._coef)
        else:
            self._step_host += 1
        for gi, group in enumerate(self.param_groups):
            for fg in group.get("_flats", []):
                self._step_flat(group, fg, gi)
        return loss

    @torch.no_grad()
    def _step_flat(self, group, fg: _FlatGroup, gi: int):
        beta1, beta2 = group["betas"]
        grads = []
        for p in fg.params:
            g = getattr(p, "_tdpa_grad_override", None)
            grads.append(g if g is not None else p.grad)
        on_gpu = fg.exp_avg.device.type == "cuda"

        if fg.mt_ready:
            from . import ext
            # the kernel reads each grad by raw pointer as p.numel() dense
            # elements of ONE dtype per flat
            grad_dtype = None
            for p, g in zip(fg.params, grads):
                if g is None:
                    continue
                if g.numel() != p.numel() or not g.is_contiguous():
                    raise ValueError(
                        f"FusedAdamW: grad of shape {tuple(g.shape)}, "
                        f"strides {g.stride()} for a param of shape "
                        f"{tuple(p.shape)}: need a contiguous grad of "
                        f"{p.numel()} elements")
                if g.device != p.device:
                    raise ValueError(f"FusedAdamW: grad on {g.device}, "
                                     f"param on {p.device}")
                if grad_dtype is None:
                    grad_dtype = g.dtype
                    if grad_dtype not in (torch.bfloat16, torch.float32):
                        raise TypeError("FusedAdamW: grads must be bf16 or "
                                        f"fp32, got {grad_dtype}")
                elif g.dtype != grad_dtype:
                    raise TypeError(
                        f"FusedAdamW: grads of {grad_dtype} and {g.dtype} "
                        f"in one {fg.uniform_dtype} flat; the kernel reads "
                        "one grad dtype per flat")
            key = tuple(g.data_ptr() if g is not None else 0 for g in grads)
            if getattr(fg, "_gptr_key", None) != key:
                fg._gptr_key = key
                fg._gptr_dev = torch.tensor(
                    list(key), dtype=torch.int64).to(fg.exp_avg.device)
            gptrs = fg._gptr_dev
            if grad_dtype is None:
                grad_dtype = fg.uniform_dtype
            ext("multi_adamw").multi_adamw_step_dev(
                fg.cpid, fg.coff, fg.pptrs, gptrs, fg.mptrs, fg.moffs,
                fg.numels, fg.exp_avg, fg.exp_avg_sq, self._coef[gi],
                beta1, beta2, group["eps"],
                fg.uniform_dtype == torch.bfloat16,
                grad_dtype == torch.bfloat16)
        else:
            g32 = [g.to(p.dtype) if g is not None
                   else torch.zeros_like(p) for p, g in zip(fg.params, grads)]
            torch._foreach_copy_(fg.grad_views, g32)
            # grad-None params must be SKIPPED (stock torch semantics): save
            # their flat segments and restore after the whole-flat update
            saves = []
            for i, p in enumerate(fg.params):
                if grads[i] is None:
                    o, n = fg.offs[i], p.numel()
                    saves.append((o, n, fg.master[o:o + n].clone(),
                                  fg.exp_avg[o:o + n].clone(),
                                  fg.exp_avg_sq[o:o + n].clone()))
            if on_gpu:
                from . import ext
                ext("fused_adamw").adamw_step_dev(
                    fg.master, fg.grad32, fg.exp_avg, fg.exp_avg_sq,
                    self._coef[gi], beta1, beta2, group["eps"])
            else:
                fused_adamw_(fg.master, fg.grad32, fg.exp_avg,
                             fg.exp_avg_sq, self._step, group["lr"], beta1,
                             beta2, group["eps"], group["weight_decay"])
            for o, n, ms, es, vs in saves:
                fg.master[o:o + n].copy_(ms)
                fg.exp_avg[o:o + n].copy_(es)
                fg.exp_avg_sq[o:o + n].copy_(vs)
            torch._foreach_copy_(fg.params, fg.master_views)

    def zero_grad(self, set_to_none: bool = True):
        for group in self.param_groups:
            for p in group["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def state_dict(self):
        if not self._built:
            self._build()
        return {
            "step": self._step,
            "groups": [
                [{"master": fg.master, "exp_avg": fg.exp_avg,
                  "exp_avg_sq": fg.exp_avg_sq}
                 for fg in g.get("_flats", [])]
                for g in self.param_groups],  # master None => in-place fp32
        }

    @torch.no_grad()
    def load_state_dict(self, sd):
        if not self._built:
            self._build()
        self._set_step(sd["step"])
        for g, gsds in zip(self.param_groups, sd["groups"]):
            for fg, fsd in zip(g.get("_flats", []), gsds):
                if fg.master is not None and fsd["master"] is not None:
                    fg.master.copy_(fsd["master"])
                    torch._foreach_copy_(fg.params, fg.master_views)
                fg.exp_avg.copy_(fsd["exp_avg"])
                fg.exp_avg_sq.copy_(fsd["exp_avg_sq"])
