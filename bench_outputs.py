"""``bench.py --dump-outputs``: seeded sampling and .npy writing, shared by
the dp/tp path (bench.py) and the pipeline path (bench_pp.py)."""

from __future__ import annotations

import os

import numpy as np
import torch

# fixed seed and sizes so two builds pick the same elements (a whole job
# stays far below 64 MB even at 8 ranks)
DUMP_SEED = 20240
DUMP_PER_PARAM = 2048
DUMP_LOGITS = 1 << 18


def sample_params(params):
    """Seeded sample of every parameter, concatenated in parameter order."""
    g = torch.Generator(device="cpu").manual_seed(DUMP_SEED)
    parts = []
    for p in params:
        flat = p.detach().reshape(-1)
        if flat.numel() > DUMP_PER_PARAM:
            idx = torch.randint(0, flat.numel(), (DUMP_PER_PARAM,),
                                generator=g)
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    return torch.cat(parts)


def sample_logits(logits):
    """Seeded sample of a (B, S, V) logits tensor (indexed per dim, so a
    strided view is never materialized)."""
    logits = logits.detach()
    if logits.numel() <= DUMP_LOGITS:
        return logits.float().cpu()
    g = torch.Generator(device="cpu").manual_seed(DUMP_SEED + 1)
    idx = [torch.randint(0, n, (DUMP_LOGITS,), generator=g).to(logits.device)
           for n in logits.shape]
    return logits[tuple(idx)].float().cpu()


def dump_outputs(dirpath, outputs, rank, world):
    """Write each rank's arrays as float32 ``DIR/<name>.npy`` (``_rank<r>``
    suffix in multi-rank jobs)."""
    os.makedirs(dirpath, exist_ok=True)
    for name, t in outputs.items():
        fname = f"{name}.npy" if world == 1 else f"{name}_rank{rank}.npy"
        np.save(os.path.join(dirpath, fname),
                t.detach().float().cpu().numpy())
