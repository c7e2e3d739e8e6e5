"""In-tree build of the gfx950 HIP extension.

Drives torch.utils.cpp_extension's hipcc path (``.hip`` sources compile with
hipcc directly — no hipify) and drops ``_tdpa_hip.*.so`` next to this file so
the built artifact travels with the repo snapshot to the GPU box.

Usage: ``python -m torchdistpackage_amd.ops.build`` or
``__graft_entry__.build()``.
"""

from __future__ import annotations

import os


HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")

SOURCES = [
    "bindings.cpp",
    "norms.hip",
    "elementwise.hip",
    "attention.hip",
    "attention_v2.hip",
    "cross_entropy.hip",
    "probe.hip",
    "gemm.hip",
    "rope_swiglu.hip",
    "gemv.hip",
    "gemv_int8.hip",
    "gemv_int4.hip",
    "decode_attn.hip",
    "decode_attn_fp8.hip",
    "kv_fp8.hip",
    "prefill_attn.hip",
    "chunk_attn.hip",
    "grouped_gemm.hip",
    "moe_route.hip",
    "sample.hip",
    "fused_decode.hip",
]

# A second module, ``_tdpa_nopk``: translation units built without
# packed-fp32 VALU forms.  It is a compiler flag for the whole unit (headers
# and device library included), which one module's sources cannot take one by
# one; a function attribute instead stops every header inline from inlining
# into the kernels (docs/design/kernels.md, "decode_attn_paged.hip").
NOPK_SOURCES = [
    "bindings_nopk.cpp",
    "decode_attn_paged.hip",
]
NOPK_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


def _build_module(name: str, sources, hip_flags, verbose: bool) -> str:
    from torch.utils.cpp_extension import load

    build_dir = os.path.join(HERE, "_build", name) if name != "_tdpa_hip" \
        else os.path.join(HERE, "_build")
    os.makedirs(build_dir, exist_ok=True)
    load(
        name=name,
        sources=[os.path.join(CSRC, s) for s in sources],
        extra_cflags=["-O3"],
        extra_cuda_cflags=["-O3", "--offload-arch=gfx950"] + hip_flags,
        build_directory=build_dir,
        verbose=verbose,
        is_python_module=False,  # just build; we load it ourselves
    )
    # copy the built .so next to this file (in-tree, snapshot-visible)
    import glob
    import shutil
    sos = glob.glob(os.path.join(build_dir, name + "*.so"))
    assert sos, f"no .so produced in {build_dir}"
    dest = os.path.join(HERE, os.path.basename(sos[0]))
    shutil.copy2(sos[0], dest)
    if verbose:
        print(f"[ops.build] built {dest}")
    return dest


def build(verbose: bool = True) -> str:
    os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
    os.environ.setdefault("MAX_JOBS", str(min(os.cpu_count() or 4, 16)))
    dest = _build_module("_tdpa_hip", SOURCES, [], verbose)
    _build_module("_tdpa_nopk", NOPK_SOURCES, NOPK_FLAGS, verbose)
    return dest


if __name__ == "__main__":
    build()
