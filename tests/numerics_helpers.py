"""Input families, fp64 references and the error yardstick shared by
tests/test_ops_numerics.py (CPU paths) and tests/test_ops_numerics_gpu.py
(HIP kernels), the optimizer numerics files, and, from "Matmul family" on,
tests/test_matmul_numerics.py and tests/test_matmul_numerics_gpu.py, and, from
"training attention: exact inputs" on, tests/test_attention_numerics.py and
tests/test_attention_numerics_gpu.py.

Every generator is seeded and returns CPU tensors ALREADY ROUNDED to the
dtype under test, so the fp64 reference is computed from exactly the values
the kernel reads.  The yardstick compares the error of the code under test
against the error torch's own implementation makes in the same dtype on the
same values (the idiom of ``_gemm_yardstick`` in tests/test_ops_gpu.py).

Floors (the bound never drops below these), all derived or taken from the
existing suite:
- bf16 forward outputs   2**-8: one output ulp relative to the largest value
- bf16 gradients         2**-7: one ulp for the stored forward quantity plus
                                one for the gradient
- fp32 outputs/gradients 1e-5 : the fp32 tolerance of test_rmsnorm/layernorm
- saved mean / rstd      1e-5   relative
- CE loss 2e-3 absolute, lse / target logit 1e-3 absolute
  (test_fused_cross_entropy, test_ce_partial_fwd_kernel)
"""

import math

import torch
import torch.nn.functional as F

MARGIN = 2.5                 # the project's existing yardstick margin
TINY = 1e-30                 # only keeps an all-zero reference from dividing by 0

FLOOR_BF16_FWD = 2.0 ** -8
FLOOR_BF16_GRAD = 2.0 ** -7
FLOOR_FP32 = 1e-5
FLOOR_STATS = 1e-5
FLOOR_CE_LOSS = 2e-3         # absolute
FLOOR_LSE = 1e-3             # absolute (CE lse, CE target logit, attention lse)


def floors(dtype):
    """(forward floor, gradient floor) for outputs stored in ``dtype``."""
    if dtype == torch.bfloat16:
        return FLOOR_BF16_FWD, FLOOR_BF16_GRAD
    assert dtype == torch.float32
    return FLOOR_FP32, FLOOR_FP32


def dtype_name(dtype):
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dtype]


# --------------------------------------------------------------- yardstick

def _err(t, ref, absolute, tiny):
    d = (t.detach().double().cpu() - ref).abs().max().item()
    if absolute:
        return d
    return d / max(ref.abs().max().item(), tiny)


def yardstick(got, ref, lib, floor, *, absolute=False, tiny=TINY, what=""):
    """Assert e(got) <= max(2.5 * e(lib), floor) with
    e(t) = max|t - ref| / max(max|ref|, tiny)   (or max|t - ref| when
    ``absolute``).  ``ref`` is the fp64 result, ``lib`` torch's own result in
    the dtype under test.  Nothing is ever masked out: the reference and the
    result must be finite everywhere.  Returns (e_got, e_lib).

    ``tiny`` defaults to a value that only guards the division.  A caller
    passes a larger one for a quantity whose exact value is zero by
    cancellation (see ``attn_dq_cancel_scale``): there max|ref| is fp64
    rounding noise and the size of the cancelling terms is the only
    meaningful unit of error."""
    ref = ref.detach().double().cpu()
    assert ref.shape == got.shape == lib.shape, \
        f"{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(lib.shape)}"
    assert torch.isfinite(ref).all(), f"{what}: fp64 reference is not finite"
    assert torch.isfinite(got).all(), f"{what}: result is not finite"
    e_got = _err(got, ref, absolute, tiny)
    e_lib = _err(lib, ref, absolute, tiny)
    if not math.isfinite(e_lib):        # torch itself broke: no yardstick
        e_lib = math.inf
    bound = max(MARGIN * e_lib, floor)
    print(f"NUMERICS {what}: e_got={e_got:.3e} e_lib={e_lib:.3e} "
          f"bound={bound:.3e}")
    assert e_got <= bound, \
        f"{what}: e(got)={e_got:.3e} > max({MARGIN}*e(lib)={e_lib:.3e}, " \
        f"floor={floor:.3e})"
    return e_got, e_lib


def fwd_bwd(fn, tensors, dy, dtype, device):
    """Run ``fn(*tensors)`` and its backward with the tensors cast to
    (dtype, device).  Returns (y, [grads])."""
    ins = [t.detach().to(device=device, dtype=dtype).requires_grad_(True)
           for t in tensors]
    y = fn(*ins)
    y.backward(dy.detach().to(device=y.device, dtype=y.dtype))
    return y.detach(), [i.grad.detach() for i in ins]


def check_fwd_bwd(got_fn, lib_fn, ref_fn, tensors, dy, names, dtype, device,
                  lib_dtype, what, tiny=None):
    """Forward output and every gradient of ``got_fn`` (run in ``dtype`` on
    ``device``) against ``ref_fn`` in fp64 on the CPU, with ``lib_fn`` (run
    in ``lib_dtype`` on ``device``) as the yardstick.  ``tiny`` maps a
    gradient's name to the yardstick's ``tiny`` for it."""
    tiny = tiny or {}
    f_fwd, f_grad = floors(dtype)
    y, grads = fwd_bwd(got_fn, tensors, dy, dtype, device)
    y_ref, g_ref = fwd_bwd(ref_fn, tensors, dy, torch.float64, "cpu")
    y_lib, g_lib = fwd_bwd(lib_fn, tensors, dy, lib_dtype, device)
    assert y.dtype == dtype
    yardstick(y, y_ref, y_lib, f_fwd, what=f"{what} y")
    for n, g, gr, gl in zip(names, grads, g_ref, g_lib):
        assert g.dtype == dtype
        yardstick(g, gr, gl, f_grad, tiny=tiny.get(n, TINY),
                  what=f"{what} d{n}")


def _gen(*key):
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------- norms

NORM_SHAPES = [
    (3, 64),
    (5, 768),
    (2, 2056),      # NC = 2 with a partial chunk
    (2, 6144),      # NC = 3
    (2, 8192),      # NC = 4 edge
    (3, 1027),      # scalar kernels, D % 8 != 0
    (2050, 64),     # grid-stride: two blocks take two rows
]
BF16_V8_SHAPE = (2, 8200)   # bf16 above the register path: *_bwd_bf16v8


def norm_families(dtype):
    fams = ["randn", "shift30"]
    if dtype == torch.float32:
        fams.append("shift1000")
    fams += ["near_const", "outlier_first", "outlier_last", "zero_var",
             "tiny", "huge"]
    return fams


def norm_input(family, rows, D, dtype):
    """(x, w, b, dy) for a norm over the last dim, rounded to ``dtype``."""
    g = _gen("norm", family, rows, D, dtype)
    r = _randn((rows, D), g)
    if family == "randn":
        x = r
    elif family == "shift30":
        x = 30.0 + r
    elif family == "shift1000":
        x = 1000.0 + r
    elif family == "near_const":
        if dtype == torch.float32:
            x = 100.0 + 1e-3 * r
        else:
            # 3.0 with 1% of the entries one bf16 ulp (2**-6) higher
            up = torch.rand((rows, D), generator=g, dtype=torch.float64) < 0.01
            up[:, D // 3] = True
            x = 3.0 + up.double() * 2.0 ** -6
    elif family == "outlier_first":
        x = r
        x[:, 0] = 1000.0
    elif family == "outlier_last":
        x = r
        x[:, -1] = 1000.0
    elif family == "zero_var":
        x = r
        x[0] = 0.0
        x[1] = 7.0
    elif family == "tiny":
        x = 1e-4 * r
    elif family == "huge":
        x = 1e3 * r
    else:
        raise KeyError(family)
    w = _randn((D,), g)
    b = _randn((D,), g)
    dy = _randn((rows, D), g)
    return tuple(t.to(dtype) for t in (x, w, b, dy))


def layer_norm_stats_ref(x, eps):
    x64 = x.double()
    mean = x64.mean(-1)
    rstd = (x64.var(-1, unbiased=False) + eps).rsqrt()
    return mean, rstd


def layer_norm_stats_two_pass_fp32(x, eps):
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = (xf - mean).pow(2).mean(-1)
    return mean.squeeze(-1), torch.rsqrt(var + eps)


def rms_norm_formula(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def layer_norm_one_pass_fp32(x, w, b, eps):
    """The one-pass formula var = E[x^2] - E[x]^2 from fp32 sums, used for
    every row whatever its mean (the LayerNorm forward kernels once did;
    they now keep it only while mean^2 <= var).  Kept as the teeth check."""
    xf = x.float()
    D = xf.shape[-1]
    mu = xf.sum(-1, keepdim=True) / D
    var = (xf * xf).sum(-1, keepdim=True) / D - mu * mu
    return (xf - mu) * torch.rsqrt(var + eps) * w.float() + b.float()


# ------------------------------------------------------------- activations

ACT_FAMILIES = ["linspace", "saturate", "tiny", "randn3"]
_SATURATE = [20.0, -20.0, 100.0, -100.0, 1e4, -1e4]
_TINY = [0.0, -0.0, 1e-3, -1e-3, 1e-6, -1e-6]


def act_input(family, shape, dtype):
    """Pre-activation tensor of ``shape`` rounded to ``dtype``."""
    g = _gen("act", family, shape, dtype)
    n = math.prod(shape)
    if family == "linspace":
        vals = torch.linspace(-12.0, 12.0, 193, dtype=torch.float64)
    elif family == "saturate":
        vals = torch.tensor(_SATURATE, dtype=torch.float64)
    elif family == "tiny":
        vals = torch.tensor(_TINY, dtype=torch.float64)
    elif family == "randn3":
        return (3.0 * _randn(shape, g)).to(dtype)
    else:
        raise KeyError(family)
    x = vals[torch.arange(n) % vals.numel()].reshape(shape)
    return x.to(dtype)


def act_other(tag, shape, dtype):
    """randn operand (dy, the gate's other input, a bias)."""
    return _randn(shape, _gen("other", tag, shape, dtype)).to(dtype)


def act_bias(tag, shape, dtype):
    """randn bias with every other column 0, so that half the columns see
    the pre-activation family exactly."""
    b = _randn(shape, _gen("bias", tag, shape, dtype))
    b[..., ::2] = 0.0
    return b.to(dtype)


def gelu_tanh(u):
    return F.gelu(u, approximate="tanh")


# ----------------------------------------------------------- cross-entropy

CE_FAMILIES = ["randn3", "randn30", "shift1000", "neg_inf", "margin"]
CE_SHAPES = [(5, 8), (4, 1000), (3, 1003), (2, 4104)]


def ce_input(family, N, V):
    """(bf16 logits, int64 targets in range, bool mask of -inf entries)."""
    g = _gen("ce", family, N, V)
    r = _randn((N, V), g)
    t = torch.randint(0, V, (N,), generator=g)
    masked = torch.zeros(N, V, dtype=torch.bool)
    rows = torch.arange(N)
    if family == "randn3":
        x = (3.0 * r).bfloat16()
    elif family == "randn30":
        x = (30.0 * r).bfloat16()
    elif family == "shift1000":
        x = (1000.0 + 3.0 * r).bfloat16()
    elif family == "neg_inf":
        x = (3.0 * r).bfloat16()
        for row in range(N):
            perm = torch.randperm(V, generator=g)
            masked[row, perm[: V // 2]] = True
            t[row] = perm[V // 2 + int(t[row]) % (V - V // 2)]
        x[masked] = float("-inf")
    elif family == "margin":
        x = (3.0 * r).bfloat16()
        x[rows, t] = float("-inf")
        # multiples of 0.5 below 128 are bf16 values: the margin is >= 40
        top = torch.ceil((x.double().max(-1).values + 40.0) * 2.0) / 2.0
        assert top.max() < 128.0
        x[rows, t] = top.bfloat16()
        assert ((x.double()[rows, t][:, None] - x.double()) >= 40.0) \
            .sum() == N * (V - 1)
    else:
        raise KeyError(family)
    return x, t, masked


def ce_ref(x, t):
    """fp64 (mean loss, dlogits of the mean loss, per-row lse)."""
    x64 = x.double()
    N = x64.shape[0]
    lse = torch.logsumexp(x64, -1)
    tgt = x64.gather(-1, t.unsqueeze(-1)).squeeze(-1)
    loss = (lse - tgt).mean()
    p = torch.exp(x64 - lse.unsqueeze(-1))
    p[torch.arange(N), t] -= 1.0
    return loss, p / N, lse


# --------------------------------------------------------------- attention

ATTN_FAMILIES = ["randn", "peaky", "v_offset", "uniform", "dominant_key"]
ATTN_SHAPES = [            # (B, H, Hkv, S, D)
    (1, 2, 2, 192, 64),
    (1, 2, 2, 100, 128),
    (1, 4, 2, 192, 128),
]


def attn_input(family, B, H, Hkv, S, D):
    """(q, k, v, do) in bf16; q/do (B,H,S,D), k/v (B,Hkv,S,D)."""
    g = _gen("attn", family, B, H, Hkv, S, D)
    q = _randn((B, H, S, D), g)
    k = _randn((B, Hkv, S, D), g)
    v = _randn((B, Hkv, S, D), g)
    do = _randn((B, H, S, D), g)
    if family == "randn":
        pass
    elif family == "peaky":
        q, k = 4.0 * q, 4.0 * k
    elif family == "v_offset":
        v = 100.0 + v
    elif family == "uniform":
        k = k[:, :, :1].expand(B, Hkv, S, D).contiguous()
    elif family == "dominant_key":
        k[:, :, 0] *= 8.0
    else:
        raise KeyError(family)
    return tuple(t.bfloat16() for t in (q, k, v, do))


def _attn_scores(q, k, causal, scale):
    rep = q.shape[1] // k.shape[1]
    ke = k if rep == 1 else k.repeat_interleave(rep, 1)
    s = torch.matmul(q, ke.transpose(-1, -2))
    if s.dtype != torch.float64:
        s = s.float()
    s = s * scale
    if causal:
        S = q.shape[-2]
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).tril_()
        s = s.masked_fill(~mask, float("-inf"))
    return s


def attn_chain(q, k, v, causal, scale):
    """softmax((q @ k^T).float() * scale).to(dtype) @ v — the eager chain
    (fp64 stays fp64).  Differentiable."""
    rep = q.shape[1] // k.shape[1]
    ve = v if rep == 1 else v.repeat_interleave(rep, 1)
    s = _attn_scores(q, k, causal, scale)
    return torch.matmul(torch.softmax(s, -1).to(q.dtype), ve)


def attn_dq_cancel_scale(q, k, v, do, causal, scale):
    """Unit of error for dq when all keys are identical.

    dq_i = sum_j ds_ij k_j with ds_ij = p_ij (dp_ij - delta_i) * scale.  With
    k_j = k_0 for every j this is k_0 * sum_j ds_ij, and sum_j ds_ij = 0
    identically, so the exact dq is 0 and the fp64 reference holds only its
    own rounding noise (~1e-16).  An error relative to that is noise over
    noise.  What a kernel can be held to is the size of the terms that
    cancel: max_i sum_j |ds_ij| * max|k|, computed here in fp64."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    rep = q.shape[1] // k.shape[1]
    ve = v if rep == 1 else v.repeat_interleave(rep, 1)
    p = torch.softmax(_attn_scores(q, k, causal, scale), -1)
    dp = torch.matmul(do, ve.transpose(-1, -2))
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    return (ds.abs().sum(-1).max() * k.abs().max()).item()


def attn_lse(q, k, causal, scale):
    return torch.logsumexp(_attn_scores(q, k, causal, scale), -1)


# --------------------------------------------------------------- optimizer
#
# One AdamW step is judged element by element, each output against the size
# of the terms that can cancel in it (the idea of ``attn_dq_cancel_scale``):
#   e_m = max |m' - ref| / (|b1*m| + |(1-b1)*g| + TINY)
#   e_v = max |v' - ref| / (ref + TINY)
#   e_p = max |p' - ref| / (|p*(1-lr*wd)|
#                           + lr/bc1 * (|b1*m| + |(1-b1)*g|)
#                             / (sqrt(v'_ref/bc2) + eps) + TINY)
# and held to e(kernel) <= max(2.5 * e(lib), FLOOR_OPT) where lib is
# torch.optim.AdamW(foreach=False) in fp32 on the same device.
# FLOOR_OPT = 2**-21 is 4 fp32 ulp (ulp = 2**-23): m' = b1*m + (1-b1)*g
# rounds two products and one sum (3 roundings of at most half an ulp of the
# terms), the coefficients b1 / 1-b1 are each rounded once (half an ulp of
# their term), and v' and p' repeat the pattern with one more division and
# square root; 4 ulp covers the recurrence plus the coefficient rounding
# without leaving room for a coefficient formed in fp32 (1.f - 0.999f is
# 1.3e-5 off, 27 times the floor).

OPT_FAMILIES = ["randn", "small_p", "eps_scale", "tiny_grad", "big_grad",
                "wide", "zero_grad"]
OPT_STEPS = [1, 2, 10, 1000]
OPT_BETAS = [(0.9, 0.95), (0.9, 0.999)]
OPT_HYPER = dict(lr=1e-3, eps=1e-8, weight_decay=0.1)
FLOOR_OPT = 2.0 ** -21


def opt_input(family, n, step, betas, dtype=torch.float32):
    """fp32 CPU (p, g, m, v) entering AdamW step ``step``.  ``dtype`` bf16
    rounds p and g to bf16 (m and v are fp32 state whatever the params are).

    The moments are the stationary ones for iid gradients of scale s after
    step-1 steps: m = randn*s*sqrt((1-b1)/(1+b1))*(1-b1^(t-1)),
    v = s^2*(1-b2^(t-1))*U(0.5, 1.5); both 0 for step 1."""
    gen = _gen("opt", family, n, step, betas, dtype)
    b1, b2 = betas
    p = _randn((n,), gen)
    r = _randn((n,), gen)
    s = torch.ones(n, dtype=torch.float64)        # gradient scale
    if family == "randn":
        g = r
    elif family == "small_p":                     # the update dominates
        p = 1e-4 * p
        g = r
    elif family == "eps_scale":                   # sqrt(v) ~ eps
        s = s * 1e-8
        g = r * s
    elif family == "tiny_grad":
        s = s * 1e-12
        g = r * s
    elif family == "big_grad":
        s = s * 1e12
        g = r * s
    elif family == "wide":                        # |g| log-uniform 1e-10..1e6
        u = torch.rand(n, generator=gen, dtype=torch.float64)
        s = 10.0 ** (u * 16.0 - 10.0)
        g = torch.sign(r) * s
    elif family == "zero_grad":                   # pure decay, never NaN
        g = torch.zeros(n, dtype=torch.float64)
    else:
        raise KeyError(family)
    t = step - 1
    m = _randn((n,), gen) * s * math.sqrt((1 - b1) / (1 + b1)) * (1 - b1 ** t)
    v = s * s * (1 - b2 ** t) * \
        (0.5 + torch.rand(n, generator=gen, dtype=torch.float64))
    if family == "zero_grad":
        m[::2] = 0.0
        v[::2] = 0.0
    p, g = p.to(dtype).float(), g.to(dtype).float()
    return p, g, m.float(), v.float()


def adamw_ref(p, g, m, v, step, lr, betas, eps, weight_decay):
    """One AdamW step in fp64 with the user's double hyper-parameters.
    Returns (p', m', v')."""
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    b1, b2 = betas
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    p2 = p * (1 - lr * weight_decay) \
        - lr / bc1 * m2 / ((v2 / bc2).sqrt() + eps)
    return p2, m2, v2


def adamw_lib(p, g, m, v, step, lr, betas, eps, weight_decay, device="cpu"):
    """The same step by torch.optim.AdamW(foreach=False) in fp32 on
    ``device``, its state preloaded with step-1, m and v."""
    pp = torch.nn.Parameter(p.detach().float().to(device).clone())
    pp.grad = g.detach().float().to(device).clone()
    opt = torch.optim.AdamW([pp], lr=lr, betas=betas, eps=eps,
                            weight_decay=weight_decay, foreach=False)
    opt.state[pp] = {"step": torch.tensor(float(step - 1)),
                     "exp_avg": m.detach().float().to(device).clone(),
                     "exp_avg_sq": v.detach().float().to(device).clone()}
    opt.step()
    st = opt.state[pp]
    assert int(st["step"]) == step
    return pp.detach(), st["exp_avg"], st["exp_avg_sq"]


def optim_err(got, ins, step, lr, betas, eps, weight_decay, keep=None):
    """{"p","m","v"} -> element-wise error of got = (p', m', v') against
    ``adamw_ref`` of ins = (p, g, m, v), in the units described above.
    ``keep`` (bool mask) restricts the maximum to those elements."""
    p, g, m, v = (t.detach().double().cpu() for t in ins)
    gp, gm, gv = (t.detach().double().cpu() for t in got)
    rp, rm, rv = adamw_ref(p, g, m, v, step, lr, betas, eps, weight_decay)
    b1, b2 = betas
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    mterms = (b1 * m).abs() + ((1 - b1) * g).abs()
    e = {
        "m": (gm - rm).abs() / (mterms + TINY),
        "v": (gv - rv).abs() / (rv + TINY),
        "p": (gp - rp).abs() / ((p * (1 - lr * weight_decay)).abs()
                                + lr / bc1 * mterms
                                / ((rv / bc2).sqrt() + eps) + TINY),
    }
    out = {}
    for k, t in e.items():
        if keep is not None:
            t = t[keep]
        assert not torch.isnan(t).any(), f"{k}: NaN in a result"
        out[k] = t.max().item() if t.numel() else 0.0
    return out


def optim_check(got, ins, step, hyper, betas, device, what, keep=None,
                floor=FLOOR_OPT, lib=None):
    """Assert e(got) <= max(2.5 * e(lib), floor) for p', m' and v'.
    Returns (e_got, e_lib) dicts."""
    if lib is None:
        lib = adamw_lib(*ins, step, hyper["lr"], betas, hyper["eps"],
                        hyper["weight_decay"], device=device)
    args = (step, hyper["lr"], betas, hyper["eps"], hyper["weight_decay"])
    e_got = optim_err(got, ins, *args, keep=keep)
    e_lib = optim_err(lib, ins, *args, keep=keep)
    bad = []
    for k in ("p", "m", "v"):
        bound = max(MARGIN * e_lib[k], floor)
        print(f"NUMERICS {what} {k}: e_got={e_got[k]:.3e} "
              f"e_lib={e_lib[k]:.3e} bound={bound:.3e}")
        if not e_got[k] <= bound:
            bad.append(f"{k}: e(got)={e_got[k]:.3e} > max({MARGIN}*"
                       f"e(lib)={e_lib[k]:.3e}, floor={floor:.3e})")
    assert not bad, f"{what}: " + "; ".join(bad)
    return e_got, e_lib


def adamw_emulate(p, g, m, v, step, lr, betas, eps, weight_decay,
                  coef="double", eps_inside=False):
    """The HIP kernels' arithmetic in fp32 torch ops on the CPU (no fused
    multiply-add).  coef="double": 1-b1, 1-b2, bc2, lr/bc1 and 1-lr*wd formed
    in double and rounded once, as the kernels do.  coef="fp32": formed in
    fp32 from the rounded betas, as they once did.  ``eps_inside`` puts eps
    under the square root (a wrong kernel, for the teeth check)."""
    f32 = torch.float32
    p, g, m, v = (t.detach().to(f32).clone() for t in (p, g, m, v))
    b1, b2 = betas
    T = lambda x: torch.tensor(x, dtype=f32)
    b1f, b2f, epsf = T(b1), T(b2), T(eps)
    if coef == "double":
        omb1, omb2 = T(1 - b1), T(1 - b2)
        bc2 = T(1 - b2 ** step)
        step_size = T(lr / (1 - b1 ** step))
        decay = T(1 - lr * weight_decay)
    else:
        assert coef == "fp32"
        one = T(1.0)
        omb1, omb2 = one - b1f, one - b2f
        bc1 = one - torch.pow(b1f, T(float(step)))
        bc2 = one - torch.pow(b2f, T(float(step)))
        step_size = T(lr) / bc1
        decay = one - T(lr) * T(weight_decay)
    m2 = m * b1f + g * omb1
    v2 = v * b2f + g * g * omb2
    if eps_inside:
        den = torch.sqrt(v2 / bc2 + epsf)
    else:
        den = torch.sqrt(v2 / bc2) + epsf
    p2 = p * decay - step_size * m2 / den
    return p2, m2, v2


# --------------------------------------------------------------------- EMA
#
# ema' = d*ema + (1-d)*p, each element against the terms that add up to it:
#   e = max |ema' - ref| / (|d*ema| + |(1-d)*p| + TINY)
# FLOOR_EMA = 2**-22 (2 fp32 ulp): d and 1-d are each rounded once (half an
# ulp of their term), the two products and the sum round once each.

FLOOR_EMA = 2.0 ** -22


def ema_err(got, ema, p, decay):
    ema, p = ema.detach().double().cpu(), p.detach().double().cpu()
    ref = decay * ema + (1 - decay) * p
    e = (got.detach().double().cpu() - ref).abs() / \
        ((decay * ema).abs() + ((1 - decay) * p).abs() + TINY)
    assert not torch.isnan(e).any()
    return e.max().item()


# --------------------------------------------------------------- l2norm_sq
#
# A sum of n non-negative terms: every rounding is relative to a partial sum
# that is at most the result, so the relative error is at most (number of
# roundings on the longest chain) * 2**-24.  The kernel's chain for the
# largest size tested (2048*256+13) is 1 (square) + 2 (per-thread serial)
# + 6 + 4 (wave, block) + 8 (per-thread partials) + 6 + 4 = 31 <= 64.

FLOOR_L2NORM = 64 * 2.0 ** -24


# ===========================================================================
# Matmul family: GEMM / GEMV / decode attention / RoPE
# (tests/test_matmul_numerics.py on the CPU, tests/test_matmul_numerics_gpu.py
# on the HIP kernels; docs/design/kernels.md "Matmul-family numerics")
# ===========================================================================

# ------------------------------------------------------ exact-integer family
#
# Operands are integers in [-4, 4] stored in bf16 and K <= 16384, so every
# product (<= 16) and every partial sum (<= 16 * 16384 = 2**18, plus a bias
# of at most 4) is an integer below 2**24: fp32 accumulation is exact in ANY
# order.  The only rounding is the final fp32 -> bf16, so the result must
# equal the fp64 product rounded once, bit for bit.

EXACT_MAX_K = 16384


def int_mat(tag, shape, lo=-4, hi=4):
    """Integers in [lo, hi] as bf16."""
    g = _gen("int", tag, shape, lo, hi)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)


def exact_mm_ref(A, B, bias=None):
    """(A (M,K) @ B (N,K)^T [+ bias]) in fp64, rounded once to bf16."""
    assert A.shape[1] == B.shape[1] <= EXACT_MAX_K
    r = A.double().cpu() @ B.double().cpu().t()
    if bias is not None:
        r = r + bias.double().cpu()
    return r.to(torch.bfloat16)


def check_equal(got, ref, what):
    """Bit equality of two tensors without NaN; reports the first
    mismatching index."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert got.dtype == ref.dtype, f"{what}: dtype {got.dtype} vs {ref.dtype}"
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    idx = tuple(bad.nonzero()[0].tolist())
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first "
        f"at {idx}: got {got[idx].item()!r}, want {ref[idx].item()!r}")


def gemm_operands(kind, A, B):
    """The two tensors a GEMM binding of ``kind`` takes for the logical
    product A (M,K) @ B (N,K)^T:
      fprop  x (M,K),  w (N,K)
      dgrad  dy (M,K), w (K,N)
      wgrad  dy (K,M), x (K,N)"""
    if kind == "fprop":
        return A, B
    if kind == "dgrad":
        return A, B.t().contiguous()
    assert kind == "wgrad"
    return A.t().contiguous(), B.t().contiguous()


# (tiles_m, tiles_n) -> what the 256x256 kernel does with the grid.  nwg is
# tiles_m * tiles_n (* splitk); xcd_remap branches on nwg % 8.
GEMM_GRIDS_FPROP = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 3), (3, 3), (4, 2)]
GEMM_GRIDS_DGRAD = [(1, 1), (3, 1), (2, 3)]
GEMM_GRIDS_WGRAD = [(1, 1), (3, 2), (4, 1)]
# nslot = K / 32 = 1..9: 1-3 a ring that never fills, 4-6 an empty main loop,
# 7-9 the first main-loop group (ns_main = (nslot - 3) & ~3 = 4)
GEMM_KS = [32, 64, 96, 128, 160, 224, 256, 288]


def gemm_grid_id(tm, tn, splitk=1):
    gsup = 4 if tm % 4 == 0 else (2 if tm % 2 == 0 else 1)
    return f"grid{tm}x{tn}-gsup{gsup}-nwgmod8_{(tm * tn * splitk) % 8}"


def gemm_k_id(K):
    ns = K // 32
    how = "ring_never_fills" if ns <= 3 else \
        ("empty_main_loop" if ns <= 6 else "first_main_group")
    return f"K{K}-nslot{ns}-{how}"


# gemv: (M, N, K).  MT arms 1, 2, 4 (M=3 padded), 8 (M=5 padded), 16 (M=9
# padded), 32 (M=17 padded).  The x tile is KT = 2048 for MT <= 16 and 1024
# for MT = 32, so 2048 / 2056 / 4104 (resp. 1024 / 1032) sit on and just past
# a tile edge; K = 8 and 16 leave most of the wave idle.  Odd N ends on the
# ``two == false`` wave, N = 1 is that wave alone, N = 1000 is many blocks.
GEMV_SHAPES = [
    (1, 1, 8), (1, 7, 2048), (1, 1000, 2056),
    (2, 9, 16), (2, 8, 2048), (2, 7, 4104),
    (3, 1, 2056), (3, 9, 2048), (4, 1000, 4104), (4, 2, 1024),
    (5, 7, 2048), (8, 9, 2056), (8, 1, 8), (8, 1000, 1032),
    (9, 7, 2056), (9, 8, 2048), (16, 9, 4104), (16, 1, 16),
    (17, 9, 1024), (17, 7, 1032), (32, 9, 1032), (32, 1, 1024),
    (32, 1000, 2056), (32, 2, 8),
]


def gemv_id(shape):
    M, N, K = shape
    mt = next(t for t in (1, 2, 4, 8, 16, 32) if M <= t)
    return f"M{M}-MT{mt}-N{N}{'-odd' if N % 2 else ''}-K{K}"


def selection_matrix(tag, M, K):
    """(A, idx): A (M, K) is 0/1 with A[i, idx[i]] = 1, idx a random map of
    the M rows onto distinct columns when M <= K (a row-permuted selection)."""
    g = _gen("sel", tag, M, K)
    idx = torch.randperm(K, generator=g)[:M] if M <= K else \
        torch.randint(0, K, (M,), generator=g)
    A = torch.zeros(M, K, dtype=torch.bfloat16)
    A[torch.arange(M), idx] = 1.0
    return A, idx


# --------------------------------------------------------- precision family
#
# Per-element error, so that an element that is small by cancellation is
# judged against the size of the terms that cancel in it:
#   e(t) = max_ij |t - ref|_ij / (2**-9 |ref|_ij + 2**-24 (|A| @ |B|^T)_ij)
# and e(kernel) <= max(2.5 * e(library), 1.0).  A correctly rounded bf16
# result has |t - ref| <= 2**-8 |ref| (8 significand bits), i.e. e <= 2, and
# the library measures 1.9-2.0 on every family, so 2.5 * e(library) is the
# active term and the floor of 1.0 never widens the bound.

MM_FAMILIES = ["randn", "shift", "cancel", "wide"]
FLOOR_MM = 1.0


def mm_input(family, M, N, K):
    """bf16 A (M,K), B (N,K)."""
    g = _gen("mm", family, M, N, K)
    A, B = _randn((M, K), g), _randn((N, K), g)
    if family == "randn":
        pass
    elif family == "shift":       # mean 8: sums are large, fp32 error shows
        A, B = 8.0 + A, 8.0 + B
    elif family == "cancel":      # columns in +- pairs: ref ~ 0, |A||B| large
        A, B = A.to(torch.bfloat16).double(), B.to(torch.bfloat16).double()
        A[:, 1::2] = -A[:, 0::2]
        B[:, 1::2] = B[:, 0::2] + 2.0 ** -5 * _randn((N, K // 2), g)
    elif family == "wide":        # per-row scales 2**-6 .. 2**6
        sa = 2.0 ** torch.randint(-6, 7, (M, 1), generator=g).double()
        sb = 2.0 ** torch.randint(-6, 7, (N, 1), generator=g).double()
        A, B = A * sa, B * sb
    else:
        raise KeyError(family)
    return A.to(torch.bfloat16), B.to(torch.bfloat16)


def mm_ref_mag(A, B, bias=None):
    """fp64 (A @ B^T [+ bias], |A| @ |B|^T [+ |bias|])."""
    A64, B64 = A.double().cpu(), B.double().cpu()
    ref = A64 @ B64.t()
    mag = A64.abs() @ B64.abs().t()
    if bias is not None:
        ref = ref + bias.double().cpu()
        mag = mag + bias.double().cpu().abs()
    return ref, mag


def mm_err(t, ref, mag):
    t = t.detach().double().cpu()
    assert t.shape == ref.shape
    assert torch.isfinite(t).all(), "result is not finite"
    return ((t - ref).abs() / (2.0 ** -9 * ref.abs() + 2.0 ** -24 * mag)) \
        .max().item()


def mm_check(got, lib, ref, mag, what):
    """Assert e(got) <= max(2.5 * e(lib), 1.0).  Returns (e_got, e_lib)."""
    e_got, e_lib = mm_err(got, ref, mag), mm_err(lib, ref, mag)
    bound = max(MARGIN * e_lib, FLOOR_MM)
    print(f"NUMERICS {what}: e_got={e_got:.3e} e_lib={e_lib:.3e} "
          f"bound={bound:.3e}")
    assert e_got <= bound, \
        f"{what}: e(got)={e_got:.3e} > max({MARGIN}*e(lib)={e_lib:.3e}, " \
        f"floor={FLOOR_MM})"
    return e_got, e_lib


# --------------------------------------------------- decode-attention needles
#
# q rows are +-1 Walsh patterns; the needle key of a row is 4 * its pattern,
# every other key is +-0.25 at random, v lies in [1, 2) and is distinct per
# key.  With scale 1/sqrt(D) the needle scores 4*sqrt(D) (32 at D = 64) and
# any other key at most sqrt(D)/4 in magnitude (2), the needle of another row
# exactly 0 (Walsh rows are orthogonal): a lead of >= 30 nats, > 43 bits.
# Over <= 4160 keys everything else weighs < 4160 * 2**-43 < 2**-30 of the
# result, far below half a bf16 ulp (2**-9), and v, being a bf16 number, sits
# at the centre of its rounding interval: the output row must be the needle's
# v row bit for bit.

NEEDLE_SMAX = [1, 40, 72, 200, 256]
# (Hq, Hkv, Sq): M = (Hq / Hkv) * Sq = 1, 2, 4, 6 (padded MT 8), 8, 16
NEEDLE_HEADS = [(2, 2, 1), (2, 2, 2), (8, 2, 1), (6, 2, 2), (8, 2, 2),
                (8, 2, 4)]


def _walsh(D):
    H = torch.ones(1, 1, dtype=torch.float64)
    while H.shape[0] < D:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    assert H.shape[0] == D
    return H


def needle_probe_positions(L):
    """Key positions probed in a cache of L visible keys: all of them up to
    72, otherwise both sides of every 64-chunk edge, both ends, and a stride
    of 7 in between."""
    if L <= 72:
        return list(range(L))
    pos = set(range(0, L, 7)) | {0, 1, L - 2, L - 1}
    for e in range(64, L + 1, 64):
        pos |= {e - 2, e - 1, e, e + 1}
    return sorted(p for p in pos if 0 <= p < L)


def needle_input(tag, D, Hq, Hkv, Sq, Smax, pos0, needles):
    """One needle per (batch row, kv head, pattern).

    ``pos0``: list of B ints, row i of batch b sees keys [0, pos0[b] + i].
    ``needles``: (B, P) int positions, distinct within a batch row; query row
    m = g * Sq + i of a kv head carries pattern m % P and must return the v
    row of key needles[b, m % P].

    Returns (q, k_base, v_base, want): q (B, Hq, Sq, D) bf16; the caches are
    ``k_base.narrow(2, 16, Smax)`` / ``v_base.narrow(2, 24, Smax)`` of
    NaN-margined allocations, NaN from key pos0[b] + Sq on; want
    (B, Hq, Sq, D) bf16."""
    g = _gen("needle", tag, D, Hq, Hkv, Sq, Smax)
    B = len(pos0)
    G = Hq // Hkv
    needles = torch.as_tensor(needles, dtype=torch.long).reshape(B, -1)
    P = needles.shape[1]
    W = _walsh(D)
    nan = float("nan")
    kb = torch.full((B, Hkv, Smax + 32, D), nan, dtype=torch.float64)
    vb = torch.full((B, Hkv, Smax + 48, D), nan, dtype=torch.float64)
    k, v = kb.narrow(2, 16, Smax), vb.narrow(2, 24, Smax)
    j = torch.arange(Smax)
    q = torch.empty(B, Hkv, G * Sq, D, dtype=torch.float64)
    want = torch.empty(B, Hkv, G * Sq, D, dtype=torch.float64)
    for b in range(B):
        L = pos0[b] + Sq
        assert 0 <= pos0[b] and L <= Smax
        assert len(set(needles[b].tolist())) == P
        kk = 0.25 * (torch.randint(0, 2, (Hkv, L, D), generator=g) * 2 - 1)
        vv = 1.0 + torch.randint(0, 128, (Hkv, L, D), generator=g) / 128.0
        vv[:, :, 0] = 1.0 + (j[:L] % 128) / 128.0          # distinct per key
        vv[:, :, 1] = 1.0 + (j[:L] // 128) / 128.0
        vv[:, :, 2] = 1.0 + torch.arange(Hkv)[:, None] / 128.0
        for h in range(Hkv):
            for p in range(P):
                n = int(needles[b, p])
                assert 0 <= n < L
                kk[h, n] = 4.0 * W[1 + (h * 16 + p) % (D - 1)]
            for m in range(G * Sq):
                p = m % P
                q[b, h, m] = W[1 + (h * 16 + p) % (D - 1)]
                want[b, h, m] = vv[h, int(needles[b, p])]
        k[b, :, :L] = kk
        v[b, :, :L] = vv
    bf = torch.bfloat16
    return (q.reshape(B, Hq, Sq, D).to(bf), kb.to(bf), vb.to(bf),
            want.reshape(B, Hq, Sq, D).to(bf))


def needle_views(kb, vb, Smax):
    kc, vc = kb.narrow(2, 16, Smax), vb.narrow(2, 24, Smax)
    return kc, vc


def needle_grid(Smax, Sq, M):
    """(pos0 list, needles (B, P)) for two calls on one cache size:
    'full'  every batch row has all Smax keys; row b's first needle sits on
            probe position b (the others are spread behind it)
    'ragged' batch row b is one probe length long and its first needle is its
            LAST visible-to-all key."""
    out = {}
    vis = Smax - Sq + 1                 # keys every query row sees
    P = min(M, vis)
    step = vis // P
    probes = needle_probe_positions(vis)
    out["full"] = ([Smax - Sq] * len(probes),
                   [[(b + p * step) % vis for p in range(P)] for b in probes])
    pos0, needles = [], []
    for n in probes:                    # n + 1 keys visible to every row
        Pn = min(M, n + 1)
        if Pn < P:
            continue                    # one P per call
        st = (n + 1) // P
        pos0.append(n)
        needles.append([(n - p * st) % (n + 1) for p in range(P)])
    out["ragged"] = (pos0, needles)
    return out


def check_needles(got, want, what):
    """Every output row must be its needle's v row, bit for bit."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    if torch.equal(got.contiguous(), want.contiguous()):
        return
    bad = ((got != want) | torch.isnan(got)).any(-1)
    idx = tuple(bad.nonzero()[0].tolist())
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} rows are not their "
        f"needle's v row, first (batch, head, row) = {idx}: got "
        f"{got[idx][:4].tolist()}..., want {want[idx][:4].tolist()}...")


def multi_needle_input(tag, D, Smax, positions, M=1):
    """B = 1, Hkv = 1, Hq = M, Sq = 1: every q row is the same pattern and
    the n = 2 or 4 keys at ``positions`` all carry 4 * pattern, so the output
    must be the exact mean of their v rows.  Their bf16 mantissas are made
    multiples of n, so the mean is a bf16 number.  Returns
    (q, k_base, v_base, want)."""
    n = len(positions)
    assert n in (2, 4) and len(set(positions)) == n
    q, kb, vb, _ = needle_input(tag, D, M, 1, 1, Smax, [Smax - 1],
                                [[positions[0]]])
    k, v = needle_views(kb, vb, Smax)
    q[:] = q[0, 0]
    step = 128.0 / n
    for i, pos in enumerate(positions):
        k[0, 0, pos] = k[0, 0, positions[0]]
        row = (v[0, 0, pos].double() * step).floor() / step
        row[3] = 1.0 + i * n / 128.0                     # distinct rows
        v[0, 0, pos] = row.to(v.dtype)
    mean = sum(v[0, 0, pos].double() for pos in positions) / n
    want = mean.to(torch.bfloat16)
    assert torch.equal(want.double(), mean)
    return q, kb, vb, want.expand(1, M, 1, D)


MULTI_NEEDLES = [      # (positions in a 256-key cache, what they pin)
    ((3, 12), "two waves of one split"),
    ((5, 37), "one lane group, two steps"),
    ((63, 64), "last key of a chunk and first key of the next"),
    ((63, 100), "two neighbouring splits"),
    ((10, 250), "first and last split"),
    ((3, 12, 20, 100), "three needles in one split, one in the next: "
                       "the merge must weigh by l"),
]


def causal_needle_input(tag, D, G, Sq, Smax, pos0, istar):
    """B = 1, Hkv = 1, Hq = G.  Group g's needle sits at key pos0 + istar[g]
    (distinct per group), so rows i >= istar[g] of group g must return its v
    row exactly and rows i < istar[g] do not see it.  Returns
    (q, k_base, v_base, want, exact) with exact a (1, G, Sq) bool mask."""
    assert len(istar) == G and len(set(istar)) == G and max(istar) < Sq
    q, kb, vb, _ = needle_input(tag, D, G, 1, Sq, Smax, [pos0], [[0]])
    k, v = needle_views(kb, vb, Smax)
    W = _walsh(D)
    k[0, 0, 0] = 0.25 * W[D - 1]          # undo needle_input's own needle
    want = torch.zeros(1, G, Sq, D, dtype=torch.bfloat16)
    exact = torch.zeros(1, G, Sq, dtype=torch.bool)
    for g_ in range(G):
        n = pos0 + istar[g_]
        q[0, g_] = W[1 + g_]
        k[0, 0, n] = 4.0 * W[1 + g_]
        want[0, g_] = v[0, 0, n]
        exact[0, g_, istar[g_]:] = True
    return q, kb, vb, want, exact


def decode_ref64(q, kc, vc, pos0, scale=None):
    """fp64 decode attention on the CPU (NaN tails allowed).  (B,Hq,Sq,D)."""
    B, Hq, Sq, D = q.shape
    Hkv, Smax = kc.shape[1], kc.shape[2]
    G = Hq // Hkv
    scale = scale or 1.0 / math.sqrt(D)
    out = torch.empty(B, Hkv, G * Sq, D, dtype=torch.float64)
    q64 = q.double().cpu().reshape(B, Hkv, G * Sq, D)
    for b in range(B):
        L = pos0[b] + Sq
        k = kc[b, :, :L].double().cpu()
        v = vc[b, :, :L].double().cpu()
        s = q64[b] @ k.transpose(-1, -2) * scale            # (Hkv, M, L)
        row = torch.arange(G * Sq) % Sq
        vis = torch.arange(L)[None, :] <= (pos0[b] + row[:, None])
        s = s.masked_fill(~vis, float("-inf"))
        out[b] = torch.softmax(s, -1) @ v
    return out.reshape(B, Hq, Sq, D)


# ---------------------------------------------------------------------- RoPE

ROPE_DIMS = [16, 64, 80, 128]
ROPE_FAMILIES = ["randn", "wide", "rotation"]


def rope_tables(rows, D, base=10000.0):
    """fp32 (rows, D/2) cos / sin with position- and d-dependent entries;
    row 0 is cos = 1, sin = 0."""
    inv = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.outer(torch.arange(rows, dtype=torch.float64), inv)
    return fr.cos().float(), fr.sin().float()


def rope_input(family, shape):
    """bf16 x of ``shape`` (..., D) and a dy of the same shape."""
    g = _gen("rope", family, shape)
    D = shape[-1]
    x = _randn(shape, g)
    if family == "randn":
        pass
    elif family == "wide":
        x = x * 2.0 ** torch.randint(-6, 7, shape[:-1] + (1,),
                                     generator=g).double()
    elif family == "rotation":    # every (x1, x2) pair is a unit vector
        phi = x[..., :D // 2] * math.pi
        x = torch.cat([phi.cos(), phi.sin()], -1)
    else:
        raise KeyError(family)
    return x.to(torch.bfloat16), _randn(shape, g).to(torch.bfloat16)


def rope_formula(x, cos, sin, pos0):
    """Eager rotate-half over (..., S, D) in x's dtype with the table rows
    cast to it.  Differentiable."""
    S, hd = x.shape[-2], x.shape[-1]
    c = cos[pos0:pos0 + S].to(device=x.device, dtype=x.dtype)
    s = sin[pos0:pos0 + S].to(device=x.device, dtype=x.dtype)
    x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope_lib(x, cos, sin, pos0):
    """The yardstick: rotate-half in fp32, rounded once to x's dtype."""
    return rope_formula(x.float(), cos, sin, pos0).to(x.dtype)


def rope_all_bf16(x, cos, sin, pos0):
    """Tables and every product rounded to bf16 (the CPU fallback's formula
    before it moved to fp32).  Kept as the teeth check."""
    assert x.dtype == torch.bfloat16
    return rope_formula(x, cos, sin, pos0)


def rope_case(family, D, layout, B=2, H=3, S=5):
    """(x, dy, cos, sin, view): ``view(x)`` is the (B, H, S, D) tensor the op
    sees.  layout "contiguous", or "permuted": the Llama projection output
    (S, B, H*D) read in place as (B, H, S, D).  Tables have S + 8 rows."""
    cos, sin = rope_tables(S + 8, D)
    if layout == "contiguous":
        x, dy = rope_input(family, (B, H, S, D))
        return x, dy, cos, sin, lambda t: t
    assert layout == "permuted"
    x, _ = rope_input(family, (S, B, H * D))
    _, dy = rope_input(family, (B, H, S, D))
    return x, dy, cos, sin, \
        lambda t: t.view(S, B, H, D).permute(1, 2, 0, 3)


# ---------------------------------------- training attention: exact inputs
#
# The decode needle idea carried to the training kernels.  q rows are +-1
# Walsh patterns, the target key of a row is 4 * its pattern, every other key
# is +-0.25 at random, scale = 1/sqrt(D).  The target scores 4*sqrt(D), any
# random key at most sqrt(D)/4 in magnitude and the target of another pattern
# exactly 0, so the target leads by >= 4*sqrt(D) - sqrt(D)/4 nats (30 at
# D = 64, e**-30 < 1e-13).  Then
#   o    is the target's v row bit for bit (v is a bf16 number and everything
#        else weighs < 2**-30 of it),
#   dv   at a key is the sum of do over the rows that chose it.  do holds
#        integers in [-4, 4] and the sum is kept exactly representable in
#        bf16, so |dv - sum| <= 2**-24 (a sum that is exactly 0 still picks
#        up e**-30-sized terms, hence not bit-equal),
#   dS   at the target is P * (dP - delta) with dP = do . v_target and
#        delta = do . o = do . v_target: both are sums of multiples of 2**-7
#        below 2**11, exact in fp32 in any order, so dS is exactly 0 if the
#        kernel takes dP and delta from the same row; elsewhere P <= e**-30.
#        Hence |dq|, |dk| <= 2**-20 everywhere.
# The tie input gives each pattern two keys 4*W[1+p] +- 2*W[D/2+p] that both
# score exactly 4*sqrt(D): o must be (v_a + v_b) / 2 bit for bit (v on
# multiples of 2**-6, so the mean is a bf16 number), which pins the
# online-softmax rescale at equal maxima across two key tiles, and dq/dk are
# O(1) and checked per element against fp64 (``check_train_case``).

TRAIN_EDGE = 32              # targets sit on both sides of every multiple
TRAIN_TIE_GAP = 65           # distance between the two keys of a tie pair
BOUND_TRAIN_DV = 2.0 ** -24
BOUND_TRAIN_ZERO = 2.0 ** -20


def _train_candidates(S):
    pos = {0, 1, S - 2, S - 1}
    for e in range(TRAIN_EDGE, S, TRAIN_EDGE):
        pos |= {e - 1, e}
    return sorted(p for p in pos if 0 <= p < S)


def _train_base(g, B, H, Hkv, S, D, vstep):
    """Random +-0.25 keys, distinct v rows on multiples of 1/vstep in [1, 2),
    integer do in [-4, 4].  fp64."""
    k = 0.25 * (torch.randint(0, 2, (B, Hkv, S, D), generator=g) * 2.0 - 1.0)
    v = 1.0 + torch.randint(0, vstep, (B, Hkv, S, D), generator=g) / vstep
    j = torch.arange(S)
    v[:, :, :, 0] = 1.0 + (j % vstep) / vstep              # distinct per key
    v[:, :, :, 1] = 1.0 + (j // vstep) / vstep
    v[:, :, :, 2] = 1.0 + (torch.arange(Hkv)[:, None] % vstep) / vstep
    do = torch.randint(-4, 5, (B, H, S, D), generator=g).double()
    return k.double(), v.double(), do


def _pick(cands, count, cap):
    """Least-used candidate (ties: first); None if all are at the cap."""
    best = min(cands, key=lambda t: count[t])
    return best if count[best] < cap else None


def train_needle_input(tag, B, H, Hkv, S, D, causal):
    """One target key per query row.  Returns a dict with q, do (B,H,S,D),
    k, v (B,Hkv,S,D) in bf16, ``target`` (B,H,S) long, ``o_want`` bf16 and
    ``dv_want`` (B,Hkv,S,D) fp64, kind = "needle".

    Per (batch row, kv head) at most D-1 target keys: key 0 always, the rest
    on both sides of every multiple of 32 (hence 64) plus keys 1, S-2, S-1,
    the window rotated per (batch row, kv head) when there are more than fit.
    Rows are dealt to targets 32-row q-tile by q-tile: a row that is itself a
    target position takes it (the diagonal, which sits on both sides of every
    q-tile edge); then, from the last row of the tile backwards and rotating
    through the q-heads of the kv head, one row goes to each 32-key tile the
    mask allows and the tile has not reached yet (to its least-used target);
    every other row goes to the least-used target it can see.  A q-tile with
    at least as many free rows as key tiles therefore reaches every key tile
    it may see (asserted); a ragged last one reaches as many as it can.
    No target is chosen by more than 31 * rep rows of its kv head
    (rep = H / Hkv q-heads share it), asserted.  A cap of 31 per kv head,
    which would keep |sum of do| <= 124 < 256 by counting alone, cannot be
    met: under a causal mask rows 0..62 see only keys 0, 1, 31 and 32, which
    is 63 rows per q-head for 4 targets.  What such a cap is for, that the
    sum of do at every key is a bf16 number both per q-head (the kernel's
    partial) and after the GQA sum, is therefore asserted on the sums
    themselves (``_train_finish``)."""
    g = _gen("train_needle", tag, B, H, Hkv, S, D, causal)
    rep = H // Hkv
    W = _walsh(D)
    k, v, do = _train_base(g, B, H, Hkv, S, D, 128)
    q = torch.empty(B, H, S, D, dtype=torch.float64)
    target = torch.empty(B, H, S, dtype=torch.long)
    cand = _train_candidates(S)
    cap = 31 * rep
    T = TRAIN_EDGE
    for b in range(B):
        for hk in range(Hkv):
            if len(cand) > D - 1:
                rest = [c for c in cand if c != 0]
                r0 = ((b * Hkv + hk) * (D - 2)) % len(rest)
                rest = (rest + rest)[r0:r0 + D - 2]
                tg = [0] + sorted(rest)
            else:
                tg = cand
            pat = {t: 1 + n for n, t in enumerate(tg)}
            for t in tg:
                k[b, hk, t] = 4.0 * W[pat[t]]
            by_tile = {}
            for t in tg:
                by_tile.setdefault(t // T, []).append(t)
            count = {t: 0 for t in tg}
            covered = set()

            def assign(h, i, t):
                count[t] += 1
                covered.add((i // T, t // T))
                target[b, h, i] = t
                q[b, h, i] = W[pat[t]]

            for i0 in range(0, S, T):
                rows = range(i0, min(S, i0 + T))
                qt = i0 // T
                tiles = [kt for kt in sorted(by_tile)
                         if not causal or kt * T <= rows[-1]]
                slots = []
                for i in rows:
                    for gq in range(rep):
                        h = hk * rep + (gq + qt + b) % rep
                        if i in pat and count[i] < cap:     # the diagonal
                            assign(h, i, i)
                        else:
                            slots.append((h, i))
                duty = [kt for kt in tiles if (qt, kt) not in covered]
                for n, (h, i) in enumerate(slots[::-1]):
                    vis = [t for t in tg if not causal or t <= i]
                    t = None
                    if n < len(duty):
                        c = [x for x in by_tile[duty[n]] if x in vis]
                        t = _pick(c, count, cap) if c else None
                    if t is None:
                        t = _pick(vis, count, cap + 1)
                    assign(h, i, t)
                if len(slots) >= len(tiles):
                    for kt in tiles:
                        assert (qt, kt) in covered, (tag, qt, kt)
            assert max(count.values()) <= cap, (tag, max(count.values()), cap)
    return _train_finish("needle", q, k, v, do, target, None, rep)


def _tie_pairs(S, gap):
    """(a, a + gap) key pairs with all positions distinct: one starting at
    key 0, one ending on the last key, a = 1..3 and the last key of every
    32-key tile, whose
    partner is the first key of a tile two further on."""
    want = [0, S - 1 - gap, 1, 2, 3] + \
        list(range(TRAIN_EDGE - 1, S, TRAIN_EDGE))
    used, pairs = set(), []
    for a in want:
        if a < 0 or a + gap >= S or a in used or a + gap in used:
            continue
        used |= {a, a + gap}
        pairs.append((a, a + gap))
    return sorted(pairs)


def train_tie_input(tag, B, H, Hkv, S, D, causal):
    """Like ``train_needle_input``, but pattern p < D/2 - 1 has two keys
    4*W[1+p] +- 2*W[D/2+p], 65 keys apart (S // 2 when S < 130, so that short
    sequences have pairs at all), both scoring exactly 4*sqrt(D).  A row that
    sees both keys of its pair must return (v_a + v_b) / 2; a causal row
    that sees only the first key (which only happens before its partner, at
    the start of the sequence for the pair at key 0) is a single-needle row
    on that key.  ``target`` is (B,H,S,2) with -1 for an unseen partner."""
    g = _gen("train_tie", tag, B, H, Hkv, S, D, causal)
    rep = H // Hkv
    W = _walsh(D)
    k, v, do = _train_base(g, B, H, Hkv, S, D, 64)
    q = torch.empty(B, H, S, D, dtype=torch.float64)
    target = torch.full((B, H, S, 2), -1, dtype=torch.long)
    gap = TRAIN_TIE_GAP if S >= 2 * TRAIN_TIE_GAP else max(1, S // 2)
    allp = _tie_pairs(S, gap) if S > 1 else []
    npat = D // 2 - 1
    for b in range(B):
        for hk in range(Hkv):
            if len(allp) > npat:
                r0 = ((b * Hkv + hk) * npat) % len(allp)
                pairs = sorted((allp + allp)[r0:r0 + npat])
                if (0, gap) not in pairs:
                    pairs[0] = (0, gap)
            else:
                pairs = allp
            if not pairs:                  # S = 1: a single needle at key 0
                k[b, hk, 0] = 4.0 * W[1]
                q[b, hk * rep:(hk + 1) * rep] = W[1]
                target[b, hk * rep:(hk + 1) * rep, :, 0] = 0
                continue
            for p, (a, c) in enumerate(pairs):
                k[b, hk, a] = 4.0 * W[1 + p] + 2.0 * W[D // 2 + p]
                k[b, hk, c] = 4.0 * W[1 + p] - 2.0 * W[D // 2 + p]
            ends = {c: p for p, (a, c) in enumerate(pairs)}
            starts = {a: p for p, (a, c) in enumerate(pairs)}
            count = {p: 0 for p in range(len(pairs))}
            for gq in range(rep):
                h = hk * rep + gq
                for i in range(S):
                    both = [p for p, (a, c) in enumerate(pairs)
                            if not causal or c <= i]
                    if both:
                        p = ends[i] if i in ends else \
                            _pick(both[(i + gq) % len(both):] +
                                  both[:(i + gq) % len(both)], count, 1 << 30)
                        target[b, h, i, 1] = pairs[p][1]
                    else:
                        one = [p for p, (a, c) in enumerate(pairs) if a <= i]
                        assert one, "key 0 starts a pair"
                        p = starts[i] if i in starts else \
                            _pick(one, count, 1 << 30)
                    count[p] += 1
                    target[b, h, i, 0] = pairs[p][0]
                    q[b, h, i] = W[1 + p]
    return _train_finish("tie", q, k, v, do, target[..., 0], target[..., 1],
                         rep)


def _train_finish(kind, q, k, v, do, ta, tb, rep):
    B, H, S, D = q.shape
    Hkv = H // rep
    bf = torch.bfloat16
    for t in (q, k, v, do):
        assert torch.equal(t.to(bf).double(), t), "inputs are bf16 numbers"
    hk = (torch.arange(H) // rep)[None, :, None].expand(B, H, S)
    bb = torch.arange(B)[:, None, None].expand(B, H, S)
    o = v[bb, hk, ta]
    w = torch.ones(B, H, S, 1, dtype=torch.float64)
    if tb is not None:
        two = tb >= 0
        o = torch.where(two[..., None], (o + v[bb, hk, tb.clamp_min(0)]) / 2, o)
        w = torch.where(two[..., None], 0.5 * w, w)
    dvh = torch.zeros(B, H, S, D, dtype=torch.float64)     # per q-head
    hh = torch.arange(H)[None, :, None].expand(B, H, S)
    dvh.index_put_((bb, hh, ta), w * do, accumulate=True)
    if tb is not None:
        sel = tb >= 0
        dvh.index_put_((bb[sel], hh[sel], tb[sel]), (w * do)[sel],
                       accumulate=True)
    dv = dvh.view(B, Hkv, rep, S, D).sum(2)
    assert torch.equal(o.to(bf).double(), o), "expected o is a bf16 number"
    assert torch.equal(dvh.to(bf).double(), dvh), \
        "per-head sum of do is a bf16 number"
    assert torch.equal(dv.to(bf).double(), dv), "sum of do is a bf16 number"
    target = ta if tb is None else torch.stack([ta, tb], -1)
    return dict(kind=kind, q=q.to(bf), k=k.to(bf), v=v.to(bf), do=do.to(bf),
                target=target, o_want=o.to(bf), dv_want=dv)


def attn_ref64(q, k, v, do, causal, scale):
    """fp64 attention forward and backward on the CPU with the per-element
    magnitudes the tie check needs.  Returns a dict of o, lse, dq, dk, dv,
    mag_dq = |dS| @ |k| and mag_dk = |dS|^T @ |q| summed over the q-heads of
    a kv head."""
    q, k, v, do = (t.detach().double().cpu() for t in (q, k, v, do))
    B, H, S, D = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    ke = k.repeat_interleave(rep, 1)
    ve = v.repeat_interleave(rep, 1)
    s = _attn_scores(q, k, causal, scale)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ ve
    dp = do @ ve.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale

    def fold(t):
        return t.view(B, Hkv, rep, S, D).sum(2)

    return dict(o=o, lse=lse, dq=ds @ ke, dk=fold(ds.transpose(-1, -2) @ q),
                dv=fold(p.transpose(-1, -2) @ do),
                mag_dq=ds.abs() @ ke.abs(),
                mag_dk=fold(ds.abs().transpose(-1, -2) @ q.abs()))


def _worst(err, bound, what, fails):
    """Print the worst element of err against bound; append a message to
    ``fails`` if it exceeds it.  Returns max err."""
    err = err.detach().double().cpu()
    if not torch.isfinite(err).all():
        fails.append(f"{what}: result is not finite")
        return math.inf
    i = int((err - bound).argmax())
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i),
                                                    err.shape))
    e = float(err.flatten()[i])
    bd = float(bound.flatten()[i]) if torch.is_tensor(bound) else float(bound)
    print(f"NUMERICS {what}: max|err|={float(err.max()):.3e} "
          f"worst err/bound={e:.3e}/{bd:.3e} at {idx}")
    if not e <= bd:
        fails.append(f"{what}: |err|={e:.3e} > bound {bd:.3e} at {idx}")
    return float(err.max())


def check_train_case(got, case, causal, what, ref=None):
    """``got``: dict of o, dq, dk, dv (bf16) and lse (fp32) from the code
    under test on a ``train_needle_input`` / ``train_tie_input`` case.

    o: bit for bit.  lse: within FLOOR_LSE of fp64.  Needle: dv within 2**-24
    of the sum of do, |dq|, |dk| <= 2**-20.  Tie: dv within 2**-20 of fp64
    (which is a bf16 number up to e**-30 terms) and, per element,
    |dq - fp64| <= 2**-7 * mag + 2**-20 (same for dk) with mag the sum of the
    absolute values of the element's terms; 2**-7 = FLOOR_BF16_GRAD covers
    three bf16 roundings of 2**-9 each (the dS operand, the output, and the
    GQA partial sum or the dS workspace), the 2**-20 term the rows whose
    do . (v_a - v_b) is exactly 0, where mag is 1e-12 and only noise is left.

    Every quantity is checked before anything is raised, so one miss does
    not hide the others; the AssertionError names each as "<what> <name>:".
    Returns the worst dq and dk error over (mag + 2**-13) for a tie case."""
    D = case["q"].shape[-1]
    scale = 1.0 / math.sqrt(D)
    if ref is None:
        ref = attn_ref64(case["q"], case["k"], case["v"], case["do"], causal,
                         scale)
    fails = []
    for n in ("o", "dq", "dk", "dv"):
        assert got[n].dtype == torch.bfloat16, f"{what} {n}: {got[n].dtype}"
        assert got[n].shape == ref[n].shape, f"{what} {n}: {got[n].shape}"
    try:
        check_needles(got["o"], case["o_want"], what + " o")
    except AssertionError as e:
        fails.append(str(e))
    _worst((got["lse"].double().cpu() - ref["lse"]).abs(), FLOOR_LSE,
           what + " lse", fails)
    g = {n: got[n].detach().double().cpu() for n in ("dq", "dk", "dv")}
    out = None
    if case["kind"] == "needle":
        _worst((g["dv"] - case["dv_want"]).abs(), BOUND_TRAIN_DV,
               what + " dv", fails)
        _worst(g["dq"].abs(), BOUND_TRAIN_ZERO, what + " dq", fails)
        _worst(g["dk"].abs(), BOUND_TRAIN_ZERO, what + " dk", fails)
    else:
        _worst((g["dv"] - ref["dv"]).abs(), BOUND_TRAIN_ZERO, what + " dv",
               fails)
        out = []
        for n in ("dq", "dk"):
            err, mag = (g[n] - ref[n]).abs(), ref["mag_" + n]
            _worst(err, FLOOR_BF16_GRAD * mag + BOUND_TRAIN_ZERO,
                   f"{what} {n}", fails)
            out.append(float((err / (mag + 2.0 ** -13)).max()))
        out = tuple(out)
    assert not fails, "; ".join(fails)
    return out


def _saved_lse(t):
    """lse as saved by the attention autograd function that produced ``t``
    (every one of them saves it last), found through views and reshapes."""
    todo, seen = [t.grad_fn], set()
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if hasattr(n, "saved_tensors"):
            return n.saved_tensors[-1].detach()
        todo.extend(f for f, _ in n.next_functions)
    raise AssertionError("no attention function in the graph")


def run_attention(fn, case, device):
    """o, lse, dq, dk, dv of ``fn(q, k, v)`` -> (B,H,S,D) on a case's
    inputs (or on a (q, k, v, do) tuple)."""
    if not isinstance(case, dict):
        case = dict(zip(("q", "k", "v", "do"), case))
    q, k, v = (case[n].to(device).requires_grad_(True) for n in "qkv")
    o = fn(q, k, v)
    lse = _saved_lse(o)
    o.backward(case["do"].to(device))
    return dict(o=o.detach(), lse=lse, dq=q.grad, dk=k.grad, dv=v.grad)


def _sbh(t):
    """(B, H, S, D) -> contiguous (S, B, H*D)."""
    B, H, S, D = t.shape
    return t.permute(2, 0, 1, 3).reshape(S, B, H * D).contiguous()


def _bhsd(t, H):
    """(S, B, H*D) -> (B, H, S, D) view."""
    S, B, HD = t.shape
    return t.view(S, B, H, HD // H).permute(1, 2, 0, 3)


def run_fused_qkv(fn, case, device, causal):
    """The case through ``fn`` = ops.fused_qkv_attention: qkv is built as
    (S, B, 3*H*hd) from the case's q, k, v (H == Hkv), dqkv is split back.
    Also returns the raw ``dqkv`` (every element of which is a gradient)."""
    if not isinstance(case, dict):
        case = dict(zip(("q", "k", "v", "do"), case))
    H = case["q"].shape[1]
    assert case["k"].shape[1] == H
    qkv = torch.cat([_sbh(case[n]) for n in "qkv"], -1).to(device)
    qkv.requires_grad_(True)
    o = fn(qkv, H, causal=causal)
    lse = _saved_lse(o)
    o.backward(_sbh(case["do"]).to(device))
    dq, dk, dv = (_bhsd(g.contiguous(), H)
                  for g in qkv.grad.chunk(3, -1))
    return dict(o=_bhsd(o.detach(), H), lse=lse, dq=dq, dk=dk, dv=dv,
                dqkv=qkv.grad)


def run_gqa(fn, case, device, causal):
    """The case through ``fn`` = ops.gqa_attention with v a strided view of
    an (S, B, Hkv*hd) buffer, as the Llama block passes it."""
    if not isinstance(case, dict):
        case = dict(zip(("q", "k", "v", "do"), case))
    H, Hkv = case["q"].shape[1], case["k"].shape[1]
    q, k = (case[n].to(device).requires_grad_(True) for n in "qk")
    vbuf = _sbh(case["v"]).to(device).requires_grad_(True)
    o = fn(q, k, _bhsd(vbuf, Hkv), causal=causal)
    lse = _saved_lse(o)
    o.backward(_sbh(case["do"]).to(device))
    return dict(o=_bhsd(o.detach(), H), lse=lse, dq=q.grad, dk=k.grad,
                dv=_bhsd(vbuf.grad, Hkv))


def run_ring_blocks(case, nblk, device):
    """Causal ring attention's block math on one device: the sequence is cut
    into ``nblk`` blocks, query block r runs ring._fwd_partial against key
    blocks r (causal), r-1, ..., 0 (full) in ring order and merges them with
    ring._merge_partials, then ring._bwd_partial per block with the merged o
    and the global lse, accumulating in fp32 as _RingAttention does."""
    from torchdistpackage_amd.parallel.context import ring
    if not isinstance(case, dict):
        case = dict(zip(("q", "k", "v", "do"), case))
    q, k, v, do = (case[n].to(device) for n in ("q", "k", "v", "do"))
    B, H, S, D = q.shape
    assert k.shape[1] == H and S % nblk == 0
    L = S // nblk
    scale = 1.0 / math.sqrt(D)
    blk = lambda t, r: t[:, :, r * L:(r + 1) * L].contiguous()  # noqa: E731
    o, lse = torch.empty_like(q), torch.empty(B, H, S, device=device)
    dq = torch.empty_like(q)
    dk = torch.zeros(B, H, S, D, dtype=torch.float32, device=device)
    dv = torch.zeros_like(dk)
    with torch.no_grad():
        for r in range(nblk):
            qr, o_acc, lse_acc = blk(q, r), None, None
            for src in range(r, -1, -1):
                o_p, lse_p = ring._fwd_partial(qr, blk(k, src), blk(v, src),
                                               src == r, scale)
                if o_acc is None:
                    o_acc, lse_acc = o_p, lse_p
                else:
                    o_acc, lse_acc = ring._merge_partials(o_acc, lse_acc,
                                                          o_p, lse_p)
            o[:, :, r * L:(r + 1) * L] = o_acc
            lse[:, :, r * L:(r + 1) * L] = lse_acc
            dq_acc = torch.zeros_like(qr, dtype=torch.float32)
            for src in range(r, -1, -1):
                dq_p, dk_p, dv_p = ring._bwd_partial(
                    blk(do, r), qr, blk(k, src), blk(v, src), o_acc, lse_acc,
                    src == r, scale)
                dq_acc += dq_p.float()
                dk[:, :, src * L:(src + 1) * L] += dk_p.float()
                dv[:, :, src * L:(src + 1) * L] += dv_p.float()
            dq[:, :, r * L:(r + 1) * L] = dq_acc.to(q.dtype)
    return dict(o=o, lse=lse, dq=dq, dk=dk.to(q.dtype), dv=dv.to(q.dtype))


def rows_reaching_other_blocks(case, L):
    """Number of rows whose target (or either key of whose pair) lies in
    another block of L keys than the row itself."""
    t = case["target"]
    B, H, S = t.shape[:3]
    t = t.reshape(B, H, S, -1)
    own = (torch.arange(S) // L)[None, None, :, None]
    return int(((t >= 0) & (t // L != own)).any(-1).sum())


def attn_yardstick(got, tensors, causal, device, what, tiny=None):
    """o, dq, dk, dv of ``got`` against the fp64 eager chain with the bf16
    eager chain on ``device`` as the yardstick, exactly as check_fwd_bwd
    does for test_flash_attention.  Returns {name: (e_got, e_lib)}."""
    q, k, v, do = tensors
    scale = 1.0 / math.sqrt(q.shape[-1])
    fn = lambda q, k, v: attn_chain(q, k, v, causal, scale)  # noqa: E731
    y_ref, g_ref = fwd_bwd(fn, (q, k, v), do, torch.float64, "cpu")
    y_lib, g_lib = fwd_bwd(fn, (q, k, v), do, torch.bfloat16, device)
    tiny = tiny or {}
    out = {"o": yardstick(got["o"], y_ref, y_lib, FLOOR_BF16_FWD,
                          what=f"{what} y")}
    for n, gr, gl in zip("qkv", g_ref, g_lib):
        out["d" + n] = yardstick(got["d" + n], gr, gl, FLOOR_BF16_GRAD,
                                 tiny=tiny.get(n, TINY), what=f"{what} d{n}")
    return out


ATTN_SHAPES_TILED = [      # (B, H, Hkv, S, D): more than one tile everywhere
    (1, 2, 2, 300, 64),
    (1, 4, 1, 257, 64),
    (1, 2, 2, 300, 128),
    (2, 4, 2, 520, 128),
]
TRAIN_S = [33, 256, 257, 300, 520]
TRAIN_HEADS = [(1, 2, 2), (2, 4, 2), (1, 4, 1)]          # (B, H, Hkv)

# knobs of ops.attention_route per head-dim-128 route; head dim 64 has one
ATTN_ROUTES = {
    "default": {},
    "recompute": {"dq_recompute": True},
    "over_budget": {"max_ds_bytes": 0},
    "no_tr16": {"no_tr16": True},
    "pstore": {"pstore": True},
    "v1": {"force_v1": True},
}
