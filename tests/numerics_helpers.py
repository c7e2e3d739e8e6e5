"""Input families, fp64 references and the error yardstick shared by
tests/test_ops_numerics.py (CPU paths) and tests/test_ops_numerics_gpu.py
(HIP kernels).

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
