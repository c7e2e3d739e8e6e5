"""The kernels that write the weights against fp64, on the GPU: AdamW (flat
and multi-tensor, eager and under hipGraph capture), EMA, the grad-norm
reduction, the in-place scale and gradient clipping.  Every element of every
output is compared.  Metrics, floors and input families are in
tests/numerics_helpers.py."""

import pytest
import torch

import numerics_helpers as H
import torchdistpackage_amd.ops as ops
from torchdistpackage_amd.ops.optim import FusedAdamW

pytestmark = pytest.mark.gpu

DEV = "cuda"
HY = H.OPT_HYPER
BF16, FP32 = torch.bfloat16, torch.float32
GRID_CAP = 2048 * 256          # elements one pass of the capped grid covers


def _args(step, betas):
    return (step, HY["lr"], betas, HY["eps"], HY["weight_decay"])


def _flat_step(ins, step, betas):
    p, g, m, v = (t.to(DEV) for t in ins)
    ops.fused_adamw_(p, g, m, v, step, HY["lr"], betas[0], betas[1],
                     HY["eps"], HY["weight_decay"])
    assert torch.equal(g.cpu().view(torch.int32),
                       ins[1].view(torch.int32)), "the grad must not be written"
    return p, m, v


# ------------------------------------------------------------- flat kernel

@pytest.mark.parametrize("betas", H.OPT_BETAS, ids=lambda b: f"b{b[1]}")
@pytest.mark.parametrize("step", H.OPT_STEPS)
@pytest.mark.parametrize("family", H.OPT_FAMILIES)
def test_adamw_flat(family, step, betas):
    ins = H.opt_input(family, 1031, step, betas)
    got = _flat_step(ins, step, betas)
    for t in got:
        assert torch.isfinite(t).all()
    H.optim_check(got, ins, step, HY, betas, DEV,
                  f"adamw flat {family} t={step} b2={betas[1]}")


def test_adamw_flat_grid_stride():
    step, betas = 10, (0.9, 0.999)
    ins = H.opt_input("randn", GRID_CAP + 7, step, betas)
    got = _flat_step(ins, step, betas)
    H.optim_check(got, ins, step, HY, betas, DEV, "adamw flat grid-stride")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_adamw_flat_nonfinite_grad(bad):
    step, betas, n, at = 10, (0.9, 0.999), 1031, 517
    ins = list(H.opt_input("randn", n, step, betas))
    ins[1] = ins[1].clone()
    ins[1][at] = bad
    got = _flat_step(ins, step, betas)
    lib = H.adamw_lib(*ins, *_args(step, betas), device=DEV)
    for t, want, name in zip(got, lib, "pmv"):
        assert torch.equal(torch.isfinite(t), torch.isfinite(want)), name
        assert not torch.isfinite(t[at]), name
    keep = torch.ones(n, dtype=torch.bool)
    keep[at] = False
    H.optim_check(got, ins, step, HY, betas, DEV, f"adamw flat grad={bad}",
                  keep=keep, lib=lib)


# ----------------------------------------------- multi-tensor (FusedAdamW)

# Flat offsets return to a multiple of 4 after every pair, so the params at
# even positions take the float4 arm (with tails of 1, 1, 2, 3 and 0
# elements and chunk ends at 65536, 65537 and 2*65536+5) and those at odd
# positions the scalar arm.  ``odd_first`` puts a 3-element param in front:
# every later m/v offset and master pointer moves by 3.
MT_NUMELS = [65536, 65537, 7, 2 * 65536 + 5, 3, 1030, 2, 1027, 1, 1024]
MT_NONE = 5                     # the param whose grad is None (the 1030)
MT_STEP, MT_BETAS = 10, (0.9, 0.999)


def _mt_setup(numels, pdtype, gdtype, layout, none_at):
    """params on the GPU with grads attached; returns (params, per-param
    fp32 CPU inputs)."""
    ins = [H.opt_input("randn", n, MT_STEP, MT_BETAS) for n in numels]
    # round to what the kernel reads; opt_input seeds by n, so roll to make
    # params of one size differ
    for i, (p, g, m, v) in enumerate(ins):
        ins[i] = tuple(x.roll(i) for x in (p.to(pdtype).float(),
                                           g.to(gdtype).float(), m, v))
    if layout == "flat_views":
        assert pdtype == FP32
        flat = torch.zeros(sum(numels) + 1, dtype=FP32, device=DEV)
        params, off = [], 1
        for n in numels:
            params.append(flat.narrow(0, off, n))
            off += n
    else:
        params = [torch.empty(n, dtype=pdtype, device=DEV) for n in numels]
    for p, t in zip(params, ins):
        p.copy_(t[0])
    for i, (p, t) in enumerate(zip(params, ins)):
        if i == none_at:
            continue
        g = t[1].to(device=DEV, dtype=gdtype)
        if gdtype == pdtype:
            p.grad = g
        else:
            p._tdpa_grad_override = g
    return params, ins


def _mt_preload(opt, ins_by_flat, step):
    sd = opt.state_dict()
    sd["step"] = step - 1
    flats = [fsd for g in sd["groups"] for fsd in g]
    assert len(flats) == len(ins_by_flat)
    for fsd, ins in zip(flats, ins_by_flat):
        fsd["exp_avg"] = torch.cat([t[2] for t in ins])
        fsd["exp_avg_sq"] = torch.cat([t[3] for t in ins])
    opt.load_state_dict(sd)


def _mt_check(fg, params, ins, none_at, hyper, what, step=MT_STEP,
              betas=MT_BETAS):
    """One flat after one step: master/m/v of every param against fp64,
    the grad-None param untouched, bf16 params == master.to(bf16)."""
    assert fg.mt_ready, "the multi-tensor kernel must be the path taken"
    if fg.master is not None:
        master = fg.master
    else:
        master = torch.cat([p.detach().reshape(-1) for p in params])
    cat = tuple(torch.cat([t[k] for t in ins]) for k in range(4))
    n = cat[0].numel()
    keep = torch.ones(n, dtype=torch.bool)
    if none_at is not None:
        o, k = fg.offs[none_at], ins[none_at][0].numel()
        keep[o:o + k] = False
        assert torch.equal(master[o:o + k].cpu(), ins[none_at][0]), \
            "grad-None param was modified"
        assert torch.equal(fg.exp_avg[o:o + k].cpu(), ins[none_at][2])
        assert torch.equal(fg.exp_avg_sq[o:o + k].cpu(), ins[none_at][3])
    for p, o in zip(params, fg.offs):
        want = master[o:o + p.numel()].to(p.dtype)
        assert torch.equal(p.detach().reshape(-1), want), \
            f"{what}: param != master.to({p.dtype})"
    H.optim_check((master, fg.exp_avg, fg.exp_avg_sq), cat, step, hyper,
                  betas, DEV, what, keep=keep)


# narrow() views of one flat at an odd offset are the fp32 (ZeRO) layout
MT_CASES = [(p, g, lay)
            for p, g in [(BF16, BF16), (BF16, FP32), (FP32, FP32),
                         (FP32, BF16)]
            for lay in ["separate", "odd_first", "flat_views"]
            if lay != "flat_views" or p == FP32]


@pytest.mark.parametrize(
    "pdtype,gdtype,layout", MT_CASES,
    ids=[f"{H.dtype_name(p)}-{H.dtype_name(g)}-{lay}"
         for p, g, lay in MT_CASES])
def test_adamw_multi_tensor(pdtype, gdtype, layout):
    numels = ([3] if layout == "odd_first" else []) + MT_NUMELS
    none_at = MT_NONE + (1 if layout == "odd_first" else 0)
    params, ins = _mt_setup(numels, pdtype, gdtype, layout, none_at)
    opt = FusedAdamW(params, lr=HY["lr"], betas=MT_BETAS, eps=HY["eps"],
                     weight_decay=HY["weight_decay"])
    _mt_preload(opt, [ins], MT_STEP)
    opt.step()
    assert opt.state_dict()["step"] == MT_STEP
    fg = opt.param_groups[0]["_flats"][0]
    assert (fg.master is None) == (pdtype == FP32)
    # the zero-moment check of a skipped param: preload put randn state
    # there, so "untouched" is the statement (checked in _mt_check)
    _mt_check(fg, params, ins, none_at, HY,
              f"multi adamw {pdtype}/{gdtype} {layout}")


def test_adamw_multi_tensor_none_grad_moments_stay_zero():
    params, ins = _mt_setup([1027, 1030, 65537], BF16, BF16, "separate", 1)
    opt = FusedAdamW(params, lr=HY["lr"], betas=MT_BETAS)
    before = params[1].detach().clone()
    for _ in range(3):
        opt.step()
    fg = opt.param_groups[0]["_flats"][0]
    o = fg.offs[1]
    assert torch.equal(params[1].detach(), before)
    assert (fg.exp_avg[o:o + 1030] == 0).all()
    assert (fg.exp_avg_sq[o:o + 1030] == 0).all()
    assert (fg.exp_avg[:o] != 0).any() and (fg.exp_avg[o + 1030:] != 0).any()


def test_adamw_mixed_dtype_group():
    """fp32 and bf16 params in ONE group: two flats, one coefficient row."""
    numels = [1027, 65537, 7, 1030]
    pb, ib = _mt_setup(numels, BF16, BF16, "separate", None)
    pf, if_ = _mt_setup([n + 4 for n in numels], FP32, FP32, "separate",
                        None)
    order = [pb[0], pf[0], pf[1], pb[1], pb[2], pf[2], pb[3], pf[3]]
    opt = FusedAdamW(order, lr=HY["lr"], betas=MT_BETAS, eps=HY["eps"],
                     weight_decay=HY["weight_decay"])
    _mt_preload(opt, [ib, if_], MT_STEP)
    opt.step()
    flats = opt.param_groups[0]["_flats"]
    assert [fg.uniform_dtype for fg in flats] == [BF16, FP32]
    _mt_check(flats[0], pb, ib, None, HY, "mixed group bf16 flat")
    _mt_check(flats[1], pf, if_, None, HY, "mixed group fp32 flat")


def test_adamw_two_groups():
    """Two groups with different lr and weight decay."""
    pa, ia = _mt_setup([1027, 65537], BF16, BF16, "separate", None)
    pb, ib = _mt_setup([1030, 7, 65536], BF16, BF16, "separate", None)
    hb = dict(HY, lr=3e-2, weight_decay=0.0)
    opt = FusedAdamW([{"params": pa},
                      {"params": pb, "lr": hb["lr"],
                       "weight_decay": hb["weight_decay"]}],
                     lr=HY["lr"], betas=MT_BETAS, eps=HY["eps"],
                     weight_decay=HY["weight_decay"])
    _mt_preload(opt, [ia, ib], MT_STEP)
    opt.step()
    _mt_check(opt.param_groups[0]["_flats"][0], pa, ia, None, HY,
              "two groups, first")
    _mt_check(opt.param_groups[1]["_flats"][0], pb, ib, None, hb,
              "two groups, second")


def _trajectory_ref(p0, grads, hyper, betas):
    """fp64 AdamW over the list of per-step grads; (p, m, v)."""
    p = p0.double()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        p, m, v = H.adamw_ref(p, g, m, v, t, hyper["lr"], betas,
                              hyper["eps"], hyper["weight_decay"])
    return p, m, v


def test_adamw_trajectory_20_steps():
    """20 eager steps against an fp64 trajectory, torch's fp32 AdamW as the
    yardstick.  Floor: 20 steps of at most FLOOR_OPT each."""
    n, steps, betas = 65537 + 1027, 20, (0.9, 0.999)
    gen = torch.Generator().manual_seed(20)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(steps)]
    params = [p0[:65537].clone().to(DEV), p0[65537:].clone().to(DEV)]
    lib_p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = FusedAdamW(params, betas=betas, **HY)
    lib = torch.optim.AdamW([lib_p], betas=betas, foreach=False, **HY)
    for g in grads:
        gd = g.to(DEV)
        params[0].grad, params[1].grad = gd[:65537].clone(), \
            gd[65537:].clone()
        lib_p.grad = gd
        opt.step()
        lib.step()
    rp, rm, rv = _trajectory_ref(p0, grads, HY, betas)
    fg = opt.param_groups[0]["_flats"][0]
    st = lib.state[lib_p]
    floor = steps * H.FLOOR_OPT
    H.yardstick(torch.cat(params), rp, lib_p.detach(), floor,
                what="trajectory p")
    H.yardstick(fg.exp_avg, rm, st["exp_avg"], floor, what="trajectory m")
    H.yardstick(fg.exp_avg_sq, rv, st["exp_avg_sq"], floor,
                what="trajectory v")


# ------------------------------------------------------------ graph capture

@pytest.mark.parametrize("pdtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_adamw_graphed_step_counts_and_follows_lr(pdtype):
    """GraphedStep(opt.step, warmup=3) + 7 replays is 10 steps: the bias
    corrections must advance on every replay, and an lr changed between
    replays (sync_lr) must take effect."""
    from torchdistpackage_amd.utils_graph import GraphedStep
    betas = (0.9, 0.95)
    numels = [1027, 65537, 7]
    gen = torch.Generator().manual_seed(31)
    p0 = [torch.randn(n, generator=gen).to(pdtype).float() for n in numels]
    g0 = [torch.randn(n, generator=gen).to(pdtype).float() for n in numels]

    def make():
        ps = [t.to(device=DEV, dtype=pdtype) for t in p0]
        for p, g in zip(ps, g0):
            p.grad = g.to(device=DEV, dtype=pdtype)
        return ps, FusedAdamW(ps, betas=betas, **HY)

    def state(ps, opt):
        fg = opt.param_groups[0]["_flats"][0]
        master = fg.master if fg.master is not None else torch.cat(ps)
        for p, o in zip(ps, fg.offs):
            assert torch.equal(p, master[o:o + p.numel()].to(pdtype))
        return master, fg.exp_avg, fg.exp_avg_sq

    ps_g, opt_g = make()
    ps_e, opt_e = make()
    gs = GraphedStep(opt_g.step, warmup=3)
    for _ in range(7):
        gs.replay()
    for _ in range(10):
        opt_e.step()
    torch.cuda.synchronize()
    assert opt_g.state_dict()["step"] == 10
    assert opt_e.state_dict()["step"] == 10

    grads = [torch.cat(g0)] * 10
    ref = _trajectory_ref(torch.cat(p0), grads, HY, betas)
    floor = 10 * H.FLOOR_OPT
    for got, lib, r, name in zip(state(ps_g, opt_g), state(ps_e, opt_e),
                                 ref, "pmv"):
        H.yardstick(got, r, lib, floor, what=f"graphed 10 steps {name}")

    # an lr schedule: 3 more steps at a third of the lr
    lr2 = HY["lr"] / 3
    opt_g.param_groups[0]["lr"] = lr2
    opt_g.sync_lr()
    opt_e.param_groups[0]["lr"] = lr2
    for _ in range(3):
        gs.replay()
        opt_e.step()
    torch.cuda.synchronize()
    assert opt_g.state_dict()["step"] == 13
    p, m, v = ref
    for t in range(11, 14):
        p, m, v = H.adamw_ref(p, grads[0], m, v, t, lr2, betas, HY["eps"],
                              HY["weight_decay"])
    floor = 13 * H.FLOOR_OPT
    for got, lib, r, name in zip(state(ps_g, opt_g), state(ps_e, opt_e),
                                 (p, m, v), "pmv"):
        H.yardstick(got, r, lib, floor, what=f"graphed lr change {name}")


# ---------------------------------------------------------------------- EMA

EMA_OFFSETS = [(0, 0), (1, 0), (0, 2), (3, 3), (2, 1)]   # (ema, param)
EMA_DECAYS = [0.0, 0.9, 0.9999, 1.0]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, GRID_CAP * 4 + 5])
@pytest.mark.parametrize("pdtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_ema_update(pdtype, n):
    gen = H._gen("ema", pdtype, n)
    ema0 = torch.randn(n + 3, generator=gen)
    ema0[::5] = 0.0                       # a fresh EMA: the param term alone
    p0 = torch.randn(n + 3, generator=gen).to(pdtype)
    p_dev = p0.to(DEV)
    # every offset with every decay; at the large size one decay per offset
    # (the arms taken depend on the offset alone)
    if n > 10000:
        combos = [(o, EMA_DECAYS[(i + 2) % 4])
                  for i, o in enumerate(EMA_OFFSETS)]
    else:
        combos = [(o, d) for o in EMA_OFFSETS for d in EMA_DECAYS]
    for (eo, po), decay in combos:
        buf = ema0.to(DEV)
        lib = ema0.to(DEV)
        ema, p = buf.narrow(0, eo, n), p_dev.narrow(0, po, n)
        ops.ema_update_(ema, p, decay)
        lib_v = lib.narrow(0, eo, n)
        lib_v.lerp_(p.float(), 1.0 - decay)
        what = f"ema {pdtype} n={n} off=({eo},{po}) d={decay}"
        # nothing outside the view is written
        outside = torch.ones(n + 3, dtype=torch.bool)
        outside[eo:eo + n] = False
        assert torch.equal(buf.cpu()[outside], ema0[outside]), what
        e_in, p_in = ema0[eo:eo + n], p0[po:po + n]
        e_got = H.ema_err(ema, e_in, p_in, decay)
        e_lib = H.ema_err(lib_v, e_in, p_in, decay)
        bound = max(H.MARGIN * e_lib, H.FLOOR_EMA)
        print(f"NUMERICS {what}: e_got={e_got:.3e} e_lib={e_lib:.3e} "
              f"bound={bound:.3e}")
        assert e_got <= bound, what
        if decay == 1.0:
            assert torch.equal(ema.cpu(), e_in), what
        if decay == 0.0:
            assert torch.equal(ema.cpu(), p_in.float()), what


def test_ema_update_strided_param():
    """A non-contiguous param is read through its strides."""
    n = 1027
    ema0 = torch.randn(n)
    pbuf = torch.randn(2 * n).to(DEV)
    ema = ema0.to(DEV)
    ops.ema_update_(ema, pbuf[::2], 0.9)
    e_got = H.ema_err(ema, ema0, pbuf[::2], 0.9)
    assert e_got <= H.FLOOR_EMA, e_got


# ---------------------------------------------------------------- l2norm_sq

def _l2_input(family, n, dtype):
    gen = H._gen("l2", family, n, dtype)
    r = torch.randn(n, generator=gen, dtype=torch.float64)
    if family == "randn":
        x = r
    elif family == "constant":
        x = torch.full((n,), 0.3, dtype=torch.float64)
    elif family == "spike":
        x = 1e-2 * r
        x[n // 2] = 1e4
    elif family == "wide":
        u = torch.rand(n, generator=gen, dtype=torch.float64)
        x = torch.sign(r) * 10.0 ** (u * 12.0 - 8.0)
    else:
        raise KeyError(family)
    return x.to(dtype)


@pytest.mark.parametrize("n", [1, 255, 257, 99991, GRID_CAP + 13])
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_l2norm_sq(dtype, n):
    for family in ("randn", "constant", "spike", "wide"):
        x = _l2_input(family, n, dtype)
        xd = x.to(DEV)
        got = ops.l2norm_sq(xd)
        assert got.dtype == FP32 and got.dim() == 0
        ref = x.double().pow(2).sum()
        lib = xd.float().pow(2).sum()
        H.yardstick(got.reshape(1), ref.reshape(1), lib.reshape(1),
                    H.FLOOR_L2NORM, what=f"l2norm_sq {dtype} n={n} {family}")
        for _ in range(4):
            again = ops.l2norm_sq(xd)
            assert torch.equal(again, got), \
                f"l2norm_sq {dtype} n={n} {family}: not bit-repeatable " \
                f"({again.item()!r} vs {got.item()!r})"
        assert torch.equal(xd.cpu(), x), "the input must not be written"


# ------------------------------------------------------------------- scale_

@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0, 0.0])
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_scale_inplace(dtype, s):
    n = GRID_CAP + 13
    x = H._randn((n,), H._gen("scale", dtype)).to(dtype)
    xd = x.to(DEV)
    want = (xd.float() * s).to(dtype)
    ops.scale_(xd, s)
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(xd.view(bits), want.view(bits))
    ref = x.double() * s
    floor = 2.0 ** -8 if dtype == BF16 else 2.0 ** -23
    H.yardstick(xd, ref, want, floor, what=f"scale_ {dtype} s={s}")


# ---------------------------------------------------------- clip_grad_norm_

@pytest.mark.parametrize("max_norm", [1.0, 1e6], ids=["clips", "leaves"])
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
def test_clip_grad_norm_single_gpu(dtype, max_norm):
    from torchdistpackage_amd.parallel.pipeline.grad_clip import \
        clip_grad_norm_
    gen = H._gen("clip", dtype)
    shapes = [(67, 129), (1027,), (3,), (300, 301)]
    gs = [H._randn(s, gen).to(dtype) for s in shapes]
    params = [torch.zeros(s, dtype=dtype, device=DEV) for s in shapes]
    for p, g in zip(params, gs):
        p.grad = g.to(DEV)
    # one non-contiguous grad: the transpose of a (129, 67) buffer
    params[0].grad = gs[0].t().contiguous().to(DEV).t()
    assert not params[0].grad.is_contiguous()
    frozen = torch.zeros(5, dtype=dtype, device=DEV)      # grad None
    norm = clip_grad_norm_(params + [frozen], max_norm, groups=[])
    ref_sq = sum(g.double().pow(2).sum() for g in gs)
    lib_sq = sum(g.to(DEV).float().pow(2).sum() for g in gs)
    H.yardstick(norm.reshape(1), ref_sq.sqrt().reshape(1),
                lib_sq.sqrt().reshape(1), H.FLOOR_L2NORM,
                what=f"clip norm {dtype}")
    scale = max_norm / (ref_sq.sqrt().item() + 1e-6)
    f_fwd, _ = H.floors(dtype)
    for p, g in zip(params, gs):
        if scale >= 1.0:
            assert torch.equal(p.grad.cpu(), g), "grads must be left alone"
            continue
        lib = (g.to(DEV).float() * scale).to(dtype)
        H.yardstick(p.grad, g.double() * scale, lib, f_fwd,
                    what=f"clipped grad {dtype} {tuple(g.shape)}")
    assert frozen.grad is None


# ------------------------------------------------------ host argument checks
# Every rejected input stays inside its own storage even if the kernel ran.

def test_adamw_step_rejects_bad_arguments():
    n = 1027
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    a = (1, 1e-3, 0.9, 0.95, 1e-8, 0.0)
    ops.fused_adamw_(p, g, m, v, *a)                       # the good call
    long_g = torch.zeros(n + 5, device=DEV)
    big = torch.zeros(2 * n, device=DEV)
    with pytest.raises(RuntimeError, match="elements"):
        ops.fused_adamw_(p, long_g, m, v, *a)
    with pytest.raises(RuntimeError, match="elements"):
        ops.fused_adamw_(p, g, long_g, v, *a)
    with pytest.raises(RuntimeError, match="elements"):
        ops.fused_adamw_(p, g, m, long_g, *a)
    for bad in range(1, 4):
        ts = [p, g, m, v]
        ts[bad] = big[::2]
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.fused_adamw_(*ts, *a)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.fused_adamw_(p, g.double(), m, v, *a)


def test_ema_update_rejects_bad_arguments():
    n = 1027
    e = ops.ext("ema_update")
    ema = torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError, match="elements"):
        e.ema_update(ema, torch.zeros(n + 5, device=DEV), 0.9)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.ema_update(ema, torch.zeros(2 * n, device=DEV)[::2], 0.9)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.ema_update(torch.zeros(2 * n, device=DEV)[::2],
                     torch.zeros(n, device=DEV), 0.9)
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        e.ema_update(ema, torch.zeros(n, device=DEV, dtype=torch.float64),
                     0.9)


def test_fused_adamw_rejects_bad_grads():
    n = 1030

    def fresh():
        ps = [torch.zeros(n, dtype=BF16, device=DEV) for _ in range(2)]
        for p in ps:
            p.grad = torch.zeros(n, dtype=BF16, device=DEV)
        return ps, FusedAdamW(ps)

    ps, opt = fresh()
    ps[1]._tdpa_grad_override = torch.zeros(2 * n, dtype=BF16,
                                            device=DEV)[::2]
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    ps, opt = fresh()
    ps[1]._tdpa_grad_override = torch.zeros(n + 2, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="contiguous grad of 1030"):
        opt.step()
    ps, opt = fresh()
    ps[1]._tdpa_grad_override = torch.zeros(n, dtype=FP32, device=DEV)
    with pytest.raises(TypeError, match="one grad dtype per flat"):
        opt.step()
