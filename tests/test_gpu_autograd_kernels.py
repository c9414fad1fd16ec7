"""The autograd-path kernels (tac_kernels.hip: tanh_gauss_fwd, tanh_gauss_bwd,
sac_q_loss_fwd, sac_pi_loss_fwd, polyak_, adam_step_) against the float64
references of kernel_refs.py, their autograd wrappers in ops/functional.py,
and the host gates of the bindings.  fp32 compute mode throughout.

algo/graph.py and the eager SAC.update_* run these on every visual training
run and every MLP run that does not take the engine.

Bounds (kernel_refs.tgh_fwd_bounds, tgh_bwd_bounds, qloss_ref, piloss_ref,
polyak_ref, adam_bounds) are first order and summed over the operations,
as the module docstring of test_gpu_heads_losses.py sets out: U = 2^-23 per
rounded fp32 operation, L_f = 4x the measured error of torch's own fp32 op
on this GPU (floor 2^-22) per libm call, rounding_bound() per reduction.
What is particular to these kernels:
  * the head is tg_ref's with hl = mu | log_std, so tg_fwd_bounds applies
    unchanged; deterministic means eps = 0 (prob = mu, a copy: exact) and
    ls_c is a clamp (exact);
  * the backward takes se = exp(ls_c) eps (one libm call, one rounding)
    and a vector seed dlogp[B], an input without error of its own;
  * the losses add one quotient per block atomically in any order:
    rounding_bound(B, .) holds for every order, the quotients are inside
    the U |loss| the references charge; a fractional done costs one more
    rounding of gamma (1 - done);
  * dlogp = alpha / B is one correctly rounded division: exact;
  * polyak: two products and a sum, U each; exact for rho in {0, 1};
  * Adam: kernel_refs.adam_bounds.
kernel_refs' clamp of (-5, 2) and the models' default (-20, 2) are both
run: at -20, std * eps falls below the spacing of mu, and a head that
rebuilds the noise as (prob - mu) / std loses it (logp off by eps^2 / 2
per element; test_kernel_refs.py shows the miss on the CPU).

Worst err / bound on an MI355X over all cases below: tanh_gauss_fwd pi
0.24, prob 0.50, logp 0.018; tanh_gauss_bwd dmu 0.41, dls 0.34;
sac_q_loss_fwd dq 0.42, loss 0.017; sac_pi_loss_fwd dq 0.00, loss 0.007;
adam_step_ p 0.31, m 0.49, v 0.48; polyak_ 0.45.  The measured L_f were 3.2e-7
for exp, 5.5e-7 for tanh and the floor 2^-22 for log1p."""

import pytest
import torch

import kernel_refs as kr
from test_gpu_heads_losses import _i64, _libm_tol, _ratio, _sent

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
AL = kr.TG_ACT_LIMIT
VARIANTS = [(False, True), (False, False), (True, True), (True, False)]


def _vid(v):
    return ("det" if v[0] else "sampled") + ("_logp" if v[1] else "_nologp")


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.ops import require_extension
    Fo.set_compute_dtype("fp32")
    return require_extension()


def _dev(*ts):
    return [t.to(DEV) for t in ts]


# -- tanh_gauss_fwd / tanh_gauss_bwd --------------------------------------------

_HEAD = {}


def _head(ext, case, clamp, det):
    """Inputs and one forward with logp per (case, clamp, det), shared by
    the forward and backward tests."""
    key = (case, clamp, det)
    if key not in _HEAD:
        mu, ls, eps = kr.tgh_inputs(*case, *clamp)
        pi, logp, prob, ls_c = ext.tanh_gauss_fwd(*_dev(mu, ls, eps), AL,
                                                  *clamp, det, True)
        torch.cuda.synchronize()
        _HEAD[key] = dict(mu=mu, ls=ls, eps=eps, pi=pi.cpu(), logp=logp.cpu(),
                          prob=prob.cpu(), ls_c=ls_c.cpu())
    return _HEAD[key]


def _head_tol(h, clamp):
    x = (-2 * h["prob"].double()).clamp_max(20.0).float()
    ls_c = h["ls"].clamp(*clamp)
    return dict(exp=max(_libm_tol(torch.exp, ls_c), _libm_tol(torch.exp, x)),
                tanh=_libm_tol(torch.tanh, h["prob"]),
                log1p=_libm_tol(torch.log1p, x.exp()))


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("clamp", kr.TGH_CLAMPS, ids=kr.tgh_id)
@pytest.mark.parametrize("case", kr.TGH_CASES, ids=kr.tgh_id)
def test_tanh_gauss_fwd_against_float64(ext, case, clamp, variant):
    det, wl = variant
    B, A = case
    h = _head(ext, case, clamp, det)
    if wl:
        out = (h["pi"], h["prob"], h["ls_c"], h["logp"])
    else:
        pi, logp, prob, ls_c = ext.tanh_gauss_fwd(
            *_dev(h["mu"], h["ls"], h["eps"]), AL, *clamp, det, False)
        out = (pi.cpu(), prob.cpu(), ls_c.cpu(), None)
    a = (h["mu"], h["ls"], h["eps"], AL, *clamp, det, wl)
    tol = _head_tol(h, clamp)
    print("libm tolerances:", tol)
    ref, bnd = kr.tgh_ref(*a), kr.tgh_fwd_bounds(*a, tol=tol)
    tag = f"tanh_gauss_fwd {B}x{A} lo={clamp[0]} {_vid(variant)}"
    assert out[0].shape == out[1].shape == out[2].shape == (B, A)
    _ratio(tag + " pi", out[0], ref[0], bnd[0])
    _ratio(tag + " prob", out[1], ref[1], bnd[1] + 1e-300)
    assert torch.equal(out[2].double(), ref[2]), "ls_c is a clamp: exact"
    if det:
        assert torch.equal(out[1], h["mu"])
    if wl:
        assert out[3].shape == (B,)
        _ratio(tag + " logp", out[3], ref[3], bnd[3])
    assert bool((out[0].abs() <= AL).all())


def test_tanh_gauss_fwd_refuses_wide_rows(ext):
    z = torch.zeros(3, 65, device=DEV)
    with pytest.raises(RuntimeError, match="tanh_gauss_fwd"):
        ext.tanh_gauss_fwd(z, z, z, AL, -20.0, 2.0, False, True)


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("clamp", kr.TGH_CLAMPS, ids=kr.tgh_id)
@pytest.mark.parametrize("case", kr.TGH_CASES, ids=kr.tgh_id)
def test_tanh_gauss_bwd_against_float64(ext, case, clamp, variant):
    det, wl = variant
    B, A = case
    lo, hi = clamp
    h = _head(ext, case, clamp, det)
    dpi, dlogp = kr.tgh_bwd_operands(B, A)
    a = (h["mu"], h["ls"], h["eps"], h["prob"], h["ls_c"], dpi, dlogp, AL,
         lo, hi, det, wl)
    tol = dict(tanh=_libm_tol(torch.tanh, h["prob"]),
               exp=_libm_tol(torch.exp, h["ls_c"]))
    ref, bnd = kr.tgh_bwd_ref(*a), kr.tgh_bwd_bounds(*a, tol=tol)
    dmu, dls = ext.tanh_gauss_bwd(
        *_dev(dpi, dlogp, h["mu"], h["ls"], h["eps"], h["prob"], h["ls_c"]),
        AL, lo, hi, det, wl)
    torch.cuda.synchronize()
    tag = f"tanh_gauss_bwd {B}x{A} lo={lo} {_vid(variant)}"
    _ratio(tag + " dmu", dmu, ref[0], bnd[0])
    _ratio(tag + " dls", dls, ref[1], bnd[1])
    raw = h["ls"]
    outside = (raw < lo) | (raw > hi)
    edge = (raw == lo) | (raw == hi)
    got = dls.cpu()
    assert bool((got[outside] == 0).all()), "gradient through the clamp"
    if wl:
        assert bool((got[edge] != 0).all()), "the clamp mask is inclusive"
    if B * A >= 30:
        assert bool(outside.any()) and bool((raw == lo).any()) \
            and bool((raw == hi).any())
        assert bool((h["prob"].abs() > 10).any()), "saturated tanh"


# -- sac_q_loss_fwd / sac_pi_loss_fwd -------------------------------------------

@pytest.mark.parametrize("B", kr.FLAT_LOSS_B)
def test_sac_q_loss_fwd_against_float64(ext, B):
    h = kr.QLOSS_HYPER
    t = kr.flat_qloss_inputs(B)
    ref, bnd = kr.qloss_ref(t, B, h["alpha"], h["gamma"], h["scale"])
    loss, dq1, dq2 = ext.sac_q_loss_fwd(
        *_dev(t["q1"], t["q2"], t["q1t"], t["q2t"], t["logp"], t["rew"],
              t["done"]), h["alpha"], h["gamma"], h["scale"])
    torch.cuda.synchronize()
    assert loss.shape == () and dq1.shape == dq2.shape == (B,)
    _ratio(f"sac_q_loss_fwd B={B} loss", loss, ref["loss"], bnd["loss"])
    _ratio(f"sac_q_loss_fwd B={B} dq1", dq1, ref["dq1"], bnd["dq1"])
    _ratio(f"sac_q_loss_fwd B={B} dq2", dq2, ref["dq2"], bnd["dq2"])


@pytest.mark.parametrize("B", kr.FLAT_LOSS_B)
def test_sac_pi_loss_fwd_against_float64(ext, B):
    alpha = kr.QLOSS_HYPER["alpha"]
    t = kr.piloss_inputs(B, 1, seed=31)
    ref, bnd = kr.piloss_ref(t, B, alpha)
    loss, dq1, dq2, dlogp = ext.sac_pi_loss_fwd(
        *_dev(t["q1"], t["q2"], t["logp"]), alpha)
    torch.cuda.synchronize()
    assert loss.shape == () and dq1.shape == dq2.shape == dlogp.shape == (B,)
    _ratio(f"sac_pi_loss_fwd B={B} loss", loss, ref["loss"], bnd["loss"])
    for k, got in (("dq1", dq1), ("dq2", dq2)):
        _ratio(f"sac_pi_loss_fwd B={B} {k}", got, ref[k].double(),
               bnd[k].double() + 1e-300)
    tie = t["q1"] == t["q2"]
    lt = t["q1"] < t["q2"]
    g1, g2 = dq1.cpu(), dq2.cpu()
    assert bool(tie.any())
    assert torch.equal(g1[tie], g2[tie]), "ties: -0.5 / B on both critics"
    assert bool((g1[tie] < 0).all())
    assert bool((g2[lt] == 0).all()) and bool((g1[~lt & ~tie] == 0).all())
    want = torch.full((B,), kr.piloss_dlogp_ref(B, alpha),
                      dtype=torch.float64).float()
    assert torch.equal(dlogp.cpu(), want), "dlogp = alpha / B exactly"


# -- adam_step_ -----------------------------------------------------------------

@pytest.mark.parametrize("wd", kr.ADAM_FLAT_WD)
@pytest.mark.parametrize("step", kr.ADAM_FLAT_STEPS)
@pytest.mark.parametrize("n", kr.ADAM_FLAT_N)
def test_adam_step_against_float64(ext, n, step, wd):
    hyper = dict(kr.ADAM_HYPER, wd=wd)
    p, g, m, v, _ = kr.adam_state(n, step, False, seed=step)
    ref = kr.adam_ref(p, g, m, v, None, step, hyper)
    bounds = kr.adam_bounds(p, g, m, ref, hyper)
    bufs = []
    for t in (p, g, m, v):
        buf = _sent(n + GUARD)
        buf[:n] = t.to(DEV)
        bufs.append(buf)
    ctr = _i64(step - 1)
    ext.adam_step_(*(b[:n] for b in bufs), ctr, hyper["lr"], hyper["b1"],
                   hyper["b2"], hyper["eps"], wd)
    torch.cuda.synchronize()
    assert int(ctr) == step, "the binding bumps the device counter once"
    for nm, buf, r, b in zip("pmv", (bufs[0], bufs[2], bufs[3]), ref, bounds):
        _ratio(f"adam_step_ n={n} t={step} wd={wd} {nm}", buf[:n], r, b)
    assert torch.equal(bufs[1][:n].cpu(), g), "g is read only"
    for buf in bufs:
        assert bool((buf[n:] == kr.SENTINEL).all()), "write past the end"


# -- polyak_ ----------------------------------------------------------------------

@pytest.mark.parametrize("rho", kr.POLYAK_RHO)
@pytest.mark.parametrize("n", kr.POLYAK_N)
def test_polyak_against_float64(ext, n, rho):
    targ, src = kr.polyak_inputs(n)
    ref, bnd = kr.polyak_ref(targ, src, rho)
    tb, sb = _sent(n + GUARD), _sent(n + GUARD)
    tb[:n], sb[:n] = targ.to(DEV), src.to(DEV)
    ext.polyak_(tb[:n], sb[:n], rho)
    torch.cuda.synchronize()
    _ratio(f"polyak_ n={n} rho={rho}", tb[:n], ref, bnd)
    if rho in (0.0, 1.0):
        assert torch.equal(tb[:n].cpu(), src if rho == 0.0 else targ)
    assert torch.equal(sb[:n].cpu(), src), "src is read only"
    assert bool((tb[n:] == kr.SENTINEL).all()), "write past the end"
    assert bool((sb[n:] == kr.SENTINEL).all())


# -- through ops/functional.py ------------------------------------------------------

def _head_leaves(case, clamp):
    mu, ls, eps = kr.tgh_inputs(*case, *clamp)
    mu, ls, eps = _dev(mu, ls, eps)
    return mu.requires_grad_(True), ls.requires_grad_(True), eps


def test_tanh_gauss_head_autograd_equals_raw_bindings(ext):
    from torch_actor_critic_amd.ops import functional as Fo
    case, clamp = (6, 6), kr.TGH_CLAMPS[1]
    dpi, dlogp = _dev(*kr.tgh_bwd_operands(*case))
    for det, wl in VARIANTS:
        mu, ls, eps = _head_leaves(case, clamp)
        pi, logp = Fo.tanh_gauss_head(mu, ls, eps, AL, *clamp, det, wl)
        assert (logp is None) == (not wl)
        raw = ext.tanh_gauss_fwd(mu.detach(), ls.detach(), eps, AL, *clamp,
                                 det, wl)
        assert torch.equal(pi, raw[0])
        outs, seeds = [pi], [dpi * 3.5]
        if wl:
            assert torch.equal(logp, raw[1])
            outs, seeds = [pi, logp], [dpi * 3.5, dlogp * -0.25]
        dmu, dls = torch.autograd.grad(outs, [mu, ls], seeds)
        want = ext.tanh_gauss_bwd(dpi * 3.5, dlogp * -0.25 if wl
                                  else torch.zeros_like(dlogp), mu.detach(),
                                  ls.detach(), eps, raw[2], raw[3], AL,
                                  *clamp, det, wl)
        assert torch.equal(dmu, want[0]) and torch.equal(dls, want[1])


def test_sliced_head_outputs_backpropagate_zeros_to_the_other_rows(ext):
    """algo/graph.py runs one stacked 2B-row actor forward and feeds only
    logp_all[B:] / pi_all[B:] to the policy loss."""
    from torch_actor_critic_amd.ops import functional as Fo
    case, clamp = (6, 6), kr.TGH_CLAMPS[1]
    B = case[0] // 2
    mu, ls, eps = _head_leaves(case, clamp)
    dpi, dlogp = _dev(*kr.tgh_bwd_operands(*case))
    pi_all, logp_all = Fo.tanh_gauss_head(mu, ls, eps, AL, *clamp)
    loss = (pi_all[B:] * dpi[B:]).sum() + (logp_all[B:] * dlogp[B:]).sum()
    loss.backward()
    raw = ext.tanh_gauss_fwd(mu.detach(), ls.detach(), eps, AL, *clamp,
                             False, True)
    dpi[:B], dlogp[:B] = 0.0, 0.0
    want = ext.tanh_gauss_bwd(dpi, dlogp, mu.detach(), ls.detach(), eps,
                              raw[2], raw[3], AL, *clamp, False, True)
    for got, w in ((mu.grad, want[0]), (ls.grad, want[1])):
        assert bool((got[:B] == 0).all()), "rows outside the slice"
        assert torch.equal(got, w)
        assert bool((got[B:] != 0).any())


def test_sac_losses_autograd_scale_the_raw_seeds(ext):
    from torch_actor_critic_amd.ops import functional as Fo
    B, h = 257, kr.QLOSS_HYPER
    hs = (h["alpha"], h["gamma"], h["scale"])
    t = {k: v.to(DEV) for k, v in kr.flat_qloss_inputs(B).items()}
    q1, q2 = t["q1"].requires_grad_(True), t["q2"].requires_grad_(True)
    rest = (t["q1t"], t["q2t"], t["logp"], t["rew"], t["done"])
    loss = Fo.sac_q_loss(q1, q2, *rest, *hs)
    raw = ext.sac_q_loss_fwd(q1.detach(), q2.detach(), *rest, *hs)
    assert float(loss) == pytest.approx(float(raw[0]), rel=1e-5)
    (loss * -3.5).backward()
    assert torch.equal(q1.grad, raw[1] * -3.5)
    assert torch.equal(q2.grad, raw[2] * -3.5)

    t = {k: v.to(DEV) for k, v in kr.piloss_inputs(B, 1, seed=31).items()}
    q1, q2, logp = (t[k].requires_grad_(True) for k in ("q1", "q2", "logp"))
    loss = Fo.sac_pi_loss(q1, q2, logp, h["alpha"])
    raw = ext.sac_pi_loss_fwd(q1.detach(), q2.detach(), logp.detach(),
                              h["alpha"])
    (loss * 0.75).backward()
    for leaf, seed in zip((q1, q2, logp), raw[1:]):
        assert torch.equal(leaf.grad, seed * 0.75)


# -- host gates ---------------------------------------------------------------------
#
# Every argument set below is one the gate refuses on the host, before any
# launch; only tensors the kernels would read or write out of bounds, from
# the wrong memory or in the wrong type.

def _z(*s, **k):
    return torch.zeros(*s, device=DEV, **k)


def _strided(*s):
    return _z(*s[:-1], 2 * s[-1])[..., ::2]


HEAD_NAMES = ("dpi", "dlogp", "mu", "log_std", "eps", "prob", "ls_c")


def _head_args():
    B, A = 3, 6
    a = {k: _z(B, A) for k in HEAD_NAMES}
    a["dlogp"] = _z(B)
    return a


HEAD_FWD_GATES = {
    "log_std_rows_short": lambda: dict(log_std=_z(2, 6)),
    "eps_wrong_width": lambda: dict(eps=_z(3, 5)),
    "eps_on_cpu": lambda: dict(eps=torch.zeros(3, 6)),
    "eps_float64": lambda: dict(eps=_z(3, 6, dtype=torch.float64)),
    "log_std_1d": lambda: dict(log_std=_z(18)),
    "mu_strided": lambda: dict(mu=_strided(3, 6)),
    "mu_1d": lambda: dict(mu=_z(18), log_std=_z(18), eps=_z(18)),
    "A_above_64": lambda: dict(mu=_z(3, 65), log_std=_z(3, 65),
                               eps=_z(3, 65)),
}


@pytest.mark.parametrize("gate", HEAD_FWD_GATES)
def test_tanh_gauss_fwd_host_gate(ext, gate):
    a = _head_args()
    a.update(HEAD_FWD_GATES[gate]())
    with pytest.raises(RuntimeError, match="tanh_gauss_fwd"):
        ext.tanh_gauss_fwd(a["mu"], a["log_std"], a["eps"], AL, -20.0, 2.0,
                           False, True)
    torch.cuda.synchronize()


HEAD_BWD_GATES = {
    "dlogp_short": lambda: dict(dlogp=_z(2)),
    "dlogp_2d": lambda: dict(dlogp=_z(3, 1)),
    "dlogp_float64": lambda: dict(dlogp=_z(3, dtype=torch.float64)),
    "dpi_wrong_width": lambda: dict(dpi=_z(3, 5)),
    "log_std_on_cpu": lambda: dict(log_std=torch.zeros(3, 6)),
    "eps_float64": lambda: dict(eps=_z(3, 6, dtype=torch.float64)),
    "eps_rows_short": lambda: dict(eps=_z(2, 6)),
    "prob_short": lambda: dict(prob=_z(17)),
    "ls_c_strided": lambda: dict(ls_c=_strided(3, 6)),
    "mu_on_cpu": lambda: dict(mu=torch.zeros(3, 6)),
    "A_above_64": lambda: {k: (_z(3) if k == "dlogp" else _z(3, 65))
                           for k in HEAD_NAMES},
}


@pytest.mark.parametrize("gate", HEAD_BWD_GATES)
def test_tanh_gauss_bwd_host_gate(ext, gate):
    a = _head_args()
    a.update(HEAD_BWD_GATES[gate]())
    with pytest.raises(RuntimeError, match="tanh_gauss_bwd"):
        ext.tanh_gauss_bwd(*(a[k] for k in HEAD_NAMES), AL, -20.0, 2.0,
                           False, True)
    torch.cuda.synchronize()


QLOSS_NAMES = ("q1", "q2", "q1t", "q2t", "logp", "rew", "done")
QLOSS_GATES = {
    "q2_short": lambda: dict(q2=_z(7)),
    "q1t_short": lambda: dict(q1t=_z(7)),
    "q2t_on_cpu": lambda: dict(q2t=torch.zeros(8)),
    "logp_float64": lambda: dict(logp=_z(8, dtype=torch.float64)),
    "rew_strided": lambda: dict(rew=_strided(8)),
    "rew_2d": lambda: dict(rew=_z(8, 1)),
    "done_short": lambda: dict(done=_z(0)),
    "q1_2d": lambda: {k: _z(8, 1) for k in QLOSS_NAMES},
    "q1_on_cpu": lambda: dict(q1=torch.zeros(8)),
}


@pytest.mark.parametrize("gate", QLOSS_GATES)
def test_sac_q_loss_fwd_host_gate(ext, gate):
    a = {k: _z(8) for k in QLOSS_NAMES}
    a.update(QLOSS_GATES[gate]())
    with pytest.raises(RuntimeError, match="sac_q_loss_fwd"):
        ext.sac_q_loss_fwd(*(a[k] for k in QLOSS_NAMES), 0.2, 0.99, 1.0)
    torch.cuda.synchronize()


PILOSS_GATES = {
    "q2_short": lambda: dict(q2=_z(7)),
    "logp_short": lambda: dict(logp=_z(7)),
    "logp_float64": lambda: dict(logp=_z(8, dtype=torch.float64)),
    "q2_on_cpu": lambda: dict(q2=torch.zeros(8)),
    "logp_strided": lambda: dict(logp=_strided(8)),
    "q1_2d": lambda: dict(q1=_z(8, 1), q2=_z(8, 1), logp=_z(8, 1)),
}


@pytest.mark.parametrize("gate", PILOSS_GATES)
def test_sac_pi_loss_fwd_host_gate(ext, gate):
    a = dict(q1=_z(8), q2=_z(8), logp=_z(8))
    a.update(PILOSS_GATES[gate]())
    with pytest.raises(RuntimeError, match="sac_pi_loss_fwd"):
        ext.sac_pi_loss_fwd(a["q1"], a["q2"], a["logp"], 0.2)
    torch.cuda.synchronize()


POLYAK_GATES = {
    "src_short": lambda: dict(src=_sent(7)),
    "src_long": lambda: dict(src=_sent(9)),
    "src_on_cpu": lambda: dict(src=torch.zeros(8)),
    "src_float64": lambda: dict(src=_z(8, dtype=torch.float64)),
    "src_strided": lambda: dict(src=_sent(16)[::2]),
    "targ_strided": lambda: dict(targ=_sent(16)[::2]),
    "targ_on_cpu": lambda: dict(targ=torch.full((8,), kr.SENTINEL)),
}


@pytest.mark.parametrize("gate", POLYAK_GATES)
def test_polyak_host_gate(ext, gate):
    a = dict(targ=_sent(8), src=_sent(8))
    a.update(POLYAK_GATES[gate]())
    with pytest.raises(RuntimeError, match="polyak_"):
        ext.polyak_(a["targ"], a["src"], 0.5)
    torch.cuda.synchronize()
    assert bool((a["targ"] == kr.SENTINEL).all()), "refused call wrote targ"


ADAM_GATES = {
    "g_short": lambda: dict(g=_sent(7)),
    "m_short": lambda: dict(m=_sent(7)),
    "v_short": lambda: dict(v=_sent(0)),
    "v_float64": lambda: dict(v=_z(8, dtype=torch.float64)),
    "g_on_cpu": lambda: dict(g=torch.zeros(8)),
    "m_strided": lambda: dict(m=_sent(16)[::2]),
    "step_int32": lambda: dict(step=_z(1, dtype=torch.int32)),
    "step_float": lambda: dict(step=_z(1)),
    "step_two": lambda: dict(step=_z(2, dtype=torch.int64)),
    "step_empty": lambda: dict(step=_z(0, dtype=torch.int64)),
    "step_on_cpu": lambda: dict(step=torch.zeros(1, dtype=torch.int64)),
}


@pytest.mark.parametrize("gate", ADAM_GATES)
def test_adam_step_host_gate(ext, gate):
    a = dict(p=_sent(8), g=_sent(8), m=_sent(8), v=_sent(8), step=_i64(3))
    state = dict(a)
    a.update(ADAM_GATES[gate]())
    with pytest.raises(RuntimeError, match="adam_step_"):
        ext.adam_step_(a["p"], a["g"], a["m"], a["v"], a["step"], 1e-3, 0.9,
                       0.999, 1e-8, 0.0)
    torch.cuda.synchronize()
    for k in ("p", "g", "m", "v"):
        assert bool((state[k] == kr.SENTINEL).all()), f"refused call wrote {k}"
    assert int(state["step"]) == 3, "refused call bumped the counter"


def test_empty_inputs_return_without_a_launch(ext):
    e2, e1 = _z(0, 6), _z(0)
    pi, logp, prob, ls_c = ext.tanh_gauss_fwd(e2, e2, e2, AL, -20.0, 2.0,
                                              False, True)
    assert pi.shape == prob.shape == ls_c.shape == (0, 6)
    assert logp.shape == (0,)
    dmu, dls = ext.tanh_gauss_bwd(e2, e1, e2, e2, e2, e2, e2, AL, -20.0,
                                  2.0, False, True)
    assert dmu.shape == dls.shape == (0, 6)
    loss, dq1, dq2 = ext.sac_q_loss_fwd(*([e1] * 7), 0.2, 0.99, 1.0)
    assert float(loss) == 0.0 and dq1.shape == dq2.shape == (0,)
    loss, dq1, dq2, dlogp = ext.sac_pi_loss_fwd(e1, e1, e1, 0.2)
    assert float(loss) == 0.0 and dlogp.shape == (0,)
    ext.polyak_(e1, e1, 0.5)
    ctr = _i64(3)
    ext.adam_step_(e1, e1, e1, e1, ctr, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    torch.cuda.synchronize()
    assert int(ctr) == 3, "nothing to step: the counter stays"
