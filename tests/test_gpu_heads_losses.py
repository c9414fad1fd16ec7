"""The SAC engine's head, loss and temperature kernels (fused.hip: tg_fwd2,
tg_bwd2, the unweighted qloss2, piloss2, alpha_update) against the float64
references of kernel_refs.py, and the host gates of their bindings.

The noise is taken out of the comparison first: tg_fwd2 with hl = 0
returns the kernel's own eps bit for bit (test_gpu_philox.py holds that
draw to the host generator), and the reference takes this eps as an input.

Bounds (kernel_refs.tg_fwd_bounds, tg_bwd_bounds, qloss_ref, piloss_ref,
alpha_bounds), elementwise and first order, U = 2^-23, L_f the tolerance of
libm call f:
  * a rounded fp32 operation is charged U of the magnitude of its result
    (twice its worst case, see below), an input's bound is carried through
    by the magnitude of the partial derivative;
  * L_f = 4x the largest relative error of torch's own fp32 op on the GPU
    against float64 on the arguments the kernel sees, floor 2^-22;
  * reductions (logp over A, the losses and mean_logp over B) through
    kernel_refs.rounding_bound;
  * prob = mu + exp(ls) eps:   (L_exp + U)|std eps| + U|prob|
  * pi = al tanh(prob):        al (L_tanh|t| + (1 - t^2) b_prob) + U|pi|
  * logp: per element three roundings of the Gaussian term, b_prob twice
    (directly and through softplus, whose derivative is sigmoid(x) <= 1),
    L_exp sigmoid(x) + L_log1p softplus(x) for the two calls, 2.1e-9 where
    x > 20 returns x, one rounding per difference; summed over A plus
    rounding_bound(A, sum|term|);
  * dp = dpi al (1 - t^2) cancels to zero at saturation, so its error is
    absolute: |dpi al| (2|t| L_tanh|t| + U t^2 + U(1 - t^2)) + ...;
  * log_alpha: ulp32 + 1e-4|u| for the cancellation in 1 - powf(b, t)
    (as kernel_refs.adam_bounds) plus the errors of m and v carried
    through du/dm and du/dv.
The charge is U, not 2^-24, because a correct evaluation must stay under
HALF of every bound (test_kernel_refs.py asserts that of a plain fp32
evaluation in the kernel's order on these inputs), and an output that is a
single rounded operation on exact inputs reaches 2^-24 exactly.  A wrong
branch, mask, sign, constant or accumulation is off by orders of magnitude
more.  Worst err / bound on an MI355X over all cases below: tg_fwd2 pi
0.19, prob 0.48, logp 0.012; tg_bwd2 dmu 0.47, dls 0.22; qloss2 dq 0.38,
dy2 0.38, loss_acc 0.013; piloss2 dq 0.00, dy2 0.22, loss_acc 0.039,
mean_logp 0.003; alpha_update log_alpha 0.43, m 0.14, v 0.17 (the CPU
emulation's worst are 0.49, 0.41, 0.36, 0.38 and 0.43 for prob, dmu, dq,
qloss2's dy2 and log_alpha).  The measured L_f were the floor 2^-22 for exp and
log1p (at most 2.8e-7 for exp) and up to 5.1e-7 for tanh."""

import math

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
ARGS = (kr.TG_ACT_LIMIT, kr.TG_LO, kr.TG_HI)
ALPHA = kr.QLOSS_HYPER["alpha"]


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


def _libm_tol(fn, x32):
    """4x the largest relative error of torch's fp32 `fn` on the GPU
    against float64 on the same arguments (normal results only), floor
    2^-22: an implementation independent of the kernel under test."""
    x32 = x32.to(DEV).float()
    got, ref = fn(x32).double(), fn(x32.double())
    ok = ref.abs() >= 2.0 ** -126
    rel = float(((got - ref).abs() / ref.abs())[ok].max()) if ok.any() else 0
    return max(4 * rel, kr.LIBM_FLOOR)


def _sent(*shape):
    return torch.full(shape, kr.SENTINEL, device=DEV)


def _ratio(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    r = float((err / bound).max())
    print(f"{name}: max err/bound = {r:.4f}")
    assert bool((err <= bound).all()), (name, r)


def _i64(v):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


# -- tg_fwd2 / tg_bwd2 --------------------------------------------------------

_FWD = {}


def _fwd(ext, case):
    """One forward per case, shared by the forward and backward tests."""
    if case in _FWD:
        return _FWD[case]
    R, A, B0, ld0, col0, ld1, col1 = case
    hl = kr.tg_hl(case).to(DEV)
    ctr = _i64(kr.TG_CTR)
    # the kernel's own noise: hl = 0 makes prob_out the noise itself
    eps = _sent(R, A)
    scratch = torch.zeros(R, A, device=DEV)
    ext.tg_fwd2(torch.zeros_like(hl), scratch, 0, scratch, 0, R,
                torch.zeros(R, device=DEV), eps, ctr, kr.TG_SEED, *ARGS, 1)
    assert torch.equal(eps, ext.tg_eps(kr.TG_CTR + 1, kr.TG_SEED, R, A, hl))
    out0, out1 = _sent(B0 + 1, ld0), _sent(R - B0 + 1, ld1)
    logp, prob = _sent(R + GUARD), _sent(R * A + GUARD)
    ext.tg_fwd2(hl, out0, col0, out1, col1, B0, logp, prob, ctr,
                kr.TG_SEED, *ARGS, 1)
    torch.cuda.synchronize()
    assert int(ctr) == kr.TG_CTR
    _FWD[case] = dict(hl=hl, eps=eps.cpu(), out0=out0.cpu(), out1=out1.cpu(),
                      logp=logp.cpu(), prob=prob.cpu())
    return _FWD[case]


def _tg_tol(hl, eps):
    _, prob, _ = kr.tg_ref(hl, eps, *ARGS)
    A = hl.shape[1] // 2
    ls = hl[:, A:].clamp(kr.TG_LO, kr.TG_HI)
    x = (-2 * prob).clamp_max(20.0).float()
    return dict(exp=max(_libm_tol(torch.exp, ls), _libm_tol(torch.exp, x)),
                tanh=_libm_tol(torch.tanh, prob),
                log1p=_libm_tol(torch.log1p, x.exp()))


@pytest.mark.parametrize("case", kr.TG_CASES, ids=kr.tg_id)
def test_tg_fwd2_against_float64(ext, case):
    R, A, B0, ld0, col0, ld1, col1 = case
    f = _fwd(ext, case)
    hl = f["hl"].cpu()
    ref = kr.tg_ref(hl, f["eps"], *ARGS)
    tol = _tg_tol(hl, f["eps"])
    print("libm tolerances:", tol)
    b_pi, b_prob, b_logp = kr.tg_fwd_bounds(hl, f["eps"], *ARGS, tol=tol)
    pi = torch.cat([f["out0"][:B0, col0:col0 + A],
                    f["out1"][:R - B0, col1:col1 + A]])
    _ratio(f"tg_fwd2 {kr.tg_id(case)} pi", pi, ref[0], b_pi)
    _ratio(f"tg_fwd2 {kr.tg_id(case)} prob",
           f["prob"][:R * A].view(R, A), ref[1], b_prob)
    _ratio(f"tg_fwd2 {kr.tg_id(case)} logp", f["logp"][:R], ref[2], b_logp)
    # nothing outside the two owned blocks, in columns or rows
    for out, rows, col in ((f["out0"], B0, col0), (f["out1"], R - B0, col1)):
        own = torch.zeros_like(out, dtype=torch.bool)
        own[:rows, col:col + A] = True
        assert bool((out[~own] == kr.SENTINEL).all()), "stray pi write"
        assert bool((out[own] != kr.SENTINEL).all())
    assert bool((f["logp"][R:] == kr.SENTINEL).all())
    assert bool((f["prob"][R * A:] == kr.SENTINEL).all())
    assert bool((pi.abs() <= kr.TG_ACT_LIMIT).all())


@pytest.mark.parametrize("alpha_on_dev", [True, False], ids=["dev", "host"])
@pytest.mark.parametrize("second", [True, False], ids=["dxc2", "nodxc2"])
@pytest.mark.parametrize("case", kr.TG_CASES, ids=kr.tg_id)
def test_tg_bwd2_against_float64(ext, case, second, alpha_on_dev):
    R, A = case[:2]
    B = kr.tg_bwd_rows(case)
    f = _fwd(ext, case)
    hl = f["hl"].cpu()
    prob = f["prob"][:R * A].view(R, A).contiguous()
    dxa, dxb, col = kr.tg_bwd_operands(case, B)
    assert col > 0
    da = dxa[:, col:col + A]
    db = dxb[:, col:col + A] if second else None
    a = (hl, prob, da, db, ALPHA, B) + ARGS
    tol = dict(tanh=_libm_tol(torch.tanh, prob[:B]))
    ref, bnd = kr.tg_bwd_ref(*a), kr.tg_bwd_bounds(*a, tol=tol)

    dmu, dls = _sent(B, A), _sent(B, A)
    # the scalar that must NOT be used is set far off
    alpha_dev = torch.full((1,), ALPHA, device=DEV) if alpha_on_dev else None
    ext.tg_bwd2(dxa.to(DEV), col, dxb.to(DEV) if second else None,
                alpha_dev, 99.0 if alpha_on_dev else ALPHA, f["hl"],
                prob.to(DEV), dmu, dls, B, *ARGS)
    torch.cuda.synchronize()
    tag = f"tg_bwd2 {kr.tg_id(case)} dxc2={second} dev={alpha_on_dev}"
    _ratio(tag + " dmu", dmu, ref[0], bnd[0])
    _ratio(tag + " dls", dls, ref[1], bnd[1])
    raw = hl[:B, A:]
    outside = (raw < kr.TG_LO) | (raw > kr.TG_HI)
    edge = (raw == kr.TG_LO) | (raw == kr.TG_HI)
    got = dls.cpu()
    assert bool((got[outside] == 0).all()), "gradient through the clamp"
    assert bool((got[edge] != 0).all()), "the clamp mask is inclusive"
    if B * A >= 9:
        assert bool(outside.any()) and bool(edge.any())


def test_tg_bwd2_covers_both_clamp_ends():
    raws = torch.cat([kr.tg_hl(c)[:kr.tg_bwd_rows(c), c[1]:].reshape(-1)
                      for c in kr.TG_CASES])
    for v in (kr.TG_LO, kr.TG_HI, kr.TG_LO - 1, kr.TG_HI + 3):
        assert bool((raws == v).any()), v


# -- qloss2 (unweighted) ---------------------------------------------------------

def _run_qloss(ext, t, B, h2, fused, alpha_on_dev, bump):
    h = kr.QLOSS_HYPER
    d = {k: v.to(DEV) for k, v in t.items()}
    out = dict(loss=torch.full((1,), kr.LOSS_ACC0, device=DEV),
               dq1=_sent(B + GUARD), dq2=_sent(B + GUARD))
    fuse_args = (None, None, None, None, 0)
    if fused:
        out["dy0"], out["dy1"] = _sent(B * h2 + GUARD), _sent(B * h2 + GUARD)
        fuse_args = (d["wt0"], d["wt1"], out["dy0"], out["dy1"], h2)
    ctrs = [_i64(v) for v in (5, 17, 1000)]
    alpha_dev = torch.full((1,), h["alpha"], device=DEV) \
        if alpha_on_dev else None
    ext.qloss2(d["q1"], d["q2"], d["q1t"], d["q2t"], d["logp"], d["rew"],
               d["done"], alpha_dev, 99.0 if alpha_on_dev else h["alpha"],
               out["loss"], out["dq1"], out["dq2"], B, h["gamma"],
               h["scale"], *fuse_args, *(ctrs if bump else ()))
    torch.cuda.synchronize()
    want = [6, 18, 1001] if bump else [5, 17, 1000]
    assert [int(c) for c in ctrs] == want, "counter bump"
    return {k: v.cpu() for k, v in out.items()}


def _check_loss_outputs(tag, out, ref, bnd, B, h2, fused):
    total = kr.LOSS_ACC0 + ref["loss"]
    _ratio(tag + " loss_acc", out["loss"][0], total,
           bnd["loss"] + kr.U * total.abs())
    keys = ["dq1", "dq2"] + (["dy0", "dy1"] if fused else [])
    for k in keys:
        n = ref[k].numel()
        _ratio(f"{tag} {k}", out[k][:n].view(ref[k].shape), ref[k],
               bnd[k] + 1e-300)
        assert bool((out[k][n:] == kr.SENTINEL).all()), f"{k}: tail written"


@pytest.mark.parametrize("h2", kr.LOSS_H2)
@pytest.mark.parametrize("B", kr.LOSS_B_FUSED)
def test_qloss2_fused_against_float64(ext, B, h2):
    h = kr.QLOSS_HYPER
    t = kr.qloss_inputs(B, h2)
    ref, bnd = kr.qloss_ref(t, B, h["alpha"], h["gamma"], h["scale"])
    for on_dev, bump in ((True, True), (False, False)):
        out = _run_qloss(ext, t, B, h2, True, on_dev, bump)
        _check_loss_outputs(f"qloss2 B={B} h2={h2} dev={on_dev}", out, ref,
                            bnd, B, h2, True)


def test_qloss2_unfused_and_fused_limit(ext):
    h = kr.QLOSS_HYPER
    B = kr.LOSS_B_UNFUSED
    t = kr.qloss_inputs(B, 0)
    ref, bnd = kr.qloss_ref(t, B, h["alpha"], h["gamma"], h["scale"])
    for on_dev, bump in ((True, False), (False, True)):
        out = _run_qloss(ext, t, B, 0, False, on_dev, bump)
        _check_loss_outputs(f"qloss2 B={B} unfused dev={on_dev}", out, ref,
                            bnd, B, 0, False)
    t = kr.qloss_inputs(1025, 24)
    with pytest.raises(RuntimeError, match="at most 1024"):
        _run_qloss(ext, t, 1025, 24, True, False, True)


# -- piloss2 ------------------------------------------------------------------------

def _run_piloss(ext, t, B, h2, fused, with_mean, alpha_on_dev):
    d = {k: v.to(DEV) for k, v in t.items()}
    out = dict(loss=torch.full((1,), kr.LOSS_ACC0, device=DEV),
               dq1=_sent(B + GUARD), dq2=_sent(B + GUARD))
    if with_mean:
        out["mean_logp"] = _sent(1)
    fuse_args = (None, None, None, None, 0)
    if fused:
        out["dy0"], out["dy1"] = _sent(B * h2 + GUARD), _sent(B * h2 + GUARD)
        fuse_args = (d["wt0"], d["wt1"], out["dy0"], out["dy1"], h2)
    alpha_dev = torch.full((1,), ALPHA, device=DEV) if alpha_on_dev else None
    ext.piloss2(d["q1"], d["q2"], d["logp"], alpha_dev,
                99.0 if alpha_on_dev else ALPHA, out["loss"],
                out.get("mean_logp"), out["dq1"], out["dq2"], B, *fuse_args)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_piloss(tag, t, out, ref, bnd, B, h2, fused, with_mean):
    _check_loss_outputs(tag, out, ref, bnd, B, h2, fused)
    if with_mean:
        _ratio(tag + " mean_logp", out["mean_logp"][0], ref["mean_logp"],
               bnd["mean_logp"])
    tie = t["q1"] == t["q2"]
    lt = t["q1"] < t["q2"]
    g1, g2 = out["dq1"][:B], out["dq2"][:B]
    half = torch.tensor(-0.5 / B, dtype=torch.float64)
    whole = torch.tensor(-1.0 / B, dtype=torch.float64)
    for g in (g1, g2):
        assert bool(((g[tie].double() - half).abs() <= kr.U * half.abs())
                    .all()), "tie rows take -0.5 / B on both critics"
    assert bool((g2[lt] == 0).all()) and bool((g1[~lt & ~tie] == 0).all())
    assert bool(((g1[lt].double() - whole).abs() <= kr.U * whole.abs()).all())
    assert bool(((g2[~lt & ~tie].double() - whole).abs()
                 <= kr.U * whole.abs()).all())


@pytest.mark.parametrize("h2", kr.LOSS_H2)
@pytest.mark.parametrize("B", kr.LOSS_B_FUSED)
def test_piloss2_fused_against_float64(ext, B, h2):
    t = kr.piloss_inputs(B, h2)
    ref, bnd = kr.piloss_ref(t, B, ALPHA)
    for with_mean, on_dev in ((True, True), (False, False)):
        out = _run_piloss(ext, t, B, h2, True, with_mean, on_dev)
        _check_piloss(f"piloss2 B={B} h2={h2} mean={with_mean}", t, out, ref,
                      bnd, B, h2, True, with_mean)


@pytest.mark.parametrize("B", kr.LOSS_B_FUSED + [kr.LOSS_B_UNFUSED])
def test_piloss2_unfused_against_float64(ext, B):
    t = kr.piloss_inputs(B, 0)
    ref, bnd = kr.piloss_ref(t, B, ALPHA)
    for with_mean, on_dev in ((True, False), (False, True)):
        out = _run_piloss(ext, t, B, 0, False, with_mean, on_dev)
        _check_piloss(f"piloss2 B={B} unfused mean={with_mean}", t, out, ref,
                      bnd, B, 0, False, with_mean)
    if B == kr.LOSS_B_UNFUSED:
        with pytest.raises(RuntimeError, match="at most 1024"):
            _run_piloss(ext, kr.piloss_inputs(1025, 24), 1025, 24, True,
                        True, True)


# -- alpha_update -------------------------------------------------------------------

def test_alpha_update_five_steps_against_float64(ext):
    f32 = dict(device=DEV, dtype=torch.float32)
    la = torch.full((1,), kr.ALPHA_LOG0, **f32)
    alpha = _sent(1)
    m, v = torch.zeros(1, **f32), torch.zeros(1, **f32)
    step = _i64(0)
    te, lr = kr.ALPHA_TARGET_ENTROPY, kr.ALPHA_LR
    zero_g = 0
    for k, ml in enumerate(kr.ALPHA_MEAN_LOGP):
        before = (float(la), float(m), float(v))
        ext.alpha_update(la, alpha, m, v, step, torch.full((1,), ml, **f32),
                         te, lr)
        torch.cuda.synchronize()
        assert int(step) == k + 1
        ref = kr.alpha_ref(*before, k, ml, te, lr)
        bnd = kr.alpha_bounds(before[1], before[2], ref)
        zero_g += ref[4] == 0.0
        for nm, got, r, b in zip(("log_alpha", "m", "v"),
                                 (float(la), float(m), float(v)), ref, bnd):
            ratio = abs(got - r) / b
            print(f"alpha_update step {k + 1} {nm}: err/bound = {ratio:.4f}")
            assert ratio <= 1.0, (k + 1, nm, ratio)
        if ref[4] == 0.0:
            assert float(m) == float(torch.tensor(0.9) * before[1])
        # alpha_dev is exp of the value just written
        want = math.exp(float(la))
        tol = _libm_tol(torch.exp, la)
        assert abs(float(alpha) - want) <= (tol + kr.U) * want
    assert zero_g == 1 and int(step) == 5


# -- host gates ---------------------------------------------------------------------

def _tg_fwd_call(ext, **over):
    R, A = 4, 6
    a = dict(hl=torch.zeros(R, 2 * A, device=DEV), out0=_sent(2, 10), col0=3,
             out1=_sent(2, 8), col1=2, B0=2, logp=_sent(R), prob=_sent(R * A),
             ctr=_i64(0), seed=0, ctr_add=0)
    a.update(over)
    ext.tg_fwd2(a["hl"], a["out0"], a["col0"], a["out1"], a["col1"], a["B0"],
                a["logp"], a["prob"], a["ctr"], a["seed"], *ARGS,
                a["ctr_add"])
    return a


TG_FWD_GATES = {
    "A_above_64": lambda: dict(hl=torch.zeros(4, 130, device=DEV),
                               out0=_sent(2, 80), out1=_sent(2, 80),
                               prob=_sent(4 * 65)),
    "hl_odd_columns": lambda: dict(hl=torch.zeros(4, 11, device=DEV)),
    "hl_1d": lambda: dict(hl=torch.zeros(48, device=DEV)),
    "hl_on_cpu": lambda: dict(hl=torch.zeros(4, 12)),
    "hl_float64": lambda: dict(hl=torch.zeros(4, 12, device=DEV,
                                              dtype=torch.float64)),
    "hl_strided": lambda: dict(hl=torch.zeros(4, 24, device=DEV)[:, ::2]),
    "logp_short": lambda: dict(logp=_sent(3)),
    "prob_short": lambda: dict(prob=_sent(23)),
    "col0_past_ld": lambda: dict(col0=5),
    "col1_past_ld": lambda: dict(col1=3),
    "col0_negative": lambda: dict(col0=-1),
    "B0_negative": lambda: dict(B0=-1),
    "B0_above_R": lambda: dict(B0=5, out0=_sent(5, 10)),
    "out0_rows_short": lambda: dict(out0=_sent(1, 10)),
    "out1_rows_short": lambda: dict(B0=1),
    "out1_float64": lambda: dict(out1=torch.zeros(2, 8, device=DEV,
                                                  dtype=torch.float64)),
    "ctr_int32": lambda: dict(ctr=torch.zeros(1, dtype=torch.int32,
                                              device=DEV)),
}


@pytest.mark.parametrize("gate", TG_FWD_GATES)
def test_tg_fwd2_host_gate(ext, gate):
    over = TG_FWD_GATES[gate]()
    a = dict(out0=_sent(2, 10), out1=_sent(2, 8), logp=_sent(4),
             prob=_sent(24))
    a.update(over)
    with pytest.raises(RuntimeError, match="tg_fwd2"):
        _tg_fwd_call(ext, **a)
    torch.cuda.synchronize()
    for k in ("out0", "out1", "logp", "prob"):
        if a[k].dtype == torch.float32:
            assert bool((a[k] == kr.SENTINEL).all()), f"refused call wrote {k}"


def test_tg_fwd2_accepts_row_offset_in_col(ext):
    """The engine addresses rows B.. of one slab through the offset:
    off = row * ld + col."""
    a = _tg_fwd_call(ext, out1=_sent(5, 8), col1=3 * 8 + 2)
    torch.cuda.synchronize()
    own = torch.zeros(5, 8, dtype=torch.bool)
    own[3:5, 2:8] = True
    out1 = a["out1"].cpu()
    assert bool((out1[~own] == kr.SENTINEL).all())
    assert bool((out1[own] != kr.SENTINEL).all())
    with pytest.raises(RuntimeError, match="tg_fwd2"):
        _tg_fwd_call(ext, out1=_sent(5, 8), col1=4 * 8 + 2)


def _tg_bwd_call(ext, **over):
    B, A = 3, 6
    a = dict(dxc=torch.zeros(B, 10, device=DEV), col0=2, dxc2=None,
             alpha_dev=None, hl=torch.zeros(4, 2 * A, device=DEV),
             prob=torch.zeros(4, A, device=DEV), dmu=_sent(B, A),
             dls=_sent(B, A), B=B)
    a.update(over)
    ext.tg_bwd2(a["dxc"], a["col0"], a["dxc2"], a["alpha_dev"], ALPHA,
                a["hl"], a["prob"], a["dmu"], a["dls"], a["B"], *ARGS)
    return a


TG_BWD_GATES = {
    "A_above_64": lambda: dict(hl=torch.zeros(4, 130, device=DEV),
                               dmu=_sent(3, 65), dls=_sent(3, 65),
                               prob=torch.zeros(4, 65, device=DEV),
                               dxc=torch.zeros(3, 80, device=DEV)),
    "dmu_wrong_width": lambda: dict(dmu=_sent(3, 5)),
    "dls_wrong_rows": lambda: dict(dls=_sent(4, 6)),
    "dmu_on_cpu": lambda: dict(dmu=torch.zeros(3, 6)),
    "B_zero": lambda: dict(B=0, dmu=_sent(0, 6), dls=_sent(0, 6)),
    "hl_rows_short": lambda: dict(hl=torch.zeros(2, 12, device=DEV)),
    "prob_short": lambda: dict(prob=torch.zeros(17, device=DEV)),
    "col0_past_ld": lambda: dict(col0=5),
    "col0_negative": lambda: dict(col0=-1),
    "dxc_rows_short": lambda: dict(dxc=torch.zeros(2, 10, device=DEV)),
    "dxc_float64": lambda: dict(dxc=torch.zeros(3, 10, device=DEV,
                                                dtype=torch.float64)),
    "dxc2_other_shape": lambda: dict(dxc2=torch.zeros(3, 12, device=DEV)),
    "alpha_dev_two": lambda: dict(alpha_dev=torch.zeros(2, device=DEV)),
}


@pytest.mark.parametrize("gate", TG_BWD_GATES)
def test_tg_bwd2_host_gate(ext, gate):
    a = dict(dmu=_sent(3, 6), dls=_sent(3, 6))
    a.update(TG_BWD_GATES[gate]())
    with pytest.raises(RuntimeError, match="tg_bwd2"):
        _tg_bwd_call(ext, **a)
    torch.cuda.synchronize()
    for k in ("dmu", "dls"):
        if a[k].is_cuda:
            assert bool((a[k] == kr.SENTINEL).all()), f"refused call wrote {k}"
    _tg_bwd_call(ext)                       # the valid form passes


@pytest.mark.parametrize("A", [0, 65])
def test_tg_eps_host_gate(ext, A):
    with pytest.raises(RuntimeError, match="tg_eps"):
        ext.tg_eps(1, 0, 2, A, torch.zeros(1, device=DEV))


def _loss_operands(B, h2):
    z = lambda *s: torch.zeros(*s, device=DEV)
    return dict(q1=z(B), q2=z(B), q1t=z(B), q2t=z(B), logp=z(B), rew=z(B),
                done=z(B), alpha_dev=None, loss=z(1), dq1=_sent(B),
                dq2=_sent(B), B=B, wt0=z(h2), wt1=z(h2), dy0=_sent(B * h2),
                dy1=_sent(B * h2), h2=h2, bump=(), mean=None)


def _qloss_call(ext, **over):
    a = _loss_operands(8, 4)
    a.update(over)
    ext.qloss2(a["q1"], a["q2"], a["q1t"], a["q2t"], a["logp"], a["rew"],
               a["done"], a["alpha_dev"], ALPHA, a["loss"], a["dq1"],
               a["dq2"], a["B"], 0.99, 1.0, a["wt0"], a["wt1"], a["dy0"],
               a["dy1"], a["h2"], *a["bump"])
    return a


def _piloss_call(ext, **over):
    a = _loss_operands(8, 4)
    a.update(over)
    ext.piloss2(a["q1"], a["q2"], a["logp"], a["alpha_dev"], ALPHA,
                a["loss"], a["mean"], a["dq1"], a["dq2"], a["B"], a["wt0"],
                a["wt1"], a["dy0"], a["dy1"], a["h2"])
    return a


def _z(*s, **k):
    return torch.zeros(*s, device=DEV, **k)


LOSS_GATES = {
    "B_zero": lambda: dict(B=0),
    "q1_short": lambda: dict(q1=_z(7)),
    "q2_float64": lambda: dict(q2=_z(8, dtype=torch.float64)),
    "logp_on_cpu": lambda: dict(logp=torch.zeros(8)),
    "dq1_short": lambda: dict(dq1=_sent(7)),
    "dq2_strided": lambda: dict(dq2=_sent(16)[::2]),
    "loss_acc_two": lambda: dict(loss=_z(2)),
    "alpha_dev_int": lambda: dict(alpha_dev=_z(1, dtype=torch.int64)),
    "wt3_0_short": lambda: dict(wt0=_z(3)),
    "wt3_1_missing": lambda: dict(wt1=None),
    "dy2_0_short": lambda: dict(dy0=_sent(31)),
    "dy2_1_missing": lambda: dict(dy1=None),
    "dy2_1_alone": lambda: dict(dy0=None),
    "h2_zero": lambda: dict(h2=0),
}
QLOSS_GATES = dict(LOSS_GATES, **{
    "q1t_short": lambda: dict(q1t=_z(7)),
    "q2t_on_cpu": lambda: dict(q2t=torch.zeros(8)),
    "rew_short": lambda: dict(rew=_z(7)),
    "done_float64": lambda: dict(done=_z(8, dtype=torch.float64)),
    "bump_int32": lambda: dict(bump=(_z(1, dtype=torch.int32),)),
    "bump_two": lambda: dict(bump=(_i64(0), _z(2, dtype=torch.int64))),
})
PILOSS_GATES = dict(LOSS_GATES, **{
    "mean_logp_two": lambda: dict(mean=_z(2)),
    "mean_logp_on_cpu": lambda: dict(mean=torch.zeros(1)),
})


def _untouched(a):
    torch.cuda.synchronize()
    for k in ("dq1", "dq2", "dy0", "dy1"):
        if a.get(k) is not None and a[k].is_cuda:
            assert bool((a[k] == kr.SENTINEL).all()), f"refused call wrote {k}"


@pytest.mark.parametrize("gate", QLOSS_GATES)
def test_qloss2_host_gate(ext, gate):
    a = _loss_operands(8, 4)
    a.update(QLOSS_GATES[gate]())
    with pytest.raises(RuntimeError, match="qloss2"):
        _qloss_call(ext, **a)
    _untouched(a)


@pytest.mark.parametrize("gate", PILOSS_GATES)
def test_piloss2_host_gate(ext, gate):
    a = _loss_operands(8, 4)
    a.update(PILOSS_GATES[gate]())
    with pytest.raises(RuntimeError, match="piloss2"):
        _piloss_call(ext, **a)
    _untouched(a)


def test_loss_gates_pass_the_valid_forms(ext):
    _qloss_call(ext)
    _qloss_call(ext, bump=(_i64(0), _i64(1), _i64(2)))
    _qloss_call(ext, wt0=None, wt1=None, dy0=None, dy1=None, h2=0)
    _piloss_call(ext)
    _piloss_call(ext, mean=_z(1), wt0=None, wt1=None, dy0=None, dy1=None,
                 h2=0)
    torch.cuda.synchronize()


ALPHA_GATES = {
    "log_alpha_on_cpu": lambda: dict(log_alpha=torch.zeros(1)),
    "alpha_dev_two": lambda: dict(alpha_dev=_z(2)),
    "m_float64": lambda: dict(m=_z(1, dtype=torch.float64)),
    "v_empty": lambda: dict(v=_z(0)),
    "step_float": lambda: dict(step=_z(1)),
    "step_two": lambda: dict(step=_z(2, dtype=torch.int64)),
    "mean_logp_two": lambda: dict(mean_logp=_z(2)),
}


@pytest.mark.parametrize("gate", ALPHA_GATES)
def test_alpha_update_host_gate(ext, gate):
    a = dict(log_alpha=_sent(1), alpha_dev=_sent(1), m=_sent(1), v=_sent(1),
             step=_i64(3), mean_logp=_z(1))
    state = dict(a)
    a.update(ALPHA_GATES[gate]())
    with pytest.raises(RuntimeError, match="alpha_update"):
        ext.alpha_update(a["log_alpha"], a["alpha_dev"], a["m"], a["v"],
                         a["step"], a["mean_logp"], -6.0, 3e-4)
    torch.cuda.synchronize()
    for k in ("log_alpha", "alpha_dev", "m", "v"):
        if a[k] is state[k]:
            assert bool((a[k] == kr.SENTINEL).all()), f"refused call wrote {k}"
    assert int(a["step"][0]) == (3 if a["step"] is state["step"] else 0)
