"""The dense weight-gradient kernels (fused.hip: mwgrad, mwgrad_het,
their combine kernels and mwgrad_het_adam) against the float64 references
of kernel_refs.py, in fp32 AND bf16 compute mode.

Exact tests use small-integer operands (test_kernel_refs.py proves on the
CPU that every partial sum is then exact in either dtype), so dw and db
must equal the reference bit for bit under any tile walk, split-M slab
plan or staging path.  Rounding tests use randn operands and
kernel_refs.rounding_bound.  dw / db are views into one sentinel-filled
buffer with guard gaps, so a stray or missing write shows.  The two
env-gated plans (TAC_AMD_WGRAD_XCD, TAC_AMD_WGRAD_RNRK) are latched once
per process and run in fresh children (wgrad_env_worker.py)."""

import os
import subprocess
import sys

import pytest
import torch

import kernel_refs as kr
import wgrad_env_worker as wk

pytestmark = pytest.mark.gpu

DEV = wk.DEV
DTYPES = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


@pytest.fixture(autouse=True)
def _fp32_mode():
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("fp32")
    yield
    Fo.set_compute_dtype("fp32")


def _set_dtype(dtype):
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype(dtype)


def _skip_if_het_plan_overridden():
    for var in wk.ENV.values():
        if var in os.environ:
            pytest.skip(f"{var} overrides the het plan under test")


def _check_mwgrad_plan(case, bf16):
    split, m_chunk, chunks, tiles = kr.mwgrad_plan(case.M, case.N, case.K,
                                                   case.nz, bf16)
    want = case.expect[1 if bf16 else 0]
    if want == "split":
        assert split > 1, "case no longer splits along M"
    elif want is not None:
        assert (split, case.M - (split - 1) * m_chunk) == want
    return split


def _check_het_plan(ext, case, bf16):
    plan = kr.het_plan(case.problems, bf16)
    assert plan == kr.HET_PLANS[(case.name, bf16, False, False)]
    assert wk.split_of(ext, case.problems) == plan[0], \
        "the plan mirror and the host disagree"
    return plan


# ---------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", kr.MWGRAD_CASES, ids=lambda c: c.name)
def test_mwgrad_exact(ext, case, dtype):
    _check_mwgrad_plan(case, dtype == "bf16")
    ops = kr.wgrad_operands(case.problems, "int")
    refs = kr.wgrad_refs(ops)
    _set_dtype(dtype)
    out = wk.launch_mwgrad(ext, case, ops)
    msgs = wk.mismatches(f"{case.name} {dtype}", ops, out, refs)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", kr.MWGRAD_HET_CASES, ids=lambda c: c.name)
def test_mwgrad_het_exact(ext, case, dtype):
    _skip_if_het_plan_overridden()
    _set_dtype(dtype)
    _check_het_plan(ext, case, dtype == "bf16")
    ops = kr.wgrad_operands(case.problems, "int")
    refs = kr.wgrad_refs(ops)
    out = wk.launch_het(ext, ops)
    msgs = wk.mismatches(f"{case.name} {dtype}", ops, out, refs)
    assert not msgs, "\n".join(msgs)


# ---------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------

def _check_rounding(what, name, ops, run):
    """run() launches under the current dtype and returns a WgOut."""
    outs = {}
    for dtype in DTYPES:
        refs = kr.wgrad_refs(ops, bf16=dtype == "bf16")
        _set_dtype(dtype)
        out = run(dtype == "bf16")
        assert out.stray_writes() == 0
        outs[dtype] = out.flat.cpu()
        worst = 0.0
        for z, (o, (dw, db, s_dw, s_db)) in enumerate(zip(ops, refs)):
            pairs = [("dw", out.dws[z], dw, s_dw)]
            if o.prob.bias:
                pairs.append(("db", out.dbs[z], db, s_db))
            for nm, got, ref, s_abs in pairs:
                err = (got.cpu().double() - ref).abs()
                bound = kr.rounding_bound(o.prob.M, s_abs)
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert bool((err <= bound).all()), \
                    (name, dtype, z, nm, ratio)
        print(f"{what} rounding {name} {dtype}: max err/bound = "
              f"{worst:.4f}")
    assert not torch.equal(outs["fp32"], outs["bf16"]), \
        "bf16 mode gave fp32 bits: the dtype flag did not take effect"


@pytest.mark.parametrize("name", kr.MWGRAD_ROUNDING_CASES)
def test_mwgrad_rounding(ext, name):
    case = kr.mwgrad_case(name)
    ops = kr.wgrad_operands(case.problems, "randn", seed=7)

    def run(bf16):
        _check_mwgrad_plan(case, bf16)
        return wk.launch_mwgrad(ext, case, ops)
    _check_rounding("mwgrad", name, ops, run)


@pytest.mark.parametrize("name", kr.MWGRAD_HET_ROUNDING_CASES)
def test_mwgrad_het_rounding(ext, name):
    _skip_if_het_plan_overridden()
    case = kr.het_case(name)
    ops = kr.wgrad_operands(case.problems, "randn", seed=7)

    def run(bf16):
        _check_het_plan(ext, case, bf16)
        return wk.launch_het(ext, ops)
    _check_rounding("mwgrad_het", name, ops, run)


# ---------------------------------------------------------------------------
# mwgrad_het_adam: the gradient it leaves behind and the Adam step on it
# ---------------------------------------------------------------------------

ADAM_STEP = 2


def _guarded(t):
    """t as a view into a sentinel buffer with GUARD floats on each side:
    (whole buffer, view)."""
    buf = torch.full((t.numel() + 2 * wk.GUARD,), kr.SENTINEL, device=DEV)
    view = buf[wk.GUARD:wk.GUARD + t.numel()]
    view.copy_(t)
    return buf, view


def _guards_intact(buf):
    b = buf.cpu()
    return bool((b[:wk.GUARD] == kr.SENTINEL).all()
                and (b[-wk.GUARD:] == kr.SENTINEL).all())


# (case, dtype, epilogue the launch must take)
HET_ADAM_MODES = [("phase64", "bf16", "quarter"),
                  ("many_tiles", "fp32", "unsplit"),
                  ("many_tiles", "bf16", "unsplit"),
                  ("phase64", "fp32", "combine")]


@pytest.mark.parametrize("name,dtype,mode", HET_ADAM_MODES)
def test_mwgrad_het_adam_grad_exact(ext, name, dtype, mode):
    """The flat gradient equals the float64 reference exactly; p, m, v,
    target and the W^T slots follow adam_ref on that gradient within
    kernel_refs.adam_bounds, in the quarter epilogue (one K-step), the
    un-split multi-step epilogue and the split-M combine."""
    _skip_if_het_plan_overridden()
    case = kr.het_case(name)
    bf16 = dtype == "bf16"
    _set_dtype(dtype)
    split, m_chunk, chunks, blk = _check_het_plan(ext, case, bf16)
    assert mode == ("combine" if split > 1 else
                    "quarter" if chunks == 1 else "unsplit")
    ops = kr.wgrad_operands(case.problems, "int")
    refs = kr.wgrad_refs(ops)

    # flat layout w|b per problem: the slices tile the buffer exactly once
    offs, n = [], 0
    for p in case.problems:
        offs.append(n)
        n += p.N * p.K + (p.N if p.bias else 0)
    g_ref = torch.cat([torch.cat([dw.reshape(-1)] + ([db] if o.prob.bias
                                                     else []))
                       for o, (dw, db, _, _) in zip(ops, refs)])
    assert g_ref.numel() == n
    hyper = kr.ADAM_HYPER
    p0, g32, m0, v0, t0 = kr.adam_state(n, ADAM_STEP, True, seed=11,
                                        g=g_ref.float())
    ref = kr.adam_ref(p0, g32, m0, v0, t0, ADAM_STEP, hyper)
    bounds = kr.adam_bounds(p0, g32, m0, ref, hyper)

    bufs = {k: _guarded(t) for k, t in
            dict(p=p0, m=m0, v=v0, targ=t0,
                 grad=torch.full((n,), kr.SENTINEL)).items()}
    grad = bufs["grad"][1]
    dws = [grad[o:o + p.N * p.K].view(p.N, p.K)
           for o, p in zip(offs, case.problems)]
    dbs = [grad[o + p.N * p.K:o + p.N * p.K + (p.N if p.bias else 0)]
           for o, p in zip(offs, case.problems)]
    wt_bufs = [_guarded(torch.full((p.N * p.K,), kr.SENTINEL))
               for p in case.problems]
    wts = [v.view(p.K, p.N) for (_, v), p in zip(wt_bufs, case.problems)]
    step = torch.full((1,), ADAM_STEP, dtype=torch.int64, device=DEV)

    class _Out:                      # what het_args needs of a WgOut
        pass
    out = _Out()
    out.dws, out.dbs = dws, dbs
    ext.mwgrad_het_adam(*wk.het_args(ops, out), bufs["p"][1], grad,
                        bufs["m"][1], bufs["v"][1], step, hyper["lr"],
                        hyper["b1"], hyper["b2"], hyper["eps"], hyper["wd"],
                        wts, bufs["targ"][1], hyper["rho"])
    torch.cuda.synchronize()

    msg = kr.describe_mismatch(grad.cpu().double(), g_ref)
    assert msg == "", f"{name} {dtype} grad: {msg}"
    for k, (buf, _) in bufs.items():
        assert _guards_intact(buf), f"stray write around {k}"
    for nm, key, r, b in zip("pmvt", ("p", "m", "v", "targ"), ref, bounds):
        err = (bufs[key][1].cpu().double() - r).abs()
        ratio = float((err / b.clamp_min(1e-300)).max())
        print(f"mwgrad_het_adam {name} {dtype} ({mode}) {nm}: "
              f"max err/bound = {ratio:.4f}")
        assert bool((err <= b).all()), (nm, ratio)
    p_new = bufs["p"][1]
    for o, p, wt, (wbuf, _) in zip(offs, case.problems, wts, wt_bufs):
        assert torch.equal(wt, p_new[o:o + p.N * p.K].view(p.N, p.K).t())
        assert _guards_intact(wbuf), "stray write around a W^T cache"


# ---------------------------------------------------------------------------
# env-gated plans, each in a fresh process
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("env", [("XCD",), ("RNRK",), ("XCD", "RNRK")],
                         ids=lambda e: "+".join(e))
def test_mwgrad_het_env_variants(env):
    """TAC_AMD_WGRAD_XCD / TAC_AMD_WGRAD_RNRK are latched at the first
    het launch of a process, so every variant runs all het cases in a
    worker process of its own; it exits non-zero on any mismatch with
    the float64 reference."""
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    child = {k: v for k, v in os.environ.items()
             if k not in wk.ENV.values()}
    child["PYTHONPATH"] = repo
    for key in env:
        child[wk.ENV[key]] = "1"
    r = subprocess.run([sys.executable,
                        os.path.join(here, "wgrad_env_worker.py"), *env],
                       env=child, capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:],
                               r.stderr[-3000:])
    assert "wgrad_env_worker: OK" in r.stdout


# ---------------------------------------------------------------------------
# host gates
# ---------------------------------------------------------------------------

def test_mwgrad_host_gates(ext):
    """mwgrad holds two problems and one MASK instantiation per launch:
    anything else is refused before a launch, outputs untouched."""
    case = kr.mwgrad_case("ragged_masked_nz2")
    ops = kr.wgrad_operands(case.problems, "int")
    M, N, K = case.M, case.N, case.K
    dys = [o.dy.to(DEV) for o in ops]
    masks = [o.mask.to(DEV) for o in ops]
    xs = [o.x.to(DEV) for o in ops]
    out = wk.WgOut(case.problems + case.problems[:1])     # three slots

    def call(dys, masks, xs, dws, dbs):
        ext.mwgrad(dys, masks, xs, dws, dbs, M, N, K, N, K, 0)

    def three(lst):
        return lst + lst[:1]

    with pytest.raises(RuntimeError, match="1..2 problems"):
        call(three(dys), three(masks), three(xs), out.dws, out.dbs)
    with pytest.raises(RuntimeError, match="1..2 problems"):
        call([], [], [], [], [])
    with pytest.raises(RuntimeError, match="one entry per problem"):
        call(dys, masks, xs[:1], out.dws[:2], out.dbs[:2])
    with pytest.raises(RuntimeError, match="one entry per problem"):
        call(dys, masks, xs, out.dws[:1], out.dbs[:2])
    with pytest.raises(RuntimeError, match="one entry per problem"):
        call(dys, masks, xs, out.dws[:2], out.dbs[:1])
    with pytest.raises(RuntimeError, match="ymasks"):
        call(dys, masks[:1], xs, out.dws[:2], out.dbs[:2])
    with pytest.raises(RuntimeError, match="all present or all absent"):
        call(dys, [masks[0], None], xs, out.dws[:2], out.dbs[:2])
    with pytest.raises(RuntimeError, match="all present or all absent"):
        call(dys, [None, masks[1]], xs, out.dws[:2], out.dbs[:2])
    torch.cuda.synchronize()
    assert bool((out.flat == kr.SENTINEL).all()), "a refused call wrote"
