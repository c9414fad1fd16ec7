"""adam_t (fused.hip: Adam + polyak target + dense and conv W^T refresh
in one launch) against the float64 reference kernel_refs.adam_ref.

Bounds (kernel_refs.adam_bounds), elementwise against adam_ref:
    |dm|    <= 4 * 2^-24 * (b1|m| + (1 - b1)(wd|p| + |g|))
    |dv|    <= 8 * 2^-24 * v_ref
    |dp|    <= ulp32(p_ref) + 1e-4 * |u_ref|
    |dtarg| <= 2 * ulp32(targ_ref) + 1e-4 * |u_ref|
m and v are three rounded operations each; p is one final rounding plus
the update's relative error, dominated by the cancellation in
1 - powf(b2, t) at small t.  A skipped or doubled element is wrong by
|u| itself, four orders of magnitude above the margin.  A plain fp32
evaluation in the kernel's order stays under half of every bound
(test_kernel_refs.py), which is what makes the assertion fair.  On an
MI355X the kernel's worst err/bound over all cases below was 0.31 (p),
0.43 (m), 0.48 (v) and 0.34 (targ), equal to the CPU emulation's to the
printed digits."""

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


def _guarded(t):
    """(sentinel buffer, view holding t) with GUARD floats on each side."""
    buf = torch.full((t.numel() + 2 * GUARD,), kr.SENTINEL, device=DEV)
    view = buf[GUARD:GUARD + t.numel()]
    view.copy_(t)
    return buf, view


def _guards_intact(buf):
    b = buf.cpu()
    return bool((b[:GUARD] == kr.SENTINEL).all()
                and (b[-GUARD:] == kr.SENTINEL).all())


def _slabs():
    """(offsets, cache shapes, bss) of the layout in kernel_refs."""
    offs, shapes, bss = [], [], []
    for off, N, K in kr.ADAM_T_DENSE:
        offs.append(off)
        shapes.append((K, N))
        bss.append(1)
    off, (oc, ic, kh, kw) = kr.ADAM_T_CONV
    offs.append(off)
    shapes.append((ic, oc * kh * kw))
    bss.append(kh * kw)
    return offs, shapes, bss


def _caches(shapes):
    bufs = [_guarded(torch.full((r * c,), kr.SENTINEL)) for r, c in shapes]
    return bufs, [v.view(r, c) for (_, v), (r, c) in zip(bufs, shapes)]


@pytest.mark.parametrize("wd", [0.0, 2.0 ** -7])
@pytest.mark.parametrize("with_targ", [True, False])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_t_against_float64(ext, step, with_targ, wd):
    n = kr.ADAM_T_N
    hyper = dict(kr.ADAM_HYPER, wd=wd)
    p0, g, m0, v0, t0 = kr.adam_state(n, step, with_targ, seed=step)
    ref = kr.adam_ref(p0, g, m0, v0, t0, step, hyper)
    bounds = kr.adam_bounds(p0, g, m0, ref, hyper)
    u = ref[4]

    bufs = {k: _guarded(t) for k, t in
            dict(p=p0, g=g, m=m0, v=v0).items()}
    if with_targ:
        bufs["targ"] = _guarded(t0)
    offs, shapes, bss = _slabs()
    wt_bufs, wts = _caches(shapes)
    step_t = torch.full((1,), step, dtype=torch.int64, device=DEV)
    ext.adam_t(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1],
               step_t, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"],
               hyper["wd"], offs, wts,
               bufs["targ"][1] if with_targ else None, hyper["rho"], bss)
    torch.cuda.synchronize()

    for k, (buf, _) in bufs.items():
        assert _guards_intact(buf), f"stray write around {k}"
    assert torch.equal(bufs["g"][1].cpu(), g), "the gradient was modified"
    keys = ("p", "m", "v") + (("targ",) if with_targ else ())
    for nm, r, b in zip(keys, ref, bounds):
        err = (bufs[nm][1].cpu().double() - r).abs()
        ratio = float((err / b).max())
        print(f"adam_t step={step} targ={with_targ} wd={wd} {nm}: "
              f"max err/bound = {ratio:.4f}")
        assert bool((err <= b).all()), (nm, ratio)

    # every element moved (the grid-stride wrap and the tail included)
    p_new = bufs["p"][1].cpu()
    visible = u.abs() > 4 * kr.ulp32(p0.double())
    assert int(visible.sum()) > 0.99 * n
    moved = (p_new.double() - p0.double()).abs() > 0.5 * u.abs()
    assert bool(moved[visible].all()), \
        f"{int((~moved & visible).sum())} elements did not move"

    # W^T caches: bit-equal to the new parameters, nothing outside them
    for (off, N, K), wt in zip(kr.ADAM_T_DENSE, wts):
        assert torch.equal(wt.cpu(), p_new[off:off + N * K].view(N, K).t())
    off, (oc, ic, kh, kw) = kr.ADAM_T_CONV
    slab = p_new[off:off + oc * ic * kh * kw].view(oc, ic, kh, kw)
    assert torch.equal(wts[-1].cpu(), kr.transpose_ref(slab))
    for buf, _ in wt_bufs:
        assert _guards_intact(buf), "stray write around a W^T cache"


def test_adam_t_host_gates(ext):
    """The slab table the kernel's early-break search relies on is
    checked on the host: every refused call raises before the launch and
    leaves state and caches untouched."""
    n = 4096
    p0, g, m0, v0, _ = kr.adam_state(n, 1, False)
    bufs = {k: _guarded(t) for k, t in dict(p=p0, g=g, m=m0, v=v0).items()}
    wt_bufs, (wa, wb) = _caches([(8, 16), (4, 30)])    # 128 and 120 floats
    step_t = torch.ones(1, dtype=torch.int64, device=DEV)
    h = kr.ADAM_HYPER

    def call(offs, wts, bss=()):
        ext.adam_t(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1],
                   step_t, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                   offs, wts, None, 0.0, list(bss))

    with pytest.raises(RuntimeError, match="one W\\^T cache per slab"):
        call([0, 200], [wa])
    with pytest.raises(RuntimeError, match="one W\\^T cache per slab"):
        call([0], [wa, wb])
    with pytest.raises(RuntimeError, match="bss"):
        call([0, 200], [wa, wb], [1])
    with pytest.raises(RuntimeError, match="strictly increasing"):
        call([200, 0], [wa, wb])                     # unsorted
    with pytest.raises(RuntimeError, match="strictly increasing"):
        call([0, 0], [wa, wb])                       # doubled
    with pytest.raises(RuntimeError, match="strictly increasing"):
        call([0, 127], [wa, wb])                     # overlap by one
    with pytest.raises(RuntimeError, match="strictly increasing"):
        call([-1, 200], [wa, wb])
    with pytest.raises(RuntimeError, match="inside"):
        call([0, n - 119], [wa, wb])                 # one past the end
    with pytest.raises(RuntimeError, match="W\\^T cache 1"):
        call([0, 200], [wa, wb], [1, 7])             # 30 % 7 != 0
    torch.cuda.synchronize()
    for k, t in dict(p=p0, g=g, m=m0, v=v0).items():
        assert torch.equal(bufs[k][1].cpu(), t), f"a refused call wrote {k}"
    for buf, _ in wt_bufs:
        assert bool((buf == kr.SENTINEL).all()), "a refused call wrote W^T"

    # the valid forms: adjacent slabs, conv block size dividing the width
    call([0, 128], [wa, wb])
    call([0, n - 120], [wa, wb], [1, 6])
    torch.cuda.synchronize()
