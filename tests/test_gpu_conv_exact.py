"""The implicit-GEMM conv kernels (conv.hip) against float64 references
built by kernel_refs.py: every instantiation (fp32/bf16, ReLU, masked,
compiled 8/4/3 family and the runtime fallback), the multi-problem
launches, the shared-input twin wgrad and the direct `out=` path.

Exact tests use small-integer operands (see kernel_refs.py; the CPU
test test_kernel_refs.py proves every partial sum stays below 2^24), so
outputs must equal the float64 reference bit for bit in both compute
dtypes.  Rounding tests use randn operands and the derived bound
kernel_refs.rounding_bound."""

import functools
import os
import subprocess
import sys
import types

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["fp32", "bf16"]
geoms = pytest.mark.parametrize("geom", kr.CONV_GEOMS, ids=kr.conv_id)
dtypes = pytest.mark.parametrize("dtype", DTYPES)


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


# CPU operands and float64 references: computed once, shared, read-only
@functools.lru_cache(maxsize=None)
def _ops(geom, seed=0, kind="int"):
    return kr.conv_operands(geom, kind, seed)


@functools.lru_cache(maxsize=None)
def _fwd_ref(geom, seed, bias, relu):
    o = _ops(geom, seed)
    return kr.conv_fwd_ref(o.x, o.w, o.b if bias else None, geom[7], relu)[0]


@functools.lru_cache(maxsize=None)
def _bwd_ref(geom, seed, masked, x_seed=None):
    """(dx, dw, db) for operand set `seed`; x_seed: take x from another
    set (the shared-input twin wgrad)."""
    o = _ops(geom, seed)
    x = o.x if x_seed is None else _ops(geom, x_seed).x
    return kr.conv_bwd_ref(x, o.w, o.dy, geom[7], o.mask if masked else None)


def _d(t):
    return None if t is None else t.to(DEV)


def _wt(w):
    oc, ic, kh, kw = w.shape
    return w.permute(1, 0, 2, 3).reshape(ic, oc * kh * kw).contiguous()


def _poison(*shapes):
    """Leave sentinel-filled blocks in the caching allocator, so that the
    `torch::empty` outputs the launchers allocate next do not start as
    zeros: every logical element has to be written by the kernel."""
    for s in shapes:
        t = torch.full(tuple(s), kr.SENTINEL, device=DEV)
        del t


def _same(name, out, ref):
    msg = kr.describe_mismatch(out.cpu().double(), ref.reshape(out.shape))
    assert msg == "", f"{name}: {msg}"


# ---------------------------------------------------------------------------
# exact: forward
# ---------------------------------------------------------------------------

@dtypes
@geoms
def test_conv_fwd_exact(ext, geom, dtype):
    S = geom[7]
    o = _ops(geom)
    x, w, b = _d(o.x), _d(o.w), _d(o.b)
    _set_dtype(dtype)
    for bias in (True, False):
        for relu in (False, True):
            ref = _fwd_ref(geom, 0, bias, relu)
            _poison(ref.shape)
            y = ext.conv2d_fwd(x, w, b if bias else None, S, relu)
            _same(f"fwd bias={bias} relu={relu} {dtype}", y, ref)


@dtypes
@geoms
def test_conv_fwd_multi_exact(ext, geom, dtype):
    """2-4 problems per launch, distinct x / w / bias, one bias None."""
    S = geom[7]
    _set_dtype(dtype)
    for nz in (2, 3, 4):
        relu = nz != 3
        sets = [_ops(geom, z) for z in range(nz)]
        has_b = [z != nz - 2 for z in range(nz)]
        _poison(*[_fwd_ref(geom, 0, True, relu).shape] * nz)
        ys = ext.conv2d_fwd_multi(
            [_d(o.x) for o in sets], [_d(o.w) for o in sets],
            [_d(o.b) if hb else None for o, hb in zip(sets, has_b)],
            S, relu)
        assert len(ys) == nz
        for z, y in enumerate(ys):
            _same(f"fwd_multi nz={nz} [{z}] {dtype}", y,
                  _fwd_ref(geom, z, has_b[z], relu))


# ---------------------------------------------------------------------------
# exact: dgrad
# ---------------------------------------------------------------------------

def _assert_uncovered_zero(name, geom, dx):
    unc = kr.uncovered(geom)
    if bool(unc.any()):
        vals = dx.cpu()[:, :, unc]
        assert bool((vals == 0).all()), \
            f"{name}: dx != 0 at pixels no window covers"


@dtypes
@geoms
def test_conv_dgrad_exact(ext, geom, dtype):
    S = geom[7]
    o = _ops(geom)
    x_like, w, dy, wt = _d(o.x), _d(o.w), _d(o.dy), _d(_wt(o.w))
    _set_dtype(dtype)
    for masked in (False, True):
        ref = _bwd_ref(geom, 0, masked)[0]
        _poison(ref.shape)
        dx = ext.conv2d_dgrad(dy, _d(o.mask) if masked else None, wt,
                              x_like, w, S)
        name = f"dgrad masked={masked} {dtype}"
        _same(name, dx, ref)
        _assert_uncovered_zero(name, geom, dx)


@dtypes
@geoms
def test_conv_dgrad_multi_exact(ext, geom, dtype):
    S = geom[7]
    sets = [_ops(geom, 0), _ops(geom, 1)]
    _set_dtype(dtype)
    for masked in (False, True):
        _poison(sets[0].x.shape, sets[0].x.shape)
        dxs = ext.conv2d_dgrad_multi(
            [_d(o.dy) for o in sets],
            [_d(o.mask) if masked else None for o in sets],
            [_d(_wt(o.w)) for o in sets], _d(sets[0].x), _d(sets[0].w), S)
        assert len(dxs) == 2
        for z, dx in enumerate(dxs):
            name = f"dgrad_multi masked={masked} [{z}] {dtype}"
            _same(name, dx, _bwd_ref(geom, z, masked)[0])
            _assert_uncovered_zero(name, geom, dx)


@geoms
def test_conv_wt_cache_layout(ext, geom):
    """Fo._conv_wt under an active cache (transpose_multi with a block
    size) gives the bits of the torch permute, and caches them."""
    from torch_actor_critic_amd.ops import functional as Fo
    w = _d(_ops(geom).w)
    cache = {}
    Fo.set_graph_opt(cache, False)
    try:
        wt = Fo._conv_wt(ext, w)
        again = Fo._conv_wt(ext, w)
    finally:
        Fo.set_graph_opt(None, False)
    assert again is wt and w.data_ptr() in cache
    assert torch.equal(wt.cpu(), _wt(_ops(geom).w))
    assert torch.equal(Fo._conv_wt(ext, w).cpu(), _wt(_ops(geom).w))


# ---------------------------------------------------------------------------
# exact: wgrad
# ---------------------------------------------------------------------------

@dtypes
@geoms
def test_conv_wgrad_exact(ext, geom, dtype):
    S = geom[7]
    o = _ops(geom)
    x, w, dy = _d(o.x), _d(o.w), _d(o.dy)
    _set_dtype(dtype)
    for masked in (False, True):
        _, dw_ref, db_ref = _bwd_ref(geom, 0, masked)
        _poison(dw_ref.shape, db_ref.shape)
        dw, db = ext.conv2d_wgrad(dy, _d(o.mask) if masked else None, x, w,
                                  S)
        _same(f"wgrad dw masked={masked} {dtype}", dw, dw_ref)
        _same(f"wgrad db masked={masked} {dtype}", db, db_ref)


def _wgrad_multi(ext, geom, masked, shared, out):
    S = geom[7]
    sets = [_ops(geom, 0), _ops(geom, 1)]
    x0 = _d(sets[0].x)
    xs = [x0, x0] if shared else [x0, _d(sets[1].x)]
    res = ext.conv2d_wgrad_multi(
        [_d(o.dy) for o in sets],
        [_d(o.mask) if masked else None for o in sets],
        xs, _d(sets[0].w), S, out=out)
    assert len(res) == 4
    return res


def _check_wgrad_multi(name, geom, res, masked, shared):
    for z in range(2):
        _, dw_ref, db_ref = _bwd_ref(geom, z, masked,
                                     x_seed=0 if shared else None)
        _same(f"{name} dw[{z}]", res[2 * z], dw_ref)
        _same(f"{name} db[{z}]", res[2 * z + 1], db_ref)


@dtypes
@geoms
def test_conv_wgrad_multi_distinct_exact(ext, geom, dtype):
    """nz = 2 with distinct inputs: conv_wgrad_kernel with p1."""
    _set_dtype(dtype)
    o = _ops(geom)
    for masked in (False, True):
        _poison(o.w.shape, o.b.shape, o.w.shape, o.b.shape)
        res = _wgrad_multi(ext, geom, masked, shared=False, out=[])
        _check_wgrad_multi(f"wgrad_multi distinct masked={masked} {dtype}",
                           geom, res, masked, False)


@dtypes
@geoms
def test_conv_wgrad_multi_shared_exact(ext, geom, dtype):
    """The same x tensor passed twice: conv_wgrad2s_kernel."""
    _set_dtype(dtype)
    o = _ops(geom)
    for masked in (False, True):
        _poison(o.w.shape, o.b.shape, o.w.shape, o.b.shape)
        res = _wgrad_multi(ext, geom, masked, shared=True, out=[])
        _check_wgrad_multi(f"wgrad_multi shared masked={masked} {dtype}",
                           geom, res, masked, True)


@dtypes
@geoms
def test_conv_wgrad_multi_out_exact(ext, geom, dtype):
    """out=[dw0, db0, dw1, db1]: the sentinel-filled gradient buffers
    end fully overwritten, for both wgrad kernels and nz = 1."""
    _set_dtype(dtype)
    o = _ops(geom)
    for shared in (False, True):
        out = [torch.full(tuple(s), kr.SENTINEL, device=DEV)
               for s in (o.w.shape, o.b.shape, o.w.shape, o.b.shape)]
        res = _wgrad_multi(ext, geom, True, shared, out)
        for r, buf in zip(res, out):
            assert r.data_ptr() == buf.data_ptr()
        _check_wgrad_multi(f"wgrad_multi out= shared={shared} {dtype}",
                           geom, out, True, shared)
    out = [torch.full(tuple(s), kr.SENTINEL, device=DEV)
           for s in (o.w.shape, o.b.shape)]
    ext.conv2d_wgrad_multi([_d(o.dy)], [None], [_d(o.x)], _d(o.w), geom[7],
                           out=out)
    _, dw_ref, db_ref = _bwd_ref(geom, 0, False)
    _same(f"wgrad out= nz=1 dw {dtype}", out[0], dw_ref)
    _same(f"wgrad out= nz=1 db {dtype}", out[1], db_ref)


# ---------------------------------------------------------------------------
# rounding (randn operands, derived bound)
# ---------------------------------------------------------------------------

ROUNDING_GEOMS = [kr.CONV_KNOWN[2], kr.CONV_FALLBACK[1]]
rgeoms = pytest.mark.parametrize("geom", ROUNDING_GEOMS, ids=kr.conv_id)


def _within_bound(name, out, ref, s_abs, k_red):
    err = (out.cpu().double().reshape(ref.shape) - ref).abs()
    bound = kr.rounding_bound(k_red, s_abs)
    ratio = float((err / bound).max())
    print(f"{name}: max err/bound = {ratio:.4f}")
    assert bool((err <= bound).all()), (name, ratio)


def _rounded(t, dtype):
    return kr.bf16_round(t) if dtype == "bf16" else t


@rgeoms
def test_conv_fwd_rounding(ext, geom):
    B, IC, IH, IW, OC, KH, KW, S = geom
    o = _ops(geom, 7, "randn")
    outs = {}
    for dtype in DTYPES:
        ref, s_abs = kr.conv_fwd_ref(_rounded(o.x, dtype),
                                     _rounded(o.w, dtype), o.b, S, False)
        _set_dtype(dtype)
        y = ext.conv2d_fwd(_d(o.x), _d(o.w), _d(o.b), S, False)
        outs[dtype] = y.cpu()
        _within_bound(f"conv fwd {kr.conv_id(geom)} {dtype}", y, ref, s_abs,
                      IC * KH * KW)
    assert not torch.equal(outs["fp32"], outs["bf16"])


@rgeoms
def test_conv_dgrad_rounding(ext, geom):
    B, IC, IH, IW, OC, KH, KW, S = geom
    o = _ops(geom, 7, "randn")
    outs = {}
    for dtype in DTYPES:
        dy, w = _rounded(o.dy, dtype), _rounded(o.w, dtype)
        ref = kr.conv_bwd_ref(o.x, w, dy, S)[0]
        s_abs = kr.conv_bwd_abs(o.x, w, dy, S)[0]
        _set_dtype(dtype)
        dx = ext.conv2d_dgrad(_d(o.dy), None, _d(_wt(o.w)), _d(o.x),
                              _d(o.w), S)
        outs[dtype] = dx.cpu()
        _within_bound(f"conv dgrad {kr.conv_id(geom)} {dtype}", dx, ref,
                      s_abs, OC * KH * KW)
    assert not torch.equal(outs["fp32"], outs["bf16"])


@rgeoms
def test_conv_wgrad_rounding(ext, geom):
    B, IC, IH, IW, OC, KH, KW, S = geom
    OH, OW = kr.conv_out_hw(geom)
    o = _ops(geom, 7, "randn")
    outs = {}
    for dtype in DTYPES:
        # bf16 mode stages dy rounded, and sums db from that staged tile
        dy, x = _rounded(o.dy, dtype), _rounded(o.x, dtype)
        _, dw_ref, db_ref = kr.conv_bwd_ref(x, o.w, dy, S)
        _, dw_abs, db_abs = kr.conv_bwd_abs(x, o.w, dy, S)
        _set_dtype(dtype)
        dw, db = ext.conv2d_wgrad(_d(o.dy), None, _d(o.x), _d(o.w), S)
        outs[dtype] = dw.cpu()
        name = f"conv wgrad {kr.conv_id(geom)} {dtype}"
        _within_bound(name + " dw", dw, dw_ref, dw_abs, B * OH * OW)
        _within_bound(name + " db", db, db_ref, db_abs, B * OH * OW)
    assert not torch.equal(outs["fp32"], outs["bf16"])


# ---------------------------------------------------------------------------
# autograd level (fp32, integer operands: still exact)
# ---------------------------------------------------------------------------

AUTOGRAD_GEOMS = [kr.CONV_KNOWN[1], kr.CONV_FALLBACK[0]]
ageoms = pytest.mark.parametrize("geom", AUTOGRAD_GEOMS, ids=kr.conv_id)


@functools.lru_cache(maxsize=None)
def _autograd_ref(geom, seed, bias, relu, x_seed=None):
    """y and (dx, dw, db) of loss = sum(conv(x) * dy), ReLU included."""
    o = _ops(geom, seed)
    x = o.x if x_seed is None else _ops(geom, x_seed).x
    y, _ = kr.conv_fwd_ref(x, o.w, o.b if bias else None, geom[7], relu)
    grads = kr.conv_bwd_ref(x, o.w, o.dy, geom[7], y if relu else None)
    return y, grads


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


@ageoms
@pytest.mark.parametrize("mask_env", [None, "1"])
@pytest.mark.parametrize("bias", [True, False])
def test_conv2d_autograd_exact(geom, bias, mask_env, monkeypatch):
    from torch_actor_critic_amd.ops import functional as Fo
    if mask_env is None:
        monkeypatch.delenv("TAC_AMD_CONV_MASK", raising=False)
    else:
        monkeypatch.setenv("TAC_AMD_CONV_MASK", mask_env)
    o = _ops(geom)
    x, w = _leaf(o.x), _leaf(o.w)
    b = _leaf(o.b) if bias else None
    y = Fo.conv2d(x, w, b, geom[7], relu=True)
    (y * _d(o.dy)).sum().backward()
    y_ref, (dx, dw, db) = _autograd_ref(geom, 0, bias, True)
    _same("y", y.detach(), y_ref)
    _same("dx", x.grad, dx)
    _same("dw", w.grad, dw)
    if bias:
        _same("db", b.grad, db)


@ageoms
def test_conv2d_autograd_direct_wgrad_exact(ext, geom, monkeypatch):
    """Under set_graph_opt(cache, True) with pre-allocated .grad buffers:
    wgrad writes straight into them and dgrad reads the cached
    transpose_multi layout."""
    from torch_actor_critic_amd.ops import functional as Fo
    monkeypatch.delenv("TAC_AMD_CONV_MASK", raising=False)
    o = _ops(geom)
    x, w, b = _leaf(o.x), _leaf(o.w), _leaf(o.b)
    w.grad = torch.full_like(w, kr.SENTINEL)
    b.grad = torch.full_like(b, kr.SENTINEL)
    gw, gb = w.grad, b.grad
    cache = {}
    Fo.set_graph_opt(cache, True)
    try:
        y = Fo.conv2d(x, w, b, geom[7], relu=True)
        (y * _d(o.dy)).sum().backward()
    finally:
        Fo.set_graph_opt(None, False)
    y_ref, (dx, dw, db) = _autograd_ref(geom, 0, True, True)
    assert w.grad is gw and b.grad is gb      # written in place
    _same("y", y.detach(), y_ref)
    _same("dx", x.grad, dx)
    _same("dw", gw, dw)
    _same("db", gb, db)
    assert torch.equal(cache[w.data_ptr()][1].cpu(), _wt(o.w))


@ageoms
@pytest.mark.parametrize("shared", [False, True])
def test_conv2d_pair_exact(geom, shared, monkeypatch):
    """conv2d_pair against the float64 reference (not against conv2d),
    with two inputs and with one input tensor given twice."""
    from torch_actor_critic_amd.ops import functional as Fo
    monkeypatch.delenv("TAC_AMD_CONV_MASK", raising=False)
    o1, o2 = _ops(geom, 0), _ops(geom, 1)
    x1 = _leaf(o1.x)
    x2 = x1 if shared else _leaf(o2.x)
    w1, b1, w2, b2 = _leaf(o1.w), _leaf(o1.b), _leaf(o2.w), _leaf(o2.b)
    y1, y2 = Fo.conv2d_pair(x1, x2, w1, b1, w2, b2, geom[7], True)
    ((y1 * _d(o1.dy)).sum() + (y2 * _d(o2.dy)).sum()).backward()
    r1, (dx1, dw1, db1) = _autograd_ref(geom, 0, True, True)
    r2, (dx2, dw2, db2) = _autograd_ref(geom, 1, True, True,
                                        x_seed=0 if shared else None)
    _same("y1", y1.detach(), r1)
    _same("y2", y2.detach(), r2)
    if shared:
        _same("dx", x1.grad, dx1 + dx2)
    else:
        _same("dx1", x1.grad, dx1)
        _same("dx2", x2.grad, dx2)
    for nm, g, r in (("dw1", w1.grad, dw1), ("db1", b1.grad, db1),
                     ("dw2", w2.grad, dw2), ("db2", b2.grad, db2)):
        _same(nm, g, r)


@ageoms
def test_conv2d_quad_exact(geom, monkeypatch):
    from torch_actor_critic_amd.ops import functional as Fo
    monkeypatch.delenv("TAC_AMD_CONV_MASK", raising=False)
    sets = [_ops(geom, z) for z in range(4)]
    mods = [types.SimpleNamespace(weight=_d(o.w), bias=_d(o.b))
            for o in sets[:2]]
    mods += [types.SimpleNamespace(weight=_leaf(o.w), bias=_leaf(o.b))
             for o in sets[2:]]
    xt1, xt2 = _d(sets[0].x), _d(sets[1].x)
    x1, x2 = _leaf(sets[2].x), _leaf(sets[3].x)
    ys = Fo.conv2d_quad(xt1, xt2, x1, x2, *mods, geom[7], True)
    assert not ys[0].requires_grad and not ys[1].requires_grad
    ((ys[2] * _d(sets[2].dy)).sum()
     + (ys[3] * _d(sets[3].dy)).sum()).backward()
    for z in range(4):
        _same(f"y[{z}]", ys[z].detach(), _autograd_ref(geom, z, True,
                                                       True)[0])
    for z, x in ((2, x1), (3, x2)):
        _, (dx, dw, db) = _autograd_ref(geom, z, True, True)
        _same(f"dx[{z}]", x.grad, dx)
        _same(f"dw[{z}]", mods[z].weight.grad, dw)
        _same(f"db[{z}]", mods[z].bias.grad, db)


# ---------------------------------------------------------------------------
# TAC_AMD_CONV_LDS=1 forward variant (read once per process)
# ---------------------------------------------------------------------------

def test_conv_fwd_lds_variant_child_process():
    """The variable is latched at the first conv call, so the variant is
    run by a worker script in a fresh process; it exits non-zero on any
    mismatch with the float64 reference."""
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    env = {**os.environ, "TAC_AMD_CONV_LDS": "1", "PYTHONPATH": repo}
    r = subprocess.run([sys.executable,
                        os.path.join(here, "conv_lds_worker.py")],
                       env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:],
                               r.stderr[-3000:])
    assert "conv_lds_worker: OK" in r.stdout
