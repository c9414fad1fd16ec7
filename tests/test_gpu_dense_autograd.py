"""The dense autograd Functions of ops/functional.py (_NativeLinear,
_PairedLinear, _QuadLinear; linear_relu, mlp_forward, linear_pair,
linear_quad) bit-exactly against float64.

The kernels below them (mgemm, mwgrad, transpose_multi) have their own
exact tests; these are about what the Functions decide: the relu mask,
which gradients exist, the cached transposed weight and the in-place
.grad writes of the graphed update.

Operands are small integers (kernel_refs' "int" kind: x, w, dy in
{-3..3}, bias in {-8..8}), so every product and partial sum is an integer
far below 2^24 and every operand is exact in bf16: outputs and all
gradients equal the float64 reference bit for bit in both compute modes,
whatever the summation order.  The reference is the same network written
with F.linear / F.relu on float64 CPU leaves carrying the same
requires_grad flags, differentiated by plain autograd; relu at y == 0
passes no gradient in either."""

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# both sides of the small-GEMM gate, odd sizes, N = 1, more than one tile
SHAPES = [(1, 6, 17), (64, 70, 33), (65, 1, 257), (130, 6, 33)]


def _sid(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(autouse=True)
def fp32_mode():
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("fp32")
    yield
    Fo.set_compute_dtype("fp32")
    Fo.set_graph_opt(None, False)


@pytest.fixture
def Fo():
    from torch_actor_critic_amd.ops import functional
    return functional


def _ops(M, N, K, seed=0, twins=2):
    """Integer operands of `twins` layers [N, K] on inputs [M, K]."""
    g = kr._gen(11000 + M * 7 + N * 3 + K + seed)
    d = {}
    for i in range(1, twins + 1):
        d[f"x{i}"] = kr.operand(g, (M, K), "int")
        d[f"w{i}"] = kr.operand(g, (N, K), "int")
        d[f"b{i}"] = kr.bias_operand(g, N, "int")
        d[f"dy{i}"] = kr.operand(g, (M, N), "int")
    return d


def _leaves(vals, needs, device, dtype):
    """name -> leaf tensor (or None) with the given requires_grad flags."""
    out = {}
    for k, v in vals.items():
        if v is None:
            out[k] = None
        else:
            out[k] = v.to(device=device, dtype=dtype) \
                .requires_grad_(needs.get(k, False))
    return out


def _lin(x, w, b, relu):
    y = F.linear(x, w, b)
    return F.relu(y) if relu else y


def _grads(outs, dys, leaves):
    """name -> gradient (None where autograd has none) of sum(out * dy)
    over the outputs with a dy (an output that depends on no leaf that
    requires grad, as the reference's frozen twin, has nothing to give)."""
    req = [(k, v) for k, v in leaves.items()
           if v is not None and v.requires_grad]
    pairs = [(o, d.to(device=o.device, dtype=o.dtype))
             for o, d in zip(outs, dys) if d is not None and o.requires_grad]
    gs = torch.autograd.grad([o for o, _ in pairs], [v for _, v in req],
                             [d for _, d in pairs], allow_unused=True)
    return {k: g for (k, _), g in zip(req, gs)}


def _same(name, got, ref):
    msg = kr.describe_mismatch(got.detach().double().cpu(), ref.detach())
    assert msg == "", f"{name}: {msg}"


def _compare(native, reference, vals, needs, dys, unused_is_zero=False):
    """Run `native` on GPU fp32 leaves and `reference` on CPU float64
    leaves; outputs and every gradient must agree bit for bit, and a
    gradient is None on one side exactly when it is on the other (with
    unused_is_zero a reference None may be native zeros: an output that
    the backward pass never reached)."""
    nl = _leaves(vals, needs, DEV, torch.float32)
    rl = _leaves(vals, needs, "cpu", torch.float64)
    no, ro = native(nl), reference(rl)
    assert len(no) == len(ro)
    for i, (a, b) in enumerate(zip(no, ro)):
        _same(f"output {i}", a, b)
    gn, gr = _grads(no, dys, nl), _grads(ro, dys, rl)
    assert gn.keys() == gr.keys() and gn
    for k in gn:
        if gr[k] is None and gn[k] is not None and unused_is_zero:
            assert bool((gn[k] == 0).all()), k
            continue
        assert (gn[k] is None) == (gr[k] is None), \
            f"{k}: native {gn[k] is None}, reference {gr[k] is None}"
        if gr[k] is not None:
            _same(f"grad {k}", gn[k], gr[k])
    return nl, no, gn


class _Spy:
    """Records what a Function's backward returns."""

    def __init__(self, monkeypatch, cls):
        self.returned = []
        inner = cls.backward

        def backward(ctx, *dys):
            out = inner(ctx, *dys)
            self.returned.append(out)
            return out
        monkeypatch.setattr(cls, "backward", staticmethod(backward))


ALL1 = dict(x1=True, w1=True, b1=True)
ALL2 = dict(x1=True, x2=True, w1=True, b1=True, w2=True, b2=True)


# -- linear_relu / mlp_forward ------------------------------------------------------

@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_linear_relu_exact(Fo, shape, relu, bias):
    v = _ops(*shape, twins=1)
    if not bias:
        v["b1"] = None
    dy = v.pop("dy1")
    _compare(lambda t: [Fo.linear_relu(t["x1"], t["w1"], t["b1"], relu)],
             lambda t: [_lin(t["x1"], t["w1"], t["b1"], relu)],
             v, ALL1, [dy])
    if relu and shape[0] * shape[1] > 50:
        y = _lin(v["x1"], v["w1"], v["b1"], False)
        assert bool((y > 0).any()) and bool((y < 0).any())
        if shape[0] * shape[1] > 500:
            assert bool((y == 0).any()), "a pre-activation of exactly 0"


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_linear_relu_strided_input_exact(Fo, shape):
    """x is every other column of a wider leaf: the gradient lands in
    those columns and the others stay zero."""
    M, N, K = shape
    v = _ops(M, N, K, seed=1, twins=1)
    g = kr._gen(11500 + M)
    v["x1"] = kr.operand(g, (M, 2 * K), "int")
    dy = v.pop("dy1")
    nl, _, gn = _compare(
        lambda t: [Fo.linear_relu(t["x1"][:, ::2], t["w1"], t["b1"], True)],
        lambda t: [_lin(t["x1"][:, ::2], t["w1"], t["b1"], True)],
        v, ALL1, [dy])
    assert not nl["x1"][:, ::2].is_contiguous()
    assert bool((gn["x1"][:, 1::2] == 0).all())


@pytest.mark.parametrize("relu_last", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("M", [1, 65, 130])
def test_mlp_forward_exact(Fo, M, relu_last):
    """33 -> 70 -> 6: the values stay below 2^24 through both layers
    (|h| <= 33 * 9 + 8, |y| <= 70 * 3 * 305 + 8, gradients likewise)."""
    a, b = _ops(M, 70, 33, seed=2, twins=1), _ops(M, 6, 70, seed=3, twins=1)
    v = dict(x1=a["x1"], w1=a["w1"], b1=a["b1"], w2=b["w1"], b2=b["b1"])

    def net(t):
        return [Fo.mlp_forward(t["x1"], [_Layer(t["w1"], t["b1"]),
                                         _Layer(t["w2"], t["b2"])],
                               relu_last)]

    def ref(t):
        h = _lin(t["x1"], t["w1"], t["b1"], True)
        return [_lin(h, t["w2"], t["b2"], relu_last)]
    _compare(net, ref, v, dict(ALL1, w2=True, b2=True), [b["dy1"]])


def test_linear_relu_bf16_mode_exact(Fo):
    """bf16 MFMA inputs, fp32 accumulation: integers in {-8..8} are exact
    in bf16, so the bf16 mode is exact too."""
    v = _ops(64, 70, 33, seed=4, twins=1)
    dy = v.pop("dy1")
    for t in list(v.values()) + [dy]:
        assert torch.equal(kr.bf16_round(t), t)
    Fo.set_compute_dtype("bf16")
    try:
        _compare(lambda t: [Fo.linear_relu(t["x1"], t["w1"], t["b1"], True)],
                 lambda t: [_lin(t["x1"], t["w1"], t["b1"], True)],
                 v, ALL1, [dy])
    finally:
        Fo.set_compute_dtype("fp32")


# -- linear_pair ------------------------------------------------------------------------

def _pair(Fo, relu):
    return lambda t: list(Fo.linear_pair(t["x1"], t["x2"], t["w1"], t["b1"],
                                         t["w2"], t["b2"], relu))


def _pair_ref(relu):
    return lambda t: [_lin(t["x1"], t["w1"], t["b1"], relu),
                      _lin(t["x2"], t["w2"], t["b2"], relu)]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_linear_pair_distinct_inputs_exact(Fo, shape, relu):
    v = _ops(*shape, seed=5)
    dys = [v.pop("dy1"), v.pop("dy2")]
    _compare(_pair(Fo, relu), _pair_ref(relu), v, ALL2, dys)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_linear_pair_shared_input_exact(Fo, shape, relu, monkeypatch):
    """One x feeds both layers: the sum2 dgrad writes dx1 = both branches
    and the Function returns dx2 = None (no accumulate kernel)."""
    v = _ops(*shape, seed=6)
    del v["x2"]
    dys = [v.pop("dy1"), v.pop("dy2")]
    spy = _Spy(monkeypatch, Fo._PairedLinear)
    _compare(lambda t: list(Fo.linear_pair(t["x1"], t["x1"], t["w1"],
                                           t["b1"], t["w2"], t["b2"], relu)),
             lambda t: [_lin(t["x1"], t["w1"], t["b1"], relu),
                        _lin(t["x1"], t["w2"], t["b2"], relu)],
             v, dict(ALL2), dys)
    (ret,) = spy.returned
    assert ret[0] is not None and ret[1] is None and ret[6] is None
    assert all(r is not None for r in ret[2:6])


# -- linear_quad ------------------------------------------------------------------------

class _Layer:
    def __init__(self, w, b):
        self.weight, self.bias = w, b


def _quad_vals(shape, seed):
    live, targ = _ops(*shape, seed=seed), _ops(*shape, seed=seed + 50)
    v = {k: live[k] for k in ("x1", "x2", "w1", "b1", "w2", "b2")}
    v.update({"t" + k: targ[k] for k in ("x1", "x2", "w1", "b1", "w2", "b2")})
    return v, [live["dy1"], live["dy2"]]


def _quad(Fo, relu, shared=False):
    def run(t):
        x2 = t["x1"] if shared else t["x2"]
        return list(Fo.linear_quad(
            t["tx1"], t["tx2"], t["x1"], x2,
            _Layer(t["tw1"], t["tb1"]), _Layer(t["tw2"], t["tb2"]),
            _Layer(t["w1"], t["b1"]), _Layer(t["w2"], t["b2"]), relu))
    return run


def _quad_ref(relu, shared=False):
    def run(t):
        x2 = t["x1"] if shared else t["x2"]
        with torch.no_grad():
            yt = [_lin(t["tx1"], t["tw1"], t["tb1"], relu),
                  _lin(t["tx2"], t["tw2"], t["tb2"], relu)]
        return yt + [_lin(t["x1"], t["w1"], t["b1"], relu),
                     _lin(x2, t["w2"], t["b2"], relu)]
    return run


@pytest.mark.parametrize("shared", [False, True], ids=["distinct", "shared"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_linear_quad_exact(Fo, shape, relu, shared):
    """Target outputs equal a separate forward on the target weights and
    are not differentiable; target weights and inputs get no gradient
    although they require one."""
    v, dys = _quad_vals(shape, 7)
    needs = dict(ALL2, tx1=True, tw1=True, tb1=True, tw2=True, tb2=True)
    nl, no, gn = _compare(_quad(Fo, relu, shared), _quad_ref(relu, shared),
                          v, needs, [None, None] + dys)
    assert not no[0].requires_grad and not no[1].requires_grad
    assert no[2].requires_grad and no[3].requires_grad
    for k in ("tx1", "tw1", "tb1", "tw2", "tb2"):
        assert gn[k] is None, f"{k} received a gradient"
    # the targets' own forward, not the live weights'
    assert not torch.equal(v["tw1"], v["w1"])


# -- graph-opt: in-place .grad writes and the cached transposed weight ----------------

def test_graph_opt_writes_grads_in_place_and_returns_none(Fo, monkeypatch):
    """Under set_graph_opt(cache, True) with pre-allocated .grad the wgrad
    lands in .grad itself (overwriting what was there: a sentinel would
    show an accumulate) and the Function returns None for w and b."""
    M, N, K = 64, 70, 33
    v = _ops(M, N, K, seed=8)
    dys = [v.pop("dy1"), v.pop("dy2")]
    rl = _leaves(v, ALL2, "cpu", torch.float64)
    want = _grads(_pair_ref(True)(rl), dys, rl)
    nl = _leaves(v, ALL2, DEV, torch.float32)
    bufs = {}
    for k in ("w1", "b1", "w2", "b2"):
        nl[k].grad = torch.full_like(nl[k], kr.SENTINEL)
        bufs[k] = nl[k].grad
    spy = _Spy(monkeypatch, Fo._PairedLinear)
    cache = {}
    Fo.set_graph_opt(cache, True)
    try:
        y1, y2 = _pair(Fo, True)(nl)
        torch.autograd.backward([y1, y2], [d.to(DEV) for d in dys])
    finally:
        Fo.set_graph_opt(None, False)
    torch.cuda.synchronize()
    (ret,) = spy.returned
    assert all(r is None for r in ret[2:]), "direct wgrad returns no tensor"
    for k in ("w1", "b1", "w2", "b2"):
        assert nl[k].grad is bufs[k], f"{k}.grad was replaced"
        _same(f"{k}.grad", nl[k].grad, want[k])
    for k in ("x1", "x2"):
        _same(f"{k}.grad", nl[k].grad, want[k])
    assert nl["w1"].data_ptr() in cache and nl["w2"].data_ptr() in cache


@pytest.mark.parametrize("which", ["linear", "pair", "quad"])
def test_graph_opt_leaves_a_frozen_layers_grad_alone(Fo, which):
    """The policy phase backpropagates through the frozen critic: its
    .grad from the critic phase must survive, and x still gets dx."""
    M, N, K = 64, 6, 33
    v, dys = _quad_vals((M, N, K), 9)
    needs = dict(x1=True, x2=True)
    rl = _leaves(v, needs, "cpu", torch.float64)
    nl = _leaves(v, needs, DEV, torch.float32)
    for k in ("w1", "b1", "w2", "b2"):
        nl[k].requires_grad_(True)
        nl[k].grad = torch.full_like(nl[k], kr.SENTINEL)
        nl[k].requires_grad_(False)          # frozen, as sac._freeze does
    if which == "linear":
        run = lambda t: [Fo.linear_relu(t["x1"], t["w1"], t["b1"], True)]
        ref = lambda t: [_lin(t["x1"], t["w1"], t["b1"], True)]
        dys = dys[:1]
    elif which == "pair":
        run, ref = _pair(Fo, True), _pair_ref(True)
    else:
        run, ref = _quad(Fo, True), _quad_ref(True)
        dys = [None, None] + dys
    want = _grads(ref(rl), dys, rl)
    Fo.set_graph_opt({}, True)
    try:
        got = _grads(run(nl), dys, nl)
    finally:
        Fo.set_graph_opt(None, False)
    torch.cuda.synchronize()
    for k in ("w1", "b1", "w2", "b2"):
        assert bool((nl[k].grad == kr.SENTINEL).all()), f"{k}.grad clobbered"
    _same("dx1", got["x1"], want["x1"])
    if which != "linear":
        _same("dx2", got["x2"], want["x2"])


def test_wt_cache_follows_the_weight_only_after_a_refresh(Fo):
    """The documented contract of the cached transposed weight: after an
    in-place change of w the dgrad still reads the OLD transpose until
    refresh_wt_cache runs (the graphed update refreshes once per phase,
    right after its Adam step)."""
    M, N, K = 65, 6, 33
    v = _ops(M, N, K, seed=10, twins=1)
    dy = v.pop("dy1").to(DEV)
    x = v["x1"].to(DEV).requires_grad_(True)
    w = v["w1"].to(DEV).requires_grad_(True)
    b = v["b1"].to(DEV)
    cache = {}

    def dx():
        y = Fo.linear_relu(x, w, b, True)
        return y, torch.autograd.grad([y], [x], [dy])[0]

    def want(w_for_dgrad):
        y = _lin(x.detach().double().cpu(), w.detach().double().cpu(),
                 b.double().cpu(), True)
        return ((dy.double().cpu() * (y > 0)) @ w_for_dgrad)

    Fo.set_graph_opt(cache, False)
    try:
        _, g0 = dx()
        w_old = w.detach().double().cpu().clone()
        _same("dx before the change", g0, want(w_old))
        with torch.no_grad():
            w.mul_(-2.0).add_(1.0)
        w_new = w.detach().double().cpu().clone()
        assert not torch.equal(w_old, w_new)
        _, g1 = dx()
        _same("dx without a refresh reads the old transpose", g1,
              want(w_old))
        Fo.refresh_wt_cache(cache, [w])
        _, g2 = dx()
        _same("dx after the refresh", g2, want(w_new))
        assert not torch.equal(g1, g2)
    finally:
        Fo.set_graph_opt(None, False)


# -- mixed requires_grad ----------------------------------------------------------------

def _expect_nones(ret, flags):
    """A backward returns a tensor exactly for the inputs that need one."""
    for i, (r, need) in enumerate(zip(ret, flags)):
        assert (r is not None) == need, \
            f"input {i}: needs grad {need}, backward returned " \
            f"{'a tensor' if r is not None else 'None'}"


MIXED_LINEAR = {
    "only_bias": dict(b1=True),
    "only_weight": dict(w1=True),
    "bias_and_x": dict(x1=True, b1=True),
}


@pytest.mark.parametrize("needs", MIXED_LINEAR)
def test_linear_relu_mixed_requires_grad(Fo, needs, monkeypatch):
    nd = MIXED_LINEAR[needs]
    v = _ops(65, 6, 33, seed=11, twins=1)
    dy = v.pop("dy1")
    spy = _Spy(monkeypatch, Fo._NativeLinear)
    _compare(lambda t: [Fo.linear_relu(t["x1"], t["w1"], t["b1"], True)],
             lambda t: [_lin(t["x1"], t["w1"], t["b1"], True)],
             v, nd, [dy])
    (ret,) = spy.returned
    _expect_nones(ret, [nd.get(k, False) for k in ("x1", "w1", "b1")]
                  + [False])


MIXED_TWIN = {
    "only_x2": dict(x2=True),
    "only_x1": dict(x1=True),
    "only_w2_b2": dict(w2=True, b2=True),
    "only_b1": dict(b1=True),
    "x2_and_w1": dict(x2=True, w1=True),
}
TWIN_ORDER = ("x1", "x2", "w1", "b1", "w2", "b2")


@pytest.mark.parametrize("needs", MIXED_TWIN)
def test_linear_pair_mixed_requires_grad(Fo, needs, monkeypatch):
    nd = MIXED_TWIN[needs]
    v = _ops(65, 6, 33, seed=12)
    dys = [v.pop("dy1"), v.pop("dy2")]
    spy = _Spy(monkeypatch, Fo._PairedLinear)
    _compare(_pair(Fo, True), _pair_ref(True), v, nd, dys)
    (ret,) = spy.returned
    _expect_nones(ret, [nd.get(k, False) for k in TWIN_ORDER] + [False])


@pytest.mark.parametrize("needs", MIXED_TWIN)
def test_linear_quad_mixed_requires_grad(Fo, needs, monkeypatch):
    nd = MIXED_TWIN[needs]
    v, dys = _quad_vals((65, 6, 33), 13)
    spy = _Spy(monkeypatch, Fo._QuadLinear)
    _compare(_quad(Fo, True), _quad_ref(True), v, nd, [None, None] + dys)
    (ret,) = spy.returned
    live = [nd.get(k, False) for k in TWIN_ORDER]
    _expect_nones(ret, [False, False] + live[:2] + [False] * 4 + live[2:]
                  + [False])


# -- backward through one live output only --------------------------------------------

@pytest.mark.parametrize("live", [0, 1], ids=["first", "second"])
@pytest.mark.parametrize("which", ["pair", "quad"])
def test_backward_through_one_live_output(Fo, which, live):
    """Only one of the two live outputs reaches the loss.  The other one's
    dy is zeros (pair) or None (quad, which does not materialise grads):
    its layer's gradients are zero, the used layer's are exact."""
    v, dys = _quad_vals((65, 6, 33), 14)
    dys[1 - live] = None
    if which == "pair":
        run, ref = _pair(Fo, True), _pair_ref(True)
    else:
        run, ref, dys = _quad(Fo, True), _quad_ref(True), [None, None] + dys
    _, _, gn = _compare(run, ref, v, ALL2, dys, unused_is_zero=True)
    used = str(live + 1)
    for k in ("x", "w", "b"):
        assert gn[k + used] is not None and bool((gn[k + used] != 0).any())
