"""The SAC loss kernels folded into the GEMM behind them
(fused.hip: mgemm_r1_qloss, mgemm_r1_piloss; engine flags
TAC_AMD_QLOSS_FOLD / TAC_AMD_PILOSS_FOLD).

 1. each folded launch against the launch sequence it replaces, bit for
    bit (torch.equal): qloss2 -> K=1 mgemm -> masked mgemm, and piloss2 ->
    mgemm_r1, on every staging form of the small-shape kernel;
 2. the folded launches' loss outputs against the float64 references and
    bounds of kernel_refs (the ones test_gpu_heads_losses.py holds the
    loss kernels to);
 3. whole engine updates, folds on against folds off, uncaptured and
    replayed from a captured graph;
 4. the gates: every configuration without a folded form records the
    unfolded schedule, and the bindings refuse shapes outside the gate.
"""

from copy import deepcopy

import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
H = kr.QLOSS_HYPER
CTR0 = (5, 17, 1000)

FOLD_M = [1, 33, 64, 128]
# flagship | pi-phase L0 form | K % 32 != 0, float4 path | dword path
FOLD_NK = [(256, 256), (23, 256), (33, 100), (7, 23)]


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


@pytest.fixture(autouse=True)
def _restore(ext):
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("bf16")
    prev = ext.mgemm_small_mode(1)
    yield
    ext.mgemm_small_mode(prev)
    Fo.set_compute_dtype("fp32")


def _set_dtype(dtype):
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype(dtype)


def _sent(*shape):
    return torch.full(shape, kr.SENTINEL, device=DEV)


def _i64(v):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


def _gemm_operands(M, N, K, seed):
    g = kr._gen(9500 + seed)
    ws = [torch.randn(N, K, generator=g).to(DEV) for _ in range(2)]
    masks = [kr.mask_operand(g, (M, K)).to(DEV) for _ in range(2)]
    return ws, masks


def _outputs(M, N, K, ldy, with_mean):
    """Sentinel-filled outputs; dq views hold exactly M elements of a
    longer buffer so a write past row M - 1 shows."""
    o = dict(loss=torch.full((1,), kr.LOSS_ACC0, device=DEV),
             dq1=_sent(M + GUARD), dq2=_sent(M + GUARD),
             y0=_sent(M, ldy), y1=_sent(M, ldy),
             outer0=_sent(M * K + GUARD), outer1=_sent(M * K + GUARD),
             ctrs=[_i64(v) for v in CTR0])
    if with_mean:
        o["mean"] = _sent(1)
    return o


def _assert_same(tag, a, b, M, N, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), \
            (tag, k, kr.describe_mismatch(a[k].double().cpu(),
                                          b[k].double().cpu()))
    for k in ("y0", "y1"):
        assert bool(torch.isfinite(a[k][:, :N]).all()), (tag, k)
        assert bool((a[k][:, N:] == kr.SENTINEL).all()), (tag, k, "pad")
    for k in ("dq1", "dq2"):
        assert bool((a[k][M:] == kr.SENTINEL).all()), (tag, k, "tail")
        assert bool((a[k][:M] != kr.SENTINEL).all()), (tag, k)


# ---------------------------------------------------------------------------
# 1. folded launch == unfolded sequence
# ---------------------------------------------------------------------------

def _q_unfolded(ext, d, ws, masks, o, M, N, K, ldy, alpha_dev, alpha_host,
                bump):
    ext.qloss2(d["q1"], d["q2"], d["q1t"], d["q2t"], d["logp"], d["rew"],
               d["done"], alpha_dev, alpha_host, o["loss"], o["dq1"][:M],
               o["dq2"][:M], M, H["gamma"], H["scale"], None, None, None,
               None, 0, *(o["ctrs"] if bump else ()))
    # the K=1 dgrad of the critic's output layer: dq (x) w_last
    ext.mgemm([o["dq1"][:M], o["dq2"][:M]], [d["wt0"], d["wt1"]],
              [None, None], [o["outer0"], o["outer1"]], [None, None],
              M, K, 1, 1, K, False, [], [], [], 0, 0, 0, [])
    ext.mgemm([o["outer0"], o["outer1"]], ws, [None, None],
              [o["y0"], o["y1"]], masks, M, N, K, K, ldy, False,
              [], [], [], 0, 0, 0, [])


def _q_folded(ext, d, ws, masks, o, M, N, K, ldy, alpha_dev, alpha_host,
              bump):
    ext.mgemm_r1_qloss(
        d["q1"], d["q2"], d["q1t"], d["q2t"], d["logp"], d["rew"], d["done"],
        alpha_dev, alpha_host, o["loss"], o["dq1"][:M], o["dq2"][:M],
        H["gamma"], H["scale"], *(o["ctrs"] if bump else (None,) * 3),
        [d["wt0"], d["wt1"]], ws, [o["y0"], o["y1"]], masks,
        [o["outer0"], o["outer1"]], M, N, K, ldy)


def _q_inputs(M, K):
    t = kr.qloss_inputs(M, K)
    t["q2"][0] = t["q1"][0]          # a tie row
    if M > 1:
        assert float(t["done"][-1]) == 1.0 and float(t["done"][0]) == 0.0
    return t


@pytest.mark.parametrize("N,K", FOLD_NK)
@pytest.mark.parametrize("M", FOLD_M)
def test_qloss_fold_equals_unfolded_sequence(ext, M, N, K):
    t = _q_inputs(M, K)
    d = {k: v.to(DEV) for k, v in t.items()}
    ws, masks = _gemm_operands(M, N, K, M + N)
    ldy = N + 3
    for on_dev in (True, False):
        for bump in (True, False):
            # the scalar that must NOT be used is set far off
            alpha_dev = (torch.full((1,), H["alpha"], device=DEV)
                         if on_dev else None)
            alpha_host = 99.0 if on_dev else H["alpha"]
            res = []
            for fn in (_q_unfolded, _q_folded):
                o = _outputs(M, N, K, ldy, False)
                fn(ext, d, ws, masks, o, M, N, K, ldy, alpha_dev,
                   alpha_host, bump)
                torch.cuda.synchronize()
                want = [c + 1 for c in CTR0] if bump else list(CTR0)
                assert [int(c) for c in o["ctrs"]] == want, fn.__name__
                res.append(o)
            tag = f"q M={M} N={N} K={K} dev={on_dev} bump={bump}"
            _assert_same(tag, res[1], res[0], M, N,
                         ("y0", "y1", "dq1", "dq2", "outer0", "outer1",
                          "loss"))
            dq = res[1]["dq1"][:M].cpu()
            if M > 1:      # generic seeds, not powers of two
                assert bool((torch.frexp(dq)[0].abs() != 0.5).any())
            assert float(res[1]["loss"]) != kr.LOSS_ACC0


@pytest.mark.parametrize("N,K", FOLD_NK)
@pytest.mark.parametrize("M", FOLD_M)
def test_piloss_fold_equals_unfolded_sequence(ext, M, N, K):
    t = kr.piloss_inputs(M, K)
    assert bool((t["q1"] == t["q2"]).any())         # the tie branch
    d = {k: v.to(DEV) for k, v in t.items()}
    ws, masks = _gemm_operands(M, N, K, M + N + 1)
    rows = [d["wt0"], d["wt1"]]
    ldy = N + 3
    for on_dev in (True, False):
        for with_mean in (True, False):
            alpha_dev = (torch.full((1,), H["alpha"], device=DEV)
                         if on_dev else None)
            alpha_host = 99.0 if on_dev else H["alpha"]
            res = []
            for folded in (False, True):
                o = _outputs(M, N, K, ldy, with_mean)
                ys = [o["y0"], o["y1"]]
                if folded:
                    ext.mgemm_r1_piloss(
                        d["q1"], d["q2"], d["logp"], alpha_dev, alpha_host,
                        o["loss"], o.get("mean"), o["dq1"][:M], o["dq2"][:M],
                        rows, ws, ys, masks, M, N, K, ldy)
                else:
                    ext.piloss2(d["q1"], d["q2"], d["logp"], alpha_dev,
                                alpha_host, o["loss"], o.get("mean"),
                                o["dq1"][:M], o["dq2"][:M], M, None, None,
                                None, None, 0)
                    ext.mgemm_r1([o["dq1"][:M], o["dq2"][:M]], rows, ws, ys,
                                 masks, M, N, K, ldy)
                torch.cuda.synchronize()
                res.append(o)
            tag = f"pi M={M} N={N} K={K} dev={on_dev} mean={with_mean}"
            keys = ["y0", "y1", "dq1", "dq2", "loss"]
            if with_mean:
                keys.append("mean")
                assert float(res[1]["mean"]) != kr.SENTINEL
            _assert_same(tag, res[1], res[0], M, N, keys)
            # the pi fold has no outer-product output
            assert bool((res[1]["outer0"] == kr.SENTINEL).all())


# ---------------------------------------------------------------------------
# 2. loss outputs of the folded launches against float64
# ---------------------------------------------------------------------------

def _ratio(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    r = float((err / bound).max())
    print(f"{name}: max err/bound = {r:.4f}")
    assert bool((err <= bound).all()), (name, r)


@pytest.mark.parametrize("M", FOLD_M)
def test_folded_losses_against_float64(ext, M):
    N, K = 33, 100
    ldy = N
    ws, masks = _gemm_operands(M, N, K, M)

    t = kr.qloss_inputs(M, K)
    ref, bnd = kr.qloss_ref(t, M, H["alpha"], H["gamma"], H["scale"])
    d = {k: v.to(DEV) for k, v in t.items()}
    o = _outputs(M, N, K, ldy, False)
    _q_folded(ext, d, ws, masks, o, M, N, K, ldy, None, H["alpha"], True)
    torch.cuda.synchronize()
    total = kr.LOSS_ACC0 + ref["loss"]
    _ratio(f"q fold M={M} loss_acc", o["loss"][0], total,
           bnd["loss"] + kr.U * total.abs())
    for k in ("dq1", "dq2"):
        _ratio(f"q fold M={M} {k}", o[k][:M], ref[k], bnd[k] + 1e-300)

    t = kr.piloss_inputs(M, K)
    ref, bnd = kr.piloss_ref(t, M, H["alpha"])
    d = {k: v.to(DEV) for k, v in t.items()}
    o = _outputs(M, N, K, ldy, True)
    ext.mgemm_r1_piloss(d["q1"], d["q2"], d["logp"], None, H["alpha"],
                        o["loss"], o["mean"], o["dq1"][:M], o["dq2"][:M],
                        [d["wt0"], d["wt1"]], ws, [o["y0"], o["y1"]], masks,
                        M, N, K, ldy)
    torch.cuda.synchronize()
    total = kr.LOSS_ACC0 + ref["loss"]
    _ratio(f"pi fold M={M} loss_acc", o["loss"][0], total,
           bnd["loss"] + kr.U * total.abs())
    _ratio(f"pi fold M={M} mean_logp", o["mean"][0], ref["mean_logp"],
           bnd["mean_logp"])
    for k in ("dq1", "dq2"):
        _ratio(f"pi fold M={M} {k}", o[k][:M], ref[k], bnd[k] + 1e-300)


# ---------------------------------------------------------------------------
# 3 / 4. engine: folds on against folds off, and the gates
# ---------------------------------------------------------------------------

FLAGSHIP = dict(B=64, O=17, A=6, hidden=[256, 256])
RAGGED = dict(B=33, O=11, A=3, hidden=[64, 64])


def _engine(B, O, A, hidden, sample=False, capture=False, learn_alpha=False,
            prioritized=False):
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    torch.manual_seed(11)
    device = torch.device(DEV)
    actor = Actor(O, A, hidden, act_limit=1.0).to(device)
    critic = DoubleCritic(O, A, hidden).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)
    buf = ReplayBuffer(512, O, A, device=device)
    if prioritized:
        buf.set_prioritized()
    if sample:
        rng = np.random.default_rng(3)
        n = 300
        buf.store_batch(rng.standard_normal((n, O)).astype(np.float32),
                        rng.uniform(-1, 1, (n, A)).astype(np.float32),
                        rng.standard_normal(n).astype(np.float32),
                        rng.standard_normal((n, O)).astype(np.float32),
                        (rng.uniform(size=n) > 0.9).astype(np.float32))
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=B, start_steps=0, steps_per_epoch=1,
              max_ep_len=100, update_after=0, update_every=1, save_every=10,
              learn_alpha=learn_alpha)
    eng = FusedSACEngine(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, B, device, sample=sample,
                         capture=capture, philox_seed=7)
    return eng, pi_opt, q_opt, target_flat


def _batch(i, B, O, A):
    g = torch.Generator().manual_seed(50 + i)
    s = torch.randn(B, O, generator=g)
    a = torch.rand(B, A, generator=g) * 2 - 1
    r = torch.randn(B, generator=g)
    ns = torch.randn(B, O, generator=g)
    d = (torch.rand(B, generator=g) > 0.9).float()
    return [t.to(DEV) for t in (s, a, r, ns, d)]


def _run(monkeypatch, flags, shape, steps=5, **kw):
    """Updates under TAC_AMD_QLOSS_FOLD = TAC_AMD_PILOSS_FOLD = flags;
    returns (state dict, (q fold, pi fold) as recorded)."""
    monkeypatch.setenv("TAC_AMD_QLOSS_FOLD", flags)
    monkeypatch.setenv("TAC_AMD_PILOSS_FOLD", flags)
    eng, pi_opt, q_opt, target_flat = _engine(**shape, **kw)
    for i in range(steps):
        if kw.get("capture"):
            eng.step()
        else:
            if not kw.get("sample"):
                eng.load_batch(*_batch(i, shape["B"], shape["O"],
                                       shape["A"]))
            eng._run_once()
    torch.cuda.synchronize()
    st = dict(actor=pi_opt.fp.flat, critic=q_opt.fp.flat,
              actor_m=pi_opt.m, actor_v=pi_opt.v, critic_m=q_opt.m,
              critic_v=q_opt.v, target=target_flat,
              loss_q=eng.loss_q_acc, loss_pi=eng.loss_pi_acc, ctr=eng.ctr,
              step_q=q_opt.step_t, step_pi=pi_opt.step_t)
    for j, wt in enumerate(list(eng._c_tr_dst) + list(eng._a_tr_dst)):
        st[f"wt{j}"] = wt
    if kw.get("learn_alpha"):
        st["log_alpha"] = eng.log_alpha
        st["mean_logp"] = eng.mean_logp
    st = {k: v.clone() for k, v in st.items()}
    return st, (eng._qloss_fold, eng._piloss_fold)


def _assert_state_equal(tag, on, off, steps):
    for k, v in off.items():
        assert bool(torch.isfinite(v.double()).all()), (tag, k)
        assert torch.equal(v, on[k]), \
            (tag, k, kr.describe_mismatch(on[k].double().cpu(),
                                          v.double().cpu()))
    assert float(off["loss_q"].abs().sum()) > 0
    for k in ("ctr", "step_q", "step_pi"):
        assert int(on[k]) == steps, (tag, k, int(on[k]))


@pytest.mark.parametrize("shape,learn_alpha",
                         [(FLAGSHIP, False), (RAGGED, True)],
                         ids=["flagship", "ragged_learn_alpha"])
def test_engine_updates_equal_with_and_without_folds(monkeypatch, shape,
                                                     learn_alpha):
    on, took = _run(monkeypatch, "1", shape, learn_alpha=learn_alpha)
    off, kept = _run(monkeypatch, "0", shape, learn_alpha=learn_alpha)
    assert took == (True, True) and kept == (False, False)
    _assert_state_equal("uncaptured", on, off, 5)


def test_engine_captured_replays_equal_with_and_without_folds(monkeypatch):
    kw = dict(sample=True, capture=True)
    on, took = _run(monkeypatch, "1", FLAGSHIP, steps=3, **kw)
    off, kept = _run(monkeypatch, "0", FLAGSHIP, steps=3, **kw)
    assert took == (True, True) and kept == (False, False)
    # two warm-up passes ahead of the capture, then the three replays
    _assert_state_equal("captured", on, off, 5)


def test_gate_one_hidden_layer_keeps_qloss2(monkeypatch):
    shape = dict(B=64, O=17, A=6, hidden=[64])
    on, took = _run(monkeypatch, "1", shape)
    off, _ = _run(monkeypatch, "0", shape)
    assert took == (False, True)
    _assert_state_equal("hidden [64]", on, off, 5)


def test_gate_fp32_records_parent_schedule(monkeypatch):
    _set_dtype("fp32")
    on, took = _run(monkeypatch, "1", FLAGSHIP)
    off, _ = _run(monkeypatch, "0", FLAGSHIP)
    assert took == (False, False)
    _assert_state_equal("fp32", on, off, 5)


def test_gate_small_mode_off_records_parent_schedule(ext, monkeypatch):
    ext.mgemm_small_mode(0)
    on, took = _run(monkeypatch, "1", FLAGSHIP)
    off, _ = _run(monkeypatch, "0", FLAGSHIP)
    assert took == (False, False)
    _assert_state_equal("small mode 0", on, off, 5)


def test_gate_prioritized_buffer_keeps_qloss2(monkeypatch):
    kw = dict(sample=True, prioritized=True)
    on, took = _run(monkeypatch, "1", FLAGSHIP, steps=3, **kw)
    off, _ = _run(monkeypatch, "0", FLAGSHIP, steps=3, **kw)
    assert took[0] is False
    _assert_state_equal("prioritized", on, off, 3)


def test_gate_loss_fuse_records_parent_schedule(monkeypatch):
    monkeypatch.setenv("TAC_AMD_LOSS_FUSE", "1")
    on, took = _run(monkeypatch, "1", FLAGSHIP)
    off, _ = _run(monkeypatch, "0", FLAGSHIP)
    assert took == (False, False)
    _assert_state_equal("loss fuse", on, off, 5)


@pytest.mark.parametrize("M,K,nz", [(129, 64, 2), (64, 257, 2), (64, 64, 1)],
                         ids=["M129", "K257", "nz1"])
def test_folded_bindings_refuse_outside_the_gate(ext, M, K, nz):
    N = 8
    tq = kr.qloss_inputs(M, K)
    d = {k: v.to(DEV) for k, v in tq.items()}
    ws, masks = _gemm_operands(M, N, K, 0)
    rows = [d["wt0"], d["wt1"]][:nz]
    o = _outputs(M, N, K, N, True)
    ys = [o["y0"], o["y1"]][:nz]
    before = {k: v.clone() for k, v in o.items() if k != "ctrs"}
    with pytest.raises(RuntimeError, match="mgemm_r1_qloss"):
        ext.mgemm_r1_qloss(
            d["q1"], d["q2"], d["q1t"], d["q2t"], d["logp"], d["rew"],
            d["done"], None, H["alpha"], o["loss"], o["dq1"][:M],
            o["dq2"][:M], H["gamma"], H["scale"], *o["ctrs"], rows,
            ws[:nz], ys, masks[:nz], [o["outer0"], o["outer1"]][:nz],
            M, N, K, N)
    with pytest.raises(RuntimeError, match="mgemm_r1_piloss"):
        ext.mgemm_r1_piloss(
            d["q1"], d["q2"], d["logp"], None, H["alpha"], o["loss"],
            o["mean"], o["dq1"][:M], o["dq2"][:M], rows, ws[:nz], ys,
            masks[:nz], M, N, K, N)
    torch.cuda.synchronize()
    for k, v in before.items():      # a refused call touches nothing
        assert torch.equal(o[k], v), k
    assert [int(c) for c in o["ctrs"]] == list(CTR0)
    assert ext.mgemm_r1_fold_ok(64, 64) and ext.mgemm_r1_fold_ok(128, 256)
    assert not ext.mgemm_r1_fold_ok(129, 64)
    assert not ext.mgemm_r1_fold_ok(64, 257)
