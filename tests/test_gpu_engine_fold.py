"""The three launch folds of the fused SAC engine (Adam in the wgrad
launch, the counter bump committed by qloss2, the rank-1 A operand of the
pi-phase dgrad) against the same engine with all three switched off."""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, O, A = 64, 11, 3          # OC = 14, padded stride 16 (OCp != OC)
ALPHA, GAMMA, POLYAK, SCALE = 0.2, 0.99, 0.995, 1.0
FLAGS = ("TAC_AMD_WGRAD_ADAM", "TAC_AMD_BUMP_FOLD", "TAC_AMD_R1_DGRAD")


@pytest.fixture(autouse=True)
def _fp32_mode():
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("fp32")
    yield
    Fo.set_compute_dtype("fp32")


def _build(monkeypatch, hid, fold, sample=False, capture=False, seed=0,
           fill=None, adam_default=False):
    """An engine (and everything it updates) from fixed initial state."""
    from copy import deepcopy
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    for f in FLAGS:
        monkeypatch.setenv(f, "1" if fold else "0")
    if adam_default:
        monkeypatch.delenv("TAC_AMD_WGRAD_ADAM")
    torch.manual_seed(11)
    device = torch.device(DEV)
    actor = Actor(O, A, hid, act_limit=1.0).to(device)
    critic = DoubleCritic(O, A, hid).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)
    buf = ReplayBuffer(4096, O, A, device=device)
    if fill is not None:
        rng = np.random.default_rng(fill)
        buf.store_batch(rng.standard_normal((512, O)).astype(np.float32),
                        rng.standard_normal((512, A)).astype(np.float32),
                        rng.standard_normal(512).astype(np.float32),
                        rng.standard_normal((512, O)).astype(np.float32),
                        np.zeros(512, dtype=np.float32))
    sac = SAC(alpha=ALPHA, gamma=GAMMA, polyak=POLYAK, reward_scale=SCALE,
              epochs=1, batch_size=B, start_steps=0, steps_per_epoch=1,
              max_ep_len=100, update_after=0, update_every=1, save_every=10)
    eng = FusedSACEngine(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, B, device, sample=sample,
                         capture=capture, philox_seed=seed)
    assert eng._bump_fold == fold and eng._r1_dgrad == fold
    assert eng._wgrad_adam == fold
    return dict(eng=eng, actor=actor, critic=critic, target=target,
                pi_opt=pi_opt, q_opt=q_opt, target_flat=target_flat)


def _batch():
    g = torch.Generator().manual_seed(5)
    s = torch.randn(B, O, generator=g)
    a = torch.rand(B, A, generator=g) * 2 - 1
    r = torch.randn(B, generator=g)
    ns = torch.randn(B, O, generator=g)
    d = (torch.rand(B, generator=g) > 0.9).float()
    return s, a, r, ns, d


def _one_update(e):
    e["eng"].load_batch(*[t.to(DEV) for t in _batch()])
    e["eng"]._run_once()
    torch.cuda.synchronize()


@pytest.mark.parametrize("hid", [[64, 64], [64]])
def test_folded_update_matches_unfolded_fp32(monkeypatch, hid):
    on = _build(monkeypatch, hid, True)
    off = _build(monkeypatch, hid, False)
    _one_update(on)
    _one_update(off)
    # the folds took effect: both Adam steps rode in the wgrad launches
    assert on["eng"]._adam_fused == {id(on["q_opt"]): True,
                                     id(on["pi_opt"]): True}
    assert not any(off["eng"]._adam_fused.values())

    # same noise drawn (ctr+1 read ahead of the commit == bumped ctr)
    assert torch.equal(on["eng"].prob, off["eng"].prob)
    for k in ("q_opt", "pi_opt"):
        g_on, g_off = on[k].fp.flat_grad, off[k].fp.flat_grad
        assert g_off.abs().max() > 0
        assert torch.allclose(g_on, g_off, atol=5e-5, rtol=1e-3), \
            (k, (g_on - g_off).abs().max())
        for name, x, y in (("p", on[k].fp.flat, off[k].fp.flat),
                           ("m", on[k].m, off[k].m),
                           ("v", on[k].v, off[k].v)):
            assert torch.allclose(x, y, atol=1e-6, rtol=0), \
                (k, name, (x - y).abs().max())
        assert int(on[k].step_t.item()) == int(off[k].step_t.item()) == 1
    assert torch.allclose(on["target_flat"], off["target_flat"], atol=1e-6,
                          rtol=0)
    assert int(on["eng"].ctr.item()) == int(off["eng"].ctr.item()) == 1
    # the W^T caches follow the updated weights exactly
    eng = on["eng"]
    for w, wt in zip(eng._c_tr_src + eng._a_tr_src,
                     eng._c_tr_dst + eng._a_tr_dst):
        assert torch.equal(wt, w.detach().t())


@pytest.mark.parametrize("hid", [[64, 64], [64]])
def test_folded_update_bf16_no_worse_than_unfolded(monkeypatch, hid):
    """No bf16 gradient tolerance is coded for the engine, so both engines
    are held against the eager fp32 update: the rank-1 operand rounds to
    bf16 once where the K=1 launch + restaging rounded twice, so folding
    must not move the gradients further from fp32.  The error is the
    relative L2 distance over a whole flat gradient — single elements move
    either way when a rounding is removed, the norm is what may not grow."""
    import test_gpu_engine as base
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.ops import require_extension
    ext = require_extension()

    errs, engs = {}, {}
    for fold in (True, False):
        e = engs[fold] = _build(monkeypatch, hid, fold)
        cpu = [copy.deepcopy(e[k]).cpu()
               for k in ("actor", "critic", "target")]
        Fo.set_compute_dtype("bf16")
        try:
            _one_update(e)
        finally:
            Fo.set_compute_dtype("fp32")
        eps = ext.tg_eps(1, 0, 2 * B, A, e["eng"].prob).cpu()
        assert (base.B, base.ALPHA, base.GAMMA, base.SCALE) == \
            (B, ALPHA, GAMMA, SCALE)
        ref = base._eager_reference(*cpu, *_batch(), eps)
        for k, rk in (("q_opt", "cgrad"), ("pi_opt", "agrad")):
            g = e[k].fp.flat_grad.cpu()
            errs[(fold, rk)] = float((g - ref[rk]).norm() / ref[rk].norm())
    print("bf16 relative L2 grad error vs eager fp32:", errs)
    for rk in ("cgrad", "agrad"):
        assert errs[(True, rk)] <= 1.10 * errs[(False, rk)], errs

    # State after the update, folded against unfolded, in the mode the
    # flagship runs: bf16 at batch 64 does not split along M, so the Adam
    # step rode in the quarter-tile epilogue.  Same bounds as the fp32
    # case.  They hold in bf16 because dqp is -1/B, -1/(2B) or 0, powers
    # of two at B = 64: rounding dqp * w once gives the same bf16 value
    # as rounding w and scaling, so the gradients do not move at all.
    on, off = engs[True], engs[False]
    assert on["eng"]._adam_fused == {id(on["q_opt"]): True,
                                     id(on["pi_opt"]): True}
    assert torch.equal(on["eng"].prob, off["eng"].prob)
    for k in ("q_opt", "pi_opt"):
        g_on, g_off = on[k].fp.flat_grad, off[k].fp.flat_grad
        assert torch.allclose(g_on, g_off, atol=5e-5, rtol=1e-3), \
            (k, (g_on - g_off).abs().max())
        for name, x, y in (("p", on[k].fp.flat, off[k].fp.flat),
                           ("m", on[k].m, off[k].m),
                           ("v", on[k].v, off[k].v)):
            assert torch.allclose(x, y, atol=1e-6, rtol=0), \
                (k, name, (x - y).abs().max())
        assert int(on[k].step_t.item()) == int(off[k].step_t.item()) == 1
    assert torch.allclose(on["target_flat"], off["target_flat"], atol=1e-6,
                          rtol=0)
    eng = on["eng"]
    for w, wt in zip(eng._c_tr_src + eng._a_tr_src,
                     eng._c_tr_dst + eng._a_tr_dst):
        assert torch.equal(wt, w.detach().t())


def test_folded_captured_replay_advances_and_is_deterministic(monkeypatch):
    results = []
    for _ in range(2):
        e = _build(monkeypatch, [64, 64], True, sample=True, capture=True,
                   seed=99, fill=17)
        eng = e["eng"]
        assert eng.graph is not None
        ctr0 = int(eng.ctr.item())
        q0 = int(e["q_opt"].step_t.item())
        p0 = int(e["pi_opt"].step_t.item())
        for _ in range(5):
            eng.step()
        torch.cuda.synchronize()
        assert int(eng.ctr.item()) == ctr0 + 5
        assert int(e["q_opt"].step_t.item()) == q0 + 5
        assert int(e["pi_opt"].step_t.item()) == p0 + 5
        results.append((e["pi_opt"].fp.flat.clone(),
                        e["q_opt"].fp.flat.clone(),
                        e["target_flat"].clone()))
        assert all(torch.isfinite(x).all() for x in results[-1])
    for x, y in zip(*results):
        assert torch.equal(x, y)


class _CountingExt:
    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def counted(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return counted


# launcher calls of one sampled, fixed-alpha update: [64, 64] is the
# flagship topology (26 unfolded; -2 adam_t, -1 bump3, -1 K=1 dgrad), one
# hidden layer has 3 fewer forward/dgrad launches per network pair
@pytest.mark.parametrize("hid,fold,want", [
    ([64, 64], True, 22), ([64, 64], False, 26),
    ([64], True, 16), ([64], False, 20)])
def test_launch_count(monkeypatch, hid, fold, want):
    e = _build(monkeypatch, hid, fold, sample=True, fill=3)
    eng = e["eng"]
    eng._run_once()              # settles the per-optimizer coverage gate
    eng.ext = _CountingExt(eng.ext)
    eng._run_once()
    torch.cuda.synchronize()
    calls = eng.ext.calls
    assert len(calls) == want, calls
    assert ("adam_t" in calls) == (not fold)
    assert ("bump3" in calls) == (not fold)
    assert calls.count("mgemm_r1") == (1 if fold else 0)


@pytest.mark.parametrize("dtype,fused", [("fp32", True), ("bf16", False)])
def test_default_folds_adam_only_where_the_wgrad_splits(monkeypatch, dtype,
                                                        fused):
    """Unset, TAC_AMD_WGRAD_ADAM folds Adam into the split-M combine (fp32
    at batch 64: four 16-row slabs) and leaves the un-split bf16 launch
    its adam_t."""
    from torch_actor_critic_amd.ops import functional as Fo
    on = _build(monkeypatch, [64, 64], True)
    auto = _build(monkeypatch, [64, 64], True, adam_default=True)
    assert auto["eng"]._wgrad_adam and not auto["eng"]._wgrad_adam_unsplit
    Fo.set_compute_dtype(dtype)
    try:
        _one_update(on)
        auto["eng"].ext = _CountingExt(auto["eng"].ext)
        _one_update(auto)
    finally:
        Fo.set_compute_dtype("fp32")
    calls = auto["eng"].ext.calls
    assert calls.count("adam_t") == (0 if fused else 2)
    assert calls.count("mwgrad_het_adam") == (2 if fused else 0)
    assert set(auto["eng"]._adam_fused.values()) == {fused}
    for k in ("q_opt", "pi_opt"):
        assert torch.equal(auto[k].fp.flat_grad, on[k].fp.flat_grad)
        assert torch.allclose(auto[k].fp.flat, on[k].fp.flat, atol=1e-6,
                              rtol=0)
