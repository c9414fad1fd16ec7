"""Prioritized-replay kernels against their plain-torch definitions:
``per_sample`` / ``gather2p`` against ``ReplayBuffer.draw``, ``per_update`` /
``per_set_range`` against the halving-order tree and float64 leaves, the
weighted ``qloss2`` against float64, and the engine schedule on the n-step
ring fixture of tests/test_nstep.py.

The definitions run on a CPU twin holding a copy of the GPU tree, so the
expected values come from IEEE fp32 arithmetic in the documented order."""

from copy import deepcopy

import numpy as np
import pytest
import torch

import test_nstep
from test_nstep import ACT, OBS, RING, T_TOTAL, transitions
from test_per import (assert_tree_consistent, fill, make_per,
                      random_priorities, set_leaves)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


def _twin(buf):
    """CPU buffer with a copy of buf's tree, scalars and ring."""
    tw = deepcopy(buf)
    for name, val in vars(buf).items():
        if isinstance(val, torch.Tensor):
            setattr(tw, name, val.detach().cpu().clone())
    tw.device = torch.device("cpu")
    off = 0
    tw._per_pad = []
    for n in tw._per_n:
        pad = -(-n // 64) * 64
        tw._per_pad.append(tw._per_tree[off:off + pad])
        off += pad
    return tw


def _pow_tol(x32, expo):
    """4x the largest relative error of fp32 torch.pow on the GPU against
    float64 on the same inputs, floor 2^-22."""
    got = torch.pow(x32, expo).double()
    ref = x32.double() ** float(expo)
    rel = float(((got - ref).abs() / ref.abs()).max())
    return max(4 * rel, 2.0 ** -22)


# -- per_sample == draw -----------------------------------------------------

SAMPLE_CASES = [(48, 1, 64), (48, 1, 333), (200, 2, 64), (200, 2, 333),
                (5000, 3, 64), (5000, 3, 333), (262_214, 4, 1024)]


@pytest.mark.parametrize("kind", ["integer", "fp32"])
@pytest.mark.parametrize("size,L,B", SAMPLE_CASES)
def test_per_sample_matches_draw(size, L, B, kind):
    buf = make_per(size, DEV, obs_dim=1)
    assert buf._per_L == L
    if kind == "integer":
        g = torch.Generator().manual_seed(size + B)
        p = torch.randint(0, 5, (size,), generator=g).float()
        p[torch.randperm(size, generator=g)[:size // 4]] = 0.0
    else:
        p = random_priorities(size, size + B)
    set_leaves(buf, p.to(DEV))
    tw = _twin(buf)
    assert_tree_consistent(tw)
    idx, prob, u = _ext().per_sample(buf._per_tree, size, buf._philox,
                                     buf._philox_seed, B)
    torch.cuda.synchronize()
    assert int(buf._philox.item()) == 1
    assert idx.dtype == torch.int64 and idx.shape == prob.shape == (B,)
    want_idx, want_prob = tw.draw(u.cpu())
    assert torch.equal(idx.cpu(), want_idx)
    assert torch.equal(prob.cpu(), want_prob)
    assert (p[idx.cpu()] > 0).all()
    assert torch.equal(buf.draw(u)[0], idx)     # the definition on the GPU
    if kind == "integer":
        cum = torch.cumsum(p.long(), 0)
        # targets are not integers: the slot holds floor(u) as an integer
        want = torch.searchsorted(cum, u.cpu().floor().long(), right=True)
        inside = u.cpu() < float(cum[-1])       # u may round up to the root
        assert inside.sum() >= B - 1
        assert torch.equal(idx.cpu()[inside], want[inside])
    # the exported u obeys its definition: stratum j.  The bounds are the
    # fp32 products: u = fl(fl(j + u01) * seg) with j <= fl(j + u01) <= j + 1
    # and rounding is monotone, so fl(j * seg) <= u <= fl((j + 1) * seg)
    root = tw.per_levels()[0][0]
    seg = root / torch.tensor(float(B))
    j = torch.arange(B, dtype=torch.float32)
    assert (u.cpu() >= j * seg).all() and (u.cpu() <= (j + 1) * seg).all()
    _, _, u2 = _ext().per_sample(buf._per_tree, size, buf._philox,
                                 buf._philox_seed, B)
    assert int(buf._philox.item()) == 2
    assert (u2 != u).float().mean() > 0.9       # a fresh u01 per counter
    assert (u2.cpu() >= j * seg).all() and (u2.cpu() <= (j + 1) * seg).all()


def test_per_sample_empty_tree():
    buf = make_per(200, DEV, obs_dim=1)
    idx, prob, u = _ext().per_sample(buf._per_tree, 200, buf._philox, 0, 64)
    assert idx.tolist() == [0] * 64 and prob.tolist() == [1.0] * 64
    assert u.tolist() == [0.0] * 64


def test_frequencies_follow_priorities():
    """200 slots with priorities 1 + (i % 4), B = 250: root 500, segment
    width exactly 2, 400 draws.  A slot overlaps at most 3 segments, so its
    count has variance <= 400 * 0.75, sigma <= 17.4; the bound is 6 sigma
    and adjacent priority classes are 200 apart."""
    buf = make_per(200, DEV, obs_dim=1)
    p = 1.0 + (torch.arange(200) % 4).float()
    set_leaves(buf, p.to(DEV))
    assert float(buf.per_levels()[0]) == 500.0
    counts = torch.zeros(200, dtype=torch.long, device=DEV)
    ext = _ext()
    for _ in range(400):
        idx, _, _ = ext.per_sample(buf._per_tree, 200, buf._philox, 5, 250)
        counts += torch.bincount(idx, minlength=200)
    dev = (counts.cpu().double() - 200 * p.double()).abs()
    print("largest deviation:", float(dev.max()))
    assert int(counts.sum()) == 400 * 250
    assert (dev <= 104).all()


def test_replay_sample_p_gathers_drawn_slots():
    buf = make_per(200, DEV, obs_dim=5, act_dim=2)
    fill(buf, 230)
    buf.update_priorities(torch.arange(200, device=DEV),
                          torch.arange(200, device=DEV).float() % 7)
    buf.set_beta(0.5)
    tw = _twin(buf)
    b = buf.sample(333)
    ref = buf.sample_at(b.indices)
    for f in ("states", "actions", "rewards", "next_states", "done"):
        assert torch.equal(getattr(b, f), getattr(ref, f)), f
    prob = tw.per_levels()[-1][b.indices.cpu()] / tw.per_levels()[0][0]
    w = (200 * prob.double()) ** -0.5
    np.testing.assert_allclose(b.weights.cpu().numpy(),
                               (w / w.max()).numpy(), rtol=1e-5)
    out = buf.make_static_batch(64)
    buf.sample_into(out)
    assert torch.equal(out.states, buf.state[out.indices])
    assert float(out.weights.max()) == 1.0


# -- per_update / per_set_range ------------------------------------------------

@pytest.mark.parametrize("size,B", [(48, 64), (200, 64), (5000, 64),
                                    (5000, 1024), (5000, 1500)])
def test_per_update_and_set_range_tree(size, B):
    alpha, eps = 0.6, 1e-6
    buf = make_per(size, DEV, alpha=alpha, eps=eps)
    n = {48: 60, 200: 230, 5000: 4990}[size]
    fill(buf, n, chunk=50)                     # 48 / 200: a range wraps
    torch.cuda.synchronize()
    assert_tree_consistent(buf)
    leaves = buf.per_levels()[-1]
    written = min(n, size)
    assert torch.equal(leaves[:written].cpu(), torch.ones(written))
    assert float(leaves[written:].abs().sum()) == 0.0
    before = leaves.cpu().clone()

    g = torch.Generator().manual_seed(size + B)
    idx = torch.randint(0, written, (B,), generator=g)
    idx[B // 2:B // 2 + 8] = idx[:8]           # duplicates for certain: in
    idx[-3:] = idx[0]                          # a wave, across waves and
    #                                            (B = 1500) across chunks
    td = torch.rand(B, generator=g) * 20
    td[::7] = 0.0
    buf.update_priorities(idx.to(DEV), td.to(DEV))
    torch.cuda.synchronize()
    assert_tree_consistent(buf)                # exact, from kernel's leaves

    a32, e32 = np.float32(alpha), np.float32(eps)
    x32 = td.to(DEV) + float(e32)
    tol = _pow_tol(x32, float(a32))
    p64 = (x32.double() ** float(a32)).cpu()
    winner = {}
    for pos, s in enumerate(idx.tolist()):
        winner[s] = pos                        # highest position wins
    assert len(winner) < B
    got = leaves.cpu().double()
    slots = torch.tensor(list(winner))
    want = p64[torch.tensor(list(winner.values()))]
    rel = ((got[slots] - want).abs() / want).max()
    print("pow tolerance", tol, "worst leaf error", float(rel))
    assert rel <= tol
    untouched = torch.ones(size, dtype=torch.bool)
    untouched[slots] = False
    assert torch.equal(leaves.cpu()[untouched], before[untouched])
    mp = float(buf._max_priority)
    want_mp = max(1.0, float(p64.max()))
    assert abs(mp - want_mp) <= tol * want_mp
    # the next store carries the grown max_priority, wrap included
    start = buf.ptr
    fill(buf, 20, chunk=20, t0=n)
    torch.cuda.synchronize()
    new = (start + torch.arange(20)) % size
    assert torch.equal(leaves.cpu()[new], torch.full((20,), mp))
    assert_tree_consistent(buf)
    buf.store(np.zeros(2), np.zeros(1), 0.0, np.zeros(2), 0.0)
    assert float(leaves[(start + 20) % size]) == mp
    assert_tree_consistent(buf)


# -- weighted qloss2 ----------------------------------------------------------

def _qloss_inputs(B, h2, seed):
    """Dyadic inputs: with gamma = 0.5, alpha = 0.25, scale = 2 the backup
    and both errors are exact in fp32, so the only rounding under test is
    the weight's pow and the products that follow it."""
    g = torch.Generator().manual_seed(seed)
    r8 = lambda: (torch.randint(-40, 41, (B,), generator=g).float() / 8)
    # the backup is a multiple of 1/64, q an odd multiple of 1/128: e != 0
    t = dict(q1=r8() + 1 / 128, q2=r8() - 1 / 128, q1t=r8(), q2t=r8(),
             logp=r8(), rew=r8(),
             done=(torch.rand(B, generator=g) < 0.3).float(),
             prob=torch.rand(B, generator=g) * 0.02 + 1e-4,
             wt0=torch.randn(h2, generator=g),
             wt1=torch.randn(h2, generator=g))
    return {k: v.to(DEV) for k, v in t.items()}


def _run_qloss(t, B, h2, size, beta, weighted):
    f32 = dict(device=DEV, dtype=torch.float32)
    out = dict(loss=torch.zeros(1, **f32), dq1=torch.zeros(B, 1, **f32),
               dq2=torch.zeros(B, 1, **f32), dy0=torch.zeros(B, h2, **f32),
               dy1=torch.zeros(B, h2, **f32), td=torch.zeros(B, **f32))
    ctr = [torch.full((1,), 7, dtype=torch.int64, device=DEV)
           for _ in range(3)]
    per = ()
    if weighted:
        per = (t["prob"],
               torch.full((1,), size, dtype=torch.int64, device=DEV),
               torch.full((1,), beta, **f32), out["td"])
    _ext().qloss2(t["q1"], t["q2"], t["q1t"], t["q2t"], t["logp"], t["rew"],
                  t["done"], None, 0.25, out["loss"], out["dq1"], out["dq2"],
                  B, 0.5, 2.0, t["wt0"], t["wt1"], out["dy0"], out["dy1"],
                  h2, *ctr, *per)
    torch.cuda.synchronize()
    assert [int(c) for c in ctr] == [8, 8, 8]      # the bump still commits
    return out


@pytest.mark.parametrize("B", [64, 1000])
def test_weighted_qloss2_against_float64(B):
    h2, size = 24, 50_000
    t = _qloss_inputs(B, h2, B)
    beta32 = float(torch.tensor(0.4, dtype=torch.float32))
    out = _run_qloss(t, B, h2, size, 0.4, weighted=True)
    d = lambda x: x.double().cpu().reshape(-1)
    x32 = float(size) * t["prob"]
    tol_w = 2 * _pow_tol(x32, -beta32)         # w is a quotient of two pows
    w = x32.double().cpu() ** -beta32
    w = w / w.max()
    backup = 2.0 * d(t["rew"]) + 0.5 * (1 - d(t["done"])) * (
        torch.min(d(t["q1t"]), d(t["q2t"])) - 0.25 * d(t["logp"]))
    e1, e2 = d(t["q1"]) - backup, d(t["q2"]) - backup
    assert (e1 != 0).all() and (e2 != 0).all()
    rtol = 1e-5 + tol_w
    print("tolerance on w:", tol_w)
    assert torch.equal(d(out["td"]), 0.5 * (e1.abs() + e2.abs()))
    np.testing.assert_allclose(float(out["loss"]),
                               float((w * (e1 ** 2 + e2 ** 2)).mean()),
                               rtol=rtol)
    s1, s2 = 2 * w * e1 / B, 2 * w * e2 / B
    np.testing.assert_allclose(d(out["dq1"]).numpy(), s1.numpy(), rtol=rtol)
    np.testing.assert_allclose(d(out["dq2"]).numpy(), s2.numpy(), rtol=rtol)
    np.testing.assert_allclose(
        out["dy0"].double().cpu().numpy(),
        (s1[:, None] * d(t["wt0"])[None]).numpy(), rtol=rtol)
    np.testing.assert_allclose(
        out["dy1"].double().cpu().numpy(),
        (s2[:, None] * d(t["wt1"])[None]).numpy(), rtol=rtol)


@pytest.mark.parametrize("B", [64, 1000])
def test_weighted_qloss2_equal_probs_is_unweighted(B):
    h2 = 24
    t = _qloss_inputs(B, h2, 100 + B)
    g = torch.Generator().manual_seed(B)
    for k in ("q1", "q2", "q1t", "q2t", "logp", "rew"):   # general floats
        t[k] = torch.randn(B, generator=g).to(DEV)
    t["prob"] = torch.full((B,), 0.0123, device=DEV)
    a = _run_qloss(t, B, h2, 777, 0.7, weighted=True)
    b = _run_qloss(t, B, h2, 777, 0.7, weighted=False)
    for k in ("loss", "dq1", "dq2", "dy0", "dy1"):
        assert torch.equal(a[k], b[k]), k
    assert float(b["td"].abs().sum()) == 0.0


# -- engine ---------------------------------------------------------------------

ALPHA, EPS = 0.6, 1e-6


class _PerRing(test_nstep.ReplayBuffer):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.set_prioritized(ALPHA, EPS)


def _ring(monkeypatch, n, **kw):
    """The n-step ring fixture, prioritized, with uneven priorities."""
    monkeypatch.setattr(test_nstep, "ReplayBuffer", _PerRing)
    buf = test_nstep.make_ring(DEV, gamma=0.5, n_step=n, **kw)
    assert buf.prioritized and buf.ptr == 12 and buf.size == RING
    assert torch.equal(buf.per_levels()[-1].cpu(), torch.ones(RING))
    buf.update_priorities(torch.arange(RING, device=DEV),
                          (torch.arange(RING, device=DEV) % 5).float())
    buf.set_beta(0.4)
    return buf


def _engine(buf, batch, capture=False):
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    from test_gpu_nstep import _models
    sac, actor, critic, target, pi_opt, q_opt, target_flat = \
        _models(buf, batch)
    eng = FusedSACEngine(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, batch, torch.device(DEV), sample=True,
                         capture=capture, philox_seed=3)
    return eng, q_opt, pi_opt


def _step_and_check(eng, buf, n):
    """One engine step: rows against sample_at(eng.idx, n), probabilities
    against the tree before the step, the tree after it against
    _update_priorities_ref of the exported td."""
    tw = _twin(buf)
    eng.step()
    torch.cuda.synchronize()
    B, O, OC = eng.B, eng.O, eng.OC
    idx = eng.idx.clone()
    ref = buf.sample_at(idx, n)
    assert torch.equal(eng.XC[:B, :O], ref.states)
    assert torch.equal(eng.XC[:B, O:OC], ref.actions)
    assert torch.equal(eng.XC[B:, :O], ref.next_states)
    assert torch.equal(eng.XC2[:, :O], ref.states)
    assert torch.equal(eng.rew, ref.rewards)
    assert torch.equal(eng.done, ref.done)
    assert torch.equal(eng.XC[:B, 0].round().long() % RING, idx)
    leaves0, root0 = tw.per_levels()[-1], tw.per_levels()[0][0]
    assert torch.equal(eng.pprob.cpu(), leaves0[idx.cpu()] / root0)
    assert (leaves0[idx.cpu()] > 0).all()
    # stratified: batch position j lies in stratum j of the cumulative sum
    cum = torch.cumsum(leaves0.double(), 0)
    j = torch.arange(B, dtype=torch.float64)
    seg, slack = float(root0) / B, 64 * 2.0 ** -24 * float(root0)
    assert (cum[idx.cpu()] >= j * seg - slack).all()
    assert ((cum - leaves0.double())[idx.cpu()] <= (j + 1) * seg + slack).all()
    # the priority update
    assert_tree_consistent(buf)
    td = eng.td.clone()
    assert (td > 0).any()
    tw._update_priorities_ref(idx.cpu(), td.cpu())
    tol = _pow_tol(td + float(np.float32(EPS)), float(np.float32(ALPHA)))
    got, want = buf.per_levels()[-1].cpu().double(), \
        tw.per_levels()[-1].double()
    assert float(((got - want).abs() / want).max()) <= tol
    untouched = torch.ones(RING, dtype=torch.bool)
    untouched[idx.cpu()] = False
    assert torch.equal(got[untouched], want[untouched])
    mp, want_mp = float(buf._max_priority), float(tw._max_priority)
    assert abs(mp - want_mp) <= tol * want_mp
    return idx, ref


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("obs_dim,act_dim,batch",
                         [(OBS, ACT, 256), (300, 17, 64)])
def test_gather2p_engine_step(monkeypatch, n, obs_dim, act_dim, batch):
    buf = _ring(monkeypatch, n, obs_dim=obs_dim, act_dim=act_dim)
    eng, q_opt, pi_opt = _engine(buf, batch)
    assert eng.per
    idx, ref = _step_and_check(eng, buf, n)
    assert int(eng.ctr.item()) == 1                 # counters advanced once
    assert int(q_opt.step_t.item()) == 1 and int(pi_opt.step_t.item()) == 1
    if n > 1:
        assert (ref.next_states[:, 0] - 1000 != ref.states[:, 0]).any()
    _step_and_check(eng, buf, n)
    assert int(eng.ctr.item()) == 2


def test_gather2p_captured_sees_later_stores(monkeypatch):
    buf = _ring(monkeypatch, 3)
    eng, _, _ = _engine(buf, 256, capture=True)
    assert eng.graph is not None
    _step_and_check(eng, buf, 3)
    # 5 more transitions after capture: t = 60..64 land in slots 12..16
    s, a, r, ns = transitions(T_TOTAL + 5)
    lo = T_TOTAL
    buf.store_batch(s[lo:], a[lo:], r[lo:], ns[lo:], np.zeros(5),
                    np.zeros(5))
    torch.cuda.synchronize()
    mp = float(buf._max_priority)
    assert buf.per_levels()[-1][12:17].tolist() == [mp] * 5
    assert mp == float(buf.per_levels()[-1].max())
    assert_tree_consistent(buf)
    buf.set_beta(1.0)                                # seen by the replay
    idx, ref = _step_and_check(eng, buf, 3)
    assert float(eng.XC[:256, 0].max()) >= T_TOTAL   # new data is sampled
    assert float((ref.next_states[:, 0] - 1000).max()) == T_TOTAL + 4


def test_sac_train_per_gpu(monkeypatch):
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    from torch_actor_critic_amd.algo.sac import SAC
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam

    ext = _ext()
    calls = {"gather2p": 0, "gather2n": 0, "gather2": 0}

    def counted(name):
        real = getattr(ext, name)

        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return fn

    for name in calls:
        monkeypatch.setattr(ext, name, counted(name))

    device = torch.device(DEV)
    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor = Actor(3, 1, [64, 64], act_limit=2.0).to(device)
    critic = DoubleCritic(3, 1, [64, 64]).to(device)
    buf = ReplayBuffer(1000, 3, 1, device=device)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=64, start_steps=100, steps_per_epoch=300,
              max_ep_len=100, update_after=100, update_every=50,
              save_every=10, n_step=3, per=True)
    m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                  FlatAdam(critic), render=False, logging=False)
    assert isinstance(sac._graph, FusedSACEngine) and sac._graph.per
    assert calls["gather2p"] >= 1
    assert calls["gather2"] == 0 and calls["gather2n"] == 0
    assert np.isfinite(m["loss_q"]) and np.isfinite(m["loss_pi"])
    assert m["loss_q"] != 0.0
    assert float(buf._beta_dev) == 1.0
    levels = buf.per_levels()
    leaves = levels[-1][:300]
    assert (leaves > 0).all() and float(leaves.min()) != float(leaves.max())
    assert float(levels[-1][300:].abs().sum()) == 0.0
    assert_tree_consistent(buf)      # the root is the sum of its level


def test_sac_train_per_gpu_eager_fallback(caplog):
    """No fused engine (here: the reference's next-state policy loss): the
    autograd-captured update must not be chosen for a prioritized buffer;
    training runs eager updates on the prioritized GPU samplers."""
    import logging
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.algo.sac import SAC
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam

    device = torch.device(DEV)
    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor = Actor(3, 1, [32, 32], act_limit=2.0).to(device)
    critic = DoubleCritic(3, 1, [32, 32]).to(device)
    buf = ReplayBuffer(1000, 3, 1, device=device)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=32, start_steps=100, steps_per_epoch=200,
              max_ep_len=100, update_after=100, update_every=50,
              save_every=10, n_step=3, per=True, reference_pi_loss=True)
    with caplog.at_level(logging.INFO):
        m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                      FlatAdam(critic), render=False, logging=False)
    assert sac._graph is None and sac._graph_failed
    assert sum("prioritized replay" in r.getMessage()
               for r in caplog.records) == 1            # one log line
    assert np.isfinite(m["loss_q"]) and m["loss_q"] != 0.0
    leaves = buf.per_levels()[-1][:200]
    assert (leaves > 0).all() and float(leaves.min()) != float(leaves.max())
    assert_tree_consistent(buf)
