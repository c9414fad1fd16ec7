"""N-step gathers (replay_sample_into_n and gather2n: the flat and concat
instantiations of replay_draw.h::gather_kernel<Draw::UniformN>) against
``ReplayBuffer.sample_at`` on the ring fixture of tests/test_nstep.py.

``state[:, 0]`` of a sampled row is the global step t, so the slot the
kernel drew is ``t % 48`` and the reference is ``sample_at`` at exactly
those slots.  With gamma = 0.5 and small-integer rewards every product
and partial sum is exactly representable in fp32, so fused and unfused
arithmetic agree and the comparison is exact equality."""

from copy import deepcopy

import numpy as np
import pytest
import torch

from test_nstep import (ACT, KIND_T, N, OBS, RING, T_TOTAL, frac_reward,
                        make_ring, transitions, window_kinds)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("states", "actions", "rewards", "next_states", "done")


def _slots(t_col):
    return (t_col.round().long() % RING)


def _assert_batch_equal(got, ref):
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(ref, f)), f


def test_replay_sample_n_exact():
    buf = make_ring(DEV, gamma=0.5)
    b = buf.sample(1024)
    torch.cuda.synchronize()
    assert int(buf._philox.item()) == 1
    ref = buf.sample_at(_slots(b.states[:, 0]), N)
    _assert_batch_equal(b, ref)
    # input condition: every window kind is among the drawn rows
    kinds = window_kinds(b.states[:, 0].cpu(),
                         (b.next_states[:, 0] - 1000).cpu())
    assert kinds == set(KIND_T), kinds
    # same counter, 1-step kernel: the same slots are drawn
    buf.set_n_step(1, 0.5)
    buf._philox.zero_()
    b1 = buf.sample(1024)
    assert torch.equal(b1.states, b.states)
    _assert_batch_equal(b1, buf.sample_at(_slots(b.states[:, 0]), 1))


def test_replay_sample_into_n_exact():
    buf = make_ring(DEV, gamma=0.5)
    out = buf.make_static_batch(333)
    buf.sample_into(out)
    torch.cuda.synchronize()
    _assert_batch_equal(out, buf.sample_at(_slots(out.states[:, 0]), N))


def test_replay_sample_n_general_gamma():
    """gamma = 0.99, non-integer rewards.  Copies are exact.  The kernel
    and the reference both form gamma^m by repeated fp32 multiply, round
    each product and add in ascending m; the only licence the kernel has
    is fusing a multiply into the following add.  One fused-vs-unfused
    step differs by at most one rounding, 2^-24 relative to the magnitude
    of the running value, which never exceeds S = sum_m |gamma^m r_m|
    (resp. 1 + gamma^(M-1) for done_eff = 1 - gamma^(M-1) (1 - d)); there
    are at most n such steps in the sum and n in the discount chain, and
    each rounding can be counted on both sides: 4 n 2^-24 S."""
    gamma = 0.99
    buf = make_ring(DEV, gamma=gamma, reward=frac_reward)
    b = buf.sample(1024)
    torch.cuda.synchronize()
    ref = buf.sample_at(_slots(b.states[:, 0]), N)
    for f in ("states", "actions", "next_states"):
        assert torch.equal(getattr(b, f), getattr(ref, f)), f
    t0 = b.states[:, 0].cpu().numpy().astype(np.int64)
    t1 = (b.next_states[:, 0] - 1000).cpu().numpy().astype(np.int64)
    r = np.array([frac_reward(t) for t in range(T_TOTAL)], dtype=np.float64)
    S = np.array([sum(abs(gamma ** m * r[a + m]) for m in range(z - a + 1))
                  for a, z in zip(t0, t1)])
    eps = 4 * N * 2.0 ** -24
    d_rew = (b.rewards - ref.rewards).abs().cpu().numpy().astype(np.float64)
    d_done = (b.done - ref.done).abs().cpu().numpy().astype(np.float64)
    print("max |d reward| / bound:", float((d_rew / (eps * S + 1e-300)).max()),
          " max |d done| / bound:",
          float((d_done / (eps * (1 + gamma ** (t1 - t0)))).max()))
    assert (d_rew <= eps * S).all()
    assert (d_done <= eps * (1 + gamma ** (t1 - t0))).all()
    # and the values are what float64 says, to fp32 accuracy
    np.testing.assert_allclose(
        b.rewards.cpu().numpy(),
        [sum(gamma ** m * r[a + m] for m in range(z - a + 1))
         for a, z in zip(t0, t1)], rtol=0, atol=float(eps * S.max()))


def test_sample_n_empty_ring_reads_slot_zero_only():
    buf = make_ring(DEV, gamma=0.5, total=0)
    assert buf.size == 0
    b = buf.sample(64)
    torch.cuda.synchronize()
    assert float(b.rewards.abs().sum()) == 0.0
    assert torch.equal(b.done, torch.zeros_like(b.done))
    assert float(b.next_states.abs().sum()) == 0.0


def _models(buf, batch, hidden=(64, 64)):
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    torch.manual_seed(11)
    device = torch.device(DEV)
    O, A = buf.obs_dim, buf.act_dim
    actor = Actor(O, A, list(hidden), act_limit=1.0).to(device)
    critic = DoubleCritic(O, A, list(hidden)).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)
    sac = SAC(alpha=0.2, gamma=buf.gamma, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=batch, start_steps=0, steps_per_epoch=1,
              max_ep_len=100, update_after=0, update_every=1, save_every=10,
              n_step=buf.n_step)
    return sac, actor, critic, target, pi_opt, q_opt, target_flat


def _engine(buf, batch, capture=False, seed=3):
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    sac, actor, critic, target, pi_opt, q_opt, target_flat = \
        _models(buf, batch)
    return FusedSACEngine(sac, actor, critic, target, buf, pi_opt, q_opt,
                          target_flat, batch, torch.device(DEV), sample=True,
                          capture=capture, philox_seed=seed)


def _assert_engine_rows(eng, buf, n):
    """XC / XC2 / rew / done of the engine against sample_at(slots, n)."""
    B, O, OC = eng.B, eng.O, eng.OC
    XC, XC2 = eng.XC.clone(), eng.XC2.clone()
    ref = buf.sample_at(_slots(XC[:B, 0]), n)
    assert torch.equal(XC[:B, :O], ref.states)
    assert torch.equal(XC[:B, O:OC], ref.actions)
    assert torch.equal(XC[B:, :O], ref.next_states)
    assert torch.equal(XC2[:, :O], ref.states)
    assert torch.equal(eng.rew, ref.rewards)
    assert torch.equal(eng.done, ref.done)
    assert eng.OCp > OC
    assert float(XC[:, OC:].abs().sum()) == 0.0     # pad columns stay 0
    assert float(XC2[:, OC:].abs().sum()) == 0.0
    return XC, ref


@pytest.mark.parametrize("obs_dim,act_dim,batch",
                         [(OBS, ACT, 256), (300, 17, 64)])
def test_gather2n_engine_step(obs_dim, act_dim, batch):
    """One uncaptured engine step launches gather2n; (300, 17) covers the
    strided row copy (obs_dim > block) and the odd padded stride."""
    buf = make_ring(DEV, gamma=0.5, obs_dim=obs_dim, act_dim=act_dim)
    eng = _engine(buf, batch)
    assert (eng.OC, eng.OCp) == ((14, 16) if obs_dim == OBS else (317, 320))
    eng.step()
    torch.cuda.synchronize()
    assert int(eng.ctr.item()) == 1
    XC, ref = _assert_engine_rows(eng, buf, N)
    assert (ref.next_states[:, 0] - 1000 != ref.states[:, 0]).any()
    # same counter value, the 1-step kernel: identical slots
    buf.set_n_step(1, 0.5)
    eng._gather(0)
    torch.cuda.synchronize()
    assert torch.equal(eng.XC[:batch, 0], XC[:batch, 0])
    ref1 = buf.sample_at(_slots(XC[:batch, 0]), 1)
    assert torch.equal(eng.rew, ref1.rewards)
    assert torch.equal(eng.XC[batch:, :obs_dim], ref1.next_states)


def test_gather2n_captured_sees_later_stores():
    buf = make_ring(DEV, gamma=0.5)
    eng = _engine(buf, 256, capture=True)
    assert eng.graph is not None
    eng.step()
    torch.cuda.synchronize()
    _assert_engine_rows(eng, buf, N)
    # 5 more transitions after capture: t = 60..64 land in slots 12..16
    s, a, r, ns = transitions(T_TOTAL + 5)
    lo = T_TOTAL
    buf.store_batch(s[lo:], a[lo:], r[lo:], ns[lo:], np.zeros(5),
                    np.zeros(5))
    assert buf.ptr == 17
    eng.step()
    torch.cuda.synchronize()
    XC, ref = _assert_engine_rows(eng, buf, N)
    t_last = ref.next_states[:, 0] - 1000
    assert float(t_last.max()) == T_TOTAL + 4       # new data is sampled,
    assert float(XC[:256, 0].min()) >= 17           # t=12..16 is gone,
    # and the old newest slot (t=59) no longer stops a window
    assert ((XC[:256, 0] == 58) & (t_last == 61)).any()


def test_autograd_graph_batch_is_nstep():
    from torch_actor_critic_amd.algo.graph import GraphedSACUpdate
    buf = make_ring(DEV, gamma=0.5)
    sac, actor, critic, target, pi_opt, q_opt, target_flat = \
        _models(buf, 128)
    g =GraphedSACUpdate(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, 128, torch.device(DEV))
    g.step()
    torch.cuda.synchronize()
    b = g.batch
    _assert_batch_equal(b, buf.sample_at(_slots(b.states[:, 0]), N))
    assert (b.next_states[:, 0] - 1000 != b.states[:, 0]).any()


def test_sac_train_nstep_gpu(monkeypatch):
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    from torch_actor_critic_amd.algo.sac import SAC
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.ops import require_extension
    from torch_actor_critic_amd.optim import FlatAdam

    ext = require_extension()
    calls = {"gather2n": 0, "gather2": 0}
    real_n, real_1 = ext.gather2n, ext.gather2

    def gather2n(*a, **k):
        calls["gather2n"] += 1
        return real_n(*a, **k)

    def gather2(*a, **k):
        calls["gather2"] += 1
        return real_1(*a, **k)

    monkeypatch.setattr(ext, "gather2n", gather2n)
    monkeypatch.setattr(ext, "gather2", gather2)

    device = torch.device(DEV)
    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor = Actor(3, 1, [64, 64], act_limit=2.0).to(device)
    critic = DoubleCritic(3, 1, [64, 64]).to(device)
    buf = ReplayBuffer(1000, 3, 1, device=device)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=64, start_steps=100, steps_per_epoch=300,
              max_ep_len=100, update_after=100, update_every=50,
              save_every=10, n_step=3)
    m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                  FlatAdam(critic), render=False, logging=False)
    assert isinstance(sac._graph, FusedSACEngine)
    assert sac._graph.buffer.n_step == 3
    assert calls["gather2n"] >= 1 and calls["gather2"] == 0
    assert np.isfinite(m["loss_q"]) and np.isfinite(m["loss_pi"])
    assert m["loss_q"] != 0.0
    assert torch.nonzero(buf.episode_end).flatten().tolist() == \
        [99, 199, 299]
    assert int(buf._ptr_dev.item()) == 300
