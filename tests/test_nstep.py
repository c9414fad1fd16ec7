"""N-step returns in replay sampling: ``ReplayBuffer.sample_at(idx, n)``
is the executable definition; these tests pin it to a hand-written table
and cover the buffer guards, the staging store, the SAC loop and the CLI.

The ring fixture built here is shared with tests/test_gpu_nstep.py:

* ``max_size=48, obs_dim=11, act_dim=3``; 60 transitions written through
  ``WindowedStore`` / ``store_batch`` in uneven chunks, so the ring is
  full and wrapped with ``ptr == 12`` (slots 0..11 hold t=48..59, slots
  12..47 hold t=12..47, the newest slot is 11).
* ``state[:, 0]`` is the global step t, ``next_state[:, 0]`` is 1000 + t,
  so sampled and bootstrap slots are recoverable from a batch.
* Episode lengths cycle 7, 5, 6 and alternately end by ``done=1`` and by
  ``end=1, done=0`` (truncation).  The stream starts 3 steps into the
  first 7-step episode: with an episode starting at t=0 the cycle puts an
  episode end exactly on slot 47 (t=47), and then no window could ever
  wrap the ring end, which is one of the window kinds under test.
  Episodes therefore end at t = 3, 8, 14, 21, 26, 32, 39, 44, 50, 57
  (done, truncated, done, ...), and t=58, 59 are an unfinished episode.
* Rewards are small integers in [-8, 8]: ``r(t) = 7 t mod 17 - 8``.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from torch_actor_critic_amd.algo.act import WindowedStore
from torch_actor_critic_amd.buffer.replay import ReplayBuffer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RING, OBS, ACT, T_TOTAL, N = 48, 11, 3, 60, 4


def episode_flags(total):
    """(done[t], end[t]) of the fixture's episode pattern."""
    done = np.zeros(total, dtype=np.float32)
    end = np.zeros(total, dtype=np.float32)
    lens, pos, ep, k = (7, 5, 6), 3, 0, 0
    for t in range(total):
        pos += 1
        if pos == lens[k]:
            end[t] = 1.0
            if ep % 2 == 0:
                done[t] = 1.0
            pos, ep, k = 0, ep + 1, (k + 1) % 3
    return done, end


def int_reward(t):
    return float((7 * t) % 17 - 8)


def frac_reward(t):
    # non-integer rewards for the general-gamma test
    return float(np.float32(np.sin(0.7 * t) * 3.3))


def transitions(total, obs_dim=OBS, act_dim=ACT, reward=int_reward):
    """Small-integer rows (exact in fp32) keyed by the global step."""
    t = np.arange(total)[:, None]
    s = ((t * 13 + np.arange(obs_dim)[None]) % 23).astype(np.float32)
    s[:, 0] = np.arange(total)
    ns = ((t * 5 + np.arange(obs_dim)[None]) % 19).astype(np.float32)
    ns[:, 0] = 1000 + np.arange(total)
    a = ((t * 3 + np.arange(act_dim)[None]) % 11 - 5).astype(np.float32)
    r = np.array([reward(i) for i in range(total)], dtype=np.float32)
    return s, a, r, ns


def make_ring(device="cpu", gamma=0.5, n_step=N, size=RING, total=T_TOTAL,
              obs_dim=OBS, act_dim=ACT, reward=int_reward):
    buf = ReplayBuffer(size, obs_dim, act_dim, device=device)
    buf.set_n_step(n_step, gamma)
    s, a, r, ns = transitions(total, obs_dim, act_dim, reward)
    done, end = episode_flags(total)
    ws = WindowedStore(buf, 9)
    for t in range(total):
        ws.store(s[t], a[t], r[t], ns[t], done[t], end[t])
        if t in (3, 20, 21, 52):     # uneven chunks: 4, 9, 8, 1, 9, ...
            ws.flush()
    ws.flush()
    return buf


# slot kinds of the fixture at n=4, by global step t of the sampled slot
KIND_T = {
    "full": 15,          # 15,16,17,18
    "terminal": 24,      # 24,25,26(done)
    "truncation": 19,    # 19,20,21(end, done=0)
    "newest_stop": 58,   # 58,59(newest)
    "wrap": 46,          # slots 46,47,0,1
    "is_newest": 59,
}


def window_kinds(t_sampled, t_last):
    """Which of the kinds above occur among sampled rows (inputs check for
    the GPU tests): classified from the fixture's layout alone."""
    done, end = episode_flags(T_TOTAL)
    kinds = set()
    for ts, tl in zip(t_sampled.tolist(), t_last.tolist()):
        ts, tl = int(ts), int(tl)
        m = tl - ts + 1
        if ts == T_TOTAL - 1:
            kinds.add("is_newest")
        elif tl == T_TOTAL - 1 and not end[tl]:
            kinds.add("newest_stop")
        elif m == N and not end[tl]:
            kinds.add("full")
        if m > 1 and done[tl]:
            kinds.add("terminal")
        if m > 1 and end[tl] and not done[tl]:
            kinds.add("truncation")
        if ts % RING > tl % RING:
            kinds.add("wrap")
    return kinds


def test_fixture_layout():
    buf = make_ring()
    assert buf.ptr == 12 and buf.size == RING
    assert int(buf._ptr_dev.item()) == 12
    assert int(buf._size_dev.item()) == RING
    want_t = np.array([48 + i if i < 12 else i for i in range(RING)])
    np.testing.assert_array_equal(buf.state[:, 0].numpy(), want_t)
    done, end = episode_flags(T_TOTAL)
    np.testing.assert_array_equal(buf.done.numpy(), done[want_t])
    np.testing.assert_array_equal(buf.episode_end.numpy(), end[want_t])
    assert [t for t in range(T_TOTAL) if end[t]] == \
        [3, 8, 14, 21, 26, 32, 39, 44, 50, 57]
    assert [t for t in range(T_TOTAL) if done[t]] == [3, 14, 26, 39, 50]
    assert buf.rewards.abs().max() <= 8


def test_sample_at_hand_table():
    """gamma = 0.5, n = 4.  r(t) for the steps used below:
    15:-5 16:2 17:-8 18:-1 19:6 20:-4 21:3 24:7 25:-3 26:4
    46:8 47:-2 48:5 49:-5 58:7 59:-3."""
    buf = make_ring(gamma=0.5)
    #        t   reward                          done_eff  t of next_state
    table = [
        (15, -5 + 0.5 * 2 + 0.25 * -8 + 0.125 * -1, 0.875, 18),   # full n
        (24, 7 + 0.5 * -3 + 0.25 * 4, 1.0, 26),         # terminal inside
        (19, 6 + 0.5 * -4 + 0.25 * 3, 0.75, 21),        # truncation inside
        (58, 7 + 0.5 * -3, 0.5, 59),                    # stops at newest
        (46, 8 + 0.5 * -2 + 0.25 * 5 + 0.125 * -5, 0.875, 49),  # wraps
        (59, -3.0, 0.0, 59),                            # i == newest
        (26, 4.0, 1.0, 26),                             # terminal itself
        (21, 3.0, 0.0, 21),                             # truncated itself
    ]
    assert table[0][1] == -6.125 and table[4][1] == 7.625
    assert [row[0] for row in table[:6]] == list(KIND_T.values())
    s, a, r, ns = transitions(T_TOTAL)
    idx = torch.tensor([row[0] % RING for row in table])
    b = buf.sample_at(idx)              # buffer default: n_step = 4
    b4 = buf.sample_at(idx, 4)
    for k, (t, rew, deff, t_ns) in enumerate(table):
        assert float(b.rewards[k]) == rew, (t, float(b.rewards[k]))
        assert float(b.done[k]) == deff, (t, float(b.done[k]))
        np.testing.assert_array_equal(b.states[k].numpy(), s[t])
        np.testing.assert_array_equal(b.actions[k].numpy(), a[t])
        np.testing.assert_array_equal(b.next_states[k].numpy(), ns[t_ns])
    for x, y in zip((b.states, b.actions, b.rewards, b.next_states, b.done),
                    (b4.states, b4.actions, b4.rewards, b4.next_states,
                     b4.done)):
        assert torch.equal(x, y)
    kinds = window_kinds(b.states[:, 0], b.next_states[:, 0] - 1000)
    assert kinds == set(KIND_T)


def test_n1_is_todays_batch():
    buf = make_ring()
    plain = ReplayBuffer(RING, OBS, ACT)
    assert plain.n_step == 1
    assert plain.episode_end is None and plain._ptr_dev is None
    s, a, r, ns = transitions(T_TOTAL)
    done, _ = episode_flags(T_TOTAL)
    for lo, hi in ((0, 4), (4, 13), (13, 60)):
        plain.store_batch(s[lo:hi], a[lo:hi], r[lo:hi], ns[lo:hi],
                          done[lo:hi])
    assert plain.episode_end is None and plain._ptr_dev is None
    idx = torch.arange(RING)
    want = (plain.state[idx], plain.actions[idx], plain.rewards[idx],
            plain.next_state[idx], plain.done[idx])
    for b in (plain.sample_at(idx), buf.sample_at(idx, 1),
              buf.sample_at(idx, n_step=1)):
        got = (b.states, b.actions, b.rewards, b.next_states, b.done)
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    # switching an n-step ring back to 1-step sampling is allowed
    buf.set_n_step(1, 0.5)
    b = buf.sample_at(idx)
    assert torch.equal(b.rewards, want[2]) and torch.equal(b.done, want[4])
    # CPU sample(): unchanged index draw, n-step applied after it
    buf.set_n_step(N, 0.5)
    buf._rng = np.random.default_rng(5)
    plain._rng = np.random.default_rng(5)
    b4, b1 = buf.sample(16), plain.sample(16)
    assert torch.equal(b4.states, b1.states)
    ref = buf.sample_at((b1.states[:, 0] % RING).long(), N)
    assert torch.equal(b4.rewards, ref.rewards)
    assert torch.equal(b4.next_states, ref.next_states)


def test_guards():
    buf = ReplayBuffer(16, 2, 1)
    for bad in (0, -1, 65):
        with pytest.raises(ValueError):
            buf.set_n_step(bad, 0.9)
    buf.set_n_step(1, 0.9)      # n=1 on anything is fine
    buf.store(np.zeros(2), np.zeros(1), 1.0, np.zeros(2), 0.0)
    buf.set_n_step(1, 0.9)
    with pytest.raises(ValueError):
        buf.set_n_step(2, 0.9)  # non-empty: no episode boundaries recorded
    assert buf.episode_end is None and buf.n_step == 1
    with pytest.raises(ValueError):
        buf.sample_at(torch.tensor([0]), 2)
    ok = ReplayBuffer(16, 2, 1)
    ok.set_n_step(64, 0.9)
    assert ok.episode_end.shape == (16,)
    assert ok.episode_end.dtype == torch.float32
    assert ok._ptr_dev.dtype == torch.int64 and ok._ptr_dev.shape == (1,)


def test_store_defaults_end_to_done_and_mirrors_ptr():
    buf = ReplayBuffer(4, 2, 1)
    buf.set_n_step(3, 0.5)
    z2, z1 = np.zeros(2), np.zeros(1)
    buf.store(z2, z1, 1.0, z2, 1.0)             # end defaults to done
    buf.store(z2, z1, 1.0, z2, 0.0, end=1.0)    # truncation
    buf.store(z2, z1, 1.0, z2, 0.0)
    assert buf.episode_end.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert int(buf._ptr_dev.item()) == 3
    # store_batch longer than the ring: only the tail survives, the
    # device write head follows the host one
    n = 7
    buf.store_batch(np.zeros((n, 2)), np.zeros((n, 1)),
                    np.arange(n, dtype=np.float32), np.zeros((n, 2)),
                    np.zeros(n), np.array([0, 0, 0, 0, 1, 0, 0.]))
    assert buf.ptr == (3 + n) % 4 == int(buf._ptr_dev.item())
    assert buf.size == 4 == int(buf._size_dev.item())
    # slots after the wrap: ptr=2 -> slot order 2,3,0,1 holds r=3,4,5,6
    assert buf.rewards.tolist() == [5.0, 6.0, 3.0, 4.0]
    assert buf.episode_end.tolist() == [0.0, 0.0, 0.0, 1.0]


def test_not_full_ring_stops_at_newest():
    buf = ReplayBuffer(64, 2, 1)
    buf.set_n_step(N, 0.5)
    t = np.arange(20, dtype=np.float32)
    buf.store_batch(np.stack([t, t], 1), t[:, None], np.ones(20),
                    np.stack([t + 1000, t], 1), np.zeros(20))
    b = buf.sample_at(torch.tensor([10, 16, 17, 18, 19]))
    assert (b.next_states[:, 0] - 1000).tolist() == [13, 19, 19, 19, 19]
    assert b.rewards.tolist() == [1.875, 1.875, 1.75, 1.5, 1.0]
    assert b.done.tolist() == [0.875, 0.875, 0.75, 0.5, 0.0]


def test_sac_train_nstep_cpu():
    from sac.algorithm import SAC
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam

    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor = Actor(3, 1, [32, 32], act_limit=2.0)
    critic = DoubleCritic(3, 1, [32, 32])
    buf = ReplayBuffer(1000, 3, 1)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=32, start_steps=100, steps_per_epoch=300,
              max_ep_len=100, update_after=100, update_every=50,
              save_every=10, n_step=3)
    m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                  FlatAdam(critic), render=False, logging=False)
    assert np.isfinite(m["loss_q"]) and np.isfinite(m["loss_pi"])
    assert m["loss_q"] != 0.0
    assert buf.n_step == 3 and buf.gamma == 0.99 and buf.size == 300
    ends = torch.nonzero(buf.episode_end).flatten().tolist()
    assert ends == [99, 199, 299]       # the max_ep_len truncations only
    assert float(buf.done[:300].abs().sum()) == 0.0


def test_sac_nstep_needs_capable_buffer():
    from sac.algorithm import SAC

    class NoNStep:
        pass

    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=8, start_steps=0, steps_per_epoch=1,
              max_ep_len=10, update_after=0, update_every=1, save_every=10,
              n_step=2)
    actor = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="set_n_step"):
        sac.train(0, None, actor, torch.nn.Linear(1, 1), NoNStep(), None,
                  None, render=False, logging=False)


@pytest.mark.timeout(300)
def test_cli_n_step_logged_and_resumed(tmp_path, monkeypatch):
    env = {**os.environ, "PYTHONPATH": REPO}
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "main.py"), "--environment",
         "Pendulum-v1", "--epochs", "10", "--steps-per-epoch", "20",
         "--batch-size", "8", "--buffer-size", "500", "--device", "cpu",
         "--n-step", "3"], cwd=tmp_path, timeout=240, capture_output=True,
        text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = os.listdir(tmp_path / "mlruns" / "0")
    assert len(runs) == 1
    params = tmp_path / "mlruns" / "0" / runs[0] / "params"
    assert (params / "n_step").read_text() == "3"

    monkeypatch.chdir(tmp_path)
    from torch_actor_critic_amd.utils import checkpoint as ckpt
    ckpt.set_tracking_dir("mlruns")
    import main as train_main
    from sac.algorithm import SAC
    *_, sac_params, _env = train_main.load_session(runs[0],
                                                   torch.device("cpu"))
    assert sac_params["n_step"] == 3
    assert SAC(**sac_params).n_step == 3
    # a run logged before the flag existed resumes as 1-step
    (params / "n_step").unlink()
    *_, sac_params, _env = train_main.load_session(runs[0],
                                                   torch.device("cpu"))
    assert "n_step" not in sac_params
    assert SAC(**sac_params).n_step == 1
