"""N-step returns in the visual replay buffer (CPU):
``VisualReplayBuffer.sample_at(idx, shifts, n)`` is the executable
definition; these tests pin it to a literal per-row loop and cover the
composition with the random shift, the buffer guards, the store, the CPU
samplers, the SAC loop and the CLI.

The visual ring built here is the twin of the ring of tests/test_nstep.py
and is shared with tests/test_gpu_visual_nstep.py:

* ``max_size=48``; 60 transitions written one by one through
  ``store(..., end=...)``, so the ring is full and wrapped with
  ``ptr == 12`` (slots 0..11 hold t=48..59, slots 12..47 hold t=12..47).
* ``features[:, 0]`` is the global step t, ``next_features[:, 0]`` is
  1000 + t, so sampled and bootstrap slots are recoverable from a batch.
* The ``done``/``end`` flags and integer rewards of that fixture.
* fp32 frames hold ``t * P + position + 1`` (P = C*H*W; below 2^24, so
  exact), next frames the negative of it: a sampled pixel names the
  transition, the side and the position it was read from.  u8 buffers
  hold seeded random bytes (stored as the fp32 value each byte decodes
  to, which encodes back to the same byte).
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_nstep import (KIND_T, N, RING, T_TOTAL, episode_flags, int_reward,
                        window_kinds)
from torch_actor_critic_amd.buffer.visual import (VisualBatch,
                                                  VisualReplayBuffer)
from torch_actor_critic_amd.envs.visual import MultiObservation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FEAT, ACT = 5, 3
VIS = (3, 8, 8)


def ring_frames(vis, total, quantize):
    """(frames, next_frames) ``[total, *vis]`` fp32 as handed to store."""
    P = int(np.prod(vis))
    if quantize:
        rng = np.random.default_rng(23)
        b = rng.integers(0, 256, size=(2, total, *vis)).astype(np.float32)
        fr = b / np.float32(127.5) - np.float32(1.0)
        return torch.from_numpy(fr[0]), torch.from_numpy(fr[1])
    assert total * P + P < 2 ** 24
    code = (torch.arange(total, dtype=torch.float32)[:, None] * P
            + torch.arange(1, P + 1, dtype=torch.float32)[None])
    code = code.reshape(total, *vis)
    return code, -code


def ring_rows(total):
    """Small-integer feature / action rows keyed by the global step."""
    t = np.arange(total)[:, None]
    f = ((t * 13 + np.arange(FEAT)[None]) % 23).astype(np.float32)
    f[:, 0] = np.arange(total)
    nf = ((t * 5 + np.arange(FEAT)[None]) % 19).astype(np.float32)
    nf[:, 0] = 1000 + np.arange(total)
    a = ((t * 3 + np.arange(ACT)[None]) % 11 - 5).astype(np.float32)
    return f, nf, a


def fill_ring(buf, vis=VIS, total=T_TOTAL, reward=int_reward, pass_end=True):
    """Store the fixture's transitions into ``buf`` one by one."""
    f, nf, a = ring_rows(total)
    fr, nfr = ring_frames(vis, total, buf.quantize)
    done, end = episode_flags(total)
    for t in range(total):
        kw = {"end": float(end[t])} if pass_end else {}
        buf.store(MultiObservation(torch.from_numpy(f[t].copy()),
                                   fr[t].clone()),
                  a[t], reward(t),
                  MultiObservation(torch.from_numpy(nf[t].copy()),
                                   nfr[t].clone()),
                  float(done[t]), **kw)
    return buf


def make_visual_ring(device="cpu", vis=VIS, quantize=False, gamma=0.5,
                     n_step=N, size=RING, total=T_TOTAL, reward=int_reward,
                     seed=0):
    buf = VisualReplayBuffer(size, ACT, device=device, seed=seed,
                             quantize_frames=quantize)
    buf.set_n_step(n_step, gamma)
    return fill_ring(buf, vis, total, reward)


def fields(b: VisualBatch):
    return {"features": b.states.features, "frame": b.states.frame,
            "actions": b.actions, "rewards": b.rewards,
            "next_features": b.next_states.features,
            "next_frame": b.next_states.frame, "done": b.done}


def assert_batches_equal(a: VisualBatch, b: VisualBatch):
    for (name, x), y in zip(fields(a).items(), fields(b).values()):
        assert torch.equal(x, y), name


def slots_of(b: VisualBatch):
    return b.states.features[:, 0].round().long() % RING


def loop_windows(buf, idx, n):
    """The window rule as a literal per-row loop in numpy fp32:
    (last slot, reward sum, effective done) per row."""
    S = buf.max_size
    rew = buf.rewards.cpu().numpy()
    done = buf.done.cpu().numpy()
    end = buf.episode_end.cpu().numpy()
    newest = (buf.ptr - 1) % S if buf.size else 0
    g = np.float32(buf.gamma)
    out = []
    for i in idx:
        R, disc, j = np.float32(0.0), np.float32(1.0), i
        for m in range(n):
            j = (i + m) % S
            if m > 0:
                disc = np.float32(disc * g)
            R = np.float32(R + np.float32(disc * rew[j]))
            if done[j] != 0 or end[j] != 0 or j == newest:
                break
        deff = np.float32(np.float32(1.0)
                          - np.float32(disc * np.float32(1.0 - done[j])))
        out.append((j, float(R), float(deff)))
    return out


@pytest.fixture(scope="module")
def ring():
    """The fp32 fixture at gamma 0.5, n = 4; tests must not change it."""
    return make_visual_ring()


def test_fixture_layout(ring):
    assert ring.ptr == 12 and ring.size == RING
    assert int(ring._ptr_dev.item()) == 12
    assert int(ring._size_dev.item()) == RING
    want_t = np.array([48 + i if i < 12 else i for i in range(RING)])
    np.testing.assert_array_equal(ring.features[:, 0].numpy(), want_t)
    np.testing.assert_array_equal(ring.next_features[:, 0].numpy(),
                                  1000 + want_t)
    done, end = episode_flags(T_TOTAL)
    np.testing.assert_array_equal(ring.done.numpy(), done[want_t])
    np.testing.assert_array_equal(ring.episode_end.numpy(), end[want_t])
    P = int(np.prod(VIS))
    np.testing.assert_array_equal(ring.frames[:, 0, 0, 0].numpy(),
                                  want_t * P + 1)
    np.testing.assert_array_equal(ring.next_frames[:, 2, 7, 7].numpy(),
                                  -(want_t * P + P))


@pytest.mark.parametrize("n", [1, 2, 4, 64])
def test_sample_at_is_the_per_row_loop(ring, n):
    idx = list(range(RING))
    b = ring.sample_at(torch.tensor(idx), None, n)
    assert b.shifts is None
    want = loop_windows(ring, idx, n)
    for k, (i, (last, R, deff)) in enumerate(zip(idx, want)):
        assert float(b.rewards[k]) == R, (i, float(b.rewards[k]), R)
        assert float(b.done[k]) == deff, (i, float(b.done[k]), deff)
        assert torch.equal(b.states.features[k], ring.features[i])
        assert torch.equal(b.states.frame[k], ring.frames[i])
        assert torch.equal(b.actions[k], ring.actions[i])
        assert torch.equal(b.next_states.features[k],
                           ring.next_features[last])
        assert torch.equal(b.next_states.frame[k], ring.next_frames[last])
    lasts = [w[0] for w in want]
    if n == 1:
        assert lasts == idx
        assert torch.equal(b.rewards, ring.rewards)
        assert torch.equal(b.done, ring.done)
    else:
        assert lasts != idx
    if n == N:
        assert torch.equal(ring.sample_at(torch.tensor(idx)).rewards,
                           b.rewards)          # the buffer's own n_step
        kinds = window_kinds(b.states.features[:, 0],
                             b.next_states.features[:, 0] - 1000)
        assert kinds == set(KIND_T)


def test_sample_at_hand_rows(ring):
    """gamma = 0.5, n = 4; the rows of test_nstep's hand table."""
    table = [(15, -6.125, 0.875, 18), (24, 6.5, 1.0, 26),
             (19, 4.75, 0.75, 21), (58, 5.5, 0.5, 59),
             (46, 7.625, 0.875, 49), (59, -3.0, 0.0, 59)]
    b = ring.sample_at(torch.tensor([row[0] % RING for row in table]))
    P = int(np.prod(VIS))
    for k, (t0, rew, deff, t1) in enumerate(table):
        assert float(b.rewards[k]) == rew and float(b.done[k]) == deff
        assert float(b.states.frame[k, 0, 0, 0]) == t0 * P + 1
        assert float(b.next_states.frame[k, 0, 0, 0]) == -(t1 * P + 1)
        assert float(b.next_states.features[k, 0]) == 1000 + t1


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("vis,pad", [((3, 8, 8), 4), ((2, 7, 10), 3)])
def test_sample_at_shifts_state_at_idx_and_next_at_last(vis, pad, quantize):
    buf = make_visual_ring(vis=vis, quantize=quantize)
    buf.set_random_shift(pad)
    idx = torch.arange(RING)
    g = torch.Generator().manual_seed(4)
    shifts = torch.randint(0, 2 * pad + 1, (RING, 4), generator=g,
                           dtype=torch.int32)
    shifts[0] = torch.tensor([0, 0, 2 * pad, 2 * pad])
    b = buf.sample_at(idx, shifts, N)
    last = torch.tensor([w[0] for w in loop_windows(buf, idx.tolist(), N)])
    assert (last != idx).any()
    assert torch.equal(b.shifts, shifts)
    assert torch.equal(
        b.states.frame,
        VisualReplayBuffer.shift_frames(buf._dec_frames(buf.frames[idx]),
                                        shifts[:, 0:2], pad))
    assert torch.equal(
        b.next_states.frame,
        VisualReplayBuffer.shift_frames(
            buf._dec_frames(buf.next_frames[last]), shifts[:, 2:4], pad))
    assert torch.equal(b.next_states.features, buf.next_features[last])
    # the shift leaves every other field alone
    plain = buf.sample_at(idx, None, N)
    for name in ("features", "actions", "rewards", "next_features", "done"):
        assert torch.equal(fields(b)[name], fields(plain)[name]), name


def test_set_n_step_guards():
    buf = VisualReplayBuffer(16, 2)
    assert buf.n_step == 1 and buf.MAX_N_STEP == 64
    for bad in (0, -1, 65):
        with pytest.raises(ValueError, match="n_step"):
            buf.set_n_step(bad, 0.9)
    buf.set_n_step(1, 0.9)              # n = 1 allocates nothing
    assert buf.episode_end is None and buf._ptr_dev is None
    mo = MultiObservation(torch.zeros(3), torch.zeros(1, 4, 4))
    buf.store(mo, np.zeros(2), 1.0, mo, 0.0)
    buf.set_n_step(1, 0.9)
    with pytest.raises(ValueError, match="empty"):
        buf.set_n_step(2, 0.9)          # no episode boundaries recorded
    assert buf.episode_end is None and buf.n_step == 1
    with pytest.raises(ValueError, match="set_n_step"):
        buf.sample_at(torch.tensor([0]), None, 2)
    # before the first store: the observation shape is not needed
    ok = VisualReplayBuffer(16, 2)
    ok.set_n_step(64, 0.9)
    assert not ok._alloc_done
    assert ok.n_step == 64 and ok.gamma == 0.9
    assert ok.episode_end.shape == (16,)
    assert ok.episode_end.dtype == torch.float32
    assert ok._ptr_dev.dtype == torch.int64 and ok._ptr_dev.shape == (1,)
    ok.store(mo, np.zeros(2), 1.0, mo, 0.0)
    ok.set_n_step(3, 0.5)               # changing n later is allowed
    assert ok.n_step == 3 and ok.gamma == 0.5


def test_store_records_end_and_mirrors_ptr():
    buf = VisualReplayBuffer(4, 2)
    buf.set_n_step(3, 0.5)
    mo = MultiObservation(torch.zeros(3), torch.zeros(1, 4, 4))
    z = np.zeros(2)
    buf.store(mo, z, 1.0, mo, 1.0)              # end defaults to done
    buf.store(mo, z, 1.0, mo, 0.0, end=1.0)     # truncation
    buf.store(mo, z, 1.0, mo, 0.0)
    assert buf.episode_end.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert buf.done.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert int(buf._ptr_dev.item()) == 3 == buf.ptr
    buf.store(mo, z, 1.0, mo, 0.0, end=1.0)
    assert int(buf._ptr_dev.item()) == 0 == buf.ptr      # ring wrap
    buf.store(mo, z, 2.0, mo, 0.0)              # overwrites slot 0
    assert buf.episode_end.tolist() == [0.0, 1.0, 0.0, 1.0]
    assert buf.done.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert int(buf._ptr_dev.item()) == 1 == buf.ptr
    assert buf.size == 4 == int(buf._size_dev.item())


@pytest.mark.parametrize("pad", [0, 3])
def test_one_step_buffer_is_unchanged(pad):
    """No set_n_step, set_n_step(1) and an n-step ring switched back to 1
    give the same batches bit for bit at equal seeds."""
    def build(how):
        buf = VisualReplayBuffer(RING, ACT, seed=5)
        if how == "set1":
            buf.set_n_step(1, 0.5)
        elif how == "back":
            buf.set_n_step(N, 0.5)
        fill_ring(buf, pass_end=(how == "back"))
        if how == "back":
            buf.set_n_step(1, 0.5)
        buf.set_random_shift(pad)
        return buf

    never, set1, back = build("never"), build("set1"), build("back")
    for buf in (never, set1):
        assert buf.episode_end is None and buf._ptr_dev is None
        assert buf.n_step == 1
    want = never.sample(16)
    outs = []
    for buf in (never, set1, back):
        out = buf.make_static_batch(16)
        torch.manual_seed(9)
        buf.sample_into(out)
        outs.append(out)
    for buf, out in zip((set1, back), outs[1:]):
        assert_batches_equal(buf.sample(16), want)
        assert_batches_equal(out, outs[0])
        if pad:
            assert torch.equal(out.shifts, outs[0].shifts)
    # and it is the plain 1-step batch
    idx = slots_of(want)
    assert torch.equal(want.rewards, never.rewards[idx])
    assert torch.equal(want.done, never.done[idx])
    assert torch.equal(want.next_states.features, never.next_features[idx])


@pytest.mark.parametrize("pad", [0, 4])
def test_cpu_samplers_follow_sample_at(pad):
    buf = make_visual_ring(seed=3)
    buf.set_random_shift(pad)
    b = buf.sample(32)
    assert len(set(slots_of(b).tolist())) == 32     # without replacement
    assert_batches_equal(b, buf.sample_at(slots_of(b), b.shifts, N))
    assert (b.next_states.features[:, 0] - 1000
            != b.states.features[:, 0]).any()
    out = buf.make_static_batch(64)
    torch.manual_seed(1)
    buf.sample_into(out)
    assert_batches_equal(out, buf.sample_at(slots_of(out), out.shifts, N))
    assert (out.next_states.features[:, 0] - 1000
            != out.states.features[:, 0]).any()
    if pad:
        assert (b.shifts != pad).any() and (out.shifts != pad).any()
    else:
        assert b.shifts is None and out.shifts is None
    # same slot draw as a 1-step buffer with the same seeds
    one = make_visual_ring(seed=3, n_step=1)
    one.set_random_shift(pad)
    assert torch.equal(one.sample(32).states.features, b.states.features)


class ScheduledEpisodes:
    """Env wrapper: every odd episode terminates (done=True) on its third
    step; the others run until the trainer truncates them."""

    def __init__(self, env):
        self.env = env
        self.action_space = env.action_space
        self.observation_space = env.observation_space
        self.episode, self.t = -1, 0

    def seed(self, seed):
        self.env.seed(seed)

    def reset(self):
        self.episode += 1
        self.t = 0
        return self.env.reset()

    def step(self, action):
        obs, reward, _done, info = self.env.step(action)
        self.t += 1
        return obs, reward, self.episode % 2 == 1 and self.t == 3, info


def test_sac_train_visual_nstep_cpu():
    from sac.algorithm import SAC
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.models.visual import (VisualActor,
                                                      VisualDoubleCritic)
    from torch_actor_critic_amd.optim import FlatAdam

    env = ScheduledEpisodes(envs.make("VisualCheetahRun-v0"))
    obs_dim = env.observation_space.shape[0]
    act_dim = env.action_space.shape[0]
    actor = VisualActor(obs_dim, act_dim, (3, 84, 84), [16, 16], 1.0)
    critic = VisualDoubleCritic(obs_dim, act_dim, (3, 84, 84), [16, 16])
    buf = VisualReplayBuffer(100, act_dim)
    epochs, spe, max_len = 2, 16, 5
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=epochs, batch_size=4, start_steps=8,
              steps_per_epoch=spe, max_ep_len=max_len, update_after=8,
              update_every=4, save_every=10, n_step=3, aug_shift=2)
    m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                  FlatAdam(critic), render=False, logging=False)
    assert np.isfinite(m["loss_q"]) and np.isfinite(m["loss_pi"])
    assert m["loss_q"] != 0.0
    assert buf.n_step == 3 and buf.gamma == 0.99 and buf.shift_pad == 2
    assert buf.size == epochs * spe == int(buf._ptr_dev.item())
    # what the loop should have stored, from the schedule alone
    want_done, want_end = [], []
    episode, t = 0, 0
    for _e in range(epochs):
        for k in range(spe):
            t += 1
            term = episode % 2 == 1 and t == 3
            trunc = t == max_len
            want_done.append(float(term and not trunc))
            want_end.append(float(term or trunc or k == spe - 1))
            if term or trunc:
                episode, t = episode + 1, 0
        episode, t = episode + 1, 0         # the reset closing the epoch
    assert sum(want_done) >= 2 and sum(want_end) > sum(want_done) + 2
    assert buf.done[:buf.size].tolist() == want_done
    assert buf.episode_end[:buf.size].tolist() == want_end


@pytest.mark.timeout(300)
def test_cli_visual_n_step_logged_and_resumed(tmp_path, monkeypatch):
    env = {**os.environ, "PYTHONPATH": REPO}
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "main.py"), "--environment",
         "VisualCheetahRun-v0", "--epochs", "10", "--steps-per-epoch", "20",
         "--batch-size", "8", "--buffer-size", "300", "--device", "cpu",
         "--n-step", "3", "--aug-shift", "2"], cwd=tmp_path, timeout=240,
        capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = os.listdir(tmp_path / "mlruns" / "0")
    assert len(runs) == 1
    params = tmp_path / "mlruns" / "0" / runs[0] / "params"
    assert (params / "n_step").read_text() == "3"
    assert (params / "environment").read_text() == "VisualCheetahRun-v0"

    monkeypatch.chdir(tmp_path)
    from torch_actor_critic_amd.utils import checkpoint as ckpt
    ckpt.set_tracking_dir("mlruns")
    import main as train_main
    from sac.algorithm import SAC
    *_, sac_params, saved_env = train_main.load_session(
        runs[0], torch.device("cpu"))
    assert saved_env == "VisualCheetahRun-v0"
    assert sac_params["n_step"] == 3 and sac_params["aug_shift"] == 2
    assert SAC(**sac_params).n_step == 3


def test_main_hands_n_step_to_sac_and_trains_one_epoch(monkeypatch):
    """main() in process on the visual env: one tiny epoch with updates
    through SAC(n_step=3), the buffer switched to 3-step windows."""
    import main as train_main

    seen = {}
    real_sac = train_main.SAC

    def tiny_sac(**kw):
        kw.update(start_steps=4, update_after=4, update_every=4,
                  max_ep_len=6)
        sac = real_sac(**kw)
        seen["sac"] = sac
        return sac

    real_init_buffer = train_main.init_buffer

    def init_buffer(*a, **k):
        seen["buffer"] = real_init_buffer(*a, **k)
        return seen["buffer"]

    monkeypatch.setattr(train_main, "SAC", tiny_sac)
    monkeypatch.setattr(train_main, "init_buffer", init_buffer)
    monkeypatch.setattr(train_main, "gpu_fork", lambda n: None)
    monkeypatch.setattr(train_main.comm, "init_distributed", lambda: None)
    monkeypatch.setattr(train_main.ckpt, "set_experiment", lambda e: None)
    monkeypatch.setattr(sys, "argv", [
        "main.py", "--disable-logging", "--device", "cpu", "--environment",
        "VisualCheetahRun-v0", "--buffer-size", "50", "--epochs", "1",
        "--steps-per-epoch", "12", "--batch-size", "4", "--n-step", "3",
        "--aug-shift", "2"])
    train_main.main()
    assert seen["sac"].n_step == 3
    buf = seen["buffer"]
    assert isinstance(buf, VisualReplayBuffer)
    assert buf.n_step == 3 and buf.shift_pad == 2 and buf.size == 12
    assert torch.nonzero(buf.episode_end).flatten().tolist() == [5, 11]
