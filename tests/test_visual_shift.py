"""DrQ random-shift augmentation of the visual replay buffer (CPU).

``VisualReplayBuffer.shift_frames`` is the executable definition
(replicate-pad by ``pad``, crop at ``(dy, dx)``); these tests pin it to
``F.pad`` + slicing and cover the CPU samplers, the guards, the SAC loop
hook and the CLI.  The shift is an integer translation, so every frame
comparison is exact.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from torch_actor_critic_amd.buffer.replay import ReplayBuffer
from torch_actor_critic_amd.buffer.visual import (VisualBatch,
                                                  VisualReplayBuffer)
from torch_actor_critic_amd.envs.visual import MultiObservation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, H, W), pad
SHAPES = [((3, 8, 8), 4), ((2, 7, 10), 3), ((1, 5, 5), 6), ((3, 84, 84), 4)]


def pad_crop(frames, shifts, pad):
    """Replicate-pad + crop, one sample at a time."""
    H, W = frames.shape[-2:]
    padded = F.pad(frames, (pad, pad, pad, pad), mode="replicate")
    return torch.stack([
        padded[b, :, dy:dy + H, dx:dx + W]
        for b, (dy, dx) in enumerate(shifts.tolist())])


@pytest.mark.parametrize("vis,pad", SHAPES)
def test_shift_frames_is_replicate_pad_and_crop(vis, pad):
    g = torch.Generator().manual_seed(11)
    B = 16
    frames = torch.randn(B, *vis, generator=g)
    shifts = torch.randint(0, 2 * pad + 1, (B, 2), generator=g)
    # the extreme shifts are always among the cases
    shifts[0] = torch.tensor([0, 0])
    shifts[1] = torch.tensor([2 * pad, 2 * pad])
    shifts[2] = torch.tensor([0, 2 * pad])
    out = VisualReplayBuffer.shift_frames(frames, shifts, pad)
    assert out.dtype == frames.dtype and out.shape == frames.shape
    assert torch.equal(out, pad_crop(frames, shifts, pad))
    # int32 shifts (what the samplers emit) give the same result
    assert torch.equal(
        VisualReplayBuffer.shift_frames(frames, shifts.to(torch.int32), pad),
        out)


@pytest.mark.parametrize("vis,pad", SHAPES)
def test_centre_shift_is_identity(vis, pad):
    frames = torch.randn(5, *vis, generator=torch.Generator().manual_seed(3))
    centre = torch.full((5, 2), pad)
    assert torch.equal(VisualReplayBuffer.shift_frames(frames, centre, pad),
                       frames)


def make_buffer(n=40, feat=5, vis=(3, 8, 8), seed=3, quantize=True):
    """Slot i is recoverable from features[:, 0]; frames are random."""
    buf = VisualReplayBuffer(64, 4, seed=seed, quantize_frames=quantize)
    rng = np.random.default_rng(7)
    for i in range(n):
        f = np.full(feat, float(i), dtype=np.float32)
        fr = np.clip(rng.standard_normal(vis).astype(np.float32), -1, 1)
        nfr = np.clip(rng.standard_normal(vis).astype(np.float32), -1, 1)
        buf.store(MultiObservation(torch.tensor(f), torch.tensor(fr)),
                  np.full(4, float(i), dtype=np.float32), float(i),
                  MultiObservation(torch.tensor(f + 0.5), torch.tensor(nfr)),
                  float(i % 2))
    return buf


def batch_tensors(b: VisualBatch):
    return (b.states.features, b.states.frame, b.actions, b.rewards,
            b.next_states.features, b.next_states.frame, b.done)


def assert_batches_equal(a: VisualBatch, b: VisualBatch):
    for x, y in zip(batch_tensors(a), batch_tensors(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("quantize", [True, False])
def test_cpu_sample_into_shifts_frames_only(quantize):
    pad = 4
    buf = make_buffer(quantize=quantize)
    buf.set_random_shift(pad)
    assert buf.shift_pad == pad
    out = buf.make_static_batch(32)
    assert out.shifts.dtype == torch.int32 and out.shifts.shape == (32, 4)
    torch.manual_seed(5)
    buf.sample_into(out)
    idx = out.states.features[:, 0].to(torch.long)
    assert (idx >= 0).all() and (idx < buf.size).all()
    sh = out.shifts
    assert (sh >= 0).all() and (sh <= 2 * pad).all()
    assert len(torch.unique(sh)) > 1
    stored = buf._dec_frames(buf.frames[idx])
    nstored = buf._dec_frames(buf.next_frames[idx])
    assert torch.equal(out.states.frame,
                       VisualReplayBuffer.shift_frames(stored, sh[:, :2], pad))
    assert torch.equal(out.next_states.frame,
                       VisualReplayBuffer.shift_frames(nstored, sh[:, 2:],
                                                       pad))
    # some frame did move
    assert not torch.equal(out.states.frame, stored)
    # the other fields are the stored rows
    assert torch.equal(out.states.features, buf.features[idx])
    assert torch.equal(out.next_states.features, buf.next_features[idx])
    assert torch.equal(out.actions, buf.actions[idx])
    assert torch.equal(out.rewards, buf.rewards[idx])
    assert torch.equal(out.done, buf.done[idx])
    # sample_at is the same function of (slots, shifts)
    assert_batches_equal(out, buf.sample_at(idx, sh))


def test_cpu_sample_shifts_with_the_numpy_rng():
    pad = 2
    buf = make_buffer()
    buf.set_random_shift(pad)
    b = buf.sample(16)
    assert b.shifts.shape == (16, 4) and b.shifts.dtype == torch.int32
    assert (b.shifts >= 0).all() and (b.shifts <= 2 * pad).all()
    idx = b.states.features[:, 0].to(torch.long)
    assert len(set(idx.tolist())) == 16     # still without replacement
    assert_batches_equal(b, buf.sample_at(idx, b.shifts))
    stored = buf._dec_frames(buf.frames[idx])
    assert torch.equal(
        b.states.frame,
        VisualReplayBuffer.shift_frames(stored, b.shifts[:, :2], pad))


def test_sample_at_unshifted_and_plain_batch_has_no_shifts():
    buf = make_buffer()
    idx = torch.tensor([3, 0, 39, 3])
    b = buf.sample_at(idx)
    assert b.shifts is None
    assert torch.equal(b.states.frame, buf._dec_frames(buf.frames[idx]))
    assert buf.make_static_batch(4).shifts is None
    assert buf.sample(4).shifts is None
    # a batch made before augmentation was switched on cannot take shifts
    out = buf.make_static_batch(4)
    buf.set_random_shift(1)
    with pytest.raises(ValueError, match="make_static_batch"):
        buf.sample_into(out)


def test_shift_off_reproduces_a_fresh_buffer():
    fresh, toggled = make_buffer(), make_buffer()
    toggled.set_random_shift(4)
    toggled.set_random_shift(0)
    assert toggled.shift_pad == 0
    o1, o2 = fresh.make_static_batch(16), toggled.make_static_batch(16)
    assert o2.shifts is None
    torch.manual_seed(9)
    fresh.sample_into(o1)
    torch.manual_seed(9)
    toggled.sample_into(o2)
    assert_batches_equal(o1, o2)
    assert_batches_equal(fresh.sample(16), toggled.sample(16))


def test_shift_on_draws_the_same_cpu_slots():
    """The shift draw comes after the slot draw in both CPU samplers."""
    plain, aug = make_buffer(), make_buffer()
    aug.set_random_shift(3)
    o1, o2 = plain.make_static_batch(16), aug.make_static_batch(16)
    torch.manual_seed(2)
    plain.sample_into(o1)
    torch.manual_seed(2)
    aug.sample_into(o2)
    assert torch.equal(o1.states.features, o2.states.features)
    assert torch.equal(plain.sample(16).states.features,
                       aug.sample(16).states.features)


@pytest.mark.parametrize("bad", [-1, 33, 1.5])
def test_set_random_shift_rejects(bad):
    buf = make_buffer(n=1)
    with pytest.raises(ValueError, match="shift pad"):
        buf.set_random_shift(bad)
    assert buf.shift_pad == 0
    buf.set_random_shift(32)
    assert buf.shift_pad == 32


def sac_kwargs(**kw):
    return dict(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
                epochs=1, batch_size=8, start_steps=0, steps_per_epoch=1,
                max_ep_len=10, update_after=0, update_every=1, save_every=10,
                **kw)


def test_sac_aug_shift_needs_a_visual_buffer():
    from sac.algorithm import SAC

    sac = SAC(**sac_kwargs(aug_shift=2))
    assert sac.aug_shift == 2
    actor = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="ReplayBuffer"):
        sac.train(0, None, actor, torch.nn.Linear(1, 1),
                  ReplayBuffer(10, 3, 1), None, None, render=False,
                  logging=False)
    with pytest.raises(ValueError, match="aug_shift"):
        SAC(**sac_kwargs(aug_shift=-1))
    assert SAC(**sac_kwargs()).aug_shift == 0


def test_sac_train_switches_the_buffer_on():
    """train() hands the pad to the buffer before anything samples; the
    eager visual update then trains on shifted batches."""
    from sac.algorithm import SAC
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.models.visual import (VisualActor,
                                                      VisualDoubleCritic)
    from torch_actor_critic_amd.optim import FlatAdam

    env = envs.make("DeepMindWallRunner-v0")
    obs_dim = env.observation_space.shape[0]
    act_dim = env.action_space.shape[0]
    actor = VisualActor(obs_dim, act_dim, (3, 64, 64), [16, 16], 1.0)
    critic = VisualDoubleCritic(obs_dim, act_dim, (3, 64, 64), [16, 16])
    buf = VisualReplayBuffer(100, act_dim)
    sac = SAC(**{**sac_kwargs(aug_shift=4), "batch_size": 4,
                 "start_steps": 8, "steps_per_epoch": 12, "update_after": 8,
                 "update_every": 4, "max_ep_len": 6})
    m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                  FlatAdam(critic), render=False, logging=False)
    assert buf.shift_pad == 4
    assert np.isfinite(m["loss_q"]) and np.isfinite(m["loss_pi"])
    assert m["loss_q"] != 0.0


@pytest.mark.timeout(300)
def test_cli_aug_shift_logged_and_resumed(tmp_path, monkeypatch):
    env = {**os.environ, "PYTHONPATH": REPO}
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "main.py"), "--environment",
         "DeepMindWallRunner-v0", "--epochs", "10", "--steps-per-epoch", "20",
         "--batch-size", "8", "--buffer-size", "300", "--device", "cpu",
         "--aug-shift", "3"], cwd=tmp_path, timeout=240, capture_output=True,
        text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = os.listdir(tmp_path / "mlruns" / "0")
    assert len(runs) == 1
    params = tmp_path / "mlruns" / "0" / runs[0] / "params"
    assert (params / "aug_shift").read_text() == "3"

    monkeypatch.chdir(tmp_path)
    from torch_actor_critic_amd.utils import checkpoint as ckpt
    ckpt.set_tracking_dir("mlruns")
    import main as train_main
    from sac.algorithm import SAC
    *_, sac_params, _env = train_main.load_session(runs[0],
                                                   torch.device("cpu"))
    assert sac_params["aug_shift"] == 3
    assert SAC(**sac_params).aug_shift == 3
    # a run logged before the flag existed resumes with augmentation off
    (params / "aug_shift").unlink()
    *_, sac_params, _env = train_main.load_session(runs[0],
                                                   torch.device("cpu"))
    assert "aug_shift" not in sac_params
    assert SAC(**sac_params).aug_shift == 0


def test_cli_aug_shift_default_and_resume_override(monkeypatch):
    """Flag rules of main(): fresh runs default to 0; on a resume the
    logged value stands unless the flag is given."""
    import main as train_main

    seen = {}

    class Stop(Exception):
        pass

    def fake_sac(**kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(train_main, "SAC", fake_sac)
    monkeypatch.setattr(train_main, "gpu_fork", lambda n: None)
    monkeypatch.setattr(train_main.comm, "init_distributed", lambda: None)
    monkeypatch.setattr(train_main.ckpt, "set_experiment", lambda e: None)
    monkeypatch.setattr(
        train_main, "load_session",
        lambda run, dev: (None, None, None, None, 0,
                          {"aug_shift": 3, "n_step": 1}, "Pendulum-v1"))
    base = ["main.py", "--disable-logging", "--device", "cpu",
            "--environment", "Pendulum-v1", "--buffer-size", "10"]
    for extra, want in (([], 0), (["--aug-shift", "5"], 5),
                        (["--run", "x"], 3),
                        (["--run", "x", "--aug-shift", "0"], 0),
                        (["--run", "x", "--aug-shift", "2"], 2)):
        seen.clear()
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(Stop):
            train_main.main()
        assert seen["aug_shift"] == want, extra
