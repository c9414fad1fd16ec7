"""GPU tests of ``visual_gather_shift_kernel``: the DrQ random shift fused
into the one-kernel Philox gather+dequantize of the visual replay buffer.

The reference is ``VisualReplayBuffer.sample_at(slots, shifts)`` (pure
torch, pinned to replicate-pad + crop in tests/test_visual_shift.py).
The shift is an integer translation, so the fp32-buffer comparisons are
bit-exact; the u8-buffer comparison carries only the dequantisation's
rounding (``atol=1e-6``, as in ``test_visual_fused_sample_gpu``).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_SLOTS, FEAT, ACT = 300, 6, 4


def position_code(vis):
    """frame[c, y, x] = c*H*W + y*W + x + 1: integers below 2^24, so a
    pixel names the source position it was read from."""
    C, H, W = vis
    return torch.arange(1, C * H * W + 1, dtype=torch.float32).reshape(vis)


def make_buffer(vis, quantize, seed=3, n=N_SLOTS):
    """``features[:, 0]`` holds the slot.  fp32 buffers hold the position
    code in every slot (negated for next frames), so a sampled pixel
    decodes to the source position it was read from; u8 buffers hold
    random bytes."""
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
    from torch_actor_critic_amd.envs.visual import MultiObservation

    buf = VisualReplayBuffer(n + 50, ACT, device=DEV, seed=seed,
                             quantize_frames=quantize)
    mo = MultiObservation(torch.zeros(FEAT, device=DEV),
                          torch.zeros(*vis, device=DEV))
    buf.store(mo, np.zeros(ACT, dtype=np.float32), 0.0, mo, 0.0)
    slot = torch.arange(n, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(17)
    buf.features[:n] = slot[:, None] + \
        torch.arange(FEAT, device=DEV)[None] * 1000.0
    buf.next_features[:n] = buf.features[:n] + 0.5
    buf.actions[:n] = slot[:, None] - torch.arange(ACT, device=DEV)[None]
    buf.rewards[:n] = slot * 3.0
    buf.done[:n] = slot % 2
    if quantize:
        buf.frames[:n] = torch.randint(
            0, 256, (n, *vis), generator=g, dtype=torch.uint8).to(DEV)
        buf.next_frames[:n] = torch.randint(
            0, 256, (n, *vis), generator=g, dtype=torch.uint8).to(DEV)
    else:
        code = position_code(vis).to(DEV)
        buf.frames[:n] = code
        buf.next_frames[:n] = -code
    buf.size = n
    buf.ptr = n % buf.max_size
    buf._size_dev.fill_(n)
    return buf


def fields(b):
    return {"features": b.states.features, "frame": b.states.frame,
            "actions": b.actions, "rewards": b.rewards,
            "next_features": b.next_states.features,
            "next_frame": b.next_states.frame, "done": b.done}


def sampled(buf, B):
    out = buf.make_static_batch(B)
    buf.sample_into(out)
    torch.cuda.synchronize()
    return out


def check_shifts_in_range(out, pad):
    sh = out.shifts
    assert sh.dtype == torch.int32 and sh.shape == (out.actions.shape[0], 4)
    assert int(sh.min()) >= 0 and int(sh.max()) <= 2 * pad


# (3,8,8): the basic case.  (2,7,10): non-square, odd H, W % 4 != 0 (the
# scalar-store path with a partial last group).  (1,5,5): pad larger than
# the frame, every read clamps.  (3,84,84): 6 slices.  (2,12,10): B=1.
# (5,33,28): 165 rows over 2 slices, a short last slice.  (1,9,3200): 9
# rows over 8 slices of 2 rows, so the last three slices are empty.
EXACT = [((3, 8, 8), 4, 64), ((2, 7, 10), 3, 64), ((1, 5, 5), 6, 64),
         ((3, 84, 84), 4, 8), ((2, 12, 10), 3, 1), ((5, 33, 28), 2, 8),
         ((1, 9, 3200), 32, 4)]


@pytest.mark.parametrize("vis,pad,B", EXACT)
def test_shift_gather_exact_fp32(vis, pad, B):
    buf = make_buffer(vis, quantize=False)
    buf.set_random_shift(pad)
    out = sampled(buf, B)
    check_shifts_in_range(out, pad)
    slots = out.states.features[:, 0].to(torch.long)
    assert int(slots.min()) >= 0 and int(slots.max()) < N_SLOTS
    ref = buf.sample_at(slots, out.shifts)
    for (name, a), b in zip(fields(out).items(), fields(ref).values()):
        assert torch.equal(a, b), name
    if B > 1:
        # not the trivial batch: some row is off-centre in each frame
        assert bool((out.shifts[:, :2] != pad).any())
        assert bool((out.shifts[:, 2:] != pad).any())


def test_emitted_shifts_are_true():
    """Read the shift off the centre pixel through the position code:
    at (2,12,10) p=3 the source of output pixel (6,5) is (6+dy-3, 5+dx-3),
    inside the frame for every dy, dx in 0..6, so no clamp hides it."""
    vis, pad, (cy, cx) = (2, 12, 10), 3, (6, 5)
    C, H, W = vis
    buf = make_buffer(vis, quantize=False)
    buf.set_random_shift(pad)
    out = sampled(buf, 64)
    check_shifts_in_range(out, pad)
    for frame, sign, cols in ((out.states.frame, 1, slice(0, 2)),
                              (out.next_states.frame, -1, slice(2, 4))):
        code = (sign * frame[:, 0, cy, cx]).to(torch.long) - 1
        dy = code // W - cy + pad
        dx = code % W - cx + pad
        got = torch.stack([dy, dx], dim=1).to(torch.int32)
        assert torch.equal(got, out.shifts[:, cols])
    assert len(torch.unique(out.shifts)) > 1


@pytest.mark.parametrize("vis,pad,B", [((3, 8, 8), 4, 64),
                                       ((3, 84, 84), 4, 8)])
def test_shift_gather_u8(vis, pad, B):
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer

    buf = make_buffer(vis, quantize=True)
    buf.set_random_shift(pad)
    out = sampled(buf, B)
    check_shifts_in_range(out, pad)
    slots = out.states.features[:, 0].to(torch.long)
    for frame, store, cols in (
            (out.states.frame, buf.frames, slice(0, 2)),
            (out.next_states.frame, buf.next_frames, slice(2, 4))):
        stored = store[slots].to(torch.float32) / 127.5 - 1.0
        ref = VisualReplayBuffer.shift_frames(stored, out.shifts[:, cols],
                                              pad)
        assert torch.allclose(frame, ref, atol=1e-6, rtol=0), \
            (frame - ref).abs().max()
    assert torch.equal(out.actions, buf.actions[slots])
    assert torch.equal(out.rewards, buf.rewards[slots])
    assert torch.equal(out.done, buf.done[slots])
    assert torch.equal(out.next_states.features, buf.next_features[slots])


@pytest.mark.parametrize("quantize", [True, False])
def test_same_draw_as_the_plain_kernel(quantize):
    vis, B = (3, 8, 8), 64
    buf = make_buffer(vis, quantize=quantize)
    plain = sampled(buf, B)
    buf._philox.zero_()
    buf.set_random_shift(4)
    aug = sampled(buf, B)
    for name in ("features", "next_features", "actions", "rewards", "done"):
        assert torch.equal(fields(plain)[name], fields(aug)[name]), name
    assert not torch.equal(plain.states.frame, aug.states.frame)
    # switched off again: the plain path, bit for bit
    buf._philox.zero_()
    buf.set_random_shift(0)
    off = sampled(buf, B)
    assert off.shifts is None
    for (name, a), b in zip(fields(plain).items(), fields(off).values()):
        assert torch.equal(a, b), name


def test_shift_distribution():
    """B=1024, p=4: each of the 4 columns is uniform over 9 values, so a
    value's count is Binomial(1024, 1/9): mean 113.8, sigma 10.05; the
    bounds are mean +- 6 sigma.  State and next-state shifts are
    independent: P(equal) = 1/81, expected 12.6 rows of 1024."""
    pad, B = 4, 1024
    buf = make_buffer((3, 8, 8), quantize=True, seed=1234)
    buf.set_random_shift(pad)
    out = sampled(buf, B)
    sh = out.shifts.cpu()
    for col in range(4):
        counts = torch.bincount(sh[:, col], minlength=2 * pad + 1)
        print(f"shift column {col} counts: {counts.tolist()}")
        assert counts.numel() == 2 * pad + 1
        assert int(counts.min()) >= 53 and int(counts.max()) <= 174, counts
    same = int((sh[:, :2] == sh[:, 2:]).all(dim=1).sum())
    print(f"rows with state shift == next-state shift: {same}")
    assert same < B // 4
    first = out.shifts.clone()
    buf.sample_into(out)
    torch.cuda.synchronize()
    assert not torch.equal(first, out.shifts)


def test_visual_graphed_update_with_random_shift():
    """The captured visual SAC update with augmentation on: the shifted
    gather is the graph's first node and draws fresh shifts per replay."""
    from copy import deepcopy
    from torch_actor_critic_amd.algo.graph import GraphedSACUpdate
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import (VisualActor,
                                                      VisualDoubleCritic)
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    Fo.set_compute_dtype("fp32")
    torch.manual_seed(5)
    device = torch.device(DEV)
    actor = VisualActor(16, 4, (3, 64, 64), [32, 32],
                        act_limit=1.0).to(device)
    critic = VisualDoubleCritic(16, 4, (3, 64, 64), [32, 32]).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)

    buf = VisualReplayBuffer(200, act_dim=4, device=device)
    mo = MultiObservation(torch.randn(16, device=device),
                          torch.randn(3, 64, 64, device=device))
    buf.store(mo, np.zeros(4), 0.0, mo, 0.0)
    n = 100
    buf.features[:n].normal_()
    buf.next_features[:n].normal_()
    buf.frames[:n].random_(0, 255)
    buf.next_frames[:n].random_(0, 255)
    buf.actions[:n].uniform_(-1, 1)
    buf.rewards[:n].normal_()
    buf.size = n
    buf.ptr = n % buf.max_size
    buf._size_dev.fill_(n)
    buf.set_random_shift(4)

    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=8, start_steps=0, steps_per_epoch=1,
              max_ep_len=10, update_after=0, update_every=1, save_every=10)
    g = GraphedSACUpdate(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, 8, device)
    assert g.batch.shifts is not None
    p0 = pi_opt.fp.flat.clone()
    t0 = target_flat.clone()
    seen = []
    for _ in range(5):
        g.step()
        torch.cuda.synchronize()
        seen.append(g.batch.shifts.clone())
    assert all(int(s.min()) >= 0 and int(s.max()) <= 8 for s in seen)
    assert not torch.equal(seen[-2], seen[-1])
    assert not torch.allclose(p0, pi_opt.fp.flat)
    assert not torch.allclose(t0, target_flat)
    lq, lp = g.read_and_reset_losses(5)
    assert np.isfinite(lq) and np.isfinite(lp)
    assert torch.isfinite(pi_opt.fp.flat).all()
    assert torch.isfinite(q_opt.fp.flat).all()
    assert torch.isfinite(target_flat).all()
