"""GPU tests of ``visual_gather_n_kernel`` and ``visual_store_n_kernel``:
n-step returns in the one-kernel Philox gather of the visual replay
buffer, with and without the random shift, against
``VisualReplayBuffer.sample_at(slots, shifts, n)`` on the visual ring of
tests/test_visual_nstep.py (pinned there to a literal per-row loop).

``features[:, 0]`` of a sampled row is the global step t, so the slot the
kernel drew is ``t % 48``.  With gamma = 0.5 and small-integer rewards
every product and partial sum is exact in fp32, and the shift is an
integer translation, so the fp32-buffer comparisons are bit-exact; the
u8-buffer frames carry only the dequantisation's rounding (``atol=1e-6``,
as in tests/test_gpu_visual_shift.py).
"""

from copy import deepcopy

import numpy as np
import pytest
import torch

from test_nstep import (KIND_T, N, RING, T_TOTAL, episode_flags, frac_reward,
                        window_kinds)
from test_visual_nstep import (ACT, FEAT, fields, fill_ring,
                               make_visual_ring, slots_of)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def sampled(buf, B):
    out = buf.make_static_batch(B)
    buf.sample_into(out)
    torch.cuda.synchronize()
    return out


def assert_equal_to_sample_at(out, buf, n, frames_atol=None,
                              values_atol=None):
    """Every field equal to sample_at at the drawn slots and shifts;
    ``frames_atol`` for u8 frames, ``values_atol`` for reward and done at
    a gamma whose products are not exact."""
    ref = buf.sample_at(slots_of(out), out.shifts, n)
    for (name, a), b in zip(fields(out).items(), fields(ref).values()):
        atol = None
        if name in ("frame", "next_frame"):
            atol = frames_atol
        elif name in ("rewards", "done"):
            atol = values_atol
        if atol is not None:
            assert torch.allclose(a, b, atol=atol, rtol=0), \
                (name, float((a - b).abs().max()))
        else:
            assert torch.equal(a, b), name
    return ref


def t_first_last(out):
    return (out.states.features[:, 0].cpu(),
            (out.next_states.features[:, 0] - 1000).cpu())


def one_step_twin(buf, counter=0):
    """The same ring read by the 1-step kernels at the given counter."""
    buf.set_n_step(1, buf.gamma)
    buf._philox.fill_(counter)
    return buf


def test_gather_n_exact_fp32():
    buf = make_visual_ring(DEV, gamma=0.5)
    out = sampled(buf, 1024)
    assert int(buf._philox.item()) == 1 and out.shifts is None
    assert_equal_to_sample_at(out, buf, N)
    # input condition: every window kind is among the drawn rows
    kinds = window_kinds(*t_first_last(out))
    assert kinds == set(KIND_T), kinds
    # same counter, the 1-step kernel: the same slots are drawn
    one = sampled(one_step_twin(buf), 1024)
    assert torch.equal(one.states.features, out.states.features)
    assert torch.equal(one.states.frame, out.states.frame)
    assert_equal_to_sample_at(one, buf, 1)


# (3,8,8): the basic case.  (2,7,10): W % 4 != 0, the scalar tail.
# (1,5,5): pad larger than the frame, every read clamps.  (3,84,84): 6
# slices that must agree on the last slot.  (5,33,28): 165 rows over 2
# slices, a short last slice.  (1,9,3200): 9 rows over 8 slices of 2 rows,
# so the last three slices are empty and still reach the barrier.
# n = 2: two-slot windows.  n = 64: windows longer than any episode.
SHIFTED = [((3, 8, 8), 4, 1024, N), ((2, 7, 10), 3, 256, N),
           ((1, 5, 5), 6, 64, N), ((3, 84, 84), 4, 64, N),
           ((5, 33, 28), 2, 64, N), ((1, 9, 3200), 32, 8, N),
           ((3, 8, 8), 2, 64, 2), ((3, 8, 8), 2, 64, 64),
           ((2, 12, 10), 3, 1, N)]


@pytest.mark.parametrize("vis,pad,B,n", SHIFTED)
def test_gather_n_shift_exact_fp32(vis, pad, B, n):
    # seed 2: row 0 draws slot 23 at counter 1 (t = 23, window 23..26),
    # so the single row of the B = 1 case is a multi-slot window
    buf = make_visual_ring(DEV, vis=vis, gamma=0.5, n_step=n, seed=2)
    buf.set_random_shift(pad)
    out = sampled(buf, B)
    sh = out.shifts
    assert sh.dtype == torch.int32 and sh.shape == (B, 4)
    assert int(sh.min()) >= 0 and int(sh.max()) <= 2 * pad
    assert_equal_to_sample_at(out, buf, n)
    t0, t1 = t_first_last(out)
    assert bool((t1 != t0).any())           # some window has > 1 slot
    assert int((t1 - t0).max()) <= n - 1
    if B > 1:
        # not the trivial batch: some row is off-centre in each frame
        assert bool((sh[:, :2] != pad).any())
        assert bool((sh[:, 2:] != pad).any())
    # a shifted 1-step buffer at the same counter: same slots and shifts
    one = sampled(one_step_twin(buf), B)
    assert torch.equal(one.states.features, out.states.features)
    assert torch.equal(one.shifts, sh)
    assert torch.equal(one.states.frame, out.states.frame)


@pytest.mark.parametrize("vis,pad,B", [((3, 8, 8), 0, 256),
                                       ((3, 84, 84), 0, 16),
                                       ((2, 7, 10), 0, 64),
                                       ((3, 8, 8), 4, 256),
                                       ((3, 84, 84), 4, 16),
                                       ((2, 7, 10), 3, 64)])
def test_gather_n_u8(vis, pad, B):
    buf = make_visual_ring(DEV, vis=vis, quantize=True, gamma=0.5)
    assert buf.frames.dtype == torch.uint8
    buf.set_random_shift(pad)
    out = sampled(buf, B)
    assert (out.shifts is None) == (pad == 0)
    assert_equal_to_sample_at(out, buf, N, frames_atol=1e-6)
    t0, t1 = t_first_last(out)
    assert bool((t1 != t0).any())
    # the next frame is the last slot's, not the drawn slot's
    own = buf.sample_at(slots_of(out), out.shifts, 1).next_states.frame
    assert not torch.allclose(out.next_states.frame, own, atol=0.1)


@pytest.mark.parametrize("vis", [(3, 8, 8), (2, 7, 10)])
def test_gather_n_unshifted_exact_fp32_shapes(vis):
    """The unshifted n-step path at a vector and a scalar-tail width."""
    buf = make_visual_ring(DEV, vis=vis, gamma=0.5)
    out = sampled(buf, 64)
    assert_equal_to_sample_at(out, buf, N)
    t0, t1 = t_first_last(out)
    assert bool((t1 != t0).any())


@pytest.mark.parametrize("pad", [0, 4])
def test_gather_n_general_gamma(pad):
    """gamma = 0.99, non-integer rewards.  Copies are exact; reward and
    done carry the bound derived in
    tests/test_gpu_nstep.py::test_replay_sample_n_general_gamma: the
    kernel may only fuse a multiply into the following add, each such
    step differs by one rounding of a value bounded by S = sum_m
    |gamma^m r_m| (resp. 1 + gamma^(M-1)), with at most n steps in the sum
    and n in the discount chain, counted on both sides: 4 n 2^-24 S."""
    gamma = 0.99
    buf = make_visual_ring(DEV, gamma=gamma, reward=frac_reward)
    buf.set_random_shift(pad)
    out = sampled(buf, 1024)
    ref = buf.sample_at(slots_of(out), out.shifts, N)
    for name in ("features", "frame", "actions", "next_features",
                 "next_frame"):
        assert torch.equal(fields(out)[name], fields(ref)[name]), name
    t0, t1 = (x.numpy().astype(np.int64) for x in t_first_last(out))
    r = np.array([frac_reward(t) for t in range(T_TOTAL)], dtype=np.float64)
    S = np.array([sum(abs(gamma ** m * r[a + m]) for m in range(z - a + 1))
                  for a, z in zip(t0, t1)])
    eps = 4 * N * 2.0 ** -24
    d_rew = (out.rewards - ref.rewards).abs().cpu().numpy().astype(np.float64)
    d_done = (out.done - ref.done).abs().cpu().numpy().astype(np.float64)
    print("max |d reward| / bound:", float((d_rew / (eps * S + 1e-300)).max()),
          " max |d done| / bound:",
          float((d_done / (eps * (1 + gamma ** (t1 - t0)))).max()))
    assert (d_rew <= eps * S).all()
    assert (d_done <= eps * (1 + gamma ** (t1 - t0))).all()
    # and the values are what float64 says, to fp32 accuracy
    np.testing.assert_allclose(
        out.rewards.cpu().numpy(),
        [sum(gamma ** m * r[a + m] for m in range(z - a + 1))
         for a, z in zip(t0, t1)], rtol=0, atol=float(eps * S.max()))
    done_flag, _ = episode_flags(T_TOTAL)
    np.testing.assert_allclose(
        out.done.cpu().numpy(),
        1.0 - gamma ** (t1 - t0) * (1.0 - done_flag[t1].astype(np.float64)),
        rtol=0, atol=float((eps * (1 + gamma ** (t1 - t0))).max()))


def test_gather_n_empty_ring_reads_slot_zero_only():
    buf = make_visual_ring(DEV, gamma=0.5, total=1)
    # one transition gave the ring its shape; empty it again
    buf.ptr = buf.size = 0
    buf._size_dev.zero_()
    buf._ptr_dev.zero_()
    buf.rewards.fill_(1.0)
    out = sampled(buf, 64)
    assert torch.equal(out.rewards, torch.ones_like(out.rewards))
    assert torch.equal(out.done, torch.zeros_like(out.done))
    assert torch.equal(out.next_states.frame,
                       buf.next_frames[:1].expand_as(out.next_states.frame))


@pytest.mark.parametrize("quantize", [False, True])
def test_store_fast_path_equals_the_cpu_ring(quantize):
    cpu = make_visual_ring("cpu", quantize=quantize)
    gpu = make_visual_ring(DEV, quantize=quantize)
    torch.cuda.synchronize()
    assert gpu._native_ext() is not None
    assert gpu.ptr == cpu.ptr == 12 and gpu.size == cpu.size == RING
    assert int(gpu._ptr_dev.item()) == 12
    assert int(gpu._size_dev.item()) == RING
    for name in ("episode_end", "rewards", "done", "actions", "features",
                 "next_features", "frames", "next_frames"):
        a, b = getattr(gpu, name).cpu(), getattr(cpu, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert float(gpu.episode_end.sum()) > float(gpu.done.sum()) > 0
    # end defaults to done, and the write head wraps to 0 in the mirror
    small = make_visual_ring(DEV, size=4, total=0)
    fill_ring(small, total=4, pass_end=False)       # t = 3 is terminal
    torch.cuda.synchronize()
    assert int(small._ptr_dev.item()) == 0 == small.ptr
    assert small.done.tolist() == [0.0, 0.0, 0.0, 1.0]
    assert torch.equal(small.episode_end, small.done)


def test_captured_replay_draws_fresh_windows():
    buf = make_visual_ring(DEV, gamma=0.5)
    buf.set_random_shift(4)
    out = buf.make_static_batch(256)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        buf.sample_into(out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.sample_into(out)
    seen = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert_equal_to_sample_at(out, buf, N)
        t0, t1 = t_first_last(out)
        assert bool((t1 != t0).any())
        seen.append((out.states.features[:, 0].clone(), out.shifts.clone()))
    for (a_t, a_s), (b_t, b_s) in zip(seen, seen[1:]):
        assert not torch.equal(a_t, b_t) and not torch.equal(a_s, b_s)


def test_visual_graphed_update_on_an_nstep_shifted_buffer():
    from torch_actor_critic_amd.algo.graph import GraphedSACUpdate
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.models.visual import (VisualActor,
                                                      VisualDoubleCritic)
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    Fo.set_compute_dtype("fp32")
    torch.manual_seed(5)
    device = torch.device(DEV)
    vis = (3, 64, 64)
    actor = VisualActor(FEAT, ACT, vis, [32, 32], act_limit=1.0).to(device)
    critic = VisualDoubleCritic(FEAT, ACT, vis, [32, 32]).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)

    buf = make_visual_ring(DEV, vis=vis, quantize=True, gamma=0.99, n_step=3)
    buf.set_random_shift(4)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=8, start_steps=0, steps_per_epoch=1,
              max_ep_len=10, update_after=0, update_every=1, save_every=10,
              n_step=3, aug_shift=4)
    g = GraphedSACUpdate(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, 8, device)
    assert g.batch.shifts is not None
    p0, q0 = pi_opt.fp.flat.clone(), q_opt.fp.flat.clone()
    t0 = target_flat.clone()
    for _ in range(3):
        g.step()
        torch.cuda.synchronize()
        # gamma = 0.99: reward and done within a few fp32 roundings of
        # the unfused reference (|r| <= 8, 3 terms)
        assert_equal_to_sample_at(g.batch, buf, 3, frames_atol=1e-6,
                                  values_atol=1e-5)
    assert not torch.allclose(p0, pi_opt.fp.flat)
    assert not torch.allclose(q0, q_opt.fp.flat)
    assert not torch.allclose(t0, target_flat)
    lq, lp = g.read_and_reset_losses(3)
    assert np.isfinite(lq) and np.isfinite(lp)
    assert torch.isfinite(pi_opt.fp.flat).all()
    assert torch.isfinite(q_opt.fp.flat).all()
    assert torch.isfinite(target_flat).all()
