"""The device Philox4x32-10 (replay_draw.h::philox4, as tac_kernels.hip and
fused.hip each compiled it) and every draw built on it, against the host
generator of kernel_refs.py, which test_kernel_refs.py holds to the
published known-answer vectors.

Words, slots, shifts, prioritized targets and the tg_fwd2-versus-tg_eps
comparison are exact.  Rings hold the slot index in their payload, so the
drawn slot is read back from the gathered data.  All samplers bump the
device counter before they draw, so the first call on a fresh buffer keys
on counter 1; gather2 and tg_fwd2 key on ctr + ctr_add and leave the
counter alone.

A ring above 2^32 slots cannot be entered through the bindings without
that much storage (the slot indexes the ring), so the modulus above one
word is checked on the host only (test_kernel_refs.py).
visual_sample_into_shift refuses pad = 0 by design; pad = 0 goes through
the buffer, which then launches the plain gather: its slots are checked
against the same draw.

Noise values (tg_eps, philox_randn_) are compared with the float64
Box-Muller of the same fp32 uniforms under
    |eps_kernel - eps64| <= 5e-5 * max(1, R),  R = sqrt(-2 ln u0),
5e-5 being the absolute tolerance of everything the project builds on this
noise (test_gpu_engine.py): a cap, not a measurement.  numpy's fp32
evaluation of the formula stays inside a tenth of it (test_kernel_refs.py);
a wrong word, sin for cos or swapped uniforms is off by O(1).  Worst
err / cap measured on an MI355X: tg_eps 0.0080, philox_randn_ 0.0084."""

import numpy as np
import pytest
import torch

import kernel_refs as kr
from test_gpu_visual_shift import make_buffer as make_visual

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


# -- the generator itself ---------------------------------------------------

WORD_SEEDS = [0, 1, 2 ** 32, 0x9e3779b97f4a7c15]
WORD_CHI = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3]
WORD_CLO0 = [0, 2 ** 32 - 3]
WORD_N = 257


@pytest.mark.parametrize("seed", WORD_SEEDS, ids=hex)
def test_philox_words_match_host(ext, seed):
    """Both translation units' copies, word for word, with subsequences
    crossing the 32-bit boundary of the counter's low word."""
    for chi in WORD_CHI:
        for clo0 in WORD_CLO0:
            want = torch.from_numpy(
                kr.philox_rows(seed, chi, WORD_N, clo0).astype(np.int64))
            a = ext.philox_words(kr.as_i64(seed), chi, clo0, WORD_N)
            b = ext.philox_words2(kr.as_i64(seed), chi, clo0, WORD_N)
            assert a.dtype == torch.int64 and a.shape == (WORD_N, 4)
            assert torch.equal(a, b), (hex(chi), clo0)
            msg = kr.describe_mismatch(a.cpu(), want)
            assert not msg, (hex(chi), clo0, msg)
    with pytest.raises(RuntimeError, match="philox_words"):
        ext.philox_words(0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="philox_words2"):
        ext.philox_words2(0, 0, 0, 0)


# -- uniform replay ---------------------------------------------------------

def _ring(cap, size, seed, obs=3, act=2):
    """state[:, 0] = slot, every other field a function of the slot."""
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    buf = ReplayBuffer(cap, obs, act, device=DEV, seed=seed)
    slot = torch.arange(cap, dtype=torch.float32, device=DEV)
    buf.state.copy_(slot[:, None] + torch.arange(obs, device=DEV)[None] * 0.25)
    buf.next_state.copy_(buf.state + 0.5)
    buf.actions.copy_(-slot[:, None] - torch.arange(act, device=DEV)[None])
    buf.rewards.copy_(slot * 3)
    buf.done.copy_(slot % 2)
    buf.size = size
    buf.ptr = size % cap
    buf._size_dev.fill_(size)
    return buf


def _want_slots(seed, ctr, B, size):
    w = kr.philox_rows(seed, ctr, B)
    return torch.from_numpy(kr.draw_index(w[:, 0], w[:, 1], size))


def _check_rows(buf, b, want):
    slots = b.states[:, 0].cpu().long()
    assert torch.equal(slots, want)
    ref = buf.sample_at(want.to(DEV))
    for f in ("states", "actions", "rewards", "next_states", "done"):
        assert torch.equal(getattr(b, f), getattr(ref, f)), f


@pytest.mark.parametrize("B", [64, 333])
@pytest.mark.parametrize("size", [1, 48, 5000])
def test_replay_sample_draws_host_slots(size, B):
    seed = 1234 + size
    buf = _ring(max(size, 8), size, seed)
    b = buf.sample(B)                       # replay_sample, counter 1
    assert int(buf._philox) == 1
    _check_rows(buf, b, _want_slots(seed, 1, B, size))
    out = buf.make_static_batch(B)
    buf.sample_into(out)                    # replay_sample_into, counter 2
    assert int(buf._philox) == 2
    _check_rows(buf, out, _want_slots(seed, 2, B, size))
    if size > 1:
        assert not torch.equal(b.states, out.states)
    # a counter whose high word is set keys c2 and c3 alike
    buf._philox.fill_(2 ** 33 + 6)
    b = buf.sample(B)
    _check_rows(buf, b, _want_slots(seed, 2 ** 33 + 7, B, size))


# -- gather2 and the counter bump qloss2 commits ----------------------------

def _gather2(ext, buf, ctr, B, ctr_add, ldc=8):
    xc = torch.full((2 * B, ldc), kr.SENTINEL, device=DEV)
    xc2 = torch.full((B, ldc), kr.SENTINEL, device=DEV)
    rew = torch.zeros(B, device=DEV)
    done = torch.zeros(B, device=DEV)
    ext.gather2(buf.state, buf.actions, buf.rewards, buf.next_state,
                buf.done, buf._size_dev, ctr, buf._philox_seed, xc, xc2,
                rew, done, B, ctr_add)
    return xc, xc2, rew, done


def _check_gather2(buf, got, want):
    xc, xc2, rew, done = got
    B, O, A = want.numel(), buf.obs_dim, buf.act_dim
    w = want.to(DEV)
    assert torch.equal(xc[:B, 0].cpu().long(), want)
    assert torch.equal(xc[:B, :O], buf.state[w])
    assert torch.equal(xc2[:, :O], buf.state[w])
    assert torch.equal(xc[:B, O:O + A], buf.actions[w])
    assert torch.equal(xc[B:, :O], buf.next_state[w])
    assert torch.equal(rew, buf.rewards[w]) and torch.equal(done, buf.done[w])
    assert bool((xc[:, O + A:] == kr.SENTINEL).all())
    assert bool((xc2[:, O:] == kr.SENTINEL).all())


@pytest.mark.parametrize("B", [64, 333])
def test_gather2_keys_on_ctr_plus_ctr_add(ext, B):
    seed, size = 77, 5000
    buf = _ring(size, size, seed)
    ctr = torch.full((1,), 9, dtype=torch.int64, device=DEV)
    for add in (0, 1):
        got = _gather2(ext, buf, ctr, B, add)
        assert int(ctr) == 9                # gather2 never bumps
        _check_gather2(buf, got, _want_slots(seed, 9 + add, B, size))
    # the engine's schedule: gather2(ctr_add=1), qloss2 commits the bump,
    # the next gather2(ctr_add=1) draws the next counter
    h = kr.QLOSS_HYPER
    t = {k: v.to(DEV) for k, v in kr.qloss_inputs(64, 0).items()}
    steps = [torch.full((1,), v, dtype=torch.int64, device=DEV)
             for v in (100, 200)]
    z = lambda *s: torch.zeros(*s, device=DEV)
    ext.qloss2(t["q1"], t["q2"], t["q1t"], t["q2t"], t["logp"], t["rew"],
               t["done"], None, h["alpha"], z(1), z(64), z(64), 64,
               h["gamma"], h["scale"], None, None, None, None, 0,
               ctr, steps[0], steps[1])
    assert [int(ctr), int(steps[0]), int(steps[1])] == [10, 101, 201]
    got = _gather2(ext, buf, ctr, B, 1)
    _check_gather2(buf, got, _want_slots(seed, 11, B, size))
    assert not torch.equal(_want_slots(seed, 10, B, size),
                           _want_slots(seed, 11, B, size))


# -- visual gather: slots and the four shifts ---------------------------------

@pytest.mark.parametrize("quant", [True, False], ids=["u8", "fp32"])
@pytest.mark.parametrize("vis", [(1, 8, 8), (1, 7, 5)],
                         ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_visual_gather_draws_host_slots_and_shifts(pad, vis, quant):
    B, n, seed = 64, 300, 5 + pad
    buf = make_visual(vis, quant, seed=seed, n=n)
    w = kr.philox_rows(seed, 1, B)
    want_slots = torch.from_numpy(kr.draw_index(w[:, 0], w[:, 1], n))
    want_shifts = torch.from_numpy(
        kr.draw_shifts(w[:, 2], w[:, 3], pad)).to(torch.int32)
    plain = buf.make_static_batch(B)        # shift_pad = 0: plain gather
    assert plain.shifts is None
    buf.sample_into(plain)
    assert int(buf._philox) == 1
    assert torch.equal(plain.states.features[:, 0].cpu().long(), want_slots)
    if pad == 0:
        assert not want_shifts.any()        # span 1: every shift is 0
        with pytest.raises(RuntimeError, match="pad"):
            _ = _shift_binding_pad0(buf, plain)
        assert int(buf._philox) == 1        # refused before the bump
        return
    buf.set_random_shift(pad)
    buf._philox.fill_(0)                    # the same counter again
    out = buf.make_static_batch(B)
    buf.sample_into(out)                    # visual_sample_into_shift
    assert int(buf._philox) == 1
    assert torch.equal(out.states.features[:, 0].cpu().long(), want_slots)
    assert torch.equal(out.shifts.cpu(), want_shifts + pad)
    assert int(want_shifts.min()) == -pad and int(want_shifts.max()) == pad
    ref = buf.sample_at(want_slots.to(DEV), (want_shifts + pad).to(DEV))
    tol = dict(atol=1e-6, rtol=0) if quant else dict(atol=0, rtol=0)
    torch.testing.assert_close(out.states.frame, ref.states.frame, **tol)
    torch.testing.assert_close(out.next_states.frame,
                               ref.next_states.frame, **tol)
    assert torch.equal(out.rewards, ref.rewards)


def _shift_binding_pad0(buf, out):
    from torch_actor_critic_amd.ops import require_extension
    shifts = torch.zeros(out.actions.shape[0], 4, dtype=torch.int32,
                         device=DEV)
    require_extension().visual_sample_into_shift(
        buf.features, buf.frames, buf.next_features, buf.next_frames,
        buf.actions, buf.rewards, buf.done, buf._size_dev, buf._philox,
        buf._philox_seed, out.states.features, out.states.frame,
        out.next_states.features, out.next_states.frame, out.actions,
        out.rewards, out.done, 0, buf.vis_dim[-2], buf.vis_dim[-1], shifts)


# -- prioritized targets ------------------------------------------------------

@pytest.mark.parametrize("B", [64, 333])
def test_per_sample_targets_match_host(ext, B):
    from test_per import make_per, random_priorities, set_leaves
    size, seed = 5000, 31
    buf = make_per(size, DEV, obs_dim=1)
    set_leaves(buf, random_priorities(size, size + B).to(DEV))
    root = float(buf.per_levels()[0][0])
    for ctr in (1, 2):
        _, _, u = ext.per_sample(buf._per_tree, size, buf._philox, seed, B)
        assert int(buf._philox) == ctr
        w = kr.philox_rows(seed, ctr, B)
        want = kr.per_targets(w[:, 0], root, B)
        assert np.array_equal(u.cpu().numpy(), want), ctr


# -- noise --------------------------------------------------------------------

def _noise_check(name, got, want64, radius):
    cap = kr.NOISE_CAP * np.maximum(1.0, radius)
    ratio = float((np.abs(got.astype(np.float64) - want64) / cap).max())
    print(f"{name}: worst err / cap = {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)
    return ratio


@pytest.mark.parametrize("R,A", [(1, 1), (3, 6), (5, 17), (2, 64)])
def test_tg_eps_against_host(ext, R, A):
    like = torch.zeros(1, device=DEV)
    for seed, ctr in ((0, 1), (kr.TG_SEED, kr.TG_CTR), (-5, 2 ** 33 + 1)):
        got = ext.tg_eps(ctr, seed, R, A, like)
        assert got.shape == (R, A) and got.dtype == torch.float32
        want, radius = kr.noise_eps64(seed, ctr, R, A)
        _noise_check(f"tg_eps R={R} A={A} seed={seed}",
                     got.cpu().numpy(), want, radius)


@pytest.mark.parametrize("n", [1, 4, 5, 1023])
def test_philox_randn_against_host(ext, n):
    seed = 42
    buf = torch.full((n + 2 * GUARD,), kr.SENTINEL, device=DEV)
    out = buf[GUARD:GUARD + n]
    ctr = torch.full((1,), 6, dtype=torch.int64, device=DEV)
    ext.philox_randn_(out, ctr, seed)
    assert int(ctr) == 7                    # bumped, then keyed on 7
    b = buf.cpu()
    assert bool((b[:GUARD] == kr.SENTINEL).all()), "write before the start"
    assert bool((b[-GUARD:] == kr.SENTINEL).all()), "tail written past n"
    n4 = -(-n // 4)
    w = kr.philox_rows(seed, 7, n4)
    u = [kr.uniform32(w[:, k]) for k in range(4)]
    c0, s0, r0 = kr.box_muller64(u[0], u[1])
    c1, s1, r1 = kr.box_muller64(u[2], u[3])
    want = np.stack([c0, s0, c1, s1], 1).reshape(-1)[:n]
    radius = np.stack([r0, r0, r1, r1], 1).reshape(-1)[:n]
    _noise_check(f"philox_randn_ n={n}", out.cpu().numpy(), want, radius)


@pytest.mark.parametrize("R,A", [(1, 1), (3, 6), (5, 17), (2, 64)])
def test_tg_fwd2_noise_is_tg_eps(ext, R, A):
    """hl = 0: mu = 0, log_std = 0, std = 1, so prob_out is the noise bit
    for bit; the key is the device counter plus ctr_add."""
    seed = kr.TG_SEED
    hl = torch.zeros(R, 2 * A, device=DEV)
    ctr = torch.full((1,), kr.TG_CTR, dtype=torch.int64, device=DEV)
    for add in (0, 1):
        out0 = torch.zeros(R, A, device=DEV)
        logp = torch.zeros(R, device=DEV)
        prob = torch.full((R, A), kr.SENTINEL, device=DEV)
        ext.tg_fwd2(hl, out0, 0, out0, 0, R, logp, prob, ctr, seed,
                    1.0, -5.0, 2.0, add)
        assert int(ctr) == kr.TG_CTR        # tg_fwd2 never bumps
        eps = ext.tg_eps(kr.TG_CTR + add, seed, R, A, hl)
        assert torch.equal(prob, eps), add
    if R * A > 1:
        assert not torch.equal(ext.tg_eps(kr.TG_CTR, seed, R, A, hl),
                               ext.tg_eps(kr.TG_CTR + 1, seed, R, A, hl))
