"""HBM-resident replay buffer.

API-compatible with the reference ``ReplayBuffer``
(``buffer/replay_buffer.py:8-54``: ctor (size, obs_dim, act_dim),
``store(obs, act, rew, next_obs, done)``, ``sample(batch_size) -> Batch``)
but designed for MI355X:

* Storage is preallocated **device tensors** — 1M HalfCheetah transitions
  (~200 MB fp32) sit in the 288 GB HBM3E and never round-trip to host.
* ``sample`` on GPU is ONE fused HIP kernel: Philox uniform index draw +
  gather of all five fields into contiguous batch tensors, with the
  Philox counter held in device memory so the kernel is hipGraph-
  replayable (each replay draws fresh indices).
* Sampling is with replacement (deviation from the reference's
  ``random.sample`` without replacement, buffer/replay_buffer.py:46 —
  collision probability for 64 of 1e6 is negligible and the on-device
  draw avoids a host round-trip; documented per SURVEY.md Q8).
* ``store`` accepts single transitions (reference semantics) or batched
  slabs (``store_batch``) that stream host->device asynchronously.
* Optional n-step returns (extension, default off): after
  ``set_n_step(n, gamma)`` every sampler returns the discounted n-step
  reward sum, the next state n steps later and an *effective* done, so
  the unchanged 1-step loss kernels compute the n-step Bellman target
  (``sample_at`` is the executable definition).
"""

import typing as t
from dataclasses import dataclass

import numpy as np
import torch


@dataclass(frozen=True)
class Batch:
    """``done`` is the *effective* done: with 1-step sampling the stored
    flag; with n-step sampling ``1 - gamma^(M-1) * (1 - done[last])`` for
    a window of M <= n transitions, so that ``gamma * (1 - done)`` in the
    loss equals ``gamma^M * (1 - done[last])``.  ``rewards`` is then the
    discounted sum over the window and ``next_states`` its last slot's."""
    states: torch.Tensor
    actions: torch.Tensor
    rewards: torch.Tensor
    next_states: torch.Tensor
    done: torch.Tensor


class ReplayBuffer:
    def __init__(self, size: int, obs_dim: int, act_dim: int,
                 device: t.Union[str, torch.device] = "cpu",
                 seed: int = 0):
        size = int(size)
        self.device = torch.device(device)
        self.obs_dim = obs_dim
        self.act_dim = act_dim
        dev = self.device
        self.state = torch.zeros((size, obs_dim), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((size, act_dim), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(size, dtype=torch.float32, device=dev)
        self.next_state = torch.zeros((size, obs_dim), dtype=torch.float32, device=dev)
        self.done = torch.zeros(size, dtype=torch.float32, device=dev)

        self.ptr = 0
        self.size = 0
        self.max_size = size

        self._rng = np.random.default_rng(seed)
        # Device-side Philox state for the fused sample+gather kernel:
        # [counter]; seed passed separately. Incremented BY the kernel.
        self._philox = torch.zeros(1, dtype=torch.int64, device=dev)
        self._philox_seed = seed
        # device-side valid-size mirror for graph-captured sampling
        self._size_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        # n-step returns (set_n_step): off by default — nothing below is
        # allocated, copied or launched while n_step == 1
        self.n_step = 1
        self.gamma = 1.0
        self.episode_end: t.Optional[torch.Tensor] = None
        self._ptr_dev: t.Optional[torch.Tensor] = None

    MAX_N_STEP = 64   # one wave64 lane per window slot in the gather kernels

    def set_n_step(self, n: int, gamma: float) -> None:
        """Sample n-step returns with discount ``gamma`` from now on.
        For n > 1 the ring gains an ``episode_end`` field (1 where an
        episode ended after the transition for ANY reason, truncation
        included) and a device mirror of the write head, so the buffer
        must still be empty."""
        n = int(n)
        if not 1 <= n <= self.MAX_N_STEP:
            raise ValueError(
                f"n_step must be in 1..{self.MAX_N_STEP}, got {n}")
        if n > 1 and self.episode_end is None:
            if self.size != 0:
                raise ValueError(
                    "set_n_step(n > 1) needs an empty buffer: transitions "
                    "stored so far carry no episode boundaries")
            self.episode_end = torch.zeros(self.max_size,
                                           dtype=torch.float32,
                                           device=self.device)
            self._ptr_dev = torch.zeros(1, dtype=torch.int64,
                                        device=self.device)
            self._ptr_dev.fill_(self.ptr)
        self.n_step = n
        self.gamma = float(gamma)

    # -- store ----------------------------------------------------------

    def _to_dev(self, x, shape) -> torch.Tensor:
        tt = torch.as_tensor(x, dtype=torch.float32)
        return tt.reshape(shape)

    def store(self, obs, act, rew, next_obs, done, end=None):
        """``end`` (default: ``done``) marks the last transition of an
        episode, whatever ended it; only n-step sampling reads it."""
        i = self.ptr
        self.state[i] = self._to_dev(obs, (self.obs_dim,))
        self.actions[i] = self._to_dev(act, (self.act_dim,))
        self.rewards[i] = float(rew)
        self.next_state[i] = self._to_dev(next_obs, (self.obs_dim,))
        self.done[i] = float(done)
        if self.episode_end is not None:
            self.episode_end[i] = float(done if end is None else end)
        self.ptr = (self.ptr + 1) % self.max_size
        self.size = min(self.size + 1, self.max_size)
        self._size_dev.fill_(self.size)
        if self._ptr_dev is not None:
            self._ptr_dev.fill_(self.ptr)

    def store_batch(self, obs, act, rew, next_obs, done, end=None):
        """Vectorized ring write of n transitions (one or two slab copies)."""
        obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32)
        n = obs.shape[0]
        act = torch.as_tensor(np.asarray(act), dtype=torch.float32).reshape(n, self.act_dim)
        rew = torch.as_tensor(np.asarray(rew), dtype=torch.float32).reshape(n)
        next_obs = torch.as_tensor(np.asarray(next_obs), dtype=torch.float32).reshape(n, self.obs_dim)
        done = torch.as_tensor(np.asarray(done), dtype=torch.float32).reshape(n)
        fields = [(self.state, obs.reshape(n, self.obs_dim)),
                  (self.actions, act), (self.rewards, rew),
                  (self.next_state, next_obs), (self.done, done)]
        if self.episode_end is not None:
            end = done if end is None else torch.as_tensor(
                np.asarray(end), dtype=torch.float32).reshape(n)
            fields.append((self.episode_end, end))
        n_total = n
        if n > self.max_size:
            # only the last max_size transitions survive a full wrap
            keep = self.max_size
            fields = [(dst, src[-keep:]) for (dst, src) in fields]
            self.ptr = (self.ptr + (n - keep)) % self.max_size
            n = keep
        first = min(n, self.max_size - self.ptr)
        for (dst, src) in fields:
            dst[self.ptr:self.ptr + first].copy_(src[:first], non_blocking=True)
            if n > first:
                dst[:n - first].copy_(src[first:], non_blocking=True)
        self.ptr = (self.ptr + n) % self.max_size
        self.size = min(self.size + n_total, self.max_size)
        self._size_dev.fill_(self.size)
        if self._ptr_dev is not None:
            self._ptr_dev.fill_(self.ptr)

    # -- sample ---------------------------------------------------------

    def _native_ext(self):
        if self.device.type != "cuda":
            return None
        from ..ops import use_native, require_extension
        if use_native(self.state):
            return require_extension()
        return None

    def sample(self, batch_size: int) -> Batch:
        ext = self._native_ext()
        if ext is not None and self.n_step > 1:
            s, a, r, ns, d = ext.replay_sample_n(
                self.state, self.actions, self.rewards, self.next_state,
                self.done, self.episode_end, self._size_dev, self._ptr_dev,
                self._philox, self._philox_seed, self.n_step, self.gamma,
                batch_size)
            return Batch(s, a, r, ns, d)
        if ext is not None:
            s, a, r, ns, d = ext.replay_sample(
                self.state, self.actions, self.rewards, self.next_state,
                self.done, self._size_dev, self._philox, self._philox_seed,
                batch_size)
            return Batch(s, a, r, ns, d)
        idx = self._rng.choice(self.size, size=batch_size, replace=False)
        idx = torch.as_tensor(idx, dtype=torch.long, device=self.device)
        return self.sample_at(idx)

    def make_static_batch(self, batch_size: int) -> Batch:
        """Preallocated batch tensors for hipGraph-captured sampling."""
        f32 = dict(dtype=torch.float32, device=self.device)
        return Batch(torch.zeros(batch_size, self.obs_dim, **f32),
                     torch.zeros(batch_size, self.act_dim, **f32),
                     torch.zeros(batch_size, **f32),
                     torch.zeros(batch_size, self.obs_dim, **f32),
                     torch.zeros(batch_size, **f32))

    def sample_into(self, out: Batch) -> None:
        """Graph-capturable sampling into preallocated batch tensors."""
        ext = self._native_ext()
        if ext is not None and self.n_step > 1:
            ext.replay_sample_into_n(
                self.state, self.actions, self.rewards, self.next_state,
                self.done, self.episode_end, self._size_dev, self._ptr_dev,
                self._philox, self._philox_seed, self.n_step, self.gamma,
                out.states, out.actions, out.rewards, out.next_states,
                out.done)
            return
        if ext is not None:
            ext.replay_sample_into(
                self.state, self.actions, self.rewards, self.next_state,
                self.done, self._size_dev, self._philox, self._philox_seed,
                out.states, out.actions, out.rewards, out.next_states,
                out.done)
            return
        idx = torch.randint(0, max(self.size, 1), (out.states.shape[0],),
                            device=self.device)
        b = self.sample_at(idx)
        out.states.copy_(b.states)
        out.actions.copy_(b.actions)
        out.rewards.copy_(b.rewards)
        out.next_states.copy_(b.next_states)
        out.done.copy_(b.done)

    def sample_at(self, idx: torch.Tensor,
                  n_step: t.Optional[int] = None) -> Batch:
        """The batch for ring slots ``idx`` (plain torch, CPU or GPU) —
        the definition the n-step gather kernels are tested against.

        For slot i the window walks j = i, i+1, ... (mod max_size), adding
        ``gamma^m * rewards[j]`` in fp32 in this order, and closes at the
        first j with ``done[j]`` or ``episode_end[j]`` set, at the newest
        slot (the walk never crosses the write head) or after n slots.
        With M slots walked and j the last one: state/action come from
        slot i, next_state from slot j, reward is the sum and done is
        ``1 - gamma^(M-1) * (1 - done[j])`` (gamma^(M-1) by repeated fp32
        multiply).  A truncated episode (episode_end without done) thus
        bootstraps from its own last next_state.  ``n_step=1`` is the
        plain 1-step batch."""
        n = self.n_step if n_step is None else int(n_step)
        if n <= 1:
            return Batch(
                self.state[idx], self.actions[idx], self.rewards[idx],
                self.next_state[idx], self.done[idx])
        if self.episode_end is None:
            raise ValueError("n-step sampling needs set_n_step(n > 1) "
                             "before the first store")
        idx = torch.as_tensor(idx, dtype=torch.long, device=self.device)
        S = self.max_size
        newest = (self.ptr - 1) % S if self.size else 0
        gamma = torch.tensor(self.gamma, dtype=torch.float32,
                             device=self.device)
        R = torch.zeros(idx.shape, dtype=torch.float32, device=self.device)
        disc = torch.ones_like(R)
        last = idx.clone()
        active = torch.ones(idx.shape, dtype=torch.bool, device=self.device)
        for m in range(n):
            j = (idx + m) % S
            R = torch.where(active, R + disc * self.rewards[j], R)
            last = torch.where(active, j, last)
            stop = ((self.done[j] != 0) | (self.episode_end[j] != 0)
                    | (j == newest))
            active = active & ~stop
            if m + 1 < n:
                disc = torch.where(active, disc * gamma, disc)
        done_eff = 1.0 - disc * (1.0 - self.done[last])
        return Batch(self.state[idx], self.actions[idx], R,
                     self.next_state[last], done_eff)
