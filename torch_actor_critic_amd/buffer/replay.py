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
* Optional prioritized replay (extension, default off): after
  ``set_prioritized(alpha, eps)`` the ring carries a fan-out-64 sum tree
  of fp32 priorities in HBM; samplers draw stratified from it and return
  the drawn slots and importance weights, ``update_priorities`` writes
  ``(|td| + eps)^alpha`` back (``draw`` / ``_update_priorities_ref`` are
  the executable definitions).
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
    # prioritized replay only (None otherwise): the ring slots drawn and
    # the importance weights (size * prob)^-beta / max_j of the same
    indices: t.Optional[torch.Tensor] = None
    weights: t.Optional[torch.Tensor] = None


PER_FAN = 64    # sum-tree fan-out: one wave64 loads all children of a node


def per_layout(cap: int) -> t.Tuple[int, t.List[int], t.List[int], int]:
    """(L, nodes per level, offset of each padded level, total floats) of
    the sum tree over ``cap`` leaves: level L is the leaves, level k node i
    sums level k+1 nodes 64i..64i+63, every level is zero-padded to a
    multiple of 64 and the levels are stored root first."""
    L = 1
    while PER_FAN ** L < cap:
        L += 1
    ns = [cap]
    for _ in range(L):
        ns.insert(0, -(-ns[0] // PER_FAN))
    offs, total = [], 0
    for n in ns:
        offs.append(total)
        total += -(-n // PER_FAN) * PER_FAN
    return L, ns, offs, total


def per_node_sum(c: torch.Tensor) -> torch.Tensor:
    """Sum of the 64 children ``c[..., :64]`` in the fixed halving order —
    what a ``__shfl_down`` reduction leaves in lane 0."""
    v = c
    for s in (32, 16, 8, 4, 2, 1):
        v = v[..., :s] + v[..., s:2 * s]
    return v[..., 0]


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
        # prioritized replay (set_prioritized): off by default — nothing
        # below is allocated, copied or launched while it is off
        self.prioritized = False
        self.per_alpha = 0.0
        self.per_eps = 0.0
        self._per_tree: t.Optional[torch.Tensor] = None
        self._per_pad: t.List[torch.Tensor] = []
        self._per_n: t.List[int] = []
        self._per_L = 0
        self._max_priority: t.Optional[torch.Tensor] = None
        self._beta_dev: t.Optional[torch.Tensor] = None

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

    # -- prioritized replay ---------------------------------------------

    def set_prioritized(self, alpha: float = 0.6, eps: float = 1e-6) -> None:
        """Sample proportionally to ``(|td| + eps)^alpha`` from now on.
        Allocates the sum tree (see ``per_layout``), so the buffer must
        still be empty: slots never written have priority 0 and are never
        drawn."""
        if self.size != 0:
            raise ValueError(
                "set_prioritized needs an empty buffer: transitions stored "
                "so far carry no priority")
        if not alpha >= 0.0 or not eps > 0.0:
            raise ValueError(
                f"need alpha >= 0 and eps > 0, got {alpha}, {eps}")
        L, ns, offs, total = per_layout(self.max_size)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._per_tree = torch.zeros(total, **f32)
        self._per_L, self._per_n = L, ns
        self._per_pad = [
            self._per_tree[o:o + -(-n // PER_FAN) * PER_FAN]
            for o, n in zip(offs, ns)]
        self._max_priority = torch.ones(1, **f32)
        self._beta_dev = torch.ones(1, **f32)
        self.per_alpha, self.per_eps = float(alpha), float(eps)
        self.prioritized = True

    def set_beta(self, beta: float) -> None:
        """Importance-weight exponent; a device scalar, so captured
        launches see the annealing."""
        self._beta_dev.fill_(float(beta))

    def per_levels(self) -> t.List[torch.Tensor]:
        """The L+1 unpadded levels of the sum tree, root first (views)."""
        return [p[:n] for p, n in zip(self._per_pad, self._per_n)]

    def _per_refresh(self, leaves: torch.Tensor) -> None:
        """Recompute every ancestor of the given leaves from its children
        (never by a delta: the tree is a function of its leaves)."""
        nodes = leaves
        for k in range(self._per_L - 1, -1, -1):
            nodes = torch.unique(nodes // PER_FAN)
            kids = self._per_pad[k + 1].view(-1, PER_FAN)[nodes]
            self._per_pad[k][nodes] = per_node_sum(kids)

    def _per_store(self, start: int, count: int) -> None:
        """Give the ``count`` slots from ``start`` (mod max_size) the
        current max priority — one launch on the GPU, no host read."""
        ext = self._native_ext()
        if ext is not None:
            ext.per_set_range(self._per_tree, self.max_size, start, count,
                              self._max_priority)
            return
        slots = (start + torch.arange(count, device=self.device)) \
            % self.max_size
        self._per_pad[self._per_L][slots] = self._max_priority
        self._per_refresh(slots)

    def draw(self, u: torch.Tensor) -> t.Tuple[torch.Tensor, torch.Tensor]:
        """(slot, probability) for fp32 targets ``u`` in [0, root) — plain
        torch, the definition the descent kernels are tested against.

        From the root, at every level: load the 64 children c of the
        node, form the inclusive prefix P by Hillis-Steele (the kernel's
        ``__shfl_up`` order), pick the first lane with P > u and c > 0
        (the scan is not monotone in floating point, so without the c > 0
        guard a zero child could win); if u rounded past the end the last
        lane with c > 0; lane 0 in an empty tree.  Then u = max(u -
        (P[pick] - c[pick]), 0) and descend.  prob = leaf / root, or 1 for
        an empty tree."""
        u = torch.as_tensor(u, dtype=torch.float32,
                            device=self.device).clone()
        node = torch.zeros(u.shape, dtype=torch.long, device=self.device)
        lanes = torch.arange(PER_FAN, device=self.device)
        leaf = torch.zeros_like(u)
        for k in range(1, self._per_L + 1):
            c = self._per_pad[k].view(-1, PER_FAN)[node]
            P = c.clone()
            for off in (1, 2, 4, 8, 16, 32):
                P = torch.cat([P[..., :off], P[..., off:] + P[..., :-off]],
                              dim=-1)
            pos = c > 0
            hit = pos & (P > u[..., None])
            first = torch.where(hit, lanes, PER_FAN).amin(-1)
            last = torch.where(pos, lanes, -1).amax(-1)
            pick = torch.where(first < PER_FAN, first, last.clamp(min=0))
            Pp = P.gather(-1, pick[..., None])[..., 0]
            cp = c.gather(-1, pick[..., None])[..., 0]
            u = (u - (Pp - cp)).clamp(min=0)
            node = node * PER_FAN + pick
            leaf = cp
        root = self._per_pad[0][0]
        prob = torch.where(root == 0, torch.ones_like(leaf), leaf / root)
        return node, prob

    def _update_priorities_ref(self, idx: torch.Tensor,
                               td: torch.Tensor) -> None:
        """Plain-torch definition of ``update_priorities`` (and its CPU
        path): p = (td + eps)^alpha in fp32; where a slot occurs more than
        once the highest batch position wins; max_priority grows to the
        largest p; all ancestors are recomputed."""
        idx = torch.as_tensor(idx, dtype=torch.long,
                              device=self.device).reshape(-1)
        td = torch.as_tensor(td, dtype=torch.float32,
                             device=self.device).reshape(-1)
        p = (td + self.per_eps) ** self.per_alpha
        uniq, inv = torch.unique(idx, return_inverse=True)
        pos = torch.arange(idx.numel(), device=self.device)
        win = torch.zeros_like(uniq).scatter_reduce(0, inv, pos, "amax")
        self._per_pad[self._per_L][uniq] = p[win]
        torch.maximum(self._max_priority, p.max().reshape(1),
                      out=self._max_priority)
        self._per_refresh(uniq)

    def update_priorities(self, idx: torch.Tensor, td: torch.Tensor) -> None:
        """New priorities ``(td + eps)^alpha`` for the slots ``idx`` from
        their absolute TD errors ``td``; see ``_update_priorities_ref``."""
        ext = self._native_ext()
        if ext is None:
            self._update_priorities_ref(idx, td)
            return
        idx = torch.as_tensor(idx, dtype=torch.long,
                              device=self.device).reshape(-1).contiguous()
        td = torch.as_tensor(td, dtype=torch.float32,
                             device=self.device).reshape(-1).contiguous()
        ext.per_update(self._per_tree, self.max_size, idx, td,
                       self.per_alpha, self.per_eps, self._max_priority)

    def is_weights(self, prob: torch.Tensor) -> torch.Tensor:
        """Importance weights (size * prob)^-beta over their batch maximum
        (plain torch, no host sync; the fused engine forms the same inside
        its loss kernel)."""
        w = (self._size_dev.to(torch.float32) * prob) ** (-self._beta_dev)
        return w / w.max()

    def _per_targets(self, batch_size: int) -> torch.Tensor:
        """Stratified fp32 targets u_j = (j + u01_j) * (root / B) from the
        host generator (CPU sampling; the kernels draw u01 from Philox)."""
        u01 = torch.as_tensor(
            self._rng.random(batch_size, dtype=np.float32),
            device=self.device)
        j = torch.arange(batch_size, dtype=torch.float32, device=self.device)
        seg = self._per_pad[0][0] / torch.tensor(
            float(batch_size), dtype=torch.float32, device=self.device)
        return (j + u01) * seg

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
        if self.prioritized:
            self._per_store(i, 1)
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
        if self.prioritized and n > 0:
            self._per_store(self.ptr, n)
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

    def _per_args(self):
        """Ring + tree arguments shared by the prioritized samplers; the
        n-step fields are placeholders while n_step == 1."""
        nstep = self.n_step > 1
        return (self.state, self.actions, self.rewards, self.next_state,
                self.done, self.episode_end if nstep else self.done,
                self._size_dev, self._ptr_dev if nstep else self._size_dev,
                self._per_tree, self._philox, self._philox_seed,
                self.n_step, self.gamma)

    def sample(self, batch_size: int) -> Batch:
        ext = self._native_ext()
        if self.prioritized and ext is not None:
            s, a, r, ns, d, idx, prob = ext.replay_sample_p(
                *self._per_args(), batch_size)
            return Batch(s, a, r, ns, d, idx, self.is_weights(prob))
        if self.prioritized:
            idx, prob = self.draw(self._per_targets(batch_size))
            b = self.sample_at(idx)
            return Batch(b.states, b.actions, b.rewards, b.next_states,
                         b.done, idx, self.is_weights(prob))
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
        per = ()
        if self.prioritized:
            per = (torch.zeros(batch_size, dtype=torch.int64,
                               device=self.device),
                   torch.zeros(batch_size, **f32))
        return Batch(torch.zeros(batch_size, self.obs_dim, **f32),
                     torch.zeros(batch_size, self.act_dim, **f32),
                     torch.zeros(batch_size, **f32),
                     torch.zeros(batch_size, self.obs_dim, **f32),
                     torch.zeros(batch_size, **f32), *per)

    def sample_into(self, out: Batch) -> None:
        """Graph-capturable sampling into preallocated batch tensors."""
        ext = self._native_ext()
        if self.prioritized:
            if out.indices is None or out.weights is None:
                raise ValueError("prioritized sample_into needs a batch "
                                 "from make_static_batch after "
                                 "set_prioritized")
            if ext is not None:
                # probabilities land in out.weights, then become weights
                ext.replay_sample_into_p(
                    *self._per_args(), out.states, out.actions, out.rewards,
                    out.next_states, out.done, out.indices, out.weights)
                out.weights.copy_(self.is_weights(out.weights))
                return
            b = self.sample(out.states.shape[0])
            for dst, src in zip(
                    (out.states, out.actions, out.rewards, out.next_states,
                     out.done, out.indices, out.weights),
                    (b.states, b.actions, b.rewards, b.next_states, b.done,
                     b.indices, b.weights)):
                dst.copy_(src)
            return
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
