"""Visual replay buffer: dense device arrays, not object arrays.

API-compatible with the reference ``VisualReplayBuffer``
(``buffer/visual_replay_buffer.py:21-66``: ctor (size, act_dim) —
vis/feature dims inferred lazily from the first stored observation, since
the reference stores arbitrary ``MultiObservation`` objects) but stores
features and frames as two dense tensors per side:
``features [N, F]`` fp32 and ``frames [N, C, H, W]`` — frames optionally
uint8-quantized (scale [-1,1] -> u8) to fit 1M 3x64x64 transitions in
~25 GB of the 288 GB HBM3E instead of ~98 GB fp32.

Optional n-step returns (extension, default off), as in ``ReplayBuffer``:
after ``set_n_step(n, gamma)`` every sampler returns the discounted n-step
reward sum, the features and frame of the window's last slot as the next
state and an *effective* done (``sample_at`` is the executable definition).
It composes with the random shift: the state shift applies to the sampled
slot's frame, the next-state shift to the last slot's next frame.
"""

import typing as t
from dataclasses import dataclass

import numpy as np
import torch

from ..envs.visual import MultiObservation


@dataclass(frozen=True)
class VisualBatch:
    """With n-step sampling ``rewards``, ``next_states`` and ``done`` are
    the window's discounted sum, last next state and effective done, as in
    ``buffer.replay.Batch``."""
    states: MultiObservation
    actions: torch.Tensor
    rewards: torch.Tensor
    next_states: MultiObservation
    done: torch.Tensor
    # random-shift augmentation: int32 [B,4] (dy_s, dx_s, dy_n, dx_n) the
    # frames of each row were shifted by; None when augmentation is off
    shifts: t.Optional[torch.Tensor] = None


class VisualReplayBuffer:
    # largest random-shift pad: keeps the 16-bit modulo bias below 0.1%
    MAX_SHIFT_PAD = 32
    MAX_N_STEP = 64   # one wave64 lane per window slot in the gather kernel

    def __init__(self, size: int, act_dim: int,
                 device: t.Union[str, torch.device] = "cpu",
                 seed: int = 0, quantize_frames: bool = True):
        self.max_size = int(size)
        self.act_dim = act_dim
        self.device = torch.device(device)
        self.quantize = quantize_frames
        self.ptr = 0
        self.size = 0
        self._rng = np.random.default_rng(seed)
        self._alloc_done = False
        dev = self.device
        self.actions = torch.zeros((self.max_size, act_dim),
                                   dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(self.max_size, dtype=torch.float32, device=dev)
        self.done = torch.zeros(self.max_size, dtype=torch.float32, device=dev)
        # device-side valid-size mirror (graph-captured sampling)
        self._size_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        # device Philox counter for the fused one-kernel gather
        self._philox = torch.zeros(1, dtype=torch.int64, device=dev)
        self._philox_seed = int(seed)
        # DrQ random-shift augmentation pad (extension; 0 = off)
        self.shift_pad = 0
        # n-step returns (set_n_step): off by default — nothing below is
        # allocated, copied or launched while n_step == 1
        self.n_step = 1
        self.gamma = 1.0
        self.episode_end: t.Optional[torch.Tensor] = None
        self._ptr_dev: t.Optional[torch.Tensor] = None

    def set_n_step(self, n: int, gamma: float) -> None:
        """Sample n-step returns with discount ``gamma`` from now on.
        For n > 1 the ring gains an ``episode_end`` field (1 where an
        episode ended after the transition for ANY reason, truncation
        included) and a device mirror of the write head, so the buffer
        must still be empty; neither depends on the observation shape, so
        this works before the first ``store``."""
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

    def set_random_shift(self, pad: int) -> None:
        """DrQ random-shift augmentation of sampled frames: replicate-pad
        by ``pad`` pixels and crop back at an offset drawn per sample,
        independently for the state and the next-state frame.  ``0``
        turns it off.  Stored frames are never changed."""
        if int(pad) != pad or not 0 <= pad <= self.MAX_SHIFT_PAD:
            raise ValueError(
                f"shift pad must be an integer in 0..{self.MAX_SHIFT_PAD}, "
                f"got {pad!r}")
        self.shift_pad = int(pad)

    @staticmethod
    def shift_frames(frames_f32: torch.Tensor, shifts: torch.Tensor,
                     pad: int) -> torch.Tensor:
        """The definition of the augmentation.  ``frames_f32 [B,C,H,W]``,
        ``shifts [B,2]`` integer ``(dy, dx)`` in ``0..2*pad``:

            out[b,c,y,x] = src[b,c, clamp(y+dy-pad, 0, H-1),
                                    clamp(x+dx-pad, 0, W-1)]

        i.e. replicate-pad by ``pad`` and crop at ``(dy, dx)``;
        ``(pad, pad)`` is the identity."""
        B, C, H, W = frames_f32.shape
        dev = frames_f32.device
        sh = shifts.to(device=dev, dtype=torch.long).reshape(B, 2)
        ys = (torch.arange(H, device=dev)[None] + sh[:, :1] - pad)
        xs = (torch.arange(W, device=dev)[None] + sh[:, 1:] - pad)
        ys = ys.clamp_(0, H - 1)[:, None, :, None]
        xs = xs.clamp_(0, W - 1)[:, None, None, :]
        b = torch.arange(B, device=dev)[:, None, None, None]
        c = torch.arange(C, device=dev)[None, :, None, None]
        return frames_f32[b, c, ys, xs]

    def _alloc(self, obs: MultiObservation):
        feat_dim = int(obs.features.numel())
        vis_dim = tuple(obs.frame.shape)
        dev = self.device
        fdt = torch.uint8 if self.quantize else torch.float32
        self.features = torch.zeros((self.max_size, feat_dim),
                                    dtype=torch.float32, device=dev)
        self.frames = torch.zeros((self.max_size, *vis_dim), dtype=fdt, device=dev)
        self.next_features = torch.zeros_like(self.features)
        self.next_frames = torch.zeros_like(self.frames)
        self.feat_dim = feat_dim
        self.vis_dim = vis_dim
        self._alloc_done = True

    def _enc_frame(self, frame: torch.Tensor) -> torch.Tensor:
        if not self.quantize:
            return frame.to(torch.float32)
        return ((frame.clamp(-1, 1) + 1.0) * 127.5).round().to(torch.uint8)

    def _dec_frames(self, frames: torch.Tensor) -> torch.Tensor:
        if not self.quantize:
            return frames
        return frames.to(torch.float32) / 127.5 - 1.0

    def store(self, obs: MultiObservation, act, rew,
              next_obs: MultiObservation, done, end=None):
        """``end`` (default: ``done``) marks the last transition of an
        episode, whatever ended it; only n-step sampling reads it."""
        if not self._alloc_done:
            self._alloc(obs)
        end = float(done if end is None else end)
        ext = self._native_ext()
        if ext is not None:
            # the n-step store kernel also writes episode_end and _ptr_dev
            self._store_fast(ext, obs, act, rew, next_obs, done, end)
        else:
            i = self.ptr
            self.features[i] = obs.features.reshape(-1).to(self.device)
            self.frames[i] = self._enc_frame(obs.frame.to(self.device))
            self.next_features[i] = \
                next_obs.features.reshape(-1).to(self.device)
            self.next_frames[i] = \
                self._enc_frame(next_obs.frame.to(self.device))
            self.actions[i] = torch.as_tensor(
                np.asarray(act), dtype=torch.float32
            ).reshape(self.act_dim)
            self.rewards[i] = float(rew)
            self.done[i] = float(done)
            if self.episode_end is not None:
                self.episode_end[i] = end
                self._ptr_dev.fill_((i + 1) % self.max_size)
        self.ptr = (self.ptr + 1) % self.max_size
        self.size = min(self.size + 1, self.max_size)
        self._size_dev.fill_(self.size)

    def _store_fast(self, ext, obs, act, rew, next_obs, done, end):
        """GPU store: stage the transition through pinned buffers and run
        ONE fused quantize+write kernel (the eager path costs ~10 aten
        copies plus a CPU-side u8 encode chain per env step)."""
        if not hasattr(self, "_stage"):
            fd, vd, ad = self.feat_dim, self.vis_dim, self.act_dim
            pin = dict(dtype=torch.float32, pin_memory=True)
            dev = dict(dtype=torch.float32, device=self.device)
            self._stage = {
                "pf": torch.empty(fd, **pin), "pF": torch.empty(*vd, **pin),
                "pnf": torch.empty(fd, **pin),
                "pnF": torch.empty(*vd, **pin),
                "pa": torch.empty(ad, **pin),
                "f": torch.empty(fd, **dev), "F": torch.empty(*vd, **dev),
                "nf": torch.empty(fd, **dev),
                "nF": torch.empty(*vd, **dev),
                "a": torch.empty(ad, **dev),
            }
            # guards the previous call's non_blocking H2D copies: the CPU
            # must not rewrite a pinned staging buffer while the copy out
            # of it is still in flight (during random-action warmup
            # nothing else drains the stream)
            self._h2d_done = torch.cuda.Event()
            self._h2d_done.record()
        st = self._stage
        self._h2d_done.synchronize()
        # obs is usually last step's next_obs (state = nstate in the env
        # loop): ping-pong the staged buffers instead of re-staging —
        # saves one pinned CPU copy + one H2D of the 84 KB frame per step.
        # CONTRACT: the skip keys on tensor IDENTITY, so environments must
        # return freshly-allocated observation tensors each step (ours do;
        # envs/core.py documents this).  An env that mutates its
        # observation tensors in place would pass the identity check with
        # stale staged contents.
        last = getattr(self, "_last_next_src", None)
        if (last is not None and obs.features is last[0]
                and obs.frame is last[1]):
            st["f"], st["nf"] = st["nf"], st["f"]
            st["F"], st["nF"] = st["nF"], st["F"]
            st["pf"], st["pnf"] = st["pnf"], st["pf"]
            st["pF"], st["pnF"] = st["pnF"], st["pF"]
        else:
            st["pf"].copy_(obs.features.reshape(-1))
            st["pF"].copy_(obs.frame)
            st["f"].copy_(st["pf"], non_blocking=True)
            st["F"].copy_(st["pF"], non_blocking=True)
        st["pnf"].copy_(next_obs.features.reshape(-1))
        st["pnF"].copy_(next_obs.frame)
        st["pa"].copy_(torch.as_tensor(np.asarray(act),
                                       dtype=torch.float32).reshape(-1))
        for d, p in (("nf", "pnf"), ("nF", "pnF"), ("a", "pa")):
            st[d].copy_(st[p], non_blocking=True)
        self._h2d_done.record()
        self._last_next_src = (next_obs.features, next_obs.frame)
        if self.episode_end is not None:
            ext.visual_store_into_n(st["f"], st["F"], st["nf"], st["nF"],
                                    st["a"], float(rew), float(done), end,
                                    self.features, self.frames,
                                    self.next_features, self.next_frames,
                                    self.actions, self.rewards, self.done,
                                    self.episode_end, self._ptr_dev,
                                    self.ptr)
            return
        ext.visual_store_into(st["f"], st["F"], st["nf"], st["nF"],
                              st["a"], float(rew), float(done),
                              self.features, self.frames,
                              self.next_features, self.next_frames,
                              self.actions, self.rewards, self.done,
                              self.ptr)

    def make_static_batch(self, batch_size: int) -> VisualBatch:
        """Preallocated batch tensors for hipGraph-captured sampling."""
        assert self._alloc_done, "store at least one transition first"
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)

        def mo():
            return MultiObservation(
                torch.zeros(batch_size, self.feat_dim, **f32),
                torch.zeros(batch_size, *self.vis_dim, **f32))

        shifts = None
        if self.shift_pad > 0:
            shifts = torch.zeros(batch_size, 4, dtype=torch.int32, device=dev)
        return VisualBatch(mo(), torch.zeros(batch_size, self.act_dim, **f32),
                           torch.zeros(batch_size, **f32), mo(),
                           torch.zeros(batch_size, **f32), shifts)

    def _native_ext(self):
        if self.device.type != "cuda" or not self._alloc_done:
            return None
        from ..ops import use_native, require_extension
        if use_native(self.features):
            return require_extension()
        return None

    def _nstep_window(self, idx: torch.Tensor, n: int):
        """(last slot, reward sum, effective done) of the n-step windows
        that start at ``idx``; see ``sample_at``."""
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
        return last, R, 1.0 - disc * (1.0 - self.done[last])

    def sample_at(self, idx: torch.Tensor,
                  shifts: t.Optional[torch.Tensor] = None,
                  n_step: t.Optional[int] = None) -> VisualBatch:
        """The batch for given slots and, optionally, given ``[B,4]``
        shifts ``(dy_s, dx_s, dy_n, dx_n)`` at the current ``shift_pad``
        (``None`` = unshifted).  The reference the samplers are tested
        against.

        ``n_step`` (default: the buffer's) > 1 gives n-step returns by the
        window rule of ``ReplayBuffer.sample_at``: from slot i the window
        walks j = i, i+1, ... (mod max_size), adding ``gamma^m *
        rewards[j]`` in fp32 in this order (gamma^m by repeated fp32
        multiply), and closes at the first j with ``done[j]`` or
        ``episode_end[j]`` set, at the newest slot (the walk never crosses
        the write head) or after n slots.  With M slots walked and
        ``last`` the final one: state features, state frame and action
        come from slot i, next features and next frame from slot
        ``last``, reward is the sum and done is ``1 - gamma^(M-1) *
        (1 - done[last])``.  The state shift then applies to the frame of
        slot i, the next-state shift to the next frame of slot ``last``."""
        n = self.n_step if n_step is None else int(n_step)
        idx = torch.as_tensor(idx, dtype=torch.long, device=self.device)
        last, rewards, done = idx, self.rewards[idx], self.done[idx]
        if n > 1:
            if self.episode_end is None:
                raise ValueError("n-step sampling needs set_n_step(n > 1) "
                                 "before the first store")
            last, rewards, done = self._nstep_window(idx, n)
        frames = self._dec_frames(self.frames[idx])
        next_frames = self._dec_frames(self.next_frames[last])
        if shifts is not None:
            shifts = torch.as_tensor(shifts, device=self.device)
            frames = self.shift_frames(frames, shifts[:, 0:2],
                                       self.shift_pad)
            next_frames = self.shift_frames(next_frames, shifts[:, 2:4],
                                            self.shift_pad)
        return VisualBatch(
            MultiObservation(self.features[idx], frames),
            self.actions[idx], rewards,
            MultiObservation(self.next_features[last], next_frames),
            done, shifts)

    def sample_into(self, out: VisualBatch) -> None:
        """Graph-capturable sampling.  On GPU: ONE fused Philox
        gather+dequantize kernel (replaces ~18 aten index/copy/decode
        launches per captured update), which also applies the random
        shift when ``shift_pad > 0`` and walks the n-step window when
        ``n_step > 1``; CPU fallback uses pure tensor ops (torch RNG is
        hipGraph-aware)."""
        pad = self.shift_pad
        if pad > 0 and out.shifts is None:
            raise ValueError("random-shift sample_into needs a batch from "
                             "make_static_batch after set_random_shift()")
        ext = self._native_ext()
        if ext is not None and self.n_step > 1:
            ext.visual_sample_into_n(
                self.features, self.frames, self.next_features,
                self.next_frames, self.actions, self.rewards, self.done,
                self.episode_end, self._size_dev, self._ptr_dev,
                self._philox, self._philox_seed, self.n_step, self.gamma,
                out.states.features, out.states.frame,
                out.next_states.features, out.next_states.frame,
                out.actions, out.rewards, out.done, pad, self.vis_dim[-2],
                self.vis_dim[-1], out.shifts if pad > 0 else None)
            return
        if ext is not None:
            args = (self.features, self.frames, self.next_features,
                    self.next_frames, self.actions, self.rewards, self.done,
                    self._size_dev, self._philox, self._philox_seed,
                    out.states.features, out.states.frame,
                    out.next_states.features, out.next_states.frame,
                    out.actions, out.rewards, out.done)
            if pad > 0:
                ext.visual_sample_into_shift(
                    *args, pad, self.vis_dim[-2], self.vis_dim[-1],
                    out.shifts)
            else:
                ext.visual_sample_into(*args)
            return
        B = out.actions.shape[0]
        u = torch.rand(B, device=self.device)
        size = self._size_dev.clamp(min=1).to(torch.float32)
        idx = (u * size).long().clamp_(max=self.max_size - 1)
        shifts = None
        if pad > 0:
            out.shifts.copy_(torch.randint(0, 2 * pad + 1, (B, 4),
                                           device=self.device))
            shifts = out.shifts
        b = self.sample_at(idx, shifts)
        out.states.features.copy_(b.states.features)
        out.states.frame.copy_(b.states.frame)
        out.next_states.features.copy_(b.next_states.features)
        out.next_states.frame.copy_(b.next_states.frame)
        out.actions.copy_(b.actions)
        out.rewards.copy_(b.rewards)
        out.done.copy_(b.done)

    def sample(self, batch_size: int) -> VisualBatch:
        idx_np = self._rng.choice(self.size, size=batch_size, replace=False)
        shifts = None
        if self.shift_pad > 0:
            shifts = torch.as_tensor(
                self._rng.integers(0, 2 * self.shift_pad + 1,
                                   size=(batch_size, 4)).astype(np.int32))
        return self.sample_at(torch.as_tensor(idx_np, dtype=torch.long),
                              shifts)
