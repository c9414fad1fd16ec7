"""Fast environment-interaction path.

The env loop is host-side and serial (MuJoCo-like physics can't move to
the GPU — SURVEY.md §7 hard parts), so per-step cost is pure latency:
an eager B=1 actor forward is ~15 Python-dispatched kernel launches plus
a device sync.  This module cuts it to: one pinned H2D copy, ONE
hipGraph replay (the whole actor forward incl. Philox noise), one pinned
D2H copy, one event sync (~25 us/step instead of ~1 ms).

``WindowedStore`` batches the interaction window's transitions in host
pinned buffers and flushes them to the HBM ring ONCE per update window —
semantically identical to per-step stores (the reference samples only at
burst time, sac/algorithm.py:273-278) but 6 launches per window instead
of 6 per step.
"""

import numpy as np
import torch


class ActKernel:
    """Single-kernel acting path: the whole stochastic actor forward for
    one state runs as ONE launch (ops/csrc/fused.hip::act_kernel) — no
    graph replay, no per-layer launches, self-bumped Philox noise."""

    def __init__(self, actor, obs_dim: int, act_dim: int,
                 device: torch.device, philox_seed: int = 0):
        from ..models.mlp import Actor as MlpActor
        from ..ops import require_extension
        if type(actor) is not MlpActor:
            raise TypeError("ActKernel needs the plain MLP Actor")
        if any(l.out_features > 256 for l in actor.layers) or act_dim > 64:
            raise ValueError("shape outside act-kernel limits")
        self.ext = require_extension()
        self.ws = [l.weight for l in actor.layers]
        self.bs = [l.bias for l in actor.layers]
        self.wmu = actor.mu_layer.weight
        self.bmu = actor.mu_layer.bias
        self.wls = actor.log_std_layer.weight
        self.bls = actor.log_std_layer.bias
        self.act_limit = float(actor.act_limit)
        self.lo = float(actor.log_min_std)
        self.hi = float(actor.log_max_std)
        self.seed = philox_seed ^ 0x5ACB
        self.ctr = torch.zeros(1, dtype=torch.int64, device=device)
        self.obs_in = torch.zeros(obs_dim, device=device)
        self.obs_pin = torch.zeros(obs_dim, pin_memory=True)
        self.act_out = torch.zeros(act_dim, device=device)
        self.act_pin = torch.zeros(act_dim, pin_memory=True)
        self.flag_pin = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.flag_np = self.flag_pin.numpy()
        self.ev = torch.cuda.Event()
        import os
        self._pinned_ok = os.environ.get("TAC_AMD_ACT_PINNED", "1") != "0"
        # TAC_AMD_ACT_SYNC: 1 (default) drives the pinned path with one
        # native call per env step (copy in, launch, spin, copy out in
        # C++), 0 keeps the launch and the spin in Python
        self._sync = os.environ.get("TAC_AMD_ACT_SYNC", "1") != "0"
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        # pre-marshalled launch handle (referenced tensors stay alive via
        # self.*): one int-arg pybind call per env step
        self._handle = self.ext.act_prepare(
            self.obs_pin, self.ws, self.bs, self.wmu, self.bmu, self.wls,
            self.bls, self.act_out, self.act_pin, self.flag_pin, self.ctr,
            self.seed, self.act_limit, self.lo, self.hi)

    def act(self, state: np.ndarray) -> np.ndarray:
        # zero-copy I/O on the pinned path: the kernel READS the
        # observation from and WRITES the action + a system-scope
        # completion flag to host-pinned memory; the host spins on the
        # flag — no H2D/D2H copies, no event sync
        if self._pinned_ok and self._sync:
            obs = np.ascontiguousarray(state, dtype=np.float32).reshape(-1)
            out = np.empty(self.act_dim, dtype=np.float32)
            if self.ext.act_sync(self._handle, obs, out):
                return out
            # flag never landed: drain the stream once, then give up on
            # the pinned path for this session (obs_pin holds the state)
            torch.cuda.synchronize()
            if self.flag_np[0] != 0:
                return self.act_pin.numpy().copy()
            self._pinned_ok = False
        else:
            self.obs_pin.copy_(torch.from_numpy(
                np.asarray(state, dtype=np.float32)))
        if self._pinned_ok:
            self.flag_pin[0] = 0
            self.ext.act_fire(self._handle)
            fl = self.flag_np
            for _ in range(2_000_000):
                if fl[0] != 0:
                    return self.act_pin.numpy().copy()
            torch.cuda.synchronize()
            if fl[0] != 0:
                return self.act_pin.numpy().copy()
            self._pinned_ok = False
        self.obs_in.copy_(self.obs_pin, non_blocking=True)
        self.ext.act_step(self.obs_in, self.ws, self.bs, self.wmu,
                          self.bmu, self.wls, self.bls, self.act_out,
                          self.ctr, self.seed, self.act_limit, self.lo,
                          self.hi)
        self.act_pin.copy_(self.act_out, non_blocking=True)
        self.ev.record()
        self.ev.synchronize()
        return self.act_pin.numpy().copy()


def make_act_path(actor, obs_dim, act_dim, device, philox_seed: int = 0):
    """Best available single-state acting path: the one-launch act
    kernel when the actor fits its limits, else the captured act-graph."""
    try:
        return ActKernel(actor, obs_dim, act_dim, device, philox_seed)
    except Exception:  # noqa: BLE001
        return ActGraph(actor, obs_dim, act_dim, device)


class BatchedActKernel:
    """Batched acting path for evaluation: the whole MLP-actor forward for
    up to ``max_rows`` states runs as ONE launch
    (ops/csrc/fused.hip::act_batch_kernel), deterministic or stochastic.

    Evaluation is not the latency-critical serial path, so I/O goes
    through device buffers with pinned staging copies and one event sync.
    The Philox counter is a host-side Python int passed to the kernel by
    value and bumped only by stochastic calls — nothing here shares state
    with the training ``ActKernel``."""

    path = "kernel"
    MAX_LAYERS = 4      # ACT_MAXL
    MAX_OBS = 512       # ACT_MAXW

    def __init__(self, actor, obs_dim: int, act_dim: int, max_rows: int,
                 device: torch.device, philox_seed: int = 0):
        from ..models.mlp import Actor as MlpActor
        from ..ops import require_extension
        if type(actor) is not MlpActor:
            raise TypeError("BatchedActKernel needs the plain MLP Actor")
        if (any(l.out_features > 256 for l in actor.layers)
                or not 1 <= len(actor.layers) <= self.MAX_LAYERS
                or act_dim > 64 or obs_dim > self.MAX_OBS):
            raise ValueError("shape outside act-kernel limits")
        if torch.device(device).type != "cuda":
            raise ValueError("BatchedActKernel needs a cuda device")
        if max_rows < 1:
            raise ValueError("max_rows must be >= 1")
        self.ext = require_extension()
        self.actor = actor
        self.obs_dim = int(obs_dim)
        self.act_dim = int(act_dim)
        self.max_rows = int(max_rows)
        self.act_limit = float(actor.act_limit)
        self.lo = float(actor.log_min_std)
        self.hi = float(actor.log_max_std)
        self.seed = philox_seed ^ 0xE7A1
        self.ctr = 0    # host-side step counter (stochastic calls only)
        self.obs_in = torch.zeros(max_rows, obs_dim, device=device)
        self.obs_pin = torch.zeros(max_rows, obs_dim, pin_memory=True)
        self.act_out = torch.zeros(max_rows, act_dim, device=device)
        self.act_pin = torch.zeros(max_rows, act_dim, pin_memory=True)
        self.ev = torch.cuda.Event()

    def launch(self, n: int, deterministic: bool, ctr: int):
        """One kernel launch on rows [0, n) of obs_in -> act_out with the
        actor's live weights."""
        a = self.actor
        self.ext.act_batch(
            self.obs_in, [l.weight for l in a.layers],
            [l.bias for l in a.layers], a.mu_layer.weight, a.mu_layer.bias,
            a.log_std_layer.weight, a.log_std_layer.bias, self.act_out,
            n, bool(deterministic), int(ctr), self.seed, self.act_limit,
            self.lo, self.hi)

    def act(self, states, deterministic: bool = True) -> np.ndarray:
        s = np.asarray(states, dtype=np.float32).reshape(-1, self.obs_dim)
        n = s.shape[0]
        if not 1 <= n <= self.max_rows:
            raise ValueError(f"{n} states for max_rows={self.max_rows}")
        self.obs_pin[:n].copy_(torch.from_numpy(s))
        self.obs_in[:n].copy_(self.obs_pin[:n], non_blocking=True)
        if not deterministic:
            self.ctr += 1
        self.launch(n, deterministic, self.ctr)
        self.act_pin[:n].copy_(self.act_out[:n], non_blocking=True)
        self.ev.record()
        self.ev.synchronize()
        return self.act_pin[:n].numpy().copy()


class EagerBatchedAct:
    """Fallback with BatchedActKernel's ``act`` signature: vector
    observations are stacked into one actor call; MultiObservation states
    go through the actor one env at a time (the visual models treat
    batched and unbatched inputs differently — DEVIATIONS Q7 — so
    stacking them is unsafe)."""

    path = "eager"

    def __init__(self, actor, device=None):
        self.actor = actor
        self.device = device or next(actor.parameters()).device

    def act(self, states, deterministic: bool = True) -> np.ndarray:
        from ..envs.visual import MultiObservation
        with torch.no_grad():
            if len(states) and isinstance(states[0], MultiObservation):
                out = []
                for st in states:
                    mo = MultiObservation(st.features.to(self.device),
                                          st.frame.to(self.device))
                    a, _ = self.actor(mo, deterministic=deterministic,
                                      with_logprob=False)
                    out.append(a.detach().cpu().numpy().reshape(-1))
                return np.stack(out)
            s = torch.as_tensor(np.asarray(states, dtype=np.float32),
                                device=self.device)
            if s.ndim == 1:
                s = s.unsqueeze(0)
            a, _ = self.actor(s, deterministic=deterministic,
                              with_logprob=False)
        return a.detach().cpu().numpy()


def make_batched_act_path(actor, obs_dim, act_dim, max_rows, device,
                          philox_seed: int = 0):
    """Batched acting path for evaluation: the one-launch kernel on cuda
    when the actor fits its limits, the eager path otherwise (CPU, visual
    actors, oversize MLPs).  ``.path`` is "kernel" or "eager"."""
    device = torch.device(device)
    if device.type == "cuda":
        try:
            return BatchedActKernel(actor, obs_dim, act_dim, max_rows,
                                    device, philox_seed)
        except (TypeError, ValueError):
            pass
    return EagerBatchedAct(actor, device)


class ActGraph:
    """hipGraph-captured single-state stochastic actor forward."""

    def __init__(self, actor, obs_dim: int, act_dim: int,
                 device: torch.device, warmup: int = 3):
        self.device = device
        self.obs_in = torch.zeros(1, obs_dim, device=device)
        self.obs_pin = torch.zeros(obs_dim, pin_memory=True)
        self.act_pin = torch.zeros(1, act_dim, pin_memory=True)
        self.ev = torch.cuda.Event()

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                actor(self.obs_in, deterministic=False, with_logprob=False)
        torch.cuda.current_stream().wait_stream(s)

        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.act_out, _ = actor(self.obs_in, deterministic=False,
                                    with_logprob=False)

    def act(self, state: np.ndarray) -> np.ndarray:
        self.obs_pin.copy_(torch.from_numpy(np.asarray(state,
                                                       dtype=np.float32)))
        self.obs_in.copy_(self.obs_pin.view(1, -1), non_blocking=True)
        self.graph.replay()
        self.act_pin.copy_(self.act_out, non_blocking=True)
        self.ev.record()
        self.ev.synchronize()
        return self.act_pin[0].numpy().copy()


class WindowedStore:
    """Host-side staging of up to `window` transitions, flushed to the
    replay ring in one batched write."""

    def __init__(self, buffer, window: int):
        self.buffer = buffer
        obs_dim, act_dim = buffer.obs_dim, buffer.act_dim
        self.obs = np.zeros((window, obs_dim), dtype=np.float32)
        self.act = np.zeros((window, act_dim), dtype=np.float32)
        self.rew = np.zeros(window, dtype=np.float32)
        self.nobs = np.zeros((window, obs_dim), dtype=np.float32)
        self.done = np.zeros(window, dtype=np.float32)
        # episode-boundary flags, staged only for an n-step buffer
        self.end = np.zeros(window, dtype=np.float32) \
            if getattr(buffer, "n_step", 1) > 1 else None
        self.n = 0
        self.window = window

    def store(self, obs, act, rew, next_obs, done, end=None):
        i = self.n
        self.obs[i] = obs
        self.act[i] = act
        self.rew[i] = rew
        self.nobs[i] = next_obs
        self.done[i] = done
        if self.end is not None:
            self.end[i] = done if end is None else end
        self.n += 1
        if self.n == self.window:
            self.flush()

    def flush(self):
        if self.n == 0:
            return
        n = self.n
        if self.end is not None:
            self.buffer.store_batch(self.obs[:n], self.act[:n], self.rew[:n],
                                    self.nobs[:n], self.done[:n],
                                    self.end[:n])
        else:
            self.buffer.store_batch(self.obs[:n], self.act[:n], self.rew[:n],
                                    self.nobs[:n], self.done[:n])
        self.n = 0


class VisualActGraph:
    """hipGraph-captured single-state stochastic VISUAL actor forward
    (conv trunk + dual-stream tanh-Gaussian head) with pinned-staging
    I/O — replaces ~0.4 ms of eager per-step acting with two H2D
    copies + one graph replay + one D2H copy.  Philox noise is drawn by
    a captured device-counter kernel, so every replay acts with fresh
    noise (same mechanism as the update graphs)."""

    def __init__(self, actor, feat_dim: int, vis_dim, act_dim: int,
                 device: torch.device, warmup: int = 3):
        from ..envs.visual import MultiObservation
        self.device = device
        self.feat_in = torch.zeros(feat_dim, device=device)
        self.frame_in = torch.zeros(*vis_dim, device=device)
        self.feat_pin = torch.zeros(feat_dim, pin_memory=True)
        self.frame_pin = torch.zeros(*vis_dim, pin_memory=True)
        self.act_pin = torch.zeros(act_dim, pin_memory=True)
        self.ev = torch.cuda.Event()
        mo = MultiObservation(self.feat_in, self.frame_in)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                actor(mo, deterministic=False, with_logprob=False)
        torch.cuda.current_stream().wait_stream(s)

        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.act_out, _ = actor(mo, deterministic=False,
                                    with_logprob=False)

    def act(self, state, buffer=None) -> np.ndarray:
        # when the buffer's fused store already staged this observation
        # on device (state is last step's next_obs), read it D2D instead
        # of re-uploading the 84 KB frame through pinned memory
        staged = None
        if buffer is not None:
            last = getattr(buffer, "_last_next_src", None)
            st = getattr(buffer, "_stage", None)
            if (last is not None and st is not None
                    and state.features is last[0]
                    and state.frame is last[1]):
                staged = (st["nf"], st["nF"])
        if staged is not None:
            self.feat_in.copy_(staged[0], non_blocking=True)
            self.frame_in.copy_(staged[1], non_blocking=True)
        else:
            self.feat_pin.copy_(state.features.reshape(-1))
            self.frame_pin.copy_(state.frame)
            self.feat_in.copy_(self.feat_pin, non_blocking=True)
            self.frame_in.copy_(self.frame_pin, non_blocking=True)
        self.graph.replay()
        self.act_pin.copy_(self.act_out.reshape(-1), non_blocking=True)
        self.ev.record()
        self.ev.synchronize()
        return self.act_pin.numpy().copy()
