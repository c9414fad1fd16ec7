"""Soft Actor-Critic (fixed entropy temperature, twin Q, polyak targets).

API-compatible with the reference ``sac/algorithm.py``: free functions
``eval_pi_loss`` (:30), ``eval_q_loss`` (:46), ``update_targets`` (:77)
and class ``SAC`` (:85) with ``update_critic`` (:115), ``update_policy``
(:143), ``save_model`` (:164), ``train`` (:182) under the same
signatures and hyperparameter semantics (Appendix A of SURVEY.md).

Deliberate fixes over the reference (each documented in SURVEY.md §8):
 * Q1: the actor gradient all-reduce runs AFTER backward (the reference
   averages stale gradients, algorithm.py:155-156).
 * Q2: the policy loss samples the policy on ``state`` (standard SAC);
   the reference's next_state sampling is available via
   ``SAC(..., reference_pi_loss=True)``.
 * Q3: episode stats are reduced once per epoch (the reference does
   blocking pickled p2p per env step, algorithm.py:262-271).
 * Q11: MultiObservation vs ndarray action dispatch is an explicit type
   check, not try/except TypeError.
 * Q12: optional learned entropy temperature via
   ``SAC(..., learn_alpha=True)`` (default off = reference-faithful).

MI355X-first data path: the replay batch, both networks, the optimizers
and the target live in HBM; one SAC update on GPU is a fixed kernel
sequence with no host sync (losses accumulate in device tensors), so the
whole update can be captured into a hipGraph and replayed
(``algo/graph.py``); gradient reduction is a single flat-bucket RCCL
all-reduce per module per update.
"""

import logging
import typing as t
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn
import tqdm

from ..buffer.replay import Batch
from ..envs.visual import MultiObservation
from ..ops import functional as Fo
from ..optim import FlatAdam
from ..parallel import comm
from ..parallel.flat import FlatParams, flatten_module_like
from ..utils import checkpoint as ckpt
from ..utils.profiling import Throughput, roctx_range

logger = logging.getLogger(__name__)


# ---------------------------------------------------------------------------
# Free-function losses (reference API surface)
# ---------------------------------------------------------------------------

def eval_pi_loss(actor, critic, state, next_state, alpha,
                 use_next_state: bool = False):
    """Policy loss (alpha*logp - min(q1,q2)).mean().

    Standard SAC samples the policy on ``state``; ``use_next_state=True``
    reproduces the reference quirk (algorithm.py:37-38).
    """
    pi_state = next_state if use_next_state else state
    pi, logp_pi = actor(pi_state)
    q1, q2 = critic(state, pi)
    return Fo.sac_pi_loss(q1, q2, logp_pi, alpha)


def eval_q_loss(actor, critic, target_critic, states, actions, rewards,
                next_states, done, alpha, gamma, reward_scale, weights=None,
                return_td=False):
    """Twin-Q Bellman MSE (reference algorithm.py:46-74).  ``weights``
    (prioritized replay) scale each row's squared errors; ``return_td``
    also returns the rows' absolute TD errors (|e1| + |e2|) / 2."""
    with torch.no_grad():
        a2, logp_ac = actor(next_states)
        q1_t, q2_t = target_critic(next_states, a2)
    q1, q2 = critic(states, actions)
    loss = Fo.sac_q_loss(q1, q2, q1_t, q2_t, logp_ac, rewards, done,
                         alpha, gamma, reward_scale, weights=weights)
    if not return_td:
        return loss
    with torch.no_grad():
        backup = reward_scale * rewards + gamma * (1.0 - done) * (
            torch.min(q1_t, q2_t) - alpha * logp_ac)
        td = 0.5 * ((q1 - backup).abs() + (q2 - backup).abs())
    return loss, td


def update_targets(source: nn.Module, target: nn.Module, polyak: float):
    """Per-module polyak average (reference algorithm.py:77-81).  Used on
    the generic path; the flat-buffer path uses ops.polyak_ (one kernel)."""
    with torch.no_grad():
        for src, targ in zip(source.parameters(), target.parameters()):
            targ.data.mul_(polyak).add_(src.data, alpha=1.0 - polyak)


def _freeze(module: nn.Module, flag: bool):
    for p in module.parameters():
        p.requires_grad = not flag


# ---------------------------------------------------------------------------
# SAC
# ---------------------------------------------------------------------------

class SAC:
    def __init__(
        self,
        alpha: float,
        gamma: float,
        polyak: float,
        reward_scale: float,
        epochs: int,
        batch_size: int,
        start_steps: int,
        steps_per_epoch: int,
        max_ep_len: int,
        update_after: int,
        update_every: int,
        save_every: int,
        *,
        reference_pi_loss: bool = False,
        learn_alpha: bool = False,
        target_entropy: t.Optional[float] = None,
        use_graph: bool = True,
        eval_every: int = 0,
        eval_episodes: int = 10,
        eval_envs: int = 8,
        n_step: int = 1,
        per: bool = False,
        per_alpha: float = 0.6,
        per_beta: float = 0.4,
        per_eps: float = 1e-6,
        aug_shift: int = 0,
    ):
        self.alpha = float(alpha)
        self.gamma = float(gamma)
        self.polyak = float(polyak)
        self.reward_scale = float(reward_scale)
        self.epochs = int(epochs)
        self.batch_size = int(batch_size)
        self.start_steps = int(start_steps)
        self.steps_per_epoch = int(steps_per_epoch)
        self.max_ep_len = int(max_ep_len)
        self.update_after = int(update_after)
        self.update_every = int(update_every)
        self.save_every = int(save_every)
        self.reference_pi_loss = reference_pi_loss
        self.use_graph = use_graph
        # n-step returns (extension; 1 = the reference's 1-step backup).
        # The replay buffer forms the n-step reward sum / next state /
        # effective done at sampling time, the losses are unchanged
        self.n_step = int(n_step)
        if self.n_step < 1:
            raise ValueError(f"n_step must be >= 1, got {n_step}")

        # prioritized replay (extension; default off): the buffer samples
        # proportionally to (|td| + per_eps)^per_alpha, the critic loss is
        # importance-weighted with an exponent annealed from per_beta to
        # 1 over the run; the policy loss is not weighted
        self.per = bool(per)
        self.per_alpha = float(per_alpha)
        self.per_beta = float(per_beta)
        self.per_eps = float(per_eps)

        # DrQ random-shift augmentation of sampled frames (extension; 0 =
        # off): the visual replay buffer pads by this many pixels and
        # crops at a random offset, per sample and per frame.  Acting and
        # evaluation never augment
        self.aug_shift = int(aug_shift)
        if self.aug_shift < 0:
            raise ValueError(f"aug_shift must be >= 0, got {aug_shift}")

        # optional learned entropy temperature (default off)
        self.learn_alpha = learn_alpha
        self.target_entropy = target_entropy
        self._log_alpha: t.Optional[torch.Tensor] = None
        self._alpha_opt = None

        # populated by train()
        self._target_flat: t.Optional[torch.Tensor] = None
        self._critic_fp: t.Optional[FlatParams] = None
        self._actor_fp: t.Optional[FlatParams] = None
        self._graph = None
        self._graph_failed = False
        # optional state normalizer (reference ships one as dead code,
        # SURVEY.md Q9; wire-in via main.py --normalize-states).  Both
        # sides of every stored transition (s, s') are normalized with
        # the same statistics snapshot taken at the top of the env step;
        # the update path then consumes normalized states only.
        self.normalizer = None

        # periodic deterministic evaluation (extension; default off =
        # reference-faithful): every `eval_every` epochs, `eval_episodes`
        # episodes on `eval_envs` lockstep env copies built by
        # `eval_env_fn` (set by the caller, like `normalizer`)
        self.eval_every = int(eval_every)
        self.eval_episodes = int(eval_episodes)
        self.eval_envs = int(eval_envs)
        self.eval_env_fn: t.Optional[t.Callable[[], t.Any]] = None
        self._eval_act_path = None

    # -- single-module updates (reference method surface) ---------------

    def _alpha_value(self):
        if self.learn_alpha and self._log_alpha is not None:
            return self._log_alpha.exp()
        return self.alpha

    def update_critic(self, q_opt, actor, critic, target_critic,
                      samples: Batch, buffer=None):
        """``buffer``: with a prioritized batch, where the new priorities
        of its slots are written."""
        q_opt.zero_grad()
        # only a prioritized ReplayBuffer batch carries weights
        weights = getattr(samples, "weights", None)
        weighted = weights is not None
        loss_q = eval_q_loss(
            actor, critic, target_critic, samples.states, samples.actions,
            samples.rewards, samples.next_states, samples.done,
            self._alpha_value(), self.gamma, self.reward_scale,
            weights=weights, return_td=weighted)
        if weighted:
            loss_q, td = loss_q
            if buffer is not None:
                buffer.update_priorities(samples.indices, td)
        loss_q.backward()
        self._allreduce(critic, self._critic_fp)
        q_opt.step()
        return loss_q

    def update_policy(self, pi_opt, actor, critic, samples: Batch):
        _freeze(critic, True)
        pi_opt.zero_grad()
        pi_state = samples.next_states if self.reference_pi_loss \
            else samples.states
        pi, logp_pi = actor(pi_state)
        q1, q2 = critic(samples.states, pi)
        loss_pi = Fo.sac_pi_loss(q1, q2, logp_pi, self._alpha_value())
        loss_pi.backward()
        # Q1 fix: all-reduce AFTER backward (reference: before, :155-156)
        self._allreduce(actor, self._actor_fp)
        pi_opt.step()
        _freeze(critic, False)

        if self.learn_alpha:
            self._update_alpha(logp_pi.detach())
        return loss_pi

    def _update_alpha(self, logp: torch.Tensor):
        self._alpha_opt.zero_grad()
        loss_alpha = -(self._log_alpha
                       * (logp + self.target_entropy)).mean()
        loss_alpha.backward()
        self._alpha_opt.step()

    def _allreduce(self, module: nn.Module, fp: t.Optional[FlatParams]):
        if not comm.is_initialized():
            return
        if fp is not None:
            comm.allreduce_grads(fp.flat_grad)     # ONE bucket
        else:
            for p in module.parameters():
                if p.grad is not None:
                    comm.allreduce_grads(p.grad)

    def _maybe_build_graph(self, actor, critic, target_critic, buffer,
                           pi_opt, q_opt, device):
        """Build the hipGraph-captured update on first use (GPU +
        FlatAdam only).  Falls back to the eager path on any capture
        failure (logged once)."""
        if self._graph is not None:
            return self._graph
        if (self._graph_failed or not self.use_graph
                or device.type != "cuda"
                or self._critic_fp is None or self._actor_fp is None):
            return None
        # 1st choice: the hand-scheduled fused engine (plain MLP models)
        from ..buffer.replay import ReplayBuffer
        from ..models.mlp import Actor as MlpActor
        from ..models.mlp import DoubleCritic as MlpDoubleCritic
        if (type(actor) is MlpActor and type(critic) is MlpDoubleCritic
                and isinstance(buffer, ReplayBuffer)
                and buffer.act_dim <= 64
                # the engine implements the standard (state-sampled)
                # policy loss; the reference's next-state quirk (Q2)
                # runs on the autograd graph below, which honors it
                and not self.reference_pi_loss):
            try:
                from .engine import FusedSACEngine
                self._graph = FusedSACEngine(
                    self, actor, critic, target_critic, buffer, pi_opt,
                    q_opt, self._target_flat, self.batch_size, device,
                    philox_seed=10000 * comm.proc_id())
                logger.info("fused SAC update engine captured (world=%d)",
                            comm.num_procs())
                return self._graph
            except Exception as e:  # noqa: BLE001
                logger.warning("fused engine capture failed (%r); trying "
                               "autograd graph", e)
        if self.learn_alpha:
            self._graph_failed = True
            return None
        if getattr(buffer, "prioritized", False):
            # the autograd-captured update knows neither the weights nor
            # the priority update: training with it would be silently wrong
            logger.info("prioritized replay: no captured update for this "
                        "model/buffer, using eager updates")
            self._graph_failed = True
            return None
        try:
            from .graph import GraphedSACUpdate
            self._graph = GraphedSACUpdate(
                self, actor, critic, target_critic, buffer, pi_opt, q_opt,
                self._target_flat, self.batch_size, device)
            logger.info("SAC update captured into hipGraph "
                        "(world=%d)", comm.num_procs())
        except Exception as e:  # noqa: BLE001
            logger.warning("hipGraph capture failed, using eager updates: "
                           "%r", e)
            self._graph_failed = True
            self._graph = None
        return self._graph

    def update_targets_fast(self, critic):
        if self._target_flat is not None and self._critic_fp is not None:
            Fo.polyak_(self._target_flat, self._critic_fp.flat, self.polyak)
        else:
            update_targets(critic, self._target_critic, self.polyak)

    # -- checkpointing ---------------------------------------------------

    def save_model(self, actor, critic, pi_opt, q_opt, epoch: int):
        """Same artifact layout as the reference (algorithm.py:164-180):
        actor/, critic/ logged models + auxiliaries {pi_opt, q_opt, epoch}."""
        dev = next(actor.parameters()).device
        actor_cpu = deepcopy(actor).cpu()
        critic_cpu = deepcopy(critic).cpu()
        ckpt.log_model(actor_cpu, "actor")
        ckpt.log_model(critic_cpu, "critic")
        aux = {
            "pi_opt": pi_opt.state_dict(),
            "q_opt": q_opt.state_dict(),
            "epoch": epoch,
        }
        # learned entropy temperature (extension; absent for fixed alpha,
        # keeping the reference auxiliaries layout otherwise identical)
        if self.learn_alpha:
            la = None
            if self._graph is not None and hasattr(self._graph, "log_alpha"):
                la = self._graph.log_alpha
            elif self._log_alpha is not None:
                la = self._log_alpha
            if la is not None:
                aux["log_alpha"] = float(la.detach().cpu().reshape(-1)[0])
        ckpt.log_state_dict(aux, "auxiliaries")
        del actor_cpu, critic_cpu
        _ = dev

    # -- environment interaction helpers ---------------------------------

    @staticmethod
    def _state_to_device(state, device):
        if isinstance(state, MultiObservation):
            return MultiObservation(state.features.to(device),
                                    state.frame.to(device))
        return torch.as_tensor(np.asarray(state, dtype=np.float32),
                               device=device)

    def _select_action(self, actor, state, device):
        with torch.no_grad():
            s = self._state_to_device(state, device)
            action, _ = actor(s, deterministic=False, with_logprob=False)
        return action.detach().cpu().numpy()

    def _run_evaluation(self, actor, device):
        """Deterministic evaluation of the live actor on fresh env copies.
        Every rank plays ceil(eval_episodes / world) episodes (seeds offset
        per rank) and the per-episode results are merged with the same
        collective as the training stats, so ranks stay in step.  Touches
        neither the training env, the buffer, the training act path nor
        the normalizer statistics."""
        from .evaluate import evaluate
        world = comm.num_procs()
        n_local = -(-self.eval_episodes // world)
        if (self._eval_act_path is None
                or self._eval_act_path.actor is not actor):
            # built once per actor and reused by every evaluation
            from .act import make_batched_act_path
            probe = self.eval_env_fn()
            self._eval_act_path = make_batched_act_path(
                actor, probe.observation_space.shape[0],
                probe.action_space.shape[0], max(self.eval_envs, 1),
                device, 10000 * comm.proc_id())
            if hasattr(probe, "close"):
                probe.close()
        res = evaluate(
            actor, self.eval_env_fn, n_local, self.max_ep_len,
            num_envs=self.eval_envs, deterministic=True, device=device,
            normalizer=self.normalizer,
            seed=12345 + 1000 * comm.proc_id(),
            act_path=self._eval_act_path)
        rets = comm.gather_stats(res["returns"])
        lens = comm.gather_stats([float(n) for n in res["lengths"]])
        return {"eval_reward": float(np.mean(rets)),
                "eval_reward_std": float(np.std(rets)),
                "eval_episode_length": float(np.mean(lens))}

    # -- main loop --------------------------------------------------------

    def train(self, start_epoch: int, env, actor, critic, buffer,
              pi_opt, q_opt, render: bool = True, logging: bool = True):
        device = next(actor.parameters()).device
        self._target_critic = target_critic = deepcopy(critic)
        _freeze(target_critic, True)

        # flat-buffer fast path when the optimizers are FlatAdam
        self._actor_fp = pi_opt.fp if isinstance(pi_opt, FlatAdam) else None
        self._critic_fp = q_opt.fp if isinstance(q_opt, FlatAdam) else None
        self._target_flat = flatten_module_like(target_critic) \
            if self._critic_fp is not None else None

        if self.learn_alpha and self._log_alpha is None:
            if self.target_entropy is None:
                # -dim(A) heuristic
                act_dim = getattr(actor, "act_dim", None)
                self.target_entropy = -float(act_dim) if act_dim else -1.0
            self._log_alpha = torch.tensor(
                float(np.log(self.alpha)), requires_grad=True, device=device)
            self._alpha_opt = torch.optim.Adam([self._log_alpha], lr=3e-4)

        # initial weight sync: one broadcast per flat buffer (C1)
        if comm.is_initialized():
            if self._actor_fp is not None:
                comm.sync_flat_params(self._actor_fp.flat)
                comm.sync_flat_params(self._critic_fp.flat)
                comm.sync_flat_params(self._target_flat)
            else:
                for m in (actor, critic, target_critic):
                    for p in m.parameters():
                        comm.sync_flat_params(p.data)

        # n-step returns: before the staging store below is built, which
        # stages episode-boundary flags only for an n-step buffer
        if self.n_step > 1:
            if not hasattr(buffer, "set_n_step"):
                raise ValueError(
                    f"n_step={self.n_step} needs a replay buffer with "
                    f"set_n_step(); {type(buffer).__name__} samples 1-step "
                    "transitions only")
            buffer.set_n_step(self.n_step, self.gamma)
        # prioritized replay: likewise before the first store
        if self.per:
            if not hasattr(buffer, "set_prioritized"):
                raise ValueError(
                    "per=True needs a replay buffer with set_prioritized(); "
                    f"{type(buffer).__name__} samples uniformly only")
            if not getattr(buffer, "prioritized", False):
                buffer.set_prioritized(self.per_alpha, self.per_eps)

        # random-shift augmentation: before the update graph is captured,
        # whose static batch carries the shift tensor
        if self.aug_shift > 0:
            if not hasattr(buffer, "set_random_shift"):
                raise ValueError(
                    f"aug_shift={self.aug_shift} needs a replay buffer with "
                    f"set_random_shift(); {type(buffer).__name__} holds no "
                    "frames")
            buffer.set_random_shift(self.aug_shift)

        # per-rank seeding (reference algorithm.py:203-205)
        seed = 10000 * comm.proc_id()
        torch.manual_seed(seed)
        np.random.seed(seed)

        # fast acting path: captured B=1 actor forward + windowed ring
        # stores (GPU, vector-obs envs only; visual envs use eager acting)
        act_graph = None
        wstore = None
        if (device.type == "cuda" and self.use_graph
                and hasattr(buffer, "obs_dim")):
            try:
                from .act import WindowedStore, make_act_path
                act_graph = make_act_path(actor, buffer.obs_dim,
                                          buffer.act_dim, device,
                                          10000 * comm.proc_id())
                wstore = WindowedStore(buffer, self.update_every)
            except Exception as e:  # noqa: BLE001
                logger.warning("act-graph capture failed (%r); using eager "
                               "acting", e)
                act_graph = None
                wstore = None

        state = env.reset()

        rank0 = comm.proc_id() == 0
        pbar = tqdm.trange(start_epoch, start_epoch + self.epochs, ncols=0,
                           initial=start_epoch, disable=not rank0)
        metrics = {"episode_length": 0.0, "reward": 0.0,
                   "loss_q": 0.0, "loss_pi": 0.0,
                   "updates_per_sec": 0.0, "env_steps_per_sec": 0.0}
        thr = Throughput()

        try:
            self._train_epochs(
                pbar, env, actor, critic, target_critic, buffer, pi_opt,
                q_opt, act_graph, wstore, state, device, metrics, thr,
                rank0, render, logging)
        except RuntimeError as err:
            # a hung/failed collective (peer rank died) surfaces here as
            # a timeout RuntimeError: checkpoint what we have and exit
            # nonzero instead of hanging forever (the reference hangs in
            # its blocking p2p, sac/algorithm.py:262-271; gpu_fork's
            # parent monitor then reaps the surviving ranks)
            logger.error("training aborted by a failed collective or "
                         "runtime error: %r — writing emergency "
                         "checkpoint", err)
            if rank0 and logging:
                try:
                    self.save_model(actor, critic, pi_opt, q_opt,
                                    self._last_epoch)
                except Exception:  # noqa: BLE001
                    logger.exception("emergency checkpoint failed")
            raise
        return metrics

    def _train_epochs(self, pbar, env, actor, critic, target_critic,
                      buffer, pi_opt, q_opt, act_graph, wstore, state,
                      device, metrics, thr, rank0, render, logging):
        step = 0
        ep_ret, ep_len = 0.0, 0
        _tried_visual_act = False
        first_epoch = None
        for e in pbar:
            self._last_epoch = e
            if self.per:
                # importance exponent: per_beta -> 1.0 at the last epoch
                first_epoch = e if first_epoch is None else first_epoch
                frac = ((e - first_epoch) / (self.epochs - 1)
                        if self.epochs > 1 else 1.0)
                buffer.set_beta(
                    self.per_beta + (1.0 - self.per_beta) * min(frac, 1.0))
            episode_rewards: t.List[float] = []
            episode_lengths: t.List[float] = []
            # device-side loss accumulators — no per-update host sync
            loss_q_acc = torch.zeros((), device=device)
            loss_pi_acc = torch.zeros((), device=device)
            n_updates = 0

            for k in range(self.steps_per_epoch):
                if (self.normalizer is not None
                        and not isinstance(state, MultiObservation)):
                    st = torch.as_tensor(np.asarray(state, dtype=np.float32))
                    self.normalizer.update(st)
                    state = self.normalizer.normalize_state(st).numpy()
                if step < self.start_steps:
                    action = env.action_space.sample()
                else:
                    if (act_graph is None and not _tried_visual_act
                            and device.type == "cuda" and self.use_graph
                            and isinstance(state, MultiObservation)):
                        # lazily capture the visual act graph — the obs
                        # dims come from the first MultiObservation
                        _tried_visual_act = True
                        try:
                            from .act import VisualActGraph
                            act_graph = VisualActGraph(
                                actor, int(state.features.numel()),
                                tuple(state.frame.shape),
                                int(np.prod(env.action_space.shape)),
                                device)
                        except Exception as e:  # noqa: BLE001
                            logger.warning(
                                "visual act-graph capture failed (%r); "
                                "using eager acting", e)
                    if act_graph is not None:
                        if isinstance(state, MultiObservation):
                            action = act_graph.act(state, buffer=buffer)
                        else:
                            action = act_graph.act(state)
                    else:
                        action = self._select_action(actor, state, device)

                next_state, reward, done, _info = env.step(action)
                thr.tick_env()
                ep_len += 1
                ep_ret += float(reward)
                # n-step windows must not run into the next episode: the
                # boundary is marked wherever the env is reset after this
                # transition — termination, the max_ep_len truncation
                # (stored with done=False) and the reset that closes
                # every epoch
                store_kw = {}
                if self.n_step > 1:
                    store_kw["end"] = float(
                        bool(done) or ep_len == self.max_ep_len
                        or k == self.steps_per_epoch - 1)
                done = False if ep_len == self.max_ep_len else done

                # store next_state normalized with the SAME statistics
                # snapshot as `state` above (no update here — the stats
                # update for next_state happens when it becomes `state`
                # next iteration), so every stored (s, s') pair uses one
                # consistent snapshot
                store_next = next_state
                if (self.normalizer is not None
                        and not isinstance(next_state, MultiObservation)):
                    nst = torch.as_tensor(
                        np.asarray(next_state, dtype=np.float32))
                    store_next = \
                        self.normalizer.normalize_state(nst).numpy()
                if wstore is not None:
                    wstore.store(state, action, float(reward), store_next,
                                 float(done), **store_kw)
                else:
                    buffer.store(state, action, float(reward), store_next,
                                 float(done), **store_kw)
                state = next_state

                if done or ep_len == self.max_ep_len:
                    episode_rewards.append(ep_ret)
                    episode_lengths.append(ep_len)
                    state = env.reset()
                    ep_ret, ep_len = 0.0, 0
                    if render and rank0:
                        env.render()

                step += 1
                if step > self.update_after and step % self.update_every == 0:
                    if wstore is not None:
                        wstore.flush()  # updates must see this window
                    graph = self._maybe_build_graph(
                        actor, critic, target_critic, buffer, pi_opt, q_opt,
                        device)
                    if graph is not None:
                        with roctx_range("sac_update_burst"):
                            for _u in range(self.update_every):
                                graph.step()
                        thr.tick_update(self.update_every)
                        n_updates += self.update_every
                    else:
                        for _u in range(self.update_every):
                            samples = buffer.sample(self.batch_size)
                            loss_q = self.update_critic(
                                q_opt, actor, critic, target_critic, samples,
                                **({"buffer": buffer} if self.per else {}))
                            loss_pi = self.update_policy(
                                pi_opt, actor, critic, samples)
                            self.update_targets_fast(critic)
                            loss_q_acc += loss_q.detach()
                            loss_pi_acc += loss_pi.detach()
                            n_updates += 1

            if wstore is not None:
                wstore.flush()

            # epoch-level stat reduction (Q3 fix; reference did per-step p2p)
            all_rews = comm.gather_stats(episode_rewards)
            all_lens = comm.gather_stats(episode_lengths)
            if n_updates:
                if self._graph is not None:
                    lq, lp = self._graph.read_and_reset_losses(n_updates)
                    metrics["loss_q"] = lq
                    metrics["loss_pi"] = lp
                else:
                    metrics["loss_q"] = float(loss_q_acc.item()) / n_updates
                    metrics["loss_pi"] = float(loss_pi_acc.item()) / n_updates
            if all_rews:
                metrics["reward"] = float(np.mean(all_rews))
                metrics["episode_length"] = float(np.mean(all_lens))
            metrics.update(thr.rates())
            thr.reset()
            if comm.is_initialized():
                cs = comm.collective_stats()
                if cs["allreduce_n"]:
                    metrics["allreduce_ms_per_call"] = (
                        1000.0 * cs["allreduce_s"] / cs["allreduce_n"])

            # periodic deterministic evaluation (all ranks; its metrics
            # are per-epoch extras, never carried over in `metrics`)
            eval_metrics = {}
            if (self.eval_every > 0 and self.eval_env_fn is not None
                    and (e + 1) % self.eval_every == 0):
                eval_metrics = self._run_evaluation(actor, device)
                thr.reset()   # evaluation time is not training throughput

            if rank0 and logging:
                if (e + 1) % self.save_every == 0:
                    self.save_model(actor, critic, pi_opt, q_opt, e)
                ckpt.log_metrics({**metrics, **eval_metrics}, step=e)
            if rank0:
                pbar.set_postfix(step=step, **{
                    k: round(v, 3)
                    for k, v in {**metrics, **eval_metrics}.items()})

            # fresh episode each epoch (reference algorithm.py:305-307)
            state = env.reset()
            ep_ret, ep_len = 0.0, 0

        return metrics
