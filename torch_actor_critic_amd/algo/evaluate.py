"""Batched policy evaluation.

``evaluate`` rolls out a fixed number of episodes on K env copies stepped
in lockstep, with ONE batched actor call per step for all K slots
(``algo/act.py::BatchedActKernel`` on the GPU for MLP actors, the eager
fallback elsewhere).  The policy is deterministic (``tanh(mu) *
act_limit``) by default — the number an SAC user plots, and what
``run_agent.py`` reports after the fact.

Episode quota is fixed up front: episode ``j`` belongs to slot ``j % K``
and results come back in episode-index order.  ("First ``episodes``
episodes to finish" would over-sample short episodes and make the result
depend on K.)  A slot that has finished its quota is masked: its env is
no longer stepped and its action row is ignored.

The function is side-effect free with respect to training: it builds its
own envs, never updates the normalizer, and leaves the global torch /
numpy RNG state as it found it.
"""

import typing as t

import numpy as np
import torch

from ..envs.visual import MultiObservation
from .act import make_batched_act_path


def _observe(obs, normalizer):
    """Training's observation convention: vector observations go through
    the normalizer (statistics are NOT updated here); MultiObservation
    passes through."""
    if isinstance(obs, MultiObservation):
        return obs
    obs = np.asarray(obs, dtype=np.float32)
    if normalizer is not None:
        obs = normalizer.normalize_state(torch.as_tensor(obs)).numpy()
    return obs


def evaluate(actor, env_fn: t.Callable[[], t.Any], episodes: int,
             max_ep_len: int, *, num_envs: int = 8,
             deterministic: bool = True, device=None, normalizer=None,
             seed: int = 12345, act_path=None,
             render: bool = False) -> dict:
    """Roll out ``episodes`` episodes of ``actor`` on ``min(num_envs,
    episodes)`` lockstep env copies; an episode ends on ``done`` or after
    ``max_ep_len`` steps.  Env ``i`` is seeded with ``seed + i``.

    Returns ``returns`` and ``lengths`` (episode-index order) plus
    ``mean_return``, ``std_return`` and ``mean_length``."""
    episodes = int(episodes)
    max_ep_len = int(max_ep_len)
    if episodes < 1 or max_ep_len < 1 or num_envs < 1:
        raise ValueError("episodes, max_ep_len and num_envs must be >= 1")
    K = min(int(num_envs), episodes)
    device = torch.device(device) if device is not None \
        else next(actor.parameters()).device

    torch_state = torch.get_rng_state()
    numpy_state = np.random.get_state()
    cuda_state = None
    try:
        envs = []
        for i in range(K):
            env = env_fn()
            if hasattr(env, "seed"):
                env.seed(seed + i)
            envs.append(env)

        if act_path is None:
            obs_dim = envs[0].observation_space.shape[0]
            act_dim = envs[0].action_space.shape[0]
            act_path = make_batched_act_path(actor, obs_dim, act_dim, K,
                                             device)
        if (device.type == "cuda" and not deterministic
                and getattr(act_path, "path", "eager") == "eager"):
            # eager stochastic acting may draw from the device generator
            cuda_state = torch.cuda.get_rng_state(device)

        # slot i runs episodes i, i + K, i + 2K, ...
        quota = [len(range(i, episodes, K)) for i in range(K)]
        played = [0] * K
        returns = [0.0] * episodes
        lengths = [0] * episodes
        states = [_observe(env.reset(), normalizer) for env in envs]
        ep_ret = [0.0] * K
        ep_len = [0] * K
        active = [True] * K

        while any(active):
            actions = act_path.act(states, deterministic)
            for i in range(K):
                if not active[i]:
                    continue
                obs, reward, done, _info = envs[i].step(actions[i])
                ep_ret[i] += float(reward)
                ep_len[i] += 1
                if render and i == 0:
                    envs[0].render()
                if done or ep_len[i] >= max_ep_len:
                    j = i + played[i] * K
                    returns[j] = ep_ret[i]
                    lengths[j] = ep_len[i]
                    played[i] += 1
                    ep_ret[i], ep_len[i] = 0.0, 0
                    if played[i] == quota[i]:
                        active[i] = False
                        continue
                    obs = envs[i].reset()
                states[i] = _observe(obs, normalizer)

        for env in envs:
            if hasattr(env, "close"):
                env.close()
    finally:
        torch.set_rng_state(torch_state)
        np.random.set_state(numpy_state)
        if cuda_state is not None:
            torch.cuda.set_rng_state(cuda_state, device)

    return {
        "returns": returns,
        "lengths": lengths,
        "mean_return": float(np.mean(returns)),
        "std_return": float(np.std(returns)),
        "mean_length": float(np.mean(lengths)),
    }
