"""Batched deterministic evaluation (algo/evaluate.py) on the CPU eager
path: episode quota and ordering, length cap, repeatability, RNG and
normalizer isolation, the training-loop hook, two-rank merging and the
CLI flags."""

import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

from torch_actor_critic_amd import envs
from torch_actor_critic_amd.algo.evaluate import evaluate
from torch_actor_critic_amd.envs.core import Box, Env

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 40


# -- scripted env: everything is a closed form of (seed, n, t) -------------

def _ep_len(seed, n):
    return 3 + (seed + n) % 5


def _reward(seed, n, t):
    # binary fractions: sums are exact in floating point
    return (seed % 7) + 0.25 * n + 0.5 * t


def _ep_return(seed, n, length):
    return sum(_reward(seed, n, t) for t in range(1, length + 1))


class ScriptedEnv(Env):
    """Action-independent env: episode n of an env seeded `seed` lasts
    3 + (seed + n) % 5 steps; obs and reward are functions of (seed, n, t)."""

    def __init__(self):
        self.action_space = Box(-1.0, 1.0, (1,))
        self.observation_space = Box(-np.inf, np.inf, (2,))
        self._seed, self._n, self._t = 0, -1, 0
        self.n_steps = 0

    def seed(self, seed):
        super().seed(seed)
        self._seed, self._n = seed, -1

    def _obs(self):
        return np.array([self._seed + 0.5 * self._n, self._t],
                        dtype=np.float32)

    def reset(self):
        self._n += 1
        self._t = 0
        return self._obs()

    def step(self, action):
        assert np.asarray(action).shape == (1,)
        self._t += 1
        self.n_steps += 1
        done = self._t >= _ep_len(self._seed, self._n)
        return self._obs(), _reward(self._seed, self._n, self._t), done, {}


class StubActor(nn.Module):
    def __init__(self):
        super().__init__()
        self.p = nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, x, deterministic=False, with_logprob=True):
        self.calls.append((tuple(x.shape), deterministic))
        return torch.zeros(x.shape[0], 1), None


def _expected(episodes, K, max_ep_len=10 ** 9):
    """Quota rule: episode j is the (j // K)-th episode of slot j % K,
    whose env is seeded SEED + j % K."""
    rets, lens = [], []
    for j in range(episodes):
        seed, n = SEED + j % K, j // K
        length = min(_ep_len(seed, n), max_ep_len)
        lens.append(length)
        rets.append(_ep_return(seed, n, length))
    return rets, lens


def test_quota_and_episode_order():
    actor = StubActor()
    made = []

    def env_fn():
        made.append(ScriptedEnv())
        return made[-1]

    res = evaluate(actor, env_fn, 7, 100, num_envs=3, seed=SEED)
    rets, lens = _expected(7, 3)
    assert len(res["returns"]) == 7 and len(res["lengths"]) == 7
    assert res["lengths"] == lens          # episode-index order
    assert res["returns"] == rets
    assert res["mean_return"] == pytest.approx(np.mean(rets))
    assert res["std_return"] == pytest.approx(np.std(rets))
    assert res["mean_length"] == pytest.approx(np.mean(lens))
    # exactly K envs, none stepped past its quota (slot 0 plays 3
    # episodes, slots 1 and 2 play 2)
    assert len(made) == 3
    for i, env in enumerate(made):
        assert env.n_steps == sum(lens[i::3])
    # ONE batched deterministic actor call per lockstep step, all K rows
    assert all(c == ((3, 2), True) for c in actor.calls)
    assert len(actor.calls) == max(sum(lens[i::3]) for i in range(3))


@pytest.mark.parametrize("K", [1, 7, 16])
def test_quota_rule_for_other_env_counts(K):
    res = evaluate(StubActor(), ScriptedEnv, 7, 100, num_envs=K, seed=SEED)
    rets, lens = _expected(7, min(K, 7))
    assert Counter(zip(res["returns"], res["lengths"])) == \
        Counter(zip(rets, lens))
    assert res["returns"] == rets and res["lengths"] == lens


def test_length_cap():
    res = evaluate(StubActor(), ScriptedEnv, 7, 4, num_envs=3, seed=SEED)
    rets, lens = _expected(7, 3, max_ep_len=4)
    assert all(n <= 4 for n in res["lengths"])
    assert 3 in res["lengths"] and 4 in res["lengths"]
    assert res["lengths"] == lens and res["returns"] == rets


def _pendulum_actor():
    from networks.linear import Actor
    torch.manual_seed(3)
    return Actor(3, 1, [16, 16], act_limit=2.0)


@pytest.mark.parametrize("deterministic", [True, False])
def test_repeatable_and_rng_isolated(deterministic):
    actor = _pendulum_actor()
    env_fn = lambda: envs.make("Pendulum-v1")  # noqa: E731
    torch.manual_seed(77)
    np.random.seed(77)
    t0, n0 = torch.get_rng_state(), np.random.get_state()
    a = evaluate(actor, env_fn, 5, 25, num_envs=3,
                 deterministic=deterministic, seed=9)
    b = evaluate(actor, env_fn, 5, 25, num_envs=3,
                 deterministic=deterministic, seed=9)
    assert a["returns"] == b["returns"] and a["lengths"] == [25] * 5
    assert len(set(a["returns"])) == 5     # distinct seeded start states
    assert torch.equal(torch.get_rng_state(), t0)
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) \
        and n0[2:] == n1[2:]
    c = evaluate(actor, env_fn, 5, 25, num_envs=3,
                 deterministic=deterministic, seed=10)
    assert c["returns"] != a["returns"]


def test_normalizer_is_read_only():
    from torch_actor_critic_amd.utils.normalizer import (
        WelfordVarianceEstimate)
    norm = WelfordVarianceEstimate()
    g = torch.Generator().manual_seed(1)
    for _ in range(10):
        norm.update(torch.randn(3, generator=g) * 2 + 1)
    count, mean, m2 = norm.count, norm.mean.clone(), norm.m2.clone()
    actor = _pendulum_actor()
    env_fn = lambda: envs.make("Pendulum-v1")  # noqa: E731
    with_norm = evaluate(actor, env_fn, 3, 20, num_envs=2, normalizer=norm)
    assert norm.count == count
    assert torch.equal(norm.mean, mean) and torch.equal(norm.m2, m2)
    # ... and it IS applied: the policy sees different inputs
    without = evaluate(actor, env_fn, 3, 20, num_envs=2)
    assert with_norm["returns"] != without["returns"]


def _train(eval_every, epochs=3, log=None, monkeypatch=None, **kw):
    from buffer.replay_buffer import ReplayBuffer
    from networks.linear import Actor, DoubleCritic
    from sac.algorithm import SAC
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.utils import checkpoint as ckpt

    if log is not None:
        monkeypatch.setattr(
            ckpt, "log_metrics",
            lambda metrics, step=0: log.append((step, dict(metrics))))
    torch.manual_seed(21)
    env = envs.make("Pendulum-v1")
    env.seed(5)
    actor = Actor(3, 1, [16, 16], act_limit=2.0)
    critic = DoubleCritic(3, 1, [16, 16])
    buf = ReplayBuffer(2000, 3, 1)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=epochs, batch_size=16, start_steps=20,
              steps_per_epoch=60, max_ep_len=30, update_after=20,
              update_every=10, save_every=1000, eval_every=eval_every,
              eval_episodes=3, **kw)
    sac.eval_env_fn = lambda: envs.make("Pendulum-v1")
    m = sac.train(0, env, actor, critic, buf, pi_opt, q_opt, render=False,
                  logging=log is not None)
    return m, pi_opt.fp.flat.clone(), q_opt.fp.flat.clone()


def test_training_logs_eval_only_on_eval_epochs(monkeypatch):
    log = []
    m, _, _ = _train(2, log=log, monkeypatch=monkeypatch)
    assert [step for step, _ in log] == [0, 1, 2]
    keys = ("eval_reward", "eval_reward_std", "eval_episode_length")
    for step, metrics in log:
        for k in keys:
            assert (k in metrics) == (step == 1), (step, k)
        assert "reward" in metrics
    ev = log[1][1]
    assert np.isfinite(ev["eval_reward"]) and ev["eval_reward"] < 0
    assert ev["eval_reward_std"] >= 0
    assert ev["eval_episode_length"] == 30.0
    assert not any(k in m for k in keys)   # nothing lingers in `metrics`


def test_eval_off_by_default():
    from sac.algorithm import SAC
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=16, start_steps=20, steps_per_epoch=60,
              max_ep_len=30, update_after=20, update_every=10, save_every=10)
    assert sac.eval_every == 0 and sac.eval_episodes == 10
    assert sac.eval_envs == 8 and sac.eval_env_fn is None


def test_evaluation_does_not_perturb_training():
    m_on, a_on, c_on = _train(1, epochs=2)
    m_off, a_off, c_off = _train(0, epochs=2)
    assert torch.equal(a_on, a_off)
    assert torch.equal(c_on, c_off)
    assert m_on["reward"] == m_off["reward"]
    assert m_on["loss_q"] == m_off["loss_q"]


# -- two ranks ---------------------------------------------------------------

def _worker_eval_train(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from buffer.replay_buffer import ReplayBuffer
    from networks.linear import Actor, DoubleCritic
    from sac.algorithm import SAC
    from torch_actor_critic_amd.algo import evaluate as ev_mod
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel import comm
    comm.init_distributed(backend="gloo")

    seen = []
    real_evaluate = ev_mod.evaluate

    def spy_evaluate(actor, env_fn, episodes, *a, **kw):
        res = real_evaluate(actor, env_fn, episodes, *a, **kw)
        seen.append((episodes, kw["seed"], list(res["returns"])))
        return res
    ev_mod.evaluate = spy_evaluate

    torch.manual_seed(50 + rank)
    env = envs.make("Pendulum-v1")
    env.seed(rank)
    actor = Actor(3, 1, [16, 16], act_limit=2.0)
    critic = DoubleCritic(3, 1, [16, 16])
    buf = ReplayBuffer(2000, 3, 1)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=16, start_steps=20, steps_per_epoch=60,
              max_ep_len=30, update_after=20, update_every=10,
              save_every=100, eval_every=1, eval_episodes=4, eval_envs=2)
    sac.eval_env_fn = lambda: envs.make("Pendulum-v1")
    logged = []
    real_run = sac._run_evaluation

    def spy_run(*a, **kw):
        out = real_run(*a, **kw)
        logged.append(out)
        return out
    sac._run_evaluation = spy_run
    sac.train(0, env, actor, critic, buf, pi_opt, q_opt, render=False,
              logging=False)
    q.put((rank, seen, logged))
    import torch.distributed as dist
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_split_and_merge_evaluation():
    from torch_actor_critic_amd.parallel.launch import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port(29541)
    procs = [ctx.Process(target=_worker_eval_train, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(2):
        rank, seen, logged = q.get(timeout=280)
        out[rank] = (seen, logged)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    all_returns = []
    for rank in (0, 1):
        seen, logged = out[rank]
        assert len(seen) == 1 and len(logged) == 1
        episodes, seed, returns = seen[0]
        assert episodes == 2 and len(returns) == 2
        assert seed == 12345 + 1000 * rank
        all_returns += returns
    assert out[0][1][0] == out[1][1][0]    # same merged metrics everywhere
    assert out[0][1][0]["eval_reward"] == pytest.approx(
        np.mean(all_returns), rel=1e-12)
    assert out[0][1][0]["eval_reward_std"] == pytest.approx(
        np.std(all_returns), rel=1e-12)


# -- CLI -----------------------------------------------------------------------

@pytest.mark.timeout(300)
def test_cli_eval_flags_and_parallel_run_agent(tmp_path):
    env = {**os.environ, "PYTHONPATH": REPO}
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "main.py"), "--environment",
         "Pendulum-v1", "--device", "cpu", "--epochs", "2",
         "--steps-per-epoch", "60", "--eval-every", "1",
         "--eval-episodes", "2", "--eval-envs", "2"],
        cwd=tmp_path, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = os.listdir(tmp_path / "mlruns" / "0")
    assert len(runs) == 1
    run_dir = tmp_path / "mlruns" / "0" / runs[0]
    lines = (run_dir / "metrics" / "eval_reward").read_text().split("\n")
    entries = [ln.split() for ln in lines if ln.strip()]
    assert [int(e[2]) for e in entries] == [0, 1]
    assert all(np.isfinite(float(e[1])) for e in entries)
    assert (run_dir / "params" / "eval_every").read_text() == "1"

    # save_every=10 writes no checkpoint within 2 epochs; give the run the
    # Pendulum-shaped golden actor artifact so run_agent has one to load
    import shutil
    shutil.copytree(os.path.join(REPO, "tests", "fixtures", "golden_mlflow",
                                 "actor"), run_dir / "artifacts" / "actor")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "run_agent.py"), "--run",
         runs[0], "--episodes", "3", "--parallel", "3", "--headless",
         "--device", "cpu"],
        cwd=tmp_path, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "return: mean" in r.stdout and "3 episodes, 3 envs" in r.stdout
