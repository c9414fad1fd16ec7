"""Batched act kernel (ops/csrc/fused.hip::act_batch_kernel) and the
evaluation path built on it: deterministic parity against a CPU fp32
forward, tail-row safety, the host-counter Philox stream, the evaluator
and the training-loop hook on the kernel path."""

import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77.0


@pytest.fixture(autouse=True)
def _fp32_mode():
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("fp32")
    yield
    Fo.set_compute_dtype("fp32")


def _actor(O, A, hid, act_limit=1.5, seed=0):
    from torch_actor_critic_amd.models.mlp import Actor
    torch.manual_seed(seed)
    return Actor(O, A, hid, act_limit=act_limit).to(DEV)


def _kernel(actor, O, A, max_rows, seed=0):
    from torch_actor_critic_amd.algo.act import BatchedActKernel
    return BatchedActKernel(actor, O, A, max_rows, torch.device(DEV), seed)


def _cpu_reference(actor, x: np.ndarray) -> np.ndarray:
    ref = copy.deepcopy(actor).cpu()
    with torch.no_grad():
        a, _ = ref(torch.from_numpy(x), deterministic=True,
                   with_logprob=False)
    return a.numpy()


# N: below one tile / one full tile / across a tile boundary / several
# tiles with a ragged tail.  O: K < 4 / scalar tail of the unroll-by-4
# loop / Humanoid.  Hidden: one layer / non-uniform, below one wavefront /
# the default.  A: 1 / 6 / 17.
GRID = [
    (1, 3, [64], 1),
    (3, 11, [32, 48, 16], 6),
    (8, 376, [256, 256], 17),
    (9, 11, [256, 256], 6),
    (33, 3, [32, 48, 16], 17),
    (33, 376, [64], 1),
]


@pytest.mark.parametrize("N,O,hid,A", GRID)
def test_deterministic_parity(N, O, hid, A):
    actor = _actor(O, A, hid, seed=N + O)
    x = np.random.default_rng(O * 100 + N).standard_normal(
        (N, O)).astype(np.float32)
    k = _kernel(actor, O, A, max_rows=N)
    got = k.act(x, deterministic=True)
    assert got.shape == (N, A) and got.dtype == np.float32
    np.testing.assert_allclose(got, _cpu_reference(actor, x), atol=1e-4,
                               rtol=0)
    assert k.ctr == 0          # deterministic calls never touch the counter


def test_deterministic_parity_strided_rows():
    """x rows with ldx > O (a column slice of a wider buffer)."""
    from torch_actor_critic_amd.ops import require_extension
    ext = require_extension()
    N, O, LDX, A = 9, 11, 16, 6
    actor = _actor(O, A, [256, 256], seed=4)
    x = np.random.default_rng(8).standard_normal((N, O)).astype(np.float32)
    wide = torch.full((N, LDX), float("nan"), device=DEV)
    wide[:, :O] = torch.from_numpy(x).to(DEV)
    view = wide[:, :O]
    assert view.stride(0) == LDX
    out = torch.full((N, A), SENTINEL, device=DEV)
    ext.act_batch(view, [l.weight for l in actor.layers],
                  [l.bias for l in actor.layers], actor.mu_layer.weight,
                  actor.mu_layer.bias, actor.log_std_layer.weight,
                  actor.log_std_layer.bias, out, N, True, 0, 0,
                  float(actor.act_limit), -20.0, 2.0)
    np.testing.assert_allclose(out.cpu().numpy(), _cpu_reference(actor, x),
                               atol=1e-4, rtol=0)


@pytest.mark.parametrize("deterministic", [True, False])
def test_tail_rows_are_not_written(deterministic):
    O, A = 11, 6
    actor = _actor(O, A, [64], seed=2)
    k = _kernel(actor, O, A, max_rows=16)
    k.act_out.fill_(SENTINEL)
    x = np.random.default_rng(1).standard_normal((9, O)).astype(np.float32)
    got = k.act(x, deterministic=deterministic)
    out = k.act_out.cpu().numpy()
    assert (out[9:] == SENTINEL).all()
    assert (out[:9] != SENTINEL).all()
    np.testing.assert_array_equal(out[:9], got)


def test_limits_raise():
    from torch_actor_critic_amd.algo.act import (BatchedActKernel,
                                                 make_batched_act_path)
    dev = torch.device(DEV)
    wide = _actor(5, 2, [512])
    with pytest.raises(ValueError):
        BatchedActKernel(wide, 5, 2, 8, dev)
    with pytest.raises(ValueError):
        BatchedActKernel(_actor(5, 65, [64]), 5, 65, 8, dev)
    with pytest.raises(ValueError):
        BatchedActKernel(_actor(5, 2, [8] * 5), 5, 2, 8, dev)
    k = _kernel(_actor(5, 2, [64]), 5, 2, max_rows=4)
    with pytest.raises(ValueError):
        k.act(np.zeros((5, 5), dtype=np.float32))
    assert make_batched_act_path(wide, 5, 2, 8, dev).path == "eager"
    assert make_batched_act_path(_actor(5, 2, [64]), 5, 2, 8,
                                 dev).path == "kernel"


def test_stochastic_stream():
    O, A, N = 11, 6, 9
    actor = _actor(O, A, [64, 64], seed=6)
    k = _kernel(actor, O, A, max_rows=N, seed=123)
    state = np.random.default_rng(2).standard_normal(O).astype(np.float32)
    x = np.tile(state, (N, 1))     # identical states in every row
    k.obs_in.copy_(torch.from_numpy(x).to(DEV))

    def fire(ctr, kern=k):
        kern.launch(N, False, ctr)
        return kern.act_out.cpu().numpy().copy()

    a5 = fire(5)
    np.testing.assert_array_equal(a5, fire(5))   # same (seed, counter)
    assert (a5 != fire(6)).all()
    k2 = _kernel(actor, O, A, max_rows=N, seed=124)
    k2.obs_in.copy_(k.obs_in)
    assert (a5 != fire(5, k2)).all()
    # identical states, different rows -> different actions
    for i in range(N):
        for j in range(i + 1, N):
            assert (a5[i] != a5[j]).all(), (i, j)

    # consecutive stochastic calls differ and bump the host counter;
    # deterministic calls do neither
    assert k.ctr == 0
    s1 = k.act(x, deterministic=False)
    s2 = k.act(x, deterministic=False)
    assert k.ctr == 2 and (s1 != s2).all()
    d1 = k.act(x, deterministic=True)
    d2 = k.act(x, deterministic=True)
    assert k.ctr == 2
    np.testing.assert_array_equal(d1, d2)
    np.testing.assert_array_equal(s1, fire(1))


def test_stochastic_noise_statistics():
    O, A, N, CALLS, LIM = 5, 8, 64, 32, 2.0
    actor = _actor(O, A, [32], act_limit=LIM, seed=9)
    with torch.no_grad():
        actor.mu_layer.weight.zero_()
        actor.log_std_layer.weight.zero_()
        actor.mu_layer.bias.fill_(0.3)
        actor.log_std_layer.bias.fill_(-1.0)
    k = _kernel(actor, O, A, max_rows=N, seed=31)
    x = np.random.default_rng(3).standard_normal((N, O)).astype(np.float32)
    acts = np.stack([k.act(x, deterministic=False) for _ in range(CALLS)])
    assert (np.abs(acts) < LIM).all()
    eps = (np.arctanh(acts.astype(np.float64) / LIM) - 0.3) * math.e
    n = eps.size
    assert n == 16384
    mean, std = eps.mean(), eps.std()
    print(f"eps mean {mean:+.5f} std {std:.5f}")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(std - 1) < 5 / math.sqrt(2 * n)
    # a distinct draw per (call, row, action index)
    assert np.unique(np.round(eps, 6)).size > 0.99 * n


class _ScriptedEnv:
    """Action-independent env: obs is a function of (seed, episode, t);
    records the actions it is given."""

    O, A = 5, 3

    def __init__(self):
        from torch_actor_critic_amd.envs.core import Box
        self.action_space = Box(-1.0, 1.0, (self.A,))
        self.observation_space = Box(-np.inf, np.inf, (self.O,))
        self._seed, self._n, self._t = 0, -1, 0
        self.actions = []

    def seed(self, seed):
        self._seed, self._n = seed, -1

    def _obs(self):
        return np.sin(np.arange(self.O) * (self._seed % 13 + 1)
                      + 0.7 * self._t + self._n).astype(np.float32)

    def reset(self):
        self._n += 1
        self._t = 0
        return self._obs()

    def step(self, action):
        self.actions.append(np.array(action, dtype=np.float32))
        self._t += 1
        done = self._t >= 3 + (self._seed + self._n) % 4
        return self._obs(), float(self._t), done, {}

    def close(self):
        pass


def test_evaluate_on_kernel_path_matches_eager_cpu():
    from torch_actor_critic_amd.algo.act import make_batched_act_path
    from torch_actor_critic_amd.algo.evaluate import evaluate
    O, A = _ScriptedEnv.O, _ScriptedEnv.A
    actor = _actor(O, A, [64, 64], act_limit=1.0, seed=12)

    def run(act, device, act_path=None):
        made = []

        def env_fn():
            made.append(_ScriptedEnv())
            return made[-1]
        res = evaluate(act, env_fn, 5, 5, num_envs=3, device=device,
                       seed=7, act_path=act_path)
        return res, [np.stack(e.actions) for e in made]

    path = make_batched_act_path(actor, O, A, 3, torch.device(DEV))
    assert path.path == "kernel"
    res_k, acts_k = run(actor, torch.device(DEV), path)
    cpu = copy.deepcopy(actor).cpu()
    res_e, acts_e = run(cpu, torch.device("cpu"))
    assert res_k["lengths"] == res_e["lengths"]
    assert res_k["returns"] == res_e["returns"]
    assert len(acts_k) == len(acts_e) == 3
    for ak, ae in zip(acts_k, acts_e):
        assert ak.shape == ae.shape and ak.shape[0] > 0
        np.testing.assert_allclose(ak, ae, atol=1e-4, rtol=0)
    assert path.ctr == 0


def test_training_with_evaluation_on_kernel_path(monkeypatch):
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.algo import act as act_mod
    from torch_actor_critic_amd.algo.sac import SAC
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.utils import checkpoint as ckpt

    log, train_paths = [], []
    monkeypatch.setattr(
        ckpt, "log_metrics",
        lambda metrics, step=0: log.append((step, dict(metrics))))
    real_make = act_mod.make_act_path

    def spy_make(*a, **kw):
        train_paths.append(real_make(*a, **kw))
        return train_paths[-1]
    monkeypatch.setattr(act_mod, "make_act_path", spy_make)

    torch.manual_seed(0)
    np.random.seed(0)
    Fo.set_philox_seed(0)
    device = torch.device(DEV)
    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor = Actor(3, 1, [64, 64], act_limit=2.0).to(device)
    critic = DoubleCritic(3, 1, [64, 64]).to(device)
    buf = ReplayBuffer(2000, 3, 1, device=device)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    EPOCHS, STEPS = 2, 100
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=EPOCHS, batch_size=64, start_steps=0,
              steps_per_epoch=STEPS, max_ep_len=20, update_after=60,
              update_every=50, save_every=1000, eval_every=1,
              eval_episodes=2, eval_envs=2)
    sac.eval_env_fn = lambda: envs.make("Pendulum-v1")
    sac.train(0, env, actor, critic, buf, pi_opt, q_opt, render=False,
              logging=True)

    assert [s for s, _ in log] == [0, 1]
    for _, m in log:
        for key in ("eval_reward", "eval_reward_std",
                    "eval_episode_length"):
            assert np.isfinite(m[key]), key
        assert m["eval_episode_length"] == 20.0
    assert sac._eval_act_path.path == "kernel"
    assert sac._eval_act_path.ctr == 0
    # evaluation did not advance the training noise stream: the training
    # act kernel's counter is exactly the number of training policy acts
    assert len(train_paths) == 1
    assert isinstance(train_paths[0], act_mod.ActKernel)
    assert int(train_paths[0].ctr.item()) == EPOCHS * STEPS
