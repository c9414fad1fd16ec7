"""Evaluation throughput (GPU box): env-steps/s of the eager single-env
`run_agent.run_agent` loop vs the batched evaluator (one act_batch launch
per lockstep step) at K in {1, 8, 32} env copies, on synthetic
HalfCheetah-v4 with Actor[256, 256].  Three repeats per configuration."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["TAC_AMD_FORCE_SYNTHETIC"] = "1"

import torch  # noqa: E402

from run_agent import run_agent  # noqa: E402
from torch_actor_critic_amd import envs  # noqa: E402
from torch_actor_critic_amd.algo.act import make_batched_act_path  # noqa: E402
from torch_actor_critic_amd.algo.evaluate import evaluate  # noqa: E402
from torch_actor_critic_amd.models.mlp import Actor  # noqa: E402

ENV = "HalfCheetah-v4"
EP_LEN = 1000      # the synthetic env's episode length
REPEATS = 3

dev = torch.device("cuda:0")
torch.manual_seed(0)
env = envs.make(ENV)
obs_dim = env.observation_space.shape[0]
act_dim = env.action_space.shape[0]
actor = Actor(obs_dim, act_dim, [256, 256], act_limit=1.0).to(dev)
actor.eval()


def eager_loop():
    rets = run_agent(actor, env, 1, deterministic=True, render=False,
                     device=dev)
    return EP_LEN * len(rets)


def batched(K, path):
    def run():
        res = evaluate(actor, lambda: envs.make(ENV), K, EP_LEN,
                       num_envs=K, device=dev, act_path=path)
        return sum(res["lengths"])
    return run


def measure(name, fn):
    fn()           # warm-up
    rates = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = fn()
        torch.cuda.synchronize()
        rates.append(steps / (time.perf_counter() - t0))
    print(f"{name}: " + "  ".join(f"{r:9.0f}" for r in rates)
          + "  env-steps/s", flush=True)
    return rates


results = {"eager_run_agent_K1": measure("eager run_agent (K=1)", eager_loop)}
for K in (1, 8, 32):
    path = make_batched_act_path(actor, obs_dim, act_dim, K, dev)
    assert path.path == "kernel", path.path
    results[f"batched_kernel_K{K}"] = measure(f"batched kernel  (K={K})",
                                              batched(K, path))
print(json.dumps(results))
