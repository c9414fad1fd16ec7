"""Flagship benchmark: SAC updates/sec + env steps/sec on HalfCheetah-v4
MLP (BASELINE.json headline metric).

Per bench step: ONE env step (synthetic HalfCheetah-shaped transition,
stored into the HBM replay ring) and ONE SAC update (batch sampled
on-device, critic+actor forward/backward on the gfx950 MFMA kernels,
fused Adam, polyak) — the reference's 1:1 replay ratio
(reference sac/algorithm.py:273-278: 50 updates per 50 env steps; we run
the same 50-step window structure).  On GPU the update burst replays a
captured hipGraph.

Driver contract: `python bench.py --gpus N --steps K --warmup W`; for
N>1 launched under torch.distributed.run, one rank per GPU over RCCL.
Rank 0 prints ONE JSON line; `value` is the whole-job aggregate
updates/sec over all N GPUs.

A plain run sets up, warms up, times K steps and prints the result line;
`--dump-outputs DIR` also saves what the last timed step produced, and
`--full` is where any further measurement belongs (none exist today).
"""

import argparse
import json
import os
import time

import numpy as np
import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=2000,
                   help="timed env-steps (= SAC updates, 1:1)")
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--env", default="HalfCheetah-v4")
    p.add_argument("--hidden", type=int, nargs="+", default=[256, 256])
    p.add_argument("--buffer-size", type=int, default=1_000_000)
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--update-window", type=int, default=50,
                   help="env-steps per update burst (reference: 50)")
    p.add_argument("--mode", choices=["full", "updates", "acting"],
                   default="full",
                   help="isolation: updates-only / acting-only / both")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step produced (parameters, loss accumulators, "
                        "last action) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure (none at present: a plain run already "
                        "times only the flagship workload)")
    return p.parse_args()


# --dump-outputs writes at most this many bytes in all
_DUMP_BUDGET = 64 * 2 ** 20


def dump_outputs(out_dir, arrays):
    """Write each array as out_dir/<name>.npy in float32.  If together
    they exceed the budget, every array is cut down to the same fixed,
    seeded sample of its elements (identical from run to run)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32)
              for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > _DUMP_BUDGET:
        keep = 0.99 * _DUMP_BUDGET / total
        rng = np.random.default_rng(0)
        for k, a in arrays.items():
            a = a.reshape(-1)
            n = max(1, int(a.size * keep))
            idx = np.sort(rng.choice(a.size, size=n, replace=False))
            arrays[k] = a[idx]
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def main():
    args = parse_args()
    # Self-launch N ranks when not already under torchrun/gpu_fork (the
    # reference's mpi_fork self-launches too, sac/mpi.py:10-34).  Without
    # this, `python bench.py --gpus 8` would silently measure ONE GPU.
    from torch_actor_critic_amd.parallel.launch import gpu_fork
    gpu_fork(args.gpus)
    # the bench contract is synthetic transitions (BASELINE.json): never
    # pick up a real gym/MuJoCo env even on machines that have them
    os.environ["TAC_AMD_FORCE_SYNTHETIC"] = "1"
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.parallel import comm
    from torch_actor_critic_amd.parallel.flat import flatten_module_like
    from copy import deepcopy

    rank, world = comm.init_distributed()
    on_gpu = torch.cuda.is_available()
    if on_gpu:
        # modulo: N ranks can share one visible GPU (world>1 RCCL
        # rehearsal on a single leased MI355X)
        device = torch.device(
            "cuda", int(os.environ.get("LOCAL_RANK", "0"))
            % max(torch.cuda.device_count(), 1))
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    dtype = args.dtype if on_gpu else "fp32"
    if on_gpu:
        Fo.set_compute_dtype(dtype)
    Fo.set_philox_seed(1234 + 7919 * rank)

    env = envs.make(args.env)
    env.seed(1000 + rank)
    visual = args.env in ("DeepMindWallRunner-v0", "VisualCheetahRun-v0")
    obs_dim = env.observation_space.shape[0]
    act_dim = env.action_space.shape[0]
    act_limit = float(env.action_space.high.reshape(-1)[0])

    torch.manual_seed(0)  # identical init on all ranks
    if visual:
        from torch_actor_critic_amd.models.visual import (
            VisualActor, VisualDoubleCritic)
        vis_dim = tuple(env.vis_dim)
        actor = VisualActor(obs_dim, act_dim, vis_dim, list(args.hidden),
                            act_limit).to(device)
        critic = VisualDoubleCritic(obs_dim, act_dim, vis_dim,
                                    list(args.hidden)).to(device)
    else:
        actor = Actor(obs_dim, act_dim, list(args.hidden),
                      act_limit=act_limit).to(device)
        critic = DoubleCritic(obs_dim, act_dim, list(args.hidden)).to(device)
    target_critic = deepcopy(critic)
    _freeze(target_critic, True)

    pi_opt = FlatAdam(actor, lr=3e-4)
    q_opt = FlatAdam(critic, lr=3e-4)
    target_flat = flatten_module_like(target_critic)
    if world > 1:
        comm.sync_flat_params(pi_opt.fp.flat)
        comm.sync_flat_params(q_opt.fp.flat)
        comm.sync_flat_params(target_flat)

    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=args.batch_size, start_steps=0,
              steps_per_epoch=1, max_ep_len=1000, update_after=0,
              update_every=args.update_window, save_every=10**9)

    # ---- prefill the HBM replay ring with synthetic transitions -------
    rng = np.random.default_rng(rank)
    if visual:
        from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
        # 100k visual transitions (u8 frames) fit comfortably in HBM
        buf_size = min(args.buffer_size, 100_000) if on_gpu else 2_000
        buffer = VisualReplayBuffer(buf_size, act_dim, device=device,
                                    seed=rank)
        buffer.store(env.reset(), np.zeros(act_dim), 0.0, env.reset(), 0.0)
        prefill = min(buf_size, max(4096, 4 * args.batch_size))
        # fill the dense ring tensors directly (synthetic data)
        buffer.features[:prefill].normal_()
        buffer.next_features[:prefill].normal_()
        buffer.frames[:prefill].random_(0, 255)
        buffer.next_frames[:prefill].random_(0, 255)
        buffer.actions[:prefill].uniform_(-1, 1)
        buffer.rewards[:prefill].normal_()
        buffer.ptr = prefill % buf_size
        buffer.size = prefill
        buffer._size_dev.fill_(prefill)
    else:
        buf_size = args.buffer_size if on_gpu else min(args.buffer_size,
                                                       100_000)
        buffer = ReplayBuffer(buf_size, obs_dim, act_dim, device=device,
                              seed=rank)
        prefill = max(10_000, 4 * args.batch_size)
        chunk = 10_000
        for i0 in range(0, prefill, chunk):
            n = min(chunk, prefill - i0)
            buffer.store_batch(
                rng.standard_normal((n, obs_dim)).astype(np.float32),
                rng.standard_normal((n, act_dim)).astype(np.float32),
                rng.standard_normal(n).astype(np.float32),
                rng.standard_normal((n, obs_dim)).astype(np.float32),
                np.zeros(n, dtype=np.float32))

    # ---- build the update path (hipGraph on GPU) ----------------------
    graph = None
    engine_kind = "eager"
    if on_gpu and not args.no_graph:
        try:
            if visual:
                raise RuntimeError("visual models use the autograd graph")
            from torch_actor_critic_amd.algo.engine import FusedSACEngine
            graph = FusedSACEngine(sac, actor, critic, target_critic,
                                   buffer, pi_opt, q_opt, target_flat,
                                   args.batch_size, device,
                                   philox_seed=1234 + 7919 * rank)
            engine_kind = "fused"
        except Exception as e:  # noqa: BLE001
            print(f"# fused engine failed ({e!r}); autograd graph fallback")
            from torch_actor_critic_amd.algo.graph import GraphedSACUpdate
            graph = GraphedSACUpdate(sac, actor, critic, target_critic,
                                     buffer, pi_opt, q_opt, target_flat,
                                     args.batch_size, device)
            engine_kind = "autograd-graph"

    sac._actor_fp = pi_opt.fp
    sac._critic_fp = q_opt.fp
    sac._target_flat = target_flat
    sac._target_critic = target_critic

    state = env.reset()

    act_graph = None
    vis_act = None
    if on_gpu and not visual:
        from torch_actor_critic_amd.algo.act import (WindowedStore,
                                                     make_act_path)
        act_graph = make_act_path(actor, obs_dim, act_dim, device,
                                  4321 + 7919 * rank)
        wstore = WindowedStore(buffer, args.update_window)
    elif on_gpu and visual:
        from torch_actor_critic_amd.algo.act import VisualActGraph
        vis_act = VisualActGraph(actor, obs_dim, vis_dim, act_dim, device)

    do_act = args.mode in ("full", "acting")
    do_upd = args.mode in ("full", "updates")
    last = {}  # last action / eager losses, for --dump-outputs

    def run_window(n_steps):
        """n_steps env steps then n_steps updates (reference structure)."""
        nonlocal state
        if do_act:
            if act_graph is not None:
                for _ in range(n_steps):
                    a_np = act_graph.act(state)
                    nstate, reward, done, _ = env.step(a_np)
                    wstore.store(state, a_np, float(reward), nstate,
                                 float(done))
                    state = env.reset() if done else nstate
                wstore.flush()
                last["action"] = a_np
            else:
                from torch_actor_critic_amd.envs.visual import (
                    MultiObservation)
                with torch.no_grad():
                    for _ in range(n_steps):
                        if vis_act is not None:
                            a_np = vis_act.act(state, buffer=buffer)
                        else:
                            if isinstance(state, MultiObservation):
                                s = MultiObservation(
                                    state.features.to(device),
                                    state.frame.to(device))
                            else:
                                s = torch.as_tensor(state,
                                                    dtype=torch.float32,
                                                    device=device)
                            a, _ = actor(s, deterministic=False,
                                         with_logprob=False)
                            a_np = a.detach().cpu().numpy()
                        nstate, reward, done, _ = env.step(a_np)
                        buffer.store(state, a_np, float(reward), nstate,
                                     float(done))
                        state = env.reset() if done else nstate
                last["action"] = a_np
        if not do_upd:
            return
        if graph is not None:
            for _ in range(n_steps):
                graph.step()
        else:
            for _ in range(n_steps):
                samples = buffer.sample(args.batch_size)
                loss_q = sac.update_critic(q_opt, actor, critic,
                                           target_critic, samples)
                loss_pi = sac.update_policy(pi_opt, actor, critic, samples)
                sac.update_targets_fast(critic)
            last["loss_q"], last["loss_pi"] = loss_q, loss_pi

    def sync():
        comm.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    win = args.update_window
    # warmup
    done_w = 0
    while done_w < args.warmup:
        n = min(win, args.warmup - done_w)
        run_window(n)
        done_w += n

    sync()
    t0 = time.perf_counter()
    done_s = 0
    while done_s < args.steps:
        n = min(win, args.steps - done_s)
        run_window(n)
        done_s += n
    sync()
    elapsed = time.perf_counter() - t0

    # MAX elapsed over ranks
    el_t = torch.tensor([elapsed], dtype=torch.float64)
    if world > 1:
        import torch.distributed as dist
        el_t = el_t.to(device) if on_gpu else el_t
        dist.all_reduce(el_t, op=dist.ReduceOp.MAX)
    elapsed = float(el_t.item())

    n_gpus = world if on_gpu else args.gpus
    updates_per_sec = world * args.steps / elapsed
    if rank == 0:
        result = {
            "metric": "sac_updates_per_sec",
            "value": updates_per_sec,
            "unit": "updates/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": dtype,
            "data": "synthetic",
            "config": {
                "model": (f"SAC-CNN+MLP{args.hidden}-{args.env}" if visual else f"SAC-MLP{args.hidden}-{args.env}"),
                "global_batch": args.batch_size * world,
                "seq_len": 1,
                "parallelism": f"dp{world}",
                "obs_dim": obs_dim,
                "act_dim": act_dim,
                "replay_buffer": buf_size,
                "env_steps_per_sec": updates_per_sec,
                "update_window": win,
                "graph": graph is not None,
                "engine": engine_kind,
                "mode": args.mode,
            },
        }
        if args.dump_outputs:
            def host(x):
                return x.detach().float().cpu().numpy()
            outs = {"actor_params": host(pi_opt.fp.flat),
                    "critic_params": host(q_opt.fp.flat),
                    "target_critic_params": host(target_flat)}
            if "action" in last:
                outs["last_action"] = np.asarray(last["action"])
            if do_upd and graph is not None:
                # summed over every update since the engine was built
                outs["loss_q_acc"] = host(graph.loss_q_acc)
                outs["loss_pi_acc"] = host(graph.loss_pi_acc)
            elif "loss_q" in last:
                outs["loss_q"] = host(last["loss_q"])
                outs["loss_pi"] = host(last["loss_pi"])
            dump_outputs(args.dump_outputs, outs)
        print(json.dumps(result))

    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
