"""Micro-timing of the visual replay gather (GPU box): the plain
``sample_into`` against the random-shift one, B=64, quantized frames,
(3,64,64) and (3,84,84).

Each variant is timed two ways, in alternating rounds so that drift hits
both alike: eager calls (counter bump + gather launch, host clock around
a synchronised loop) and a captured graph of GRAPH_CALLS calls, which is
how the update engine runs it and takes the launch cost out.

    python scripts/visual_gather_micro.py [--plain-only] [--rounds N]
                                          [--n-step N]

``--plain-only`` is for commits from before the random shift existed.
``--n-step N`` (N > 1) adds the n-step gather, unshifted and shifted, on
the same buffer; episodes end every EPISODE slots, so all but a few
windows are N slots long.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer  # noqa: E402
from torch_actor_critic_amd.envs.visual import MultiObservation  # noqa: E402
from torch_actor_critic_amd.ops import require_extension  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument("--plain-only", action="store_true")
parser.add_argument("--rounds", type=int, default=7)
parser.add_argument("--pad", type=int, default=4)
parser.add_argument("--n-step", type=int, default=1)
args = parser.parse_args()

dev = torch.device("cuda:0")
require_extension()
B, SLOTS, FEAT, ACT = 64, 8192, 17, 6
EAGER_CALLS, GRAPH_CALLS, GRAPH_REPLAYS = 2000, 32, 100
EPISODE = 500


def make_buffer(vis):
    buf = VisualReplayBuffer(SLOTS, ACT, device=dev, seed=1)
    if args.n_step > 1:
        buf.set_n_step(args.n_step, 0.99)
        buf.episode_end[EPISODE - 1::EPISODE] = 1.0
    mo = MultiObservation(torch.zeros(FEAT, device=dev),
                          torch.zeros(*vis, device=dev))
    buf.store(mo, np.zeros(ACT, dtype=np.float32), 0.0, mo, 0.0)
    buf.features.normal_()
    buf.next_features.normal_()
    buf.frames.random_(0, 256)
    buf.next_frames.random_(0, 256)
    buf.size = SLOTS
    buf.ptr = 0
    buf._size_dev.fill_(SLOTS)
    if args.n_step > 1:
        buf._ptr_dev.fill_(0)
    return buf


def select(buf, n_step, pad):
    if not args.plain_only:
        buf.set_random_shift(pad)
    if args.n_step > 1:
        buf.set_n_step(n_step, 0.99)


def eager_us(buf, out):
    for _ in range(50):
        buf.sample_into(out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(EAGER_CALLS):
        buf.sample_into(out)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / EAGER_CALLS * 1e6


def capture(buf, out):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        buf.sample_into(out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            buf.sample_into(out)
    return g


def graph_us(g):
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(GRAPH_REPLAYS):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (GRAPH_REPLAYS * GRAPH_CALLS) * 1e6


def report(name, xs):
    print(f"  {name}: median {statistics.median(xs):.2f} us "
          f"(min {min(xs):.2f}, max {max(xs):.2f}, {len(xs)} rounds)")


for vis in ((3, 64, 64), (3, 84, 84)):
    buf = make_buffer(vis)
    # name -> (n_step, pad)
    variants = {"plain": (1, 0)}
    if not args.plain_only:
        variants[f"shift p={args.pad}"] = (1, args.pad)
    if args.n_step > 1:
        variants[f"n={args.n_step} plain"] = (args.n_step, 0)
        if not args.plain_only:
            variants[f"n={args.n_step} shift p={args.pad}"] = \
                (args.n_step, args.pad)
    outs, graphs = {}, {}
    for name, (n_step, pad) in variants.items():
        select(buf, n_step, pad)
        outs[name] = buf.make_static_batch(B)
        graphs[name] = capture(buf, outs[name])
    times = {(n, k): [] for n in variants for k in ("eager", "graph")}
    for _ in range(args.rounds):
        for name, (n_step, pad) in variants.items():
            select(buf, n_step, pad)
            times[name, "eager"].append(eager_us(buf, outs[name]))
            times[name, "graph"].append(graph_us(graphs[name]))
    n = int(np.prod(vis))
    moved = B * 2 * n * (1 + 4)       # u8 read + f32 write, both frames
    print(f"visual gather B={B} frame={vis} u8: {moved / 1e6:.2f} MB/call")
    for (name, kind), xs in times.items():
        report(f"{name:16s} {kind} per call", xs)
