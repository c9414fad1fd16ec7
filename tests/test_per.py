"""Prioritized replay on the CPU: the sum tree in the ring
(``ReplayBuffer.set_prioritized``), its plain-torch definitions ``draw`` and
``_update_priorities_ref``, the weighted critic loss, the SAC loop and the
CLI.  The helpers here are shared with tests/test_gpu_per.py."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from torch_actor_critic_amd.buffer.replay import (Batch, ReplayBuffer,
                                                  per_layout, per_node_sum)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(48, 1), (200, 2), (5000, 3)]      # (max_size, tree depth L)


def make_per(size, device="cpu", obs_dim=2, act_dim=1, alpha=0.6, eps=1e-6):
    buf = ReplayBuffer(size, obs_dim, act_dim, device=device)
    buf.set_prioritized(alpha, eps)
    return buf


def fill(buf, n, chunk=50, t0=0):
    """n transitions in batches of `chunk`; state[:, 0] is the global step."""
    for lo in range(t0, t0 + n, chunk):
        t = np.arange(lo, min(lo + chunk, t0 + n), dtype=np.float32)
        z = np.zeros((len(t), buf.obs_dim), dtype=np.float32)
        z[:, 0] = t
        buf.store_batch(z, np.zeros((len(t), buf.act_dim)), t, z,
                        np.zeros(len(t)))


def halving_sum(c):
    """The node sum spelled out as in the issue, on a [..., 64] tensor."""
    v = c.clone()
    for s in (32, 16, 8, 4, 2, 1):
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
    return v[..., 0]


def assert_tree_consistent(buf):
    """Every internal node equals the halving-tree sum of its children,
    exactly; padding is zero."""
    levels = buf.per_levels()
    L = len(levels) - 1
    assert levels[L].numel() == buf.max_size and levels[0].numel() == 1
    for k in range(L):
        kids = levels[k + 1]
        n = levels[k].numel()
        assert n == -(-kids.numel() // 64)
        padded = torch.zeros(n * 64, dtype=torch.float32, device=kids.device)
        padded[:kids.numel()] = kids
        want = halving_sum(padded.view(n, 64))
        assert torch.equal(levels[k], want), f"level {k}"
    for pad, n in zip(buf._per_pad, buf._per_n):
        assert pad.numel() % 64 == 0
        assert float(pad[n:].abs().sum()) == 0.0


def set_leaves(buf, p):
    """Install leaf priorities `p` (fp32 [max_size]) and rebuild the tree."""
    leaves = buf.per_levels()[-1]
    leaves.copy_(torch.as_tensor(p, dtype=torch.float32))
    buf._per_refresh(torch.arange(buf.max_size, device=buf.device))
    buf.size = buf.max_size
    buf._size_dev.fill_(buf.size)


# -- layout / tree invariant ----------------------------------------------

def test_layout_and_off_by_default():
    plain = ReplayBuffer(48, 2, 1)
    assert plain.prioritized is False and plain._per_tree is None
    assert plain._max_priority is None and plain._beta_dev is None
    fill(plain, 10)
    assert plain._per_tree is None
    b = plain.sample(4)
    assert b.indices is None and b.weights is None
    # positional construction keeps working
    z = torch.zeros(1)
    assert Batch(z, z, z, z, z).weights is None
    for size, L in SIZES + [(1, 1), (64, 1), (65, 2), (4096, 2), (4097, 3),
                            (262214, 4), (1_000_000, 4)]:
        gotL, ns, offs, total = per_layout(size)
        assert gotL == L == max(1, math.ceil(round(math.log(size, 64), 9)))
        assert ns[0] == 1 and ns[-1] == size and len(ns) == L + 1
        assert all(o % 64 == 0 for o in offs) and total % 64 == 0
    assert per_layout(1_000_000)[3] * 4 < 4.2e6      # about 4 MB
    with pytest.raises(ValueError):
        plain.set_prioritized()                      # not empty


@pytest.mark.parametrize("size,L", SIZES)
def test_tree_invariant_after_stores_and_updates(size, L):
    buf = make_per(size)
    assert len(buf.per_levels()) == L + 1
    assert_tree_consistent(buf)
    assert float(buf.per_levels()[0]) == 0.0
    n = 230 if size == 200 else min(size, 333) - 7
    fill(buf, n, chunk=50)                  # 200-slot ring: a batch wraps
    assert_tree_consistent(buf)
    leaves = buf.per_levels()[-1]
    written = min(n, size)
    assert torch.equal(leaves[:written], torch.ones(written))
    assert float(leaves[written:].abs().sum()) == 0.0    # never written
    g = torch.Generator().manual_seed(size)
    for _ in range(3):
        idx = torch.randint(0, written, (64,), generator=g)
        td = torch.rand(64, generator=g) * 3
        buf.update_priorities(idx, td)
        assert_tree_consistent(buf)
    buf.store(np.zeros(2), np.zeros(1), 0.0, np.zeros(2), 0.0)
    assert_tree_consistent(buf)
    if size == 200:
        assert buf.ptr == 31 and buf.size == 200
    # per_node_sum is the spelled-out halving order
    c = torch.rand(7, 64, generator=g)
    assert torch.equal(per_node_sum(c), halving_sum(c))


def test_store_longer_than_ring():
    buf = make_per(48)
    fill(buf, 130, chunk=130)
    assert_tree_consistent(buf)
    assert torch.equal(buf.per_levels()[-1], torch.ones(48))


# -- draw -------------------------------------------------------------------

def random_priorities(size, seed):
    """fp32 priorities in [0.01, 10], a quarter of the slots zero."""
    g = torch.Generator().manual_seed(seed)
    p = 0.01 + torch.rand(size, generator=g) * 9.99
    p[torch.randperm(size, generator=g)[:size // 4]] = 0.0
    return p


@pytest.mark.parametrize("size,L", SIZES)
def test_draw_against_float64(size, L):
    buf = make_per(size)
    p = random_priorities(size, 7 + size)
    set_leaves(buf, p)
    root = float(buf.per_levels()[0])
    n = 10_000
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n * root
    u = u.to(torch.float32)
    u = u[u < root]
    idx, prob = buf.draw(u)
    assert (p[idx] > 0).all()
    cum = torch.cumsum(p.double(), 0)
    hi, lo = cum[idx], cum[idx] - p.double()[idx]
    # <= 4 levels x (6 scan adds + 6 node adds) x 2^-24 < 48 * 2^-24
    tol = 64 * 2.0 ** -24 * root
    ud = u.double()
    print("worst excess / tol:",
          float(torch.maximum(lo - ud, ud - hi).max() / tol))
    assert (ud >= lo - tol).all() and (ud <= hi + tol).all()
    assert torch.equal(prob, p[idx] / buf.per_levels()[0][0])


@pytest.mark.parametrize("size,L", SIZES)
def test_draw_integer_priorities_is_searchsorted(size, L):
    buf = make_per(size)
    g = torch.Generator().manual_seed(size)
    p = torch.randint(0, 5, (size,), generator=g).float()
    p[torch.randperm(size, generator=g)[:size // 4]] = 0.0
    set_leaves(buf, p)
    cum = torch.cumsum(p.long(), 0)
    root = int(cum[-1])
    assert float(buf.per_levels()[0]) == root < 2 ** 24    # all sums exact
    # every integer target and every half-way point
    u = torch.arange(0, root, 0.5, dtype=torch.float32)
    idx, prob = buf.draw(u)
    want = torch.searchsorted(cum, u.floor().long(), right=True)
    assert torch.equal(idx, want)
    assert torch.equal(prob, p[idx] / root)


def test_draw_fallback_and_empty_tree():
    buf = make_per(200)
    p = random_priorities(200, 3)
    p[150:] = 0.0
    set_leaves(buf, p)
    last = int(torch.nonzero(p).max())
    root = buf.per_levels()[0][0]
    past = torch.nextafter(root, torch.tensor(float("inf")))
    idx, prob = buf.draw(torch.stack([root, past]))
    assert idx.tolist() == [last, last]
    assert torch.equal(prob, (p[last] / root).expand(2))
    empty = make_per(5000)
    idx, prob = empty.draw(torch.tensor([0.0, 1.0]))
    assert idx.tolist() == [0, 0] and prob.tolist() == [1.0, 1.0]
    b = empty.sample(4)
    assert b.indices.tolist() == [0] * 4


def test_cpu_sample_is_stratified_and_weighted():
    buf = make_per(200)
    fill(buf, 200)
    p = 1.0 + (torch.arange(200) % 4).float()
    set_leaves(buf, p)
    buf.set_beta(0.5)
    b = buf.sample(50)                  # segment width 500 / 50 = 10
    cum = torch.cumsum(p.double(), 0)
    seg = 10.0
    lo = cum[b.indices] - p.double()[b.indices]
    j = torch.arange(50, dtype=torch.float64)
    assert (cum[b.indices] > j * seg).all() and (lo < (j + 1) * seg).all()
    assert torch.equal(b.states[:, 0], b.indices.float())
    w = (200 * (p[b.indices] / 500.0)).double() ** -0.5
    np.testing.assert_allclose(b.weights.numpy(), (w / w.max()).numpy(),
                               rtol=1e-6)
    out = buf.make_static_batch(16)
    assert out.indices.dtype == torch.int64 and out.weights.shape == (16,)
    buf.sample_into(out)
    assert torch.equal(out.states[:, 0], out.indices.float())
    assert float(out.weights.max()) == 1.0


# -- update_priorities ----------------------------------------------------------

def test_update_priorities_duplicates_and_max_priority():
    buf = make_per(200, alpha=0.5, eps=0.25)
    fill(buf, 100)
    assert float(buf._max_priority) == 1.0
    idx = torch.tensor([5, 9, 5, 70, 9, 5])
    td = torch.tensor([8.75, 0.0, 3.75, 15.75, 0.75, 0.0])
    buf.update_priorities(idx, td)
    leaves = buf.per_levels()[-1]
    # (td + 0.25)^0.5: the highest batch position wins a duplicated slot
    assert float(leaves[5]) == 0.5          # position 5, not 3.0 or 2.0
    assert float(leaves[9]) == 1.0          # position 4, not 0.5
    assert float(leaves[70]) == 4.0
    assert float(leaves[6]) == 1.0 and float(leaves[100]) == 0.0
    assert float(buf._max_priority) == 4.0  # max over every p of the batch
    assert_tree_consistent(buf)
    assert float(buf.per_levels()[0]) == 100 - 3 + 0.5 + 1.0 + 4.0
    # max_priority never shrinks, and the next store receives it
    buf.update_priorities(torch.tensor([70]), torch.tensor([0.0]))
    assert float(buf._max_priority) == 4.0
    fill(buf, 3, t0=100)
    assert leaves[100:103].tolist() == [4.0] * 3
    buf.store(np.zeros(2), np.zeros(1), 0.0, np.zeros(2), 0.0)
    assert float(leaves[103]) == 4.0 and float(leaves[104]) == 0.0
    assert_tree_consistent(buf)
    # the ref on a twin gives the same tree
    twin = make_per(200, alpha=0.5, eps=0.25)
    fill(twin, 100)
    twin._update_priorities_ref(idx, td)
    assert float(twin.per_levels()[-1][5]) == 0.5


# -- weights --------------------------------------------------------------

def test_weighted_q_loss_and_gradients():
    from torch_actor_critic_amd.ops import functional as Fo
    g = torch.Generator().manual_seed(0)
    B, size, beta, gamma, alpha, scale = 37, 1234, 0.7, 0.97, 0.2, 2.0
    q1, q2, q1t, q2t, logp, rew = (torch.randn(B, generator=g)
                                   for _ in range(6))
    done = (torch.rand(B, generator=g) < 0.3).float()
    prob = torch.rand(B, generator=g) * 0.01 + 1e-4
    buf = make_per(2000)
    buf._size_dev.fill_(size)
    buf.set_beta(beta)
    w = buf.is_weights(prob)
    q1.requires_grad_(True)
    q2.requires_grad_(True)
    loss = Fo.sac_q_loss(q1, q2, q1t, q2t, logp, rew, done, alpha, gamma,
                         scale, weights=w)
    loss.backward()
    d = lambda x: x.detach().double()
    w64 = (size * d(prob)) ** -beta
    w64 = w64 / w64.max()
    backup = scale * d(rew) + gamma * (1 - d(done)) * (
        torch.min(d(q1t), d(q2t)) - alpha * d(logp))
    e1, e2 = d(q1) - backup, d(q2) - backup
    np.testing.assert_allclose(w.numpy(), w64.numpy(), rtol=1e-6)
    np.testing.assert_allclose(float(loss.detach()),
                               float((w64 * (e1 ** 2 + e2 ** 2)).mean()),
                               rtol=1e-6)
    scale_g = float((2 * w64 * e1.abs() / B).max())
    np.testing.assert_allclose(q1.grad.numpy(), (2 * w64 * e1 / B).numpy(),
                               rtol=1e-6, atol=1e-6 * scale_g)
    np.testing.assert_allclose(q2.grad.numpy(), (2 * w64 * e2 / B).numpy(),
                               rtol=1e-6, atol=1e-6 * scale_g)
    # without weights the loss is what it was
    plain = Fo.sac_q_loss(q1, q2, q1t, q2t, logp, rew, done, alpha, gamma,
                          scale)
    np.testing.assert_allclose(float(plain.detach()),
                               float((e1 ** 2 + e2 ** 2).mean()), rtol=1e-6)


# -- training / CLI ------------------------------------------------------------

def test_sac_train_per_cpu():
    from sac.algorithm import SAC
    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam

    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor = Actor(3, 1, [32, 32], act_limit=2.0)
    critic = DoubleCritic(3, 1, [32, 32])
    buf = ReplayBuffer(1000, 3, 1)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=32, start_steps=100, steps_per_epoch=300,
              max_ep_len=100, update_after=100, update_every=50,
              save_every=10, per=True, n_step=3)
    m = sac.train(0, env, actor, critic, buf, FlatAdam(actor),
                  FlatAdam(critic), render=False, logging=False)
    assert np.isfinite(m["loss_q"]) and np.isfinite(m["loss_pi"])
    assert m["loss_q"] != 0.0
    assert buf.prioritized and buf.per_alpha == 0.6 and buf.n_step == 3
    leaves = buf.per_levels()[-1][:300]
    assert (leaves > 0).all() and float(leaves.min()) != float(leaves.max())
    assert float(buf.per_levels()[-1][300:].abs().sum()) == 0.0
    assert float(buf._beta_dev) == 1.0
    assert_tree_consistent(buf)


def test_beta_schedule_and_capable_buffer():
    from sac.algorithm import SAC
    kw = dict(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              batch_size=8, start_steps=0, steps_per_epoch=1, max_ep_len=10,
              update_after=0, update_every=1, save_every=10)

    class NoPer:
        pass

    sac = SAC(epochs=1, per=True, **kw)
    with pytest.raises(ValueError, match="set_prioritized"):
        sac.train(0, None, torch.nn.Linear(1, 1), torch.nn.Linear(1, 1),
                  NoPer(), None, None, render=False, logging=False)
    assert SAC(epochs=1, **kw).per is False

    from torch_actor_critic_amd import envs
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    betas = []
    buf = ReplayBuffer(100, 3, 1)
    real = buf.set_beta
    buf.set_beta = lambda b: (betas.append(b), real(b))[1]
    env = envs.make("Pendulum-v1")
    env.seed(0)
    actor, critic = Actor(3, 1, [8], act_limit=2.0), DoubleCritic(3, 1, [8])
    sac = SAC(epochs=5, per=True, per_beta=0.4, **{**kw, "update_after": 99})
    sac.train(3, env, actor, critic, buf, FlatAdam(actor), FlatAdam(critic),
              render=False, logging=False)
    np.testing.assert_allclose(betas, [0.4, 0.55, 0.7, 0.85, 1.0], rtol=1e-12)


@pytest.mark.timeout(300)
def test_cli_per_logged_and_resumed(tmp_path, monkeypatch):
    env = {**os.environ, "PYTHONPATH": REPO}
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "main.py"), "--environment",
         "Pendulum-v1", "--epochs", "10", "--steps-per-epoch", "20",
         "--batch-size", "8", "--buffer-size", "500", "--device", "cpu",
         "--per", "--per-alpha", "0.7", "--per-beta", "0.5"],
        cwd=tmp_path, timeout=240, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = os.listdir(tmp_path / "mlruns" / "0")
    assert len(runs) == 1
    params = tmp_path / "mlruns" / "0" / runs[0] / "params"
    assert (params / "per").read_text() == "1"
    assert (params / "per_alpha").read_text() == "0.7"
    assert (params / "per_beta").read_text() == "0.5"

    monkeypatch.chdir(tmp_path)
    from torch_actor_critic_amd.utils import checkpoint as ckpt
    ckpt.set_tracking_dir("mlruns")
    import main as train_main
    from sac.algorithm import SAC
    *_, sac_params, _env = train_main.load_session(runs[0],
                                                   torch.device("cpu"))
    assert sac_params["per"] == 1 and sac_params["per_alpha"] == 0.7
    sac = SAC(**sac_params)
    assert sac.per is True and sac.per_alpha == 0.7 and sac.per_beta == 0.5
    # a run logged before the flags existed resumes with uniform replay
    for name in ("per", "per_alpha", "per_beta"):
        (params / name).unlink()
    *_, sac_params, _env = train_main.load_session(runs[0],
                                                   torch.device("cpu"))
    assert "per" not in sac_params and SAC(**sac_params).per is False
