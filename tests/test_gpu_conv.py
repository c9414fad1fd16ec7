"""GPU parity tests: implicit-GEMM conv kernels vs plain PyTorch fp32
references, and the visual model path end-to-end on GPU."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


@pytest.fixture(autouse=True)
def _fp32_mode():
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("fp32")
    yield
    Fo.set_compute_dtype("fp32")


# the reference CNN's layer shapes at 64px and 84px inputs
SHAPES = [
    # B, IC, IH, OC, KH, S
    (8, 3, 64, 32, 8, 4),
    (8, 32, 15, 64, 4, 2),
    (8, 64, 6, 64, 3, 1),
    (4, 3, 84, 32, 8, 4),
    (2, 32, 20, 64, 4, 2),
    (2, 64, 9, 64, 3, 1),
]


@pytest.mark.parametrize("B,IC,IH,OC,KH,S", SHAPES)
def test_conv_fwd_parity(ext, B, IC, IH, OC, KH, S):
    torch.manual_seed(0)
    x = torch.randn(B, IC, IH, IH)
    w = torch.randn(OC, IC, KH, KH) / KH
    b = torch.randn(OC)
    ref = F.conv2d(x, w, b, stride=S)
    out = ext.conv2d_fwd(x.to(DEV), w.to(DEV), b.to(DEV), S, False).cpu()
    assert out.shape == ref.shape
    assert torch.allclose(out, ref, atol=1e-3, rtol=1e-4), \
        (out - ref).abs().max()


@pytest.mark.parametrize("B,IC,IH,OC,KH,S", SHAPES[:3])
def test_conv_bwd_parity(ext, B, IC, IH, OC, KH, S):
    torch.manual_seed(1)
    x = torch.randn(B, IC, IH, IH, requires_grad=True)
    w = (torch.randn(OC, IC, KH, KH) / KH).requires_grad_(True)
    b = torch.randn(OC, requires_grad=True)
    y = F.conv2d(x, w, b, stride=S)
    dy = torch.randn_like(y)
    y.backward(dy)

    wt = w.detach().permute(1, 0, 2, 3).reshape(
        IC, OC * KH * KH).contiguous()
    dx = ext.conv2d_dgrad(dy.to(DEV), None, wt.to(DEV),
                          x.detach().to(DEV), w.detach().to(DEV), S)
    dw, db = ext.conv2d_wgrad(dy.to(DEV), None, x.detach().to(DEV),
                              w.detach().to(DEV), S)
    assert torch.allclose(dx.cpu(), x.grad, atol=1e-3, rtol=1e-4), \
        (dx.cpu() - x.grad).abs().max()
    assert torch.allclose(dw.cpu().view_as(w), w.grad, atol=1e-3,
                          rtol=1e-4), (dw.cpu().view_as(w) - w.grad).abs().max()
    assert torch.allclose(db.cpu(), b.grad, atol=1e-3, rtol=1e-4)


def test_conv_autograd_function():
    from torch_actor_critic_amd.ops import functional as Fo
    torch.manual_seed(2)
    x = torch.randn(4, 3, 32, 32)
    w = torch.randn(16, 3, 8, 8) / 8
    b = torch.randn(16)

    x1 = x.clone().requires_grad_(True)
    w1 = w.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    y1 = F.conv2d(x1, w1, b1, stride=4)
    y1.square().mean().backward()

    x2 = x.to(DEV).requires_grad_(True)
    w2 = w.to(DEV).requires_grad_(True)
    b2 = b.to(DEV).requires_grad_(True)
    y2 = Fo.conv2d(x2, w2, b2, 4)
    y2.square().mean().backward()

    assert torch.allclose(y2.cpu(), y1, atol=1e-4)
    assert torch.allclose(x2.grad.cpu(), x1.grad, atol=1e-4)
    assert torch.allclose(w2.grad.cpu(), w1.grad, atol=1e-4)
    assert torch.allclose(b2.grad.cpu(), b1.grad, atol=1e-5)


def test_visual_actor_gpu_matches_cpu():
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import VisualActor
    torch.manual_seed(3)
    actor = VisualActor(obs_dim=24, act_dim=5, vis_dim=(3, 64, 64),
                        hidden_sizes=[32, 32])
    feats = torch.randn(4, 24)
    frames = torch.randn(4, 3, 64, 64)
    pi_c, logp_c = actor(MultiObservation(feats, frames),
                         deterministic=True)
    actor_g = VisualActor(obs_dim=24, act_dim=5, vis_dim=(3, 64, 64),
                          hidden_sizes=[32, 32]).to(DEV)
    actor_g.load_state_dict(actor.state_dict())
    pi_g, logp_g = actor_g(MultiObservation(feats.to(DEV), frames.to(DEV)),
                           deterministic=True)
    assert torch.allclose(pi_g.cpu(), pi_c, atol=1e-3), \
        (pi_g.cpu() - pi_c).abs().max()
    assert torch.allclose(logp_g.cpu(), logp_c, atol=1e-2)


def test_visual_sac_update_on_gpu():
    """One eager SAC update of the visual model entirely on GPU (conv
    kernels on the hot path) produces finite losses and gradients."""
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import (VisualActor,
                                                      VisualDoubleCritic)
    from torch_actor_critic_amd.optim import FlatAdam
    from copy import deepcopy

    torch.manual_seed(4)
    device = torch.device(DEV)
    actor = VisualActor(16, 4, (3, 64, 64), [32, 32],
                        act_limit=1.0).to(device)
    critic = VisualDoubleCritic(16, 4, (3, 64, 64), [32, 32]).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)

    buf = VisualReplayBuffer(100, act_dim=4, device=device)
    for i in range(20):
        mo = MultiObservation(torch.randn(16, device=device),
                              torch.randn(3, 64, 64, device=device))
        buf.store(mo, np.random.randn(4), float(i), mo, 0.0)

    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=8, start_steps=0, steps_per_epoch=1,
              max_ep_len=10, update_after=0, update_every=1, save_every=10)
    sac._critic_fp = q_opt.fp
    sac._actor_fp = pi_opt.fp
    sac._target_flat = None
    sac._target_critic = target

    samples = buf.sample(8)
    loss_q = sac.update_critic(q_opt, actor, critic, target, samples)
    loss_pi = sac.update_policy(pi_opt, actor, critic, samples)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss_q.item()))
    assert np.isfinite(float(loss_pi.item()))
    assert torch.isfinite(q_opt.fp.flat_grad).all()
    assert torch.isfinite(pi_opt.fp.flat_grad).all()


def test_visual_graphed_update_on_gpu():
    """The autograd hipGraph path captures the full visual SAC update
    (conv fwd/bwd kernels inside the graph) and replays it."""
    from copy import deepcopy
    from torch_actor_critic_amd.algo.graph import GraphedSACUpdate
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import (VisualActor,
                                                      VisualDoubleCritic)
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    torch.manual_seed(5)
    device = torch.device(DEV)
    actor = VisualActor(16, 4, (3, 64, 64), [32, 32],
                        act_limit=1.0).to(device)
    critic = VisualDoubleCritic(16, 4, (3, 64, 64), [32, 32]).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)

    buf = VisualReplayBuffer(200, act_dim=4, device=device)
    mo = MultiObservation(torch.randn(16, device=device),
                          torch.randn(3, 64, 64, device=device))
    buf.store(mo, np.zeros(4), 0.0, mo, 0.0)
    n = 100
    buf.features[:n].normal_()
    buf.next_features[:n].normal_()
    buf.frames[:n].random_(0, 255)
    buf.next_frames[:n].random_(0, 255)
    buf.actions[:n].uniform_(-1, 1)
    buf.rewards[:n].normal_()
    buf.size = n
    buf.ptr = n % buf.max_size
    buf._size_dev.fill_(n)

    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=8, start_steps=0, steps_per_epoch=1,
              max_ep_len=10, update_after=0, update_every=1, save_every=10)
    g = GraphedSACUpdate(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, 8, device)
    p0 = pi_opt.fp.flat.clone()
    t0 = target_flat.clone()
    for _ in range(5):
        g.step()
    torch.cuda.synchronize()
    assert not torch.allclose(p0, pi_opt.fp.flat)
    assert not torch.allclose(t0, target_flat)
    lq, lp = g.read_and_reset_losses(5)
    assert np.isfinite(lq) and np.isfinite(lp)
    assert torch.isfinite(pi_opt.fp.flat).all()


def test_paired_double_critic_matches_sequential():
    """The lockstep (paired-launch) VisualDoubleCritic forward/backward
    must match running q1/q2 sequentially."""
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import VisualDoubleCritic
    torch.manual_seed(9)
    device = torch.device(DEV)
    vdc = VisualDoubleCritic(12, 4, (3, 64, 64), [32, 32]).to(device)
    feats = torch.randn(6, 12, device=device)
    frames = torch.randn(6, 3, 64, 64, device=device)
    act = torch.randn(6, 4, device=device)
    mo = MultiObservation(feats, frames)

    q1p, q2p = vdc(mo, act)                      # paired path
    q1s = vdc.q1(mo, act)                        # sequential path
    q2s = vdc.q2(mo, act)
    assert torch.allclose(q1p, q1s, atol=1e-4), (q1p - q1s).abs().max()
    assert torch.allclose(q2p, q2s, atol=1e-4)

    # backward parity on a scalar loss
    loss_p = (q1p.square().mean() + q2p.square().mean())
    gp = torch.autograd.grad(loss_p, list(vdc.parameters()),
                             allow_unused=True)
    q1s2 = vdc.q1(mo, act)
    q2s2 = vdc.q2(mo, act)
    loss_s = (q1s2.square().mean() + q2s2.square().mean())
    gs = torch.autograd.grad(loss_s, list(vdc.parameters()),
                             allow_unused=True)
    for a, b in zip(gp, gs):
        if a is None and b is None:
            continue
        assert torch.allclose(a, b, atol=1e-3, rtol=1e-3), \
            (a - b).abs().max()


def test_visual_fused_sample_gpu():
    """The one-kernel Philox gather+dequantize matches the buffer
    contents: rows are self-consistent and frames round-trip through the
    u8 quantization within its step size."""
    import torch
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
    from torch_actor_critic_amd.envs.visual import MultiObservation

    n, feat, vis = 300, 6, (3, 8, 8)
    buf = VisualReplayBuffer(500, 4, device="cuda:0", seed=3)
    rng = np.random.default_rng(7)
    for i in range(n):
        f = np.full(feat, float(i), dtype=np.float32)
        frame = np.clip(rng.standard_normal(vis).astype(np.float32), -1, 1)
        mo = MultiObservation(torch.tensor(f), torch.tensor(frame))
        buf.store(mo, np.full(4, float(i), dtype=np.float32), float(i),
                  mo, float(i % 2))
    out = buf.make_static_batch(64)
    buf.sample_into(out)
    torch.cuda.synchronize()
    sv = out.states.features.cpu()
    idx = sv[:, 0].to(torch.long)
    assert (idx >= 0).all() and (idx < n).all()
    # row consistency across fields
    assert torch.allclose(out.actions.cpu()[:, 0].to(torch.long).float(),
                          idx.float())
    assert torch.allclose(out.rewards.cpu(), idx.float())
    assert torch.allclose(out.done.cpu(), (idx % 2).float())
    # frames dequantize to the stored values within the u8 step
    stored = buf.frames.cpu()[idx].to(torch.float32) / 127.5 - 1.0
    assert torch.allclose(out.states.frame.cpu(), stored, atol=1e-6)
    # fresh draws on the next call (device counter bumped)
    prev = out.states.features.clone()
    buf.sample_into(out)
    torch.cuda.synchronize()
    assert not torch.equal(prev, out.states.features)


def test_quad_forward_with_target_matches_sequential():
    """The 4-problem (target twins + live twins) critic-phase forward
    equals running target and live DoubleCritics separately, and its
    backward produces the same live-critic gradients."""
    import copy
    import torch
    from torch_actor_critic_amd.models.visual import VisualDoubleCritic
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.ops import functional as Fo

    Fo.set_compute_dtype("fp32")
    torch.manual_seed(21)
    B, feat, act_dim, vis = 16, 12, 4, (3, 36, 36)
    dc = VisualDoubleCritic(feat, act_dim, vis, [32, 32],
                            [8, 16, 16], [4, 3, 3], [2, 2, 1]).to(DEV)
    tg = copy.deepcopy(dc)
    for p in tg.parameters():
        p.requires_grad_(False)

    s = MultiObservation(torch.randn(B, feat, device=DEV),
                         torch.rand(B, *vis, device=DEV))
    ns = MultiObservation(torch.randn(B, feat, device=DEV),
                          torch.rand(B, *vis, device=DEV))
    a = torch.rand(B, act_dim, device=DEV) * 2 - 1
    a2 = torch.rand(B, act_dim, device=DEV) * 2 - 1

    # sequential reference
    dc.zero_grad()
    with torch.no_grad():
        r1t, r2t = tg(ns, a2)
    r1, r2 = dc(s, a)
    (r1.sum() + r2.sum()).backward()
    ref_grads = [p.grad.clone() for p in dc.parameters()
                 if p.grad is not None]

    dc.zero_grad()
    q1t, q2t, q1, q2 = dc.forward_with_target(tg, s, a, ns, a2)
    assert not q1t.requires_grad and not q2t.requires_grad
    assert torch.allclose(q1t, r1t, atol=1e-4), (q1t - r1t).abs().max()
    assert torch.allclose(q2t, r2t, atol=1e-4)
    assert torch.allclose(q1, r1, atol=1e-4)
    assert torch.allclose(q2, r2, atol=1e-4)
    (q1.sum() + q2.sum()).backward()
    got = [p.grad.clone() for p in dc.parameters() if p.grad is not None]
    assert len(got) == len(ref_grads)
    for g, r in zip(got, ref_grads):
        assert torch.allclose(g, r, atol=1e-3, rtol=1e-3), \
            (g - r).abs().max()


def test_visual_act_graph():
    """Captured B=1 visual acting: correct shape/range, fresh Philox
    noise per replay, and the sac.train lazy path completes a short
    visual training run with policy actions."""
    import torch
    from torch_actor_critic_amd.algo.act import VisualActGraph
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import VisualActor

    torch.manual_seed(3)
    dev = torch.device(DEV)
    actor = VisualActor(16, 4, (3, 64, 64), [32, 32],
                        act_limit=1.0).to(dev)
    vag = VisualActGraph(actor, 16, (3, 64, 64), 4, dev)
    mo = MultiObservation(torch.randn(16), torch.randn(3, 64, 64))
    a1 = vag.act(mo)
    a2 = vag.act(mo)
    assert a1.shape == (4,)
    assert np.all(np.abs(a1) <= 1.0 + 1e-6)
    assert not np.allclose(a1, a2)          # fresh noise per replay
    # different observation influences the action distribution
    mo2 = MultiObservation(torch.randn(16) * 3, torch.rand(3, 64, 64))
    a3 = vag.act(mo2)
    assert np.isfinite(a3).all()

    # sac.train exercises the lazy capture (start_steps=0 -> policy acts)
    from torch_actor_critic_amd.algo.sac import SAC
    from torch_actor_critic_amd.buffer.visual import VisualReplayBuffer
    from torch_actor_critic_amd.models.visual import VisualDoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd import envs

    env = envs.make("DeepMindWallRunner-v0")
    env.seed(0)
    actor2 = VisualActor(168, 56, (3, 64, 64), [32, 32],
                         act_limit=1.0).to(dev)
    critic2 = VisualDoubleCritic(168, 56, (3, 64, 64), [32, 32]).to(dev)
    buf = VisualReplayBuffer(2000, 56, device=dev)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=8, start_steps=0, steps_per_epoch=60,
              max_ep_len=50, update_after=30, update_every=10,
              save_every=10**9)
    sac.train(0, env, actor2, critic2, buf,
              FlatAdam(actor2), FlatAdam(critic2), render=False,
              logging=False)
    assert buf.size >= 60


def test_visual_trunk_b1_parity(ext):
    """Fused single-workgroup B=1 conv trunk vs the tiled conv kernels
    and a plain torch reference, both visual geometries and grayscale."""
    import torch.nn.functional as TF
    for (C, H, W) in [(3, 84, 84), (3, 64, 64), (1, 64, 64)]:
        torch.manual_seed(9)
        x = torch.randn(C, H, W, device=DEV)
        w1 = torch.randn(32, C, 8, 8, device=DEV) * 0.1
        b1 = torch.randn(32, device=DEV) * 0.1
        w2 = torch.randn(64, 32, 4, 4, device=DEV) * 0.05
        b2 = torch.randn(64, device=DEV) * 0.1
        w3 = torch.randn(64, 64, 3, 3, device=DEV) * 0.05
        b3 = torch.randn(64, device=DEV) * 0.1
        out = ext.visual_trunk_b1(x, w1, b1, w2, b2, w3, b3, 4, 2, 1)
        xr = x.unsqueeze(0).cpu()
        r = TF.relu(TF.conv2d(xr, w1.cpu(), b1.cpu(), stride=4))
        r = TF.relu(TF.conv2d(r, w2.cpu(), b2.cpu(), stride=2))
        r = TF.relu(TF.conv2d(r, w3.cpu(), b3.cpu(), stride=1))
        ref = r.reshape(-1)
        assert out.shape == ref.shape
        assert torch.allclose(out.cpu(), ref, atol=1e-3, rtol=1e-4), \
            ((C, H, W), (out.cpu() - ref).abs().max())


def test_visual_actor_b1_fast_path_matches_batched(ext):
    """VisualActor acting fast path (B=1 no_grad fused trunk) must give
    the same deterministic action as the batched tile-kernel path."""
    from torch_actor_critic_amd.envs.visual import MultiObservation
    from torch_actor_critic_amd.models.visual import VisualActor
    torch.manual_seed(17)
    actor = VisualActor(17, 6, (3, 84, 84), [64, 64], 1.0).to(DEV)
    feats = torch.randn(17, device=DEV)
    frame = torch.randn(3, 84, 84, device=DEV)
    with torch.no_grad():
        a1, _ = actor(MultiObservation(feats, frame), deterministic=True,
                      with_logprob=False)
        a2, _ = actor(MultiObservation(feats.unsqueeze(0).repeat(2, 1),
                                       frame.unsqueeze(0).repeat(2, 1, 1, 1)),
                      deterministic=True, with_logprob=False)
    assert torch.allclose(a1.reshape(-1), a2[0], atol=5e-4, rtol=1e-4), \
        (a1.reshape(-1) - a2[0]).abs().max()


def _trunk_id(case):
    return "x".join(str(v) for v in case[0])


@pytest.mark.parametrize("case", kr.TRUNK_CASES, ids=_trunk_id)
def test_visual_trunk_b1_output_larger_than_frame(ext, case):
    """Strides 4/1/1 (1x36x36: layer 2 writes 1600 floats, the frame has
    1296): layer 2's output is larger than the frame, so it must not be
    placed over layer 1's output, which layer 2 is still reading.
    Integer operands keep all three layers exact (test_kernel_refs.py),
    so the fused trunk must equal the float64 reference bit for bit."""
    vis, filters, strides = case
    x, ws, bs = kr.trunk_operands(vis, filters)
    ref = kr.trunk_ref(x, ws, bs, strides)[-1][0].reshape(-1)
    dev = [t.to(DEV) for t in (x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
    out = ext.visual_trunk_b1(*dev, *strides)
    msg = kr.describe_mismatch(out.cpu().double(), ref)
    assert msg == "", msg


@pytest.mark.parametrize("case", kr.TRUNK_CASES, ids=_trunk_id)
def test_cnn_trunk_b1_env_matches_tiled_path(case, monkeypatch):
    """_CnnTrunk with TAC_AMD_TRUNK_B1=1 returns the tiled-path answer
    at the geometries above: with integer conv operands both conv stacks
    are exact, so the dense layers see identical bits."""
    from torch_actor_critic_amd.models.visual import simple_cnn
    vis, filters, strides = case
    x, ws, bs = kr.trunk_operands(vis, filters)
    net = simple_cnn(vis, list(filters), [8, 4, 3], list(strides))
    with torch.no_grad():
        for i in range(3):
            conv = getattr(net, f"conv_{i}")
            conv.weight.copy_(ws[i])
            conv.bias.copy_(bs[i])
    net = net.to(DEV)
    frame = x.unsqueeze(0).to(DEV)
    with torch.no_grad():
        monkeypatch.delenv("TAC_AMD_TRUNK_B1", raising=False)
        tiled = net(frame)
        flat_ref = net.flatten(net.conv_2(net.conv_1(net.conv_0(frame))))
        monkeypatch.setenv("TAC_AMD_TRUNK_B1", "1")
        fused = net(frame)
    want = kr.trunk_ref(x, ws, bs, strides)[-1][0].reshape(1, -1)
    assert kr.describe_mismatch(flat_ref.cpu().double(), want) == ""
    assert tiled.shape == fused.shape == (1, 1)
    assert torch.equal(fused, tiled), (fused, tiled)
