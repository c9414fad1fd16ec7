"""The small-shape mgemm path (fused.hip: mgemm_small_kernel, taken in
bf16 mode when M <= 128 and K, K2 <= 256) against the pipelined kernel it
replaces (bit for bit, randn operands), against float64 (integer
operands), at the host gate, and through five engine updates.

The shapes are the 15 launches of one flagship update (HalfCheetah,
batch 64, hidden 256) plus the smallest ones that reach every staging
form: ragged M / N / K, K around the 32-wide MFMA chunk, strided and
offset A, the dword and the float4 load forms, 1 / 2 / 4 problems."""

import pytest
import torch

import kernel_refs as kr
from kernel_refs import MgCase

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


@pytest.fixture(autouse=True)
def _restore(ext):
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype("fp32")
    prev = ext.mgemm_small_mode(1)
    yield
    ext.mgemm_small_mode(prev)
    Fo.set_compute_dtype("fp32")


def _set_dtype(dtype):
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype(dtype)


def _dev(t):
    return None if t is None else t.to(DEV)


def _b(n, *on):
    return tuple(i in on for i in range(n))


# name, case, y_offs: per-problem column offsets into ONE [M, ldy] output
# (the actor heads), or None for one output per problem
FLAGSHIP = [
    (MgCase("actor_fwd_l0", 128, 256, 17, relu=True, lda=32), None),
    (MgCase("actor_fwd_l1", 128, 256, 256, relu=True), None),
    (MgCase("actor_heads", 128, 6, 256, nz=2, bias=(True, True), ldy=12),
     (0, 6)),
    (MgCase("critic_fwd_l0_nz4", 64, 256, 23, nz=4, bias=(True,) * 4,
            relu=True, lda=32), None),
    (MgCase("critic_fwd_l1_nz4", 64, 256, 256, nz=4, bias=(True,) * 4,
            relu=True), None),
    (MgCase("critic_fwd_out_nz4", 64, 1, 256, nz=4, bias=(True,) * 4),
     None),
    (MgCase("critic_fwd_l0_nz2", 64, 256, 23, nz=2, bias=(True,) * 2,
            relu=True, lda=32), None),
    (MgCase("critic_fwd_l1_nz2", 64, 256, 256, nz=2, bias=(True,) * 2,
            relu=True), None),
    (MgCase("critic_fwd_out_nz2", 64, 1, 256, nz=2, bias=(True,) * 2),
     None),
    (MgCase("critic_dgrad_out_k1", 64, 256, 1, nz=2, bias=(False,) * 2),
     None),
    (MgCase("critic_dgrad_l1", 64, 256, 256, nz=2, bias=(False,) * 2,
            mask=True), None),
    (MgCase("pi_dgrad_l0", 64, 23, 256, nz=2, bias=(False,) * 2, mask=True,
            ldy=32), None),
    (MgCase("head_dgrad_sum2", 64, 256, 6, K2=6, bias=(False,)), None),
    (MgCase("actor_dgrad_l1", 64, 256, 256, bias=(False,), mask=True),
     None),
]
# the 15th flagship launch is mgemm_r1 at 64 x 256 x 256, nz = 2 (R1 below)

EDGES = [
    (MgCase("m1_n1_k1", 1, 1, 1), None),
    (MgCase("m1_k31", 1, 33, 31, relu=True), None),
    (MgCase("m16_k32_vec", 16, 64, 32), None),
    (MgCase("m33_k6_xoff", 33, 64, 6, lda=32, x_off=17), None),
    (MgCase("m64_k23_xoff4", 64, 33, 23, lda=32, x_off=4, relu=True), None),
    (MgCase("m65_k33_masked", 65, 33, 33, bias=(False,), mask=True), None),
    (MgCase("m128_k128_masked_relu", 128, 64, 128, relu=True, mask=True),
     None),
    (MgCase("m16_k255", 16, 256, 255, bias=(False,)), None),
    (MgCase("m64_k32_masked_vec", 64, 64, 32, bias=(False,), mask=True),
     None),
    (MgCase("x_offs_nz4", 33, 23, 17, nz=4, bias=_b(4, 0, 2), lda=32,
            x_offs=(0, 3, 8, 15), ldy=32), None),
    (MgCase("x_offs_nz2_vec", 64, 64, 128, nz=2, bias=_b(2, 1), lda=256,
            x_offs=(0, 128)), None),
    (MgCase("sum2_masked_nz2", 33, 64, 256, K2=6, nz=2, bias=_b(2, 0),
            mask=True), None),
    (MgCase("sum2_k2_256", 65, 33, 128, K2=256, relu=True), None),
]

CASES = FLAGSHIP + EDGES
R1 = [(64, 256, 256, 2), (64, 23, 256, 1)]     # M, N, K, nz


def run_mgemm(ext, o, y_offs=None):
    """One mgemm launch into sentinel-filled [M, ldy] storage; returns the
    storage tensors (one per problem, or the one shared by all)."""
    c = o.case
    lda, ldy = c.lda or c.K, c.ldy or c.N
    if c.x_offs:
        src = o.xs[0].to(DEV)
        xs = [src] * c.nz
    else:
        xs = [x.to(DEV) for x in o.xs]
    if y_offs is None:
        bufs = [torch.full((c.M, ldy), kr.SENTINEL, device=DEV)
                for _ in range(c.nz)]
        ys = bufs
    else:
        bufs = [torch.full((c.M, ldy), kr.SENTINEL, device=DEV)]
        ys = [bufs[0].view(-1)[off:] for off in y_offs]
    ext.mgemm(xs, [w.to(DEV) for w in o.ws], [_dev(b) for b in o.bs], ys,
              [_dev(m) for m in o.masks], c.M, c.N, c.K, lda, ldy, c.relu,
              [x.to(DEV) for x in o.xs2], [w.to(DEV) for w in o.ws2],
              [_dev(m) for m in o.masks2], c.K2, c.x_off, 0,
              list(c.x_offs))
    torch.cuda.synchronize()
    return [b.cpu() for b in bufs]


def run_r1(ext, o, ldy):
    nz = len(o.cols)
    ys = [torch.full((o.M, ldy), kr.SENTINEL, device=DEV)
          for _ in range(nz)]
    ext.mgemm_r1([t.to(DEV) for t in o.cols], [t.to(DEV) for t in o.rows],
                 [t.to(DEV) for t in o.ws], ys,
                 [t.to(DEV) for t in o.masks], o.M, o.N, o.K, ldy)
    torch.cuda.synchronize()
    return [y.cpu() for y in ys]


def _assert_pad(name, case, bufs, y_offs):
    """Every column outside the logical outputs still holds the sentinel,
    every column inside was written."""
    ldy = case.ldy or case.N
    written = torch.zeros(ldy, dtype=torch.bool)
    for off in (y_offs or (0,)):
        written[off:off + case.N] = True
    for z, buf in enumerate(bufs):
        assert bool((buf[:, ~written] == kr.SENTINEL).all()), \
            f"{name}[{z}]: stray writes in the pad"
        assert bool((buf[:, written] != kr.SENTINEL).all()), \
            f"{name}[{z}]: elements left unwritten"


def _both_modes(ext, fn):
    out = {}
    for mode in (0, 1):
        ext.mgemm_small_mode(mode)
        out[mode] = fn()
    return out[0], out[1]


# ---------------------------------------------------------------------------
# new path == old path, bit for bit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case,y_offs", CASES,
                         ids=[c.name for c, _ in CASES])
def test_small_equals_pipelined(ext, case, y_offs):
    assert case.M <= 128 and case.K <= 256 and case.K2 <= 256
    o = kr.mgemm_operands(case, "randn", seed=3)
    _set_dtype("bf16")
    old, new = _both_modes(ext, lambda: run_mgemm(ext, o, y_offs))
    for z, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), \
            f"{case.name}[{z}]: {int((a != b).sum())} elements differ"
    _assert_pad(case.name, case, new, y_offs)


@pytest.mark.parametrize("M,N,K,nz", R1)
def test_small_r1_equals_pipelined(ext, M, N, K, nz):
    o = kr.r1_operands(M, N, K, nz, "randn", seed=3)
    _set_dtype("bf16")
    ldy = N + 9
    old, new = _both_modes(ext, lambda: run_r1(ext, o, ldy))
    for z, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), f"r1 {M}x{N}x{K}[{z}]"
        assert bool((b[:, N:] == kr.SENTINEL).all())
        assert bool((b[:, :N] != kr.SENTINEL).all())


# ---------------------------------------------------------------------------
# the host gate
# ---------------------------------------------------------------------------

GATE = [
    ("bf16", MgCase("k257", 64, 64, 257)),
    ("bf16", MgCase("m129", 129, 64, 64)),
    ("bf16", MgCase("sum2_k2_257", 64, 33, 40, K2=257)),
    ("fp32", MgCase("fp32_small", 64, 64, 64, relu=True)),
]


@pytest.mark.parametrize("dtype,case", GATE,
                         ids=[c.name for _, c in GATE])
def test_gate_keeps_pipelined_kernel(ext, dtype, case):
    """Above the gate (and in fp32 mode) the mode changes nothing, and
    the result is still right."""
    o = kr.mgemm_operands(case, "int")
    refs = kr.mgemm_ref(o)
    _set_dtype(dtype)
    old, new = _both_modes(ext, lambda: run_mgemm(ext, o))
    for a, b, (ref, _) in zip(old, new, refs):
        assert torch.equal(a, b)
        assert kr.describe_mismatch(b[:, :case.N].double(), ref) == ""


def test_mode_switch_returns_previous(ext):
    assert ext.mgemm_small_mode(0) == 1       # the fixture set 1
    assert ext.mgemm_small_mode(1) == 0
    with pytest.raises(RuntimeError):
        ext.mgemm_small_mode(-1)
    assert ext.mgemm_small_mode(1) == 1


# ---------------------------------------------------------------------------
# against float64 (integer operands: exact in bf16, any summation order)
# ---------------------------------------------------------------------------

def _named(name):
    return next(cy for cy in CASES if cy[0].name == name)


@pytest.mark.parametrize("name", ["critic_dgrad_l1", "sum2_masked_nz2",
                                  "head_dgrad_sum2"])
def test_small_exact_vs_float64(ext, name):
    case, y_offs = _named(name)
    o = kr.mgemm_operands(case, "int")
    refs = kr.mgemm_ref(o)
    _set_dtype("bf16")
    ext.mgemm_small_mode(1)
    ys = run_mgemm(ext, o, y_offs)
    for z, (y, (ref, _)) in enumerate(zip(ys, refs)):
        assert float(ref.abs().max()) < kr.EXACT_LIMIT
        msg = kr.describe_mismatch(y[:, :case.N].double(), ref)
        assert msg == "", f"{name}[{z}]: {msg}"


def test_small_r1_exact_vs_float64(ext):
    M, N, K, nz = R1[0]
    o = kr.r1_operands(M, N, K, nz, "int")
    refs = kr.r1_ref(o)
    _set_dtype("bf16")
    ext.mgemm_small_mode(1)
    for z, (y, (ref, _)) in enumerate(zip(run_r1(ext, o, N), refs)):
        msg = kr.describe_mismatch(y.double(), ref)
        assert msg == "", f"r1[{z}]: {msg}"


# ---------------------------------------------------------------------------
# engine level: five HalfCheetah-shaped updates under each mode
# ---------------------------------------------------------------------------

B, O, A = 64, 17, 6


def _engine():
    from copy import deepcopy
    from torch_actor_critic_amd.algo.engine import FusedSACEngine
    from torch_actor_critic_amd.algo.sac import SAC, _freeze
    from torch_actor_critic_amd.buffer.replay import ReplayBuffer
    from torch_actor_critic_amd.models.mlp import Actor, DoubleCritic
    from torch_actor_critic_amd.optim import FlatAdam
    from torch_actor_critic_amd.parallel.flat import flatten_module_like

    torch.manual_seed(11)
    device = torch.device(DEV)
    actor = Actor(O, A, [256, 256], act_limit=1.0).to(device)
    critic = DoubleCritic(O, A, [256, 256]).to(device)
    target = deepcopy(critic)
    _freeze(target, True)
    pi_opt, q_opt = FlatAdam(actor), FlatAdam(critic)
    target_flat = flatten_module_like(target)
    buf = ReplayBuffer(256, O, A, device=device)
    sac = SAC(alpha=0.2, gamma=0.99, polyak=0.995, reward_scale=1.0,
              epochs=1, batch_size=B, start_steps=0, steps_per_epoch=1,
              max_ep_len=100, update_after=0, update_every=1, save_every=10)
    eng = FusedSACEngine(sac, actor, critic, target, buf, pi_opt, q_opt,
                         target_flat, B, device, sample=False,
                         capture=False, philox_seed=7)
    return eng, pi_opt, q_opt, target_flat


def _batch(i):
    g = torch.Generator().manual_seed(50 + i)
    s = torch.randn(B, O, generator=g)
    a = torch.rand(B, A, generator=g) * 2 - 1
    r = torch.randn(B, generator=g)
    ns = torch.randn(B, O, generator=g)
    d = (torch.rand(B, generator=g) > 0.9).float()
    return [t.to(DEV) for t in (s, a, r, ns, d)]


def test_engine_updates_equal_under_both_modes(ext):
    _set_dtype("bf16")
    state = {}
    for mode in (0, 1):
        ext.mgemm_small_mode(mode)
        eng, pi_opt, q_opt, target_flat = _engine()
        for i in range(5):
            eng.load_batch(*_batch(i))
            eng._run_once()
        torch.cuda.synchronize()
        state[mode] = dict(actor=pi_opt.fp.flat.clone(),
                           critic=q_opt.fp.flat.clone(),
                           target=target_flat.clone(),
                           loss_q=eng.loss_q_acc.clone(),
                           loss_pi=eng.loss_pi_acc.clone())
    for k, v in state[0].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, state[1][k]), \
            (k, float((v - state[1][k]).abs().max()))
    assert float(state[1]["loss_q"].abs().sum()) > 0
