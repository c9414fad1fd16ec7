"""mwgrad_het_adam (heterogeneous wgrad with Adam, polyak and the W^T
refresh applied in the tile / combine epilogue) against the two launches
it replaces: mwgrad_het followed by adam_t on the same inputs."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, B1, B2, EPS, WD, RHO = 3e-4, 0.9, 0.999, 1e-8, 0.0, 0.995

# (N, K, ldx, x_off, masked): edge tiles on both axes, N < 64, K not a
# multiple of 4, a strided/offset x, a width-1 problem
PROBLEMS = [(6, 64, 64, 0, False), (70, 23, 32, 5, True),
            (1, 70, 70, 0, False)]
# 12 x 32 = 384 tiles: the launcher stops splitting along M at 384 tiles,
# whatever M is, so these run the un-split tile epilogue over SEVERAL
# K-steps (one block per tile, no quarter blocks); first problem has edge
# tiles on both axes
MANY_TILES = [(250, 500, 500, 0, True)] + \
    [(256, 512, 512, 0, i % 2 == 0) for i in range(11)]


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


def _inputs(M, problems=PROBLEMS):
    """Problem operands (shared by both paths) and the flat layout
    w|b per problem."""
    g = torch.Generator().manual_seed(1000 + M)
    ops, off = [], 0
    for (N, K, ldx, x_off, masked) in problems:
        dy = torch.randn(M, N, generator=g).to(DEV)
        ym = torch.randn(M, N, generator=g).to(DEV) if masked else None
        x = torch.randn(M * ldx + x_off, generator=g).to(DEV)
        ops.append(dict(dy=dy, ym=ym, x=x, N=N, K=K, ldx=ldx, x_off=x_off,
                        w_off=off, b_off=off + N * K))
        off += N * K + N
    return ops, off


def _state(n, with_targ):
    g = torch.Generator().manual_seed(7)
    st = dict(p=(torch.rand(n, generator=g) * 2 - 1).to(DEV),
              grad=torch.zeros(n, device=DEV),
              m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV),
              targ=((torch.rand(n, generator=g) * 2 - 1).to(DEV)
                    if with_targ else None),
              step=torch.ones(1, dtype=torch.int64, device=DEV))
    return st


def _wgrad_args(ops, st, M, leave_out_last=False):
    use = ops[:-1] if leave_out_last else ops
    dws = [st["grad"][o["w_off"]:o["w_off"] + o["N"] * o["K"]]
           .view(o["N"], o["K"]) for o in use]
    dbs = [st["grad"][o["b_off"]:o["b_off"] + o["N"]] for o in use]
    return ([o["dy"] for o in use], [o["ym"] for o in use],
            [o["x"] for o in use], dws, dbs, [M] * len(use),
            [o["N"] for o in use], [o["K"] for o in use],
            [o["N"] for o in use], [o["ldx"] for o in use],
            [o["x_off"] for o in use])


def _wts(ops):
    return [torch.zeros(o["K"], o["N"], device=DEV) for o in ops]


# fp32 K-step is 16 rows, bf16 is 64: M=16 fp32 and M=64 bf16 stay
# un-split (tile epilogue); M=64 and M=256 fp32 split along M (combine)
@pytest.mark.parametrize("with_targ", [True, False])
@pytest.mark.parametrize("dtype,M", [("bf16", 64), ("fp32", 16),
                                     ("fp32", 64), ("fp32", 256)])
def test_wgrad_adam_matches_wgrad_then_adam(ext, dtype, M, with_targ):
    _check_against_wgrad_then_adam(ext, dtype, M, with_targ, PROBLEMS,
                                   split=(dtype == "fp32" and M > 16))


# M spans two K-steps in either dtype (fp32 16 rows, bf16 64 rows)
@pytest.mark.parametrize("dtype,M", [("fp32", 32), ("bf16", 128)])
def test_wgrad_adam_unsplit_multi_k_step(ext, dtype, M):
    _check_against_wgrad_then_adam(ext, dtype, M, True, MANY_TILES,
                                   split=False)


def _check_against_wgrad_then_adam(ext, dtype, M, with_targ, problems,
                                   split):
    from torch_actor_critic_amd.ops import functional as Fo
    ops, n = _inputs(M, problems)
    ref, new = _state(n, with_targ), _state(n, with_targ)
    ref_wt, new_wt = _wts(ops), _wts(ops)
    Fo.set_compute_dtype(dtype)
    try:
        # the path this case is meant to take
        assert (ext.mwgrad_het_adam_split(
            [M] * len(ops), [o["N"] for o in ops],
            [o["K"] for o in ops]) > 1) == split
        ext.mwgrad_het(*_wgrad_args(ops, ref, M))
        ext.adam_t(ref["p"], ref["grad"], ref["m"], ref["v"], ref["step"],
                   LR, B1, B2, EPS, WD, [o["w_off"] for o in ops], ref_wt,
                   ref["targ"], RHO)
        ext.mwgrad_het_adam(*_wgrad_args(ops, new, M), new["p"],
                            new["grad"], new["m"], new["v"], new["step"],
                            LR, B1, B2, EPS, WD, new_wt, new["targ"], RHO)
        torch.cuda.synchronize()
    finally:
        Fo.set_compute_dtype("fp32")

    # both paths run the same MFMA code: gradients are bit-equal
    assert torch.equal(new["grad"], ref["grad"])
    assert ref["grad"].abs().max() > 0
    # a skipped or doubled element at step 1 is off by ~lr = 3e-4;
    # contraction-order noise at |p| <= 1 is ~1e-7
    for k in ("p", "m", "v") + (("targ",) if with_targ else ()):
        assert torch.allclose(new[k], ref[k], atol=1e-6, rtol=0), \
            (k, (new[k] - ref[k]).abs().max())
    p0 = _state(n, with_targ)["p"]
    assert (new["p"] - p0).abs().min() > 0.5 * LR   # every element stepped
    for o, wn, wr in zip(ops, new_wt, ref_wt):
        assert torch.allclose(wn, wr, atol=1e-6, rtol=0)
        w = new["p"][o["w_off"]:o["w_off"] + o["N"] * o["K"]]
        assert torch.equal(wn, w.view(o["N"], o["K"]).t())


def test_wgrad_adam_without_wt_caches(ext):
    """wt slots are optional per problem."""
    M = 16
    ops, n = _inputs(M)
    ref, new = _state(n, False), _state(n, False)
    wt1 = torch.zeros(ops[1]["K"], ops[1]["N"], device=DEV)
    ext.mwgrad_het(*_wgrad_args(ops, ref, M))
    ext.adam_t(ref["p"], ref["grad"], ref["m"], ref["v"], ref["step"],
               LR, B1, B2, EPS, WD, [], [], None, 0.0)
    ext.mwgrad_het_adam(*_wgrad_args(ops, new, M), new["p"], new["grad"],
                        new["m"], new["v"], new["step"], LR, B1, B2, EPS,
                        WD, [None, wt1, None], None, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(new["grad"], ref["grad"])
    assert torch.allclose(new["p"], ref["p"], atol=1e-6, rtol=0)
    o = ops[1]
    w = new["p"][o["w_off"]:o["w_off"] + o["N"] * o["K"]]
    assert torch.equal(wt1, w.view(o["N"], o["K"]).t())


def test_wgrad_adam_coverage_gate_raises(ext):
    """A problem left out would leave its parameters without their Adam
    step: the launcher refuses and touches nothing."""
    M = 16
    ops, n = _inputs(M)
    st = _state(n, False)
    p0 = st["p"].clone()
    with pytest.raises(RuntimeError, match="tile the flat gradient"):
        ext.mwgrad_het_adam(*_wgrad_args(ops, st, M, leave_out_last=True),
                            st["p"], st["grad"], st["m"], st["v"],
                            st["step"], LR, B1, B2, EPS, WD,
                            _wts(ops[:-1]), None, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(st["p"], p0)
    assert float(st["grad"].abs().max()) == 0.0


def test_range_gate(ext):
    ok = ext.ranges_tile_exactly
    assert ok([(0, 4), (4, 2)], 6) and ok([(4, 2), (0, 4)], 6)
    assert ok([(0, 3), (3, 0), (3, 3)], 6)          # empty range ignored
    assert not ok([(0, 4), (5, 1)], 6)              # hole
    assert not ok([(0, 4), (3, 3)], 6)              # overlap
    assert not ok([(0, 4), (4, 2)], 7)              # tail missing
    assert not ok([(0, 6), (0, 6)], 6)              # doubled
    assert not ok([(1, 5)], 6)                      # head missing
