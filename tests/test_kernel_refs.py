"""CPU check of the precondition behind the exact GPU kernel tests
(test_gpu_mgemm.py, test_gpu_conv_exact.py, test_gpu_wgrad.py): for the
integer operands of every case table, the float64 reference is
integer-valued and both max|ref| and the absolute-value contraction
sum|a||b| stay below 2^24.  Then every partial sum any kernel can form,
in fp32 or from bf16-rounded operands, is exact, and bit equality is the
right assertion.  Also asserts the launch plans the wgrad case tables are
listed with, and that a plain fp32 evaluation of Adam stays within half
of the bounds the GPU Adam tests assert (test_gpu_adam_t.py).  The host
Philox4x32-10 is held to the published known-answer vectors, and the
bounds of test_gpu_heads_losses.py and the noise cap of test_gpu_philox.py
to the same fairness condition as Adam's."""

import numpy as np
import pytest
import torch

import kernel_refs as kr


def _check_exact(name, ref, s_abs):
    assert torch.equal(ref, ref.round()), f"{name}: reference not integer"
    assert float(ref.abs().max()) < kr.EXACT_LIMIT, name
    assert float(s_abs.max()) < kr.EXACT_LIMIT, name
    # s_abs bounds every partial sum, hence the reference itself
    assert bool((ref.abs() <= s_abs).all()), name


def _check_bf16_exact(name, *tensors):
    for t in tensors:
        if t is not None:
            assert torch.equal(kr.bf16_round(t), t), f"{name}: not bf16-exact"


@pytest.mark.parametrize("case", kr.MGEMM_CASES, ids=lambda c: c.name)
def test_mgemm_cases_are_exact(case):
    o = kr.mgemm_operands(case, "int")
    _check_bf16_exact(case.name, *o.xs, *o.ws, *o.xs2, *o.ws2)
    for z, (ref, s) in enumerate(kr.mgemm_ref(o)):
        _check_exact(f"{case.name}[{z}]", ref, s)
    # bf16 rounding of exact operands changes nothing
    for (r32, _), (r16, _) in zip(kr.mgemm_ref(o), kr.mgemm_ref(o, True)):
        assert torch.equal(r32, r16)
    # the layout fits its storage
    lda = case.lda or case.K
    for z in range(case.nz):
        assert o.off(z) + case.K <= lda
    assert len(case.bias) == case.nz


@pytest.mark.parametrize("case", kr.MGEMM_CASES, ids=lambda c: c.name)
def test_mgemm_cases_reach_their_path(case):
    """The host plan, recomputed, takes the path each case is named for
    in both compute dtypes."""
    for bf16 in (False, True):
        split, k_chunk, nt = kr.mgemm_plan(case.M, case.N, case.K, case.nz,
                                           bf16, case.K2 > 0)
        if case.expect == "split":
            assert split > 1 and nt == 1
            if "ragged" in case.name:
                assert case.K % k_chunk != 0
        elif case.expect == "nosplit":
            assert split == 1 and nt == 1
        elif case.expect == "nt":
            assert split == 1 and nt == 2
            assert -(-case.N // 64) % 2 == 1     # odd tile count
        else:
            assert split == 1 and nt == 1


@pytest.mark.parametrize("M,N,K", kr.R1_SHAPES)
def test_r1_cases_are_exact(M, N, K):
    o = kr.r1_operands(M, N, K, max(kr.R1_NZ), "int")
    _check_bf16_exact("r1", *o.cols, *o.rows, *o.ws)
    for col, row in zip(o.cols, o.rows):
        prod = col[:, None] * row[None, :]
        assert float(prod.abs().max()) <= 9.0
        _check_bf16_exact("r1 product", prod)
    for (ref, s), (r16, _) in zip(kr.r1_ref(o), kr.r1_ref(o, True)):
        _check_exact("r1", ref, s)
        assert torch.equal(ref, r16)


@pytest.mark.parametrize("geom", kr.CONV_GEOMS, ids=kr.conv_id)
def test_conv_cases_are_exact(geom):
    S = geom[7]
    for seed in range(4):                # the multi tests use seeds 0..3
        o = kr.conv_operands(geom, "int", seed)
        _check_bf16_exact("conv", o.x, o.w, o.b, o.dy)
        for relu in (False, True):
            ref, s = kr.conv_fwd_ref(o.x, o.w, o.b, S, relu)
            _check_exact("conv fwd", ref, s)
        for mask in (None, o.mask):
            refs = kr.conv_bwd_ref(o.x, o.w, o.dy, S, mask)
            sabs = kr.conv_bwd_abs(o.x, o.w, o.dy, S, mask)
            for nm, r, s in zip(("dx", "dw", "db"), refs, sabs):
                _check_exact(f"conv {nm}", r, s)


@pytest.mark.parametrize("case", kr.TRUNK_CASES, ids=lambda c: str(c[0]))
def test_trunk_case_is_exact(case):
    vis, filters, strides = case
    x, ws, bs = kr.trunk_operands(vis, filters)
    for i, (ref, s) in enumerate(kr.trunk_ref(x, ws, bs, strides)):
        _check_exact(f"trunk layer {i}", ref, s)
    acts = kr.trunk_ref(x, ws, bs, strides)
    # the geometry the case exists for: layer 2's output outgrows the frame
    assert acts[1][0].numel() > x.numel()
    # ... and everything still fits the kernel's 40960-float LDS plan
    assert x.numel() + acts[0][0].numel() + acts[1][0].numel() <= 40960
    assert float(acts[2][0].abs().max()) > 0


# ---------------------------------------------------------------------------
# dense wgrad
# ---------------------------------------------------------------------------

def _check_wgrad_ops_exact(name, ops):
    for z, o in enumerate(ops):
        p = o.prob
        _check_bf16_exact(name, o.dy, o.x)
        dw, db, s_dw, s_db = kr.wgrad_ref(o.dy_v, o.x_v, o.mask_v)
        _check_exact(f"{name}[{z}] dw", dw, s_dw)
        _check_exact(f"{name}[{z}] db", db, s_db)
        dw16, db16, _, _ = kr.wgrad_ref(o.dy_v, o.x_v, o.mask_v, bf16=True)
        assert torch.equal(dw, dw16) and torch.equal(db, db16)
        assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0
        # the layout fits its storage
        assert p.ld_dy >= p.N and p.x_off + p.K <= p.ld_x
        assert o.dy.shape == (p.M, p.ld_dy) and o.x.shape == (p.M, p.ld_x)
        assert (o.mask is not None) == p.mask
        if p.mask:
            assert o.mask.shape == o.dy.shape
            vals = set(o.mask_v.unique().tolist())
            assert vals == {-1.0, 0.0, 1.0}, (name, vals)


@pytest.mark.parametrize("case", kr.MWGRAD_CASES, ids=lambda c: c.name)
def test_mwgrad_cases_are_exact(case):
    assert 1 <= case.nz <= 2 and len(case.bias) == case.nz
    _check_wgrad_ops_exact(case.name, kr.wgrad_operands(case.problems, "int"))


@pytest.mark.parametrize("case", kr.MWGRAD_HET_CASES, ids=lambda c: c.name)
def test_mwgrad_het_cases_are_exact(case):
    assert 1 <= len(case.problems) <= 12
    _check_wgrad_ops_exact(case.name, kr.wgrad_operands(case.problems, "int"))


@pytest.mark.parametrize("case", kr.MWGRAD_CASES, ids=lambda c: c.name)
def test_mwgrad_cases_reach_their_path(case):
    """The host plan of fused.hip::mwgrad, recomputed, is the one each
    case is listed with, in both compute dtypes."""
    for bf16, want in zip((False, True), case.expect):
        split, m_chunk, chunks, tiles = kr.mwgrad_plan(
            case.M, case.N, case.K, case.nz, bf16)
        last = case.M - (split - 1) * m_chunk
        assert 1 <= last <= m_chunk
        if want == "split":
            assert split > 1
        elif want is not None:
            assert (split, last) == want, (case.name, bf16, split, last)
    bk32, bk16 = 16, 64
    if case.name == "unsplit_multi_step":
        for bf16, steps in ((False, 9), (True, 3)):
            split, m_chunk, chunks, tiles = kr.mwgrad_plan(
                case.M, case.N, case.K, case.nz, bf16)
            assert (split, chunks, tiles) == (1, steps, 384)
        assert case.M % bk16 == 2 and case.M % bk32 == 2
    if case.name == "interior_strided":
        # bf16 float4 staging: whole 64x64 tiles exist on both operands,
        # strides are multiples of 4 and the x offset is 16-byte aligned
        assert case.M >= 64 and case.N >= 64 and case.K >= 64
        assert case.lddy % 4 == 0 and case.ldx % 4 == 0
        assert case.x_off % 4 == 0 and case.mask
    if case.name == "edge_strided":
        assert case.x_off % 2 == 1 and case.N < 64 and case.K < 64
    if case.name == "nobias_mixed":
        assert set(case.bias) == {True, False}


@pytest.mark.parametrize("case", kr.MWGRAD_HET_CASES, ids=lambda c: c.name)
def test_mwgrad_het_cases_reach_their_path(case):
    """The plan of mwgrad_het_impl / het_split, recomputed, in both dtypes
    and under the XCD-clustered enumeration and the 128x128 sub-tiling."""
    probs = case.problems
    for bf16 in (False, True):
        for xcd in (False, True):
            for rnrk in (False, True):
                plan = kr.het_plan(probs, bf16, xcd, rnrk)
                want = kr.HET_PLANS.get((case.name, bf16, xcd, rnrk))
                if want is not None:
                    assert plan == want, (case.name, bf16, xcd, rnrk, plan)
                split, m_chunk, chunks, blk = plan
                assert 1 <= split <= 64 and split * m_chunk >= \
                    max(p.M for p in probs) > (split - 1) * m_chunk
                tiles = kr.het_tiles(probs, bf16, xcd, rnrk)
                if not (rnrk and bf16):
                    assert all(t[:2] == (1, 1) for t in tiles)
    for bf16 in (False, True):
        assert (case.name, bf16, False, False) in kr.HET_PLANS
    if case.name == "phase64":
        assert any(p.mask for p in probs) and any(p.ldx for p in probs)
        assert kr.het_plan(probs, True)[:3:2] == (1, 1)   # one K-step
    if case.name == "mixed_m":
        split, m_chunk, _, _ = kr.het_plan(probs, False)
        # the shallow problem ends inside the first slab
        assert min(p.M for p in probs) <= m_chunk and split > 2
    if case.name == "xcd_pad":
        for bf16 in (False, True):
            lin = kr.het_plan(probs, bf16)[3]
            clu = kr.het_plan(probs, bf16, xcd=True)[3]
            assert (lin, clu) == (31, 33)
            assert clu > lin and clu % 8 != 0       # grid padded past it
            assert (clu + 7) // 8 * 8 == 40
        # odd tile counts on both axes of one problem
        assert any(t[2] % 2 == 1 and t[2] > 1
                   for t in kr.het_tiles(probs, False, True))
    if case.name == "big":
        tiles = kr.het_tiles(probs, True, False, True)
        # every (rn, rk) the 128x128 body runs with ((1, 1) is the 64x64
        # body, which the other cases cover)
        assert {t[:2] for t in tiles} == {(1, 2), (2, 1), (2, 2)}
        assert all(p.M >= 1024 for p in probs)
        for key in ((True, False, False), (True, False, True)):
            split, m_chunk, _, _ = kr.het_plan(probs, *key)
            assert probs[0].M - (split - 1) * m_chunk == 6
    if case.name == "many_tiles":
        assert len(probs) == 12
        assert kr.het_plan(probs, False)[3] == 384
        assert {p.mask for p in probs} == {True, False}


def test_wgrad_case_table_properties():
    """The wgrad tables keep the properties they were chosen for."""
    plans = [(c, bf16, kr.mwgrad_plan(c.M, c.N, c.K, c.nz, bf16))
             for c in kr.MWGRAD_CASES for bf16 in (False, True)]
    # a last slab of one row
    assert any(s > 1 and c.M - (s - 1) * mc == 1
               for c, _, (s, mc, _, _) in plans)
    assert any(c.N == 1 for c in kr.MWGRAD_CASES)
    assert any(p.N == 1 for h in kr.MWGRAD_HET_CASES for p in h.problems)
    assert any(c.lddy and c.lddy % 4 == 0 and c.N >= 64
               for c in kr.MWGRAD_CASES)
    assert any(len({p.M for p in h.problems}) > 1
               for h in kr.MWGRAD_HET_CASES)
    assert any(not p.bias for h in kr.MWGRAD_HET_CASES for p in h.problems)
    # rounding_bound's +32 term is what covers the slab combine
    for name in kr.MWGRAD_ROUNDING_CASES:
        c = kr.mwgrad_case(name)
        for bf16 in (False, True):
            assert kr.mwgrad_plan(c.M, c.N, c.K, c.nz, bf16)[0] <= 32
    for name in kr.MWGRAD_HET_ROUNDING_CASES:
        for bf16 in (False, True):
            assert kr.het_plan(kr.het_case(name).problems, bf16)[0] <= 32
    # no interior-path case with an odd x offset: no caller produces one
    for probs in [c.problems for c in kr.MWGRAD_CASES] + \
            [h.problems for h in kr.MWGRAD_HET_CASES]:
        for p in probs:
            if p.ld_x % 4 == 0 and p.K >= 64 and p.M >= 64:
                assert p.x_off % 4 == 0, p


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in
    float64, so one float64 add and one rounding to fp32 follow."""
    return (a.double() * b.double() + c.double()).float()


def adam_emulate_fp32(p, g, m, v, targ, t, hyper):
    """adam_math / polyak_math of fused.hip in CPU fp32 tensor ops, in
    the order the kernel writes them."""
    f = {k: torch.tensor(x, dtype=torch.float32) for k, x in hyper.items()}
    one = torch.tensor(1.0)
    tt = torch.tensor(float(t))
    bc1 = one - torch.pow(f["b1"], tt)
    bc2 = one - torch.pow(f["b2"], tt)
    gi = _fma32(f["wd"], p, g)
    mi = _fma32(f["b1"], m, (one - f["b1"]) * gi)
    vi = _fma32(f["b2"], v, ((one - f["b2"]) * gi) * gi)
    pn = p - f["lr"] / bc1 * mi / (torch.sqrt(vi / bc2) + f["eps"])
    tn = None
    if targ is not None:
        tn = f["rho"] * targ + (one - f["rho"]) * pn
    assert pn.dtype == torch.float32 and vi.dtype == torch.float32
    return pn, mi, vi, tn


@pytest.mark.parametrize("wd", [0.0, 2.0 ** -7])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_fp32_emulation_within_half_bounds(step, wd):
    """The bounds the GPU Adam tests assert are fair: a plain fp32
    evaluation in the kernel's order stays under HALF of each."""
    hyper = dict(kr.ADAM_HYPER, wd=wd)
    p, g, m, v, targ = kr.adam_state(20000, step, True, seed=step)
    assert float(g.abs().min()) >= 0.99e-6 and float(g.abs().max()) <= 10.0
    assert float(g.abs().min()) < 1e-5 and float(g.abs().max()) > 1.0
    assert float(p.abs().max()) <= 1 / 16 and float(targ.abs().max()) <= 1 / 16
    assert (step == 1) == (float(m.abs().max()) == 0.0)
    ref = kr.adam_ref(p, g, m, v, targ, step, hyper)
    bounds = kr.adam_bounds(p, g, m, ref, hyper)
    outs = adam_emulate_fp32(p, g, m, v, targ, step, hyper)
    for nm, out, r, b in zip("pmvt", outs, ref, bounds):
        ratio = float(((out.double() - r).abs() / b).max())
        print(f"adam emulation step={step} wd={wd} {nm}: "
              f"max err/bound = {ratio:.3f}")
        assert ratio <= 0.5, (nm, ratio)
    # the update is visible: a skipped element is off by |u| itself
    u = ref[4]
    assert float((u.abs() / bounds[0]).median()) > 1000
    assert float((u.abs() / bounds[0]).min()) > 4


def test_adam_ref_uses_fp32_hyperparameters():
    """1 - b2 from the fp32-rounded 0.999 differs from the double's by
    1.3e-5 relative: the reference must take the kernel's value."""
    b2 = kr.f32_as_double(0.999)
    assert abs((1 - b2) / (1 - 0.999) - 1) > 1e-5
    p, g, m, v, _ = kr.adam_state(64, 2, False)
    r32 = kr.adam_ref(p, g, m, v, None, 2, kr.ADAM_HYPER)
    assert r32[3] is None
    assert torch.equal(r32[2], b2 * v.double()
                       + (1 - b2) * g.double() * g.double())


def test_adam_t_layout_properties():
    n = kr.ADAM_T_N
    assert n % 256 != 0 and n > 1024 * 256
    slabs = [(off, N * K) for off, N, K in kr.ADAM_T_DENSE]
    off, (oc, ic, kh, kw) = kr.ADAM_T_CONV
    slabs.append((off, oc * ic * kh * kw))
    assert kh * kw == 6
    at = 0
    for off, sz in slabs:                  # sorted, with gaps, inside n
        assert off > at
        at = off + sz
    assert at < n
    assert slabs[-1][0] >= 1024 * 256      # in the grid-stride wrap


def test_conv_geometry_table_properties():
    """The geometry table keeps the properties it was chosen for."""
    for geom in kr.CONV_GEOMS:
        B, IC, IH, IW, OC, KH, KW, S = geom
        OH, OW = kr.conv_out_hw(geom)
        assert OH >= 1 and OW >= 1
        assert (B * OH * OW) % 64 != 0
    assert all(kr.conv_is_known(g) for g in kr.CONV_KNOWN)
    assert not any(kr.conv_is_known(g) for g in kr.CONV_FALLBACK)
    ks = [g[1] * g[5] * g[6] for g in kr.CONV_GEOMS]
    assert any(k % 4 != 0 for k in ks)
    assert any(k % 4 == 0 and k % 16 != 0 for k in ks)
    assert any(g[4] > 64 for g in kr.CONV_GEOMS)
    assert any(g[1] > 64 for g in kr.CONV_GEOMS)
    assert any(g[5] != g[6] for g in kr.CONV_GEOMS)
    assert any(g[5] < g[7] for g in kr.CONV_GEOMS)
    assert sum(bool(kr.uncovered(g).any()) for g in kr.CONV_GEOMS) >= 3
    # ragged wgrad slab plan: M = 126 -> 64 + 62
    assert any(g[0] * kr.conv_out_hw(g)[0] * kr.conv_out_hw(g)[1] == 126
               for g in kr.CONV_GEOMS)


# ---------------------------------------------------------------------------
# Philox4x32-10 and the draws derived from it
# ---------------------------------------------------------------------------

# (counter c0..c3, key k0 k1, output): the known-answer vectors published
# with the generator (Random123, kat_vectors, philox4x32 10 rounds)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    clo, chi = ctr[0] | (ctr[1] << 32), ctr[2] | (ctr[3] << 32)
    seed = key[0] | (key[1] << 32)
    assert kr.philox4x32(seed, chi, clo) == want
    got = kr.philox4x32_np(seed, chi, np.array([clo], dtype=np.uint64))
    assert got.dtype == np.uint32 and tuple(int(x) for x in got[0]) == want
    # the signed form an int64 argument carries is the same key
    assert kr.philox4x32(kr.as_i64(seed), kr.as_i64(chi), clo) == want
    # nine rounds is another function
    assert kr.philox4x32(seed, chi, clo, rounds=9) != want


def test_philox_vectorised_matches_scalar():
    """Across the 32-bit boundary of the subsequence index, with high
    counter and key words set."""
    seed, chi, clo0 = 0x9e3779b97f4a7c15, 2 ** 40 + 3, 2 ** 32 - 3
    rows = kr.philox_rows(seed, chi, 7, clo0)
    for i in range(7):
        assert tuple(int(x) for x in rows[i]) == \
            kr.philox4x32(seed, chi, clo0 + i)
    assert len({tuple(r) for r in rows.tolist()}) == 7


def test_uniform32_edges():
    u = kr.uniform32(np.array([0, 0xffffffff, 0x7fffffff], dtype=np.uint32))
    assert u.dtype == np.float32
    assert float(u[0]) == 2.0 ** -32
    assert float(u[1]) == 1.0            # 2^32 - 1 rounds to 2^32; never > 1
    assert float(u[2]) == 0.5
    c, s, r = kr.box_muller64(u[1:2], u[0:1])
    assert float(r[0]) == 0.0 and float(c[0]) == 0.0 and float(s[0]) == 0.0


def test_draw_index_and_shifts():
    x, y = 0xdeadbeef, 0x01234567
    u = (x << 32) | y
    big = 2 ** 32 + 12345                # a ring larger than one word
    assert kr.draw_index(x, y, big) == u % big
    assert kr.draw_index(x, y, big) != kr.draw_index(0, y, big)
    assert kr.draw_index(x, y, 1) == 0
    xs = np.array([x, 0, 0xffffffff], dtype=np.uint32)
    ys = np.array([y, 5, 0xffffffff], dtype=np.uint32)
    for size in (1, 48, 5000, big):
        got = kr.draw_index(xs, ys, size)
        assert got.dtype == np.int64
        assert got.tolist() == [((int(a) << 32) | int(b)) % size
                                for a, b in zip(xs, ys)]
    z, w = 0x00070003, 0xfffe0009
    assert kr.draw_shifts(z, w, 0).tolist() == [0, 0, 0, 0]
    assert kr.draw_shifts(z, w, 1).tolist() == \
        [7 % 3 - 1, 3 % 3 - 1, 0xfffe % 3 - 1, 9 % 3 - 1]
    assert kr.draw_shifts(z, w, 4).tolist() == \
        [7 - 4, 3 - 4, 0xfffe % 9 - 4, 0 - 4]
    both = kr.draw_shifts(np.array([z, w]), np.array([w, z]), 4)
    assert both.shape == (2, 4) and both[1].tolist() == \
        [0xfffe % 9 - 4, -4, 3, -1]


def test_per_targets_formula():
    x = np.array([0, 0xffffffff, 0x80000000], dtype=np.uint32)
    u = kr.per_targets(x, 6.0, 3)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, float(np.float32(2 - 2.0 ** -24) * 2), 5.0]


def test_box_muller_cap_is_fair():
    """numpy's fp32 evaluation of the kernels' formula stays inside a
    tenth of NOISE_CAP * max(1, R) against float64, on the draws the GPU
    tests use and on the edge uniforms."""
    words = [kr.philox_rows(s, c, 4096) for s, c in ((0, 1), (11, 41),
                                                     (12345, 2 ** 33))]
    w = np.concatenate(words)
    edge = np.array([0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffeff,
                     0xffffff00, 0xffffffff], dtype=np.uint32)
    u0 = np.concatenate([kr.uniform32(w[:, 0]), kr.uniform32(w[:, 2]),
                         np.repeat(kr.uniform32(edge), len(edge))])
    u1 = np.concatenate([kr.uniform32(w[:, 1]), kr.uniform32(w[:, 3]),
                         np.tile(kr.uniform32(edge), len(edge))])
    c64, s64, r = kr.box_muller64(u0, u1)
    c32, s32 = kr.box_muller32(u0, u1)
    cap = kr.NOISE_CAP * np.maximum(1.0, r)
    worst = max(float((np.abs(c32 - c64) / cap).max()),
                float((np.abs(s32 - s64) / cap).max()))
    print("fp32 Box-Muller worst err / cap:", worst)
    assert worst <= 0.1
    # a structural error is O(1): sin for cos, swapped uniforms
    assert float(np.abs(s64 - c64).mean()) > 0.5
    c_sw, _, _ = kr.box_muller64(u1, u0)
    assert float(np.abs(c_sw - c64).mean()) > 0.5


# ---------------------------------------------------------------------------
# head / loss / temperature bounds are fair to a correct fp32 evaluation
# ---------------------------------------------------------------------------

def _worst(name, out, ref, bound):
    ratio = float(((out.double() - ref).abs() / bound).max())
    print(f"{name}: fp32 emulation max err/bound = {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("case", kr.TG_CASES, ids=kr.tg_id)
def test_tg_bounds_are_fair(case):
    R, A = case[:2]
    hl = kr.tg_hl(case)
    eps = kr.noise_eps32(kr.TG_SEED, kr.TG_CTR, R, A)
    args = (kr.TG_ACT_LIMIT, kr.TG_LO, kr.TG_HI)
    ref = kr.tg_ref(hl, eps, *args)
    bnd = kr.tg_fwd_bounds(hl, eps, *args)
    out = kr.tg_fwd_f32(hl, eps, *args)
    for nm, o, r, b in zip(("pi", "prob", "logp"), out, ref, bnd):
        assert _worst(f"tg_fwd {kr.tg_id(case)} {nm}", o, r, b) <= 0.5, nm
    B = kr.tg_bwd_rows(case)
    dxa, dxb, col = kr.tg_bwd_operands(case, B)
    da, db = dxa[:, col:col + A], dxb[:, col:col + A]
    prob = out[1]
    for second in (db, None):
        a = (hl, prob, da, second, 0.2, B) + args
        ref_b, bnd_b = kr.tg_bwd_ref(*a), kr.tg_bwd_bounds(*a)
        out_b = kr.tg_bwd_f32(*a)
        for nm, o, r, b in zip(("dmu", "dls"), out_b, ref_b, bnd_b):
            assert _worst(f"tg_bwd {kr.tg_id(case)} {nm}", o, r, b) <= 0.5
        # the clamp mask: zero strictly outside, alive at both ends
        raw = hl[:B, A:]
        outside = (raw < kr.TG_LO) | (raw > kr.TG_HI)
        assert bool((ref_b[1][outside] == 0).all())
        assert bool((ref_b[1][~outside] != 0).all())


def test_tg_inputs_reach_every_branch():
    """Between them the cases hold every special log_std next to every
    special mu, x = -2 prob above 20 (the softplus cut) and saturated
    tanh."""
    seen_ls, seen_mu, cut, sat = set(), set(), 0, 0
    for case in kr.TG_CASES:
        R, A = case[:2]
        hl = kr.tg_hl(case)
        seen_mu |= set(hl[:, :A].reshape(-1).tolist())
        seen_ls |= set(hl[:, A:].reshape(-1).tolist())
        eps = kr.noise_eps32(kr.TG_SEED, kr.TG_CTR, R, A)
        _, prob, _ = kr.tg_ref(hl, eps, kr.TG_ACT_LIMIT, kr.TG_LO, kr.TG_HI)
        cut += int((-2 * prob > 20).sum())
        sat += int((prob.abs() > 10).sum())
        assert case[4] + A <= case[3] and case[6] + A <= case[5]
        assert 0 <= case[2] <= R
    assert set(kr.TG_MU) <= seen_mu
    assert set(torch.tensor(kr.tg_raw_log_std()).tolist()) <= seen_ls
    assert cut >= 10 and sat >= 20
    big = kr.tg_hl(kr.TG_CASES[-1])
    A = kr.TG_CASES[-1][1]
    pairs = {(m, s) for m, s in zip(big[:, :A].reshape(-1).tolist(),
                                    big[:, A:].reshape(-1).tolist())}
    want = {(m, s) for m in kr.TG_MU
            for s in torch.tensor(kr.tg_raw_log_std()).tolist()}
    assert want <= pairs


@pytest.mark.parametrize("B", kr.LOSS_B_FUSED + [kr.LOSS_B_UNFUSED])
def test_loss_bounds_are_fair(B):
    h = kr.QLOSS_HYPER
    for h2 in kr.LOSS_H2:
        t = kr.qloss_inputs(B, h2)
        assert B == 1 or set(t["done"].tolist()) == {0.0, 1.0}
        ref, bnd = kr.qloss_ref(t, B, h["alpha"], h["gamma"], h["scale"])
        out = kr.qloss_f32(t, B, h["alpha"], h["gamma"], h["scale"])
        for k in ref:
            assert _worst(f"qloss B={B} h2={h2} {k}", out[k], ref[k],
                          bnd[k]) <= 0.5, k
        t = kr.piloss_inputs(B, h2)
        tie = t["q1"] == t["q2"]
        assert int(tie.sum()) == -(-B // 3)
        assert int((t["q1"] < t["q2"]).sum()) == -(-(B - 1) // 3)
        ref, bnd = kr.piloss_ref(t, B, h["alpha"])
        out = kr.piloss_f32(t, B, h["alpha"])
        for k in ref:
            if k.startswith("dq"):
                assert torch.equal(out[k].double(),
                                   ref[k].float().double()), k
            else:
                assert _worst(f"piloss B={B} h2={h2} {k}", out[k], ref[k],
                              bnd[k] + 1e-300) <= 0.5, k
        assert bool((ref["dq1"][tie] == -0.5 / B).all())
        assert bool((ref["dq2"][tie] == -0.5 / B).all())


def test_alpha_bounds_are_fair():
    """Five chained fp32 steps, each held against the float64 step from
    the same fp32 state."""
    assert kr.f32_as_double(0.001) != 1.0 - kr.f32_as_double(0.999)
    assert abs(kr.f32_as_double(0.001) / (1.0 - kr.f32_as_double(0.999))
               - 1.0) > 1e-5
    la, m, v = float(torch.tensor(kr.ALPHA_LOG0)), 0.0, 0.0
    zero_g = 0
    for step, ml in enumerate(kr.ALPHA_MEAN_LOGP):
        a = (la, m, v, step, ml, kr.ALPHA_TARGET_ENTROPY, kr.ALPHA_LR)
        ref = kr.alpha_ref(*a)
        bnd = kr.alpha_bounds(m, v, ref)
        out = kr.alpha_f32(*a)
        zero_g += ref[4] == 0.0
        for nm, o, r, b in zip(("log_alpha", "m", "v"), out, ref, bnd):
            ratio = abs(o - r) / b
            print(f"alpha step {step + 1} {nm}: err/bound = {ratio:.3f}")
            assert ratio <= 0.5, (step, nm)
        if step > 0 and ref[4] != 0.0:
            # the update is visible against its own bound
            assert abs(ref[3]) > 100 * bnd[0]
        la, m, v = out
    assert zero_g == 1


# ---------------------------------------------------------------------------
# the autograd-path kernels: bounds are fair to a plain fp32 evaluation in
# each kernel's order (half of every bound), and the eager fallbacks of
# ops/functional.py meet the same references on the same inputs
# ---------------------------------------------------------------------------

TGH_VARIANTS = [(False, True), (False, False), (True, True), (True, False)]


def _held(name, out, ref, bound, share=1.0):
    bound = torch.as_tensor(bound, dtype=torch.float64) + 1e-300
    r = _worst(name, out, ref, bound)
    assert r <= share, (name, r)


def _eager_head(mu, ls, eps, lo, hi, det, wl, dpi=None, dlogp=None):
    """Fo's CPU head under autograd: (pi, logp, dmu, dls)."""
    from torch_actor_critic_amd.ops import functional as Fo
    mu = mu.clone().requires_grad_(True)
    ls = ls.clone().requires_grad_(True)
    pi, logp = Fo.tanh_gauss_head(mu, ls, eps, kr.TG_ACT_LIMIT, lo, hi,
                                  det, wl)
    assert (logp is None) == (not wl)
    if dpi is None:
        return pi.detach(), logp, None, None
    seed = (pi * dpi).sum()
    if wl:
        seed = seed + (logp * dlogp).sum()
    seed.backward()
    # deterministic without logp: log_std reaches no output, its gradient
    # is None where the kernel writes zeros
    dls = ls.grad if ls.grad is not None else torch.zeros_like(ls)
    return pi.detach(), logp, mu.grad, dls


@pytest.mark.parametrize("clamp", kr.TGH_CLAMPS, ids=kr.tgh_id)
@pytest.mark.parametrize("case", kr.TGH_CASES, ids=kr.tgh_id)
def test_tgh_bounds_are_fair_and_eager_head_meets_them(case, clamp):
    B, A = case
    lo, hi = clamp
    al = kr.TG_ACT_LIMIT
    mu, ls, eps = kr.tgh_inputs(B, A, lo, hi)
    dpi, dlogp = kr.tgh_bwd_operands(B, A)
    for det, wl in TGH_VARIANTS:
        tag = f"tgh {B}x{A} lo={lo} det={det} logp={wl}"
        a = (mu, ls, eps, al, lo, hi, det, wl)
        ref, bnd, out = kr.tgh_ref(*a), kr.tgh_fwd_bounds(*a), \
            kr.tgh_fwd_f32(*a)
        assert (ref[3] is None) == (not wl) and (out[3] is None) == (not wl)
        names = ("pi", "prob", "ls_c") + (("logp",) if wl else ())
        for nm, o, r, b in zip(names, out, ref, bnd):
            _held(f"{tag} {nm}", o, r, b, 0.5)
        assert torch.equal(out[2].double(), ref[2])
        if det:
            assert torch.equal(out[1], mu)
        b_args = (mu, ls, eps, out[1], out[2], dpi, dlogp, al, lo, hi, det,
                  wl)
        ref_b, bnd_b = kr.tgh_bwd_ref(*b_args), kr.tgh_bwd_bounds(*b_args)
        out_b = kr.tgh_bwd_f32(*b_args)
        for nm, o, r, b in zip(("dmu", "dls"), out_b, ref_b, bnd_b):
            _held(f"{tag} {nm}", o, r, b, 0.5)
        outside = (ls < lo) | (ls > hi)
        assert bool((ref_b[1][outside] == 0).all())
        # the eager fallback: same reference, same bounds
        pi_e, logp_e, dmu_e, dls_e = _eager_head(mu, ls, eps, lo, hi, det,
                                                 wl, dpi, dlogp)
        _held(f"{tag} eager pi", pi_e, ref[0], bnd[0])
        if wl:
            _held(f"{tag} eager logp", logp_e.detach(), ref[3], bnd[3])
        # autograd differentiates the Jacobian term as written,
        # d/dprob (prob + softplus(-2 prob)) = 1 - 2 sigmoid(-2 prob),
        # where the kernel takes the closed form tanh(prob): near
        # prob = 0 the difference cancels, so its error is absolute in
        # |dlogp|: twice sigmoid's (one exp, a sum and a quotient) plus
        # the roundings of the difference and of autograd's two
        # accumulations into d prob, each on terms of at most |dlogp|
        extra = torch.zeros(B, 1, dtype=torch.float64)
        if wl:
            extra = dlogp.double().abs()[:, None] \
                * (2 * (kr.LIBM_TOL["exp"] + 2 * kr.U) + 4 * kr.U)
        se = torch.zeros_like(extra) if det \
            else (out[2].double().exp() * eps.double()).abs()
        _held(f"{tag} eager dmu", dmu_e, ref_b[0], bnd_b[0] + extra)
        _held(f"{tag} eager dls", dls_e, ref_b[1], bnd_b[1] + extra * se)
        assert bool((dls_e[outside] == 0).all())


def test_tgh_inputs_reach_the_small_std_cases():
    """At the models' default clamp every |mu| in {0.5, 3, 12} meets every
    log_std at or below -16 with |eps| >= 1, and there std * eps is lost
    in mu + std * eps (prob == mu) although eps is not 0."""
    lo, hi = kr.TGH_CLAMPS[1]
    assert lo == -20.0
    mu, ls, eps = kr.tgh_inputs(*kr.TGH_CASES[-1], lo, hi)
    small = ls.clamp(lo, hi) <= kr.TGH_SMALL_LS
    assert bool((eps[small].abs() >= 1).all())
    pairs = {(abs(m), s) for m, s in zip(mu[small].tolist(),
                                        ls[small].tolist())}
    inside = float(torch.nextafter(torch.tensor(lo), torch.tensor(0.0)))
    for m in (0.5, 3.0, 12.0):
        for s in (lo - 1.0, lo, inside, -18.0, -16.0):
            assert (m, s) in pairs, (m, s)
    assert set(kr.tgh_raw_log_std(lo, hi)) <= set(ls.reshape(-1).tolist())
    prob = mu + ls.clamp(lo, hi).exp() * eps
    lost = (ls.clamp(lo, hi) <= -18.0) & (mu.abs() >= 3.0) \
        & (eps.abs() < 4.0)
    assert int(lost.sum()) > 100 and bool((prob[lost] == mu[lost]).all())
    assert bool((eps[lost] != 0).all())
    # the three small cases cover the special values between them
    for c in kr.TGH_CLAMPS:
        seen = set()
        for B, A in kr.TGH_CASES[:-1]:
            assert A <= 64
            seen |= set(kr.tgh_inputs(B, A, *c)[1].reshape(-1).tolist())
        assert set(torch.tensor(kr.tgh_raw_log_std(*c)).tolist()) <= seen


@pytest.mark.parametrize("case", kr.TGH_CASES[1:], ids=kr.tgh_id)
def test_logp_rebuilt_by_subtraction_misses_at_the_default_clamp(case):
    """What the default-clamp cases are for: logp with the noise rebuilt
    as (prob - mu) / std, the head's earlier order, stays inside the bound
    at the clamp of -5 and misses it by orders of magnitude at -20."""
    B, A = case
    al = kr.TG_ACT_LIMIT
    for (lo, hi), misses in zip(kr.TGH_CLAMPS, (False, True)):
        mu, ls, eps = kr.tgh_inputs(B, A, lo, hi)
        a = (mu, ls, eps, al, lo, hi, False, True)
        ref, bnd = kr.tgh_ref(*a), kr.tgh_fwd_bounds(*a)
        old = kr.tgh_logp_by_subtraction_f32(mu, ls, eps, lo, hi)
        r = _worst(f"subtractive logp {B}x{A} lo={lo}", old, ref[3], bnd[3])
        assert (r > 100.0) if misses else (r <= 1.0), (lo, r)


def _q_leaves(t):
    """(q1, q2) as leaves for the eager losses under autograd."""
    return (t["q1"].clone().requires_grad_(True),
            t["q2"].clone().requires_grad_(True))


@pytest.mark.parametrize("B", kr.FLAT_LOSS_B)
def test_flat_loss_bounds_are_fair_and_eager_losses_meet_them(B):
    from torch_actor_critic_amd.ops import functional as Fo
    h = kr.QLOSS_HYPER
    hs = (h["alpha"], h["gamma"], h["scale"])
    t = kr.flat_qloss_inputs(B)
    if B >= 15:
        fr = torch.tensor(kr.FLAT_DONE_FRACTIONS, dtype=torch.float32)
        assert set(fr.tolist()) | {0.0, 1.0} <= set(t["done"].tolist())
        assert int((t["q1t"] == t["q2t"]).sum()) >= B // 3
        frac = (t["done"] != 0) & (t["done"] != 1)
        assert int(frac.sum()) >= B // 5
    ref, bnd = kr.qloss_ref(t, B, *hs)
    out = kr.qloss_f32(t, B, *hs)
    for k in ("loss", "dq1", "dq2"):
        _held(f"flat qloss B={B} {k}", out[k], ref[k], bnd[k], 0.5)
    q1, q2 = _q_leaves(t)
    loss = Fo.sac_q_loss(q1, q2, t["q1t"], t["q2t"], t["logp"], t["rew"],
                         t["done"], *hs)
    loss.backward()
    _held(f"eager qloss B={B} loss", loss.detach(), ref["loss"], bnd["loss"])
    _held(f"eager qloss B={B} dq1", q1.grad, ref["dq1"], bnd["dq1"])
    _held(f"eager qloss B={B} dq2", q2.grad, ref["dq2"], bnd["dq2"])

    t = kr.piloss_inputs(B, 1, seed=31)
    ref, bnd = kr.piloss_ref(t, B, h["alpha"])
    out = kr.piloss_f32(t, B, h["alpha"])
    _held(f"flat piloss B={B} loss", out["loss"], ref["loss"], bnd["loss"],
          0.5)
    for k in ("dq1", "dq2"):
        assert torch.equal(out[k].double(), ref[k].float().double()), k
    dl = kr.piloss_dlogp_ref(B, h["alpha"])
    assert abs(dl - 0.2 / B) <= kr.E32 * dl
    q1, q2 = _q_leaves(t)
    logp = t["logp"].clone().requires_grad_(True)
    loss = Fo.sac_pi_loss(q1, q2, logp, h["alpha"])
    loss.backward()
    _held(f"eager piloss B={B} loss", loss.detach(), ref["loss"],
          bnd["loss"])
    _held(f"eager piloss B={B} dq1", q1.grad, ref["dq1"], bnd["dq1"])
    _held(f"eager piloss B={B} dq2", q2.grad, ref["dq2"], bnd["dq2"])
    _held(f"eager piloss B={B} dlogp", logp.grad,
          torch.full((B,), dl, dtype=torch.float64), kr.U * dl)
    tie = t["q1"] == t["q2"]
    assert bool(tie.any())
    assert torch.equal(q1.grad[tie], q2.grad[tie])


@pytest.mark.parametrize("rho", kr.POLYAK_RHO)
def test_polyak_bound_is_fair_and_eager_polyak_meets_it(rho):
    from torch_actor_critic_amd.ops import functional as Fo
    for n in kr.POLYAK_N[:-1] + [20000]:
        targ, src = kr.polyak_inputs(n)
        ref, bnd = kr.polyak_ref(targ, src, rho)
        _held(f"polyak n={n} rho={rho}", kr.polyak_f32(targ, src, rho), ref,
              bnd, 0.5)
        got, s0 = targ.clone(), src.clone()
        Fo.polyak_(got, src, rho)
        _held(f"eager polyak n={n} rho={rho}", got, ref, bnd)
        assert torch.equal(src, s0)
        if rho in (0.0, 1.0):
            assert torch.equal(got, src if rho == 0.0 else targ)
        # a dropped element (target left as it was) is far outside
        if rho == 0.995 and n > 100:
            assert float(((targ.double() - ref).abs() / bnd).median()) > 1000


@pytest.mark.parametrize("wd", kr.ADAM_FLAT_WD)
@pytest.mark.parametrize("step", kr.ADAM_FLAT_STEPS)
def test_adam_flat_bounds_are_fair_and_eager_adam_meets_them(step, wd):
    """adam_kernel's order (no FMA) under half of adam_bounds, weight decay
    included, and the eager branch of Fo.adam_step_ under the bounds."""
    from torch_actor_critic_amd.ops import functional as Fo
    hyper = dict(kr.ADAM_HYPER, wd=wd)
    p, g, m, v, _ = kr.adam_state(20000, step, False, seed=step)
    ref = kr.adam_ref(p, g, m, v, None, step, hyper)
    bounds = kr.adam_bounds(p, g, m, ref, hyper)
    outs = kr.adam_flat_f32(p, g, m, v, step, hyper)
    for nm, o, r, b in zip("pmv", outs, ref, bounds):
        _held(f"adam_flat step={step} wd={wd} {nm}", o, r, b, 0.5)
    pe, me, ve = p.clone(), m.clone(), v.clone()
    ctr = torch.tensor([step - 1])
    Fo.adam_step_(pe, g, me, ve, ctr, hyper["lr"], hyper["b1"], hyper["b2"],
                  hyper["eps"], wd)
    assert int(ctr) == step
    for nm, o, r, b in zip("pmv", (pe, me, ve), ref, bounds):
        _held(f"eager adam step={step} wd={wd} {nm}", o, r, b)
    if wd:
        # the decay is visible in m: without it m is off by (1 - b1) wd p
        no_wd = kr.adam_ref(p, g, m, v, None, step, dict(hyper, wd=0.0))
        assert float(((no_wd[1] - ref[1]).abs() / bounds[1]).median()) > 100
