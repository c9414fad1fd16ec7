"""CPU check of the precondition behind the exact GPU kernel tests
(test_gpu_mgemm.py, test_gpu_conv_exact.py): for the integer operands of
every case table, the float64 reference is integer-valued and both
max|ref| and the absolute-value contraction sum|a||b| stay below 2^24.
Then every partial sum any kernel can form, in fp32 or from bf16-rounded
operands, is exact, and bit equality is the right assertion."""

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
