"""The live GEMM (fused.hip: mgemm, mgemm_r1, transpose_multi) against
float64 references built by kernel_refs.py.

Exact tests use small-integer operands: every partial sum is an integer
below 2^24 and every operand is bf16-exact (test_kernel_refs.py proves
that on the CPU for each case), so the output must equal the reference
bit for bit in fp32 AND bf16 mode, for any split-K / NT / slab plan.
Rounding tests use randn operands and the derived bound
kernel_refs.rounding_bound.  Every output buffer starts filled with a
sentinel so a stray or missing write shows."""

import os

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["fp32", "bf16"]


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


def _set_dtype(dtype):
    from torch_actor_critic_amd.ops import functional as Fo
    Fo.set_compute_dtype(dtype)


def _dev(t):
    return None if t is None else t.to(DEV)


def _sentinel(*shape):
    return torch.full(shape, kr.SENTINEL, device=DEV)


def run_mgemm(ext, o):
    """Launch one mgemm for the operands `o`; returns the [M, ldy]
    output buffers (sentinel outside the logical [M, N] block)."""
    c = o.case
    lda, ldy = c.lda or c.K, c.ldy or c.N
    if c.x_offs:
        src = o.xs[0].to(DEV)                   # ONE shared source
        xs = [src] * c.nz
    else:
        xs = [x.to(DEV) for x in o.xs]
    ys = [_sentinel(c.M, ldy) for _ in range(c.nz)]
    ext.mgemm(xs, [w.to(DEV) for w in o.ws], [_dev(b) for b in o.bs], ys,
              [_dev(m) for m in o.masks], c.M, c.N, c.K, lda, ldy, c.relu,
              [x.to(DEV) for x in o.xs2], [w.to(DEV) for w in o.ws2],
              [_dev(m) for m in o.masks2], c.K2, c.x_off, 0,
              list(c.x_offs))
    torch.cuda.synchronize()
    return [y.cpu() for y in ys]


def _assert_pad_untouched(name, y, N):
    pad = y[:, N:]
    assert bool((pad == kr.SENTINEL).all()), \
        f"{name}: {int((pad != kr.SENTINEL).sum())} stray writes in the pad"


def _check_plan(case, bf16):
    split, k_chunk, nt = kr.mgemm_plan(case.M, case.N, case.K, case.nz,
                                       bf16, case.K2 > 0)
    if case.expect == "split":
        assert split > 1, "case no longer reaches split-K"
    elif case.expect == "nosplit":
        assert split == 1
    elif case.expect == "nt":
        assert nt == 2 and split == 1
    return split, k_chunk, nt


def _skip_if_nt_overridden(case):
    if case.expect == "nt" and "TAC_AMD_MGEMM_NT" in os.environ:
        pytest.skip("TAC_AMD_MGEMM_NT overrides the NT plan under test")


# ---------------------------------------------------------------------------
# mgemm
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", kr.MGEMM_CASES, ids=lambda c: c.name)
def test_mgemm_exact(ext, case, dtype):
    _skip_if_nt_overridden(case)
    _check_plan(case, dtype == "bf16")
    o = kr.mgemm_operands(case, "int")
    refs = kr.mgemm_ref(o)
    _set_dtype(dtype)
    ys = run_mgemm(ext, o)
    for z, (y, (ref, _)) in enumerate(zip(ys, refs)):
        name = f"{case.name}[{z}] {dtype}"
        msg = kr.describe_mismatch(y[:, :case.N].double(), ref)
        assert msg == "", f"{name}: {msg}"
        _assert_pad_untouched(name, y, case.N)


def test_mgemm_splitk_gate_matches_unsplit(ext):
    """K = 1023 (gate off) and K = 1030 (split) share their first 1023
    columns: zeroing the last 7 must give the same output bits."""
    c_on = next(c for c in kr.MGEMM_CASES if c.name == "splitk_ragged")
    c_off = next(c for c in kr.MGEMM_CASES if c.name == "splitk_gate_off")
    assert kr.mgemm_plan(c_on.M, c_on.N, c_on.K, 1, False, False)[0] > 1
    assert kr.mgemm_plan(c_off.M, c_off.N, c_off.K, 1, False, False)[0] == 1
    o_on = kr.mgemm_operands(c_on, "int")
    o_on.xs[0][:, c_off.K:] = 0
    o_off = kr.mgemm_operands(c_off, "int")
    o_off.xs[0] = o_on.xs[0][:, :c_off.K].contiguous()
    o_off.ws[0] = o_on.ws[0][:, :c_off.K].contiguous()
    o_off.bs[0] = o_on.bs[0]
    for dtype in DTYPES:
        _set_dtype(dtype)
        assert torch.equal(run_mgemm(ext, o_on)[0], run_mgemm(ext, o_off)[0])


@pytest.mark.parametrize("case", kr.MGEMM_ROUNDING_CASES,
                         ids=lambda c: c.name)
def test_mgemm_rounding(ext, case):
    _skip_if_nt_overridden(case)
    o = kr.mgemm_operands(case, "randn", seed=7)
    outs = {}
    for dtype in DTYPES:
        bf16 = dtype == "bf16"
        _check_plan(case, bf16)
        (ref, s_abs), = kr.mgemm_ref(o, bf16=bf16)
        _set_dtype(dtype)
        y, = run_mgemm(ext, o)
        outs[dtype] = y
        err = (y.double() - ref).abs()
        bound = kr.rounding_bound(case.k_red, s_abs)
        ratio = float((err / bound).max())
        print(f"mgemm rounding {case.name} {dtype}: max err/bound = "
              f"{ratio:.4f}")
        assert bool((err <= bound).all()), (case.name, dtype, ratio)
    assert not torch.equal(outs["fp32"], outs["bf16"]), \
        "bf16 mode gave fp32 bits: the dtype flag did not take effect"


# ---------------------------------------------------------------------------
# mgemm_r1
# ---------------------------------------------------------------------------

def run_r1(ext, o, ldy):
    nz = len(o.cols)
    ys = [_sentinel(o.M, ldy) for _ in range(nz)]
    ext.mgemm_r1([t.to(DEV) for t in o.cols], [t.to(DEV) for t in o.rows],
                 [t.to(DEV) for t in o.ws], ys,
                 [t.to(DEV) for t in o.masks], o.M, o.N, o.K, ldy)
    torch.cuda.synchronize()
    return [y.cpu() for y in ys]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nz", kr.R1_NZ)
@pytest.mark.parametrize("M,N,K", kr.R1_SHAPES)
def test_mgemm_r1_exact(ext, M, N, K, nz, dtype):
    o = kr.r1_operands(M, N, K, nz, "int")
    refs = kr.r1_ref(o)
    _set_dtype(dtype)
    for ldy in (N, N + 5):
        ys = run_r1(ext, o, ldy)
        for z, (y, (ref, _)) in enumerate(zip(ys, refs)):
            name = f"r1 {M}x{N}x{K} nz={nz} ldy={ldy} [{z}] {dtype}"
            msg = kr.describe_mismatch(y[:, :N].double(), ref)
            assert msg == "", f"{name}: {msg}"
            _assert_pad_untouched(name, y, N)


def test_mgemm_r1_rounding(ext):
    M, N, K = 70, 130, 129
    o = kr.r1_operands(M, N, K, 1, "randn", seed=7)
    outs = {}
    for dtype in DTYPES:
        (ref, s_abs), = kr.r1_ref(o, bf16=dtype == "bf16")
        _set_dtype(dtype)
        y, = run_r1(ext, o, N)
        outs[dtype] = y
        err = (y.double() - ref).abs()
        bound = kr.rounding_bound(K, s_abs)
        ratio = float((err / bound).max())
        print(f"mgemm_r1 rounding {dtype}: max err/bound = {ratio:.4f}")
        assert bool((err <= bound).all()), (dtype, ratio)
    assert not torch.equal(outs["fp32"], outs["bf16"])


def test_mgemm_r1_host_gates(ext):
    """The documented host checks raise before anything is launched."""
    M, N, K = 5, 3, 8
    o = kr.r1_operands(M, N, K, 1, "int")
    col, w, mask = o.cols[0].to(DEV), o.ws[0].to(DEV), o.masks[0].to(DEV)
    row_buf = torch.zeros(K + 4, device=DEV)
    y = _sentinel(M, N)

    def call(cols, rows, ws, ys, masks, ldy=N):
        ext.mgemm_r1(cols, rows, ws, ys, masks, M, N, K, ldy)

    call([col], [row_buf[:K]], [w], [y], [mask])           # the valid form
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call([col], [row_buf[1:K + 1]], [w], [y], [mask])  # misaligned view
    with pytest.raises(RuntimeError, match="row"):
        call([col], [row_buf[:K + 4]], [w], [y], [mask])   # wrong numel
    with pytest.raises(RuntimeError, match="col"):
        call([row_buf[:M + 1]], [row_buf[:K]], [w], [y], [mask])
    with pytest.raises(RuntimeError, match="mask"):
        call([col], [row_buf[:K]], [w], [y], [mask[:-1]])
    with pytest.raises(RuntimeError, match="y "):
        call([col], [row_buf[:K]], [w], [y], [mask], ldy=N + 1)
    with pytest.raises(RuntimeError, match="1..4 problems"):
        call([col] * 5, [row_buf[:K]] * 5, [w] * 5, [y] * 5, [mask] * 5)
    with pytest.raises(RuntimeError, match="1..4 problems"):
        call([col], [row_buf[:K]], [w], [y], [])           # masks required
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# transpose_multi
# ---------------------------------------------------------------------------

def _transpose_layers():
    g = torch.Generator()
    g.manual_seed(5)
    ws = []
    # 12 layers in one launch, dense and conv interleaved
    shapes = kr.TRANSPOSE_DENSE + kr.TRANSPOSE_CONV
    for i in range(12):
        ws.append(torch.randn(shapes[(i * 3) % len(shapes)], generator=g))
    return ws


def test_transpose_multi_mixed_launch(ext):
    ws = _transpose_layers()
    assert {w.dim() for w in ws} == {2, 4}
    assert {tuple(w.shape) for w in ws} == set(kr.TRANSPOSE_DENSE
                                                + kr.TRANSPOSE_CONV)
    refs = [kr.transpose_ref(w) for w in ws]
    # one spare row after each output to catch stray writes
    bufs = [_sentinel(r.shape[0] + 1, r.shape[1]) for r in refs]
    blocks = [1 if w.dim() == 2 else w.shape[2] * w.shape[3] for w in ws]
    ext.transpose_multi([w.to(DEV) for w in ws], bufs, blocks)
    torch.cuda.synchronize()
    for i, (buf, ref) in enumerate(zip(bufs, refs)):
        out = buf.cpu()
        msg = kr.describe_mismatch(out[:-1].double(), ref.double())
        assert msg == "", f"layer {i} {tuple(ws[i].shape)}: {msg}"
        assert bool((out[-1] == kr.SENTINEL).all()), f"layer {i}: stray"


def test_transpose_multi_default_block_is_dense(ext):
    ws = [w for w in _transpose_layers() if w.dim() == 2][:3]
    wts = [_sentinel(w.shape[1], w.shape[0]) for w in ws]
    ext.transpose_multi([w.to(DEV) for w in ws], wts)
    for w, wt in zip(ws, wts):
        assert torch.equal(wt.cpu(), w.t())


def test_transpose_multi_13_layers_raises(ext):
    w = torch.zeros(2, 3, device=DEV)
    wt = torch.zeros(3, 2, device=DEV)
    with pytest.raises(RuntimeError):
        ext.transpose_multi([w] * 13, [wt] * 13)
    ext.transpose_multi([w] * 12, [wt] * 12)
    torch.cuda.synchronize()
