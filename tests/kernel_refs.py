"""Float64 CPU references, operand generators and case tables shared by
test_gpu_mgemm.py, test_gpu_conv_exact.py, conv_lds_worker.py,
test_gpu_wgrad.py, wgrad_env_worker.py, test_gpu_adam_t.py,
test_gpu_philox.py, test_gpu_heads_losses.py, test_gpu_autograd_kernels.py,
test_gpu_dense_autograd.py and the CPU precondition test
(test_kernel_refs.py).  Plain helper module, not a conftest.

Two operand kinds:
 * "int":   small integers stored as fp32 (x, w, dy, rank-1 factors in
            {-3..3}, bias in {-8..8}, masks in {-1, 0, 1}).  Every
            product and partial sum is an integer far below 2^24 and
            every operand is exact in bf16, so a correct kernel equals
            the float64 reference bit for bit in both compute dtypes,
            whatever its summation order, split or slab plan.
 * "randn": gaussian operands for the rounding tests, checked against
            rounding_bound().
"""

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import math

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 12345.0
EXACT_LIMIT = float(2 ** 24)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def int_tensor(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def operand(g, shape, kind):
    if kind == "int":
        return int_tensor(g, shape, -3, 3)
    return torch.randn(tuple(shape), generator=g)


def bias_operand(g, n, kind):
    if kind == "int":
        return int_tensor(g, (n,), -8, 8)
    return torch.randn(n, generator=g)


def mask_operand(g, shape):
    """{-1, 0, 1}: the kernels test `> 0`, so 0 and -1 must both mask."""
    return int_tensor(g, shape, -1, 1)


def bf16_round(t):
    return t.bfloat16().float()


def rounding_bound(k_red, s_abs):
    """Elementwise |out - ref| bound for a length-k_red fp32 dot product
    in any order (Higham's gamma_n), doubled for non-RNE accumulation
    inside an MFMA; the +32 covers slab combines and the bias add."""
    return 2.0 * (k_red + 32) * 2.0 ** -24 * s_abs + 1e-30


def describe_mismatch(out64, ref):
    """'' when bit-equal, else count + first mismatching index."""
    if out64.shape != ref.shape:
        return f"shape {tuple(out64.shape)} != {tuple(ref.shape)}"
    if torch.equal(out64, ref):
        return ""
    bad = (out64 != ref) | (out64.isnan() != ref.isnan())
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {ref.numel()} elements differ; first at "
            f"{idx}: got {out64[idx].item()!r}, want {ref[idx].item()!r}")


# ---------------------------------------------------------------------------
# mgemm
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class MgCase:
    name: str
    M: int
    N: int
    K: int
    nz: int = 1
    bias: Tuple[bool, ...] = (True,)     # per problem
    relu: bool = False
    lda: Optional[int] = None            # None: K (contiguous A)
    x_off: int = 0
    x_offs: Tuple[int, ...] = ()         # per-problem offsets, ONE source
    ldy: Optional[int] = None            # None: N
    mask: bool = False
    K2: int = 0                          # > 0: SUM2 second operand pair
    expect: str = ""                     # "split", "nosplit", "nt" or ""

    @property
    def k_red(self):
        return self.K + self.K2


def _b(n, *on):
    return tuple(i in on for i in range(n))


MGEMM_CASES = [
    MgCase("tile_tails", 5, 3, 7),
    MgCase("m1", 1, 70, 17),
    MgCase("n1", 64, 1, 262),
    MgCase("bf16_interior_then_edge", 64, 64, 300),
    MgCase("odd_ld_edge", 100, 23, 393),
    MgCase("two_tiles_relu_bias", 70, 130, 129, relu=True),
    MgCase("two_tiles_nobias", 70, 130, 129, bias=(False,)),
    MgCase("strided_a_y", 70, 40, 33, lda=80, x_off=11, ldy=48),
    MgCase("x_offs", 70, 40, 33, nz=3, bias=(True,) * 3, lda=120,
           x_offs=(0, 40, 87)),
    MgCase("four_problems", 33, 65, 48, nz=4, bias=_b(4, 0, 2)),
    MgCase("masked", 70, 33, 130, bias=(False,), mask=True),
    # lda % 4 == 0 and a 16-byte-aligned offset: the masked bf16 interior
    # path (the contiguous case above has lda = 130, the edge path)
    MgCase("masked_strided", 70, 33, 130, bias=(False,), mask=True,
           lda=152, x_off=12),
    MgCase("sum2", 70, 33, 40, K2=17),
    MgCase("sum2_masked", 70, 33, 40, K2=17, mask=True, bias=(False,)),
    MgCase("sum2_nz2", 70, 33, 40, K2=17, nz=2, bias=_b(2, 1)),
    MgCase("sum2_nz2_masked", 70, 33, 40, K2=17, nz=2, bias=_b(2, 0),
           mask=True),
    MgCase("splitk_ragged", 5, 70, 1030, relu=True, expect="split"),
    MgCase("splitk_ragged_nz2_ldy", 5, 70, 1030, relu=True, nz=2,
           bias=(True, True), ldy=75, expect="split"),
    MgCase("splitk_gate_off", 5, 70, 1023, relu=True, expect="nosplit"),
    MgCase("splitk_masked", 64, 64, 1100, bias=(False,), mask=True,
           expect="split"),
    MgCase("nt2_odd_tiles", 1024, 130, 20, expect="nt"),
    MgCase("nt2_sum2_masked", 1024, 130, 20, K2=9, mask=True,
           bias=(False,), expect="nt"),
]

MGEMM_ROUNDING_CASES = [
    MgCase("plain", 70, 130, 129),
    MgCase("splitk", 5, 70, 1030, expect="split"),
    MgCase("nt2", 1024, 130, 20, expect="nt"),
]


def mgemm_plan(M, N, K, nz, bf16, sum2):
    """The host launch plan of fused.hip::mgemm: (split, k_chunk, nt)."""
    bk = 128 if bf16 else 16
    gx, gy = -(-M // 64), -(-N // 64)
    tiles = gx * gy * nz
    split = 1
    if not sum2 and K >= 1024 and tiles < 128:
        kchunks = -(-K // bk)
        split = max(1, min(kchunks, (256 + tiles - 1) // tiles, 16))
    k_chunk = -(-(-(-K // split)) // bk) * bk
    split = -(-K // k_chunk)
    nt = 2 if (split == 1 and M >= 1024 and gy >= 2) else 1
    return split, k_chunk, nt


@dataclass
class MgOps:
    """CPU operands of one mgemm launch.  xs / masks are the full
    storage tensors ([M, lda]); view(t, z) is the logical [M, K] block."""
    case: MgCase
    xs: List[torch.Tensor] = field(default_factory=list)
    ws: List[torch.Tensor] = field(default_factory=list)
    bs: List[Optional[torch.Tensor]] = field(default_factory=list)
    masks: List[Optional[torch.Tensor]] = field(default_factory=list)
    xs2: List[torch.Tensor] = field(default_factory=list)
    ws2: List[torch.Tensor] = field(default_factory=list)
    masks2: List[Optional[torch.Tensor]] = field(default_factory=list)

    def off(self, z):
        c = self.case
        return c.x_offs[z] if c.x_offs else c.x_off

    def view(self, t, z):
        return t[:, self.off(z):self.off(z) + self.case.K]


def mgemm_operands(case, kind, seed=0):
    g = _gen(1000 + seed)
    c = case
    lda = c.lda or c.K
    o = MgOps(case)
    shared = operand(g, (c.M, lda), kind) if c.x_offs else None
    for z in range(c.nz):
        o.xs.append(shared if shared is not None
                    else operand(g, (c.M, lda), kind))
        o.ws.append(operand(g, (c.N, c.K), kind))
        o.bs.append(bias_operand(g, c.N, kind) if c.bias[z] else None)
        o.masks.append(mask_operand(g, (c.M, lda)) if c.mask else None)
        if c.K2:
            o.xs2.append(operand(g, (c.M, c.K2), kind))
            o.ws2.append(operand(g, (c.N, c.K2), kind))
            o.masks2.append(mask_operand(g, (c.M, c.K2)) if c.mask
                            else None)
    return o


def mgemm_ref(o, bf16=False):
    """Per problem: (float64 reference [M, N], S_abs [M, N])."""
    c = o.case
    rnd = bf16_round if bf16 else (lambda t: t)
    out = []
    for z in range(c.nz):
        a = rnd(o.view(o.xs[z], z)).double()
        if c.mask:
            a = a * (o.view(o.masks[z], z) > 0)
        w = rnd(o.ws[z]).double()
        y = a @ w.t()
        s = a.abs() @ w.abs().t()
        if c.K2:
            a2 = rnd(o.xs2[z]).double()
            if c.mask:
                a2 = a2 * (o.masks2[z] > 0)
            w2 = rnd(o.ws2[z]).double()
            y = y + a2 @ w2.t()
            s = s + a2.abs() @ w2.abs().t()
        if o.bs[z] is not None:
            y = y + o.bs[z].double()
            s = s + o.bs[z].double().abs()
        if c.relu:
            y = y.clamp_min(0.0)
        out.append((y, s))
    return out


# ---- rank-1 A operand -----------------------------------------------------

R1_SHAPES = [(5, 3, 7), (70, 130, 129), (64, 64, 256)]
R1_NZ = [1, 2, 4]


@dataclass
class R1Ops:
    M: int
    N: int
    K: int
    cols: List[torch.Tensor]
    rows: List[torch.Tensor]
    ws: List[torch.Tensor]
    masks: List[torch.Tensor]


def r1_operands(M, N, K, nz, kind, seed=0):
    g = _gen(2000 + seed)
    o = R1Ops(M, N, K, [], [], [], [])
    for _ in range(nz):
        o.cols.append(operand(g, (M,), kind))
        o.rows.append(operand(g, (K,), kind))
        o.ws.append(operand(g, (N, K), kind))
        o.masks.append(mask_operand(g, (M, K)))
    return o


def r1_ref(o, bf16=False):
    """((col ⊗ row) * (mask > 0)) @ w^T.  The product is formed in fp32
    (as the kernel does) and, in bf16 mode, rounded once after that."""
    out = []
    for col, row, w, m in zip(o.cols, o.rows, o.ws, o.masks):
        a = col[:, None] * row[None, :]            # fp32 product
        if bf16:
            a, w = bf16_round(a), bf16_round(w)
        a = a.double() * (m > 0)
        out.append((a @ w.double().t(), a.abs() @ w.double().abs().t()))
    return out


# ---- transpose_multi ------------------------------------------------------

TRANSPOSE_DENSE = [(1, 1), (65, 63), (130, 7)]
TRANSPOSE_CONV = [(5, 3, 2, 3), (65, 4, 3, 3)]


def transpose_ref(w):
    if w.dim() == 2:
        return w.t().contiguous()
    oc, ic, kh, kw = w.shape
    return w.permute(1, 0, 2, 3).reshape(ic, oc * kh * kw).contiguous()


# ---------------------------------------------------------------------------
# conv
# ---------------------------------------------------------------------------

# (B, IC, IH, IW, OC, KH, KW, S).  M = B*OH*OW is never a multiple of 64
# and a 64-row tile spans images.
CONV_KNOWN = [
    (3, 3, 20, 24, 5, 8, 8, 4),      # K = 192
    (3, 5, 11, 13, 70, 4, 4, 2),     # OC > 64; uncovered last row/col
    (3, 70, 7, 9, 33, 3, 3, 1),      # IC > 64; K = 630, K % 4 != 0
]
CONV_FALLBACK = [
    (2, 3, 9, 11, 5, 3, 3, 2),       # K = 27: K % 4 != 0, stride classes
    (2, 2, 9, 8, 4, 2, 3, 1),        # KH != KW; K = 12: %4 == 0, %16 != 0
    (2, 2, 10, 10, 3, 5, 5, 3),      # (IH - KH) % S != 0
    (2, 3, 7, 7, 4, 1, 1, 2),        # KH < S: whole stride classes are 0
    (2, 3, 8, 10, 5, 2, 2, 1),       # M = 126: wgrad slabs of 64 and 62
]
# OH = OW = 1, M = 1 < 64 (one wgrad slab).  8/8/4 is the compiled
# family, so this runs the TK = 8 instantiation at its smallest image.
CONV_ONE_PIXEL = [(1, 1, 8, 8, 1, 8, 8, 4)]
CONV_GEOMS = CONV_KNOWN + CONV_FALLBACK + CONV_ONE_PIXEL


def conv_id(geom):
    return "x".join(str(v) for v in geom)


def conv_out_hw(geom):
    B, IC, IH, IW, OC, KH, KW, S = geom
    return (IH - KH) // S + 1, (IW - KW) // S + 1


def conv_is_known(geom):
    KH, KW, S = geom[5:]
    return KH == KW and (KH, S) in ((8, 4), (4, 2), (3, 1))


@dataclass
class ConvOps:
    geom: tuple
    x: torch.Tensor
    w: torch.Tensor
    b: torch.Tensor
    dy: torch.Tensor
    mask: torch.Tensor


def conv_operands(geom, kind, seed=0):
    B, IC, IH, IW, OC, KH, KW, S = geom
    OH, OW = conv_out_hw(geom)
    g = _gen(3000 + seed)
    return ConvOps(geom,
                   operand(g, (B, IC, IH, IW), kind),
                   operand(g, (OC, IC, KH, KW), kind),
                   bias_operand(g, OC, kind),
                   operand(g, (B, OC, OH, OW), kind),
                   mask_operand(g, (B, OC, OH, OW)))


def conv_fwd_ref(x, w, b, S, relu):
    """(float64 reference, S_abs)."""
    x, w = x.double(), w.double()
    b = b.double() if b is not None else None
    y = F.conv2d(x, w, b, stride=S)
    s = F.conv2d(x.abs(), w.abs(), b.abs() if b is not None else None,
                 stride=S)
    return (y.clamp_min(0.0) if relu else y), s


def conv_bwd_ref(x, w, dy, S, mask=None):
    """float64 autograd (dx, dw, db) of conv2d(x, w, b) under the upstream
    gradient dy * (mask > 0)."""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    dy = dy.double()
    if mask is not None:
        dy = dy * (mask > 0)
    y = F.conv2d(x, w, b, stride=S)
    return torch.autograd.grad(y, (x, w, b), dy)


def conv_bwd_abs(x, w, dy, S, mask=None):
    """S_abs of the three gradients: each is bilinear with non-negative
    coefficients, so the same contraction over absolute values."""
    if mask is not None:
        dy = dy * (mask > 0)
    return conv_bwd_ref(x.abs(), w.abs(), dy.abs(), S)


# ---- fused B=1 conv trunk (8/4/3 kernels, ReLU after each layer) ---------

# 1x36x36 with strides 4/1/1: layer 2's output (64*5*5 = 1600 floats) is
# larger than the input frame (1296), so it cannot reuse the frame's slot
# while layer 1's output, stored right behind the frame, is still read.
TRUNK_SMALL = ((1, 36, 36), (32, 64, 64), (4, 1, 1))
# Same property at 1x84x84 (frame 7056, layer 2 output 64*17*17 = 18496).
# Here layer 2 has 40 work items for the kernel's 16 waves, so a wave's
# later items read layer 1's output after earlier items have written
# theirs: an overlap shows in the result.  At 36x36 each wave has one
# item and reads all it needs before it writes, so an overlap only races
# with the other waves' reads and can go unnoticed.
TRUNK_WIDE = ((1, 84, 84), (32, 64, 64), (4, 1, 1))
TRUNK_CASES = [TRUNK_SMALL, TRUNK_WIDE]


def trunk_operands(vis, filters, seed=0):
    """x in {-3..3}, weights in {-1, 0, 1}, biases in {-8..8}: small enough
    that all three layers stay exact (checked in test_kernel_refs.py)."""
    g = _gen(4000 + seed)
    x = int_tensor(g, vis, -3, 3)
    ws, bs = [], []
    c = vis[0]
    for f, k in zip(filters, (8, 4, 3)):
        ws.append(int_tensor(g, (f, c, k, k), -1, 1))
        bs.append(int_tensor(g, (f,), -8, 8))
        c = f
    return x, ws, bs


def trunk_ref(x, ws, bs, strides):
    """Per layer (float64 activation, S_abs); the last one is the output."""
    a = x.double().unsqueeze(0)
    out = []
    for w, b, s in zip(ws, bs, strides):
        a, s_abs = conv_fwd_ref(a, w, b, s, relu=True)
        out.append((a, s_abs))
    return out


def uncovered(geom):
    """Boolean [IH, IW]: input pixels that no window covers."""
    B, IC, IH, IW, OC, KH, KW, S = geom
    OH, OW = conv_out_hw(geom)
    cov = torch.zeros(IH, IW, dtype=torch.bool)
    for oy in range(OH):
        for ox in range(OW):
            cov[oy * S:oy * S + KH, ox * S:ox * S + KW] = True
    return ~cov


# ---------------------------------------------------------------------------
# dense wgrad (fused.hip: mwgrad, mwgrad_het, mwgrad_het_adam)
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class WgProb:
    """One wgrad problem: dW[N, K] = dYeff^T X, db[N] = column sums."""
    M: int
    N: int
    K: int
    lddy: Optional[int] = None           # None: N (contiguous dy and mask)
    ldx: Optional[int] = None            # None: K
    x_off: int = 0
    mask: bool = False
    bias: bool = True

    @property
    def ld_dy(self):
        return self.lddy or self.N

    @property
    def ld_x(self):
        return self.ldx or self.K


@dataclass(frozen=True)
class WgCase:
    """One mwgrad launch: nz <= 2 problems of one shape and layout."""
    name: str
    M: int
    N: int
    K: int
    nz: int = 1
    lddy: Optional[int] = None
    ldx: Optional[int] = None
    x_off: int = 0
    mask: bool = False
    bias: Tuple[bool, ...] = (True,)     # per problem
    # expected host plan per dtype: (split, rows of the last slab), the
    # string "split" (any split > 1) or None (not pinned)
    expect: Tuple = (None, None)         # (fp32, bf16)

    @property
    def problems(self):
        return [WgProb(self.M, self.N, self.K, self.lddy, self.ldx,
                       self.x_off, self.mask, self.bias[z])
                for z in range(self.nz)]


MWGRAD_CASES = [
    # all edges, one K-step
    WgCase("tile_tails", 5, 3, 7, expect=((1, 5), (1, 5))),
    # single row, two n-tiles
    WgCase("m1", 1, 70, 17, expect=((1, 1), (1, 1))),
    # one-row last slab
    WgCase("m17", 17, 70, 33, expect=((2, 1), (1, 17))),
    # width-1 critic output layer
    WgCase("n1", 64, 1, 262, expect=((4, 16), (1, 64))),
    # ragged last slab, mask, twin critics
    WgCase("ragged_masked_nz2", 70, 33, 130, nz=2, mask=True,
           bias=(True, True), expect=((5, 6), (2, 6))),
    # lddy % 4 == 0, ldx % 4 == 0 and a 16-byte-aligned offset: the bf16
    # float4 interior path for dy, mask and x
    WgCase("interior_strided", 130, 70, 130, nz=2, lddy=72, ldx=136,
           x_off=4, mask=True, bias=(True, True),
           expect=((9, 2), (3, 2))),
    # the scalar path with an odd offset
    WgCase("edge_strided", 70, 40, 33, lddy=48, ldx=80, x_off=11,
           mask=True, expect=("split", "split")),
    # db optional per problem
    WgCase("nobias_mixed", 70, 33, 40, nz=2, bias=(True, False)),
    # 384 tiles: un-split loop over several K-steps with a ragged tail
    # (fp32: 9 K-steps of 16 rows, bf16: 3 of 64; 130 = 2 * 64 + 2)
    WgCase("unsplit_multi_step", 130, 512, 1536, nz=2, bias=(True, True),
           expect=((1, 130), (1, 130))),
]

MWGRAD_ROUNDING_CASES = ["ragged_masked_nz2", "interior_strided"]


def mwgrad_case(name):
    return next(c for c in MWGRAD_CASES if c.name == name)


@dataclass(frozen=True)
class HetCase:
    name: str
    problems: Tuple[WgProb, ...]


MWGRAD_HET_CASES = [
    # the batch-64 phase table: fp32 split 4, bf16 un-split single K-step
    HetCase("phase64", (WgProb(64, 70, 23, ldx=32, x_off=5),
                        WgProb(64, 6, 64, mask=True),
                        WgProb(64, 1, 70))),
    # per-problem M: fp32 split 5, bf16 split 2; the M = 5 problem must
    # get exact zeros from every later slab
    HetCase("mixed_m", (WgProb(70, 70, 130, mask=True),
                        WgProb(5, 33, 40, lddy=36, ldx=48, x_off=3),
                        WgProb(64, 1, 70, bias=False))),
    HetCase("single", (WgProb(5, 3, 7),)),
    # odd tile counts on both axes: padded 2x2 cluster slots; 31 linear
    # and 33 clustered blocks, so the padded grid (40) overshoots
    HetCase("xcd_pad", (WgProb(70, 130, 70, mask=True),
                        WgProb(70, 3, 7),
                        WgProb(70, 200, 330, ldx=336, x_off=4))),
    # M >= 1024 with every (rn, rk) combination under RNRK, ragged 6-row
    # last slab
    HetCase("big", (WgProb(1030, 130, 200, mask=True),
                    WgProb(1030, 70, 130),
                    WgProb(1030, 1, 140),
                    WgProb(1030, 130, 40, lddy=132, mask=True))),
    # 384 tiles: un-split, several K-steps, 12 problems (the MAXW limit)
    HetCase("many_tiles", (WgProb(130, 250, 500, mask=True),)
            + tuple(WgProb(130, 256, 512, mask=(i % 2 == 1))
                    for i in range(11))),
]

MWGRAD_HET_ROUNDING_CASES = ["phase64", "mixed_m"]

# (split, m_chunk, chunks, blk) keyed by (case, bf16, xcd, rnrk) where the
# plan is pinned; asserted on the CPU (test_kernel_refs.py)
HET_PLANS = {
    ("phase64", False, False, False): (4, 16, 4, 5),
    ("phase64", True, False, False): (1, 64, 1, 5),
    ("mixed_m", False, False, False): (5, 16, 5, 9),
    ("mixed_m", True, False, False): (2, 64, 2, 9),
    ("single", False, False, False): (1, 16, 1, 1),
    ("single", True, False, False): (1, 64, 1, 1),
    ("xcd_pad", False, False, False): (5, 16, 5, 31),
    ("xcd_pad", True, False, False): (2, 64, 2, 31),
    ("xcd_pad", False, True, False): (5, 16, 5, 33),
    ("xcd_pad", True, True, False): (2, 64, 2, 33),
    ("big", False, False, False): (13, 80, 65, 24),
    ("big", True, False, False): (9, 128, 17, 24),
    ("big", True, False, True): (17, 64, 17, 12),
    ("many_tiles", False, False, False): (1, 144, 9, 384),
    ("many_tiles", True, False, False): (1, 192, 3, 384),
}


def het_case(name):
    return next(c for c in MWGRAD_HET_CASES if c.name == name)


def _cdiv(a, b):
    return -(-a // b)


def mwgrad_plan(M, N, K, nz, bf16):
    """The host launch plan of fused.hip::mwgrad:
    (split, m_chunk, chunks, tiles)."""
    bk = 64 if bf16 else 16
    chunks = _cdiv(M, bk)
    tiles = _cdiv(N, 64) * _cdiv(K, 64) * nz
    split = max(1, min(chunks, (384 + tiles - 1) // tiles))
    m_chunk = _cdiv(_cdiv(M, split), bk) * bk
    split = _cdiv(M, m_chunk)
    return split, m_chunk, chunks, tiles


def het_tiles(problems, bf16, xcd=False, rnrk=False):
    """Per problem (rn, rk, bx, bk_t, slots) as mwgrad_het_impl lays the
    block table out; slots counts the padded 2x2 cluster slots under xcd."""
    out = []
    for p in problems:
        big = rnrk and bf16 and p.M >= 1024
        rn = 2 if big and p.N >= 128 else 1
        rk = 2 if big and p.K >= 128 else 1
        bx = _cdiv(p.N, 64 * rn)
        bk_t = _cdiv(p.K, 64 * rk)
        if xcd:
            cn, ck = min(2, bx), min(2, bk_t)
            slots = _cdiv(bx, cn) * _cdiv(bk_t, ck) * cn * ck
        else:
            slots = bx * bk_t
        out.append((rn, rk, bx, bk_t, slots))
    return out


def het_plan(problems, bf16, xcd=False, rnrk=False):
    """The host launch plan of fused.hip::mwgrad_het_impl / het_split:
    (split, m_chunk, chunks, blk).  rnrk only applies to mwgrad_het (the
    Adam-carrying launch and mwgrad_het_adam_split ignore it)."""
    bk = 64 if bf16 else 16
    blk = sum(t[4] for t in het_tiles(problems, bf16, xcd, rnrk))
    max_m = max(p.M for p in problems)
    chunks = _cdiv(max_m, bk)
    split = max(1, min(chunks, (384 + blk - 1) // blk, 64))
    m_chunk = _cdiv(_cdiv(max_m, split), bk) * bk
    split = _cdiv(max_m, m_chunk)
    return split, m_chunk, chunks, blk


@dataclass
class WgOps:
    """CPU operands of one wgrad problem.  dy / mask / x are the full
    storage tensors ([M, lddy], [M, lddy], [M, ldx]); dy_v / mask_v / x_v
    the logical [M, N], [M, N], [M, K] blocks."""
    prob: WgProb
    dy: torch.Tensor
    mask: Optional[torch.Tensor]
    x: torch.Tensor

    @property
    def dy_v(self):
        return self.dy[:, :self.prob.N]

    @property
    def mask_v(self):
        return None if self.mask is None else self.mask[:, :self.prob.N]

    @property
    def x_v(self):
        p = self.prob
        return self.x[:, p.x_off:p.x_off + p.K]


def wgrad_operands(problems, kind, seed=0):
    """One WgOps per problem.  The pad columns of a strided operand hold
    ordinary operand values, so a read outside the logical block shows."""
    g = _gen(5000 + seed)
    out = []
    for p in problems:
        out.append(WgOps(p,
                         operand(g, (p.M, p.ld_dy), kind),
                         mask_operand(g, (p.M, p.ld_dy)) if p.mask
                         else None,
                         operand(g, (p.M, p.ld_x), kind)))
    return out


def wgrad_ref(dy, x, mask, bf16=False):
    """(dw64 [N, K], db64 [N], S_dw, S_db) of one wgrad problem from the
    logical dy [M, N], x [M, K] and mask [M, N] (or None):
    dyeff = rnd(dy) * (mask > 0), dw = dyeff^T @ rnd(x), db = dyeff.sum(0)
    in float64; S_* are the same contractions over absolute values.
    In bf16 mode db sums the bf16-ROUNDED dy: the kernel reads the column
    sums back from the staged (rounded, masked) LDS tile, not from global
    memory."""
    rnd = bf16_round if bf16 else (lambda t: t)
    dyeff = rnd(dy).double()
    if mask is not None:
        dyeff = dyeff * (mask > 0)
    xr = rnd(x).double()
    return (dyeff.t() @ xr, dyeff.sum(0),
            dyeff.abs().t() @ xr.abs(), dyeff.abs().sum(0))


def wgrad_refs(ops, bf16=False):
    return [wgrad_ref(o.dy_v, o.x_v, o.mask_v, bf16) for o in ops]


# ---------------------------------------------------------------------------
# Adam (+ polyak target) as adam_math / polyak_math compute it
# ---------------------------------------------------------------------------

ADAM_HYPER = dict(lr=2.0 ** -10, b1=0.9, b2=0.999, eps=1e-8, wd=0.0,
                  rho=0.995)


def f32_as_double(v):
    """A Python float as the kernel receives it: rounded to fp32, widened."""
    return float(torch.tensor(v, dtype=torch.float32).double())


def adam_ref(p, g, m, v, targ, t, hyper):
    """Float64 Adam step t on fp32 inputs.  Every hyperparameter is taken
    as the kernel receives it (rounded to fp32, then widened): 0.999f
    differs from 0.999 by 1.3e-5 relative in 1 - b2, which a reference
    built from Python doubles would show as an error of the kernel.
    Returns (p, m, v, targ, u): the new state and the update term u
    (p_new = p - u); targ is None when no target is given."""
    h = {k: f32_as_double(x) for k, x in hyper.items()}
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gi = h["wd"] * p + g
    mn = h["b1"] * m + (1.0 - h["b1"]) * gi
    vn = h["b2"] * v + (1.0 - h["b2"]) * gi * gi
    bc1 = 1.0 - h["b1"] ** float(t)
    bc2 = 1.0 - h["b2"] ** float(t)
    u = h["lr"] / bc1 * mn / ((vn / bc2).sqrt() + h["eps"])
    pn = p - u
    tn = None
    if targ is not None:
        tn = h["rho"] * targ.double() + (1.0 - h["rho"]) * pn
    return pn, mn, vn, tn, u


def ulp32(t64):
    """Spacing of fp32 at |t| (float64 tensor in, float64 out)."""
    a = t64.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf")))
            - a).double()


def adam_bounds(p, g, m, ref, hyper):
    """Elementwise bounds on |out - adam_ref| for (p, m, v, targ) from the
    fp32 inputs p, g, m and ref = adam_ref(...):
      m: three rounded operations on the terms of the sum,
      v: three rounded operations, relative to v itself,
      p: one final rounding plus the update's relative error (dominated
         by the cancellation in 1 - powf(b2, t) at small t),
      targ: two roundings plus the same update error."""
    h = {k: f32_as_double(x) for k, x in hyper.items()}
    pn, mn, vn, tn, u = ref
    e = 2.0 ** -24
    bm = 4 * e * (h["b1"] * m.double().abs() + (1.0 - h["b1"])
                  * (h["wd"] * p.double().abs() + g.double().abs()))
    bv = 8 * e * vn
    bp = ulp32(pn) + 1e-4 * u.abs()
    bt = None if tn is None else 2 * ulp32(tn) + 1e-4 * u.abs()
    return bp, bm, bv, bt


def adam_state(n, step, with_targ, seed=0, g=None):
    """fp32 (p, g, m, v, targ) for an Adam test: |p|, |targ| <= 1/16 so the
    final subtraction's ulp does not hide the update, |g| log-uniform in
    [1e-6, 10] unless given, m = v = 0 at step 1 and non-zero after.

    After step 1 the state keeps |m| >= |g| / 4 and v >= g^2 / 4, as a
    running average of gradients of this size has.  That is also the
    range in which a plain fp32 evaluation provably stays within HALF of
    adam_bounds (the fairness condition test_kernel_refs.py asserts): the
    error of m is at most 2^-24 * (|m'| + 2 (1 - b1)|gi|), one rounding
    of the result, one of the product and one of gi, which is below
    2 * 2^-24 * (b1|m| + (1 - b1)|gi|) once b1|m| >= (1 - b1)|gi|, i.e.
    |m| >= |gi| / 9.  With |m| << |g| the three roundings can reach 3 of
    the bound's 4 units (2.05 was measured on 20000 elements), still
    inside the bound but not inside its half."""
    gen = _gen(6000 + seed)
    p = (torch.rand(n, generator=gen) * 2 - 1) / 16
    targ = (torch.rand(n, generator=gen) * 2 - 1) / 16 if with_targ else None
    if g is None:
        mag = 10.0 ** (torch.rand(n, generator=gen) * 7 - 6)
        sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
        g = (mag * sign).float()
    if step > 1:
        scale = g.abs().clamp_min(1e-3)
        msign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
        m = scale * msign * (torch.rand(n, generator=gen) + 0.25)
        v = scale * scale * (torch.rand(n, generator=gen) + 0.25)
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v, targ


# adam_t flat layout: two dense slabs and one conv slab with bias gaps; n
# is no multiple of 256 and above 1024 * 256, so the kernel's grid-stride
# loop (at most 1024 blocks of 256 threads) wraps for the first threads,
# and the conv slab lies in the wrapped part.
ADAM_T_N = 262144 + 777
ADAM_T_DENSE = [(64, 70, 33), (64 + 70 * 33 + 70, 130, 257)]   # (off, N, K)
ADAM_T_CONV = (262400, (5, 3, 2, 3))                 # (off, [OC,IC,kh,kw])


# ---------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
# 3", SC'11) and the draws the kernels derive from it
# ---------------------------------------------------------------------------
#
# One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
#     (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,
#      lo(M0 * c0))
# with the 32x32 -> 64 bit products split into high and low words; after
# every round the key advances by the Weyl constants (W0, W1).  Ten rounds.

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85     # golden ratio, sqrt(3) - 1
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
NOISE_KEY = 0x517CC1B727220A95     # xor-ed into the seed by the noise draws


def as_i64(v):
    """A 64-bit pattern as the signed integer an int64 argument takes."""
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def philox4x32(seed, chi, clo, rounds=10):
    """Philox4x32 on Python ints.  The kernels' packing: counter words
    c0, c1 = low, high of clo; c2, c3 = low, high of chi; key words
    k0, k1 = low, high of seed.  Returns the four output words."""
    seed, chi, clo = seed & _M64, chi & _M64, clo & _M64
    c0, c1, c2, c3 = clo & _M32, clo >> 32, chi & _M32, chi >> 32
    k0, k1 = seed & _M32, seed >> 32
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _M32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _M32)
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def philox4x32_np(seed, chi, clo, rounds=10):
    """philox4x32 over an array of clo (any integer dtype; taken mod 2^64):
    uint32 [n, 4].  Products of two 32-bit words fit uint64 exactly."""
    seed, chi = seed & _M64, chi & _M64
    clo = np.asarray(clo).astype(np.uint64)
    m32, s32 = np.uint64(_M32), np.uint64(32)
    c0, c1 = clo & m32, clo >> s32
    c2 = np.full_like(c0, chi & _M32)
    c3 = np.full_like(c0, chi >> 32)
    k0, k1 = seed & _M32, seed >> 32
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_rows(seed, chi, n, clo0=0):
    """uint32 [n, 4]: the draws of subsequences clo0 .. clo0 + n - 1."""
    clo = (np.arange(n, dtype=np.uint64) + np.uint64(clo0 & _M64))
    return philox4x32_np(seed, chi, clo)


def uniform32(word):
    """(float32(word) + 1f) * 2^-32 in fp32, as the kernels map a word to
    (0, 1]: the conversion rounds to nearest even, so 0xffffffff gives 1."""
    w = np.asarray(word, dtype=np.uint32).astype(np.float32)
    return (w + np.float32(1.0)) * np.float32(2.0 ** -32)


def box_muller64(u0, u1):
    """float64 (R cos, R sin, R) with R = sqrt(-2 ln u0), angle 2 pi u1,
    on fp32 uniforms widened to float64."""
    u0 = np.asarray(u0, dtype=np.float32).astype(np.float64)
    u1 = np.asarray(u1, dtype=np.float32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u0))
    return r * np.cos(2.0 * np.pi * u1), r * np.sin(2.0 * np.pi * u1), r


def box_muller32(u0, u1):
    """The same formula evaluated in numpy fp32: (R cos, R sin)."""
    u0 = np.asarray(u0, dtype=np.float32)
    u1 = np.asarray(u1, dtype=np.float32)
    r = np.sqrt(np.float32(-2.0) * np.log(u0))
    ang = np.float32(6.283185307179586) * u1
    return r * np.cos(ang), r * np.sin(ang)


NOISE_CAP = 5e-5     # |eps_kernel - eps64| <= NOISE_CAP * max(1, R)


def draw_index(x, y, size):
    """((x << 32) | y) % size: the replay slot of one draw (ints or
    arrays; int64 out for arrays)."""
    if isinstance(x, (int, np.integer)) and isinstance(y, (int, np.integer)):
        return ((int(x) << 32) | int(y)) % int(size)
    u = (np.asarray(x).astype(np.uint64) << np.uint64(32)) \
        | np.asarray(y).astype(np.uint64)
    return (u % np.uint64(size)).astype(np.int64)


def draw_shifts(z, w, pad):
    """[..., 4] signed shifts (dy_s, dx_s, dy_n, dx_n) in -pad..pad, the
    order visual_gather_shift_kernel documents: z is the state frame's
    word, w the next-state frame's, 16 bits per axis (high half = y) mod
    2 pad + 1.  VisualBatch.shifts holds these plus pad."""
    z = np.asarray(z).astype(np.int64)
    w = np.asarray(w).astype(np.int64)
    span = 2 * pad + 1
    return np.stack([(z >> 16) % span - pad, (z & 0xffff) % span - pad,
                     (w >> 16) % span - pad, (w & 0xffff) % span - pad],
                    axis=-1)


def per_targets(x, root, B):
    """The stratified targets of per_sample in numpy fp32, no contraction:
    u_j = (j + (x_j >> 8) * 2^-24) * (root / B)."""
    x = np.asarray(x, dtype=np.uint32)
    u01 = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    seg = np.float32(root) / np.float32(B)
    return (np.arange(B, dtype=np.float32) + u01) * seg


def noise_eps64(seed, ctr, R, A):
    """float64 [R, A] noise of tg_fwd2 / tg_eps and its Box-Muller radius:
    element (b, a) draws philox(seed ^ NOISE_KEY, ctr, b * A + a) and uses
    words x, y."""
    w = philox_rows(seed ^ NOISE_KEY, ctr, R * A)
    c, _, r = box_muller64(uniform32(w[:, 0]), uniform32(w[:, 1]))
    return c.reshape(R, A), r.reshape(R, A)


def noise_eps32(seed, ctr, R, A):
    """The same draw through the fp32 formula: fp32 tensor [R, A]."""
    w = philox_rows(seed ^ NOISE_KEY, ctr, R * A)
    c, _ = box_muller32(uniform32(w[:, 0]), uniform32(w[:, 1]))
    return torch.from_numpy(c.reshape(R, A).astype(np.float32))


# ---------------------------------------------------------------------------
# SAC head, loss and temperature kernels (fused.hip: tg_fwd2, tg_bwd2,
# qloss2, piloss2, alpha_update)
# ---------------------------------------------------------------------------
#
# Every reference is float64 on the fp32 inputs with scalars and literals
# taken as the kernel holds them (fp32, widened).  Every bound is first
# order and summed over the operations: a rounded fp32 operation can be
# off by E32 = 2^-24 of the magnitude of its result and is charged
# U = 2 E32; an input's bound is carried through by the magnitude of the
# partial derivative; a libm call f contributes tol[f] relative
# (LIBM_FLOOR on the CPU; on the GPU 4x the measured error of torch's own
# fp32 op, never below the floor); a reduction goes through
# rounding_bound(), which carries its own factor of two.  The factor of
# two in U is what the fairness condition needs: an output that is one or
# two rounded operations on exact inputs reaches the worst case of a
# 2^-24 charge routinely, and a correct fp32 evaluation has to stay under
# HALF the bound (test_kernel_refs.py holds every *_f32 function below,
# the plain fp32 evaluation in the kernel's order, to that).

E32 = 2.0 ** -24
U = 2.0 * E32
LIBM_FLOOR = 2.0 ** -22
LIBM_TOL = dict(exp=LIBM_FLOOR, tanh=LIBM_FLOOR, log1p=LIBM_FLOOR)
LOG_2PI_F = f32_as_double(1.8378770664093453)
TWO_LN2_F = f32_as_double(1.3862943611198906)

TG_ACT_LIMIT, TG_LO, TG_HI = 2.5, -5.0, 2.0
# (R, A, B0, ld0, col0, ld1, col1)
TG_CASES = [
    (2, 1, 1, 3, 1, 2, 0),
    (6, 6, 3, 23, 17, 23, 17),
    (5, 17, 5, 20, 3, 17, 0),          # nothing goes to out1
    (4, 64, 0, 64, 0, 70, 5),          # everything goes to out1
    (130, 33, 64, 40, 7, 50, 0),
]
TG_MU = (-12.0, -3.0, 0.0, 0.5, 12.0)
TG_SEED, TG_CTR = 11, 41           # noise key and device counter


def tg_id(case):
    return "x".join(str(v) for v in case)


def tg_raw_log_std():
    """The raw log_std values every case cycles through: below, at and
    just inside both clamp ends, one interior value, beyond the top."""
    lo = torch.tensor(TG_LO)
    hi = torch.tensor(TG_HI)
    inf = torch.tensor(float("inf"))
    return [TG_LO - 1.0, TG_LO, float(torch.nextafter(lo, inf)), -1.25,
            TG_HI, float(torch.nextafter(hi, -inf)), TG_HI + 3.0]


def tg_hl(case):
    """fp32 hl [R, 2A] = mu | raw log_std.  Seven of every nine elements
    take the next special log_std, five of every eight the next special
    mu (periods 9 and 8 are coprime, so all pairs occur); the rest are
    general floats.  Offsets differ per case so the small cases cover the
    list between them."""
    R, A = case[:2]
    g = _gen(7000 + R * 100 + A)
    i = torch.arange(R * A) + R + A
    mu = torch.randn(R * A, generator=g) * 2
    ls = torch.rand(R * A, generator=g) * 5 - 4
    sp_mu = torch.tensor(TG_MU)
    sp_ls = torch.tensor(tg_raw_log_std())
    km, kl = i % 8, i % 9
    mu = torch.where(km < 5, sp_mu[km.clamp_max(4)], mu)
    ls = torch.where(kl < 7, sp_ls[kl.clamp_max(6)], ls)
    return torch.cat([mu.view(R, A), ls.view(R, A)], 1).contiguous()


def tg_ref(hl, eps, act_limit, lo, hi):
    """float64 (pi, prob, logp) of the tanh-Gaussian head on hl = mu |
    raw log_std and the noise eps.  The Jacobian term is the reference
    project's 2 ln 2 - prob - softplus(-2 prob) as it stands (see
    DEVIATIONS.md)."""
    A = hl.shape[1] // 2
    al, lo, hi = (f32_as_double(v) for v in (act_limit, lo, hi))
    mu, raw = hl[:, :A].double(), hl[:, A:].double()
    eps = eps.double()
    ls = raw.clamp(lo, hi)
    prob = mu + ls.exp() * eps
    pi = prob.tanh() * al
    sp = torch.logaddexp(torch.zeros_like(prob), -2.0 * prob)
    gauss = -0.5 * eps * eps - ls - 0.5 * LOG_2PI_F
    corr = TWO_LN2_F - prob - sp
    return pi, prob, (gauss - corr).sum(1)


def tg_fwd_bounds(hl, eps, act_limit, lo, hi, tol=LIBM_TOL):
    """Elementwise bounds (pi, prob, logp) on |kernel - tg_ref|."""
    A = hl.shape[1] // 2
    al, lo, hi = (f32_as_double(v) for v in (act_limit, lo, hi))
    mu, raw = hl[:, :A].double(), hl[:, A:].double()
    eps = eps.double()
    ls = raw.clamp(lo, hi)
    se = ls.exp() * eps
    prob = mu + se
    b_prob = (tol["exp"] + U) * se.abs() + U * prob.abs()
    t = prob.tanh()
    b_pi = al * (tol["tanh"] * t.abs() + (1 - t * t) * b_prob) \
        + U * (al * t).abs()
    # logp: gauss = ((-eps^2/2) - ls) - log(2 pi)/2, three roundings
    a1 = 0.5 * eps * eps
    a2 = -a1 - ls
    gauss = a2 - 0.5 * LOG_2PI_F
    b_gauss = U * (a1 + a2.abs() + gauss.abs())
    # softplus(x), x = -2 prob: d/dx = sigmoid(x); exp's relative error
    # enters log1p through y / (1 + y) = sigmoid(x); above x = 20 the
    # kernel returns x, short of the truth by log1p(exp(-x)) < 2.1e-9
    x = -2.0 * prob
    sig = torch.sigmoid(x)
    sp = torch.logaddexp(torch.zeros_like(x), x)
    b_sp = 2 * sig * b_prob + tol["exp"] * sig + tol["log1p"] * sp \
        + 2.1e-9 * (x > 20) + 1e-37
    c1 = TWO_LN2_F - prob
    corr = c1 - sp
    b_corr = b_prob + U * c1.abs() + b_sp + U * corr.abs()
    term = gauss - corr
    b_term = b_gauss + b_corr + U * term.abs()
    b_logp = b_term.sum(1) + rounding_bound(A, term.abs().sum(1))
    return b_pi, b_prob, b_logp


def tg_fwd_f32(hl, eps, act_limit, lo, hi):
    """Plain fp32 (pi, prob, logp) in tg_fwd2_kernel's order."""
    A = hl.shape[1] // 2
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    mu, raw = hl[:, :A], hl[:, A:]
    ls = raw.clamp(float(f(lo)), float(f(hi)))
    prob = mu + ls.exp() * eps
    pi = prob.tanh() * f(act_limit)
    x = -2.0 * prob
    sp = torch.where(x > 20.0, x, torch.log1p(torch.exp(x.clamp_max(20.0))))
    gauss = -0.5 * eps * eps - ls - f(0.5) * f(1.8378770664093453)
    corr = f(1.3862943611198906) - prob - sp
    return pi, prob, (gauss - corr).sum(1)


def tg_bwd_operands(case, B):
    """fp32 (dxc, dxc2) slabs [B, ld0] for the backward of a TG case: the
    gradient columns are [col0, col0 + A) with col0 > 0 (ld0 and a column
    offset of at least 1 are taken from the forward case)."""
    R, A, _, ld0, col0 = case[:5]
    g = _gen(7100 + R * 100 + A)
    return (torch.randn(B, ld0 + 1, generator=g),
            torch.randn(B, ld0 + 1, generator=g), col0 + 1)


def tg_bwd_rows(case):
    """Rows the backward runs over: the out0 rows, or all when B0 = 0."""
    return case[2] if case[2] > 0 else case[0]


def tg_bwd_ref(hl, prob, dpi_a, dpi_b, alpha, B, act_limit, lo, hi,
               dl=None, se=None):
    """float64 (dmu, dls) of tg_bwd2 over rows :B.  dpi_a / dpi_b are the
    logical [B, A] gradient blocks (dpi_b may be None), prob the fp32
    pre-squash sample the forward stored, alpha / B the seed of logp.
    The autograd-path kernel (tgh_bwd_ref) passes its own float64 seed
    dl [B, 1] and its own se = std * eps [B, A] instead."""
    A = hl.shape[1] // 2
    al, lo, hi, alpha = (f32_as_double(v) for v in (act_limit, lo, hi, alpha))
    mu, raw = hl[:B, :A].double(), hl[:B, A:].double()
    p = prob[:B].double()
    t = p.tanh()
    if se is None:
        se = p - mu
    dpi = dpi_a.double() + (dpi_b.double() if dpi_b is not None else 0.0)
    if dl is None:
        dl = alpha / B
    dp = dpi * al * (1 - t * t)
    g_mu = dp + dl * t
    g_ls = dp * se + dl * (se * t - 1.0)
    mask = (raw >= lo) & (raw <= hi)
    return g_mu, g_ls * mask


def tg_bwd_bounds(hl, prob, dpi_a, dpi_b, alpha, B, act_limit, lo, hi,
                  tol=LIBM_TOL, dl=None, se=None, b_se=None):
    """Elementwise bounds (dmu, dls).  dp = dpi * act_limit * (1 - t^2)
    cancels to zero at saturation, so its error is carried as an absolute
    one: t's error times 2|t|, plus the roundings of t^2 and of 1 - t^2.
    A seed dl given by the caller is an input (no error of its own) and
    enters by its magnitude; se then comes with its own bound b_se."""
    A = hl.shape[1] // 2
    al, alpha = f32_as_double(act_limit), f32_as_double(alpha)
    mu = hl[:B, :A].double()
    p = prob[:B].double()
    t = p.tanh()
    b_t = tol["tanh"] * t.abs()
    if se is None:
        se = p - mu
        b_se = U * se.abs()
    dpi = dpi_a.double() + (dpi_b.double() if dpi_b is not None else 0.0)
    b_dpi = U * dpi.abs() if dpi_b is not None else torch.zeros_like(dpi)
    if dl is None:
        dl = dl_s = alpha / B
        b_dl = U * dl
    else:
        dl_s, dl, b_dl = dl, dl.abs(), 0.0
    om = 1 - t * t
    b_om = 2 * t.abs() * b_t + U * t * t + U * om
    dp = dpi * al * om
    b_dp = (dpi * al).abs() * b_om + al * om * b_dpi + U * dp.abs()
    g_mu = dp + dl_s * t
    b_mu = b_dp + t.abs() * b_dl + dl * b_t + U * (dl * t).abs() \
        + U * g_mu.abs()
    inner = se * t - 1.0
    b_in = t.abs() * b_se + se.abs() * b_t + U * (se * t).abs() \
        + U * inner.abs()
    g_ls = dp * se + dl_s * inner
    b_ls = se.abs() * b_dp + dp.abs() * b_se + U * (dp * se).abs() \
        + dl * b_in + inner.abs() * b_dl + U * (dl * inner).abs() \
        + U * g_ls.abs()
    return b_mu + 1e-37, b_ls + 1e-37


def tg_bwd_f32(hl, prob, dpi_a, dpi_b, alpha, B, act_limit, lo, hi,
               dl=None, se=None):
    """Plain fp32 (dmu, dls) in tg_bwd2_kernel's order (dl and se as in
    tg_bwd_ref, here in fp32)."""
    A = hl.shape[1] // 2
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    mu, raw = hl[:B, :A], hl[:B, A:]
    p = prob[:B]
    t = p.tanh()
    if se is None:
        se = p - mu
    dpi = dpi_a + dpi_b if dpi_b is not None else dpi_a
    if dl is None:
        dl = f(alpha) / f(float(B))
    dp = dpi * f(act_limit) * (1.0 - t * t)
    g_mu = dp + dl * t
    g_ls = dp * se + dl * (se * t - 1.0)
    mask = ((raw >= f(lo)) & (raw <= f(hi))).float()
    return g_mu, g_ls * mask


# ---- qloss2 (unweighted) and piloss2 ---------------------------------------

LOSS_B_FUSED = [1, 63, 64, 65, 255, 257, 1000, 1024]
LOSS_B_UNFUSED = 1500
LOSS_H2 = [1, 24]
LOSS_ACC0 = 3.0
QLOSS_HYPER = dict(alpha=0.2, gamma=0.99, scale=1.7)


def qloss_inputs(B, h2, seed=0):
    """General (non-dyadic) fp32 operands; done holds both values."""
    g = _gen(8000 + 7 * B + h2 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    done = (torch.rand(B, generator=g) < 0.3).float()
    done[0] = 0.0
    done[-1] = 1.0 if B > 1 else 0.0
    return dict(q1=r(B) * 3, q2=r(B) * 3, q1t=r(B) * 3, q2t=r(B) * 3,
                logp=r(B) * 4 - 2, rew=r(B), done=done,
                wt0=r(max(h2, 1)), wt1=r(max(h2, 1)))


def qloss_ref(t, B, alpha, gamma, scale):
    """float64 dict(loss, dq1, dq2, dy0, dy1) of the unweighted qloss2 and
    the matching bounds dict, from the fp32 operands t."""
    alpha, gamma, scale = (f32_as_double(v) for v in (alpha, gamma, scale))
    d = {k: v.double() for k, v in t.items()}
    t1 = scale * d["rew"]
    t2 = alpha * d["logp"]
    mn = torch.min(d["q1t"], d["q2t"])
    t3 = mn - t2
    gd = gamma * (1.0 - d["done"])
    t4 = gd * t3
    backup = t1 + t4
    b_t3 = U * (t2.abs() + t3.abs())
    b_t4 = U * t4.abs() + gd * b_t3 + U * gd * t3.abs()
    # 1 - done is exact for done in {0, 1}; a fractional done (n-step
    # sampling) costs one more rounding of the factor gd
    frac = (d["done"] != 0.0) & (d["done"] != 1.0)
    b_t4 = b_t4 + U * gd * t3.abs() * frac
    b_bk = U * (t1.abs() + backup.abs()) + b_t4
    ref, bnd = {}, {}
    s = torch.zeros(B, dtype=torch.float64)
    b_s = torch.zeros(B, dtype=torch.float64)
    for z, q in ((0, "q1"), (1, "q2")):
        e = d[q] - backup
        b_e = U * e.abs() + b_bk
        gq = 2.0 * e / B
        b_g = 2.0 * b_e / B + U * gq.abs()
        w = d[f"wt{z}"]
        ref[f"dq{z + 1}"], bnd[f"dq{z + 1}"] = gq, b_g + 1e-37
        ref[f"dy{z}"] = gq[:, None] * w[None]
        bnd[f"dy{z}"] = w.abs()[None] * b_g[:, None] \
            + U * ref[f"dy{z}"].abs() + 1e-37
        s = s + e * e
        b_s = b_s + 2 * e.abs() * b_e + U * e * e
    b_s = b_s + U * s
    ref["loss"] = s.sum() / B
    bnd["loss"] = (b_s.sum() + rounding_bound(B, s.sum())) / B \
        + U * ref["loss"]
    return ref, bnd


def qloss_f32(t, B, alpha, gamma, scale):
    """Plain fp32 evaluation in qloss2_kernel's order."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    backup = f(scale) * t["rew"] + f(gamma) * (1.0 - t["done"]) * (
        torch.min(t["q1t"], t["q2t"]) - f(alpha) * t["logp"])
    e1, e2 = t["q1"] - backup, t["q2"] - backup
    g1, g2 = 2.0 * e1 / float(B), 2.0 * e2 / float(B)
    return dict(loss=(e1 * e1 + e2 * e2).sum() / float(B), dq1=g1, dq2=g2,
                dy0=g1[:, None] * t["wt0"][None],
                dy1=g2[:, None] * t["wt1"][None])


def piloss_inputs(B, h2, seed=0):
    """Rows 0, 3, 6, ... have q1 == q2 exactly, rows 1, 4, ... q1 < q2,
    rows 2, 5, ... q2 < q1."""
    g = _gen(9000 + 7 * B + h2 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q1 = r(B) * 3
    gap = torch.rand(B, generator=g) + 0.01
    k = torch.arange(B) % 3
    q2 = torch.where(k == 0, q1, torch.where(k == 1, q1 + gap, q1 - gap))
    return dict(q1=q1, q2=q2, logp=r(B) * 4 - 2, wt0=r(max(h2, 1)),
                wt1=r(max(h2, 1)))


def piloss_ref(t, B, alpha):
    """float64 dict(loss, mean_logp, dq1, dq2, dy0, dy1) of piloss2 and the
    matching bounds dict.  The seeds -1/B and -0.5/B are one correctly
    rounded division each."""
    alpha = f32_as_double(alpha)
    d = {k: v.double() for k, v in t.items()}
    a, b, lp = d["q1"], d["q2"], d["logp"]
    t1 = alpha * lp
    el = t1 - torch.min(a, b)
    b_el = U * (t1.abs() + el.abs())
    ref, bnd = {}, {}
    ref["loss"] = el.sum() / B
    bnd["loss"] = (b_el.sum() + rounding_bound(B, el.abs().sum())) / B \
        + U * ref["loss"].abs()
    ref["mean_logp"] = lp.sum() / B
    bnd["mean_logp"] = rounding_bound(B, lp.abs().sum()) / B \
        + U * ref["mean_logp"].abs()
    tie = a == b
    g1 = torch.where(tie, -0.5, torch.where(a < b, -1.0, 0.0)) / B
    g2 = torch.where(tie, -0.5, torch.where(b < a, -1.0, 0.0)) / B
    for z, gq in ((0, g1), (1, g2)):
        w = d[f"wt{z}"]
        ref[f"dq{z + 1}"], bnd[f"dq{z + 1}"] = gq, U * gq.abs()
        ref[f"dy{z}"] = gq[:, None] * w[None]
        bnd[f"dy{z}"] = 2 * U * ref[f"dy{z}"].abs()
    return ref, bnd


def piloss_f32(t, B, alpha):
    """Plain fp32 evaluation in piloss2_kernel's order."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    a, b, lp = t["q1"], t["q2"], t["logp"]
    el = f(alpha) * lp - torch.min(a, b)
    tie = a == b
    g1 = torch.where(tie, f(-0.5), torch.where(a < b, f(-1.0), f(0.0))) \
        / float(B)
    g2 = torch.where(tie, f(-0.5), torch.where(b < a, f(-1.0), f(0.0))) \
        / float(B)
    return dict(loss=el.sum() / float(B), mean_logp=lp.sum() / float(B),
                dq1=g1, dq2=g2, dy0=g1[:, None] * t["wt0"][None],
                dy1=g2[:, None] * t["wt1"][None])


# ---- alpha_update -------------------------------------------------------------

ALPHA_LR = 3e-4
ALPHA_TARGET_ENTROPY = -6.0
# one fresh mean_logp per step; step 3 has mean_logp == -target_entropy
# exactly in fp32, so its gradient is 0
ALPHA_MEAN_LOGP = [-3.7251, 9.13, 6.0, -0.00317, 2.5e3]
ALPHA_LOG0 = math.log(0.2)


def alpha_ref(log_alpha, m, v, step, mean_logp, target_entropy, lr):
    """One float64 step of alpha_update_kernel from the fp32 state
    (log_alpha, m, v) and the step count BEFORE the call.  The kernel's
    literals enter as fp32 constants: 0.001f is not 1 - 0.999f (they differ
    by 1.3e-5 relative), so adam_ref cannot stand in for v.  Returns
    (log_alpha, m, v, u, g): the new state, the update term and the
    gradient."""
    c = {k: f32_as_double(x) for k, x in
         dict(b1=0.9, a1=0.1, b2=0.999, a2=0.001, eps=1e-8).items()}
    la, m, v, ml, te, lr = (f32_as_double(x) for x in
                            (log_alpha, m, v, mean_logp, target_entropy, lr))
    g = -(ml + te)
    t = float(step + 1)
    mi = c["b1"] * m + c["a1"] * g
    vi = c["b2"] * v + c["a2"] * g * g
    bc1 = 1.0 - c["b1"] ** t
    bc2 = 1.0 - c["b2"] ** t
    u = lr / bc1 * mi / (math.sqrt(vi / bc2) + c["eps"])
    return la - u, mi, vi, u, g


def alpha_bounds(m, v, ref):
    """Bounds (log_alpha, m, v) on |kernel - alpha_ref| for one step.  g is
    one rounded sum; m and v are three rounded operations each on top of
    it; log_alpha is one final rounding plus the update's relative error,
    dominated by the cancellation in 1 - powf(b, t) (the 1e-4 |u| term
    kernel_refs.adam_bounds justifies)."""
    la, mi, vi, u, g = ref
    m, v = f32_as_double(m), f32_as_double(v)
    b_g = U * abs(g)
    b_m = 0.1 * b_g + U * (0.9 * abs(m) + 0.1 * abs(g)) + U * abs(mi)
    b_v = 0.001 * 2 * abs(g) * b_g \
        + U * (0.999 * v + 2 * 0.001 * g * g) + U * vi
    # the errors of m and v reach u through du/dm = u / m and
    # |du/dv| <= |u| / (2 v)
    b_u = 1e-4 * abs(u)
    if mi != 0.0:
        b_u += abs(u / mi) * b_m + abs(u) / (2 * vi) * b_v
    b_la = float(ulp32(torch.tensor(la, dtype=torch.float64))) + b_u
    return b_la, b_m + 1e-45, b_v + 1e-45


def alpha_f32(log_alpha, m, v, step, mean_logp, target_entropy, lr):
    """Plain fp32 step in alpha_update_kernel's order: (log_alpha, m, v)."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    g = -(f(mean_logp) + f(target_entropy))
    t = f(float(step + 1))
    mi = f(0.9) * f(m) + f(0.1) * g
    vi = f(0.999) * f(v) + f(0.001) * g * g
    bc1 = 1.0 - torch.pow(f(0.9), t)
    bc2 = 1.0 - torch.pow(f(0.999), t)
    la = f(log_alpha) - f(lr) / bc1 * mi / (torch.sqrt(vi / bc2) + f(1e-8))
    return float(la), float(mi), float(vi)


# ---------------------------------------------------------------------------
# The autograd-path kernels (tac_kernels.hip: tanh_gauss_fwd / _bwd,
# sac_q_loss_fwd, sac_pi_loss_fwd, polyak_, adam_step_) and the eager
# fallbacks of ops/functional.py
# ---------------------------------------------------------------------------
#
# The head takes mu, log_std and eps as three [B, A] tensors; packed as
# hl = mu | log_std it is the head of tg_ref, so tg_ref / tg_fwd_bounds /
# tg_bwd_ref / tg_bwd_bounds serve it unchanged.  Deterministic means
# eps = 0 there: prob = mu and the Gaussian term is -ls - log(2 pi) / 2.

TGH_CASES = [(2, 1), (6, 6), (5, 17), (4, 64), (130, 33)]     # (B, A)
TGH_CLAMPS = [(TG_LO, TG_HI), (-20.0, 2.0)]    # kernel_refs', the models'
TGH_SMALL_LS = -16.0      # at and below this exp(ls) |eps| < ulp(0.5) / 2


def tgh_id(v):
    return "x".join(str(int(x)) for x in v)


def tgh_raw_log_std(lo, hi):
    """Raw log_std values every case cycles through: below, at and just
    inside both clamp ends, an interior value, beyond the top; with a
    bottom below TGH_SMALL_LS also -18 and -16, where std * eps drops
    under the spacing of mu."""
    inf = torch.tensor(float("inf"))
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    out = [lo - 1.0, lo, float(torch.nextafter(f(lo), inf)), -1.25,
           hi, float(torch.nextafter(f(hi), -inf)), hi + 3.0]
    if lo < TGH_SMALL_LS:
        out += [-18.0, TGH_SMALL_LS]
    return out


def tgh_inputs(B, A, lo, hi):
    """fp32 (mu, log_std, eps) [B, A] in the pattern of tg_hl: all but two
    of every len + 2 elements take the next special log_std, five of every
    eight the next special mu (TG_MU: |mu| in {0, 0.5, 3, 12}; the periods
    9 / 11 are coprime to 8, so all pairs occur in the large case).  eps is
    a fixed seeded normal draw pushed out to |eps| >= 1 wherever the
    clamped log_std is at most TGH_SMALL_LS."""
    g = _gen(7500 + B * 100 + A + (1000 if lo < TGH_SMALL_LS else 0))
    n = B * A
    i = torch.arange(n) + B + A
    mu = torch.randn(n, generator=g) * 2
    ls = torch.rand(n, generator=g) * 5 - 4
    eps = torch.randn(n, generator=g)
    sp_mu = torch.tensor(TG_MU)
    sp_ls = torch.tensor(tgh_raw_log_std(lo, hi))
    ns = len(sp_ls)
    km, kl = i % 8, i % (ns + 2)
    mu = torch.where(km < 5, sp_mu[km.clamp_max(4)], mu)
    ls = torch.where(kl < ns, sp_ls[kl.clamp_max(ns - 1)], ls)
    small = ls.clamp(lo, hi) <= TGH_SMALL_LS
    sign = torch.where(eps < 0, -1.0, 1.0)
    eps = torch.where(small & (eps.abs() < 1), sign * (1 + eps.abs()), eps)
    return (mu.view(B, A).contiguous(), ls.view(B, A).contiguous(),
            eps.view(B, A).contiguous())


def _tgh_pack(mu, log_std, eps, det):
    hl = torch.cat([mu, log_std], 1)
    return hl, (torch.zeros_like(eps) if det else eps)


def tgh_ref(mu, log_std, eps, act_limit, lo, hi, det, with_logp):
    """float64 (pi, prob, ls_c, logp) of tanh_gauss_fwd; logp is None
    without the log-probability."""
    hl, e = _tgh_pack(mu, log_std, eps, det)
    pi, prob, logp = tg_ref(hl, e, act_limit, lo, hi)
    ls_c = log_std.double().clamp(f32_as_double(lo), f32_as_double(hi))
    return pi, prob, ls_c, (logp if with_logp else None)


def tgh_fwd_bounds(mu, log_std, eps, act_limit, lo, hi, det, with_logp,
                   tol=LIBM_TOL):
    """Bounds (pi, prob, ls_c, logp) on |kernel - tgh_ref|.  ls_c is a
    clamp and the deterministic prob a copy: both exact."""
    hl, e = _tgh_pack(mu, log_std, eps, det)
    b_pi, b_prob, b_logp = tg_fwd_bounds(hl, e, act_limit, lo, hi, tol=tol)
    if det:
        b_prob = torch.zeros_like(b_prob)
    return b_pi, b_prob, torch.zeros_like(b_prob), \
        (b_logp if with_logp else None)


def tgh_fwd_f32(mu, log_std, eps, act_limit, lo, hi, det, with_logp):
    """Plain fp32 (pi, prob, ls_c, logp) in tanh_gauss_fwd_kernel's order,
    which is tg_fwd2_kernel's."""
    hl, e = _tgh_pack(mu, log_std, eps, det)
    pi, prob, logp = tg_fwd_f32(hl, e, act_limit, lo, hi)
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))
    return pi, prob, log_std.clamp(f(lo), f(hi)), \
        (logp if with_logp else None)


def tgh_logp_by_subtraction_f32(mu, log_std, eps, lo, hi):
    """fp32 logp as the head computed it before it took the noise from
    eps: e = (prob - mu) / std rebuilt from prob = mu + std * eps.  Kept
    to show on the CPU what tgh_inputs at the default clamp catch."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    ls = log_std.clamp(float(f(lo)), float(f(hi)))
    std = ls.exp()
    prob = mu + std * eps
    e = (prob - mu) / std
    x = -2.0 * prob
    sp = torch.where(x > 20.0, x, torch.log1p(torch.exp(x.clamp_max(20.0))))
    gauss = -0.5 * e * e - ls - f(0.5) * f(1.8378770664093453)
    corr = f(1.3862943611198906) - prob - sp
    return (gauss - corr).sum(1)


def tgh_bwd_operands(B, A):
    """fp32 (dpi [B, A], dlogp [B]): general floats of both signs."""
    g = _gen(7600 + B * 100 + A)
    return torch.randn(B, A, generator=g), torch.randn(B, generator=g)


def _tgh_bwd_terms(log_std, eps, ls_c, dlogp, det, with_logp):
    """float64 seed dl [B, 1] and se = std * eps of the backward."""
    e = torch.zeros_like(eps) if det else eps
    se = ls_c.double().exp() * e.double()
    dl = dlogp.double()[:, None] if with_logp \
        else torch.zeros(len(dlogp), 1, dtype=torch.float64)
    return dl, se


def tgh_bwd_ref(mu, log_std, eps, prob, ls_c, dpi, dlogp, act_limit, lo, hi,
                det, with_logp):
    """float64 (dmu, dls) of tanh_gauss_bwd from the fp32 prob and ls_c
    the forward stored: the gradient of
        sum(dpi * pi) + sum(dlogp * logp)
    with d prob / d log_std = std * eps (0 when deterministic), through
    the clamp inclusively at both ends, as torch.clamp's backward."""
    hl = torch.cat([mu, log_std], 1)
    dl, se = _tgh_bwd_terms(log_std, eps, ls_c, dlogp, det, with_logp)
    return tg_bwd_ref(hl, prob, dpi, None, 0.0, len(mu), act_limit, lo, hi,
                      dl=dl, se=se)


def tgh_bwd_bounds(mu, log_std, eps, prob, ls_c, dpi, dlogp, act_limit, lo,
                   hi, det, with_logp, tol=LIBM_TOL):
    """Bounds (dmu, dls): tg_bwd_bounds with se = exp(ls_c) * eps charged
    one libm call and one rounding, and the seed an exact input."""
    hl = torch.cat([mu, log_std], 1)
    dl, se = _tgh_bwd_terms(log_std, eps, ls_c, dlogp, det, with_logp)
    return tg_bwd_bounds(hl, prob, dpi, None, 0.0, len(mu), act_limit, lo,
                         hi, tol=tol, dl=dl, se=se,
                         b_se=(tol["exp"] + U) * se.abs())


def tgh_bwd_f32(mu, log_std, eps, prob, ls_c, dpi, dlogp, act_limit, lo, hi,
                det, with_logp):
    """Plain fp32 (dmu, dls) in tanh_gauss_bwd_kernel's order."""
    hl = torch.cat([mu, log_std], 1)
    se = torch.zeros_like(eps) if det else ls_c.exp() * eps
    dl = dlogp[:, None] if with_logp else torch.zeros(len(dlogp), 1)
    return tg_bwd_f32(hl, prob, dpi, None, 0.0, len(mu), act_limit, lo, hi,
                      dl=dl, se=se)


# ---- sac_q_loss_fwd / sac_pi_loss_fwd ------------------------------------------
#
# qloss_ref / piloss_ref are the references (their dy0 / dy1 belong to the
# fused kernels and are not used).  The kernels reduce per block, divide
# each block's partial by B and add the quotients atomically in any order:
# rounding_bound(B, .) holds for every order of the B + 63 additions, and
# the divisions of the partials are within the U |loss| already charged.

FLAT_LOSS_B = [1, 63, 64, 65, 255, 256, 257, 1000, 64 * 256 + 3]
# done as an n-step buffer writes it: 1 - gamma^(M-1) (1 - done)
FLAT_DONE_FRACTIONS = [1.0 - 0.99, 1.0 - 0.99 ** 2, 1.0 - 0.99 ** 4]


def flat_qloss_inputs(B):
    """qloss_inputs with fractional done on every fifth row and exact
    q1t == q2t ties on every third."""
    t = qloss_inputs(B, 1, seed=31)
    i = torch.arange(B)
    fr = torch.tensor(FLAT_DONE_FRACTIONS, dtype=torch.float32)
    t["done"] = torch.where(i % 5 == 2, fr[(i // 5) % len(fr)], t["done"])
    t["q2t"] = torch.where(i % 3 == 1, t["q1t"], t["q2t"])
    return t


def piloss_dlogp_ref(B, alpha):
    """float64 seed of logp: the fp32 alpha over B, one correctly rounded
    division in the kernel."""
    return f32_as_double(alpha) / B


# ---- polyak_ -----------------------------------------------------------------

POLYAK_N = [1, 3, 4, 5, 1023, 1024 * 256 * 4 + 7]
POLYAK_RHO = [0.995, 0.0, 1.0]


def polyak_inputs(n, seed=0):
    g = _gen(6500 + seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def polyak_ref(targ, src, rho):
    """float64 (new target, bound) of targ = rho targ + (1 - rho) src with
    rho as the kernel holds it (fp32).  1 - rho is exact in fp32 for rho in
    [0.5, 1] and for 0; three rounded operations remain (two products, one
    sum), each charged U of its result.  A contraction into an FMA drops
    one of them."""
    r = f32_as_double(rho)
    assert float(torch.tensor(1.0) - torch.tensor(rho, dtype=torch.float32)) \
        == 1.0 - r
    a = r * targ.double()
    b = (1.0 - r) * src.double()
    out = a + b
    return out, U * (a.abs() + b.abs() + out.abs()) + 1e-45


def polyak_f32(targ, src, rho):
    """Plain fp32 evaluation in polyak_kernel's order."""
    r = torch.tensor(rho, dtype=torch.float32)
    return r * targ + (1.0 - r) * src


# ---- adam_step_ ----------------------------------------------------------------

ADAM_FLAT_N = [1, 255, 1024 * 256 + 777]
ADAM_FLAT_STEPS = [1, 2, 1000, 100000]
ADAM_FLAT_WD = [0.0, 2.0 ** -7]


def adam_flat_f32(p, g, m, v, t, hyper):
    """Plain fp32 (p, m, v) in adam_kernel's order (no FMA)."""
    f = {k: torch.tensor(x, dtype=torch.float32) for k, x in hyper.items()}
    one = torch.tensor(1.0)
    tt = torch.tensor(float(t))
    bc1 = one - torch.pow(f["b1"], tt)
    bc2 = one - torch.pow(f["b2"], tt)
    gi = g + f["wd"] * p
    mi = f["b1"] * m + (one - f["b1"]) * gi
    vi = f["b2"] * v + (one - f["b2"]) * gi * gi
    pn = p - f["lr"] / bc1 * mi / (torch.sqrt(vi / bc2) + f["eps"])
    return pn, mi, vi
