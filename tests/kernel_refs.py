"""Float64 CPU references, operand generators and case tables shared by
test_gpu_mgemm.py, test_gpu_conv_exact.py, conv_lds_worker.py,
test_gpu_wgrad.py, wgrad_env_worker.py, test_gpu_adam_t.py and the CPU
precondition test (test_kernel_refs.py).  Plain helper module, not a
conftest.

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
