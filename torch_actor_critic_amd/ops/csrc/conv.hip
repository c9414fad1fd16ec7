// Implicit-GEMM convolution kernels (gfx950 / CDNA4) for the visual
// actor/critic path (reference networks/convolutional.py:30-51: Nature-
// CNN trunk, valid padding, strides [4,2,1], kernels [8,4,3]).
//
// All three passes run as MFMA GEMMs over an implicitly-gathered
// im2col operand (no materialized im2col buffer):
//   fwd   : Y[m=(b,oy,ox), n=oc]  = sum_k  X[b,ic,oy*s+ky,ox*s+kx] W[oc,k]
//   dgrad : dX[m=(b,iy,ix), n=ic] = sum_k' dY[b,oc,(iy-ky)/s,(ix-kx)/s]
//                                          WT[ic, k'=(oc,ky,kx)]
//   wgrad : dW[oc, k] = sum_m dY[m,oc] im2col[m,k];  db fused
// Weight tensors stay fp32 master; bf16 mode rounds operands on stage.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <vector>

namespace convk {

#define DEVINL __device__ __forceinline__

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int TB = 64;
constexpr int BKB = 64, LDB = 72;   // bf16 K-step / LDS halves per row
constexpr int BKF = 16, LDF = 17;   // fp32

struct ConvDims {
  int B, IC, IH, IW, OC, OH, OW, KH, KW, S;
};

// ---- shared MFMA tile compute (same fragment plan as fused.hip) -------

template <bool BF16>
DEVINL void mma_tiles(const void* xs_, const void* ws_, f32x4 (&acc)[2][2],
                      int lane, int wrow, int wcol) {
  if constexpr (BF16) {
    const __bf16* xs = (const __bf16*)xs_;
    const __bf16* ws = (const __bf16*)ws_;
    const int arow = lane & 15;
    const int ak0 = (lane >> 4) * 8;
#pragma unroll
    for (int kk = 0; kk < BKB; kk += 32) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        bf16x8 a = *(const bf16x8*)&xs[(wrow + mi * 16 + arow) * LDB
                                       + kk + ak0];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          bf16x8 b = *(const bf16x8*)&ws[(wcol + ni * 16 + arow) * LDB
                                         + kk + ak0];
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, b, acc[mi][ni], 0, 0, 0);
        }
      }
    }
  } else {
    const float* xs = (const float*)xs_;
    const float* ws = (const float*)ws_;
    const int arow = lane & 15;
    const int akl = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < BKF; kk += 4) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        float a = xs[(wrow + mi * 16 + arow) * LDF + kk + akl];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          float b = ws[(wcol + ni * 16 + arow) * LDF + kk + akl];
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a, b, acc[mi][ni], 0, 0, 0);
        }
      }
    }
  }
}

template <bool BF16>
DEVINL void lds_put(void* lds, int row, int c, float v) {
  if constexpr (BF16) ((__bf16*)lds)[row * LDB + c] = (__bf16)v;
  else                ((float*)lds)[row * LDF + c] = v;
}

// im2col element: A[m, k] with m=(b,oy,ox), k=(ic,ky,kx)
DEVINL float im2col_at(const float* x, const ConvDims& d, int m, int k) {
  const int ox = m % d.OW, t1 = m / d.OW;
  const int oy = t1 % d.OH, b = t1 / d.OH;
  const int kx = k % d.KW, t2 = k / d.KW;
  const int ky = t2 % d.KH, ic = t2 / d.KH;
  const int iy = oy * d.S + ky, ix = ox * d.S + kx;
  return x[(((int64_t)b * d.IC + ic) * d.IH + iy) * d.IW + ix];
}

// incremental decompositions (divisions hoisted out of element loops)
struct MDec { int b, oy, ox; };
DEVINL MDec mdec(int m, const ConvDims& d) {
  MDec r;
  r.ox = m % d.OW;
  int t = m / d.OW;
  r.oy = t % d.OH;
  r.b = t / d.OH;
  return r;
}
DEVINL void minc(MDec& r, const ConvDims& d) {
  if (++r.ox == d.OW) { r.ox = 0; if (++r.oy == d.OH) { r.oy = 0; ++r.b; } }
}
struct KDec { int ic, ky, kx; };
DEVINL KDec kdec(int k, const ConvDims& d) {
  KDec r;
  r.kx = k % d.KW;
  int t = k / d.KW;
  r.ky = t % d.KH;
  r.ic = t / d.KH;
  return r;
}
DEVINL void kinc(KDec& r, const ConvDims& d) {
  if (++r.kx == d.KW) { r.kx = 0; if (++r.ky == d.KH) { r.ky = 0; ++r.ic; } }
}

// ---------------------------------------------------------------------------
// conv fwd: grid (ceil(M/64), ceil(OC/64)); Y NCHW scatter epilogue
// ---------------------------------------------------------------------------

struct ConvP {
  const float* x; const float* w; const float* bias; float* y;
};

// up to 4 problems per launch (blockIdx.z): the twin critics AND the
// target twins share every conv launch in the critic phase (same shapes,
// different inputs/weights) — mirrors the MLP engine's 4-problem GEMMs
struct ConvQ { ConvP p[4]; };

// TK/TS: compile-time kernel size / stride for the reference conv
// family ({8,4}, {4,2}, {3,1}); 0 = runtime fallback.  The gathers are
// VALU-bound (measured ~85 VALU insts per MFMA), so constant-folding
// the wrap/index arithmetic and using 32-bit addressing is the lever.
template <bool BF16, bool RELU, int TK, int TS>
__global__ __launch_bounds__(256)
void conv_fwd_kernel(ConvQ q, ConvDims d) {
  const ConvP& pp = q.p[blockIdx.z];
  const float* x = pp.x;
  const float* w = pp.w;
  const float* bias = pp.bias;
  float* y = pp.y;
  const int KW = TK ? TK : d.KW;
  const int KH = TK ? TK : d.KH;
  const int S = TS ? TS : d.S;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bm0 = blockIdx.x * TB;
  const int bn0 = blockIdx.y * TB;
  const int M = d.B * d.OH * d.OW;
  const int K = d.IC * KH * KW;
  constexpr int BK = BF16 ? BKB : BKF;
  constexpr int EL = BF16 ? 16 : 4;
  constexpr int LBYTES = BF16 ? (64 * LDB * 2) : (64 * LDF * 4);
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  void* xs = smem;
  void* ws = smem + LBYTES;
  f32x4 acc[2][2] = {};

  const int row = tid & 63;
  const int c00 = (tid >> 6) * EL;
  const int m_my = bm0 + row;
  const MDec md = mdec(m_my < M ? m_my : 0, d);
  const int n_my = bn0 + row;
  const float* wrow_p = n_my < d.OC ? w + (int64_t)n_my * K : nullptr;
  // 32-bit base of this thread's pixel (host checks numel < 2^31)
  const int xbase = (md.b * d.IC * d.IH + md.oy * S) * d.IW + md.ox * S;
  const int ihw = d.IH * d.IW;

  // T14 register-staged pipeline: gather tile t into regs, write LDS,
  // prefetch tile t+1 while the MFMAs run.
  float va[EL], vb[EL];
  auto load_chunk = [&](int k0) {
    int kc = (k0 + c00) < K ? (k0 + c00) : 0;
    int kx = kc % KW;
    int t2 = kc / KW;
    int ky = t2 % KH;
    int ic = t2 / KH;
#pragma unroll
    for (int e = 0; e < EL; ++e) {
      int k = k0 + c00 + e;
      float v = 0.f;
      if (m_my < M && k < K)
        v = x[xbase + ic * ihw + ky * d.IW + kx];
      va[e] = v;
      if (++kx == KW) { kx = 0; if (++ky == KH) { ky = 0; ++ic; } }
    }
    if (wrow_p && ((K & 3) == 0) && k0 + c00 + EL <= K) {
      const float4* src = (const float4*)(wrow_p + k0 + c00);
#pragma unroll
      for (int q = 0; q < EL / 4; ++q) {
        float4 f = src[q];
        vb[q*4+0]=f.x; vb[q*4+1]=f.y; vb[q*4+2]=f.z; vb[q*4+3]=f.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < EL; ++e) {
        int k = k0 + c00 + e;
        vb[e] = (wrow_p && k < K) ? wrow_p[k] : 0.f;
      }
    }
  };
  load_chunk(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
    for (int e = 0; e < EL; ++e) {
      lds_put<BF16>(xs, row, c00 + e, va[e]);
      lds_put<BF16>(ws, row, c00 + e, vb[e]);
    }
    if (k0 + BK < K) load_chunk(k0 + BK);
    __syncthreads();
    mma_tiles<BF16>(xs, ws, acc, lane, wrow, wcol);
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = bm0 + wrow + mi * 16 + crow + r;
        int oc = bn0 + wcol + ni * 16 + ccol;
        if (m < M && oc < d.OC) {
          float v = acc[mi][ni][r] + (bias ? bias[oc] : 0.f);
          if constexpr (RELU) v = fmaxf(v, 0.f);
          const int ox = m % d.OW, t1 = m / d.OW;
          const int oy = t1 % d.OH, b = t1 / d.OH;
          y[(((int64_t)b * d.OC + oc) * d.OH + oy) * d.OW + ox] = v;
        }
      }
}

// ---------------------------------------------------------------------------
// LDS-subimage conv fwd: the implicit-GEMM gather above reads every
// im2col element straight from HBM/L2 — scattered, latency-bound
// (round-1 PMC: not VALU-bound).  Here each block first stages the
// input-window ROWS its 64 output pixels need (contiguous memory,
// coalesced float4s) into LDS once, then builds the im2col A tile from
// LDS — each input byte is reused by up to KH*KW/S^2 taps without
// another VMEM round trip.  m tiles are per-image (tiles never span
// two images): grid.x = B * ceil(OH*OW/64).
// LDS plan: input slab <= 13056 floats (worst case conv2@84x84:
// 20 rows x 20 x 32ch) + the A/B bf16 tiles.
// ---------------------------------------------------------------------------

constexpr int SLAB_F = 13056;

template <bool BF16, bool RELU, int TK, int TS>
__global__ __launch_bounds__(256)
void conv_fwd_lds_kernel(ConvQ q, ConvDims d, int tiles_img) {
  const ConvP& pp = q.p[blockIdx.z];
  const float* x = pp.x;
  const float* w = pp.w;
  const float* bias = pp.bias;
  float* y = pp.y;
  const int KW = TK, KH = TK, S = TS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int img = (int)blockIdx.x / tiles_img;
  const int mt = (int)blockIdx.x % tiles_img;
  const int npx = d.OH * d.OW;
  const int m0 = mt * TB;                  // first pixel of this tile
  const int m_n = min(TB, npx - m0);       // pixels in this tile
  const int bn0 = blockIdx.y * TB;
  const int K = d.IC * KH * KW;
  constexpr int BK = BF16 ? BKB : BKF;
  constexpr int EL = BF16 ? 16 : 4;
  constexpr int LBYTES = BF16 ? (64 * LDB * 2) : (64 * LDF * 4);
  __shared__ __attribute__((aligned(16))) float slab[SLAB_F];
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  void* xs = smem;
  void* ws = smem + LBYTES;
  f32x4 acc[2][2] = {};

  // -- stage the input window rows [iy0, iy1) for all channels ---------
  const int oy0 = m0 / d.OW;
  const int oy1 = (m0 + m_n - 1) / d.OW;
  const int iy0 = oy0 * S;
  const int rows = min(d.IH - iy0, (oy1 - oy0) * S + KH);
  const int rw = rows * d.IW;              // floats per channel slab
  {
    const float* xb = x + ((int64_t)img * d.IC * d.IH + iy0) * d.IW;
    const int total = d.IC * rw;
    for (int i = tid * 4; i < total; i += 256 * 4) {
      const int ic = i / rw;
      const int r = i - ic * rw;
      if (r + 4 <= rw) {
        const float* src = xb + (int64_t)ic * d.IH * d.IW + r;
        float* dst = slab + i;
        if ((((uintptr_t)src) & 15) == 0) {
          float4 f = *(const float4*)src;
          dst[0] = f.x; dst[1] = f.y; dst[2] = f.z; dst[3] = f.w;
        } else {
          dst[0] = src[0]; dst[1] = src[1];
          dst[2] = src[2]; dst[3] = src[3];
        }
      } else {  // chunk crosses a channel boundary: per-element
        for (int e = 0; e < 4; ++e) {
          const int idx = i + e;
          if (idx >= total) break;
          const int ic2 = idx / rw, r2 = idx - ic2 * rw;
          slab[idx] = xb[(int64_t)ic2 * d.IH * d.IW + r2];
        }
      }
    }
  }
  __syncthreads();

  // -- K loop: A tile built from the LDS slab, B from the weights ------
  const int row = tid & 63;
  const int c00 = (tid >> 6) * EL;
  const int m_my = m0 + min(row, m_n - 1);
  const int oy_l = m_my / d.OW - oy0;      // local row in the slab
  const int ox = m_my - (oy_l + oy0) * d.OW;
  const bool mvalid = row < m_n;
  const int n_my = bn0 + row;
  const float* wrow_p = n_my < d.OC ? w + (int64_t)n_my * K : nullptr;
  const int sbase = (oy_l * S) * d.IW + ox * S;

  for (int k0 = 0; k0 < K; k0 += BK) {
    {
      int kc = k0 + c00;
      int kx = kc % KW;
      int t2 = kc / KW;
      int ky = t2 % KH;
      int ic = t2 / KH;
#pragma unroll
      for (int e = 0; e < EL; ++e) {
        int k = k0 + c00 + e;
        float v = 0.f;
        if (mvalid && k < K)
          v = slab[ic * rw + sbase + ky * d.IW + kx];
        lds_put<BF16>(xs, row, c00 + e, v);
        if (++kx == KW) { kx = 0; if (++ky == KH) { ky = 0; ++ic; } }
      }
    }
    {
      float vb[EL];
      if (wrow_p && ((K & 3) == 0) && k0 + c00 + EL <= K) {
        const float4* src = (const float4*)(wrow_p + k0 + c00);
#pragma unroll
        for (int qq = 0; qq < EL / 4; ++qq) {
          float4 f = src[qq];
          vb[qq*4+0]=f.x; vb[qq*4+1]=f.y; vb[qq*4+2]=f.z; vb[qq*4+3]=f.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < EL; ++e) {
          int k = k0 + c00 + e;
          vb[e] = (wrow_p && k < K) ? wrow_p[k] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < EL; ++e) lds_put<BF16>(ws, row, c00 + e, vb[e]);
    }
    __syncthreads();
    mma_tiles<BF16>(xs, ws, acc, lane, wrow, wcol);
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int mrow = wrow + mi * 16 + crow + r;
        int oc = bn0 + wcol + ni * 16 + ccol;
        if (mrow < m_n && oc < d.OC) {
          float v = acc[mi][ni][r] + (bias ? bias[oc] : 0.f);
          if constexpr (RELU) v = fmaxf(v, 0.f);
          const int m = m0 + mrow;
          const int oy = m / d.OW, oxw = m - oy * d.OW;
          y[(((int64_t)img * d.OC + oc) * d.OH + oy) * d.OW + oxw] = v;
        }
      }
}

// ---------------------------------------------------------------------------
// conv dgrad: dX = spread(dY) @ WT; WT [IC, OC*KH*KW] prepared by caller.
// m=(b,iy,ix), k'=(oc,ky,kx).  RELU mask (y>0) applied to dY on gather.
// ---------------------------------------------------------------------------

struct ConvGP {
  const float* dy; const float* ymask; const float* wt; float* dx;
};

template <bool BF16, bool MASK>
__global__ __launch_bounds__(256)
void conv_dgrad_kernel(ConvGP p0, ConvGP p1, ConvDims d) {
  const ConvGP& pp = blockIdx.z ? p1 : p0;
  const float* dy = pp.dy;
  const float* ymask = pp.ymask;
  const float* wt = pp.wt;
  float* dx = pp.dx;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bm0 = blockIdx.x * TB;
  const int bn0 = blockIdx.y * TB;
  const int M = d.B * d.IH * d.IW;
  const int K = d.OC * d.KH * d.KW;
  constexpr int BK = BF16 ? BKB : BKF;
  constexpr int EL = BF16 ? 16 : 4;
  constexpr int LBYTES = BF16 ? (64 * LDB * 2) : (64 * LDF * 4);
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  void* xs = smem;
  void* ws = smem + LBYTES;
  f32x4 acc[2][2] = {};

  const int row = tid & 63;
  const int c00 = (tid >> 6) * EL;
  const int m_my = bm0 + row;
  int ix0, iy0, b0;
  {
    int m = m_my < M ? m_my : 0;
    ix0 = m % d.IW;
    int t1 = m / d.IW;
    iy0 = t1 % d.IH;
    b0 = t1 / d.IH;
  }
  const int n_my = bn0 + row;
  const float* wtrow = n_my < d.IC ? wt + (int64_t)n_my * K : nullptr;

  // T14 register-staged pipeline (prefetch chunk t+1 during MFMAs)
  float va[EL], vb[EL];
  auto load_chunk = [&](int k0) {
    int kx = (k0 + c00) % d.KW;
    int t2 = (k0 + c00) / d.KW;
    int ky = t2 % d.KH;
    int oc = t2 / d.KH;
#pragma unroll
    for (int e = 0; e < EL; ++e) {
      int k = k0 + c00 + e;
      float v = 0.f;
      if (m_my < M && k < K) {
        const int ry = iy0 - ky, rx = ix0 - kx;
        if (ry >= 0 && rx >= 0 && ry % d.S == 0 && rx % d.S == 0) {
          const int oy = ry / d.S, ox = rx / d.S;
          if (oy < d.OH && ox < d.OW) {
            int64_t idx = (((int64_t)b0 * d.OC + oc) * d.OH + oy) * d.OW + ox;
            v = dy[idx];
            if constexpr (MASK) v = ymask[idx] > 0.f ? v : 0.f;
          }
        }
      }
      va[e] = v;
      if (++kx == d.KW) { kx = 0; if (++ky == d.KH) { ky = 0; ++oc; } }
    }
    if (wtrow && ((K & 3) == 0) && k0 + c00 + EL <= K) {
      const float4* src = (const float4*)(wtrow + k0 + c00);
#pragma unroll
      for (int q = 0; q < EL / 4; ++q) {
        float4 f = src[q];
        vb[q*4+0]=f.x; vb[q*4+1]=f.y; vb[q*4+2]=f.z; vb[q*4+3]=f.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < EL; ++e) {
        int k = k0 + c00 + e;
        vb[e] = (wtrow && k < K) ? wtrow[k] : 0.f;
      }
    }
  };
  load_chunk(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
    for (int e = 0; e < EL; ++e) {
      lds_put<BF16>(xs, row, c00 + e, va[e]);
      lds_put<BF16>(ws, row, c00 + e, vb[e]);
    }
    if (k0 + BK < K) load_chunk(k0 + BK);
    __syncthreads();
    mma_tiles<BF16>(xs, ws, acc, lane, wrow, wcol);
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = bm0 + wrow + mi * 16 + crow + r;
        int ic = bn0 + wcol + ni * 16 + ccol;
        if (m < M && ic < d.IC) {
          const int ix = m % d.IW, t1 = m / d.IW;
          const int iy = t1 % d.IH, b = t1 / d.IH;
          dx[(((int64_t)b * d.IC + ic) * d.IH + iy) * d.IW + ix] =
              acc[mi][ni][r];
        }
      }
}

// ---------------------------------------------------------------------------
// Stride-class dgrad (S>1): pixels with (iy%S, ix%S) == (cy, cx) share
// the SAME valid tap set (ky ≡ cy, kx ≡ cx mod S), so each class runs a
// dense GEMM over K_cls = OC·ceil((KH-cy)/S)·ceil((KW-cx)/S) instead of
// the full K = OC·KH·KW with (S²-1)/S² of the taps predicated to zero
// (4x less MFMA+gather work at S=2, 16x at S=4).
// grid: (ceil(Mc_max/TB), ceil(IC/TB), nz·S²); blockIdx.z = cls·nz + z.
// ---------------------------------------------------------------------------

template <bool BF16, bool MASK>
__global__ __launch_bounds__(256)
void conv_dgrad_cls_kernel(ConvGP p0, ConvGP p1, ConvDims d, int nz) {
  const int zi = (int)blockIdx.z;
  const int zz = zi % nz;
  const int cls = zi / nz;
  const int cy = cls / d.S, cx = cls % d.S;
  const int IHc = (d.IH - cy + d.S - 1) / d.S;
  const int IWc = (d.IW - cx + d.S - 1) / d.S;
  const int KHc = d.KH > cy ? (d.KH - cy + d.S - 1) / d.S : 0;
  const int KWc = d.KW > cx ? (d.KW - cx + d.S - 1) / d.S : 0;
  const int Mc = d.B * IHc * IWc;
  const int Kc = d.OC * KHc * KWc;
  const int bm0 = blockIdx.x * TB;
  if (bm0 >= Mc) return;
  const ConvGP& pp = zz ? p1 : p0;
  const float* dy = pp.dy;
  const float* ymask = pp.ymask;
  const float* wt = pp.wt;
  float* dx = pp.dx;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bn0 = blockIdx.y * TB;
  constexpr int BK = BF16 ? BKB : BKF;
  constexpr int EL = BF16 ? 16 : 4;
  constexpr int LBYTES = BF16 ? (64 * LDB * 2) : (64 * LDF * 4);
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  void* xs = smem;
  void* ws = smem + LBYTES;
  f32x4 acc[2][2] = {};

  const int row = tid & 63;
  const int c00 = (tid >> 6) * EL;
  const int m_my = bm0 + row;
  int px0, py0, b0;
  {
    int m = m_my < Mc ? m_my : 0;
    px0 = m % IWc;
    int t1 = m / IWc;
    py0 = t1 % IHc;
    b0 = t1 / IHc;
  }
  const int n_my = bn0 + row;
  const int K_full = d.OC * d.KH * d.KW;
  const float* wtrow = n_my < d.IC ? wt + (int64_t)n_my * K_full : nullptr;

  float va[EL], vb[EL];
  auto load_chunk = [&](int k0) {
    int kc = k0 + c00;
    int kxi = KWc ? kc % KWc : 0;
    int t2 = KWc ? kc / KWc : 0;
    int kyi = KHc ? t2 % KHc : 0;
    int oc = KHc ? t2 / KHc : 0;
#pragma unroll
    for (int e = 0; e < EL; ++e) {
      int k = k0 + c00 + e;
      float v = 0.f;
      float wv = 0.f;
      if (k < Kc) {
        if (m_my < Mc) {
          const int oy = py0 - kyi, ox = px0 - kxi;
          if (oy >= 0 && ox >= 0 && oy < d.OH && ox < d.OW) {
            int64_t idx = (((int64_t)b0 * d.OC + oc) * d.OH + oy) * d.OW
                          + ox;
            v = dy[idx];
            if constexpr (MASK) v = ymask[idx] > 0.f ? v : 0.f;
          }
        }
        if (wtrow) {
          const int ky = cy + kyi * d.S, kx = cx + kxi * d.S;
          wv = wtrow[(int64_t)oc * d.KH * d.KW + ky * d.KW + kx];
        }
      }
      va[e] = v;
      vb[e] = wv;
      if (++kxi == KWc) { kxi = 0; if (++kyi == KHc) { kyi = 0; ++oc; } }
    }
  };
  load_chunk(0);
  for (int k0 = 0; k0 < Kc; k0 += BK) {
#pragma unroll
    for (int e = 0; e < EL; ++e) {
      lds_put<BF16>(xs, row, c00 + e, va[e]);
      lds_put<BF16>(ws, row, c00 + e, vb[e]);
    }
    if (k0 + BK < Kc) load_chunk(k0 + BK);
    __syncthreads();
    mma_tiles<BF16>(xs, ws, acc, lane, wrow, wcol);
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = bm0 + wrow + mi * 16 + crow + r;
        int ic = bn0 + wcol + ni * 16 + ccol;
        if (m < Mc && ic < d.IC) {
          const int px = m % IWc, t1 = m / IWc;
          const int py = t1 % IHc, b = t1 / IHc;
          const int iy = cy + py * d.S, ix = cx + px * d.S;
          dx[(((int64_t)b * d.IC + ic) * d.IH + iy) * d.IW + ix] =
              acc[mi][ni][r];
        }
      }
}

// ---------------------------------------------------------------------------
// conv wgrad: dW[oc, k] = sum_m dYeff[m, oc] im2col[m, k]; db fused.
// Reduction over M; tiles: rows=oc (64), cols=k (64), i-chunks of BK.
// ---------------------------------------------------------------------------

struct ConvWP {
  const float* dy; const float* ymask; const float* x; float* part;
};

template <bool BF16, bool MASK>
__global__ __launch_bounds__(256)
void conv_wgrad_kernel(ConvWP p0, ConvWP p1, ConvDims d, int m_chunk,
                       int split) {
  // blockIdx.z = slab * nz + z
  const int nz = (p1.dy != nullptr) ? 2 : 1;
  const int zz = (int)blockIdx.z % nz;
  const int slab = (int)blockIdx.z / nz;
  const ConvWP& pp = zz ? p1 : p0;
  const float* dy = pp.dy;
  const float* ymask = pp.ymask;
  const float* x = pp.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bn0 = blockIdx.x * TB;   // oc rows
  const int bk0 = blockIdx.y * TB;   // k cols
  const int M = d.B * d.OH * d.OW;
  const int K = d.IC * d.KH * d.KW;
  const int m_lo = slab * m_chunk;
  const int m_hi = min(M, m_lo + m_chunk);
  float* dw_p = pp.part + (int64_t)slab * ((int64_t)d.OC * K + d.OC);
  float* db_p = dw_p + (int64_t)d.OC * K;
  (void)split;
  constexpr int BK = BF16 ? BKB : BKF;
  constexpr int EL = BF16 ? 16 : 4;
  constexpr int LBYTES = BF16 ? (64 * LDB * 2) : (64 * LDF * 4);
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  __shared__ float dbs[64];
  if (tid < 64) dbs[tid] = 0.f;
  f32x4 acc[2][2] = {};

  // coalesced staging (round 2): 16 lanes share a ROW (oc for the A
  // tile, k for the B tile) and read 16 CONSECUTIVE m elements — for
  // dy that is contiguous memory and for im2col stride-S runs, i.e.
  // a handful of 64B lines per instruction instead of the old
  // one-row-per-lane map's 64 scattered lines (same fix as fused.hip's
  // wstage_bf16; the conv wgrad gather was the visual update's largest
  // kernel at 53 us/call).
  const int rr = tid >> 4;           // 4 row-groups of 16 rows
  const int cc = tid & 15;           // consecutive i within the chunk
  KDec kds[4];
  MDec mds[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int k_my = bk0 + rr + 16 * p;
    kds[p] = kdec(k_my < K ? k_my : 0, d);
  }
  for (int i0 = m_lo; i0 < m_hi; i0 += BK) {
#pragma unroll
    for (int q = 0; q < (BK / 16); ++q) {
      int m = i0 + cc + 16 * q;
      mds[q & 3] = mdec(m < M ? m : 0, d);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int arow = rr + 16 * p;
      const int oc_my = bn0 + arow;
      const int k_my = bk0 + arow;
      const KDec& kd = kds[p];
#pragma unroll
      for (int q = 0; q < (BK / 16); ++q) {
        const int i = cc + 16 * q;
        const int m = i0 + i;
        const MDec& md = mds[q & 3];
        // A tile: as[oc][i] = dYeff[m, oc_my]
        float va = 0.f;
        if (m < m_hi && oc_my < d.OC) {
          int64_t idx = (((int64_t)md.b * d.OC + oc_my) * d.OH + md.oy)
                            * d.OW + md.ox;
          va = dy[idx];
          if constexpr (MASK) va = ymask[idx] > 0.f ? va : 0.f;
        }
        lds_put<BF16>(smem, arow, i, va);
        // B tile: bs[k][i] = im2col[m, k_my]
        float vb = 0.f;
        if (m < m_hi && k_my < K) {
          int iy = md.oy * d.S + kd.ky, ix = md.ox * d.S + kd.kx;
          vb = x[(((int64_t)md.b * d.IC + kd.ic) * d.IH + iy) * d.IW
                 + ix];
        }
        lds_put<BF16>(smem + LBYTES, arow, i, vb);
      }
    }
    __syncthreads();
    mma_tiles<BF16>(smem, smem + LBYTES, acc, lane, wrow, wcol);
    if (blockIdx.y == 0 && tid < 64) {
      float sm = 0.f;
      if constexpr (BF16) {
        const __bf16* as = (const __bf16*)smem;
        for (int i = 0; i < BKB; ++i) sm += (float)as[tid * LDB + i];
      } else {
        const float* as = (const float*)smem;
        for (int i = 0; i < BKF; ++i) sm += as[tid * LDF + i];
      }
      dbs[tid] += sm;
    }
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int oc = bn0 + wrow + mi * 16 + crow + r;
        int k = bk0 + wcol + ni * 16 + ccol;
        if (oc < d.OC && k < K) dw_p[(int64_t)oc * K + k] = acc[mi][ni][r];
      }
  if (blockIdx.y == 0 && tid < 64 && bn0 + tid < d.OC)
    db_p[bn0 + tid] = dbs[tid];
}

// Shared-input twin wgrad: both critics read the SAME im2col (the twin
// critics see one image batch), so each block stages the x-tile ONCE
// and runs both problems' MFMAs against it — the scattered im2col
// gather is the kernel's dominant cost and it halves.
// grid: (tiles_oc, tiles_k, split); both problems per block.
template <bool BF16, bool MASK>
__global__ __launch_bounds__(256)
void conv_wgrad2s_kernel(ConvWP p0, ConvWP p1, ConvDims d, int m_chunk,
                         int split) {
  const int slab = (int)blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bn0 = blockIdx.x * TB;
  const int bk0 = blockIdx.y * TB;
  const int M = d.B * d.OH * d.OW;
  const int K = d.IC * d.KH * d.KW;
  const int m_lo = slab * m_chunk;
  const int m_hi = min(M, m_lo + m_chunk);
  const int64_t per = (int64_t)d.OC * K + d.OC;
  float* dw_p0 = p0.part + (int64_t)slab * per;
  float* db_p0 = dw_p0 + (int64_t)d.OC * K;
  float* dw_p1 = p1.part + (int64_t)slab * per;
  float* db_p1 = dw_p1 + (int64_t)d.OC * K;
  (void)split;
  constexpr int BK = BF16 ? BKB : BKF;
  constexpr int EL = BF16 ? 16 : 4;
  constexpr int LBYTES = BF16 ? (64 * LDB * 2) : (64 * LDF * 4);
  __shared__ __attribute__((aligned(16))) char smem[3 * LBYTES];
  __shared__ float dbs0[64], dbs1[64];
  if (tid < 64) { dbs0[tid] = 0.f; dbs1[tid] = 0.f; }
  f32x4 acc0[2][2] = {}, acc1[2][2] = {};

  // coalesced staging: 16 lanes share a row, consecutive m (see the
  // conv_wgrad_kernel comment)
  const int rr = tid >> 4;
  const int cc = tid & 15;
  KDec kds[4];
  MDec mds[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int k_my = bk0 + rr + 16 * p;
    kds[p] = kdec(k_my < K ? k_my : 0, d);
  }
  for (int i0 = m_lo; i0 < m_hi; i0 += BK) {
#pragma unroll
    for (int q = 0; q < (BK / 16); ++q) {
      int m = i0 + cc + 16 * q;
      mds[q & 3] = mdec(m < M ? m : 0, d);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int arow = rr + 16 * p;
      const int oc_my = bn0 + arow;
      const int k_my = bk0 + arow;
      const KDec& kd = kds[p];
#pragma unroll
      for (int q = 0; q < (BK / 16); ++q) {
        const int i = cc + 16 * q;
        const int m = i0 + i;
        const MDec& md = mds[q & 3];
        float va0 = 0.f, va1 = 0.f, vb = 0.f;
        if (m < m_hi) {
          if (oc_my < d.OC) {
            int64_t idx = (((int64_t)md.b * d.OC + oc_my) * d.OH + md.oy)
                              * d.OW + md.ox;
            va0 = p0.dy[idx];
            va1 = p1.dy[idx];
            if constexpr (MASK) {
              va0 = p0.ymask[idx] > 0.f ? va0 : 0.f;
              va1 = p1.ymask[idx] > 0.f ? va1 : 0.f;
            }
          }
          if (k_my < K) {
            int iy = md.oy * d.S + kd.ky, ix = md.ox * d.S + kd.kx;
            vb = p0.x[(((int64_t)md.b * d.IC + kd.ic) * d.IH + iy) * d.IW
                      + ix];
          }
        }
        lds_put<BF16>(smem, arow, i, va0);
        lds_put<BF16>(smem + LBYTES, arow, i, va1);
        lds_put<BF16>(smem + 2 * LBYTES, arow, i, vb);
      }
    }
    __syncthreads();
    mma_tiles<BF16>(smem, smem + 2 * LBYTES, acc0, lane, wrow, wcol);
    mma_tiles<BF16>(smem + LBYTES, smem + 2 * LBYTES, acc1, lane, wrow,
                    wcol);
    if (blockIdx.y == 0 && tid < 64) {
      float s0 = 0.f, s1 = 0.f;
      if constexpr (BF16) {
        const __bf16* a0 = (const __bf16*)smem;
        const __bf16* a1 = (const __bf16*)(smem + LBYTES);
        for (int i = 0; i < BKB; ++i) {
          s0 += (float)a0[tid * LDB + i];
          s1 += (float)a1[tid * LDB + i];
        }
      } else {
        const float* a0 = (const float*)smem;
        const float* a1 = (const float*)(smem + LBYTES);
        for (int i = 0; i < BKF; ++i) {
          s0 += a0[tid * LDF + i];
          s1 += a1[tid * LDF + i];
        }
      }
      dbs0[tid] += s0;
      dbs1[tid] += s1;
    }
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int oc = bn0 + wrow + mi * 16 + crow + r;
        int k = bk0 + wcol + ni * 16 + ccol;
        if (oc < d.OC && k < K) {
          dw_p0[(int64_t)oc * K + k] = acc0[mi][ni][r];
          dw_p1[(int64_t)oc * K + k] = acc1[mi][ni][r];
        }
      }
  if (blockIdx.y == 0 && tid < 64 && bn0 + tid < d.OC) {
    db_p0[bn0 + tid] = dbs0[tid];
    db_p1[bn0 + tid] = dbs1[tid];
  }
}

// ---------------------------------------------------------------------------
// Fused B=1 conv trunk for the ACTING path: conv1+ReLU -> conv2+ReLU ->
// conv3+ReLU in ONE persistent workgroup, activations staged in LDS.
// The captured act graph otherwise replays three tile-GEMM conv kernels
// at batch 1 (57 us of serial latency, measured r02k) — at B=1 this is
// GEMV-shaped work: scalar VALU MACs with the image resident in LDS and
// per-wave-broadcast weight reads beat idle MFMA tiles.
// LDS budget: input 3x84x84 (84 KB) + act1 32x20x20 (51 KB) = 135 KB
// peak (<= 160 KB); act2 reuses the input region.
// ---------------------------------------------------------------------------

// One layer of the B=1 trunk, GEMV-style on one CU.  The binding limit
// of a naive per-MAC LDS read is LDS throughput (~32 floats/clk/CU for
// ds_read_b32: the 7 MFLOP trunk would move 28 MB through the LDS
// port).  Register blocking fixes it: each loaded input tap feeds OCB
// output channels (weights are wave-uniform scalar-cache loads) and
// each weight feeds PXB pixels, so LDS traffic drops by OCB and the
// independent accumulators give ILP.  KK (compile-time kernel width)
// lets the tap loops fully unroll.  Work items (oc-group x px-chunk)
// round-robin over the block's waves.
template <int OCB, int PXB, int KK>
DEVINL void conv_b1_layer(const float* __restrict__ src,
                          const float* __restrict__ w,
                          const float* __restrict__ b,
                          float* __restrict__ dst, const ConvDims& d,
                          int wid, int lane, int nw) {
  const int npx = d.OH * d.OW;
  const int KW = KK, KH = KK;
  const int IKK = d.IC * KH * KW;
  const int n_ocg = (d.OC + OCB - 1) / OCB;
  const int n_pxc = (npx + 64 * PXB - 1) / (64 * PXB);
  const int n_items = n_ocg * n_pxc;
  for (int item = wid; item < n_items; item += nw) {
    const int ocg = item / n_pxc;
    const int pxc = item - ocg * n_pxc;
    const int oc0 = ocg * OCB;
    const float* wr[OCB];
#pragma unroll
    for (int ob = 0; ob < OCB; ++ob)
      wr[ob] = w + (int64_t)min(oc0 + ob, d.OC - 1) * IKK;
    float acc[PXB][OCB];
    int oy[PXB], ox[PXB];
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb) {
      int px = pxc * 64 * PXB + pb * 64 + lane;
      if (px >= npx) px = 0;   // duplicate px 0; write is guarded
      oy[pb] = px / d.OW;
      ox[pb] = px - oy[pb] * d.OW;
#pragma unroll
      for (int ob = 0; ob < OCB; ++ob)
        acc[pb][ob] = b ? b[min(oc0 + ob, d.OC - 1)] : 0.f;
    }
    int k = 0;
    for (int ic = 0; ic < d.IC; ++ic) {
      const float* ipc = src + ic * d.IH * d.IW;
#pragma unroll
      for (int ky = 0; ky < KH; ++ky) {
#pragma unroll
        for (int kx = 0; kx < KW; ++kx, ++k) {
          float iv[PXB];
#pragma unroll
          for (int pb = 0; pb < PXB; ++pb)
            iv[pb] = ipc[(oy[pb] * d.S + ky) * d.IW + ox[pb] * d.S + kx];
#pragma unroll
          for (int ob = 0; ob < OCB; ++ob) {
            const float wv = wr[ob][k];
#pragma unroll
            for (int pb = 0; pb < PXB; ++pb)
              acc[pb][ob] += iv[pb] * wv;
          }
        }
      }
    }
#pragma unroll
    for (int pb = 0; pb < PXB; ++pb) {
      const int px = pxc * 64 * PXB + pb * 64 + lane;
      if (px >= npx) continue;
#pragma unroll
      for (int ob = 0; ob < OCB; ++ob) {
        const int oc = oc0 + ob;
        if (oc < d.OC) dst[oc * npx + px] = fmaxf(acc[pb][ob], 0.f);
      }
    }
  }
}

__global__ __launch_bounds__(1024)
void visual_trunk_b1_kernel(const float* __restrict__ x,
                            const float* __restrict__ w1,
                            const float* __restrict__ b1,
                            const float* __restrict__ w2,
                            const float* __restrict__ b2,
                            const float* __restrict__ w3,
                            const float* __restrict__ b3,
                            float* __restrict__ out,
                            ConvDims d1, ConvDims d2, ConvDims d3,
                            int a2_off) {
  __shared__ __attribute__((aligned(16))) float lds[40960];  // 160 KB
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;

  float* in = lds;                                   // 3*IH*IW
  const int in_n = d1.IC * d1.IH * d1.IW;
  float* a1 = lds + in_n;                            // 32*OH1*OW1
  const int a1_n = d1.OC * d1.OH * d1.OW;
  // layer 2 writes a2 while it still reads a1, so the two must not
  // overlap: a2 reuses the input slab when it fits there (a2_off = 0),
  // else the host places it behind a1
  float* a2 = lds + a2_off;

  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int nw = nthr >> 6;

  for (int i = tid; i < in_n; i += nthr) in[i] = x[i];
  __syncthreads();

  conv_b1_layer<8, 2, 8>(in, w1, b1, a1, d1, wid, lane, nw);
  __syncthreads();
  conv_b1_layer<8, 1, 4>(a1, w2, b2, a2, d2, wid, lane, nw);
  __syncthreads();
  conv_b1_layer<4, 1, 3>(a2, w3, b3, out, d3, wid, lane, nw);
}

// deterministic slab combine: dw[i] = sum_z part[z][i]; db likewise
__global__ __launch_bounds__(256)
void wgrad_combine_kernel(const float* __restrict__ part,
                          float* __restrict__ dw, float* __restrict__ db,
                          int64_t dw_n, int64_t oc_n, int n_slabs) {
  const int64_t total = dw_n + oc_n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    float s = 0.f;
    for (int z = 0; z < n_slabs; ++z) s += part[(int64_t)z * total + i];
    if (i < dw_n) dw[i] = s;
    else if (db) db[i - dw_n] = s;
  }
}

// both problems' combines in ONE launch (parts: [z][slab][per])
__global__ __launch_bounds__(256)
void wgrad_combine2_kernel(const float* __restrict__ p0,
                           const float* __restrict__ p1,
                           float* __restrict__ dw0, float* __restrict__ db0,
                           float* __restrict__ dw1, float* __restrict__ db1,
                           int64_t dw_n, int64_t oc_n, int n_slabs) {
  const int64_t per = dw_n + oc_n;
  const int64_t total = 2 * per;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    const int zz = (int)(i / per);
    const int64_t off = i % per;
    const float* part = zz ? p1 : p0;
    float s = 0.f;
    for (int z = 0; z < n_slabs; ++z) s += part[(int64_t)z * per + off];
    float* dw = zz ? dw1 : dw0;
    float* db = zz ? db1 : db0;
    if (off < dw_n) dw[off] = s;
    else if (db) db[off - dw_n] = s;
  }
}

// ---------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------

inline hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

extern bool* g_bf16_flag2;

ConvDims dims_of(const torch::Tensor& x, const torch::Tensor& w, int64_t s) {
  ConvDims d;
  d.B = (int)x.size(0); d.IC = (int)x.size(1);
  d.IH = (int)x.size(2); d.IW = (int)x.size(3);
  d.OC = (int)w.size(0); d.KH = (int)w.size(2); d.KW = (int)w.size(3);
  d.S = (int)s;
  d.OH = (d.IH - d.KH) / d.S + 1;
  d.OW = (d.IW - d.KW) / d.S + 1;
  return d;
}

std::vector<torch::Tensor> conv2d_fwd_multi(
    std::vector<torch::Tensor> xs, std::vector<torch::Tensor> ws,
    std::vector<c10::optional<torch::Tensor>> biases, int64_t s,
    bool relu) {
  const int nz = (int)xs.size();
  TORCH_CHECK(nz >= 1 && nz <= 4);
  auto d = dims_of(xs[0], ws[0], s);
  std::vector<torch::Tensor> ys;
  ConvQ q{};
  for (int z = 0; z < nz; ++z) {
    ys.push_back(torch::empty({d.B, d.OC, d.OH, d.OW}, xs[z].options()));
    q.p[z] = ConvP{xs[z].data_ptr<float>(), ws[z].data_ptr<float>(),
                   biases[z].has_value() ? biases[z]->data_ptr<float>()
                                         : nullptr,
                   ys[z].data_ptr<float>()};
  }
  const int M = d.B * d.OH * d.OW;
  for (int z = 0; z < nz; ++z)
    TORCH_CHECK(xs[z].numel() < INT32_MAX, "conv fwd: 32-bit indexing");
  const bool bf16 = *g_bf16_flag2;
  // LDS-subimage variant (TAC_AMD_CONV_LDS=1): per-image m tiles; each
  // block stages its input window rows once (coalesced) and builds the
  // im2col tile from LDS.  MEASURED NEGATIVE at the batch-64 visual
  // shapes (677 vs 699 updates/s cheetah, 854 vs 870 wall-runner,
  // gpurun_out/r02o): the per-image tiling adds ~58% more blocks with
  // partially-idle tails and the slab staging costs more than the LDS
  // locality saves — these kernels are launch/latency-floor-bound, not
  // gather-bound, at B=64.  Kept for larger batches / re-evaluation.
  static int lds_env = []{
    const char* e = getenv("TAC_AMD_CONV_LDS");
    return e ? atoi(e) : 0;
  }();
  const bool known = d.KW == d.KH
      && ((d.KW == 8 && d.S == 4) || (d.KW == 4 && d.S == 2)
          || (d.KW == 3 && d.S == 1));
  const int rows_max = std::min(d.IH, ((TB - 1) / d.OW + 1) * d.S + d.KH);
  const bool slab_ok = d.IC * rows_max * d.IW <= SLAB_F;
  if (lds_env == 1 && known && slab_ok) {
    const int tiles_img = (d.OH * d.OW + TB - 1) / TB;
    dim3 grid(d.B * tiles_img, (d.OC + TB - 1) / TB, nz);
    auto L2 = [&](auto b16, auto rl) {
      auto LS = [&](auto tk, auto ts) {
        hipLaunchKernelGGL((conv_fwd_lds_kernel<decltype(b16)::value,
                                                decltype(rl)::value,
                                                decltype(tk)::value,
                                                decltype(ts)::value>),
                           grid, dim3(256), 0, stream(), q, d, tiles_img);
      };
      if (d.KW == 8)
        LS(std::integral_constant<int, 8>{},
           std::integral_constant<int, 4>{});
      else if (d.KW == 4)
        LS(std::integral_constant<int, 4>{},
           std::integral_constant<int, 2>{});
      else
        LS(std::integral_constant<int, 3>{},
           std::integral_constant<int, 1>{});
    };
    if (bf16) { if (relu) L2(std::true_type{}, std::true_type{});
                else L2(std::true_type{}, std::false_type{}); }
    else      { if (relu) L2(std::false_type{}, std::true_type{});
                else L2(std::false_type{}, std::false_type{}); }
    return ys;
  }
  dim3 grid((M + TB - 1) / TB, (d.OC + TB - 1) / TB, nz);
  auto L = [&](auto b16, auto rl) {
    auto LS = [&](auto tk, auto ts) {
      hipLaunchKernelGGL((conv_fwd_kernel<decltype(b16)::value,
                                          decltype(rl)::value,
                                          decltype(tk)::value,
                                          decltype(ts)::value>),
                         grid, dim3(256), 0, stream(), q, d);
    };
    using i0 = std::integral_constant<int, 0>;
    if (d.KW == d.KH && d.KW == 8 && d.S == 4)
      LS(std::integral_constant<int, 8>{}, std::integral_constant<int, 4>{});
    else if (d.KW == d.KH && d.KW == 4 && d.S == 2)
      LS(std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{});
    else if (d.KW == d.KH && d.KW == 3 && d.S == 1)
      LS(std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{});
    else
      LS(i0{}, i0{});
  };
  if (bf16) { if (relu) L(std::true_type{}, std::true_type{});
              else L(std::true_type{}, std::false_type{}); }
  else      { if (relu) L(std::false_type{}, std::true_type{});
              else L(std::false_type{}, std::false_type{}); }
  return ys;
}

torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias, int64_t s,
                         bool relu) {
  return conv2d_fwd_multi({x}, {w}, {bias}, s, relu)[0];
}

std::vector<torch::Tensor> conv2d_dgrad_multi(
    std::vector<torch::Tensor> dys,
    std::vector<c10::optional<torch::Tensor>> ymasks,
    std::vector<torch::Tensor> wts, torch::Tensor x_like,
    torch::Tensor w, int64_t s) {
  const int nz = (int)dys.size();
  TORCH_CHECK(nz >= 1 && nz <= 2);
  auto d = dims_of(x_like, w, s);
  std::vector<torch::Tensor> dxs;
  ConvGP p[2] = {};
  const bool mask = ymasks[0].has_value();
  for (int z = 0; z < nz; ++z) {
    dxs.push_back(torch::empty_like(x_like));
    p[z] = ConvGP{dys[z].data_ptr<float>(),
                  ymasks[z].has_value() ? ymasks[z]->data_ptr<float>()
                                        : nullptr,
                  wts[z].data_ptr<float>(), dxs[z].data_ptr<float>()};
  }
  const bool bf16 = *g_bf16_flag2;
  if (d.S > 1) {
    // stride-class decomposition: dense taps per class (no predicated
    // zeros), S^2 classes fan out over blockIdx.z
    const int IHc = (d.IH + d.S - 1) / d.S;   // class (0,0) is largest
    const int IWc = (d.IW + d.S - 1) / d.S;
    const int Mc = d.B * IHc * IWc;
    dim3 grid((Mc + TB - 1) / TB, (d.IC + TB - 1) / TB,
              nz * d.S * d.S);
    auto L = [&](auto b16, auto mk) {
      hipLaunchKernelGGL((conv_dgrad_cls_kernel<decltype(b16)::value,
                                                decltype(mk)::value>),
                         grid, dim3(256), 0, stream(), p[0], p[1], d, nz);
    };
    if (bf16) { if (mask) L(std::true_type{}, std::true_type{});
                else L(std::true_type{}, std::false_type{}); }
    else      { if (mask) L(std::false_type{}, std::true_type{});
                else L(std::false_type{}, std::false_type{}); }
    return dxs;
  }
  const int M = d.B * d.IH * d.IW;
  dim3 grid((M + TB - 1) / TB, (d.IC + TB - 1) / TB, nz);
  auto L = [&](auto b16, auto mk) {
    hipLaunchKernelGGL((conv_dgrad_kernel<decltype(b16)::value,
                                          decltype(mk)::value>),
                       grid, dim3(256), 0, stream(), p[0], p[1], d);
  };
  if (bf16) { if (mask) L(std::true_type{}, std::true_type{});
              else L(std::true_type{}, std::false_type{}); }
  else      { if (mask) L(std::false_type{}, std::true_type{});
              else L(std::false_type{}, std::false_type{}); }
  return dxs;
}

torch::Tensor conv2d_dgrad(torch::Tensor dy,
                           c10::optional<torch::Tensor> ymask,
                           torch::Tensor wt, torch::Tensor x_like,
                           torch::Tensor w, int64_t s) {
  return conv2d_dgrad_multi({dy}, {ymask}, {wt}, x_like, w, s)[0];
}

std::vector<torch::Tensor> conv2d_wgrad_multi(
    std::vector<torch::Tensor> dys,
    std::vector<c10::optional<torch::Tensor>> ymasks,
    std::vector<torch::Tensor> xs, torch::Tensor w, int64_t s,
    std::vector<torch::Tensor> out) {
  const int nz = (int)dys.size();
  TORCH_CHECK(nz >= 1 && nz <= 2);
  TORCH_CHECK(out.empty() || (int)out.size() == 2 * nz,
              "out must be [dw0, db0[, dw1, db1]]");
  auto d = dims_of(xs[0], w, s);
  const int K = d.IC * d.KH * d.KW;
  const int M = d.B * d.OH * d.OW;
  // twin critics share the image batch: one x-tile stage serves both
  // problems (conv_wgrad2s_kernel)
  const bool shared = nz == 2 && xs[0].data_ptr() == xs[1].data_ptr();
  const int tiles = ((d.OC + TB - 1) / TB) * ((K + TB - 1) / TB)
                    * (shared ? 1 : nz);
  const int BKc = 64;
  int max_split = (M + BKc - 1) / BKc;
  int split = std::max(1, std::min({max_split,
                                    (256 + tiles - 1) / tiles, 64}));
  int m_chunk = ((M + split - 1) / split + BKc - 1) / BKc * BKc;
  split = (M + m_chunk - 1) / m_chunk;
  const int64_t per = (int64_t)d.OC * K + d.OC;
  const bool mask = ymasks[0].has_value();
  std::vector<torch::Tensor> outs;   // dw0, db0[, dw1, db1]
  std::vector<torch::Tensor> parts;
  ConvWP p[2] = {};
  for (int z = 0; z < nz; ++z) {
    if (out.empty()) {
      outs.push_back(torch::empty_like(w));
      outs.push_back(torch::empty({d.OC}, w.options()));
    } else {
      outs.push_back(out[2 * z]);
      outs.push_back(out[2 * z + 1]);
    }
    parts.push_back(torch::empty({split, per}, w.options()));
    p[z] = ConvWP{dys[z].data_ptr<float>(),
                  ymasks[z].has_value() ? ymasks[z]->data_ptr<float>()
                                        : nullptr,
                  xs[z].data_ptr<float>(), parts[z].data_ptr<float>()};
  }
  dim3 grid((d.OC + TB - 1) / TB, (K + TB - 1) / TB,
            (shared ? 1 : nz) * split);
  const bool bf16 = *g_bf16_flag2;
  auto L = [&](auto b16, auto mk) {
    if (shared)
      hipLaunchKernelGGL((conv_wgrad2s_kernel<decltype(b16)::value,
                                              decltype(mk)::value>),
                         grid, dim3(256), 0, stream(), p[0], p[1], d,
                         m_chunk, split);
    else
      hipLaunchKernelGGL((conv_wgrad_kernel<decltype(b16)::value,
                                            decltype(mk)::value>),
                         grid, dim3(256), 0, stream(), p[0], p[1], d,
                         m_chunk, split);
  };
  if (bf16) { if (mask) L(std::true_type{}, std::true_type{});
              else L(std::true_type{}, std::false_type{}); }
  else      { if (mask) L(std::false_type{}, std::true_type{});
              else L(std::false_type{}, std::false_type{}); }
  int64_t dw_n = (int64_t)d.OC * K;
  int blocks = (int)std::min<int64_t>((per * nz + 255) / 256, 512);
  if (nz == 2) {
    hipLaunchKernelGGL(wgrad_combine2_kernel, dim3(blocks), dim3(256), 0,
                       stream(), parts[0].data_ptr<float>(),
                       parts[1].data_ptr<float>(),
                       outs[0].data_ptr<float>(),
                       outs[1].data_ptr<float>(),
                       outs[2].data_ptr<float>(),
                       outs[3].data_ptr<float>(), dw_n,
                       (int64_t)d.OC, split);
  } else {
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(blocks), dim3(256), 0,
                       stream(), parts[0].data_ptr<float>(),
                       outs[0].data_ptr<float>(),
                       outs[1].data_ptr<float>(), dw_n,
                       (int64_t)d.OC, split);
  }
  return outs;
}

torch::Tensor visual_trunk_b1(torch::Tensor x, torch::Tensor w1,
                              c10::optional<torch::Tensor> b1,
                              torch::Tensor w2,
                              c10::optional<torch::Tensor> b2,
                              torch::Tensor w3,
                              c10::optional<torch::Tensor> b3,
                              int64_t s1, int64_t s2, int64_t s3) {
  TORCH_CHECK(x.dim() == 3, "visual_trunk_b1: unbatched CHW frame");
  auto x4 = x.unsqueeze(0);
  auto d1 = dims_of(x4, w1, s1);
  auto y1 = torch::empty({1, d1.OC, d1.OH, d1.OW}, x.options());
  auto d2 = dims_of(y1, w2, s2);
  auto y2 = torch::empty({1, d2.OC, d2.OH, d2.OW}, x.options());
  auto d3 = dims_of(y2, w3, s3);
  const int in_n = d1.IC * d1.IH * d1.IW;
  const int a1_n = d1.OC * d1.OH * d1.OW;
  const int a2_n = d2.OC * d2.OH * d2.OW;
  // a1 lives at [in_n, in_n + a1_n); a2 must stay clear of it
  const int a2_off = a2_n <= in_n ? 0 : in_n + a1_n;
  TORCH_CHECK(in_n + a1_n <= 40960 && a2_off + a2_n <= 40960,
              "visual_trunk_b1: activations exceed the 160 KB LDS plan");
  TORCH_CHECK(d1.KH == 8 && d2.KH == 4 && d3.KH == 3 &&
              d1.KW == 8 && d2.KW == 4 && d3.KW == 3,
              "visual_trunk_b1: compiled for the 8/4/3 kernel family");
  auto out = torch::empty({(int64_t)d3.OC * d3.OH * d3.OW}, x.options());
  auto bp = [](const c10::optional<torch::Tensor>& t) {
    return t.has_value() ? t->data_ptr<float>() : nullptr;
  };
  hipLaunchKernelGGL(visual_trunk_b1_kernel, dim3(1), dim3(1024), 0,
                     stream(), x.data_ptr<float>(), w1.data_ptr<float>(),
                     bp(b1), w2.data_ptr<float>(), bp(b2),
                     w3.data_ptr<float>(), bp(b3), out.data_ptr<float>(),
                     d1, d2, d3, a2_off);
  return out;
}

std::vector<torch::Tensor> conv2d_wgrad(torch::Tensor dy,
                                        c10::optional<torch::Tensor> ymask,
                                        torch::Tensor x, torch::Tensor w,
                                        int64_t s) {
  auto o = conv2d_wgrad_multi({dy}, {ymask}, {x}, w, s, {});
  return {o[0], o[1]};
}

}  // namespace convk

namespace convk { bool* g_bf16_flag2 = nullptr; }

void set_conv_bf16_flag(bool* p) { convk::g_bf16_flag2 = p; }

void register_conv(pybind11::module_& m) {
  m.def("conv2d_fwd", &convk::conv2d_fwd);
  m.def("conv2d_dgrad", &convk::conv2d_dgrad);
  m.def("conv2d_wgrad", &convk::conv2d_wgrad);
  m.def("conv2d_fwd_multi", &convk::conv2d_fwd_multi);
  m.def("conv2d_dgrad_multi", &convk::conv2d_dgrad_multi);
  m.def("visual_trunk_b1", &convk::visual_trunk_b1);
  m.def("conv2d_wgrad_multi", &convk::conv2d_wgrad_multi,
        pybind11::arg("dys"), pybind11::arg("ymasks"), pybind11::arg("xs"),
        pybind11::arg("w"), pybind11::arg("s"),
        pybind11::arg("out") = std::vector<torch::Tensor>{});
}
