// Fused SAC update engine kernels (gfx950 / CDNA4).
//
// The profiled autograd update path spends 75% of its time in GEMM
// kernels with scalar staging and ~50 of its 112 kernels on autograd
// bookkeeping (profiles/r01_baseline_update_profile.md).  These kernels
// implement a hand-scheduled update pass (driven by
// torch_actor_critic_amd/algo/engine.py) with:
//   * multi-problem GEMMs: both twin critics (or both policy heads) in
//     ONE launch via blockIdx.z;
//   * lda/ldy strides so operands read/write slices of concat-layout
//     buffers — torch.cat disappears from the update entirely;
//   * cached transposed weights (refreshed once per Adam step) so dgrad
//     is a coalesced fwd-form GEMM;
//   * vectorized (float4 -> bf16x8) LDS staging on aligned interiors;
//   * wgrad writing straight into the module's flat gradient slices
//     (no autograd accumulation);
//   * device-side alpha (learned entropy temperature) read by the loss
//     kernels and updated in-graph — per BASELINE.json's north star the
//     whole update (sample, twin-min Bellman, tanh-Gaussian sample,
//     entropy-temperature loss, polyak) replays as one hipGraph.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <pybind11/numpy.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "act_sync.h"
#include "replay_draw.h"

namespace fused {

using namespace replay;

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// Debug/test helper: the raw Philox words of subsequences clo0 ..
// clo0 + n - 1 as this translation unit compiled the generator.
__global__ __launch_bounds__(256)
void philox_words2_kernel(int64_t* __restrict__ out, uint64_t seed,
                          uint64_t chi, uint64_t clo0, int64_t n) {
  philox_words_row(out, seed, chi, clo0, n);
}

// ---------------------------------------------------------------------------
// Multi-problem MFMA GEMM (fwd-form): y = act(x @ w^T + b), x optionally
// relu-masked by `mask` (backward chain), optional second (x2,w2,mask2)
// accumulated into the same output (dgrad-sum over the twin critics /
// the two policy heads).
// ---------------------------------------------------------------------------

struct MProb {
  const float* x; const float* w; const float* bias; float* y;
  const float* mask;
  const float* x2; const float* w2; const float* mask2;
  // rank-1 A operand (R1 kernels): x[row][col] = r1_col[row] * r1_row[col]
  // formed in registers while staging, x itself is never read
  const float* r1_col;   // [M]
  const float* r1_row;   // [K], 16-byte aligned
};

constexpr int MAXZ = 4;

struct MGemm {
  MProb p[MAXZ];
  int M, N, K, lda, ldy;
  int K2;  // reduction depth of the second operand pair (SUM2)
  // split-K (skinny-M shapes, e.g. the visual 3136->512 dense layer:
  // an un-split launch is 8 workgroups on 256 CUs).  blockIdx.z =
  // slab*nz + z; slabs write raw partials, the combine kernel sums
  // deterministically and applies bias/ReLU.
  int nz, k_chunk;
  float* part;  // [split*nz][M*N] partials, or null (no split)
};

constexpr int TB = 64;        // block tile (M and N)
constexpr int BKB2 = 64;      // bf16 K-step (wgrad staging path)
constexpr int BKF2 = 16;      // fp32 K-step
constexpr int LDSB2 = 72;     // bf16 LDS halves per row (BKB2 tiles)
constexpr int LDSF2 = 17;     // fp32 LDS floats per row
// pipelined mgemm uses a deeper bf16 K-step (fewer serial tiles)
constexpr int BKP = 128;      // bf16 K-step (mgemm pipelined path)
constexpr int LDSP = 136;     // halves per row: stride 68 dwords -> 4r mod 64
                              // distinct over a 16-lane group, conflict-free

// Stage a 64 x BK tile of `src` (row-major, leading dim ld, rows base
// `r0`, cols base `k0`, bounds R x C) into LDS, optionally masked.
template <bool BF16, bool MASK>
DEVINL void stage_tile(void* lds, const float* src, const float* mask,
                       int r0, int k0, int R, int C, int ld) {
  const int tid = threadIdx.x;
  const int row = tid & 63;
  if constexpr (BF16) {
    __bf16* d = (__bf16*)lds;
    const int c0 = (tid >> 6) * 16;
    const int gr = r0 + row;
    bool interior = (r0 + 64 <= R) && (k0 + 64 <= C) && ((ld & 3) == 0)
                    && ((k0 & 3) == 0);
    if (interior) {
      const float* p = src + (int64_t)gr * ld + k0 + c0;
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 f = *(const float4*)(p + q * 4);
        v[q * 4 + 0] = f.x; v[q * 4 + 1] = f.y;
        v[q * 4 + 2] = f.z; v[q * 4 + 3] = f.w;
      }
      if constexpr (MASK) {
        const float* mp = mask + (int64_t)gr * ld + k0 + c0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float4 f = *(const float4*)(mp + q * 4);
          v[q * 4 + 0] = f.x > 0.f ? v[q * 4 + 0] : 0.f;
          v[q * 4 + 1] = f.y > 0.f ? v[q * 4 + 1] : 0.f;
          v[q * 4 + 2] = f.z > 0.f ? v[q * 4 + 2] : 0.f;
          v[q * 4 + 3] = f.w > 0.f ? v[q * 4 + 3] : 0.f;
        }
      }
      union { __bf16 h[16]; uint4 u[2]; } pk;
#pragma unroll
      for (int e = 0; e < 16; ++e) pk.h[e] = (__bf16)v[e];
      uint4* dst = (uint4*)&d[row * LDSB2 + c0];
      dst[0] = pk.u[0];
      dst[1] = pk.u[1];
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        int c = c0 + e;
        float v = 0.f;
        if (gr < R && k0 + c < C) {
          v = src[(int64_t)gr * ld + k0 + c];
          if constexpr (MASK) {
            v = mask[(int64_t)gr * ld + k0 + c] > 0.f ? v : 0.f;
          }
        }
        d[row * LDSB2 + c] = (__bf16)v;
      }
    }
  } else {
    float* d = (float*)lds;
    const int c0 = (tid >> 6) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int c = c0 + e;
      int gr = r0 + row;
      float v = 0.f;
      if (gr < R && k0 + c < C) {
        v = src[(int64_t)gr * ld + k0 + c];
        if constexpr (MASK) {
          v = mask[(int64_t)gr * ld + k0 + c] > 0.f ? v : 0.f;
        }
      }
      d[row * LDSF2 + c] = v;
    }
  }
}

template <bool BF16>
DEVINL void mma_tiles(const void* xs_, const void* ws_, f32x4 (&acc)[2][2],
                      int lane, int wrow, int wcol) {
  if constexpr (BF16) {
    const __bf16* xs = (const __bf16*)xs_;
    const __bf16* ws = (const __bf16*)ws_;
    const int arow = lane & 15;
    const int ak0 = (lane >> 4) * 8;
#pragma unroll
    for (int kk = 0; kk < BKB2; kk += 32) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        bf16x8 a = *(const bf16x8*)&xs[(wrow + mi * 16 + arow) * LDSB2
                                       + kk + ak0];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          bf16x8 b = *(const bf16x8*)&ws[(wcol + ni * 16 + arow) * LDSB2
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
    for (int kk = 0; kk < BKF2; kk += 4) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        float a = xs[(wrow + mi * 16 + arow) * LDSF2 + kk + akl];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          float b = ws[(wcol + ni * 16 + arow) * LDSF2 + kk + akl];
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a, b, acc[mi][ni], 0, 0, 0);
        }
      }
    }
  }
}

// ---- pipelined register staging (T14: write LDS, issue next tile's
// global loads, barrier, MFMA — HBM/L2 latency hides under the MFMAs) --

// Coalesced 64×BKP tile staging (bf16 pipelined path).  Thread→element
// mapping is chosen so each wavefront's load instruction touches FEW
// 64-byte lines (measured round 2: the old one-row-per-lane layout made
// every float4 instruction hit 64 distinct lines, and odd lda (e.g. the
// 393-wide Humanoid concat) fell back to fully scalar gathers — the
// large-batch GEMMs were bound by the per-CU L2 request rate, not
// bytes; FETCH_SIZE showed the re-reads L2-resident).
//
//  * aligned rows (ld%4==0): thread t = 4 lanes per row, row = t>>2,
//    lane c = t&3 reads float4 at col (q*4+c)*4 — the 4 lanes of a row
//    cover one contiguous 64B line per instruction (16 lines/wave
//    instead of 64);
//  * any ld: 16 lanes per row read consecutive dwords — 4 lines/wave
//    per instruction instead of 64 scalar-scattered.
// R1: the tile element is the fp32 product r1c[row] * r1r[col] (same
// thread→element map, same masking, one rounding at the LDS write); src
// is unused.
template <bool BF16, bool MASK, bool R1 = false>
DEVINL void load_tile_regs(float* v, const float* src, const float* mask,
                           int r0, int k0, int R, int C, int ld,
                           const float* r1c = nullptr,
                           const float* r1r = nullptr) {
  const int tid = threadIdx.x;
  if constexpr (BF16) {
    bool interior = (r0 + 64 <= R) && (k0 + BKP <= C) && ((ld & 3) == 0);
    if (interior) {
      const int row = tid >> 2;          // 4 lanes per row
      const int c = tid & 3;
      if constexpr (R1) {
        const float a = r1c[r0 + row];
        const float* p = r1r + k0 + c * 4;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float4 f = *(const float4*)(p + q * 16);
          v[q*4+0]=a*f.x; v[q*4+1]=a*f.y; v[q*4+2]=a*f.z; v[q*4+3]=a*f.w;
        }
      } else {
        const float* p = src + (int64_t)(r0 + row) * ld + k0 + c * 4;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float4 f = *(const float4*)(p + q * 16);
          v[q*4+0]=f.x; v[q*4+1]=f.y; v[q*4+2]=f.z; v[q*4+3]=f.w;
        }
      }
      if constexpr (MASK) {
        const float* mp = mask + (int64_t)(r0 + row) * ld + k0 + c * 4;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float4 f = *(const float4*)(mp + q * 16);
          v[q*4+0] = f.x > 0.f ? v[q*4+0] : 0.f;
          v[q*4+1] = f.y > 0.f ? v[q*4+1] : 0.f;
          v[q*4+2] = f.z > 0.f ? v[q*4+2] : 0.f;
          v[q*4+3] = f.w > 0.f ? v[q*4+3] : 0.f;
        }
      }
    } else {
      // row-grouped dword fallback: 16 consecutive lanes share a row
      const int rr = tid >> 4;           // 16 row-groups of 16 lanes
      const int cc = tid & 15;
#pragma unroll
      for (int p = 0; p < 4; ++p) {      // rows rr, rr+16, rr+32, rr+48
        const int gr = r0 + rr + 16 * p;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = k0 + cc + 16 * q;
          float val = 0.f;
          if (gr < R && c < C) {
            if constexpr (R1) val = r1c[gr] * r1r[c];
            else val = src[(int64_t)gr * ld + c];
            if constexpr (MASK)
              val = mask[(int64_t)gr * ld + c] > 0.f ? val : 0.f;
          }
          v[p * 8 + q] = val;
        }
      }
    }
  } else {
    const int row = tid & 63;
    const int gr = r0 + row;
    const int c0 = (tid >> 6) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int c = k0 + c0 + e;
      float val = 0.f;
      if (gr < R && c < C) {
        if constexpr (R1) val = r1c[gr] * r1r[c];
        else val = src[(int64_t)gr * ld + c];
        if constexpr (MASK)
          val = mask[(int64_t)gr * ld + c] > 0.f ? val : 0.f;
      }
      v[e] = val;
    }
  }
}

// LDS write matching load_tile_regs' thread→element mapping.  The LDS
// CONTENT layout (row*LDSP + col bf16) is unchanged — only which thread
// writes which element differs, so mma_tiles_p is untouched.  The two
// load layouts place different elements in v, so the writer needs the
// same interior predicate; pass the SAME r0/k0/R/C/ld.
template <bool BF16>
DEVINL void write_tile_lds(void* lds, const float* v,
                           int r0, int k0, int R, int C, int ld) {
  const int tid = threadIdx.x;
  if constexpr (BF16) {
    __bf16* d = (__bf16*)lds;
    bool interior = (r0 + 64 <= R) && (k0 + BKP <= C) && ((ld & 3) == 0);
    if (interior) {
      const int row = tid >> 2;
      const int c = tid & 3;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        union { __bf16 h[4]; uint2 u; } pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) pk.h[j] = (__bf16)v[q * 4 + j];
        *(uint2*)&d[row * LDSP + (q * 4 + c) * 4] = pk.u;
      }
    } else {
      const int rr = tid >> 4;
      const int cc = tid & 15;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q)
          d[(rr + 16 * p) * LDSP + cc + 16 * q] = (__bf16)v[p * 8 + q];
    }
  } else {
    float* d = (float*)lds;
    const int row = tid & 63;
    const int c0 = (tid >> 6) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[row * LDSF2 + c0 + e] = v[e];
  }
}

template <bool BF16>
DEVINL void mma_tiles_p(const void* xs_, const void* ws_,
                        f32x4 (&acc)[2][2], int lane, int wrow, int wcol) {
  if constexpr (BF16) {
    const __bf16* xs = (const __bf16*)xs_;
    const __bf16* ws = (const __bf16*)ws_;
    const int arow = lane & 15;
    const int ak0 = (lane >> 4) * 8;
#pragma unroll
    for (int kk = 0; kk < BKP; kk += 32) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        bf16x8 a = *(const bf16x8*)&xs[(wrow + mi * 16 + arow) * LDSP
                                       + kk + ak0];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          bf16x8 b = *(const bf16x8*)&ws[(wcol + ni * 16 + arow) * LDSP
                                         + kk + ak0];
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, b, acc[mi][ni], 0, 0, 0);
        }
      }
    }
  } else {
    mma_tiles<false>(xs_, ws_, acc, lane, wrow, wcol);
  }
}

template <bool BF16, bool MASK, bool R1 = false>
DEVINL void gemm_pass(const float* x, const float* w, const float* mask,
                      int M, int N, int K, int lda, int ldw,
                      void* xs, void* ws,
                      int bm0, int bn0, int lane, int wrow, int wcol,
                      int tid, f32x4 (&acc)[2][2],
                      const float* r1c = nullptr,
                      const float* r1r = nullptr) {
  constexpr int BK = BF16 ? BKP : BKF2;
  constexpr int EL = BF16 ? 32 : 4;
  float va[EL], vb[EL];
  (void)tid;
  load_tile_regs<BF16, MASK, R1>(va, x, mask, bm0, 0, M, K, lda, r1c, r1r);
  load_tile_regs<BF16, false>(vb, w, nullptr, bn0, 0, N, K, ldw);
  for (int k0 = 0; k0 < K; k0 += BK) {
    write_tile_lds<BF16>(xs, va, bm0, k0, M, K, lda);
    write_tile_lds<BF16>(ws, vb, bn0, k0, N, K, ldw);
    if (k0 + BK < K) {
      load_tile_regs<BF16, MASK, R1>(va, x, mask, bm0, k0 + BK, M, K, lda,
                                     r1c, r1r);
      load_tile_regs<BF16, false>(vb, w, nullptr, bn0, k0 + BK, N, K,
                                  ldw);
    }
    __syncthreads();
    mma_tiles_p<BF16>(xs, ws, acc, lane, wrow, wcol);
    __syncthreads();
  }
}

// N-tile-reuse pass (large-M shapes): ONE staged A tile serves NT
// 64-wide B sub-tiles per K-step, cutting the A operand's VMEM traffic
// by NT×.  Measured motivation (gpurun_out/r02q trace): at Humanoid
// B=4096 the 64×64-tile launches re-stage the 6.4 MB A operand once per
// N-tile and per problem — ~256 MB of fp32 traffic per launch against
// ~14 MB of distinct bytes, making the six forward GEMMs 48% of the
// update.  B stays per-K-step fresh-staged (weights are L2-resident);
// the NEXT A tile prefetches into a second register set before the B
// stages so its latency hides under them.
template <bool BF16, bool MASK, int NT>
DEVINL void gemm_pass_nt(const float* x, const float* w, const float* mask,
                         int M, int N, int K, int lda, int ldw,
                         void* xs, char* ws0, int lbytes,
                         int bm0, int bn0, int lane, int wrow, int wcol,
                         f32x4 (&acc)[NT][2][2]) {
  constexpr int BK = BF16 ? BKP : BKF2;
  constexpr int EL = BF16 ? 32 : 4;
  float va[EL], va2[EL], vb[EL];
  load_tile_regs<BF16, MASK>(va, x, mask, bm0, 0, M, K, lda);
  for (int k0 = 0; k0 < K; k0 += BK) {
    write_tile_lds<BF16>(xs, va, bm0, k0, M, K, lda);
    if (k0 + BK < K)
      load_tile_regs<BF16, MASK>(va2, x, mask, bm0, k0 + BK, M, K, lda);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      load_tile_regs<BF16, false>(vb, w, nullptr, bn0 + t * TB, k0, N, K,
                                  ldw);
      write_tile_lds<BF16>(ws0 + (int64_t)t * lbytes, vb, bn0 + t * TB,
                           k0, N, K, ldw);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
      mma_tiles_p<BF16>(xs, ws0 + (int64_t)t * lbytes, acc[t], lane, wrow,
                        wcol);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EL; ++e) va[e] = va2[e];
  }
}

template <bool BF16, bool MASK, bool RELU, bool SUM2, int NT>
__global__ __launch_bounds__(256)
void mgemm_nt_kernel(MGemm g) {
  const int zz = (int)blockIdx.z;
  const MProb& p = g.p[zz];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bm0 = blockIdx.x * TB;
  const int bn0 = blockIdx.y * (TB * NT);
  constexpr int LBYTES = BF16 ? (64 * LDSP * 2) : (64 * LDSF2 * 4);
  __shared__ __attribute__((aligned(16))) char smem[(1 + NT) * LBYTES];
  void* xs = smem;
  char* ws0 = smem + LBYTES;

  f32x4 acc[NT][2][2] = {};
  gemm_pass_nt<BF16, MASK, NT>(p.x, p.w, p.mask, g.M, g.N, g.K, g.lda,
                               g.K, xs, ws0, LBYTES, bm0, bn0, lane, wrow,
                               wcol, acc);
  if constexpr (SUM2) {
    gemm_pass_nt<BF16, MASK, NT>(p.x2, p.w2, p.mask2, g.M, g.N, g.K2,
                                 g.K2, g.K2, xs, ws0, LBYTES, bm0, bn0,
                                 lane, wrow, wcol, acc);
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int grow = bm0 + wrow + mi * 16 + crow + r;
          int gcol = bn0 + t * TB + wcol + ni * 16 + ccol;
          if (grow < g.M && gcol < g.N) {
            float v = acc[t][mi][ni][r];
            if (p.bias) v += p.bias[gcol];
            if constexpr (RELU) v = fmaxf(v, 0.f);
            p.y[(int64_t)grow * g.ldy + gcol] = v;
          }
        }
}

template <bool BF16, bool MASK, bool RELU, bool SUM2, bool R1 = false>
__global__ __launch_bounds__(256)
void mgemm_kernel(MGemm g) {
  const int zz = g.part ? ((int)blockIdx.z % g.nz) : (int)blockIdx.z;
  const int slab = g.part ? ((int)blockIdx.z / g.nz) : 0;
  const MProb& p = g.p[zz];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int bm0 = blockIdx.x * TB;
  const int bn0 = blockIdx.y * TB;
  constexpr int LBYTES = BF16 ? (64 * LDSP * 2) : (64 * LDSF2 * 4);
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  void* xs = smem;
  void* ws = smem + LBYTES;

  const int k_lo = slab * g.k_chunk;
  const int k_len = g.part ? min(g.K - k_lo, g.k_chunk) : g.K;

  f32x4 acc[2][2] = {};
  if constexpr (R1)   // never split-K (host gate): k_lo = 0
    gemm_pass<BF16, MASK, true>(nullptr, p.w, p.mask, g.M, g.N, g.K, g.lda,
                                g.K, xs, ws, bm0, bn0, lane, wrow, wcol,
                                tid, acc, p.r1_col, p.r1_row);
  else
    gemm_pass<BF16, MASK>(p.x + k_lo, p.w + k_lo,
                          p.mask ? p.mask + k_lo : nullptr,
                          g.M, g.N, k_len, g.lda, g.K, xs, ws,
                          bm0, bn0, lane, wrow, wcol, tid, acc);
  if constexpr (SUM2) {  // split-K never combines with SUM2 (host gate)
    gemm_pass<BF16, MASK>(p.x2, p.w2, p.mask2, g.M, g.N, g.K2, g.K2,
                          g.K2, xs, ws, bm0, bn0, lane, wrow, wcol, tid,
                          acc);
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
  float* part_out = g.part
      ? g.part + (int64_t)((int64_t)slab * g.nz + zz) * g.M * g.N
      : nullptr;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int grow = bm0 + wrow + mi * 16 + crow + r;
        int gcol = bn0 + wcol + ni * 16 + ccol;
        if (grow < g.M && gcol < g.N) {
          float v = acc[mi][ni][r];
          if (part_out) {  // raw partial; epilogue runs in the combine
            part_out[(int64_t)grow * g.N + gcol] = v;
            continue;
          }
          if (p.bias) v += p.bias[gcol];
          if constexpr (RELU) v = fmaxf(v, 0.f);
          p.y[(int64_t)grow * g.ldy + gcol] = v;
        }
      }
}

// deterministic split-K combine: y = act(sum_slab part + bias)
__global__ __launch_bounds__(256)
void mgemm_combine_kernel(MGemm g, int split, bool relu) {
  const int64_t per = (int64_t)g.M * g.N;
  const int64_t total = per * g.nz;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    const int z = (int)(i / per);
    const int64_t off = i % per;
    float s = 0.f;
    for (int sl = 0; sl < split; ++sl)
      s += g.part[((int64_t)sl * g.nz + z) * per + off];
    const MProb& p = g.p[z];
    const int m = (int)(off / g.N), n = (int)(off % g.N);
    if (p.bias) s += p.bias[n];
    if (relu) s = fmaxf(s, 0.f);
    p.y[(int64_t)m * g.ldy + n] = s;
  }
}

// ---------------------------------------------------------------------------
// SAC loss rows and their block reduction, shared by the single-block loss
// kernels (qloss2 / piloss2) and by the small-shape GEMM that forms a loss
// gradient column while staging (mgemm_small_kernel's LF modes).  The roundings
// are spelled out the way the loss kernels have always compiled (one fused
// multiply-add per row, nothing else contracted), so every kernel that
// inlines these gives the same bits whatever surrounds the call.
// ---------------------------------------------------------------------------

struct QRow { float g1, g2, sq; };   // dq1, dq2, e1^2 + e2^2

DEVINL QRow qloss_row(float q1, float q2, float q1t, float q2t, float lpn,
                      float rew, float done, float alpha, float gamma,
                      float scale, int B) {
#pragma clang fp contract(off)
  const float soft = __builtin_fmaf(-alpha, lpn, fminf(q1t, q2t));
  const float backup = scale * rew + gamma * (1.f - done) * soft;
  const float e1 = q1 - backup, e2 = q2 - backup;
  QRow r;
  r.sq = e1 * e1 + e2 * e2;
  r.g1 = 2.f * e1 / B;
  r.g2 = 2.f * e2 / B;
  return r;
}

struct PiRow { float g1, g2, s; };   // dqp1, dqp2, alpha logp - min(q1, q2)

DEVINL PiRow piloss_row(float q1, float q2, float lp, float alpha, int B) {
#pragma clang fp contract(off)
  PiRow r;
  r.s = __builtin_fmaf(alpha, lp, -fminf(q1, q2));
  float g1, g2;
  if (q1 < q2)      { g1 = -1.f; g2 = 0.f; }
  else if (q2 < q1) { g1 = 0.f;  g2 = -1.f; }
  else              { g1 = -0.5f; g2 = -0.5f; }
  r.g1 = g1 / B;
  r.g2 = g2 / B;
  return r;
}

struct QIn {
  const float* q1; const float* q2; const float* q1t; const float* q2t;
  const float* lpn; const float* rew; const float* done;
};

// one row's loss inputs (the pi-loss uses q1, q2 and lpn = logp)
struct QVals { float q1, q2, q1t, q2t, lpn, rew, done; };

DEVINL QVals qvals_load(const QIn& in, int i) {
  return QVals{in.q1[i], in.q2[i], in.q1t[i], in.q2t[i], in.lpn[i],
               in.rew[i], in.done[i]};
}

// strided per-thread sums over the whole batch: load(i) gives row i's
// inputs (from memory, or from registers filled ahead of time), each(i,
// row) sees every row
template <class L, class F>
DEVINL float qloss_rows(L&& load, float alpha, float gamma, float scale,
                        int B, F&& each) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const QVals v = load(i);
    const QRow r = qloss_row(v.q1, v.q2, v.q1t, v.q2t, v.lpn, v.rew, v.done,
                             alpha, gamma, scale, B);
    acc += r.sq;
    each(i, r);
  }
  return acc;
}

template <class L, class F>
DEVINL void piloss_rows(float (&acc)[2], L&& load, float alpha, int B,
                        F&& each) {
#pragma clang fp contract(off)
  acc[0] = 0.f;
  acc[1] = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const QVals v = load(i);
    const PiRow r = piloss_row(v.q1, v.q2, v.lpn, alpha, B);
    acc[0] += r.s;
    acc[1] += v.lpn;
    each(i, r);
  }
}

// block means of N per-thread sums (256 threads): 64-lane shuffle, one
// partial per wave through red[n][0..3], summed in wave order, / B.  Holds
// a barrier, so the whole block calls it.
template <int N>
DEVINL void loss_block_mean(float (&acc)[N], float (*red)[4], int B) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] += __shfl_down(acc[n], off);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) red[n][threadIdx.x >> 6] = acc[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n)
    acc[n] = (red[n][0] + red[n][1] + red[n][2] + red[n][3]) / B;
}

// ---------------------------------------------------------------------------
// Small-shape mgemm (bf16 compute, M <= 128, K <= 256, K2 <= 256): the
// batch-64 update's GEMMs are latency-bound, not throughput-bound.  The
// pipelined kernel above walks K in 128-wide steps with a dependent
// global round trip per step and a third one for the bias; here every
// global load of the block (A, mask, W, the SUM2 pair, bias) is issued
// before the first wait, the whole K extent is converted into LDS behind
// ONE barrier, and the MFMA chain runs over it.  Tiles are TM x TN
// (template) so a 64-row problem spreads over more CUs.
//
// Same bits as mgemm_kernel<true, ...>: identical LDS content layout
// (element k of a row at column k), identical lane -> fragment map,
// K-chunks of 32 ascending from a zero accumulator, operand 1 then the
// SUM2 operand, one fp32 -> bf16 rounding per operand, fp32 bias add and
// ReLU after the chain.  K is zero-padded to 32 (the kernel above pads to
// 128; its extra all-zero chunks add exact zeros).
// ---------------------------------------------------------------------------

constexpr int SKMAX = 256;   // host gate: K <= SKMAX and K2 <= SKMAX
constexpr int SLPAD = 8;     // row stride = Kp + 8 halves: (16k + 4) dwords,
                             // 16 consecutive rows land in distinct banks

// 4-lanes-per-row float4 form: aligned rows wholly inside the operand.
DEVINL bool small_vec_ok(const float* src, const float* mask, int r0, int R,
                         int bound, int K, int ld) {
  return (r0 + R <= bound) && ((ld & 3) == 0) && ((K & 3) == 0)
         && ((((uintptr_t)src | (uintptr_t)mask) & 15) == 0);
}

// Issue all global loads of an R x K tile (rows r0.., bound `bound`) into
// registers; nothing here waits on a load.  Out-of-range lanes read a
// clamped (valid) address and are zeroed by small_write.
//  * vec:   4 lanes x float4 per row; R = 32 splits K over two row sets
//  * !vec:  16 lanes x dword per row, rows rr + 16p
// LF != 0 (computed rank-1 column, see LossFold): the caller fills ra.
template <int R, bool MASK, bool R1, int LF = 0>
DEVINL void small_load(float (&v)[R], float (&mk)[MASK ? R : 1],
                       float (&ra)[R / 16], bool vec,
                       const float* src, const float* mask,
                       int r0, int bound, int K, int ld,
                       const float* r1c, const float* r1r) {
  const int tid = threadIdx.x;
  if (vec) {
    constexpr int G = 64 / R;
    constexpr int NQ = SKMAX / 16 / G;
    const int gr = r0 + ((tid >> 2) & (R - 1));
    const int kg = (tid >> 2) / R;
    const int c = tid & 3;
    if constexpr (R1 && LF == 0) ra[0] = r1c[gr];
    const float* base = R1 ? r1r : src + (int64_t)gr * ld;
    const float* mbase = MASK ? mask + (int64_t)gr * ld : nullptr;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q * G * 16 < K) {
        const int col = min(((q * G + kg) * 4 + c) * 4, K - 4);
        float4 f = *(const float4*)(base + col);
        v[q*4+0] = f.x; v[q*4+1] = f.y; v[q*4+2] = f.z; v[q*4+3] = f.w;
        if constexpr (MASK) {
          float4 h = *(const float4*)(mbase + col);
          mk[q*4+0] = h.x; mk[q*4+1] = h.y; mk[q*4+2] = h.z; mk[q*4+3] = h.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[q*4+j] = 0.f;
          if constexpr (MASK) mk[q*4+j] = 0.f;
        }
      }
    }
  } else {
    const int rr = tid >> 4;
    const int cc = tid & 15;
#pragma unroll
    for (int p = 0; p < R / 16; ++p) {
      const bool rows_in = r0 + 16 * p < bound;
      const int gr = min(r0 + rr + 16 * p, bound - 1);
      if constexpr (R1 && LF == 0) ra[p] = r1c[gr];
#pragma unroll
      for (int q = 0; q < SKMAX / 16; ++q) {
        if (rows_in && q * 16 < K) {
          const int col = min(cc + 16 * q, K - 1);
          if constexpr (R1) v[p*16+q] = r1r[col];
          else v[p*16+q] = src[(int64_t)gr * ld + col];
          if constexpr (MASK) mk[p*16+q] = mask[(int64_t)gr * ld + col];
        } else {
          v[p*16+q] = 0.f;
          if constexpr (MASK) mk[p*16+q] = 0.f;
        }
      }
    }
  }
}

// Convert a loaded tile and write it to LDS at columns [0, Kp) of `d`
// (row stride S halves), zero beyond the operand's bounds.  Same vec /
// r0 / bound / K as the matching small_load.
template <int R, bool MASK, bool R1>
DEVINL void small_write(__bf16* d, int S, const float (&v)[R],
                        const float (&mk)[MASK ? R : 1],
                        const float (&ra)[R / 16], bool vec,
                        int r0, int bound, int K, int Kp) {
  const int tid = threadIdx.x;
  if (vec) {
    constexpr int G = 64 / R;
    constexpr int NQ = SKMAX / 16 / G;
    const int row = (tid >> 2) & (R - 1);
    const int kg = (tid >> 2) / R;
    const int c = tid & 3;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q * G * 16 < Kp) {
        const int col = ((q * G + kg) * 4 + c) * 4;
        const bool in = col < K;
        union { __bf16 h[4]; uint2 u; } pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float x = v[q*4+j];
          if constexpr (R1) x = ra[0] * x;
          if constexpr (MASK) x = mk[q*4+j] > 0.f ? x : 0.f;
          pk.h[j] = (__bf16)(in ? x : 0.f);
        }
        *(uint2*)&d[row * S + col] = pk.u;
      }
    }
  } else {
    const int rr = tid >> 4;
    const int cc = tid & 15;
#pragma unroll
    for (int p = 0; p < R / 16; ++p) {
      const int row = rr + 16 * p;
      const bool row_in = r0 + row < bound;
#pragma unroll
      for (int q = 0; q < SKMAX / 16; ++q) {
        if (q * 16 < Kp) {
          const int col = cc + 16 * q;
          float x = v[p*16+q];
          if constexpr (R1) x = ra[p] * x;
          if constexpr (MASK) x = mk[p*16+q] > 0.f ? x : 0.f;
          d[row * S + col] = (__bf16)((row_in && col < K) ? x : 0.f);
        }
      }
    }
  }
}

// A rank-1 column that the GEMM computes itself instead of reading it: the
// SAC loss gradient dq_z (blockIdx.z = z, nz = 2) of each staged row, from
// the inputs of the loss kernel this launch replaces.  LF = 1: pi-loss
// (q1, q2, logp -> dqp_z, loss_acc, mean_logp), LF = 2: q-loss (all seven
// inputs -> dq_z, loss_acc, the counter commit).  The blockIdx.y == 0
// blocks also write their rows of dq_z, and under LF = 2 their rows of the
// unmasked fp32 outer product dq_z (x) row_z — what the K=1 GEMM that used
// to sit in front stored for the wgrad to read.  Block (0, 0, 0) alone runs
// the loss kernel's full-batch reduction; no other block reads what it
// writes.
struct LossFold {
  QIn in;                   // LF = 1 reads q1, q2 and lpn (= logp) only
  const float* alpha_dev; float alpha_host;
  float gamma, scale;
  float* loss_acc;
  float* mean_logp;         // LF = 1, may be null
  float* dq[2];             // [M] each
  float* outer[2];          // LF = 2: [M, K], 16-byte aligned
  int64_t* bump[3];         // LF = 2, each may be null
};

// What block (0, 0, 0) reads for the reduction, loaded with the block's
// other loads so the launch keeps its single memory round trip: the loss
// inputs of row threadIdx.x (B <= 128 < blockDim.x, so the shared strided
// loop visits no other row), and in thread 0 the accumulator and counters.
struct FoldPre { QVals v; float loss0; int64_t c[3]; };

template <int LF>
DEVINL void fold_preload(FoldPre& pre, const LossFold& lf, int B) {
  const int i = threadIdx.x;
  if (i < B) {
    pre.v.q1 = lf.in.q1[i];
    pre.v.q2 = lf.in.q2[i];
    pre.v.lpn = lf.in.lpn[i];
    if constexpr (LF == 2) {
      pre.v.q1t = lf.in.q1t[i];
      pre.v.q2t = lf.in.q2t[i];
      pre.v.rew = lf.in.rew[i];
      pre.v.done = lf.in.done[i];
    }
  }
  if (i == 0) {
    pre.loss0 = lf.loss_acc[0];
    if constexpr (LF == 2) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (lf.bump[j]) pre.c[j] = lf.bump[j][0];
    }
  }
}

// the loss kernel's reduction and scalar outputs, by one whole block
template <int LF>
DEVINL void fold_reduce(const FoldPre& pre, const LossFold& lf, float alpha,
                        int B) {
  __shared__ float red[2][4];
  auto load = [&](int) { return pre.v; };
  if constexpr (LF == 2) {
    float acc[1];
    acc[0] = qloss_rows(load, alpha, lf.gamma, lf.scale, B,
                        [](int, const QRow&) {});
    loss_block_mean<1>(acc, red, B);
    if (threadIdx.x == 0) {
      lf.loss_acc[0] = pre.loss0 + acc[0];
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (lf.bump[j]) lf.bump[j][0] = pre.c[j] + 1;
    }
  } else {
    float acc[2];
    piloss_rows(acc, load, alpha, B, [](int, const PiRow&) {});
    loss_block_mean<2>(acc, red, B);
    if (threadIdx.x == 0) {
      lf.loss_acc[0] = pre.loss0 + acc[0];
      if (lf.mean_logp) lf.mean_logp[0] = acc[1];
    }
  }
}

// Store an R x K tile of the unmasked fp32 products ra * v at the element
// map of small_write (same vec / r0 / bound / K); dst has row stride K.
template <int R>
DEVINL void fold_store_outer(float* dst, const float (&v)[R],
                             const float (&ra)[R / 16], bool vec, int r0,
                             int bound, int K) {
  const int tid = threadIdx.x;
  if (vec) {
    constexpr int G = 64 / R;
    constexpr int NQ = SKMAX / 16 / G;
    const int gr = r0 + ((tid >> 2) & (R - 1));
    const int kg = (tid >> 2) / R;
    const int c = tid & 3;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int col = ((q * G + kg) * 4 + c) * 4;
      if (q * G * 16 < K && col < K) {   // K % 4 == 0: whole float4 inside
        float4 f;
        // + 0: a zero-accumulator MFMA never returns -0
        f.x = ra[0] * v[q*4+0] + 0.f; f.y = ra[0] * v[q*4+1] + 0.f;
        f.z = ra[0] * v[q*4+2] + 0.f; f.w = ra[0] * v[q*4+3] + 0.f;
        *(float4*)(dst + (int64_t)gr * K + col) = f;
      }
    }
  } else {
    const int rr = tid >> 4;
    const int cc = tid & 15;
#pragma unroll
    for (int p = 0; p < R / 16; ++p) {
      const int gr = r0 + rr + 16 * p;
#pragma unroll
      for (int q = 0; q < SKMAX / 16; ++q) {
        const int col = cc + 16 * q;
        if (gr < bound && col < K)
          dst[(int64_t)gr * K + col] = ra[p] * v[p*16+q] + 0.f;
      }
    }
  }
}

DEVINL float bf16_round(float x) { return (float)(__bf16)x; }

DEVINL const LossFold& fold_arg(const LossFold& lf) { return lf; }

// LF != 0: masked R1 whose column is computed from loss inputs (1 pi, 2 q);
// the LossFold then travels as a second by-value argument.  LF = 0 has no
// such argument and compiles to what it was without the mode.
template <int TM, int TN, bool MASK, bool RELU, bool SUM2, bool R1,
          int LF = 0, class... Fold>
__global__ __launch_bounds__(256)
void mgemm_small_kernel(MGemm g, Fold... fold) {
  static_assert(sizeof...(Fold) == (LF != 0 ? 1 : 0), "one LossFold iff LF");
  static_assert((TM == 32 || TM == 64) && (TN == 32 || TN == 64), "tile");
  static_assert(!(SUM2 && R1), "R1 has no second operand");
  static_assert(LF == 0 || (R1 && MASK), "a computed column is an R1 column");
  constexpr int WM = TM / 2, WN = TN / 2;      // per-wave sub-tile
  constexpr int MI = WM / 16, NI = WN / 16;
  constexpr int KT = SUM2 ? 2 * SKMAX : SKMAX;
  __shared__ __attribute__((aligned(16))) __bf16 smem[(TM + TN)
                                                      * (KT + SLPAD)];
  const MProb& p = g.p[blockIdx.z];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * WM;
  const int wcol = (wid & 1) * WN;
  const int bm0 = blockIdx.x * TM;
  const int bn0 = blockIdx.y * TN;
  const int crow = (lane >> 4) * 4, ccol = lane & 15;

  const int Kp1 = (g.K + 31) & ~31;
  const int Kp2 = SUM2 ? ((g.K2 + 31) & ~31) : 0;
  const int S = Kp1 + Kp2 + SLPAD;
  __bf16* xs = smem;
  __bf16* ws = smem + TM * S;

  // every global load of the block, issued back to back
  float bv[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int gcol = bn0 + wcol + ni * 16 + ccol;
    bv[ni] = (p.bias && gcol < g.N) ? p.bias[gcol] : 0.f;
  }
  float va[TM], ma[MASK ? TM : 1], ra[TM / 16], vb[TN], nomask[1],
        rb[TN / 16];
  const float* a_src = R1 ? p.r1_row : p.x;
  const bool veca = small_vec_ok(a_src, MASK ? p.mask : nullptr, bm0, TM,
                                 g.M, g.K, g.lda);
  const bool vecb = small_vec_ok(p.w, nullptr, bn0, TN, g.N, g.K, g.K);
  small_load<TM, MASK, R1, LF>(va, ma, ra, veca, p.x, p.mask, bm0, g.M, g.K,
                               g.lda, p.r1_col, p.r1_row);
  // computed column: this thread's staged rows (small_load's row map) load
  // their loss inputs with everything else, ahead of the first wait
  constexpr int NFR = LF ? TM / 16 : 1;
  int frow[NFR];
  float fin[NFR][LF == 2 ? 7 : 2];
  float falpha = 0.f;
  FoldPre fpre = {};
  if constexpr (LF != 0) {
    const LossFold& lf = fold_arg(fold...);
    falpha = lf.alpha_dev ? lf.alpha_dev[0] : lf.alpha_host;
#pragma unroll
    for (int q = 0; q < NFR; ++q) {
      frow[q] = veca ? bm0 + ((tid >> 2) & (TM - 1))
                     : min(bm0 + (tid >> 4) + 16 * q, g.M - 1);
      fin[q][0] = lf.in.q1[frow[q]];
      fin[q][1] = lf.in.q2[frow[q]];
      if constexpr (LF == 2) {
        fin[q][2] = lf.in.q1t[frow[q]];
        fin[q][3] = lf.in.q2t[frow[q]];
        fin[q][4] = lf.in.lpn[frow[q]];
        fin[q][5] = lf.in.rew[frow[q]];
        fin[q][6] = lf.in.done[frow[q]];
      }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
      fold_preload<LF>(fpre, lf, g.M);
  }
  small_load<TN, false, false>(vb, nomask, rb, vecb, p.w, nullptr, bn0, g.N,
                               g.K, g.K, nullptr, nullptr);
  float va2[SUM2 ? TM : 1], ma2[(SUM2 && MASK) ? TM : 1], vb2[SUM2 ? TN : 1];
  bool veca2 = false, vecb2 = false;
  if constexpr (SUM2) {
    veca2 = small_vec_ok(p.x2, MASK ? p.mask2 : nullptr, bm0, TM, g.M, g.K2,
                         g.K2);
    vecb2 = small_vec_ok(p.w2, nullptr, bn0, TN, g.N, g.K2, g.K2);
    small_load<TM, MASK, false>(va2, ma2, ra, veca2, p.x2, p.mask2, bm0, g.M,
                                g.K2, g.K2, nullptr, nullptr);
    small_load<TN, false, false>(vb2, nomask, rb, vecb2, p.w2, nullptr, bn0,
                                 g.N, g.K2, g.K2, nullptr, nullptr);
  }

  if constexpr (LF != 0) {
    const LossFold& lf = fold_arg(fold...);
    const int z = blockIdx.z;
    // lanes that own column 0 of a staged row write that row's dq_z
    const bool wr = blockIdx.y == 0
                    && (veca ? (tid & 3) == 0 && (tid >> 2) / TM == 0
                             : (tid & 15) == 0);
#pragma unroll
    for (int q = 0; q < NFR; ++q) {
      float col;
      if constexpr (LF == 2) {
        const QRow r = qloss_row(fin[q][0], fin[q][1], fin[q][2], fin[q][3],
                                 fin[q][4], fin[q][5], fin[q][6], falpha,
                                 lf.gamma, lf.scale, g.M);
        col = z ? r.g2 : r.g1;
      } else {
        const PiRow r = piloss_row(fin[q][0], fin[q][1], 0.f, falpha, g.M);
        col = z ? r.g2 : r.g1;
      }
      const bool row_in = veca ? q == 0 : bm0 + (tid >> 4) + 16 * q < g.M;
      if (wr && row_in) lf.dq[z][frow[q]] = col;
      // LF = 2 reproduces a K=1 bf16 MFMA launch (which stored
      // bf16(dq) * bf16(w), exact in fp32) re-staged by the masked GEMM
      ra[q] = LF == 2 ? bf16_round(col) : col;
    }
    if constexpr (LF == 2) {
#pragma unroll
      for (int e = 0; e < TM; ++e) va[e] = bf16_round(va[e]);
      if (blockIdx.y == 0)
        fold_store_outer<TM>(lf.outer[z], va, ra, veca, bm0, g.M, g.K);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
      fold_reduce<LF>(fpre, lf, falpha, g.M);
  }
  small_write<TM, MASK, R1>(xs, S, va, ma, ra, veca, bm0, g.M, g.K, Kp1);
  small_write<TN, false, false>(ws, S, vb, nomask, rb, vecb, bn0, g.N, g.K,
                                Kp1);
  if constexpr (SUM2) {
    small_write<TM, MASK, false>(xs + Kp1, S, va2, ma2, ra, veca2, bm0, g.M,
                                 g.K2, Kp2);
    small_write<TN, false, false>(ws + Kp1, S, vb2, nomask, rb, vecb2, bn0,
                                  g.N, g.K2, Kp2);
  }
  __syncthreads();

  f32x4 acc[MI][NI] = {};
  const int arow = lane & 15;
  const int ak0 = (lane >> 4) * 8;
  const __bf16* xr = xs + (wrow + arow) * S + ak0;
  const __bf16* wr = ws + (wcol + arow) * S + ak0;
  const int Kt = Kp1 + Kp2;
  for (int kk = 0; kk < Kt; kk += 32) {
    bf16x8 b[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
      b[ni] = *(const bf16x8*)&wr[ni * 16 * S + kk];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      bf16x8 a = *(const bf16x8*)&xr[mi * 16 * S + kk];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, b[ni], acc[mi][ni], 0, 0, 0);
    }
  }

#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int grow = bm0 + wrow + mi * 16 + crow + r;
        const int gcol = bn0 + wcol + ni * 16 + ccol;
        if (grow < g.M && gcol < g.N) {
          float v = acc[mi][ni][r];
          if (p.bias) v += bv[ni];
          if constexpr (RELU) v = fmaxf(v, 0.f);
          p.y[(int64_t)grow * g.ldy + gcol] = v;
        }
      }
}

// ---------------------------------------------------------------------------
// The per-element Adam update, shared by adam_t_kernel and the wgrad
// epilogues that apply Adam to the gradient they just finished
// (mwgrad_het_adam): m, v, p and the optional polyak target at flat
// index i.  Returns the new parameter so the caller can also place it in
// a transposed-weight cache.
// ---------------------------------------------------------------------------

// arithmetic only: m and v are updated in place, the new parameter is
// returned.  Callers that own many elements load them all first, so the
// memory latencies overlap instead of chaining element by element.
DEVINL float adam_math(float g, float p, float& m, float& v, float lr,
                       float b1, float b2, float eps, float wd, float bc1,
                       float bc2) {
  // The roundings are spelled out (three fused multiply-adds, nothing
  // else contracted) so every kernel that inlines this gives the same
  // bits: left to the compiler, the choice varied with the surrounding
  // code, and a last-bit difference in m grows over bf16 updates.
#pragma clang fp contract(off)
  float gi = __builtin_fmaf(wd, p, g);
  float mi = __builtin_fmaf(b1, m, (1.f - b1) * gi);
  float vi = __builtin_fmaf(b2, v, ((1.f - b2) * gi) * gi);
  m = mi;
  v = vi;
  return p - lr / bc1 * mi / (sqrtf(vi / bc2) + eps);
}

// polyak target tracking of the post-Adam parameter — replaces the
// standalone polyak launch (reference semantics: the target averages
// the q_opt.step()-updated critic, and nothing mutates critic params
// between Adam and update_targets, sac/algorithm.py:139,278)
DEVINL float polyak_math(float targ, float pn, float rho) {
#pragma clang fp contract(off)
  return rho * targ + (1.f - rho) * pn;
}

DEVINL float adam_elem(float* __restrict__ p, float* __restrict__ m,
                       float* __restrict__ v, float* __restrict__ targ,
                       int64_t i, float g, float lr, float b1, float b2,
                       float eps, float wd, float bc1, float bc2,
                       float rho) {
  float mi = m[i], vi = v[i];
  const float pn = adam_math(g, p[i], mi, vi, lr, b1, b2, eps, wd, bc1,
                             bc2);
  m[i] = mi;
  v[i] = vi;
  p[i] = pn;
  if (targ) targ[i] = polyak_math(targ[i], pn, rho);
  return pn;
}

// Adam state for the wgrad kernels that update in their epilogue.  All
// pointers are flat-buffer bases; a problem's flat offset is
// dw - grad (db - grad for its bias).
constexpr int MAXW = 12;   // problems per heterogeneous wgrad launch
struct WAdam {
  float* p; float* m; float* v; float* targ;   // targ may be null
  const float* grad;
  const int64_t* step;
  float lr, b1, b2, eps, wd, rho;
  float* wt[MAXW];   // per-problem transposed-weight cache [K,N] or null
  int quarter;       // 1: four blocks per tile, a quarter epilogue each
                     // (host sets it only for single-K-step launches)
};

DEVINL float wadam_apply(const WAdam& ad, int64_t i, float g, float bc1,
                         float bc2) {
  return adam_elem(ad.p, ad.m, ad.v, ad.targ, i, g, ad.lr, ad.b1, ad.b2,
                   ad.eps, ad.wd, bc1, bc2, ad.rho);
}

// ---------------------------------------------------------------------------
// Multi-problem wgrad: dW[N,K] = sum_i dYeff[i,n] X[i,k]; db[N] fused.
// Coalesced global reads (contiguous along n / k), LDS-transposed writes.
// ---------------------------------------------------------------------------

struct WProb {
  const float* dy; const float* ymask; const float* x;
  float* dw; float* db;
};

struct WGemm {
  WProb p[2];
  int M, N, K, lddy, ldx;
  int nz, m_chunk;           // split-M: blockIdx.z = slab * nz + z
  float* part;               // [split][nz][N*K + N] partial slabs (or null)
};

// Coalesced transposed stage for the wgrad bodies: LDS content layout
// stays dst[c][i] (c = the 64-wide n/k slice, i = the 64-row m-chunk,
// stride LDSB2) but the thread→element map groups lanes so one load
// instruction touches few 64B lines (4 lanes × float4 per row when
// aligned = 16 lines/wave; 16-lane consecutive dwords otherwise = 4-8
// lines/wave) instead of the old 64-rows-per-instruction scatter.
template <bool MASK>
DEVINL void wstage_bf16(__bf16* dst, const float* __restrict__ src,
                        const float* __restrict__ msk,
                        int i0, int c0, int m_hi, int Cmax, int ld) {
  const int tid = threadIdx.x;
  const bool interior = (i0 + 64 <= m_hi) && (c0 + 64 <= Cmax)
                        && ((ld & 3) == 0) && ((c0 & 3) == 0);
  if (interior) {
    const int row = tid >> 2;        // i-row, 4 lanes each
    const int c = tid & 3;
    const float* p = src + (int64_t)(i0 + row) * ld + c0 + c * 4;
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 f = *(const float4*)(p + q * 16);
      v[q*4+0]=f.x; v[q*4+1]=f.y; v[q*4+2]=f.z; v[q*4+3]=f.w;
    }
    if constexpr (MASK) {
      const float* mp = msk + (int64_t)(i0 + row) * ld + c0 + c * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 f = *(const float4*)(mp + q * 16);
        v[q*4+0] = f.x > 0.f ? v[q*4+0] : 0.f;
        v[q*4+1] = f.y > 0.f ? v[q*4+1] : 0.f;
        v[q*4+2] = f.z > 0.f ? v[q*4+2] : 0.f;
        v[q*4+3] = f.w > 0.f ? v[q*4+3] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        dst[((q * 4 + c) * 4 + j) * LDSB2 + row] = (__bf16)v[q * 4 + j];
  } else {
    const int rr = tid >> 4;         // 16 lanes share an i-row
    const int cc = tid & 15;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int gi = i0 + rr + 16 * p;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gc = c0 + cc + 16 * q;
        float val = 0.f;
        if (gi < m_hi && gc < Cmax) {
          val = src[(int64_t)gi * ld + gc];
          if constexpr (MASK)
            val = msk[(int64_t)gi * ld + gc] > 0.f ? val : 0.f;
        }
        dst[(cc + 16 * q) * LDSB2 + rr + 16 * p] = (__bf16)val;
      }
    }
  }
}

// ADAM: with do_adam the tile epilogue also applies Adam to every
// (gn, gk) element it owns (`wt` = this problem's [K,N] transposed cache or
// null).  Hazard argument: the wgrad kernels read only dy, masks,
// activations and XC — never a weight, a W^T cache or the target
// buffer — and every flat element belongs to exactly one tile (host
// coverage gate), so writing p/m/v/target/W^T here cannot race within
// the kernel; the next reader is a later launch on the same stream.
// q >= 0 (WAdam::quarter): this block owns only the (mi, ni) =
// (q >> 1, q & 1) 16x16 sub-tile of every wave — four blocks share one
// 64x64 tile.  Adam's divisions and square root are ALU-heavy; on the few
// dozen blocks of a batch-64 phase they cost more than the adam_t launch
// they replace (measured 14 us against 5.2 + 5.7), so the epilogue is
// spread over 4x the blocks.  Each of the four blocks repeats the tile's
// whole staging + MFMA loop (so the gradient bits do not depend on q);
// that is only cheap when the loop is ONE K-step, and the launcher sets
// quarter for exactly that case.  Any longer un-split launch runs q = -1:
// one block per tile, all 16 elements per thread.
template <bool BF16, bool MASK, bool ADAM = false>
DEVINL void wgrad_tile_body(const float* __restrict__ dy,
                            const float* __restrict__ ymask,
                            const float* __restrict__ x,
                            float* __restrict__ dw_out,
                            float* __restrict__ db_out, bool has_db,
                            int M, int N, int K, int lddy, int ldx,
                            int m_lo, int m_hi, int bn0, int bk0,
                            char* smem, float* dbs,
                            const WAdam& ad = WAdam{}, bool do_adam = false,
                            float* __restrict__ wt = nullptr, int q = -1) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  constexpr int BK = BF16 ? BKB2 : BKF2;
  constexpr int LBYTES = BF16 ? (64 * LDSB2 * 2) : (64 * LDSF2 * 4);

  if (tid < 64) dbs[tid] = 0.f;
  f32x4 acc[2][2] = {};

  // ADAM: the optimizer state of all 16 owned elements is requested
  // before the staging loop, so its memory latency overlaps the dy/x
  // loads and the MFMAs instead of following them, and no load waits on
  // another element's store (the launch is a few dozen blocks: latency,
  // not bandwidth, is what the epilogue costs).
  float pv[2][2][4] = {}, mv[2][2][4] = {}, vv[2][2][4] = {},
        tv[2][2][4] = {};
  float bc1 = 1.f, bc2 = 1.f;
  if constexpr (ADAM) {
    if (do_adam) {
      const float t = (float)ad.step[0];
      bc1 = 1.f - powf(ad.b1, t);
      bc2 = 1.f - powf(ad.b2, t);
      const int64_t fo = dw_out - ad.grad;
      const int crow = (lane >> 4) * 4, ccol = lane & 15;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gn = bn0 + wrow + mi * 16 + crow + r;
            const int gk = bk0 + wcol + ni * 16 + ccol;
            const bool own = q < 0 || q == mi * 2 + ni;
            if (own && gn < N && gk < K) {
              const int64_t i = fo + (int64_t)gn * K + gk;
              pv[mi][ni][r] = ad.p[i];
              mv[mi][ni][r] = ad.m[i];
              vv[mi][ni][r] = ad.v[i];
              if (ad.targ) tv[mi][ni][r] = ad.targ[i];
            }
          }
    }
  }

  for (int i0 = m_lo; i0 < m_hi; i0 += BK) {
    // A tile: as[n][i] = dYeff[i0+i][bn0+n]; staged transposed.
    // thread: i = tid&(BK-1)... BK may be 16 (fp32): use i = tid % BK.
    {
      if constexpr (BF16) {
        wstage_bf16<MASK>((__bf16*)smem, dy, ymask, i0, bn0, m_hi, N,
                          lddy);
      } else {
        float* as = (float*)smem;
        const int ic = tid & 15;
        const int nc0 = (tid >> 4) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int n = bn0 + nc0 + e;
          int gi = i0 + ic;
          float val = 0.f;
          if (gi < m_hi && n < N) {
            val = dy[(int64_t)gi * lddy + n];
            if constexpr (MASK) {
              val = ymask[(int64_t)gi * lddy + n] > 0.f ? val : 0.f;
            }
          }
          as[(nc0 + e) * LDSF2 + ic] = val;
        }
      }
    }
    // B tile: bs[k][i] = X[i0+i][bk0+k]
    {
      if constexpr (BF16) {
        wstage_bf16<false>((__bf16*)(smem + LBYTES), x, nullptr, i0, bk0,
                           m_hi, K, ldx);
      } else {
        float* bs = (float*)(smem + LBYTES);
        const int ic = tid & 15;
        const int kc0 = (tid >> 4) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int k = bk0 + kc0 + e;
          int gi = i0 + ic;
          bs[(kc0 + e) * LDSF2 + ic] =
              (gi < m_hi && k < K) ? x[(int64_t)gi * ldx + k] : 0.f;
        }
      }
    }
    __syncthreads();
    mma_tiles<BF16>(smem, smem + LBYTES, acc, lane, wrow, wcol);
    // db: from the staged (already masked) A tile, k-tile-0 blocks only
    if (has_db && bk0 == 0 && tid < 64) {
      float s = 0.f;
      if constexpr (BF16) {
        const __bf16* as = (const __bf16*)smem;
        constexpr int NI = BKB2;
        for (int i = 0; i < NI; ++i) s += (float)as[tid * LDSB2 + i];
      } else {
        const float* as = (const float*)smem;
        for (int i = 0; i < BKF2; ++i) s += as[tid * LDSF2 + i];
      }
      dbs[tid] += s;
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
        int gn = bn0 + wrow + mi * 16 + crow + r;
        int gk = bk0 + wcol + ni * 16 + ccol;
        if (ADAM && q >= 0 && q != mi * 2 + ni) continue;
        if (gn < N && gk < K)
          dw_out[(int64_t)gn * K + gk] = acc[mi][ni][r];
      }
  if (ADAM && q > 0) db_out = nullptr;   // quarter 0 owns the bias
  if (db_out && bk0 == 0 && tid < 64 && bn0 + tid < N)
    db_out[bn0 + tid] = dbs[tid];
  if constexpr (ADAM) {
    if (!do_adam) return;   // split-M: the combine applies Adam
    const int64_t fo = dw_out - ad.grad;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int gn0 = bn0 + wrow + mi * 16 + crow;
        const int gk = bk0 + wcol + ni * 16 + ccol;
        if (gk >= K || (q >= 0 && q != mi * 2 + ni)) continue;
        float pn[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gn0 + r < N) {
            const int64_t i = fo + (int64_t)(gn0 + r) * K + gk;
            pn[r] = adam_math(acc[mi][ni][r], pv[mi][ni][r], mv[mi][ni][r],
                              vv[mi][ni][r], ad.lr, ad.b1, ad.b2, ad.eps,
                              ad.wd, bc1, bc2);
            ad.m[i] = mv[mi][ni][r];
            ad.v[i] = vv[mi][ni][r];
            ad.p[i] = pn[r];
            if (ad.targ)
              ad.targ[i] = polyak_math(tv[mi][ni][r], pn[r], ad.rho);
          }
        if (wt) {
          // the four r rows are consecutive gn: one 16-byte W^T store
          // where it is in bounds and aligned
          float* dst = wt + (int64_t)gk * N + gn0;
          if (gn0 + 3 < N && ((uintptr_t)dst & 15) == 0) {
            *(float4*)dst = make_float4(pn[0], pn[1], pn[2], pn[3]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (gn0 + r < N) dst[r] = pn[r];
          }
        }
      }
    if (db_out && bk0 == 0 && tid < 64 && bn0 + tid < N)
      wadam_apply(ad, (db_out - ad.grad) + bn0 + tid, dbs[tid], bc1, bc2);
  }
}

template <bool BF16, bool MASK>
__global__ __launch_bounds__(256)
void mwgrad_kernel(WGemm g) {
  constexpr int LBYTES = BF16 ? (64 * LDSB2 * 2) : (64 * LDSF2 * 4);
  __shared__ __attribute__((aligned(16))) char smem[2 * LBYTES];
  __shared__ float dbs[64];
  const int zz = (int)blockIdx.z % g.nz;
  const int slab = (int)blockIdx.z / g.nz;
  const WProb& p = g.p[zz];
  const int m_lo = slab * g.m_chunk;
  const int m_hi = min(g.M, m_lo + g.m_chunk);
  float* dw_out = p.dw;
  float* db_out = p.db;
  if (g.part) {
    float* base = g.part
        + ((int64_t)slab * g.nz + zz) * ((int64_t)g.N * g.K + g.N);
    dw_out = base;
    db_out = p.db ? base + (int64_t)g.N * g.K : nullptr;
  }
  wgrad_tile_body<BF16, MASK>(p.dy, p.ymask, p.x, dw_out, db_out,
                              p.db != nullptr, g.M, g.N, g.K, g.lddy,
                              g.ldx, m_lo, m_hi, (int)blockIdx.x * TB,
                              (int)blockIdx.y * TB, smem, dbs);
}

// ---------------------------------------------------------------------------
// Heterogeneous multi-problem wgrad: every layer's dW/db of a whole
// backward phase in ONE launch (per-problem shapes; linear block table).
// The workload is launch-latency-bound at batch 64 (OPTIMIZATION_LOG.md) —
// collapsing the per-layer wgrad launches buys back their launch floors.
// No split-M (phase batches are small); fully deterministic.
// ---------------------------------------------------------------------------

struct WHProb {
  const float* dy; const float* ymask; const float* x;
  float* dw; float* db;
  int M, N, K, lddy, ldx;
  int bx;      // tiles along N (at width TB*rn)
  int blk0;    // first linear block id of this problem
  // XCD-clustered enumeration (TAC_AMD_WGRAD_XCD): tiles are walked in
  // 2x2 clusters so the 8 contiguous chunks that land on the 8 XCDs
  // (wgid%8 placement, block count padded to a multiple of 8) share
  // their dy/x column slices in the XCD's own L2 — the 64x64 tile walk
  // otherwise re-reads every slice from a different XCD (57 MB/launch
  // fabric at Humanoid B=4096).  cn/ck = cluster dims, cx = clusters
  // along n; enumeration is padded to full clusters (invalid positions
  // early-return).
  int cn, ck, cx;
  int rn, rk;  // 64-wide sub-tiles per block along n / k (1 or 2):
               // large-M problems run 128x128 tiles so each staged
               // dy/x slice feeds 2x the MFMAs and the cross-tile
               // slice re-reads (the measured 58 MB/launch fabric
               // traffic at Humanoid B=4096) halve on each axis
  int64_t poff;  // element offset of this problem in a partial slab
};
struct WHArgs {
  WHProb p[MAXW];
  int np;
  int xcd_chunk;   // tiles per XCD chunk (0 = linear enumeration)
  int enum_total;  // real enumeration length (grid may be padded)
  // split-M (large batch): blockIdx.z = slab; slabs write raw partials
  // at part[slab*per_slab + p.poff + ...], one combine for EVERYTHING
  float* part;
  int m_chunk;
  int64_t per_slab;
};

// 128x128-capable wgrad body (bf16; rn/rk in {1,2} sub-tiles): each
// staged 64-wide dy/x slice feeds rn*rk MFMA tile pairs.
template <bool MASK>
DEVINL void wgrad_tile_body2(const WHProb& p, float* dw_out,
                             float* db_out, int m_lo, int m_hi,
                             int bn0, int bk0, char* smem, float* dbs) {
  constexpr int LBYTES = 64 * LDSB2 * 2;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wrow = (wid >> 1) * 32;
  const int wcol = (wid & 1) * 32;
  const int rn = p.rn, rk = p.rk;
  const int N = p.N, K = p.K;

  if (tid < 128) dbs[tid] = 0.f;
  f32x4 acc[2][2][2][2] = {};   // [ni][ki][mi][nj]

  __bf16* as0 = (__bf16*)smem;
  __bf16* as1 = (__bf16*)(smem + LBYTES);
  __bf16* bs0 = (__bf16*)(smem + 2 * LBYTES);
  __bf16* bs1 = (__bf16*)(smem + 3 * LBYTES);

  for (int i0 = m_lo; i0 < m_hi; i0 += BKB2) {
    wstage_bf16<MASK>(as0, p.dy, p.ymask, i0, bn0, m_hi, N, p.lddy);
    if (rn > 1)
      wstage_bf16<MASK>(as1, p.dy, p.ymask, i0, bn0 + TB, m_hi, N,
                        p.lddy);
    wstage_bf16<false>(bs0, p.x, nullptr, i0, bk0, m_hi, K, p.ldx);
    if (rk > 1)
      wstage_bf16<false>(bs1, p.x, nullptr, i0, bk0 + TB, m_hi, K, p.ldx);
    __syncthreads();
    mma_tiles<true>(as0, bs0, acc[0][0], lane, wrow, wcol);
    if (rk > 1) mma_tiles<true>(as0, bs1, acc[0][1], lane, wrow, wcol);
    if (rn > 1) {
      mma_tiles<true>(as1, bs0, acc[1][0], lane, wrow, wcol);
      if (rk > 1) mma_tiles<true>(as1, bs1, acc[1][1], lane, wrow, wcol);
    }
    if (db_out && bk0 == 0 && tid < 64 * rn) {
      const __bf16* as = tid < 64 ? as0 : as1;
      const int n = tid & 63;
      float s = 0.f;
      for (int i = 0; i < BKB2; ++i) s += (float)as[n * LDSB2 + i];
      dbs[tid] += s;
    }
    __syncthreads();
  }

  const int crow = (lane >> 4) * 4, ccol = lane & 15;
  for (int ni = 0; ni < rn; ++ni)
    for (int ki = 0; ki < rk; ++ki)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int gn = bn0 + ni * TB + wrow + mi * 16 + crow + r;
            int gk = bk0 + ki * TB + wcol + nj * 16 + ccol;
            if (gn < N && gk < K)
              dw_out[(int64_t)gn * K + gk] = acc[ni][ki][mi][nj][r];
          }
  if (db_out && bk0 == 0 && tid < 64 * rn && bn0 + tid < N)
    db_out[bn0 + tid] = dbs[tid];
}

template <bool BF16, bool ADAM = false>
DEVINL void mwgrad_het_body(const WHArgs& a, const WAdam& ad) {
  constexpr int LBYTES = BF16 ? (64 * LDSB2 * 2) : (64 * LDSF2 * 4);
  __shared__ __attribute__((aligned(16))) char smem[4 * LBYTES];
  __shared__ float dbs[128];
  int b = (int)blockIdx.x;
  int q = -1;
  if constexpr (ADAM) {
    // single-K-step un-split launch: four blocks per tile, one 16x16
    // quarter of each wave's sub-tiles each (see wgrad_tile_body)
    if (ad.quarter) { q = b & 3; b >>= 2; }
  }
  if (a.xcd_chunk) {
    // chunk-per-XCD remap: hardware places wgid on XCD wgid%8 (block
    // count is padded to a multiple of 8), so chunk i of the clustered
    // tile enumeration runs entirely on XCD i
    b = (b & 7) * a.xcd_chunk + (b >> 3);
    if (b >= a.enum_total) return;
  }
  int zi = 0;
#pragma unroll
  for (int i = 1; i < MAXW; ++i)
    if (i < a.np && b >= a.p[i].blk0) zi = i;
  const WHProb& p = a.p[zi];
  const int local = b - p.blk0;
  int bn0, bk0;
  if (a.xcd_chunk) {
    const int cs = p.cn * p.ck;
    const int c = local / cs, o = local - c * cs;
    const int n = (c % p.cx) * p.cn + o % p.cn;
    const int k = (c / p.cx) * p.ck + o / p.cn;
    if (n >= p.bx) return;                 // padded cluster slot
    bn0 = n * TB * p.rn;
    bk0 = k * TB * p.rk;
    const int bk_tiles = (p.K + TB * p.rk - 1) / (TB * p.rk);
    if (k >= bk_tiles) return;             // padded cluster slot
  } else {
    bn0 = (local % p.bx) * TB * p.rn;
    bk0 = (local / p.bx) * TB * p.rk;
  }
  float* dw_out = p.dw;
  float* db_out = p.db;
  int m_lo = 0, m_hi = p.M;
  if (a.part) {
    float* base = a.part + (int64_t)blockIdx.z * a.per_slab + p.poff;
    dw_out = base;
    db_out = p.db ? base + (int64_t)p.N * p.K : nullptr;
    m_lo = (int)blockIdx.z * a.m_chunk;
    m_hi = min(p.M, m_lo + a.m_chunk);
  }
  if (!ADAM && BF16 && (p.rn > 1 || p.rk > 1)) {
    if (p.ymask)
      wgrad_tile_body2<true>(p, dw_out, db_out, m_lo, m_hi, bn0, bk0,
                             smem, dbs);
    else
      wgrad_tile_body2<false>(p, dw_out, db_out, m_lo, m_hi, bn0, bk0,
                              smem, dbs);
    return;
  }
  if constexpr (ADAM) {
    // split-M slabs hold partial sums: Adam runs in the combine instead
    const bool do_adam = a.part == nullptr;
    float* wt = ad.wt[zi];
    if (p.ymask)
      wgrad_tile_body<BF16, true, true>(
          p.dy, p.ymask, p.x, dw_out, db_out, p.db != nullptr, p.M, p.N,
          p.K, p.lddy, p.ldx, m_lo, m_hi, bn0, bk0, smem, dbs, ad,
          do_adam, wt, q);
    else
      wgrad_tile_body<BF16, false, true>(
          p.dy, p.ymask, p.x, dw_out, db_out, p.db != nullptr, p.M, p.N,
          p.K, p.lddy, p.ldx, m_lo, m_hi, bn0, bk0, smem, dbs, ad,
          do_adam, wt, q);
    return;
  }
  if (p.ymask)
    wgrad_tile_body<BF16, true>(p.dy, p.ymask, p.x, dw_out, db_out,
                                p.db != nullptr, p.M, p.N, p.K, p.lddy,
                                p.ldx, m_lo, m_hi, bn0, bk0, smem, dbs);
  else
    wgrad_tile_body<BF16, false>(p.dy, p.ymask, p.x, dw_out, db_out,
                                 p.db != nullptr, p.M, p.N, p.K, p.lddy,
                                 p.ldx, m_lo, m_hi, bn0, bk0, smem, dbs);
}

template <bool BF16>
__global__ __launch_bounds__(256)
void mwgrad_het_kernel(WHArgs a) {
  mwgrad_het_body<BF16, false>(a, WAdam{});
}

// wgrad + Adam in one launch (mwgrad_het_adam): own instantiations, the
// plain kernels above keep their code
template <bool BF16>
__global__ __launch_bounds__(256)
void mwgrad_het_adam_kernel(WHArgs a, WAdam ad) {
  mwgrad_het_body<BF16, true>(a, ad);
}

// one deterministic combine for EVERY problem of the phase; ADAM also
// applies the update to each summed element (same hazard argument as the
// tile epilogue: one thread owns each flat element)
template <bool ADAM>
DEVINL void mwgrad_het_combine_body(const WHArgs& a, int split,
                                    const WAdam& ad) {
  float bc1 = 1.f, bc2 = 1.f;
  if constexpr (ADAM) {
    const float t = (float)ad.step[0];
    bc1 = 1.f - powf(ad.b1, t);
    bc2 = 1.f - powf(ad.b2, t);
  }
  const int64_t total = a.per_slab;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    float s = 0.f;
    for (int sl = 0; sl < split; ++sl)
      s += a.part[(int64_t)sl * a.per_slab + i];
    int zi = 0;
#pragma unroll
    for (int z = 1; z < MAXW; ++z)
      if (z < a.np && i >= a.p[z].poff) zi = z;
    const WHProb& p = a.p[zi];
    const int64_t off = i - p.poff;
    const int64_t dwn = (int64_t)p.N * p.K;
    if (off < dwn) p.dw[off] = s;
    else if (p.db) p.db[off - dwn] = s;
    if constexpr (ADAM) {
      if (off < dwn) {
        const float pn = wadam_apply(ad, (p.dw - ad.grad) + off, s, bc1,
                                     bc2);
        if (float* wt = ad.wt[zi]) {
          const int nn = (int)(off / p.K);
          const int kk = (int)(off - (int64_t)nn * p.K);
          wt[(int64_t)kk * p.N + nn] = pn;
        }
      } else if (p.db) {
        wadam_apply(ad, (p.db - ad.grad) + (off - dwn), s, bc1, bc2);
      }
    }
  }
}

__global__ __launch_bounds__(256)
void mwgrad_het_combine_kernel(WHArgs a, int split) {
  mwgrad_het_combine_body<false>(a, split, WAdam{});
}

__global__ __launch_bounds__(256)
void mwgrad_het_combine_adam_kernel(WHArgs a, int split, WAdam ad) {
  mwgrad_het_combine_body<true>(a, split, ad);
}

// deterministic combine of split-M wgrad slabs: for each problem z,
// dw[i] = sum_slab part[slab][z][i] (db appended after dw)
__global__ __launch_bounds__(256)
void mwgrad_combine_kernel(const float* __restrict__ part, WGemm g,
                           int split) {
  const int64_t per = (int64_t)g.N * g.K + g.N;
  const int64_t total = per * g.nz;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    const int z = (int)(i / per);
    const int64_t off = i % per;
    float sm = 0.f;
    for (int sl = 0; sl < split; ++sl)
      sm += part[((int64_t)sl * g.nz + z) * per + off];
    if (off < (int64_t)g.N * g.K) g.p[z].dw[off] = sm;
    else if (g.p[z].db) g.p[z].db[off - (int64_t)g.N * g.K] = sm;
  }
}

// ---------------------------------------------------------------------------
// Weight-transpose refresh: wt[k*N + n] = w[n*K + k], many layers per launch
// ---------------------------------------------------------------------------

constexpr int MAX_T = 12;
struct TArgs {
  const float* w[MAX_T];
  float* wt[MAX_T];
  int N[MAX_T], K[MAX_T], BS[MAX_T];
  int n_layers, blocks_per_layer;
};

// BS=1: plain [N,K] -> [K,N] (dense dgrad weights).  BS=kh*kw: conv
// [OC,IC,kh,kw] -> [IC, OC*kh*kw] block transpose (the dgrad layout of
// conv2d_dgrad; replaces an aten permute+contiguous per backward).
__global__ __launch_bounds__(256)
void transpose_multi_kernel(TArgs t) {
  const int layer = blockIdx.x / t.blocks_per_layer;
  const int slice = blockIdx.x % t.blocks_per_layer;
  if (layer >= t.n_layers) return;
  const int N = t.N[layer], K = t.K[layer], BS = t.BS[layer];
  const float* w = t.w[layer];
  float* wt = t.wt[layer];
  const int tid = threadIdx.x;
  if (BS == 1) {
    // LDS-tiled: both the global read (along k) and the global write
    // (along n) are coalesced — the naive element loop writes with
    // stride N (the 512x3136 dense layer was its worst case)
    __shared__ float tile[64][65];
    const int tiles_n = (N + 63) >> 6, tiles_k = (K + 63) >> 6;
    for (int tt = slice; tt < tiles_n * tiles_k;
         tt += t.blocks_per_layer) {
      const int n0 = (tt / tiles_k) << 6, k0 = (tt % tiles_k) << 6;
      for (int e = tid; e < 4096; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int n = n0 + r, k = k0 + c;
        tile[r][c] = (n < N && k < K) ? w[(int64_t)n * K + k] : 0.f;
      }
      __syncthreads();
      for (int e = tid; e < 4096; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int k = k0 + r, n = n0 + c;
        if (k < K && n < N) wt[(int64_t)k * N + n] = tile[c][r];
      }
      __syncthreads();
    }
    return;
  }
  const int64_t total = (int64_t)N * K * BS;
  const int64_t stride = (int64_t)t.blocks_per_layer * blockDim.x;
  for (int64_t idx = (int64_t)slice * blockDim.x + tid; idx < total;
       idx += stride) {
    int64_t n = idx / ((int64_t)K * BS);
    int64_t r = idx % ((int64_t)K * BS);
    int64_t k = r / BS, e = r % BS;
    wt[(k * N + n) * BS + e] = w[idx];
  }
}

// ---------------------------------------------------------------------------
// Prioritized replay: maintenance of the fan-out-64 sum tree the gather
// draws from (replay_draw.h has the layout and the draw;
// buffer/replay.py::_update_priorities_ref is the executable definition)
// ---------------------------------------------------------------------------

constexpr int PER_THREADS = 1024;   // 16 waves: 16 nodes per load round trip

// Recompute `count` nodes of level k from their children, one wave per
// node: node_of(t) names the t-th node.  The sum is the fixed halving
// order a __shfl_down reduction leaves in lane 0 (never a delta), so the
// tree is a deterministic function of its leaves; naming a node twice
// only stores the same value twice.  Two nodes per wave and round, so
// their loads are in flight together.
template <typename F>
DEVINL void per_resum_(float* __restrict__ tree, const PerLay& lay, int k,
                       int64_t count, F node_of) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float* kids = tree + lay.off[k + 1];
  float* out = tree + lay.off[k];
  for (int64_t t0 = (int64_t)wave * 2; t0 < count; t0 += 2 * nw) {
    const bool two = t0 + 1 < count;
    const int64_t a = node_of(t0), b = two ? node_of(t0 + 1) : a;
    float va = kids[a * 64 + lane], vb = kids[b * 64 + lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      va += __shfl_down(va, off);
      vb += __shfl_down(vb, off);
    }
    if (lane == 0) {
      out[a] = va;
      if (two) out[b] = vb;
    }
  }
}

// update_priorities in one launch: p = (td + eps)^alpha into the leaves
// (where a slot occurs more than once the highest batch position wins),
// max_priority = max(max_priority, max p), then every ancestor level by
// level.  Single block: all leaf writes must be complete before a parent
// is summed and there is no grid-wide barrier.  Plain vector stores only.
__global__ __launch_bounds__(PER_THREADS)
void per_update_kernel(float* __restrict__ tree, PerLay lay,
                       const int64_t* __restrict__ idx,
                       const float* __restrict__ td, int B, float alpha,
                       float eps, float* __restrict__ max_priority) {
  __shared__ float red[PER_THREADS / 64];
  // the first PER_THREADS slots, so the parent levels below need no second
  // dependent load for them
  __shared__ int64_t s_slot[PER_THREADS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int64_t cap = lay.n[lay.L];
  float* leaves = tree + lay.off[lay.L];
  // read up front so its latency hides under the leaf writes
  float mp0 = 0.f;
  if (threadIdx.x == 0) mp0 = max_priority[0];
  float pmax = 0.f;
  // Chunks of blockDim positions in ascending order.  Inside a wave a lane
  // yields to any later lane with the same slot; the waves of a chunk that
  // hold positions then store in wave order with a barrier in between, and
  // the chunks follow each other, so the last store to a slot is its
  // highest position's.
  for (int j0 = 0; j0 < B; j0 += blockDim.x) {
    const int j = j0 + threadIdx.x;
    const bool live = j < B;
    int64_t slot = live ? idx[j] : -1;
    if (slot >= cap) slot = -1;      // never write outside the ring
    if (j0 == 0) s_slot[threadIdx.x] = slot;
    float p = 0.f;
    bool win = slot >= 0;
    if (j0 + wave * 64 < B) {        // wave-uniform: the wave has positions
      if (live) {
        p = powf(td[j] + eps, alpha);
        pmax = fmaxf(pmax, p);
      }
      for (int m = 1; m < 64; ++m) {
        const int64_t other = __shfl(slot, m);
        if (m > lane && other == slot) win = false;
      }
    }
    const int left = B - j0;
    const int busy = left >= (int)blockDim.x ? nw : (left + 63) >> 6;
    for (int w = 0; w < busy; ++w) {
      if (w == wave && win) leaves[slot] = p;
      __syncthreads();
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    pmax = fmaxf(pmax, __shfl_down(pmax, off));
  if (lane == 0) red[wave] = pmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = mp0;
    for (int w = 0; w < nw; ++w) m = fmaxf(m, red[w]);
    max_priority[0] = m;
  }
  for (int k = lay.L - 1; k >= 0; --k) {
    const int shift = 6 * (lay.L - k);
    if (lay.n[k] <= B) {
      // a small level: every node, no index reads
      per_resum_(tree, lay, k, lay.n[k], [](int64_t t) { return t; });
    } else {
      per_resum_(tree, lay, k, B, [&](int64_t t) {
        const int64_t s = t < PER_THREADS ? s_slot[t] : idx[t];
        return (s >= 0 && s < cap ? s : 0) >> shift;
      });
    }
    __syncthreads();
  }
}

// store / store_batch: the `count` slots from `start` (mod cap) get the
// device scalar max_priority — no host read — and their ancestors are
// recomputed.  A wrapping range is two runs of nodes on every level.
__global__ __launch_bounds__(PER_THREADS)
void per_set_range_kernel(float* __restrict__ tree, PerLay lay,
                          int64_t start, int64_t count,
                          const float* __restrict__ max_priority) {
  const int64_t cap = lay.n[lay.L];
  float* leaves = tree + lay.off[lay.L];
  const float p = max_priority[0];
  const int64_t first = count < cap - start ? count : cap - start;
  for (int64_t i = threadIdx.x; i < count; i += blockDim.x)
    leaves[i < first ? start + i : i - first] = p;
  __syncthreads();
  // inclusive leaf runs [a0, b0] and, when the range wraps, [0, b1]
  const int64_t a0 = start, b0 = start + first - 1, b1 = count - first - 1;
  for (int k = lay.L - 1; k >= 0; --k) {
    const int shift = 6 * (lay.L - k);
    const int64_t lo = a0 >> shift;
    const int64_t len0 = (b0 >> shift) - lo + 1;
    const int64_t len1 = b1 >= 0 ? (b1 >> shift) + 1 : 0;
    per_resum_(tree, lay, k, len0 + len1, [&](int64_t t) {
      return t < len0 ? lo + t : t - len0;
    });
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Fused tanh-Gaussian head, stacked rows with split outputs + internal
// Philox noise (row < B0 -> out0 slice; else out1 slice)
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(64)
void tg_fwd2_kernel(const float* __restrict__ hl,  // [R, 2A]: mu | log_std
                    float* __restrict__ out0, int ld0,
                    float* __restrict__ out1, int ld1, int B0,
                    float* __restrict__ logp, float* __restrict__ prob_out,
                    const int64_t* __restrict__ ctr, int64_t ctr_add,
                    uint64_t seed,
                    int R, int A, float act_limit, float lo, float hi) {
  const int b = blockIdx.x;
  const int a = threadIdx.x;
  float acc = 0.f;
  if (a < A) {
    const int64_t i = (int64_t)b * A + a;
    // philox noise: one draw per element (use lane of the quad)
    Philox4 r = philox4(seed ^ 0x517cc1b727220a95ull,
                        (uint64_t)(ctr[0] + ctr_add), (uint64_t)i);
    float eps = philox_normal(r.x, r.y);

    float m = hl[(int64_t)b * 2 * A + a];
    float ls = fminf(fmaxf(hl[(int64_t)b * 2 * A + A + a], lo), hi);
    float std = expf(ls);
    float prob = m + std * eps;
    float pi = tanhf(prob) * act_limit;
    prob_out[i] = prob;
    if (b < B0) out0[(int64_t)b * ld0 + a] = pi;
    else        out1[(int64_t)(b - B0) * ld1 + a] = pi;
    float x = -2.f * prob;
    float sp = x > 20.f ? x : log1pf(expf(fminf(x, 20.f)));
    float gauss = -0.5f * eps * eps - ls - 0.5f * 1.8378770664093453f;
    float corr = 1.3862943611198906f - prob - sp;
    acc = gauss - corr;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if (a == 0) logp[b] = acc;
}

// one launch bumping several device counters (replay ctr + both Adam
// step counters at update start — saves two 1-thread launches)
__global__ void bump3_kernel(int64_t* a, int64_t* b, int64_t* c) {
  if (a) ++a[0];
  if (b) ++b[0];
  if (c) ++c[0];
}

// Debug/test helper: reproduce tg_fwd2's internal noise exactly so the
// eager fp32 reference can be driven with identical eps.
__global__ __launch_bounds__(64)
void tg_eps_kernel(float* __restrict__ eps_out, uint64_t ctr_val,
                   uint64_t seed, int R, int A) {
  const int b = blockIdx.x;
  const int a = threadIdx.x;
  if (a >= A) return;
  const int64_t i = (int64_t)b * A + a;
  Philox4 r = philox4(seed ^ 0x517cc1b727220a95ull, ctr_val, (uint64_t)i);
  eps_out[i] = philox_normal(r.x, r.y);
}

// backward over rows :B of the stacked forward; dpi read from the dxc
// slab at column offset; dlogp = alpha/B (policy loss seed) computed
// in-kernel from the device alpha.
__global__ __launch_bounds__(64)
void tg_bwd2_kernel(const float* __restrict__ dxc, int ld_dxc, int col0,
                    const float* __restrict__ dxc2,  // optional 2nd slab
                    const float* __restrict__ alpha_dev, float alpha_host,
                    const float* __restrict__ hl,   // [R, 2A]: mu | log_std
                    const float* __restrict__ prob,
                    float* __restrict__ dmu, float* __restrict__ dls,
                    int B, int A, float act_limit, float lo, float hi) {
  const int b = blockIdx.x;
  const int a = threadIdx.x;
  if (a >= A) return;
  const int64_t i = (int64_t)b * A + a;
  const float alpha = alpha_dev ? alpha_dev[0] : alpha_host;
  float raw = hl[(int64_t)b * 2 * A + A + a];
  float ls = fminf(fmaxf(raw, lo), hi);
  float std = expf(ls);
  float p = prob[i];
  float t = tanhf(p);
  float se = p - hl[(int64_t)b * 2 * A + a];   // std * eps
  float dpi = dxc[(int64_t)b * ld_dxc + col0 + a];
  if (dxc2) dpi += dxc2[(int64_t)b * ld_dxc + col0 + a];
  float dl = alpha / B;
  float dp = dpi * act_limit * (1.f - t * t);
  float g_mu = dp + dl * t;
  float g_ls = dp * se + dl * (se * t - 1.f);
  float mask = (raw >= lo && raw <= hi) ? 1.f : 0.f;
  dmu[i] = g_mu;
  dls[i] = g_ls * mask;
}

// ---------------------------------------------------------------------------
// Single-block losses (deterministic reductions, device-alpha aware)
// ---------------------------------------------------------------------------

// qloss: Bellman backup + twin-min MSE + gradient seeds + (optionally)
// the K=1 dgrad of the final critic layer fused in: dy2_z = dq_z x wt3_z
// (outer product; dq staged in LDS so no extra launch is needed).
constexpr int LOSS_MAXB = 1024;

// WEIGHTED (prioritized replay): importance weights w_j = (size * prob_j)^
// -beta over their batch maximum scale each row's squared errors and its
// gradient seeds, and td_j = (|e1| + |e2|) / 2 is exported for the priority
// update.  The default instantiation compiles to the unweighted kernel.
template <bool WEIGHTED>
__global__ __launch_bounds__(256)
void qloss2_kernel(const float* __restrict__ q1, const float* __restrict__ q2,
                   const float* __restrict__ q1t, const float* __restrict__ q2t,
                   const float* __restrict__ logp_next,
                   const float* __restrict__ rew, const float* __restrict__ done,
                   const float* __restrict__ alpha_dev, float alpha_host,
                   float* __restrict__ loss_acc,
                   float* __restrict__ dq1, float* __restrict__ dq2,
                   int B, float gamma, float scale,
                   const float* __restrict__ wt3_0,
                   const float* __restrict__ wt3_1,
                   float* __restrict__ dy2_0, float* __restrict__ dy2_1,
                   int h2,
                   int64_t* __restrict__ bump0, int64_t* __restrict__ bump1,
                   int64_t* __restrict__ bump2,
                   const float* __restrict__ prob,
                   const int64_t* __restrict__ size_dev,
                   const float* __restrict__ beta_dev,
                   float* __restrict__ td) {
  __shared__ float red[1][4];
  __shared__ float dqs[2][LOSS_MAXB];
  const float alpha = alpha_dev ? alpha_dev[0] : alpha_host;
  const bool fuse = dy2_0 != nullptr;
  // counters are read up front so their latency hides under the loss
  int64_t c0 = 0, c1 = 0, c2 = 0;
  if (threadIdx.x == 0) {
    if (bump0) c0 = bump0[0];
    if (bump1) c1 = bump1[0];
    if (bump2) c2 = bump2[0];
  }
  float wsize = 0.f, nbeta = 0.f, wmax = 1.f;
  if constexpr (WEIGHTED) {
    // batch maximum of the raw weights first (max is order-independent)
    __shared__ float redw[4];
    wsize = (float)size_dev[0];
    nbeta = -beta_dev[0];
    float m = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x)
      m = fmaxf(m, powf(wsize * prob[i], nbeta));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
    if ((threadIdx.x & 63) == 0) redw[threadIdx.x >> 6] = m;
    __syncthreads();
    wmax = fmaxf(fmaxf(redw[0], redw[1]), fmaxf(redw[2], redw[3]));
  }
  float acc = 0.f;
  if constexpr (WEIGHTED) {
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
      float backup = scale * rew[i] + gamma * (1.f - done[i]) *
                         (fminf(q1t[i], q2t[i]) - alpha * logp_next[i]);
      float e1 = q1[i] - backup, e2 = q2[i] - backup;
      const float w = powf(wsize * prob[i], nbeta) / wmax;
      acc += w * (e1 * e1 + e2 * e2);
      const float g1 = 2.f * (w * e1) / B;
      const float g2 = 2.f * (w * e2) / B;
      td[i] = 0.5f * (fabsf(e1) + fabsf(e2));
      dq1[i] = g1;
      dq2[i] = g2;
      if (fuse) { dqs[0][i] = g1; dqs[1][i] = g2; }
    }
  } else {
    const QIn in{q1, q2, q1t, q2t, logp_next, rew, done};
    auto load = [&](int i) { return qvals_load(in, i); };
    acc = qloss_rows(load, alpha, gamma, scale, B, [&](int i, const QRow& r) {
      dq1[i] = r.g1;
      dq2[i] = r.g2;
      if (fuse) { dqs[0][i] = r.g1; dqs[1][i] = r.g2; }
    });
  }
  float mean[1] = {acc};
  loss_block_mean<1>(mean, red, B);
  if (threadIdx.x == 0) {
    loss_acc[0] += mean[0];
    // commit the update's counter bump (replay/noise counter + both Adam
    // step counters): this single block runs after both counter readers
    // (gather2 / tg_fwd2 key on ctr+1) and before both Adam applications
    if (bump0) bump0[0] = c0 + 1;
    if (bump1) bump1[0] = c1 + 1;
    if (bump2) bump2[0] = c2 + 1;
  }
  if (fuse) {
    const int64_t total = (int64_t)B * h2;
    for (int64_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
      int i = (int)(idx / h2), j = (int)(idx % h2);
      dy2_0[idx] = dqs[0][i] * wt3_0[j];
      dy2_1[idx] = dqs[1][i] * wt3_1[j];
    }
  }
}

__global__ __launch_bounds__(256)
void piloss2_kernel(const float* __restrict__ q1, const float* __restrict__ q2,
                    const float* __restrict__ logp,
                    const float* __restrict__ alpha_dev, float alpha_host,
                    float* __restrict__ loss_acc,
                    float* __restrict__ mean_logp,
                    float* __restrict__ dq1, float* __restrict__ dq2,
                    int B,
                    const float* __restrict__ wt3_0,
                    const float* __restrict__ wt3_1,
                    float* __restrict__ dy2_0, float* __restrict__ dy2_1,
                    int h2) {
  __shared__ float red[2][4];   // loss | logp
  __shared__ float dqs[2][LOSS_MAXB];
  const float alpha = alpha_dev ? alpha_dev[0] : alpha_host;
  const bool fuse = dy2_0 != nullptr;
  float acc[2];
  auto load = [&](int i) {
    QVals v = {};
    v.q1 = q1[i]; v.q2 = q2[i]; v.lpn = logp[i];
    return v;
  };
  piloss_rows(acc, load, alpha, B, [&](int i, const PiRow& r) {
    dq1[i] = r.g1;
    dq2[i] = r.g2;
    if (fuse) { dqs[0][i] = r.g1; dqs[1][i] = r.g2; }
  });
  loss_block_mean<2>(acc, red, B);
  if (threadIdx.x == 0) {
    loss_acc[0] += acc[0];
    if (mean_logp) mean_logp[0] = acc[1];
  }
  if (fuse) {
    const int64_t total = (int64_t)B * h2;
    for (int64_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
      int i = (int)(idx / h2), j = (int)(idx % h2);
      dy2_0[idx] = dqs[0][i] * wt3_0[j];
      dy2_1[idx] = dqs[1][i] * wt3_1[j];
    }
  }
}

// ---------------------------------------------------------------------------
// Whole-policy single-state action kernel: the entire actor forward for
// ONE state (the serial env-interaction path) in ONE launch — trunk
// GEMVs through LDS, dual heads, clamp/exp, Philox noise (single block,
// so the counter self-bumps: no predecessor kernel), tanh squash.
// ---------------------------------------------------------------------------

constexpr int ACT_MAXL = 4;
constexpr int ACT_MAXW = 512;

struct ActArgs {
  const float* x;              // [O] device input state
  const float* w[ACT_MAXL];    // trunk weights [H, K]
  const float* b[ACT_MAXL];
  int width[ACT_MAXL];
  int n_layers, O, A;
  const float* wmu; const float* bmu;
  const float* wls; const float* bls;
  float* action;               // [A]
  int64_t* ctr;
  uint64_t seed;
  float act_limit, lo, hi;
};

// completion flag written to host-visible pinned memory after the
// action stores (system-scope release), so the host can spin instead of
// paying a D2H copy + event synchronization per env step.
struct ActPinned {
  float* out_host;        // pinned [A]
  int* flag_host;         // pinned [1]
};

__global__ __launch_bounds__(256)
void act_kernel(ActArgs a, ActPinned hp) {
  __shared__ __attribute__((aligned(16))) float buf[2][ACT_MAXW];
  __shared__ unsigned long long ctr_s;
  const int tid = threadIdx.x;
  if (tid == 0) ctr_s = (unsigned long long)(++a.ctr[0]);
  for (int k = tid; k < a.O; k += blockDim.x) buf[0][k] = a.x[k];
  __syncthreads();

  int cur = 0, K = a.O;
  for (int L = 0; L < a.n_layers; ++L) {
    const int H = a.width[L];
    float acc = 0.f;
    if (tid < H) {
      acc = a.b[L][tid];
      const float* wr = a.w[L] + (int64_t)tid * K;
      int k = 0;
      for (; k + 4 <= K; k += 4) {
        acc += wr[k] * buf[cur][k] + wr[k+1] * buf[cur][k+1]
             + wr[k+2] * buf[cur][k+2] + wr[k+3] * buf[cur][k+3];
      }
      for (; k < K; ++k) acc += wr[k] * buf[cur][k];
    }
    __syncthreads();
    if (tid < H) buf[1 - cur][tid] = fmaxf(acc, 0.f);
    __syncthreads();
    cur ^= 1;
    K = H;
  }

  // heads + tanh-Gaussian sample (stochastic acting path)
  if (tid < a.A) {
    float mu = a.bmu[tid], ls = a.bls[tid];
    const float* wm = a.wmu + (int64_t)tid * K;
    const float* wl = a.wls + (int64_t)tid * K;
    for (int k = 0; k < K; ++k) {
      float h = buf[cur][k];
      mu += wm[k] * h;
      ls += wl[k] * h;
    }
    ls = fminf(fmaxf(ls, a.lo), a.hi);
    Philox4 r = philox4(a.seed ^ 0x517cc1b727220a95ull, ctr_s, (uint64_t)tid);
    float eps = philox_normal(r.x, r.y);
    float act = tanhf(mu + expf(ls) * eps) * a.act_limit;
    a.action[tid] = act;
    if (hp.out_host) hp.out_host[tid] = act;
  }
  if (hp.flag_host) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
      __threadfence_system();
      *(volatile int*)hp.flag_host = 1;
    }
  }
}

// ---------------------------------------------------------------------------
// Latency-shaped form of act_kernel: the same arithmetic per output neuron,
// in the same order, but the weights reach it differently.  act_kernel has
// each thread walk its own fp32 row straight from global memory, so a wave
// load touches 64 lines for 16 bytes each and every loop iteration ends on
// a full wait (measured: 7.5 us in layer 1 and 4.5 us in the heads of an
// 18.6 us launch).  Here every load the kernel will ever need is addressed
// without the observation, so it is issued at kernel start, coalesced
// (consecutive lanes read consecutive addresses), and parked in registers:
//   * the observation and the counter (first, so their waits stay short);
//   * all biases;
//   * layer 0's [H, O] matrix as flat dwords (O is odd in practice);
//   * the hidden layers as a stream of K slabs, [H rows] x [64 columns],
//     two slabs in flight in two register sets, refilled as they drain;
//   * both heads' rows as flat dwords.
// Each piece goes through LDS once (slab rows padded to 68 floats, so the
// 16-byte row reads of 16 lanes fall on 64 different banks) and thread t
// then reads row t from LDS exactly as act_kernel reads it from memory.
// The mu rows run on wave 0 and the log-std rows on wave 1.
//
// The block is one wave per SIMD, so every instruction is paid in full:
// addresses are a per-thread offset plus uniform or immediate parts, and
// tails are handled by clamping an index (a repeated load or store of the
// same value), not by branching per element.
//
// Roundings follow what the shipped act_kernel compiles to: in the groups
// of four every product is rounded, ((p0 + p1) + p2) + p3, then acc +=
// group; the scalar K tail, both head rows and mu + exp(ls) * eps are
// fused multiply-adds.
//
// Gate (act_fast_fits): 1..4 layers; widths 4..256, multiples of 4; hidden
// layers (L >= 1) with K a multiple of 64 and H a multiple of 16; the last
// width a power of two; H0 * O <= 9216; A <= 64 and A * K_last <= 2048;
// hidden weights 16-byte aligned.
// ---------------------------------------------------------------------------

constexpr int ACTF_L0 = 36;               // layer-0 dwords per thread
constexpr int ACTF_KS = 64;               // hidden-layer slab columns
constexpr int ACTF_SV = ACTF_KS / 4;      // float4 per thread per slab
constexpr int ACTF_SS = ACTF_KS + 4;      // slab row stride in LDS
constexpr int ACTF_HV = 8;                // dwords per thread per head
constexpr int ACTF_HL = 2 * ACTF_HV * 256 + 128 * 4;

struct ActfLds {
  float act[2][256];
  float bias[ACT_MAXL][256];
  float w0[ACTF_L0 * 256];
  float slab[256 * ACTF_SS];
  float hd[ACTF_HL];
  float ls[64];
  unsigned long long ctr;
};

// position in the hidden-layer slab stream, with that layer's shape
struct ActfCur {
  int L, k0, K, H;
  const float* w;
};

DEVINL void actf_shape(const ActArgs& a, ActfCur& c) {
  // selects over statically indexed kernel arguments: no memory round trip
  c.K = c.L == 1 ? a.width[0] : c.L == 2 ? a.width[1] : a.width[2];
  c.H = c.L == 1 ? a.width[1] : c.L == 2 ? a.width[2] : a.width[3];
  c.w = c.L == 1 ? a.w[1] : c.L == 2 ? a.w[2] : a.w[3];
}

DEVINL ActfCur actf_next(const ActArgs& a, ActfCur c) {
  if (c.L < a.n_layers) {
    c.k0 += ACTF_KS;
    if (c.k0 >= c.K) { ++c.L; c.k0 = 0; actf_shape(a, c); }
  }
  return c;
}

// Slab element j of thread tid is row (tid >> 4) + 16 j, float4 column
// tid & 15.  FULL: H == 256, nothing to guard; otherwise rows in whole
// sixteens (H % 16 == 0), a uniform guard per j.
template <bool FULL>
DEVINL void actf_issue(f32x4 (&R)[ACTF_SV], const ActfCur& cu, int tid) {
  const unsigned vo = (unsigned)(tid >> 4) * cu.K + (tid & 15) * 4;
#pragma unroll
  for (int j = 0; j < ACTF_SV; ++j) {
    if (FULL || 16 * j < cu.H) {
      const float* p = cu.w + cu.k0 + (int64_t)(16 * j) * cu.K;   // uniform
      R[j] = *reinterpret_cast<const f32x4*>(p + vo);
    }
  }
}

template <bool FULL>
DEVINL void actf_commit(const f32x4 (&R)[ACTF_SV], float* slab,
                        const ActfCur& cu, int tid) {
  float* d = slab + (tid >> 4) * ACTF_SS + (tid & 15) * 4;
#pragma unroll
  for (int j = 0; j < ACTF_SV; ++j)
    if (FULL || 16 * j < cu.H)
      *reinterpret_cast<f32x4*>(d + 16 * j * ACTF_SS) = R[j];
}

__global__ __launch_bounds__(256)
void act_fast_kernel(ActArgs a, ActPinned hp) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) ActfLds s;
  const int tid = threadIdx.x;
  const int O = a.O, A = a.A, nl = a.n_layers;
  const int H0 = a.width[0];
  const int KL = nl == 1 ? a.width[0] : nl == 2 ? a.width[1]
               : nl == 3 ? a.width[2] : a.width[3];

  // ---- every load, before anything waits --------------------------------
  const float xo = a.x[tid < O ? tid : 0];
  const long long c_old = a.ctr[0];
  float br[ACT_MAXL];
#pragma unroll
  for (int L = 0; L < ACT_MAXL; ++L)
    br[L] = L < nl ? a.b[L][tid < a.width[L] ? tid : 0] : 0.f;
  // head bias: mu rows on wave 0, log-std rows on wave 1
  const int hl = tid & 63;
  const bool h_on = tid < 128 && hl < A;
  float hv = (tid < 64 ? a.bmu : a.bls)[hl < A ? hl : 0];

  // layer 0, flat; rounds in groups of six, indices clamped to the last
  float v0[ACTF_L0];
  const int n0 = H0 * O;
  const int r0 = (n0 + 255) >> 8;
#pragma unroll
  for (int g = 0; g < ACTF_L0 / 6; ++g) {
    if (6 * g < r0) {
#pragma unroll
      for (int j = 6 * g; j < 6 * g + 6; ++j)
        v0[j] = a.w[0][min(tid + 256 * j, n0 - 1)];
    }
  }

  f32x4 RA[ACTF_SV], RB[ACTF_SV];
  ActfCur cu{1, 0, 0, 0, nullptr};
  actf_shape(a, cu);
  auto issue = [&](f32x4 (&R)[ACTF_SV], const ActfCur& c) {
    if (c.L < nl) {
      if (c.H == 256) actf_issue<true>(R, c, tid);
      else actf_issue<false>(R, c, tid);
    }
  };
  issue(RA, cu);
  issue(RB, actf_next(a, cu));

  // heads, flat per head; rounds in groups of four, indices clamped
  float hm[ACTF_HV], hs[ACTF_HV];
  const int nh = A * KL;
  const int rh = (nh + 255) >> 8;
#pragma unroll
  for (int g = 0; g < ACTF_HV / 4; ++g) {
    if (4 * g < rh) {
#pragma unroll
      for (int j = 4 * g; j < 4 * g + 4; ++j) {
        const int idx = min(tid + 256 * j, nh - 1);
        hm[j] = a.wmu[idx];
        hs[j] = a.wls[idx];
      }
    }
  }

  // ---- observation, biases, layer 0 -> LDS ------------------------------
  if (tid < O) s.act[0][tid] = xo;
#pragma unroll
  for (int L = 0; L < ACT_MAXL; ++L) s.bias[L][tid] = br[L];
  if (tid == 0) {
    const long long c_new = c_old + 1;
    a.ctr[0] = c_new;
    s.ctr = (unsigned long long)c_new;
  }
#pragma unroll
  for (int g = 0; g < ACTF_L0 / 6; ++g) {
    if (6 * g < r0) {
#pragma unroll
      for (int j = 6 * g; j < 6 * g + 6; ++j)
        s.w0[min(tid + 256 * j, n0 - 1)] = v0[j];
    }
  }
  __syncthreads();

  int cur = 1;
  {
    float acc = br[0];
    if (tid < H0) {
      const float* wr = s.w0 + tid * O;
      const float* x = s.act[0];
      int k = 0;
      for (; k + 4 <= O; k += 4)
        acc += wr[k] * x[k] + wr[k+1] * x[k+1]
             + wr[k+2] * x[k+2] + wr[k+3] * x[k+3];
      for (; k < O; ++k) acc = __builtin_fmaf(wr[k], x[k], acc);
      s.act[1][tid] = fmaxf(acc, 0.f);
    }
  }

  // ---- hidden layers: the slab stream ------------------------------------
  float acc = br[1];
  auto slab_step = [&](f32x4 (&R)[ACTF_SV]) {
    if (cu.H == 256) actf_commit<true>(R, s.slab, cu, tid);
    else actf_commit<false>(R, s.slab, cu, tid);
    __syncthreads();   // slab (and the previous layer's output) visible
    issue(R, actf_next(a, actf_next(a, cu)));
    if (tid < cu.H) {
      const f32x4* wr = reinterpret_cast<const f32x4*>(s.slab + tid * ACTF_SS);
      const f32x4* x = reinterpret_cast<const f32x4*>(s.act[cur] + cu.k0);
#pragma unroll
      for (int g = 0; g < ACTF_SV; ++g) {
        const f32x4 w = wr[g], h = x[g];
        acc += w.x * h.x + w.y * h.y + w.z * h.z + w.w * h.w;
      }
    }
    if (cu.k0 + ACTF_KS >= cu.K) {   // layer done
      if (tid < cu.H) s.act[1 - cur][tid] = fmaxf(acc, 0.f);
      cur ^= 1;
      acc = s.bias[cu.L + 1 < ACT_MAXL ? cu.L + 1 : 0][tid];
    }
    __syncthreads();   // slab free for the next commit
    cu = actf_next(a, cu);
  };
  while (cu.L < nl) {
    slab_step(RA);
    if (cu.L >= nl) break;
    slab_step(RB);
  }

  // ---- heads -------------------------------------------------------------
  const int HS = KL + 4;
  {
    const int sh = 31 - __builtin_clz(KL);   // KL is a power of two
    float* hd_ls = s.hd + A * HS;
#pragma unroll
    for (int g = 0; g < ACTF_HV / 4; ++g) {
      if (4 * g < rh) {
#pragma unroll
        for (int j = 4 * g; j < 4 * g + 4; ++j) {
          const int idx = min(tid + 256 * j, nh - 1);
          const int d = (idx >> sh) * HS + (idx & (KL - 1));
          s.hd[d] = hm[j];
          hd_ls[d] = hs[j];
        }
      }
    }
  }
  __syncthreads();
  if (h_on) {
    const int row = tid < 64 ? hl : A + hl;
    const f32x4* wr = reinterpret_cast<const f32x4*>(s.hd + row * HS);
    const f32x4* x = reinterpret_cast<const f32x4*>(s.act[cur]);
    for (int g = 0; g < (KL >> 2); ++g) {
      const f32x4 w = wr[g], h = x[g];
      hv = __builtin_fmaf(w.x, h.x, hv);
      hv = __builtin_fmaf(w.y, h.y, hv);
      hv = __builtin_fmaf(w.z, h.z, hv);
      hv = __builtin_fmaf(w.w, h.w, hv);
    }
    if (tid >= 64) s.ls[hl] = hv;
  }
  __syncthreads();
  if (tid < A) {
    const float mu = hv;
    float ls = s.ls[tid];
    ls = fminf(fmaxf(ls, a.lo), a.hi);
    Philox4 r = philox4(a.seed ^ 0x517cc1b727220a95ull, s.ctr, (uint64_t)tid);
    float eps = philox_normal(r.x, r.y);
    // act_kernel's mu + exp(ls) * eps compiles to one fused multiply-add
    float act = tanhf(__builtin_fmaf(expf(ls), eps, mu)) * a.act_limit;
    a.action[tid] = act;
    if (hp.out_host) hp.out_host[tid] = act;
  }
  if (hp.flag_host) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
      __threadfence_system();
      *(volatile int*)hp.flag_host = 1;
    }
  }
}


// ---------------------------------------------------------------------------
// Batched whole-policy action kernel (evaluation path): the actor forward
// for N states in ONE launch.  Each block owns a tile of ACTB_R rows staged
// in LDS; each thread owns one output neuron, reads its weight row once and
// keeps ACTB_R accumulators, so weight traffic is paid once per tile
// instead of once per row.  Deterministic mode (tanh(mu) * act_limit)
// draws no noise; stochastic mode keys Philox on a counter passed BY VALUE
// (several blocks run, so act_kernel's single-block self-bump does not
// carry over) and a subsequence unique per (row, action index).
// ---------------------------------------------------------------------------

constexpr int ACTB_R = 8;

__global__ __launch_bounds__(256)
void act_batch_kernel(ActArgs a, int N, int ldx, int deterministic,
                      unsigned long long ctr_val) {
  __shared__ __attribute__((aligned(16))) float buf[2][ACTB_R][ACT_MAXW];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * ACTB_R;
  const int nrow = min(ACTB_R, N - row0);

  // rows past N are zero-filled, never read from x
  for (int i = tid; i < ACTB_R * a.O; i += blockDim.x) {
    const int r = i / a.O, k = i - r * a.O;
    buf[0][r][k] = r < nrow ? a.x[(int64_t)(row0 + r) * ldx + k] : 0.f;
  }
  __syncthreads();

  int cur = 0, K = a.O;
  for (int L = 0; L < a.n_layers; ++L) {
    const int H = a.width[L];
    float acc[ACTB_R];
    if (tid < H) {
      const float bias = a.b[L][tid];
#pragma unroll
      for (int r = 0; r < ACTB_R; ++r) acc[r] = bias;
      const float* wr = a.w[L] + (int64_t)tid * K;
      int k = 0;
      for (; k + 4 <= K; k += 4) {
        const float w0 = wr[k], w1 = wr[k+1], w2 = wr[k+2], w3 = wr[k+3];
#pragma unroll
        for (int r = 0; r < ACTB_R; ++r) {
          const float* h = &buf[cur][r][k];
          acc[r] += w0 * h[0] + w1 * h[1] + w2 * h[2] + w3 * h[3];
        }
      }
      for (; k < K; ++k) {
        const float w0 = wr[k];
#pragma unroll
        for (int r = 0; r < ACTB_R; ++r) acc[r] += w0 * buf[cur][r][k];
      }
#pragma unroll
      for (int r = 0; r < ACTB_R; ++r)
        buf[1 - cur][r][tid] = fmaxf(acc[r], 0.f);
    }
    __syncthreads();
    cur ^= 1;
    K = H;
  }

  // heads + tanh squash
  if (tid < a.A) {
    float mu[ACTB_R], ls[ACTB_R];
    const float bm = a.bmu[tid];
    const float* wm = a.wmu + (int64_t)tid * K;
#pragma unroll
    for (int r = 0; r < ACTB_R; ++r) mu[r] = bm;
    if (deterministic) {
      for (int k = 0; k < K; ++k) {
        const float w = wm[k];
#pragma unroll
        for (int r = 0; r < ACTB_R; ++r) mu[r] += w * buf[cur][r][k];
      }
#pragma unroll
      for (int r = 0; r < ACTB_R; ++r)
        if (r < nrow)
          a.action[(int64_t)(row0 + r) * a.A + tid] =
              tanhf(mu[r]) * a.act_limit;
    } else {
      const float bl = a.bls[tid];
      const float* wl = a.wls + (int64_t)tid * K;
#pragma unroll
      for (int r = 0; r < ACTB_R; ++r) ls[r] = bl;
      for (int k = 0; k < K; ++k) {
        const float w = wm[k], v = wl[k];
#pragma unroll
        for (int r = 0; r < ACTB_R; ++r) {
          const float h = buf[cur][r][k];
          mu[r] += w * h;
          ls[r] += v * h;
        }
      }
#pragma unroll
      for (int r = 0; r < ACTB_R; ++r) {
        if (r < nrow) {
          const float l = fminf(fmaxf(ls[r], a.lo), a.hi);
          Philox4 p = philox4(
              a.seed ^ 0x2545f4914f6cdd1dull, ctr_val,
              (uint64_t)(row0 + r) * (uint64_t)a.A + (uint64_t)tid);
          float eps = philox_normal(p.x, p.y);
          a.action[(int64_t)(row0 + r) * a.A + tid] =
              tanhf(mu[r] + expf(l) * eps) * a.act_limit;
        }
      }
    }
  }
}

// learned entropy temperature: one-thread Adam on log_alpha
// (loss = -log_alpha * (mean_logp + target_entropy))
__global__ void alpha_update_kernel(float* __restrict__ log_alpha,
                                    float* __restrict__ alpha_dev,
                                    float* __restrict__ m, float* __restrict__ v,
                                    int64_t* __restrict__ step,
                                    const float* __restrict__ mean_logp,
                                    float target_entropy, float lr) {
  float g = -(mean_logp[0] + target_entropy);
  int64_t t = ++step[0];
  float mi = 0.9f * m[0] + 0.1f * g;
  float vi = 0.999f * v[0] + 0.001f * g * g;
  m[0] = mi; v[0] = vi;
  float bc1 = 1.f - powf(0.9f, (float)t);
  float bc2 = 1.f - powf(0.999f, (float)t);
  log_alpha[0] -= lr / bc1 * mi / (sqrtf(vi / bc2) + 1e-8f);
  alpha_dev[0] = expf(log_alpha[0]);
}

// ---------------------------------------------------------------------------
// Adam with fused transposed-weight refresh: after updating flat[i],
// weight-slab elements also write their transposed copy (the dgrad
// operand cache) — removes the separate transpose kernels per update.
// ---------------------------------------------------------------------------

struct ATArgs {
  int64_t off[MAX_T];    // flat offset of each weight slab
  float* wt[MAX_T];
  int N[MAX_T], K[MAX_T];
  int BS[MAX_T];         // 1 = dense [N,K]->[K,N]; kh*kw = conv
                         // [OC,IC,kh,kw] -> [IC, OC*kh*kw] block layout
  int n_layers;
};

__global__ __launch_bounds__(256)
void adam_t_kernel(float* __restrict__ p, const float* __restrict__ g,
                   float* __restrict__ m, float* __restrict__ v,
                   const int64_t* __restrict__ step, int64_t n,
                   float lr, float b1, float b2, float eps, float wd,
                   float* __restrict__ targ, float rho, ATArgs ta) {
  const float t = (float)step[0];
  const float bc1 = 1.f - powf(b1, t);
  const float bc2 = 1.f - powf(b2, t);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const float pn = adam_elem(p, m, v, targ, i, g[i], lr, b1, b2, eps, wd,
                               bc1, bc2, rho);
    // slabs are offset-sorted (host contract): early-break keeps the
    // per-element search ~O(matching slab); 32-bit local math (weight
    // slabs are < 2^31 elements)
#pragma unroll
    for (int L = 0; L < MAX_T; ++L) {
      if (L >= ta.n_layers || i < ta.off[L]) break;
      const int64_t lo = ta.off[L];
      const int sz = ta.N[L] * ta.K[L] * ta.BS[L];
      if (i < lo + sz) {
        const int loc = (int)(i - lo);
        if (ta.BS[L] == 1) {
          int nn = loc / ta.K[L];
          int kk = loc - nn * ta.K[L];
          ta.wt[L][(int64_t)kk * ta.N[L] + nn] = pn;
        } else {
          // conv [OC,IC,kh,kw] slab: N=OC, K=IC, BS=kh*kw
          const int kb = ta.K[L] * ta.BS[L];
          int nn = loc / kb;
          int r = loc - nn * kb;
          int kk = r / ta.BS[L];
          int e = r - kk * ta.BS[L];
          ta.wt[L][((int64_t)kk * ta.N[L] + nn) * ta.BS[L] + e] = pn;
        }
        break;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------

inline hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

extern bool* g_bf16_flag;  // shared with tac_kernels.hip

inline const float* fptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr<float>() : nullptr;
}

// TAC_AMD_MGEMM_SMALL: 1 (default) routes bf16 launches with M <= 128,
// K <= 256 (K2 <= 256) to mgemm_small_kernel, 0 keeps the pipelined
// kernel for everything.  A plain global so mgemm_small_mode() can flip it
// inside one process.
static int g_small_mode = -1;

static int small_mode() {
  if (g_small_mode < 0) {
    const char* e = getenv("TAC_AMD_MGEMM_SMALL");
    g_small_mode = e ? (atoi(e) != 0) : 1;
  }
  return g_small_mode;
}

int64_t mgemm_small_mode(int64_t mode) {
  const int prev = small_mode();
  TORCH_CHECK(mode == 0 || mode == 1, "mgemm_small_mode: 0 or 1");
  g_small_mode = (int)mode;
  return prev;
}

inline bool small_gate(bool bf16, int split, int nt, int64_t M, int64_t K,
                       bool sum2, int64_t K2) {
  return small_mode() != 0 && bf16 && split == 1 && nt == 1 && M <= 128
         && K <= SKMAX && (!sum2 || K2 <= SKMAX);
}

// One tile shape is built: 32x32.  At M = 64 it spreads a 256-wide layer
// over 16 blocks per problem with 32 + 32 + 32 staged values per thread.
// 64x64 and 32x64 with the same whole-K staging were measured slower on
// every flagship launch (OPTIMIZATION_LOG.md, "Small-shape mgemm").
template <bool MASK, bool RELU, bool SUM2, bool R1>
static void launch_small(const MGemm& g) {
  constexpr int T = 32;
  dim3 grid((unsigned)((g.M + T - 1) / T), (unsigned)((g.N + T - 1) / T),
            (unsigned)g.nz);
  hipLaunchKernelGGL((mgemm_small_kernel<T, T, MASK, RELU, SUM2, R1>), grid,
                     dim3(256), 0, stream(), g);
}

void mgemm(std::vector<torch::Tensor> xs, std::vector<torch::Tensor> ws,
           std::vector<c10::optional<torch::Tensor>> bs,
           std::vector<torch::Tensor> ys,
           std::vector<c10::optional<torch::Tensor>> masks,
           int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldy,
           bool relu,
           std::vector<torch::Tensor> xs2, std::vector<torch::Tensor> ws2,
           std::vector<c10::optional<torch::Tensor>> masks2, int64_t K2,
           int64_t x_off, int64_t x2_off,
           std::vector<int64_t> x_offs) {
  const int nz = (int)xs.size();
  TORCH_CHECK(nz >= 1 && nz <= MAXZ);
  const bool sum2 = !xs2.empty();
  const bool has_mask = masks.size() && masks[0].has_value();
  MGemm g{};
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.lda = (int)lda; g.ldy = (int)ldy; g.K2 = (int)K2;
  for (int z = 0; z < nz; ++z) {
    int64_t xo = x_offs.empty() ? x_off : x_offs[z];
    g.p[z].x = xs[z].data_ptr<float>() + xo;
    g.p[z].w = ws[z].data_ptr<float>();
    g.p[z].bias = fptr(bs[z]);
    g.p[z].y = ys[z].data_ptr<float>();
    g.p[z].mask = masks.size() ? fptr(masks[z]) : nullptr;
    if (g.p[z].mask) g.p[z].mask += (x_offs.empty() ? x_off : x_offs[z]);
    if (sum2) {
      g.p[z].x2 = xs2[z].data_ptr<float>() + x2_off;
      g.p[z].w2 = ws2[z].data_ptr<float>();
      g.p[z].mask2 = masks2.size() ? fptr(masks2[z]) : nullptr;
      if (g.p[z].mask2) g.p[z].mask2 += x2_off;
    }
  }
  const bool bf16 = *g_bf16_flag;
  // split-K for deep-K, few-tile launches (e.g. visual dense 3136->512
  // at batch 64: 8 workgroups un-split on 256 CUs)
  const int BKc = bf16 ? BKP : BKF2;
  const int gx = (int)((M + TB - 1) / TB), gy = (int)((N + TB - 1) / TB);
  const int tiles = gx * gy * nz;
  int split = 1;
  if (!sum2 && K >= 1024 && tiles < 128) {
    const int kchunks = (int)((K + BKc - 1) / BKc);
    split = std::max(1, std::min({kchunks, (256 + tiles - 1) / tiles, 16}));
  }
  int k_chunk = (int)(((K + split - 1) / split + BKc - 1) / BKc * BKc);
  split = (int)((K + k_chunk - 1) / k_chunk);
  g.nz = nz;
  g.k_chunk = k_chunk;
  g.part = nullptr;
  torch::Tensor part;
  if (split > 1) {
    part = torch::empty({(int64_t)split * nz, M * N}, ys[0].options());
    g.part = part.data_ptr<float>();
  }
  // N-tile-reuse variant for large-M shapes (the Humanoid B>=1024
  // regime): one staged A tile serves NT B sub-tiles — A traffic ÷NT.
  // TAC_AMD_MGEMM_NT overrides: 0 = off, 2/4 = force that width.
  static int nt_env = []{
    const char* e = getenv("TAC_AMD_MGEMM_NT");
    return e ? atoi(e) : -1;
  }();
  // NT=2 measured +7.8% on Humanoid B=4096 updates; NT=4 LOSES (-4%):
  // at 1 block/CU the un-prefetched B stages stop hiding latency
  // (gpurun_out/r02nt A/B).
  int nt = 1;
  if (split == 1 && M >= 1024 && gy >= 2)
    nt = 2;
  if (nt_env == 0) nt = 1;
  else if (nt_env > 1 && split == 1 && gy >= 2)
    nt = std::min(nt_env, gy);
  if (small_gate(bf16, split, nt, M, K, sum2, K2)) {
    #define S2(m, r) do { \
        if (sum2) launch_small<m, r, true, false>(g); \
        else launch_small<m, r, false, false>(g); } while (0)
    if (has_mask) { if (relu) S2(true, true); else S2(true, false); }
    else          { if (relu) S2(false, true); else S2(false, false); }
    #undef S2
    return;
  }
  const int gy_nt = (gy + nt - 1) / nt;
  dim3 grid(gx, nt > 1 ? gy_nt : gy, nz * split);
  auto L = [&](auto b, auto m, auto r, auto s) {
    if (nt == 4)
      hipLaunchKernelGGL((mgemm_nt_kernel<decltype(b)::value,
                                          decltype(m)::value,
                                          decltype(r)::value,
                                          decltype(s)::value, 4>),
                         grid, dim3(256), 0, stream(), g);
    else if (nt == 2)
      hipLaunchKernelGGL((mgemm_nt_kernel<decltype(b)::value,
                                          decltype(m)::value,
                                          decltype(r)::value,
                                          decltype(s)::value, 2>),
                         grid, dim3(256), 0, stream(), g);
    else
      hipLaunchKernelGGL((mgemm_kernel<decltype(b)::value,
                                       decltype(m)::value,
                                       decltype(r)::value,
                                       decltype(s)::value>),
                         grid, dim3(256), 0, stream(), g);
  };
  // dispatch over (bf16, mask, relu, sum2)
  #define D2(b, m, r) do { if (sum2) L(b, m, r, std::true_type{}); \
                           else L(b, m, r, std::false_type{}); } while (0)
  #define D1(b, m) do { if (relu) D2(b, m, std::true_type{}); \
                        else D2(b, m, std::false_type{}); } while (0)
  if (bf16) { if (has_mask) D1(std::true_type{}, std::true_type{});
              else D1(std::true_type{}, std::false_type{}); }
  else      { if (has_mask) D1(std::false_type{}, std::true_type{});
              else D1(std::false_type{}, std::false_type{}); }
  #undef D1
  #undef D2
  if (split > 1) {
    int64_t total = (int64_t)M * N * nz;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 512);
    hipLaunchKernelGGL(mgemm_combine_kernel, dim3(blocks), dim3(256), 0,
                       stream(), g, split, relu);
  }
}

// mgemm with a rank-1 A operand: y_z = mask_z(cols_z ⊗ rows_z) @ w_z^T.
// Replaces a K=1 GEMM that only materialised the outer product for the
// next GEMM's staging to read back.  masks are [M, K] contiguous.
void mgemm_r1(std::vector<torch::Tensor> cols,
              std::vector<torch::Tensor> rows,
              std::vector<torch::Tensor> ws, std::vector<torch::Tensor> ys,
              std::vector<torch::Tensor> masks,
              int64_t M, int64_t N, int64_t K, int64_t ldy) {
  const int nz = (int)cols.size();
  TORCH_CHECK(nz >= 1 && nz <= MAXZ && (int)rows.size() == nz
              && (int)ws.size() == nz && (int)ys.size() == nz
              && (int)masks.size() == nz, "mgemm_r1: 1..4 problems");
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && ldy >= N, "mgemm_r1: shape");
  MGemm g{};
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.lda = (int)K; g.ldy = (int)ldy;
  g.nz = nz; g.k_chunk = (int)K; g.part = nullptr;
  for (int z = 0; z < nz; ++z) {
    auto f32c = [](const torch::Tensor& t) {
      return t.is_contiguous() && t.scalar_type() == torch::kFloat32;
    };
    TORCH_CHECK(f32c(cols[z]) && cols[z].numel() == M, "mgemm_r1: col ", z);
    TORCH_CHECK(f32c(rows[z]) && rows[z].numel() == K
                && ((uintptr_t)rows[z].data_ptr<float>() & 15) == 0,
                "mgemm_r1: row ", z, " must be K floats, 16-byte aligned");
    TORCH_CHECK(f32c(ws[z]) && ws[z].numel() == N * K, "mgemm_r1: w ", z);
    TORCH_CHECK(f32c(masks[z]) && masks[z].numel() == M * K,
                "mgemm_r1: mask ", z);
    TORCH_CHECK(ys[z].scalar_type() == torch::kFloat32
                && ys[z].numel() >= (M - 1) * ldy + N, "mgemm_r1: y ", z);
    g.p[z].r1_col = cols[z].data_ptr<float>();
    g.p[z].r1_row = rows[z].data_ptr<float>();
    g.p[z].w = ws[z].data_ptr<float>();
    g.p[z].y = ys[z].data_ptr<float>();
    g.p[z].mask = masks[z].data_ptr<float>();
  }
  if (small_gate(*g_bf16_flag, 1, 1, M, K, false, 0)) {
    launch_small<true, false, false, true>(g);
    return;
  }
  dim3 grid((unsigned)((M + TB - 1) / TB), (unsigned)((N + TB - 1) / TB),
            nz);
  if (*g_bf16_flag)
    hipLaunchKernelGGL((mgemm_kernel<true, true, false, false, true>), grid,
                       dim3(256), 0, stream(), g);
  else
    hipLaunchKernelGGL((mgemm_kernel<false, true, false, false, true>),
                       grid, dim3(256), 0, stream(), g);
}

void mwgrad(std::vector<torch::Tensor> dys,
            std::vector<c10::optional<torch::Tensor>> ymasks,
            std::vector<torch::Tensor> xs,
            std::vector<torch::Tensor> dws, std::vector<torch::Tensor> dbs,
            int64_t M, int64_t N, int64_t K, int64_t lddy, int64_t ldx,
            int64_t x_off) {
  const int nz = (int)dys.size();
  // WGemm holds two problems; every list is indexed by z below
  TORCH_CHECK(nz >= 1 && nz <= 2, "mwgrad: 1..2 problems, got ", nz);
  TORCH_CHECK((int)xs.size() == nz && (int)dws.size() == nz
              && (int)dbs.size() == nz,
              "mwgrad: xs/dws/dbs must hold one entry per problem");
  TORCH_CHECK(ymasks.empty() || (int)ymasks.size() == nz,
              "mwgrad: ymasks must be empty or hold one entry per problem");
  const bool has_mask = ymasks.size() && ymasks[0].has_value();
  // one MASK instantiation serves the whole launch
  for (const auto& ym : ymasks)
    TORCH_CHECK(ym.has_value() == has_mask,
                "mwgrad: masks must be all present or all absent");
  WGemm g{};
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.lddy = (int)lddy; g.ldx = (int)ldx;
  for (int z = 0; z < nz; ++z) {
    g.p[z].dy = dys[z].data_ptr<float>();
    g.p[z].ymask = ymasks.size() ? fptr(ymasks[z]) : nullptr;
    g.p[z].x = xs[z].data_ptr<float>() + x_off;
    g.p[z].dw = dws[z].data_ptr<float>();
    g.p[z].db = dbs[z].numel() ? dbs[z].data_ptr<float>() : nullptr;
  }
  const bool bf16 = *g_bf16_flag;
  const int BKc = bf16 ? BKB2 : BKF2;
  const int chunks = (int)((M + BKc - 1) / BKc);
  const int tiles = (int)(((N + TB - 1) / TB) * ((K + TB - 1) / TB) * nz);
  int split = std::max(1, std::min(chunks, (384 + tiles - 1) / tiles));
  int m_chunk = (int)(((M + split - 1) / split + BKc - 1) / BKc * BKc);
  split = (int)((M + m_chunk - 1) / m_chunk);
  g.nz = nz;
  g.m_chunk = m_chunk;
  g.part = nullptr;
  torch::Tensor part;
  if (split > 1) {
    part = torch::empty({(int64_t)split * nz, (int64_t)N * K + N},
                        dws[0].options());
    g.part = part.data_ptr<float>();
  }
  dim3 grid((N + TB - 1) / TB, (K + TB - 1) / TB, nz * split);
  if (bf16) {
    if (has_mask)
      hipLaunchKernelGGL((mwgrad_kernel<true, true>), grid, dim3(256), 0,
                         stream(), g);
    else
      hipLaunchKernelGGL((mwgrad_kernel<true, false>), grid, dim3(256), 0,
                         stream(), g);
  } else {
    if (has_mask)
      hipLaunchKernelGGL((mwgrad_kernel<false, true>), grid, dim3(256), 0,
                         stream(), g);
    else
      hipLaunchKernelGGL((mwgrad_kernel<false, false>), grid, dim3(256), 0,
                         stream(), g);
  }
  if (split > 1) {
    int64_t total = ((int64_t)N * K + N) * nz;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 512);
    hipLaunchKernelGGL(mwgrad_combine_kernel, dim3(blocks), dim3(256), 0,
                       stream(), part.data_ptr<float>(), g, split);
  }
}

static bool het_xcd() {   // XCD-clustered enumeration flag (read once)
  static int xcd_env = []{
    const char* e = getenv("TAC_AMD_WGRAD_XCD");
    return e ? atoi(e) : 0;
  }();
  return xcd_env == 1;
}

// split-M plan of a heterogeneous wgrad launch of `blk` tiles whose
// deepest problem has maxM rows: slabs along M, rows per slab, and the
// K-steps of the whole M (chunks)
struct HetSplit { int split, m_chunk, chunks; };
static HetSplit het_split(int maxM, int blk) {
  const int BKc = *g_bf16_flag ? BKB2 : BKF2;
  const int chunks = (maxM + BKc - 1) / BKc;
  int split = std::max(1, std::min({chunks, (384 + blk - 1) / blk, 64}));
  const int m_chunk = ((maxM + split - 1) / split + BKc - 1) / BKc * BKc;
  split = (maxM + m_chunk - 1) / m_chunk;
  return {split, m_chunk, chunks};
}

// Host-only: how many M slabs mwgrad_het_adam would use for these shapes
// in the current compute dtype (> 1: the combine kernel applies Adam over
// many blocks; 1: the tile epilogue does).
int64_t mwgrad_het_adam_split(std::vector<int64_t> Ms,
                              std::vector<int64_t> Ns,
                              std::vector<int64_t> Ks) {
  const bool xcd = het_xcd();
  int blk = 0, maxM = 0;
  for (size_t i = 0; i < Ms.size(); ++i) {
    const int bx = (int)((Ns[i] + TB - 1) / TB);
    const int bk_t = (int)((Ks[i] + TB - 1) / TB);
    if (xcd) {
      const int cn = std::min(2, bx), ck = std::min(2, bk_t);
      blk += ((bx + cn - 1) / cn) * ((bk_t + ck - 1) / ck) * cn * ck;
    } else {
      blk += bx * bk_t;
    }
    maxM = std::max(maxM, (int)Ms[i]);
  }
  return blk ? het_split(maxM, blk).split : 1;
}

// `ad` non-null: launch the Adam-carrying instantiations (the 128x128
// sub-tiled body has no Adam epilogue, so that knob is ignored there)
static void mwgrad_het_impl(std::vector<torch::Tensor>& dys,
                std::vector<c10::optional<torch::Tensor>>& ymasks,
                std::vector<torch::Tensor>& xs,
                std::vector<torch::Tensor>& dws,
                std::vector<torch::Tensor>& dbs,
                std::vector<int64_t>& Ms, std::vector<int64_t>& Ns,
                std::vector<int64_t>& Ks, std::vector<int64_t>& lddys,
                std::vector<int64_t>& ldxs, std::vector<int64_t>& x_offs,
                const WAdam* ad) {
  const int np = (int)dys.size();
  TORCH_CHECK(np >= 1 && np <= MAXW, "mwgrad_het: 1..12 problems");
  WHArgs a{};
  a.np = np;
  int blk = 0;
  int64_t poff = 0;
  int maxM = 0;
  const bool xcd = het_xcd();
  for (int i = 0; i < np; ++i) {
    WHProb& p = a.p[i];
    p.dy = dys[i].data_ptr<float>();
    p.ymask = fptr(ymasks[i]);
    p.x = xs[i].data_ptr<float>() + x_offs[i];
    p.dw = dws[i].data_ptr<float>();
    p.db = dbs[i].numel() ? dbs[i].data_ptr<float>() : nullptr;
    p.M = (int)Ms[i]; p.N = (int)Ns[i]; p.K = (int)Ks[i];
    p.lddy = (int)lddys[i]; p.ldx = (int)ldxs[i];
    // 128x128 sub-tiled blocks for large-M problems (bf16 body only):
    // halves the cross-tile dy/x slice re-reads on each doubled axis.
    // MEASURED NEGATIVE at Humanoid/HalfCheetah B=4096 (2345 -> 2053
    // and 3385 -> 2937 updates/s, gpurun_out/r02e vs r02c): the split-M
    // factor grows ~4x on the shrunken block count and the slab
    // combine eats the staged-byte saving; kept behind
    // TAC_AMD_WGRAD_RNRK=1 for re-evaluation.
    static int rnrk_env = []{
      const char* e = getenv("TAC_AMD_WGRAD_RNRK");
      return e ? atoi(e) : 0;
    }();
    const bool big = rnrk_env == 1 && *g_bf16_flag && p.M >= 1024
                     && ad == nullptr;
    p.rn = (big && p.N >= 128) ? 2 : 1;
    p.rk = (big && p.K >= 128) ? 2 : 1;
    p.bx = (p.N + TB * p.rn - 1) / (TB * p.rn);
    p.blk0 = blk;
    p.poff = poff;
    const int bk_t = (p.K + TB * p.rk - 1) / (TB * p.rk);
    if (xcd) {
      p.cn = std::min(2, p.bx);
      p.ck = std::min(2, bk_t);
      p.cx = (p.bx + p.cn - 1) / p.cn;
      const int ckk = (bk_t + p.ck - 1) / p.ck;
      blk += p.cx * ckk * p.cn * p.ck;   // padded to full clusters
    } else {
      p.cn = p.ck = p.cx = 1;
      blk += p.bx * bk_t;
    }
    poff += (int64_t)p.N * p.K + p.N;
    maxM = std::max(maxM, p.M);
  }
  a.enum_total = blk;
  a.xcd_chunk = 0;
  int grid_x = blk;
  if (xcd) {
    const int padded = (blk + 7) & ~7;
    a.xcd_chunk = padded / 8;
    grid_x = padded;
  }
  // split-M across blockIdx.z at large batch (mirrors mwgrad's split;
  // ONE combine covers every problem of the phase)
  const bool bf16 = *g_bf16_flag;
  const HetSplit hs = het_split(maxM, blk);
  const int split = hs.split;
  a.m_chunk = hs.m_chunk;
  a.per_slab = poff;
  a.part = nullptr;
  torch::Tensor part;
  if (split > 1) {
    part = torch::empty({(int64_t)split * poff, 1}, dws[0].options());
    a.part = part.data_ptr<float>();
  }
  dim3 grid(grid_x, 1, split);
  WAdam adk{};
  if (ad) {
    adk = *ad;
    // Quarter epilogues (four blocks per tile) only where repeating the
    // tile's staging + MFMA loop four times is cheap: the whole M is ONE
    // K-step.  A longer un-split launch (>= 384 tiles at any M) keeps one
    // block per tile and the full 16-element epilogue.
    adk.quarter = (split == 1 && hs.chunks == 1) ? 1 : 0;
    if (adk.quarter) grid.x = (unsigned)grid_x * 4;
    if (bf16)
      hipLaunchKernelGGL((mwgrad_het_adam_kernel<true>), grid, dim3(256),
                         0, stream(), a, adk);
    else
      hipLaunchKernelGGL((mwgrad_het_adam_kernel<false>), grid, dim3(256),
                         0, stream(), a, adk);
  } else if (bf16)
    hipLaunchKernelGGL((mwgrad_het_kernel<true>), grid, dim3(256), 0,
                       stream(), a);
  else
    hipLaunchKernelGGL((mwgrad_het_kernel<false>), grid, dim3(256), 0,
                       stream(), a);
  if (split > 1) {
    int blocks = (int)std::min<int64_t>((poff + 255) / 256, 768);
    if (ad)
      hipLaunchKernelGGL(mwgrad_het_combine_adam_kernel, dim3(blocks),
                         dim3(256), 0, stream(), a, split, adk);
    else
      hipLaunchKernelGGL(mwgrad_het_combine_kernel, dim3(blocks),
                         dim3(256), 0, stream(), a, split);
  }
}

void mwgrad_het(std::vector<torch::Tensor> dys,
                std::vector<c10::optional<torch::Tensor>> ymasks,
                std::vector<torch::Tensor> xs,
                std::vector<torch::Tensor> dws,
                std::vector<torch::Tensor> dbs,
                std::vector<int64_t> Ms, std::vector<int64_t> Ns,
                std::vector<int64_t> Ks, std::vector<int64_t> lddys,
                std::vector<int64_t> ldxs, std::vector<int64_t> x_offs) {
  mwgrad_het_impl(dys, ymasks, xs, dws, dbs, Ms, Ns, Ks, lddys, ldxs,
                  x_offs, nullptr);
}

// True when the half-open element ranges [off, off+len) tile [0, n)
// exactly once: no element uncovered, none covered twice.
bool ranges_tile_exactly(std::vector<std::pair<int64_t, int64_t>> r,
                         int64_t n) {
  std::sort(r.begin(), r.end());
  int64_t at = 0;
  for (const auto& q : r) {
    if (q.second <= 0) continue;
    if (q.first != at) return false;
    at += q.second;
  }
  return at == n;
}

// mwgrad_het + Adam (+polyak, +W^T refresh) in ONE launch: each tile
// applies the update to the gradient it holds in registers.  Valid only
// when nothing sits between the wgrad and Adam (single rank) and the
// problems' dW/db slices tile the flat gradient buffer exactly once —
// otherwise some parameter would miss (or double) its step, so raise.
void mwgrad_het_adam(std::vector<torch::Tensor> dys,
                     std::vector<c10::optional<torch::Tensor>> ymasks,
                     std::vector<torch::Tensor> xs,
                     std::vector<torch::Tensor> dws,
                     std::vector<torch::Tensor> dbs,
                     std::vector<int64_t> Ms, std::vector<int64_t> Ns,
                     std::vector<int64_t> Ks, std::vector<int64_t> lddys,
                     std::vector<int64_t> ldxs, std::vector<int64_t> x_offs,
                     torch::Tensor p, torch::Tensor grad, torch::Tensor m,
                     torch::Tensor v, torch::Tensor step, double lr,
                     double b1, double b2, double eps, double wd,
                     std::vector<c10::optional<torch::Tensor>> wts,
                     c10::optional<torch::Tensor> targ, double rho) {
  const int np = (int)dys.size();
  TORCH_CHECK(np >= 1 && np <= MAXW, "mwgrad_het_adam: 1..12 problems");
  TORCH_CHECK((int)wts.size() == np, "mwgrad_het_adam: one wt slot per "
              "problem");
  const int64_t n = grad.numel();
  auto flat_ok = [&](const torch::Tensor& t) {
    return t.is_contiguous() && t.scalar_type() == torch::kFloat32
        && t.numel() == n;
  };
  TORCH_CHECK(flat_ok(p) && flat_ok(grad) && flat_ok(m) && flat_ok(v),
              "mwgrad_het_adam: p/grad/m/v must be contiguous fp32 of one "
              "size");
  TORCH_CHECK(!targ.has_value() || flat_ok(*targ),
              "mwgrad_het_adam: target size");
  const float* gbase = grad.data_ptr<float>();
  std::vector<std::pair<int64_t, int64_t>> ranges;
  WAdam ad{};
  for (int i = 0; i < np; ++i) {
    const int64_t nk = Ns[i] * Ks[i];
    TORCH_CHECK(dws[i].is_contiguous() && dws[i].numel() == nk,
                "mwgrad_het_adam: dw ", i, " is not a contiguous [N,K]");
    ranges.push_back({dws[i].data_ptr<float>() - gbase, nk});
    if (dbs[i].numel()) {
      TORCH_CHECK(dbs[i].is_contiguous() && dbs[i].numel() == Ns[i],
                  "mwgrad_het_adam: db ", i);
      ranges.push_back({dbs[i].data_ptr<float>() - gbase, Ns[i]});
    }
    ad.wt[i] = nullptr;
    if (wts[i].has_value()) {
      TORCH_CHECK(wts[i]->is_contiguous() && wts[i]->numel() == nk
                  && wts[i]->scalar_type() == torch::kFloat32,
                  "mwgrad_het_adam: wt ", i, " must be a contiguous [K,N]");
      ad.wt[i] = wts[i]->data_ptr<float>();
    }
  }
  TORCH_CHECK(ranges_tile_exactly(ranges, n),
              "mwgrad_het_adam: the problems' dW/db slices do not tile the "
              "flat gradient buffer exactly once");
  ad.p = p.data_ptr<float>();
  ad.m = m.data_ptr<float>();
  ad.v = v.data_ptr<float>();
  ad.targ = targ.has_value() ? targ->data_ptr<float>() : nullptr;
  ad.grad = gbase;
  ad.step = step.data_ptr<int64_t>();
  ad.lr = (float)lr; ad.b1 = (float)b1; ad.b2 = (float)b2;
  ad.eps = (float)eps; ad.wd = (float)wd; ad.rho = (float)rho;
  mwgrad_het_impl(dys, ymasks, xs, dws, dbs, Ms, Ns, Ks, lddys, ldxs,
                  x_offs, &ad);
}

void transpose_multi(std::vector<torch::Tensor> ws,
                     std::vector<torch::Tensor> wts,
                     std::vector<int64_t> blocks) {
  TArgs t{};
  t.n_layers = (int)ws.size();
  TORCH_CHECK(t.n_layers <= MAX_T);
  for (int i = 0; i < t.n_layers; ++i) {
    t.w[i] = ws[i].data_ptr<float>();
    t.wt[i] = wts[i].data_ptr<float>();
    t.N[i] = (int)ws[i].size(0);
    t.K[i] = (int)ws[i].size(1);
    t.BS[i] = blocks.empty() ? 1 : (int)blocks[i];
    TORCH_CHECK((int64_t)t.N[i] * t.K[i] * t.BS[i] == ws[i].numel());
  }
  int64_t max_elems = 0;
  for (int i = 0; i < t.n_layers; ++i)
    max_elems = std::max(max_elems,
                         (int64_t)t.N[i] * t.K[i] * t.BS[i]);
  t.blocks_per_layer = (int)std::min<int64_t>(
      128, std::max<int64_t>(8, (max_elems + 4095) / 4096));
  hipLaunchKernelGGL(transpose_multi_kernel,
                     dim3(t.n_layers * t.blocks_per_layer), dim3(256), 0,
                     stream(), t);
}

// Replay gather writing straight into the concat-layout batch buffers
// XC [2B, ldc] / XC2 [B, ldc]: one launch, keyed on ctr[0] + ctr_add so a
// reader can run ahead of the counter bump.  gather2n carries n-step
// returns, gather2p draws from the sum tree (either n).
inline ConcatSink concat_sink(const torch::Tensor& xc,
                              const torch::Tensor& xc2, int64_t B,
                              const torch::Tensor& state) {
  return {xc.data_ptr<float>(), xc2.data_ptr<float>(), (int)B,
          (int)xc.size(1), (int)state.size(1)};
}

void gather2(torch::Tensor state, torch::Tensor act, torch::Tensor rew,
             torch::Tensor nstate, torch::Tensor done,
             torch::Tensor size_dev, torch::Tensor ctr, int64_t seed,
             torch::Tensor xc, torch::Tensor xc2, torch::Tensor orew,
             torch::Tensor od, int64_t B, int64_t ctr_add) {
  const RingArgs ring{state, act, rew, nstate, done, nullptr, size_dev,
                      nullptr, ctr};
  const BatchArgs out{xc, xc2, nullptr, orew, od, nullptr, nullptr, nullptr};
  gather_gate("gather2", ring, 1, B, out);
  launch_gather<Draw::Uniform>(stream(), ring, nullptr, PerLay{}, ctr_add,
                               seed, 1, 1.0, concat_sink(xc, xc2, B, state),
                               out, B);
}

void gather2n(torch::Tensor state, torch::Tensor act, torch::Tensor rew,
              torch::Tensor nstate, torch::Tensor done, torch::Tensor ep_end,
              torch::Tensor size_dev, torch::Tensor ptr_dev,
              torch::Tensor ctr, int64_t seed, int64_t n, double gamma,
              torch::Tensor xc, torch::Tensor xc2, torch::Tensor orew,
              torch::Tensor od, int64_t B, int64_t ctr_add) {
  const RingArgs ring{state, act, rew, nstate, done, &ep_end, size_dev,
                      &ptr_dev, ctr};
  const BatchArgs out{xc, xc2, nullptr, orew, od, nullptr, nullptr, nullptr};
  gather_gate("gather2n", ring, n, B, out);
  launch_gather<Draw::UniformN>(stream(), ring, nullptr, PerLay{}, ctr_add,
                                seed, n, gamma,
                                concat_sink(xc, xc2, B, state), out, B);
}

void gather2p(torch::Tensor state, torch::Tensor act, torch::Tensor rew,
              torch::Tensor nstate, torch::Tensor done, torch::Tensor ep_end,
              torch::Tensor size_dev, torch::Tensor ptr_dev,
              torch::Tensor tree, torch::Tensor ctr, int64_t seed, int64_t n,
              double gamma, torch::Tensor xc, torch::Tensor xc2,
              torch::Tensor orew, torch::Tensor od, torch::Tensor idx_out,
              torch::Tensor prob_out, c10::optional<torch::Tensor> u_out,
              int64_t B, int64_t ctr_add) {
  const RingArgs ring{state, act, rew, nstate, done, &ep_end, size_dev,
                      &ptr_dev, ctr};
  const BatchArgs out{xc, xc2, nullptr, orew, od, &idx_out, &prob_out,
                      u_out.has_value() ? &*u_out : nullptr};
  gather_gate("gather2p", ring, n, B, out);
  const PerLay lay = per_tree_layout(tree, state.size(0), "gather2p");
  launch_gather<Draw::Tree>(stream(), ring, &tree, lay, ctr_add, seed, n,
                            gamma, concat_sink(xc, xc2, B, state), out, B);
}

void per_update(torch::Tensor tree, int64_t cap, torch::Tensor idx,
                torch::Tensor td, double alpha, double eps,
                torch::Tensor max_priority) {
  PerLay lay = per_tree_layout(tree, cap, "per_update");
  const int64_t B = idx.numel();
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31) && idx.is_cuda() &&
              idx.is_contiguous() && idx.dtype() == torch::kInt64 &&
              td.is_cuda() && td.is_contiguous() &&
              td.dtype() == torch::kFloat32 && td.numel() >= B,
              "per_update: idx must be int64 [B], td fp32 [B], on the device");
  TORCH_CHECK(max_priority.is_cuda() &&
              max_priority.dtype() == torch::kFloat32 &&
              max_priority.numel() == 1,
              "per_update: max_priority must be an fp32 [1] device tensor");
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(PER_THREADS), 0,
                     stream(), tree.data_ptr<float>(), lay,
                     idx.data_ptr<int64_t>(), td.data_ptr<float>(), (int)B,
                     (float)alpha, (float)eps,
                     max_priority.data_ptr<float>());
}

void per_set_range(torch::Tensor tree, int64_t cap, int64_t start,
                   int64_t count, torch::Tensor max_priority) {
  PerLay lay = per_tree_layout(tree, cap, "per_set_range");
  TORCH_CHECK(start >= 0 && start < cap && count >= 1 && count <= cap,
              "per_set_range: range outside the ring");
  TORCH_CHECK(max_priority.is_cuda() &&
              max_priority.dtype() == torch::kFloat32 &&
              max_priority.numel() == 1,
              "per_set_range: max_priority must be an fp32 [1] device tensor");
  hipLaunchKernelGGL(per_set_range_kernel, dim3(1), dim3(PER_THREADS), 0,
                     stream(), tree.data_ptr<float>(), lay, start, count,
                     max_priority.data_ptr<float>());
}

// Host gates of the head / loss / temperature bindings below: every
// operand is checked before the launch, so a refused call touches nothing.
inline void need_f32(const torch::Tensor& t, int64_t n, const char* op,
                     const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
              t.is_contiguous() && t.numel() >= n, op, ": ", name,
              " must be a contiguous fp32 device tensor of at least ", n,
              " elements");
}

inline void need_f32_opt(const c10::optional<torch::Tensor>& t, int64_t n,
                         const char* op, const char* name) {
  if (t.has_value()) need_f32(*t, n, op, name);
}

inline void need_scalar_f32(const torch::Tensor& t, const char* op,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
              t.numel() == 1, op, ": ", name,
              " must be an fp32 device tensor of one element");
}

inline void need_scalar_i64(const torch::Tensor& t, const char* op,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt64 &&
              t.numel() == 1, op, ": ", name,
              " must be an int64 device tensor of one element");
}

// hl = [R, 2A] (mu | log_std), one 64-lane block per row; returns A
inline int need_hl(const torch::Tensor& hl, int64_t min_rows, const char* op) {
  TORCH_CHECK(hl.dim() == 2 && hl.size(0) >= 1 && hl.size(0) >= min_rows &&
              hl.size(0) < (int64_t(1) << 31) && hl.size(1) >= 2 &&
              hl.size(1) % 2 == 0, op, ": hl must be [R, 2A] with R >= ",
              min_rows < 1 ? 1 : min_rows);
  need_f32(hl, 0, op, "hl");
  const int64_t A = hl.size(1) / 2;
  TORCH_CHECK(A <= 64, op, ": A = ", A,
              " exceeds the 64 lanes a row's block has");
  return (int)A;
}

// A [rows, A] block of a 2-D slab starting `off` elements into it: off may
// carry whole rows (the engine addresses rows B.. of XC that way); the
// block must stay inside the slab's columns and rows.
inline void need_slab(const torch::Tensor& t, int64_t off, int64_t rows,
                      int64_t A, const char* op, const char* name) {
  need_f32(t, 0, op, name);
  TORCH_CHECK(t.dim() == 2 && t.size(1) >= 1, op, ": ", name,
              " must be 2-D");
  const int64_t ld = t.size(1);
  TORCH_CHECK(off >= 0 && off % ld + A <= ld, op, ": columns [", off % ld,
              ", ", off % ld + A, ") leave ", name, "'s ", ld, " columns");
  TORCH_CHECK(off / ld + rows <= t.size(0), op, ": ", name, " has ",
              t.size(0), " rows, ", off / ld + rows, " needed");
}

// fused K = 1 dgrad operands of the loss kernels: all four or none
inline bool need_fuse(const c10::optional<torch::Tensor>& wt3_0,
                      const c10::optional<torch::Tensor>& wt3_1,
                      const c10::optional<torch::Tensor>& dy2_0,
                      const c10::optional<torch::Tensor>& dy2_1,
                      int64_t B, int64_t h2, const char* op) {
  const bool fuse = dy2_0.has_value();
  if (!fuse) {
    TORCH_CHECK(!dy2_1.has_value(), op, ": dy2_1 given without dy2_0");
    return false;
  }
  TORCH_CHECK(B <= LOSS_MAXB, op, ": the fused dgrad stages dq in LDS and "
              "takes at most ", LOSS_MAXB, " rows, got ", B);
  TORCH_CHECK(wt3_0.has_value() && wt3_1.has_value() && dy2_1.has_value() &&
              h2 >= 1, op, ": the fused dgrad needs wt3_0, wt3_1, dy2_0, "
              "dy2_1 and h2 >= 1");
  need_f32(*wt3_0, h2, op, "wt3_0");
  need_f32(*wt3_1, h2, op, "wt3_1");
  need_f32(*dy2_0, B * h2, op, "dy2_0");
  need_f32(*dy2_1, B * h2, op, "dy2_1");
  return true;
}

void tg_fwd2(torch::Tensor hl, torch::Tensor out0,
             int64_t col0, torch::Tensor out1, int64_t col1, int64_t B0,
             torch::Tensor logp, torch::Tensor prob, torch::Tensor ctr,
             int64_t seed, double act_limit, double lo, double hi,
             int64_t ctr_add) {
  const int A = need_hl(hl, 1, "tg_fwd2");
  const int R = (int)hl.size(0);
  TORCH_CHECK(B0 >= 0 && B0 <= R, "tg_fwd2: B0 = ", B0, " outside [0, R = ",
              R, "]");
  need_slab(out0, col0, B0, A, "tg_fwd2", "out0");
  need_slab(out1, col1, R - B0, A, "tg_fwd2", "out1");
  need_f32(logp, R, "tg_fwd2", "logp");
  need_f32(prob, (int64_t)R * A, "tg_fwd2", "prob");
  need_scalar_i64(ctr, "tg_fwd2", "ctr");
  hipLaunchKernelGGL(tg_fwd2_kernel, dim3(R), dim3(64), 0, stream(),
                     hl.data_ptr<float>(),
                     out0.data_ptr<float>() + col0, (int)out0.size(1),
                     out1.data_ptr<float>() + col1, (int)out1.size(1),
                     (int)B0, logp.data_ptr<float>(), prob.data_ptr<float>(),
                     ctr.data_ptr<int64_t>(), ctr_add, (uint64_t)seed, R, A,
                     (float)act_limit, (float)lo, (float)hi);
}

void tg_bwd2(torch::Tensor dxc, int64_t col0,
             c10::optional<torch::Tensor> dxc2,
             c10::optional<torch::Tensor> alpha_dev, double alpha_host,
             torch::Tensor hl, torch::Tensor prob,
             torch::Tensor dmu, torch::Tensor dls, int64_t B,
             double act_limit, double lo, double hi) {
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31), "tg_bwd2: B must be >= 1");
  const int A = need_hl(hl, B, "tg_bwd2");
  need_f32(dmu, 0, "tg_bwd2", "dmu");
  need_f32(dls, 0, "tg_bwd2", "dls");
  TORCH_CHECK(dmu.dim() == 2 && dmu.size(0) == B && dmu.size(1) == A &&
              dls.dim() == 2 && dls.size(0) == B && dls.size(1) == A,
              "tg_bwd2: dmu and dls must be [B, A] = [", B, ", ", A, "]");
  need_f32(prob, B * A, "tg_bwd2", "prob");
  TORCH_CHECK(col0 < (int64_t(1) << 31) &&
              (dxc.dim() != 2 || col0 < dxc.size(1)),
              "tg_bwd2: col0 is a column of dxc");
  need_slab(dxc, col0, B, A, "tg_bwd2", "dxc");
  if (dxc2.has_value()) {
    need_f32(*dxc2, 0, "tg_bwd2", "dxc2");
    TORCH_CHECK(dxc2->sizes() == dxc.sizes(),
                "tg_bwd2: dxc2 must have dxc's shape");
  }
  if (alpha_dev.has_value())
    need_scalar_f32(*alpha_dev, "tg_bwd2", "alpha_dev");
  hipLaunchKernelGGL(tg_bwd2_kernel, dim3((int)B), dim3(64), 0, stream(),
                     dxc.data_ptr<float>(), (int)dxc.size(1), (int)col0,
                     fptr(dxc2),
                     fptr(alpha_dev), (float)alpha_host,
                     hl.data_ptr<float>(),
                     prob.data_ptr<float>(), dmu.data_ptr<float>(),
                     dls.data_ptr<float>(), (int)B, A, (float)act_limit,
                     (float)lo, (float)hi);
}

void qloss2(torch::Tensor q1, torch::Tensor q2, torch::Tensor q1t,
            torch::Tensor q2t, torch::Tensor logp_next, torch::Tensor rew,
            torch::Tensor done, c10::optional<torch::Tensor> alpha_dev,
            double alpha_host, torch::Tensor loss_acc, torch::Tensor dq1,
            torch::Tensor dq2, int64_t B, double gamma, double scale,
            c10::optional<torch::Tensor> wt3_0,
            c10::optional<torch::Tensor> wt3_1,
            c10::optional<torch::Tensor> dy2_0,
            c10::optional<torch::Tensor> dy2_1, int64_t h2,
            c10::optional<torch::Tensor> bump0,
            c10::optional<torch::Tensor> bump1,
            c10::optional<torch::Tensor> bump2,
            c10::optional<torch::Tensor> prob,
            c10::optional<torch::Tensor> size_dev,
            c10::optional<torch::Tensor> beta_dev,
            c10::optional<torch::Tensor> td) {
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31), "qloss2: B must be >= 1");
  const bool fuse = need_fuse(wt3_0, wt3_1, dy2_0, dy2_1, B, h2, "qloss2");
  need_f32(q1, B, "qloss2", "q1");
  need_f32(q2, B, "qloss2", "q2");
  need_f32(q1t, B, "qloss2", "q1t");
  need_f32(q2t, B, "qloss2", "q2t");
  need_f32(logp_next, B, "qloss2", "logp_next");
  need_f32(rew, B, "qloss2", "rew");
  need_f32(done, B, "qloss2", "done");
  need_f32(dq1, B, "qloss2", "dq1");
  need_f32(dq2, B, "qloss2", "dq2");
  need_scalar_f32(loss_acc, "qloss2", "loss_acc");
  if (alpha_dev.has_value())
    need_scalar_f32(*alpha_dev, "qloss2", "alpha_dev");
  if (bump0.has_value()) need_scalar_i64(*bump0, "qloss2", "bump0");
  if (bump1.has_value()) need_scalar_i64(*bump1, "qloss2", "bump1");
  if (bump2.has_value()) need_scalar_i64(*bump2, "qloss2", "bump2");
  auto iptr = [](const c10::optional<torch::Tensor>& t) -> int64_t* {
    return t.has_value() ? t->data_ptr<int64_t>() : nullptr;
  };
  const bool weighted = prob.has_value();
  if (weighted) {
    TORCH_CHECK(size_dev.has_value() && beta_dev.has_value() &&
                td.has_value(),
                "qloss2: prob needs size_dev, beta_dev and td");
    TORCH_CHECK(prob->is_cuda() && prob->is_contiguous() &&
                prob->dtype() == torch::kFloat32 && prob->numel() >= B &&
                td->is_cuda() && td->is_contiguous() &&
                td->dtype() == torch::kFloat32 && td->numel() >= B &&
                beta_dev->is_cuda() && beta_dev->dtype() == torch::kFloat32 &&
                beta_dev->numel() == 1 && size_dev->is_cuda() &&
                size_dev->dtype() == torch::kInt64 && size_dev->numel() == 1,
                "qloss2: bad prioritized-replay arguments");
  }
  auto kernel = weighted ? qloss2_kernel<true> : qloss2_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(256), 0, stream(),
                     q1.data_ptr<float>(), q2.data_ptr<float>(),
                     q1t.data_ptr<float>(), q2t.data_ptr<float>(),
                     logp_next.data_ptr<float>(), rew.data_ptr<float>(),
                     done.data_ptr<float>(), fptr(alpha_dev),
                     (float)alpha_host, loss_acc.data_ptr<float>(),
                     dq1.data_ptr<float>(), dq2.data_ptr<float>(), (int)B,
                     (float)gamma, (float)scale,
                     fuse ? fptr(wt3_0) : nullptr,
                     fuse ? fptr(wt3_1) : nullptr,
                     fuse ? dy2_0->data_ptr<float>() : nullptr,
                     fuse ? dy2_1->data_ptr<float>() : nullptr, (int)h2,
                     iptr(bump0), iptr(bump1), iptr(bump2), fptr(prob),
                     weighted ? size_dev->data_ptr<int64_t>() : nullptr,
                     fptr(beta_dev),
                     weighted ? td->data_ptr<float>() : nullptr);
}

void piloss2(torch::Tensor q1, torch::Tensor q2, torch::Tensor logp,
             c10::optional<torch::Tensor> alpha_dev, double alpha_host,
             torch::Tensor loss_acc, c10::optional<torch::Tensor> mean_logp,
             torch::Tensor dq1, torch::Tensor dq2, int64_t B,
             c10::optional<torch::Tensor> wt3_0,
             c10::optional<torch::Tensor> wt3_1,
             c10::optional<torch::Tensor> dy2_0,
             c10::optional<torch::Tensor> dy2_1, int64_t h2) {
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31), "piloss2: B must be >= 1");
  const bool fuse = need_fuse(wt3_0, wt3_1, dy2_0, dy2_1, B, h2, "piloss2");
  need_f32(q1, B, "piloss2", "q1");
  need_f32(q2, B, "piloss2", "q2");
  need_f32(logp, B, "piloss2", "logp");
  need_f32(dq1, B, "piloss2", "dq1");
  need_f32(dq2, B, "piloss2", "dq2");
  need_scalar_f32(loss_acc, "piloss2", "loss_acc");
  if (alpha_dev.has_value())
    need_scalar_f32(*alpha_dev, "piloss2", "alpha_dev");
  if (mean_logp.has_value())
    need_scalar_f32(*mean_logp, "piloss2", "mean_logp");
  hipLaunchKernelGGL(piloss2_kernel, dim3(1), dim3(256), 0, stream(),
                     q1.data_ptr<float>(), q2.data_ptr<float>(),
                     logp.data_ptr<float>(), fptr(alpha_dev),
                     (float)alpha_host, loss_acc.data_ptr<float>(),
                     mean_logp.has_value() ? mean_logp->data_ptr<float>()
                                           : nullptr,
                     dq1.data_ptr<float>(), dq2.data_ptr<float>(), (int)B,
                     fptr(wt3_0), fptr(wt3_1),
                     fuse ? dy2_0->data_ptr<float>() : nullptr,
                     fuse ? dy2_1->data_ptr<float>() : nullptr, (int)h2);
}

// ---------------------------------------------------------------------------
// mgemm_r1 with the column computed from a loss kernel's inputs: the launch
// replaces qloss2 + the K=1 dgrad + the masked dgrad (mgemm_r1_qloss), or
// piloss2 + mgemm_r1 (mgemm_r1_piloss), bit for bit.  Only the small-shape
// bf16 kernel has the folded form; mgemm_r1_fold_ok is its host gate.
// ---------------------------------------------------------------------------

bool mgemm_r1_fold_ok(int64_t M, int64_t K) {
  return M >= 1 && K >= 1 && small_gate(*g_bf16_flag, 1, 1, M, K, false, 0);
}

// the operands the two folded entries share with mgemm_r1 (nz == 2)
static void fold_gemm_args(MGemm& g, const char* op,
                           const std::vector<torch::Tensor>& rows,
                           const std::vector<torch::Tensor>& ws,
                           const std::vector<torch::Tensor>& ys,
                           const std::vector<torch::Tensor>& masks,
                           int64_t M, int64_t N, int64_t K, int64_t ldy) {
  TORCH_CHECK(rows.size() == 2 && ws.size() == 2 && ys.size() == 2
              && masks.size() == 2, op, ": exactly 2 problems (nz == 2)");
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && ldy >= N, op, ": shape");
  TORCH_CHECK(mgemm_r1_fold_ok(M, K), op, ": outside the small-shape gate "
              "(bf16 compute, M <= 128, K <= ", SKMAX, ", small mode on)");
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.lda = (int)K; g.ldy = (int)ldy;
  g.nz = 2; g.k_chunk = (int)K; g.part = nullptr;
  for (int z = 0; z < 2; ++z) {
    need_f32(rows[z], 0, op, "row");
    TORCH_CHECK(rows[z].numel() == K
                && ((uintptr_t)rows[z].data_ptr<float>() & 15) == 0,
                op, ": row ", z, " must be K floats, 16-byte aligned");
    need_f32(ws[z], 0, op, "w");
    TORCH_CHECK(ws[z].numel() == N * K, op, ": w ", z);
    need_f32(masks[z], 0, op, "mask");
    TORCH_CHECK(masks[z].numel() == M * K, op, ": mask ", z);
    TORCH_CHECK(ys[z].is_cuda() && ys[z].scalar_type() == torch::kFloat32
                && ys[z].numel() >= (M - 1) * ldy + N, op, ": y ", z);
    g.p[z].r1_row = rows[z].data_ptr<float>();
    g.p[z].w = ws[z].data_ptr<float>();
    g.p[z].y = ys[z].data_ptr<float>();
    g.p[z].mask = masks[z].data_ptr<float>();
  }
}

static void need_vecM(const torch::Tensor& t, int64_t M, const char* op,
                      const char* name) {
  need_f32(t, M, op, name);
  TORCH_CHECK(t.numel() == M, op, ": ", name, " must hold M = ", M,
              " elements");
}

template <int LF>
static void launch_small_fold(const MGemm& g, const LossFold& lf) {
  constexpr int T = 32;
  // the reducing block holds one batch row per thread (fold_preload)
  TORCH_CHECK(g.M <= 256, "folded loss: M must not exceed the block size");
  dim3 grid((unsigned)((g.M + T - 1) / T), (unsigned)((g.N + T - 1) / T), 2);
  hipLaunchKernelGGL((mgemm_small_kernel<T, T, true, false, false, true, LF,
                                         LossFold>),
                     grid, dim3(256), 0, stream(), g, lf);
}

void mgemm_r1_qloss(torch::Tensor q1, torch::Tensor q2, torch::Tensor q1t,
                    torch::Tensor q2t, torch::Tensor logp_next,
                    torch::Tensor rew, torch::Tensor done,
                    c10::optional<torch::Tensor> alpha_dev, double alpha_host,
                    torch::Tensor loss_acc, torch::Tensor dq1,
                    torch::Tensor dq2, double gamma, double scale,
                    c10::optional<torch::Tensor> bump0,
                    c10::optional<torch::Tensor> bump1,
                    c10::optional<torch::Tensor> bump2,
                    std::vector<torch::Tensor> rows,
                    std::vector<torch::Tensor> ws,
                    std::vector<torch::Tensor> ys,
                    std::vector<torch::Tensor> masks,
                    std::vector<torch::Tensor> outers,
                    int64_t M, int64_t N, int64_t K, int64_t ldy) {
  const char* op = "mgemm_r1_qloss";
  MGemm g{};
  fold_gemm_args(g, op, rows, ws, ys, masks, M, N, K, ldy);
  need_vecM(q1, M, op, "q1");
  need_vecM(q2, M, op, "q2");
  need_vecM(q1t, M, op, "q1t");
  need_vecM(q2t, M, op, "q2t");
  need_vecM(logp_next, M, op, "logp_next");
  need_vecM(rew, M, op, "rew");
  need_vecM(done, M, op, "done");
  need_vecM(dq1, M, op, "dq1");
  need_vecM(dq2, M, op, "dq2");
  need_scalar_f32(loss_acc, op, "loss_acc");
  if (alpha_dev.has_value()) need_scalar_f32(*alpha_dev, op, "alpha_dev");
  if (bump0.has_value()) need_scalar_i64(*bump0, op, "bump0");
  if (bump1.has_value()) need_scalar_i64(*bump1, op, "bump1");
  if (bump2.has_value()) need_scalar_i64(*bump2, op, "bump2");
  TORCH_CHECK(outers.size() == 2, op, ": exactly 2 outer-product buffers");
  for (int z = 0; z < 2; ++z) {
    need_f32(outers[z], M * K, op, "outer");
    TORCH_CHECK(((uintptr_t)outers[z].data_ptr<float>() & 15) == 0, op,
                ": outer ", z, " must be 16-byte aligned");
  }
  auto iptr = [](const c10::optional<torch::Tensor>& t) -> int64_t* {
    return t.has_value() ? t->data_ptr<int64_t>() : nullptr;
  };
  LossFold lf{};
  lf.in = QIn{q1.data_ptr<float>(), q2.data_ptr<float>(),
              q1t.data_ptr<float>(), q2t.data_ptr<float>(),
              logp_next.data_ptr<float>(), rew.data_ptr<float>(),
              done.data_ptr<float>()};
  lf.alpha_dev = fptr(alpha_dev);
  lf.alpha_host = (float)alpha_host;
  lf.gamma = (float)gamma;
  lf.scale = (float)scale;
  lf.loss_acc = loss_acc.data_ptr<float>();
  lf.dq[0] = dq1.data_ptr<float>();
  lf.dq[1] = dq2.data_ptr<float>();
  lf.outer[0] = outers[0].data_ptr<float>();
  lf.outer[1] = outers[1].data_ptr<float>();
  lf.bump[0] = iptr(bump0);
  lf.bump[1] = iptr(bump1);
  lf.bump[2] = iptr(bump2);
  launch_small_fold<2>(g, lf);
}

void mgemm_r1_piloss(torch::Tensor q1, torch::Tensor q2, torch::Tensor logp,
                     c10::optional<torch::Tensor> alpha_dev,
                     double alpha_host, torch::Tensor loss_acc,
                     c10::optional<torch::Tensor> mean_logp,
                     torch::Tensor dq1, torch::Tensor dq2,
                     std::vector<torch::Tensor> rows,
                     std::vector<torch::Tensor> ws,
                     std::vector<torch::Tensor> ys,
                     std::vector<torch::Tensor> masks,
                     int64_t M, int64_t N, int64_t K, int64_t ldy) {
  const char* op = "mgemm_r1_piloss";
  MGemm g{};
  fold_gemm_args(g, op, rows, ws, ys, masks, M, N, K, ldy);
  need_vecM(q1, M, op, "q1");
  need_vecM(q2, M, op, "q2");
  need_vecM(logp, M, op, "logp");
  need_vecM(dq1, M, op, "dq1");
  need_vecM(dq2, M, op, "dq2");
  need_scalar_f32(loss_acc, op, "loss_acc");
  if (alpha_dev.has_value()) need_scalar_f32(*alpha_dev, op, "alpha_dev");
  if (mean_logp.has_value()) need_scalar_f32(*mean_logp, op, "mean_logp");
  LossFold lf{};
  lf.in.q1 = q1.data_ptr<float>();
  lf.in.q2 = q2.data_ptr<float>();
  lf.in.lpn = logp.data_ptr<float>();
  lf.alpha_dev = fptr(alpha_dev);
  lf.alpha_host = (float)alpha_host;
  lf.loss_acc = loss_acc.data_ptr<float>();
  lf.mean_logp = mean_logp.has_value() ? mean_logp->data_ptr<float>()
                                         : nullptr;
  lf.dq[0] = dq1.data_ptr<float>();
  lf.dq[1] = dq2.data_ptr<float>();
  launch_small_fold<1>(g, lf);
}

void adam_t(torch::Tensor p, torch::Tensor g, torch::Tensor m,
            torch::Tensor v, torch::Tensor step, double lr, double b1,
            double b2, double eps, double wd,
            std::vector<int64_t> offsets, std::vector<torch::Tensor> wts,
            c10::optional<torch::Tensor> targ, double rho,
            std::vector<int64_t> bss) {
  ATArgs ta{};
  ta.n_layers = (int)offsets.size();
  TORCH_CHECK(ta.n_layers <= MAX_T);
  TORCH_CHECK(wts.size() == offsets.size(),
              "adam_t: one W^T cache per slab offset");
  TORCH_CHECK(bss.empty() || bss.size() == offsets.size(),
              "adam_t: bss must be empty or hold one entry per slab");
  // the kernel's slab search stops at the first offset above the
  // element: unsorted or overlapping slabs would leave a cache stale
  int64_t slab_end = 0;
  for (int i = 0; i < ta.n_layers; ++i) {
    TORCH_CHECK(offsets[i] >= slab_end,
                "adam_t: slab offsets must be strictly increasing and the "
                "slabs must not overlap (slab ", i, ")");
    slab_end = offsets[i] + wts[i].numel();
    TORCH_CHECK(wts[i].numel() > 0 && slab_end <= p.numel(),
                "adam_t: slab ", i, " does not lie inside [0, n)");
  }
  for (int i = 0; i < ta.n_layers; ++i) {
    ta.off[i] = offsets[i];
    ta.wt[i] = wts[i].data_ptr<float>();
    ta.BS[i] = bss.empty() ? 1 : (int)bss[i];
    TORCH_CHECK(wts[i].dim() == 2 && ta.BS[i] >= 1
                && wts[i].size(1) % ta.BS[i] == 0,
                "adam_t: W^T cache ", i, " must be [K, N * bs]");
    if (ta.BS[i] == 1) {
      ta.K[i] = (int)wts[i].size(0);   // dense: wt is [K, N]
      ta.N[i] = (int)wts[i].size(1);
    } else {
      ta.K[i] = (int)wts[i].size(0);   // conv: wt is [IC, OC*kh*kw]
      ta.N[i] = (int)(wts[i].size(1) / ta.BS[i]);
    }
  }
  int64_t n = p.numel();
  if (targ.has_value()) TORCH_CHECK(targ->numel() == n);
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(adam_t_kernel, dim3(blocks), dim3(256), 0, stream(),
                     p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     step.data_ptr<int64_t>(), n, (float)lr, (float)b1,
                     (float)b2, (float)eps, (float)wd,
                     targ.has_value() ? targ->data_ptr<float>() : nullptr,
                     (float)rho, ta);
}

torch::Tensor tg_eps(int64_t ctr_val, int64_t seed, int64_t R, int64_t A,
                     torch::Tensor like) {
  TORCH_CHECK(A >= 1 && A <= 64, "tg_eps: A = ", A,
              " outside 1..64 (one 64-lane block per row)");
  TORCH_CHECK(R >= 1 && R < (int64_t(1) << 31), "tg_eps: R must be >= 1");
  TORCH_CHECK(like.is_cuda() && like.scalar_type() == torch::kFloat32,
              "tg_eps: `like` must be an fp32 device tensor");
  auto out = torch::empty({R, A}, like.options());
  hipLaunchKernelGGL(tg_eps_kernel, dim3((int)R), dim3(64), 0, stream(),
                     out.data_ptr<float>(), (uint64_t)ctr_val,
                     (uint64_t)seed, (int)R, (int)A);
  return out;
}

// The one marshalling of a single-state act launch's arguments.
static ActArgs act_args(const torch::Tensor& x,
                        const std::vector<torch::Tensor>& ws,
                        const std::vector<torch::Tensor>& bs,
                        const torch::Tensor& wmu, const torch::Tensor& bmu,
                        const torch::Tensor& wls, const torch::Tensor& bls,
                        const torch::Tensor& action,
                        const torch::Tensor& ctr, int64_t seed,
                        double act_limit, double lo, double hi) {
  ActArgs a{};
  a.n_layers = (int)ws.size();
  TORCH_CHECK(a.n_layers <= ACT_MAXL);
  a.x = x.data_ptr<float>();
  a.O = (int)x.numel();
  a.A = (int)action.numel();
  int maxw = a.O;
  for (int L = 0; L < a.n_layers; ++L) {
    a.w[L] = ws[L].data_ptr<float>();
    a.b[L] = bs[L].data_ptr<float>();
    a.width[L] = (int)ws[L].size(0);
    TORCH_CHECK(a.width[L] <= 256, "act kernel: trunk width > 256");
    maxw = std::max(maxw, a.width[L]);
  }
  TORCH_CHECK(maxw <= ACT_MAXW && a.A <= 256);
  a.wmu = wmu.data_ptr<float>();
  a.bmu = bmu.data_ptr<float>();
  a.wls = wls.data_ptr<float>();
  a.bls = bls.data_ptr<float>();
  a.action = action.data_ptr<float>();
  a.ctr = ctr.data_ptr<int64_t>();
  a.seed = (uint64_t)seed;
  a.act_limit = (float)act_limit;
  a.lo = (float)lo;
  a.hi = (float)hi;
  return a;
}

// TAC_AMD_ACT_FAST: 1 (default) sends single-state act launches inside
// act_fast_kernel's gate to it, 0 keeps act_kernel for everything.  A
// plain global so act_fast_mode() can flip it inside one process.
static int g_act_fast = -1;

static bool act_fast_mode_get() {
  if (g_act_fast < 0) {
    const char* e = getenv("TAC_AMD_ACT_FAST");
    g_act_fast = e ? (atoi(e) != 0) : 1;
  }
  return g_act_fast != 0;
}

int64_t act_fast_mode(int64_t mode) {
  const int prev = act_fast_mode_get();
  TORCH_CHECK(mode == 0 || mode == 1, "act_fast_mode: 0 or 1");
  g_act_fast = (int)mode;
  return prev;
}

// Host-only gate of act_fast_kernel on shapes: obs width, trunk widths,
// action width (the limits are the kernel's register and LDS budgets).
static bool act_fast_shape_ok(int O, const int* width, int n_layers, int A) {
  if (n_layers < 1 || n_layers > ACT_MAXL) return false;
  if (O < 1 || O > 256 || A < 1 || A > 64) return false;
  for (int L = 0; L < n_layers; ++L)
    if (width[L] < 4 || width[L] > 256 || width[L] % 4 != 0) return false;
  for (int L = 1; L < n_layers; ++L)   // whole 64-column slabs, rows in 16s
    if (width[L - 1] % ACTF_KS != 0 || width[L] % 16 != 0) return false;
  const int KL = width[n_layers - 1];
  if ((KL & (KL - 1)) != 0) return false;
  if ((int64_t)width[0] * O > ACTF_L0 * 256) return false;
  if ((int64_t)A * KL > ACTF_HV * 256) return false;
  return true;
}

bool act_fast_ok(int64_t obs_dim, std::vector<int64_t> widths,
                 int64_t act_dim) {
  if (widths.empty() || widths.size() > (size_t)ACT_MAXL) return false;
  if (obs_dim < 1 || obs_dim > 256 || act_dim < 1 || act_dim > 64)
    return false;
  int w[ACT_MAXL] = {};
  for (size_t L = 0; L < widths.size(); ++L) {
    if (widths[L] < 1 || widths[L] > 256) return false;
    w[L] = (int)widths[L];
  }
  return act_fast_shape_ok((int)obs_dim, w, (int)widths.size(),
                           (int)act_dim);
}

// shape gate plus what only the pointers tell: the hidden layers are read
// as 16-byte vectors
static bool act_fast_fits(const ActArgs& a) {
  if (!act_fast_shape_ok(a.O, a.width, a.n_layers, a.A)) return false;
  for (int L = 1; L < a.n_layers; ++L)
    if (reinterpret_cast<uintptr_t>(a.w[L]) % 16 != 0) return false;
  return true;
}

static bool g_act_last_fast = false;

// every single-state act launch goes through here
static void act_launch(const ActArgs& a, const ActPinned& hp, bool fits) {
  g_act_last_fast = fits && act_fast_mode_get();
  if (g_act_last_fast)
    hipLaunchKernelGGL(act_fast_kernel, dim3(1), dim3(256), 0, stream(), a,
                       hp);
  else
    hipLaunchKernelGGL(act_kernel, dim3(1), dim3(256), 0, stream(), a, hp);
}

bool act_last_fast() { return g_act_last_fast; }

void act_step(torch::Tensor x, std::vector<torch::Tensor> ws,
              std::vector<torch::Tensor> bs, torch::Tensor wmu,
              torch::Tensor bmu, torch::Tensor wls, torch::Tensor bls,
              torch::Tensor action, torch::Tensor ctr, int64_t seed,
              double act_limit, double lo, double hi) {
  const ActArgs a = act_args(x, ws, bs, wmu, bmu, wls, bls, action, ctr,
                             seed, act_limit, lo, hi);
  act_launch(a, ActPinned{nullptr, nullptr}, act_fast_fits(a));
}

// act_step writing the action AND a completion flag to host-pinned
// memory (host spins on the flag; no D2H copy / event sync per step)
void act_step_pinned(torch::Tensor x, std::vector<torch::Tensor> ws,
                     std::vector<torch::Tensor> bs, torch::Tensor wmu,
                     torch::Tensor bmu, torch::Tensor wls,
                     torch::Tensor bls, torch::Tensor action,
                     torch::Tensor out_host, torch::Tensor flag_host,
                     torch::Tensor ctr, int64_t seed, double act_limit,
                     double lo, double hi) {
  TORCH_CHECK(out_host.is_pinned() && flag_host.is_pinned(),
              "host buffers must be pinned");
  const ActArgs a = act_args(x, ws, bs, wmu, bmu, wls, bls, action, ctr,
                             seed, act_limit, lo, hi);
  act_launch(a, ActPinned{out_host.data_ptr<float>(),
                          flag_host.data_ptr<int>()}, act_fast_fits(a));
}

void bump3(torch::Tensor a, c10::optional<torch::Tensor> b,
           c10::optional<torch::Tensor> c) {
  hipLaunchKernelGGL(bump3_kernel, dim3(1), dim3(1), 0, stream(),
                     a.data_ptr<int64_t>(),
                     b.has_value() ? b->data_ptr<int64_t>() : nullptr,
                     c.has_value() ? c->data_ptr<int64_t>() : nullptr);
}

// Pre-marshalled acting: the ActArgs are built once (act_prepare) and
// fired with a single-int pybind call per env step (act_fire) — the
// 13-argument marshalling otherwise costs microseconds per step.
struct ActHandle {
  ActArgs a;
  ActPinned hp;
  bool fits;       // act_fast_fits(a), decided once: the pointers are fixed
  bool x_pinned;   // act_sync writes the observation through a.x
};
static std::vector<ActHandle> g_act_handles;

int64_t act_prepare(torch::Tensor x, std::vector<torch::Tensor> ws,
                    std::vector<torch::Tensor> bs, torch::Tensor wmu,
                    torch::Tensor bmu, torch::Tensor wls, torch::Tensor bls,
                    torch::Tensor action, torch::Tensor out_host,
                    torch::Tensor flag_host, torch::Tensor ctr,
                    int64_t seed, double act_limit, double lo, double hi) {
  TORCH_CHECK(out_host.is_pinned() && flag_host.is_pinned());
  TORCH_CHECK(out_host.numel() == action.numel() && flag_host.numel() >= 1);
  const ActArgs a = act_args(x, ws, bs, wmu, bmu, wls, bls, action, ctr,
                             seed, act_limit, lo, hi);
  g_act_handles.push_back({a, ActPinned{out_host.data_ptr<float>(),
                                        flag_host.data_ptr<int>()},
                           act_fast_fits(a), x.is_pinned()});
  return (int64_t)g_act_handles.size() - 1;
}

void act_fire(int64_t handle) {
  auto& h = g_act_handles.at((size_t)handle);
  act_launch(h.a, h.hp, h.fits);
}

bool act_handle_fast(int64_t handle) {
  return g_act_handles.at((size_t)handle).fits && act_fast_mode_get();
}

// One native call per env step: observation in, launch, spin on the
// completion flag, action out (act_sync.h).  False means the flag did not
// land within actsync::kTimeoutS; nothing further has been launched and
// the caller decides how to drain the stream.
bool act_sync(int64_t handle, py::array obs, py::array out) {
  auto& h = g_act_handles.at((size_t)handle);
  TORCH_CHECK(h.x_pinned, "act_sync: the handle's observation buffer is "
              "not pinned host memory");
  auto f32vec = [](const py::array& v, int n) {
    return py::isinstance<py::array_t<float>>(v) && v.ndim() == 1
        && v.shape(0) == n && v.strides(0) == (py::ssize_t)sizeof(float);
  };
  TORCH_CHECK(f32vec(obs, h.a.O), "act_sync: obs must be a contiguous "
              "float32 array of length ", h.a.O);
  TORCH_CHECK(f32vec(out, h.a.A) && out.writeable(), "act_sync: out must "
              "be a writeable contiguous float32 array of length ", h.a.A);
  return actsync::run(const_cast<float*>(h.a.x),
                       static_cast<const float*>(obs.data()), h.a.O,
                       h.hp.out_host,
                       static_cast<float*>(out.mutable_data()), h.a.A,
                       h.hp.flag_host, actsync::kTimeoutS,
                       [&] { act_launch(h.a, h.hp, h.fits); });
}

// Batched acting (evaluation path): rows [0, n) of x[*, O] (row stride
// x.stride(0)) -> rows [0, n) of action[*, A].  The Philox counter comes
// from the host by value; deterministic launches ignore it.
void act_batch(torch::Tensor x, std::vector<torch::Tensor> ws,
               std::vector<torch::Tensor> bs, torch::Tensor wmu,
               torch::Tensor bmu, torch::Tensor wls, torch::Tensor bls,
               torch::Tensor action, int64_t n, bool deterministic,
               int64_t ctr_val, int64_t seed, double act_limit, double lo,
               double hi) {
  auto f32dev = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == torch::kFloat32
        && t.device() == x.device();
  };
  ActArgs a{};
  a.n_layers = (int)ws.size();
  TORCH_CHECK(a.n_layers >= 1 && a.n_layers <= ACT_MAXL
              && bs.size() == ws.size(), "act_batch: trunk depth");
  TORCH_CHECK(f32dev(x) && x.dim() == 2 && x.stride(1) == 1
              && x.stride(0) >= x.size(1), "act_batch: x must be [N, O] fp32 "
              "device rows");
  TORCH_CHECK(f32dev(action) && action.dim() == 2 && action.is_contiguous(),
              "act_batch: action must be contiguous [N, A] fp32");
  TORCH_CHECK(n >= 1 && n <= x.size(0) && n <= action.size(0),
              "act_batch: n outside the x/action buffers");
  a.x = x.data_ptr<float>();
  a.O = (int)x.size(1);
  a.A = (int)action.size(1);
  TORCH_CHECK(a.O >= 1 && a.O <= ACT_MAXW, "act_batch: obs width > ",
              ACT_MAXW);
  TORCH_CHECK(a.A >= 1 && a.A <= 64, "act_batch: act_dim > 64");
  int K = a.O;
  for (int L = 0; L < a.n_layers; ++L) {
    TORCH_CHECK(f32dev(ws[L]) && ws[L].is_contiguous() && ws[L].dim() == 2
                && ws[L].size(1) == K, "act_batch: trunk weight ", L);
    a.width[L] = (int)ws[L].size(0);
    TORCH_CHECK(a.width[L] >= 1 && a.width[L] <= 256,
                "act_batch: trunk width > 256");
    TORCH_CHECK(f32dev(bs[L]) && bs[L].is_contiguous()
                && bs[L].numel() == a.width[L], "act_batch: trunk bias ", L);
    a.w[L] = ws[L].data_ptr<float>();
    a.b[L] = bs[L].data_ptr<float>();
    K = a.width[L];
  }
  for (const torch::Tensor* w : {&wmu, &wls})
    TORCH_CHECK(f32dev(*w) && w->is_contiguous() && w->dim() == 2
                && w->size(0) == a.A && w->size(1) == K,
                "act_batch: head weight");
  for (const torch::Tensor* b : {&bmu, &bls})
    TORCH_CHECK(f32dev(*b) && b->is_contiguous() && b->numel() == a.A,
                "act_batch: head bias");
  a.wmu = wmu.data_ptr<float>();
  a.bmu = bmu.data_ptr<float>();
  a.wls = wls.data_ptr<float>();
  a.bls = bls.data_ptr<float>();
  a.action = action.data_ptr<float>();
  a.ctr = nullptr;             // the counter is a launch argument
  a.seed = (uint64_t)seed;
  a.act_limit = (float)act_limit;
  a.lo = (float)lo;
  a.hi = (float)hi;
  const int grid = (int)((n + ACTB_R - 1) / ACTB_R);
  hipLaunchKernelGGL(act_batch_kernel, dim3(grid), dim3(256), 0, stream(),
                     a, (int)n, (int)x.stride(0), deterministic ? 1 : 0,
                     (unsigned long long)ctr_val);
}

torch::Tensor philox_words2(int64_t seed, int64_t chi, int64_t clo0,
                            int64_t n) {
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 20),
              "philox_words2: n outside 1..2^20");
  auto out = torch::empty({n, 4}, torch::dtype(torch::kInt64)
                                      .device(torch::kCUDA));
  hipLaunchKernelGGL(philox_words2_kernel, dim3((int)((n + 255) / 256)),
                     dim3(256), 0, stream(), out.data_ptr<int64_t>(),
                     (uint64_t)seed, (uint64_t)chi, (uint64_t)clo0, n);
  return out;
}

void alpha_update(torch::Tensor log_alpha, torch::Tensor alpha_dev,
                  torch::Tensor m, torch::Tensor v, torch::Tensor step,
                  torch::Tensor mean_logp, double target_entropy, double lr) {
  need_scalar_f32(log_alpha, "alpha_update", "log_alpha");
  need_scalar_f32(alpha_dev, "alpha_update", "alpha_dev");
  need_scalar_f32(m, "alpha_update", "m");
  need_scalar_f32(v, "alpha_update", "v");
  need_scalar_i64(step, "alpha_update", "step");
  need_scalar_f32(mean_logp, "alpha_update", "mean_logp");
  hipLaunchKernelGGL(alpha_update_kernel, dim3(1), dim3(1), 0, stream(),
                     log_alpha.data_ptr<float>(), alpha_dev.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     step.data_ptr<int64_t>(), mean_logp.data_ptr<float>(),
                     (float)target_entropy, (float)lr);
}

}  // namespace fused

void register_fused(pybind11::module_& m) {
  m.def("mgemm", &fused::mgemm,
        "multi-problem MFMA GEMM (fwd-form, strided, masked, sum2)");
  m.def("mgemm_r1", &fused::mgemm_r1,
        "masked GEMM whose A operand is a rank-1 product formed on read");
  m.def("mgemm_r1_qloss", &fused::mgemm_r1_qloss,
        "qloss2 + K=1 dgrad + masked dgrad in one small-shape launch");
  m.def("mgemm_r1_piloss", &fused::mgemm_r1_piloss,
        "piloss2 + mgemm_r1 in one small-shape launch");
  m.def("mgemm_r1_fold_ok", &fused::mgemm_r1_fold_ok,
        "host-only: do (M, K) pass the gate of the two folded entries");
  m.def("mgemm_small_mode", &fused::mgemm_small_mode,
        "set TAC_AMD_MGEMM_SMALL's mode (0 = pipelined kernel only), "
        "returns the previous mode");
  m.def("mwgrad", &fused::mwgrad, "multi-problem wgrad + fused db");
  m.def("mwgrad_het", &fused::mwgrad_het,
        "heterogeneous multi-problem wgrad: one launch per phase");
  m.def("mwgrad_het_adam", &fused::mwgrad_het_adam,
        "heterogeneous wgrad with Adam (+polyak, +W^T) in the epilogue");
  m.def("mwgrad_het_adam_split", &fused::mwgrad_het_adam_split,
        "host-only: M slabs mwgrad_het_adam would use for these shapes");
  m.def("ranges_tile_exactly", &fused::ranges_tile_exactly,
        "host-only: do [off, off+len) ranges tile [0, n) exactly once");
  m.def("transpose_multi", &fused::transpose_multi,
        pybind11::arg("ws"), pybind11::arg("wts"),
        pybind11::arg("blocks") = std::vector<int64_t>{});
  namespace py = pybind11;
  // trailing ctr_add: the Philox key is ctr[0] + ctr_add, so a reader can
  // run ahead of the launch that commits the bump (see qloss2's bump*)
  m.def("gather2", &fused::gather2, py::arg("state"), py::arg("act"),
        py::arg("rew"), py::arg("nstate"), py::arg("done"),
        py::arg("size_dev"), py::arg("ctr"), py::arg("seed"), py::arg("xc"),
        py::arg("xc2"), py::arg("orew"), py::arg("od"), py::arg("B"),
        py::arg("ctr_add") = 0);
  m.def("gather2n", &fused::gather2n, py::arg("state"), py::arg("act"),
        py::arg("rew"), py::arg("nstate"), py::arg("done"),
        py::arg("ep_end"), py::arg("size_dev"), py::arg("ptr_dev"),
        py::arg("ctr"), py::arg("seed"), py::arg("n"), py::arg("gamma"),
        py::arg("xc"), py::arg("xc2"), py::arg("orew"), py::arg("od"),
        py::arg("B"), py::arg("ctr_add") = 0);
  m.def("gather2p", &fused::gather2p, py::arg("state"), py::arg("act"),
        py::arg("rew"), py::arg("nstate"), py::arg("done"),
        py::arg("ep_end"), py::arg("size_dev"), py::arg("ptr_dev"),
        py::arg("tree"), py::arg("ctr"), py::arg("seed"), py::arg("n"),
        py::arg("gamma"), py::arg("xc"), py::arg("xc2"), py::arg("orew"),
        py::arg("od"), py::arg("idx_out"), py::arg("prob_out"),
        py::arg("u_out"), py::arg("B"), py::arg("ctr_add") = 0);
  m.def("per_update", &fused::per_update,
        "sum tree: leaves[idx] = (td + eps)^alpha, ancestors recomputed");
  m.def("per_set_range", &fused::per_set_range,
        "sum tree: a ring range gets max_priority, ancestors recomputed");
  m.def("tg_fwd2", &fused::tg_fwd2, py::arg("hl"), py::arg("out0"),
        py::arg("col0"), py::arg("out1"), py::arg("col1"), py::arg("B0"),
        py::arg("logp"), py::arg("prob"), py::arg("ctr"), py::arg("seed"),
        py::arg("act_limit"), py::arg("lo"), py::arg("hi"),
        py::arg("ctr_add") = 0);
  m.def("tg_bwd2", &fused::tg_bwd2);
  m.def("qloss2", &fused::qloss2, py::arg("q1"), py::arg("q2"),
        py::arg("q1t"), py::arg("q2t"), py::arg("logp_next"),
        py::arg("rew"), py::arg("done"), py::arg("alpha_dev"),
        py::arg("alpha_host"), py::arg("loss_acc"), py::arg("dq1"),
        py::arg("dq2"), py::arg("B"), py::arg("gamma"), py::arg("scale"),
        py::arg("wt3_0"), py::arg("wt3_1"), py::arg("dy2_0"),
        py::arg("dy2_1"), py::arg("h2"), py::arg("bump0") = py::none(),
        py::arg("bump1") = py::none(), py::arg("bump2") = py::none(),
        py::arg("prob") = py::none(), py::arg("size_dev") = py::none(),
        py::arg("beta_dev") = py::none(), py::arg("td") = py::none());
  m.def("piloss2", &fused::piloss2);
  m.def("alpha_update", &fused::alpha_update);
  m.def("tg_eps", &fused::tg_eps);
  m.def("philox_words2", &fused::philox_words2,
        "test helper: raw Philox words of this translation unit's copy");
  m.def("adam_t", &fused::adam_t,
        pybind11::arg("p"), pybind11::arg("g"), pybind11::arg("m"),
        pybind11::arg("v"), pybind11::arg("step"), pybind11::arg("lr"),
        pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"),
        pybind11::arg("wd"), pybind11::arg("offsets"),
        pybind11::arg("wts"), pybind11::arg("targ"),
        pybind11::arg("rho"),
        pybind11::arg("bss") = std::vector<int64_t>{});
  m.def("act_step", &fused::act_step);
  m.def("bump3", &fused::bump3);
  m.def("act_step_pinned", &fused::act_step_pinned);
  m.def("act_prepare", &fused::act_prepare);
  m.def("act_fire", &fused::act_fire);
  m.def("act_sync", &fused::act_sync,
        "act_fire + host spin in one call: (handle, obs, out) -> landed");
  m.def("act_fast_ok", &fused::act_fast_ok,
        "host-only: do (obs_dim, trunk widths, act_dim) pass the shape "
        "gate of the latency-shaped act kernel");
  m.def("act_fast_mode", &fused::act_fast_mode,
        "set TAC_AMD_ACT_FAST's mode (0 = act_kernel only), returns the "
        "previous mode");
  m.def("act_handle_fast", &fused::act_handle_fast,
        "host-only: would act_fire(handle) launch the latency-shaped form");
  m.def("act_last_fast", &fused::act_last_fast,
        "host-only: did the last single-state act launch use it");
  m.def("act_batch", &fused::act_batch,
        "batched actor forward (deterministic or Philox-stochastic)");
}
