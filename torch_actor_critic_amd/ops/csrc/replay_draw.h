// The replay ring's sampling policy, shared by tac_kernels.hip (flat batch
// tensors) and fused.hip (concat-layout batch buffers): Philox4x32-10, the
// uniform and sum-tree slot draws, the n-step window walk, the one row
// gather kernel both files instantiate, its launch shape and its host gate.
#pragma once

#include <hip/hip_runtime.h>

#include <torch/extension.h>

#include <algorithm>
#include <type_traits>

#define DEVINL __device__ __forceinline__

namespace replay {

// ---------------------------------------------------------------------------
// Philox4x32-10 counter-based RNG (device-side, graph-replay-safe)
// ---------------------------------------------------------------------------

struct Philox4 {
  uint32_t x, y, z, w;
};

DEVINL uint32_t mulhilo(uint32_t a, uint32_t b, uint32_t* hi) {
  uint64_t p = (uint64_t)a * (uint64_t)b;
  *hi = (uint32_t)(p >> 32);
  return (uint32_t)p;
}

DEVINL Philox4 philox4(uint64_t seed, uint64_t ctr_hi, uint64_t ctr_lo) {
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32);
  uint32_t c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, hi1;
    uint32_t lo0 = mulhilo(M0, c0, &hi0);
    uint32_t lo1 = mulhilo(M1, c2, &hi1);
    uint32_t n0 = hi1 ^ c1 ^ k0;
    uint32_t n1 = lo1;
    uint32_t n2 = hi0 ^ c3 ^ k1;
    uint32_t n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  return {c0, c1, c2, c3};
}

// Debug/test helper: the four raw output words of subsequence clo, so the
// generator each translation unit compiled can be held against a host
// implementation (tests/kernel_refs.py::philox4x32).
DEVINL void philox_words_row(int64_t* __restrict__ out, uint64_t seed,
                             uint64_t chi, uint64_t clo0, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Philox4 r = philox4(seed, chi, clo0 + (uint64_t)i);
  out[4 * i + 0] = (int64_t)r.x;
  out[4 * i + 1] = (int64_t)r.y;
  out[4 * i + 2] = (int64_t)r.z;
  out[4 * i + 3] = (int64_t)r.w;
}

// One standard normal from two Philox words: Box-Muller's cosine branch on
// the uniforms (w + 1) * 2^-32 in (0, 1].
DEVINL float philox_normal(uint32_t w0, uint32_t w1) {
  float u0 = (w0 + 1.f) * 2.3283064365386963e-10f;
  float u1 = (w1 + 1.f) * 2.3283064365386963e-10f;
  return sqrtf(-2.f * logf(u0)) * __cosf(6.283185307179586f * u1);
}

// Uniform slot of a ring holding `size` transitions: a 64-bit uniform keeps
// the modulo bias negligible at 1e6 sizes; an empty ring draws slot 0.
DEVINL int64_t uniform_slot(const Philox4& r, uint64_t size) {
  uint64_t u = ((uint64_t)r.x << 32) | r.y;
  return (int64_t)(u % (size ? size : 1));
}

// ---------------------------------------------------------------------------
// N-step window (buffer/replay.py::sample_at is the executable definition
// of the window semantics)
// ---------------------------------------------------------------------------

// The slot written last, which closes every window.  With size == 0 slot 0
// counts as the newest, so nothing beyond it is consumed.
DEVINL int64_t newest_slot(uint64_t size, const int64_t* __restrict__ ptr_dev,
                           int64_t cap) {
  return size ? (ptr_dev[0] + cap - 1) % cap : 0;
}

// N-step window walk for one sampled slot, run by ONE full wave (all 64
// lanes active, n <= 64).  Lane m < n loads (rew, done, episode_end) of
// slot (idx+m) % cap and forms its own gamma^m by repeated multiply; a
// wave64 ballot finds the first lane whose slot closes the window
// (terminal, episode boundary, newest slot, or m == n-1), so the n slots
// cost one global-load latency instead of a chain of n dependent loads.
// R = sum_{m<M} gamma^m rew[m] is added in ascending m (the reference
// order), deff = 1 - gamma^(M-1) * (1 - done[last]); contraction is off so
// every product is rounded before it is added, as in the reference.  The
// loss kernels need no change for it: gamma * (1 - deff) ==
// gamma^M * (1 - done[last]).
// Returns the last slot of the window; all lanes get the same values.
DEVINL int64_t nstep_walk(const float* __restrict__ rew,
                          const float* __restrict__ done,
                          const float* __restrict__ ep_end, int64_t idx,
                          int64_t cap, int64_t newest, int n, float gamma,
                          float* R, float* deff) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t slot = (idx + lane) % cap;
  float r = 0.f, d = 0.f;
  bool stop = lane >= n - 1;
  if (lane < n) {
    r = rew[slot];
    d = done[slot];
    stop = stop || d != 0.f || ep_end[slot] != 0.f || slot == newest;
  }
  float disc = 1.f;
  for (int m = 0; m < n - 1; ++m)
    if (m < lane) disc *= gamma;
  // lane n-1 always votes, so the mask is never empty
  const unsigned long long mask = __ballot(stop);
  const int last = __ffsll((long long)mask) - 1;
  const float term = disc * r;
  float acc = 0.f;
  for (int m = 0; m <= last; ++m) acc += __shfl(term, m);
  *R = acc;
  const float de = 1.f - disc * (1.f - d);
  *deff = __shfl(de, last);
  return (idx + last) % cap;
}

// ---------------------------------------------------------------------------
// Prioritized replay: fan-out-64 sum tree (buffer/replay.py::per_layout is
// the layout, ::draw the executable definition of the draw)
// ---------------------------------------------------------------------------

constexpr int PER_MAXL = 8;

// Level k (0 = root, L = leaves) holds n[k] nodes at tree + off[k], padded
// with zeros to a multiple of 64 so a wave always loads 64 in-bounds children.
struct PerLay {
  int L;
  int64_t off[PER_MAXL];
  int64_t n[PER_MAXL];
};

// The layout of the sum tree over a ring of `cap` slots, checked against
// the flat tensor every per_* launch indexes with it.
inline PerLay per_tree_layout(const torch::Tensor& tree, int64_t cap,
                              const char* who) {
  PerLay lay;
  int L = 1;
  for (int64_t span = 64; span < cap; span *= 64) ++L;
  TORCH_CHECK(cap >= 1 && L < PER_MAXL, who,
              ": per: unsupported ring capacity");
  lay.L = L;
  lay.n[L] = cap;
  for (int k = L - 1; k >= 0; --k) lay.n[k] = (lay.n[k + 1] + 63) / 64;
  int64_t total = 0;
  for (int k = 0; k <= L; ++k) {
    lay.off[k] = total;
    total += (lay.n[k] + 63) / 64 * 64;
  }
  for (int k = L + 1; k < PER_MAXL; ++k) lay.off[k] = lay.n[k] = 0;
  TORCH_CHECK(tree.is_cuda() && tree.is_contiguous() &&
              tree.dtype() == torch::kFloat32 && tree.numel() == total,
              who, ": per: tree must be a contiguous fp32 device tensor of ",
              total, " elements for a ring of ", cap);
  return lay;
}

// Sum-tree descent for one target u, run by ONE full wave.  Per level,
// lane l loads child l of the current node (one coalesced 256-byte load —
// the fan-out is the wave width), a Hillis-Steele __shfl_up scan forms the
// inclusive prefix P and a ballot picks the first lane with P > u and
// c > 0.  The c > 0 guard is required: the scan is not monotone in
// floating point, so without it a zero child could win.  If u rounded past
// the end the last lane with c > 0 is taken, lane 0 in an empty tree.  The
// remainder u - (P[pick] - c[pick]), clamped at 0, goes down one level:
// L dependent loads per sample.  prob = leaf / root (1 for an empty tree).
// All lanes return the same values.
DEVINL int64_t per_descend(const float* __restrict__ tree, const PerLay& lay,
                           float u, float* prob) {
  const int lane = threadIdx.x & 63;
  int64_t node = 0;
  float leaf = 0.f;
  for (int k = 1; k <= lay.L; ++k) {
    const float c = tree[lay.off[k] + node * 64 + lane];
    float P = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float t = __shfl_up(P, off);
      if (lane >= off) P += t;
    }
    const bool pos = c > 0.f;
    const unsigned long long hit = __ballot(pos && P > u);
    const unsigned long long any = __ballot(pos);
    const int pick = hit ? __ffsll((long long)hit) - 1
                         : (any ? 63 - __clzll((long long)any) : 0);
    const float Pp = __shfl(P, pick), cp = __shfl(c, pick);
    u = fmaxf(u - (Pp - cp), 0.f);
    node = node * 64 + pick;
    leaf = cp;
  }
  const float root = tree[lay.off[0]];
  *prob = root == 0.f ? 1.f : leaf / root;
  return node;
}

// Stratified target of batch position j: u = (j + u01) * (root / B) with
// u01 = (r.x >> 8) * 2^-24 from the Philox draw the uniform gather makes.
DEVINL float per_target(const float* __restrict__ tree, const PerLay& lay,
                        uint32_t rx, int j, int B) {
#pragma clang fp contract(off)
  const float u01 = (float)(rx >> 8) * 5.9604644775390625e-8f;
  const float seg = tree[lay.off[0]] / (float)B;
  return ((float)j + u01) * seg;
}

// ---------------------------------------------------------------------------
// Replay sample + gather (Philox, with replacement)
// ---------------------------------------------------------------------------

// Where a gathered row goes.  Each sink is instantiated from one
// translation unit only (FlatSink from tac_kernels.hip, ConcatSink from
// fused.hip): every file carries its own code object, and a __global__ with
// one mangled name must not be registered from both.

// Separate batch tensors os [B, obs], oa [B, act], ons [B, obs].  A null os
// gathers nothing: the draw alone (the per_sample binding).
struct FlatSink {
  float *os, *oa, *ons;
  int obs_dim, act_dim;
  DEVINL bool gathers() const { return os != nullptr; }
  DEVINL void state(int j, int c, float v) const {
    os[(int64_t)j * obs_dim + c] = v;
  }
  DEVINL void action(int j, int c, float v) const {
    oa[(int64_t)j * act_dim + c] = v;
  }
  DEVINL void next_state(int j, int c, float v) const {
    ons[(int64_t)j * obs_dim + c] = v;
  }
};

// The update engine's concat layout, leading dimension ldc: XC [2B, ldc]
// holds (s | a) in rows :B and ns in rows B:, XC2 [B, ldc] a second s.
struct ConcatSink {
  float *xc, *xc2;
  int B, ldc, obs_dim;
  DEVINL constexpr bool gathers() const { return true; }
  DEVINL void state(int j, int c, float v) const {
    xc[(int64_t)j * ldc + c] = v;
    xc2[(int64_t)j * ldc + c] = v;
  }
  DEVINL void action(int j, int c, float v) const {
    xc[(int64_t)j * ldc + obs_dim + c] = v;
  }
  DEVINL void next_state(int j, int c, float v) const {
    xc[(int64_t)(B + j) * ldc + c] = v;
  }
};

enum class Draw {
  Uniform,   // idx_j = philox(seed, ctr, j) % size, 1-step fields
  UniformN,  // the same slot; rew/done/next_state of its n-step window
  Tree,      // stratified draw from the sum tree, either n
};

// grid.x = B (one block per sampled row), Philox key (seed, ctr[0] +
// ctr_add, j) in every mode, so for one counter value Uniform and UniformN
// pick the same slots; all threads of a block copy the row's fields.
//   Uniform:  every thread derives the slot itself: no LDS, no barrier.
//   UniformN: wave 0 walks the window while the other waves already copy
//             state and action; one barrier, then next_state of the
//             window's last slot.  orew / od carry the discounted reward
//             sum and the effective done.
//   Tree:     wave 0 draws, descends and (n > 1) walks, and hands slot and
//             last slot to the block through LDS before any copy.  Also
//             writes the drawn slot, its probability leaf / root and (tests
//             only, when u_out is given) the target.  n == 1 reads neither
//             ep_end nor ptr_dev; a sink that gathers nothing reads no ring
//             field at all and returns before the barrier.
//
// The operands every mode reads come first and the tree draw's own go last,
// in a struct that is empty for the uniform draws: the 1-step launch the
// update makes on every step keeps a kernarg segment of two cache lines.
struct TreeArgs {
  const float* tree;
  PerLay lay;
  int64_t* idx_out;
  float *prob_out, *u_out;
};
struct NoTree {};
template <Draw D>
using TreeOf = std::conditional_t<D == Draw::Tree, TreeArgs, NoTree>;

template <Draw D, class Sink>
__global__ __launch_bounds__(256)
void gather_kernel(const float* __restrict__ state,
                   const float* __restrict__ act,
                   const float* __restrict__ rew,
                   const float* __restrict__ nstate,
                   const float* __restrict__ done,
                   const int64_t* __restrict__ size_dev,
                   const int64_t* __restrict__ ctr, int64_t ctr_add,
                   uint64_t seed, Sink sink,
                   float* __restrict__ orew, float* __restrict__ od,
                   int B, int obs_dim, int act_dim,
                   const float* __restrict__ ep_end,
                   const int64_t* __restrict__ ptr_dev,
                   int64_t cap, int n, float gamma, TreeOf<D> t) {
  const int j = blockIdx.x;
  const uint64_t chi = (uint64_t)(ctr[0] + ctr_add);
  int64_t idx, last;
  if constexpr (D == Draw::Tree) {
    const float* tree = t.tree;
    const PerLay& lay = t.lay;
    int64_t* idx_out = t.idx_out;
    float *prob_out = t.prob_out, *u_out = t.u_out;
    __shared__ int64_t s_idx, s_last;
    const bool gather = sink.gathers();
    if (threadIdx.x < 64) {
      Philox4 r = philox4(seed, chi, (uint64_t)j);
      const float u = per_target(tree, lay, r.x, j, B);
      float prob;
      idx = per_descend(tree, lay, u, &prob);
      // a consistent tree never leads past the ring; keep the copies in
      // bounds whatever the tree holds
      idx = idx < cap ? idx : cap - 1;
      last = idx;
      if (gather) {
        float R, de;
        if (n > 1) {
          const int64_t newest = newest_slot(size_dev[0], ptr_dev, cap);
          last = nstep_walk(rew, done, ep_end, idx, cap, newest, n, gamma, &R,
                            &de);
        } else {
          R = rew[idx];
          de = done[idx];
        }
        if (threadIdx.x == 0) {
          orew[j] = R;
          od[j] = de;
        }
      }
      if (threadIdx.x == 0) {
        s_idx = idx;
        s_last = last;
        idx_out[j] = idx;
        prob_out[j] = prob;
        if (u_out) u_out[j] = u;
      }
    }
    if (!gather) return;
    __syncthreads();
    idx = s_idx;
    last = s_last;
  } else {
    const uint64_t size = (uint64_t)size_dev[0];
    idx = uniform_slot(philox4(seed, chi, (uint64_t)j), size);
    last = idx;
    if constexpr (D == Draw::UniformN) {
      __shared__ int64_t s_last;
      if (threadIdx.x < 64) {
        const int64_t newest = newest_slot(size, ptr_dev, cap);
        float R, de;
        last = nstep_walk(rew, done, ep_end, idx, cap, newest, n, gamma, &R,
                          &de);
        if (threadIdx.x == 0) {
          s_last = last;
          orew[j] = R;
          od[j] = de;
        }
      }
      const float* srow = state + idx * obs_dim;
      for (int c = threadIdx.x; c < obs_dim; c += blockDim.x)
        sink.state(j, c, srow[c]);
      const float* arow = act + idx * act_dim;
      for (int c = threadIdx.x; c < act_dim; c += blockDim.x)
        sink.action(j, c, arow[c]);
      __syncthreads();
      const float* nrow = nstate + s_last * obs_dim;
      for (int c = threadIdx.x; c < obs_dim; c += blockDim.x)
        sink.next_state(j, c, nrow[c]);
      return;
    }
  }
  const float* srow = state + idx * obs_dim;
  const float* nrow = nstate + last * obs_dim;
  for (int c = threadIdx.x; c < obs_dim; c += blockDim.x) {
    sink.state(j, c, srow[c]);
    sink.next_state(j, c, nrow[c]);
  }
  const float* arow = act + idx * act_dim;
  for (int c = threadIdx.x; c < act_dim; c += blockDim.x)
    sink.action(j, c, arow[c]);
  if constexpr (D == Draw::Uniform) {
    if (threadIdx.x == 0) {
      orew[j] = rew[idx];
      od[j] = done[idx];
    }
  }
}

// Block size of every gather launch: the row width rounded up to whole
// waves, between one and four of them.
inline int gather_threads(int obs_dim) {
  return std::min(256, std::max(64, (obs_dim + 63) / 64 * 64));
}

// ---------------------------------------------------------------------------
// Host gate of the gather bindings: every operand is checked before
// anything is launched, so a refused call touches nothing.
// ---------------------------------------------------------------------------

// The ring side of a gather call.  ep_end / ptr_dev are null in the 1-step
// uniform bindings, which have neither.
struct RingArgs {
  const torch::Tensor &state, &act, &rew, &nstate, &done;
  const torch::Tensor* ep_end;
  const torch::Tensor& size_dev;
  const torch::Tensor* ptr_dev;
  const torch::Tensor& ctr;
};

// The batch side.  Flat: rows = os, aux = oa, ons given, and every output
// is exactly B long.  Concat: rows = xc, aux = xc2, ons null, and the
// outputs need only be long enough.  idx / prob / u are the tree draw's
// outputs, null where the binding has none.
struct BatchArgs {
  const torch::Tensor &rows, &aux;
  const torch::Tensor* ons;
  const torch::Tensor &orew, &od;
  const torch::Tensor *idx, *prob, *u;
};

inline bool is_dev(const torch::Tensor& t, torch::ScalarType st) {
  return t.defined() && t.is_cuda() && t.is_contiguous() &&
         t.scalar_type() == st;
}

inline void gather_gate(const char* who, const RingArgs& r, int64_t n,
                        int64_t B, const BatchArgs& o) {
  for (const torch::Tensor* t : {&r.state, &r.act, &r.rew, &r.nstate,
                                 &r.done, r.ep_end, &o.rows, &o.aux, o.ons,
                                 &o.orew, &o.od, o.prob, o.u})
    TORCH_CHECK(!t || is_dev(*t, torch::kFloat32), who,
                ": tensors must be contiguous fp32 device tensors");
  TORCH_CHECK(r.state.dim() == 2 && r.act.dim() == 2 &&
              r.nstate.dim() == 2 && o.rows.dim() == 2 && o.aux.dim() == 2 &&
              (!o.ons || o.ons->dim() == 2), who,
              ": state, action and batch row tensors must be 2-D");
  const int64_t cap = r.state.size(0);
  const int64_t obs_dim = r.state.size(1), act_dim = r.act.size(1);
  TORCH_CHECK(cap >= 1 && r.rew.numel() == cap && r.done.numel() == cap &&
              (!r.ep_end || r.ep_end->numel() == cap) &&
              r.nstate.size(0) == cap && r.nstate.size(1) == obs_dim &&
              r.act.size(0) == cap, who,
              ": ring fields must share one capacity");
  for (const torch::Tensor* t : {&r.size_dev, r.ptr_dev, &r.ctr})
    TORCH_CHECK(!t || (is_dev(*t, torch::kInt64) && t->numel() == 1), who,
                ": size_dev / ptr_dev / ctr must be int64 [1] device tensors");
  TORCH_CHECK(n >= 1 && n <= 64, who, ": n_step must be in 1..64");
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31), who, ": bad batch size");
  const bool concat = o.ons == nullptr;
  const auto holds = [&](int64_t len) { return concat ? len >= B : len == B; };
  TORCH_CHECK(holds(o.orew.numel()) && holds(o.od.numel()) &&
              (!o.prob || holds(o.prob->numel())) &&
              (!o.u || holds(o.u->numel())) &&
              (!o.idx || (is_dev(*o.idx, torch::kInt64) &&
                          holds(o.idx->numel()))), who,
              ": per-row batch outputs do not hold the batch");
  if (concat) {
    TORCH_CHECK(o.rows.size(0) >= 2 * B && o.aux.size(0) >= B &&
                o.rows.size(1) >= obs_dim + act_dim &&
                o.aux.size(1) == o.rows.size(1), who,
                ": batch buffers too small");
  } else {
    TORCH_CHECK(o.rows.size(0) == B && o.rows.size(1) == obs_dim &&
                o.ons->size(0) == B && o.ons->size(1) == obs_dim &&
                o.aux.size(0) == B && o.aux.size(1) == act_dim, who,
                ": batch shape mismatch");
  }
}

// Launches gather_kernel<D, Sink> for operands gather_gate has passed: B
// blocks on `stream`, keyed on ctr[0] + ctr_add.  `tree` and `lay` are used
// by Draw::Tree alone.
template <Draw D, class Sink>
inline void launch_gather(hipStream_t stream, const RingArgs& r,
                          const torch::Tensor* tree, const PerLay& lay,
                          int64_t ctr_add, int64_t seed, int64_t n,
                          double gamma, const Sink& sink, const BatchArgs& o,
                          int64_t B) {
  const auto f32 = [](const torch::Tensor* t) {
    return t ? t->data_ptr<float>() : nullptr;
  };
  const auto i64 = [](const torch::Tensor* t) {
    return t ? t->data_ptr<int64_t>() : nullptr;
  };
  const int obs_dim = (int)r.state.size(1);
  TreeOf<D> t{};
  if constexpr (D == Draw::Tree)
    t = {f32(tree), lay, i64(o.idx), f32(o.prob), f32(o.u)};
  hipLaunchKernelGGL((gather_kernel<D, Sink>), dim3((int)B),
                     dim3(gather_threads(obs_dim)), 0, stream,
                     f32(&r.state), f32(&r.act), f32(&r.rew), f32(&r.nstate),
                     f32(&r.done), i64(&r.size_dev), i64(&r.ctr), ctr_add,
                     (uint64_t)seed, sink, f32(&o.orew), f32(&o.od), (int)B,
                     obs_dim, (int)r.act.size(1), f32(r.ep_end),
                     i64(r.ptr_dev), r.state.size(0), (int)n, (float)gamma,
                     t);
}

}  // namespace replay
