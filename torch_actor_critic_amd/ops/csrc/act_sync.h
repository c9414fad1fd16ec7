// Host core of one synchronous act step over pinned zero-copy buffers:
// copy the observation in, clear the completion flag, launch, spin on the
// flag, copy the action out.  The launch is a callable, so this header
// needs no HIP and compiles into a plain C++ test program.
#pragma once

#include <chrono>
#include <cstring>

namespace actsync {

// the wall time 2 000 000 iterations of the earlier Python spin took
constexpr double kTimeoutS = 0.1;

inline void cpu_pause() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield");
#endif
}

// Returns true once the flag is seen set (action copied to `out`), false
// when `timeout_s` of wall time passes first; after a false return it has
// launched nothing more and `out` is untouched.
template <class Launch>
inline bool run(float* obs_pin, const float* obs, int n_obs,
                const float* act_pin, float* out, int n_act, int* flag,
                double timeout_s, Launch&& launch) {
  std::memcpy(obs_pin, obs, sizeof(float) * (size_t)n_obs);
  __atomic_store_n(flag, 0, __ATOMIC_RELEASE);
  launch();
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  for (;;) {
    for (int i = 0; i < 64; ++i) {
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != 0) {
        std::memcpy(out, act_pin, sizeof(float) * (size_t)n_act);
        return true;
      }
      cpu_pause();
    }
    if (std::chrono::duration<double>(clock::now() - t0).count() > timeout_s)
      return false;
  }
}

}  // namespace actsync
