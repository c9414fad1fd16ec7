// Stand-alone host test of the act_sync spin core (ops/csrc/act_sync.h)
// with a fake launch.  Built with -fsanitize=address,undefined by
// tests/test_act_sync_host.py; never touches a GPU.
//
//   act_sync_host set     the "kernel" is a thread that reads the staged
//                         observation, writes the action, then sets the flag
//   act_sync_host never   nothing ever sets the flag: run() must give up
//                         within its wall-time bound and leave `out` alone

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "act_sync.h"

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  constexpr int O = 17, A = 6;
  std::vector<float> obs_pin(O, -1.f), obs(O), act_pin(A, 0.f), out(A, 7.f);
  for (int i = 0; i < O; ++i) obs[i] = 0.5f * (float)i;
  int flag = 1;   // stale "done" from the step before: run() must clear it
  using clock = std::chrono::steady_clock;

  if (mode == "set") {
    for (int rep = 0; rep < 200; ++rep) {
      std::thread worker;
      int launches = 0;
      const bool ok = actsync::run(
          obs_pin.data(), obs.data(), O, act_pin.data(), out.data(), A,
          &flag, 5.0, [&] {
            ++launches;
            if (__atomic_load_n(&flag, __ATOMIC_ACQUIRE) != 0) launches = -99;
            worker = std::thread([&] {
              if (rep % 2) std::this_thread::sleep_for(
                  std::chrono::microseconds(50));
              for (int j = 0; j < A; ++j)
                act_pin[j] = obs_pin[j] + obs_pin[O - 1] + (float)rep;
              __atomic_store_n(&flag, 1, __ATOMIC_RELEASE);
            });
          });
      worker.join();
      if (!ok || launches != 1) {
        std::printf("FAIL set: ok=%d launches=%d\n", (int)ok, launches);
        return 1;
      }
      for (int j = 0; j < A; ++j)
        if (out[j] != obs[j] + obs[O - 1] + (float)rep) {
          std::printf("FAIL set: out[%d]=%g\n", j, out[j]);
          return 1;
        }
      if (std::memcmp(obs_pin.data(), obs.data(), sizeof(float) * O) != 0) {
        std::printf("FAIL set: observation not staged\n");
        return 1;
      }
    }
    std::printf("OK set\n");
    return 0;
  }

  if (mode == "never") {
    const double bound = 0.05;
    int launches = 0;
    const auto t0 = clock::now();
    const bool ok = actsync::run(obs_pin.data(), obs.data(), O,
                                 act_pin.data(), out.data(), A, &flag, bound,
                                 [&] { ++launches; });
    const double dt =
        std::chrono::duration<double>(clock::now() - t0).count();
    bool fine = !ok && launches == 1 && flag == 0 && dt >= bound
        && dt < bound + 1.0;
    for (int j = 0; j < A; ++j) fine = fine && out[j] == 7.f;
    std::printf("%s never: ok=%d launches=%d flag=%d dt=%.4f\n",
                fine ? "OK" : "FAIL", (int)ok, launches, flag, dt);
    return fine ? 0 : 1;
  }

  std::printf("usage: act_sync_host set|never\n");
  return 2;
}
