// parallel_for.h — splits [0, n) over a few host threads (upload-time array fills; not a hot path). Plain C++.
#ifndef YH_PARALLEL_FOR_H_
#define YH_PARALLEL_FOR_H_
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

template <typename F>
void parallel_for(int n, F&& fn) {
  int nt = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (n < 65536 || nt == 1) {
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; t++)
    pool.emplace_back([=, &fn] {
      int lo = (int)((int64_t)n * t / nt), hi = (int)((int64_t)n * (t + 1) / nt);
      for (int i = lo; i < hi; i++) fn(i);
    });
  for (auto& th : pool) th.join();
}
#endif
