// VtPerDevice under ThreadSanitizer: sixteen threads ask for the slots of four devices a thousand times each.  Every slot must be
// built exactly once, every thread must see the same object, and an index outside 0 .. VT_MAX_DEVICES - 1 has no slot.
// Plain C++, host only: includes nothing but the store (tests/test_host_per_device.py builds and runs it).
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>
#include "per_device.hpp"

static std::atomic<int> g_built[VT_MAX_DEVICES];
struct Probe {
  int dev;
  int payload;   // plain: written by the constructor, read by every thread -- the race TSan would report
  explicit Probe(int d) : dev(d), payload(1000 + d) { g_built[d].fetch_add(1); }
};
struct Plain {   // a T without an index constructor
  int v = 7;
};

int main() {
  static VtPerDevice<Probe> store;
  static VtPerDevice<Plain> plain;
  const int devs[4] = {0, 1, 17, VT_MAX_DEVICES - 1};
  std::atomic<int> bad{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < 16; ++t)
    threads.emplace_back([&] {
      for (int i = 0; i < 1000; ++i)
        for (int d : devs) {
          Probe* p = store.at(d);
          if (!p || p != store.at(d) || p->dev != d || p->payload != 1000 + d) bad.fetch_add(1);
          Plain* q = plain.at(d);
          if (!q || q->v != 7) bad.fetch_add(1);
        }
      if (store.at(-1) || store.at(VT_MAX_DEVICES) || store.at(1 << 20)) bad.fetch_add(1);
    });
  for (std::thread& th : threads) th.join();
  int built = 0;
  for (int d = 0; d < VT_MAX_DEVICES; ++d) built += g_built[d].load();
  for (int d : devs)
    if (g_built[d].load() != 1) bad.fetch_add(1);
  if (built != 4) bad.fetch_add(1);
  std::printf("built %d bad %d\n", built, bad.load());
  return bad.load() ? 1 : 0;
}
