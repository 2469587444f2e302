// Per-device host-side state, one store for all of it.  One process may drive several GPUs from several threads
// (torch.nn.DataParallel, pretrain.py:93-94): everything the host side remembers between calls is kept PER DEVICE and
// built exactly once per device, whichever thread gets there first.  No HIP include: a host-only program can use this file.
#pragma once
#include <mutex>
#include <new>
#include <type_traits>

#define VT_MAX_DEVICES 64
inline int vt_current_device();   // common.hpp: the calling thread's current device, -1 outside 0 .. VT_MAX_DEVICES - 1

// VT_MAX_DEVICES slots of T.  A slot is constructed on its first use -- as T(dev) where T takes the index, else T() -- under
// std::call_once, and lives as long as the process (host-side handles; nothing is destroyed).  What a T holds that changes
// after construction is T's own business: atomics or a mutex of its own.
template <typename T>
class VtPerDevice {
 public:
  T* at(int dev) {   // null: no such device
    if (dev < 0 || dev >= VT_MAX_DEVICES) return nullptr;
    Slot& s = slots_[dev];
    std::call_once(s.once, [&s, dev] {
      if constexpr (std::is_constructible<T, int>::value) new (s.mem) T(dev);
      else new (s.mem) T();
    });
    return reinterpret_cast<T*>(s.mem);
  }
  T* get() { return at(vt_current_device()); }

 private:
  struct Slot {
    std::once_flag once;
    alignas(T) unsigned char mem[sizeof(T)];
  };
  Slot slots_[VT_MAX_DEVICES];
};
