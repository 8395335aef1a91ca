// Staging buffers carved out of one allocation, host code only (no HIP header: a plain C++ program can include it).
// A layout is a callable that takes its regions from a Staging in a fixed order; carve() runs it twice, to measure and
// then over an allocation of that size, so a layout is stated once and the allocation is never smaller than its takes.
#pragma once
#include <cstddef>

namespace bzr_staging {
constexpr size_t round256(size_t b) { return (b + 255) & ~size_t(255); }

struct Staging {  // 256-byte aligned regions of `base`, in order; with no base it only measures: every take is null
  char *base = nullptr;
  size_t off = 0;
  template <typename T>
  constexpr T *take(size_t count) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += round256(count * sizeof(T));
    return p;
  }
  template <typename T>
  constexpr void take(T *&p, size_t count) { p = take<T>(count); }
};

template <typename Layout>
constexpr size_t measure(Layout &&layout) {  // the bytes `layout` takes
  Staging st;
  layout(st);
  return st.off;
}

// `alloc(bytes)` leaves at least the measured bytes at `buf` (a non-zero status of its own ends the call).  The
// layout only takes regions and assigns the pointers, and must not depend on anything its first run changes: a
// second run that does not end where the first did returns `mismatch`.
template <typename Status, typename Alloc, typename Layout>
Status carve(void *&buf, Alloc &&alloc, Layout &&layout, Status mismatch) {
  const size_t bytes = measure(layout);
  if (Status s = alloc(bytes)) return s;
  Staging st{static_cast<char *>(buf)};
  layout(st);
  return st.off == bytes ? Status{} : mismatch;
}
}  // namespace bzr_staging
