// The staging carve (csrc/host/staging.hpp) on host memory: a layout measured, then carved over a buffer of exactly
// the measured size.  Every region is 256-byte aligned, inside the buffer and disjoint from the others; the last one
// ends within 255 bytes of the buffer's end; a layout whose second pass takes more than its first is an error.
// Stand-alone: includes nothing of the library but that header.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "staging.hpp"

using bzr_staging::Staging;

namespace {
int failed = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      ++failed;                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
    }                                                                  \
  } while (0)

struct Region {
  char *p;
  size_t bytes;
};
// Takes `count` elements of T and notes the region.
template <typename T>
T *take(Staging &st, std::vector<Region> &regs, size_t count) {
  T *p = st.take<T>(count);
  regs.push_back({reinterpret_cast<char *>(p), count * sizeof(T)});
  return p;
}

// Byte counts 0, 1, 255, 256, 257 in mixed element sizes, and one conditional take.
struct Mixed {
  bool with_extra;
  std::vector<Region> regs;
  void operator()(Staging &st) {
    regs.clear();
    take<char>(st, regs, 0);
    take<uint8_t>(st, regs, 1);
    take<char>(st, regs, 255);
    take<uint32_t>(st, regs, 64);             // 256 bytes
    take<char>(st, regs, 257);
    take<uint64_t>(st, regs, 33);             // 264 bytes
    if (with_extra) take<float>(st, regs, 6 * 65);  // 1560 bytes: rays of a batch of 65
    take<uint16_t>(st, regs, 3);
    take<double>(st, regs, 0);
    take<uint8_t>(st, regs, 257);
  }
};

int ok_alloc_calls = 0;
// A 256-byte aligned address in `store` (as a device allocation's), with size() - 256 bytes behind it.
char *aligned(std::vector<char> &store) {
  return store.data() + (256 - reinterpret_cast<uintptr_t>(store.data()) % 256) % 256;
}

void check_layout(bool with_extra, size_t want_bytes) {
  Mixed layout{with_extra, {}};
  std::vector<char> store;
  void *base = nullptr;
  size_t size = 0;
  auto alloc = [&](size_t bytes) {
    ++ok_alloc_calls;
    for (auto const &r : layout.regs) CHECK(r.p == nullptr);  // the measuring pass hands out no pointer
    store.resize(bytes + 256);
    base = aligned(store);
    size = bytes;
    return 0;
  };
  const size_t measured = bzr_staging::measure(layout);
  const int s = bzr_staging::carve(base, alloc, layout, -1);
  char *const buf = static_cast<char *>(base);
  CHECK(s == 0);
  CHECK(size == want_bytes);
  CHECK(size == measured);
  CHECK(layout.regs.size() == (with_extra ? 10u : 9u));
  size_t last_end = 0;
  for (size_t i = 0; i < layout.regs.size(); ++i) {
    const Region &a = layout.regs[i];
    CHECK(a.p != nullptr);
    CHECK(reinterpret_cast<uintptr_t>(a.p) % 256 == 0);
    CHECK(a.p >= buf && a.p + a.bytes <= buf + size);
    for (size_t j = i + 1; j < layout.regs.size(); ++j) {
      const Region &b = layout.regs[j];
      CHECK(a.p + a.bytes <= b.p || b.p + b.bytes <= a.p);
    }
    if (a.bytes) last_end = static_cast<size_t>(a.p + a.bytes - buf);
  }
  CHECK(last_end <= size && size - last_end <= 255);
  for (auto const &r : layout.regs)  // every byte handed out can be written
    for (size_t k = 0; k < r.bytes; ++k) r.p[k] = 1;
}
}  // namespace

int main() {
  static_assert(bzr_staging::round256(0) == 0 && bzr_staging::round256(1) == 256 && bzr_staging::round256(255) == 256 &&
                    bzr_staging::round256(256) == 256 && bzr_staging::round256(257) == 512,
                "round256");
  // 0 + 256 + 256 + 256 + 512 + 512 (+ 1792) + 256 + 0 + 512
  check_layout(false, 2560);
  check_layout(true, 2560 + 1792);
  CHECK(ok_alloc_calls == 2);

  {  // measuring does no arithmetic on a null base and returns null
    Staging st;
    CHECK(st.take<float>(100) == nullptr && st.off == 512);
    CHECK(st.take<char>(0) == nullptr && st.off == 512);
  }
  {  // nothing to take: the allocator is asked for 0 bytes, a null base is fine
    size_t asked = 1;
    void *base = nullptr;
    const int s = bzr_staging::carve(base, [&](size_t bytes) { asked = bytes; return 0; }, [](Staging &) {}, -1);
    CHECK(s == 0 && asked == 0);
  }
  {  // a layout whose second pass takes more than its first
    int pass = 0;
    std::vector<char> store(4096 + 256);
    void *base = nullptr;
    auto grow = [&](Staging &st) { st.take<char>(++pass == 1 ? 256 : 257); };
    const int s = bzr_staging::carve(base, [&](size_t) { base = aligned(store); return 0; }, grow, -1);
    CHECK(s == -1 && pass == 2);
  }
  {  // ... and one that takes less
    int pass = 0;
    std::vector<char> store(4096 + 256);
    void *base = nullptr;
    auto shrink = [&](Staging &st) { st.take<char>(++pass == 1 ? 257 : 256); };
    const int s = bzr_staging::carve(base, [&](size_t) { base = aligned(store); return 0; }, shrink, -1);
    CHECK(s == -1);
  }
  {  // the allocator's own status ends the call before the second pass
    int pass = 0;
    void *base = nullptr;
    const int s = bzr_staging::carve(base, [&](size_t) { return 7; }, [&](Staging &st) { ++pass; st.take<int>(1); }, -1);
    CHECK(s == 7 && pass == 1);
  }
  {  // the pointer-assigning take
    std::vector<char> store(1024);
    Staging st{aligned(store)};
    uint32_t *a = nullptr;
    const double *b = nullptr;
    st.take(a, 3), st.take(b, 2);
    CHECK(reinterpret_cast<char *>(a) == st.base && reinterpret_cast<const char *>(b) == st.base + 256 && st.off == 512);
  }
  std::printf("staging (host): %d failed\n", failed);
  return failed ? 1 : 0;
}
