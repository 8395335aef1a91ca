// pass_order_test.cpp -- the fused pass loop's near-first order (csrc/device/pass_order.hpp) on the host: the order
// word kept up by order_insert while the entries arrive equals the stable ascending order of the keys, exhaustively
// for every sequence of up to 6 keys over 3 distinct values, and for a few 16-entry sequences (the word's capacity).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "pass_order.hpp"

using bzr_dev::order_at;
using bzr_dev::order_insert;

static int failed = 0;

// The order the device keeps: entry e arrives behind the earlier entries with key <= its own.
static uint64_t arrive_all(const std::vector<uint32_t> &key) {
  uint64_t order = 0;
  for (uint32_t e = 0; e < key.size(); ++e) {
    uint32_t front = 0;
    for (uint32_t j = 0; j < e; ++j) front += key[j] <= key[e] ? 1u : 0u;
    order = order_insert(order, e, front);
  }
  return order;
}

static void check(const std::vector<uint32_t> &key) {
  std::vector<uint32_t> want(key.size());
  std::iota(want.begin(), want.end(), 0u);
  std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  const uint64_t order = arrive_all(key);
  bool ok = true;
  for (uint32_t p = 0; p < key.size(); ++p) ok = ok && order_at(order, p) == want[p];
  if (key.size() < bzr_dev::kOrderEntries) ok = ok && (order >> (4u * key.size())) == 0u;  // nothing past the length
  if (!ok) {
    ++failed;
    std::printf("FAILED: keys");
    for (uint32_t k : key) std::printf(" %u", k);
    std::printf(" -> order %016llx\n", static_cast<unsigned long long>(order));
  }
}

int main() {
  const uint32_t values[3] = {7u, 0x3F800000u, 0x3F800001u};  // (two of them differ in the last bit)
  long cases = 0;
  for (uint32_t len = 0; len <= 6; ++len) {
    uint32_t total = 1;
    for (uint32_t k = 0; k < len; ++k) total *= 3;
    for (uint32_t code = 0; code < total; ++code, ++cases) {
      std::vector<uint32_t> key(len);
      uint32_t c = code;
      for (uint32_t k = 0; k < len; ++k, c /= 3) key[k] = values[c % 3];
      check(key);
    }
  }
  std::vector<uint32_t> full(16);
  std::iota(full.begin(), full.end(), 100u);
  check(full);  // ascending: the identity
  std::reverse(full.begin(), full.end());
  check(full);  // strictly descending: every arrival goes to the front
  check(std::vector<uint32_t>(16, 5u));  // all equal: collection order
  uint32_t x = 12345u;
  for (int rep = 0; rep < 1000; ++rep, ++cases) {
    for (uint32_t &k : full) k = (x = x * 1664525u + 1013904223u) >> (rep % 2 ? 29 : 0);  // (every other one: many ties)
    check(full);
  }
  cases += 3;
  std::printf("pass order (host): %ld sequences, %d failed\n", cases, failed);
  return failed ? 1 : 0;
}
