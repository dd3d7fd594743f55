// Stand-alone check of csrc/dev_guard.h (the host side of the guarded device allocator): built by tests/test_host_memcheck.py with the host
// compiler under -fsanitize=address,undefined and run without a GPU.  Prints "OK <checks>" and returns 0, or names the first check that failed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dev_guard.h"

static int n_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++n_checks;                                                            \
    if (!(cond)) {                                                         \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);            \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main() {
  using namespace dev_guard;
  // the guard size: unset and <= 0 off, not a number 4096, rounded up to a multiple of 256
  CHECK(parse_bytes(nullptr) == 0);
  CHECK(parse_bytes("0") == 0);
  CHECK(parse_bytes("-5") == 0);
  CHECK(parse_bytes("yes") == 4096);
  CHECK(parse_bytes("") == 4096);
  CHECK(parse_bytes("1") == 256);
  CHECK(parse_bytes("256") == 256);
  CHECK(parse_bytes("257") == 512);
  CHECK(parse_bytes("4096") == 4096);
  CHECK(parse_bytes("5000") == 5120);

  // scan: whole, and one cleared byte at the first, a middle and the last position (the buffer is exactly the guard: a read past it is the sanitizer's)
  for (size_t n : {(size_t)1, (size_t)256, (size_t)4096}) {
    std::vector<unsigned char> g(n, 0xFF);
    CHECK(scan(g.data(), n) == -1);
    for (size_t pos : {(size_t)0, n / 2, n - 1}) {
      g[pos] = 0;
      CHECK(scan(g.data(), n) == (long)pos);
      g[pos] = 0xFE;   // any value but 0xFF counts
      CHECK(scan(g.data(), n) == (long)pos);
      g[pos] = 0xFF;
    }
    if (n > 2) {   // the FIRST bad byte is the one named
      g[n - 1] = 0; g[1] = 7;
      CHECK(scan(g.data(), n) == 1);
    }
  }
  CHECK(scan(nullptr, 0) == -1);

  // register, find, unregister
  Registry reg;
  int a = 0, b = 0;
  CHECK(reg.find(&a) == nullptr);
  reg.add(&a, 100, "first");
  reg.add(&b, 0, nullptr);
  CHECK(reg.live.size() == 2);
  CHECK(reg.find(&a) && reg.find(&a)->bytes == 100 && reg.find(&a)->label == "first");
  CHECK(reg.find(&b) && reg.find(&b)->bytes == 0 && reg.find(&b)->label.empty());
  Entry e;
  CHECK(reg.remove(&a, &e) && e.bytes == 100 && e.label == "first");
  CHECK(!reg.remove(&a, &e));          // a second free of the same pointer is not a registered one
  CHECK(reg.find(&a) == nullptr && reg.live.size() == 1);
  // a pointer the allocator hands out again: with and without a free in between, the latest size and label hold
  reg.add(&a, 4000, "second");
  CHECK(reg.find(&a)->bytes == 4000 && reg.find(&a)->label == "second");
  reg.add(&a, 16, "third");
  CHECK(reg.live.size() == 2 && reg.find(&a)->bytes == 16 && reg.find(&a)->label == "third");
  CHECK(reg.remove(&b) && reg.remove(&a) && reg.live.empty());

  // violations found at free time are remembered in order; the report spells out eight and no more, and never overruns its buffer
  for (int i = 0; i < 11; ++i) reg.remember(Entry{(size_t)(100 + i), "buf" + std::to_string(i)}, i);
  CHECK(reg.freed_bad.size() == 11 && reg.freed_bad[3].offset == 3 && reg.freed_bad[3].at_free);
  char big[4096];
  CHECK(write_report(reg.freed_bad, big, (int)sizeof(big)) == kMaxReported && kMaxReported == 8);
  const std::string s(big);
  CHECK(s.find("buf0 (100 B) +0 at free") == 0);
  CHECK(s.find("buf7 (107 B) +7") != std::string::npos);
  CHECK(s.find("buf8") == std::string::npos);
  std::vector<Violation> one{Violation{"live", 37, 155, false}};
  CHECK(write_report(one, big, (int)sizeof(big)) == 1 && std::string(big) == "live (37 B) +155");
  CHECK(write_report({}, big, (int)sizeof(big)) == 0 && big[0] == 0);
  std::vector<char> small(10, 'x');
  CHECK(write_report(reg.freed_bad, small.data(), (int)small.size()) == 8 && strlen(small.data()) == 9 && std::string(small.data()) == s.substr(0, 9));
  std::vector<char> tiny(1, 'x');
  CHECK(write_report(reg.freed_bad, tiny.data(), 1) == 8 && tiny[0] == 0);
  CHECK(write_report(reg.freed_bad, nullptr, 0) == 8);
  printf("OK %d\n", n_checks);
  return 0;
}
