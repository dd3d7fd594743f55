// Host side of the guard mode of the library's device allocator (dev_alloc / dev_free, ctx.hip; DCGP_GUARD_WS): which allocations are
// live, how many bytes each was asked for, and the scan of a guard copied back from the device.  Plain C++, no HIP: tests/dev_guard_check.cc
// runs it without a GPU.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

namespace dev_guard {

constexpr size_t kDefaultBytes = 4096;   // DCGP_GUARD_WS set, but not to a number
constexpr int kMaxReported = 8;          // violations a report spells out

// Guard size from the variable's text: nullptr (unset) and values <= 0: 0 = mode off; not a number: kDefaultBytes; rounded up to a multiple of 256.
inline size_t parse_bytes(const char* text) {
  if (!text) return 0;
  char* end = nullptr;
  const long v = strtol(text, &end, 10);
  if (end == text) return kDefaultBytes;
  if (v <= 0) return 0;
  return ((size_t)v + 255) / 256 * 256;
}

// Offset of the first byte of guard[0 .. n) that is not 0xFF, -1: the guard is whole.
inline long scan(const unsigned char* guard, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (guard[i] != 0xFF) return (long)i;
  return -1;
}

struct Entry { size_t bytes = 0; std::string label; };                       // requested bytes: the guard starts there
struct Violation { std::string label; size_t bytes = 0; long offset = 0; bool at_free = false; };   // offset: first bad byte past the requested end

struct Registry {
  std::map<const void*, Entry> live;
  std::vector<Violation> freed_bad;   // found by a free's check, not yet reported

  // a pointer the device allocator hands out a second time (after its free) simply takes the new size and label
  void add(const void* p, size_t bytes, const char* label) { live[p] = Entry{bytes, label ? label : ""}; }
  const Entry* find(const void* p) const {
    auto it = live.find(p);
    return it == live.end() ? nullptr : &it->second;
  }
  bool remove(const void* p, Entry* out = nullptr) {
    auto it = live.find(p);
    if (it == live.end()) return false;
    if (out) *out = it->second;
    live.erase(it);
    return true;
  }
  void remember(const Entry& e, long offset) { freed_bad.push_back(Violation{e.label, e.bytes, offset, true}); }
};

// "label (bytes B) +offset[ at free]; ..." of the first kMaxReported violations into report[0 .. report_len), always terminated; returns how
// many were spelled out.
inline int write_report(const std::vector<Violation>& bad, char* report, int report_len) {
  std::string s;
  int n = 0;
  for (const Violation& v : bad) {
    if (n == kMaxReported) break;
    char line[256];
    snprintf(line, sizeof(line), "%s%s (%zu B) +%ld%s", n ? "; " : "", v.label.c_str(), v.bytes, v.offset, v.at_free ? " at free" : "");
    s += line;
    ++n;
  }
  if (report && report_len > 0) {
    const size_t k = s.size() < (size_t)report_len - 1 ? s.size() : (size_t)report_len - 1;
    s.copy(report, k);
    report[k] = 0;
  }
  return n;
}

}  // namespace dev_guard
