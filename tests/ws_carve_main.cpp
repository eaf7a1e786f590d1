// ws_carve_main.cpp — stand-alone check of csrc/nc_ws.h (host compiler only, built under the
// address and undefined-behaviour sanitizers by tests/test_workspace_sizes_cpu.py).  A mixed
// layout is measured, then carved on a real buffer of exactly the measured size and written end
// to end, so a section past the measured size is a sanitizer report.  Prints one line per check
// and exits non-zero on the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nightcore-to-flac-analyzer_amd/csrc/nc_ws.h"

using nc::WsCarve;

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                  \
    }                                                            \
  } while (0)

struct Sec {
  size_t elem, count, align;
  bool skip;
};
struct Placed {
  size_t off, bytes;  // where the section should start, and its unrounded size
  char* p;
};

// the layouts of the project in small: 256-byte sections, trim's 8-byte packing, beat's
// back-to-back arrays, a reserved gap, an empty section and a closing skip(0)
static const Sec kLayout[] = {
    {8, 3, 256, false},  {4, 63, 256, false}, {4, 64, 256, false}, {4, 65, 256, false}, {8, 5, 256, true},
    {8, 3, 8, false},    {8, 7, 8, false},    {8, 9, 8, false},    {8, 10, 8, false},   {4, 10, 4, false},
    {1, 10, 1, false},   {1, 255, 256, false}, {1, 256, 256, false}, {1, 257, 256, false}, {2, 0, 256, false},
    {4, 4, 16, false},   {8, 1, 8, false},    {1, 0, 256, true},
};

static std::vector<Placed> run(WsCarve& c) {
  std::vector<Placed> out;
  for (const Sec& s : kLayout) {
    const size_t a = s.align, at = (c.bytes() + a - 1) / a * a;
    char* p = nullptr;
    if (s.skip) {
      c.skip(s.elem * s.count, a);
    } else if (s.elem == 8) {
      p = reinterpret_cast<char*>(c.take<int64_t>(s.count, a));
    } else if (s.elem == 4) {
      p = reinterpret_cast<char*>(c.take<float>(s.count, a));
    } else if (s.elem == 2) {
      p = reinterpret_cast<char*>(c.take<uint16_t>(s.count, a));
    } else {
      p = reinterpret_cast<char*>(c.take<uint8_t>(s.count, a));
    }
    out.push_back({at, s.elem * s.count, p});
  }
  return out;
}

int main() {
  // measure: no pointers, only offsets
  WsCarve m;
  const std::vector<Placed> pm = run(m);
  for (const Placed& s : pm) CHECK(s.p == nullptr);
  const size_t total = m.bytes();
  CHECK(total != SIZE_MAX && total % 256 == 0);
  std::printf("measured %zu bytes in %zu sections\n", total, pm.size());

  // carve on exactly that many bytes, 256-byte aligned
  char* base = static_cast<char*>(std::aligned_alloc(256, total));
  CHECK(base != nullptr);
  WsCarve c(base);
  const std::vector<Placed> pc = run(c);
  CHECK(c.bytes() == total);  // measure and carve modes agree on the size ...
  size_t end = 0, i = 0;
  for (const Placed& s : pc) {
    const Sec& d = kLayout[i];
    CHECK(s.off == pm[i].off && s.bytes == pm[i].bytes);  // ... and on every offset
    CHECK(s.off >= end);                                  // sections do not overlap
    CHECK(s.off % d.align == 0);
    if (!d.skip) {
      CHECK(s.p == base + s.off);                               // the pointer is the offset
      CHECK(reinterpret_cast<uintptr_t>(s.p) % d.align == 0);   // and respects its align
      std::memset(s.p, 0x5a, s.bytes);                          // inside the buffer (ASan)
    }
    end = s.off + s.bytes;
    ++i;
  }
  CHECK(end <= total);
  std::free(base);
  std::printf("carved: offsets, alignment, no overlap, inside %zu bytes\n", total);

  // skip advances the offset by its bytes rounded up; skip(0, a) only closes to a
  WsCarve k;
  k.skip(1);
  CHECK(k.bytes() == 256);
  k.skip(300, 8);
  CHECK(k.bytes() == 256 + 304);
  k.skip(0);
  CHECK(k.bytes() == 768);
  k.skip(0);
  CHECK(k.bytes() == 768);
  CHECK(k.bytes_plus(4096) == 768 + 4096);
  std::printf("skip advances\n");

  // a count whose bytes wrap size_t, and an offset that does, latch SIZE_MAX
  char dummy[8];
  WsCarve w(dummy);
  CHECK(w.take<double>(SIZE_MAX / 8 + 1) == nullptr && w.bytes() == SIZE_MAX);
  CHECK(w.take<char>(1, 1) == nullptr && w.bytes() == SIZE_MAX);  // latched: later takes stay null
  w.skip(0);
  CHECK(w.bytes() == SIZE_MAX && w.bytes_plus(4096) == SIZE_MAX);
  WsCarve w2;
  w2.skip(SIZE_MAX - 300, 1);
  CHECK(w2.bytes() == SIZE_MAX - 300);
  w2.take<char>(200, 256);  // the round-up to 256 passes the end of size_t
  CHECK(w2.bytes() == SIZE_MAX);
  WsCarve w3;
  w3.skip(SIZE_MAX / 2 + 7, 1);
  w3.take<char>(SIZE_MAX / 2 + 7, 1);  // the sum wraps
  CHECK(w3.bytes() == SIZE_MAX);
  WsCarve w4;
  w4.take<int64_t>(SIZE_MAX / 8);  // the product fits, its round-up does not
  CHECK(w4.bytes() == SIZE_MAX);
  WsCarve w5;
  w5.skip(16, 1);
  CHECK(w5.bytes_plus(SIZE_MAX - 8) == SIZE_MAX);  // slack that would wrap
  std::printf("wraps latch SIZE_MAX\n");
  return 0;
}
