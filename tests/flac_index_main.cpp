// Stand-alone driver of csrc/nc_flac_index.cpp for test_flac_cpu.py, built with the host compiler
// under -fsanitize=address,undefined.
//   flac_index_main FILE...          index each file whole and print one summary line per file
//   flac_index_main --fuzz FILE...   index every truncation and every single-bit flip of each file
// Every input sits in a heap block of exactly its own size, so a read past the end is reported.
// Exit status 0 unless an accepted index is inconsistent; a negative status of nc_flac_index is
// an expected outcome for damaged input.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/ncgpu.h"

namespace nc {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace nc

static int index_once(const std::vector<uint8_t>& bytes, bool print, const char* name) {
  std::vector<uint8_t> exact(bytes.begin(), bytes.end());
  static const uint8_t none = 0;
  const uint8_t* p = exact.empty() ? &none : exact.data();
  int64_t info[8] = {0}, n = 0;
  uint8_t md5[16] = {0};
  int rc = nc_flac_index(p, (int64_t)exact.size(), info, md5, nullptr, 0, &n);
  if (rc != 0) {
    if (print) printf("%s: status %d (%s)\n", name, rc, nc::g_err.c_str());
    return nc::g_err.empty() ? 1 : 0;  // a failure must say why
  }
  std::vector<int64_t> rows((size_t)n * 8 + 8);
  int64_t n2 = 0;
  rc = nc_flac_index(p, (int64_t)exact.size(), info, md5, rows.data(), n, &n2);
  if (rc != 0 || n2 != n) return 1;
  int64_t next = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t* r = &rows[(size_t)i * 8];
    if (r[0] < 0 || r[1] <= r[0] || r[1] > (int64_t)exact.size() || r[2] != next || r[3] < 1 || r[3] > 65535 ||
        r[6] < 6 || r[6] > 16 || (i + 1 < n && r[1] != r[8]))
      return 1;
    next += r[3];
  }
  if (next != info[3]) return 1;
  if (n > 1 && nc_flac_index(p, (int64_t)exact.size(), info, md5, rows.data(), n - 1, &n2) != -3) return 1;
  if (print)
    printf("%s: rate %lld channels %lld bits %lld samples %lld frames %lld\n", name, (long long)info[0],
           (long long)info[1], (long long)info[2], (long long)info[3], (long long)n);
  return 0;
}

int main(int argc, char** argv) {
  bool fuzz = argc > 1 && strcmp(argv[1], "--fuzz") == 0;
  int bad = 0;
  for (int a = fuzz ? 2 : 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> bytes;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    if (!fuzz) {
      bad += index_once(bytes, true, argv[a]);
      continue;
    }
    long runs = 0;
    for (size_t cut = 0; cut < bytes.size(); ++cut, ++runs)
      bad += index_once(std::vector<uint8_t>(bytes.begin(), bytes.begin() + cut), false, argv[a]);
    for (size_t bit = 0; bit < bytes.size() * 8; ++bit, ++runs) {
      std::vector<uint8_t> flipped(bytes);
      flipped[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      bad += index_once(flipped, false, argv[a]);
    }
    printf("%s: %ld damaged variants indexed\n", argv[a], runs);
  }
  if (bad) fprintf(stderr, "%d inconsistent results\n", bad);
  return bad ? 1 : 0;
}
