// Stand-alone check of gr_bgzf_scan (csrc/host/gr_bgzf.cpp) for the sanitizers: truncated and malformed headers in heap
// buffers of exactly their size, so that a read behind the end is seen.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/dev/bgzf_scan_check.cpp goldrush_amd/csrc/host/gr_bgzf.cpp -o /tmp/bgzf_scan_check && /tmp/bgzf_scan_check
#include "../../include/grpath_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::vector<unsigned char>
member(size_t payload, const std::vector<unsigned char>& extra, unsigned isize)
{
  const size_t xlen = extra.size() + 6, total = 12 + xlen + payload + 8;
  std::vector<unsigned char> m = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, (unsigned char)(xlen & 255), (unsigned char)(xlen >> 8) };
  m.insert(m.end(), extra.begin(), extra.end());
  const unsigned char bc[6] = { 'B', 'C', 2, 0, (unsigned char)((total - 1) & 255), (unsigned char)((total - 1) >> 8) };
  m.insert(m.end(), bc, bc + 6);
  m.resize(m.size() + payload, 0x03);
  for (int i = 0; i < 4; ++i) {
    m.push_back(0x11 * (i + 1));
  }
  for (int i = 0; i < 4; ++i) {
    m.push_back((unsigned char)(isize >> (8 * i)));
  }
  return m;
}

static unsigned long n_calls = 0;

// the scan on a copy of exactly n bytes; what it returns must lie inside them
static void
check(const unsigned char* src, size_t n, size_t cap)
{
  unsigned char* buf = (unsigned char*)malloc(n ? n : 1);
  if (n) {
    memcpy(buf, src, n);
  }
  std::vector<grp_bgzf_block> blocks(cap ? cap : 1);
  size_t consumed = ~(size_t)0;
  int why = -1;
  const size_t nb = gr_bgzf_scan(buf, n, blocks.data(), cap, &consumed, &why);
  ++n_calls;
  bool ok = nb <= cap && consumed <= n && why >= 0 && why <= 2;
  size_t end = 0;
  for (size_t i = 0; ok && i < nb; ++i) {
    ok = blocks[i].comp_off >= end + 18 && blocks[i].comp_off + blocks[i].comp_len + 8 <= consumed && blocks[i].text_len <= 65536;
    end = blocks[i].comp_off + blocks[i].comp_len + 8;
  }
  ok = ok && end == consumed;
  if (!ok) {
    fprintf(stderr, "bad result: n=%zu cap=%zu -> %zu blocks, consumed %zu, why %d\n", n, cap, nb, consumed, why);
    exit(1);
  }
  free(buf);
}

int
main()
{
  const std::vector<unsigned char> extra = { 'X', 'Y', 3, 0, 1, 2, 3 };
  std::vector<unsigned char> file = member(40, {}, 100), b = member(5, extra, 65536), c = member(2, {}, 0);
  file.insert(file.end(), b.begin(), b.end());
  file.insert(file.end(), c.begin(), c.end());
  // every prefix, every table capacity
  for (size_t n = 0; n <= file.size(); ++n) {
    for (size_t cap = 0; cap <= 4; ++cap) {
      check(file.data(), n, cap);
    }
  }
  // every value in every header byte of the second member (its extra field included), at every cut behind it
  const size_t at = member(40, {}, 100).size();
  for (size_t i = 0; i < 12 + extra.size() + 6; ++i) {
    for (unsigned v = 0; v < 256; ++v) {
      std::vector<unsigned char> f = file;
      f[at + i] = (unsigned char)v;
      for (size_t n = at + i + 1; n <= f.size(); n += (n < at + 40 ? 1 : 7)) {
        check(f.data(), n, 4);
      }
      check(f.data(), f.size(), 4);
    }
  }
  // XLEN and SLEN that point behind the buffer, BSIZE smaller than the header, ISIZE too large
  for (unsigned xlen : { 0u, 1u, 5u, 6u, 7u, 0xffffu }) {
    for (unsigned slen : { 0u, 1u, 2u, 3u, 0xffffu }) {
      for (unsigned bsize : { 0u, 17u, 25u, 26u, 0xffffu }) {
        std::vector<unsigned char> f = member(2, {}, 0);
        f[10] = xlen & 255, f[11] = xlen >> 8, f[14] = slen & 255, f[15] = slen >> 8, f[16] = bsize & 255, f[17] = bsize >> 8;
        for (size_t n = 0; n <= f.size(); ++n) {
          check(f.data(), n, 2);
        }
      }
    }
  }
  // noise behind a valid magic
  std::mt19937 rng(1);
  for (int t = 0; t < 20000; ++t) {
    std::vector<unsigned char> f(rng() % 64);
    for (auto& x : f) {
      x = (unsigned char)rng();
    }
    const unsigned char magic[4] = { 0x1f, 0x8b, 8, 4 };
    if (!f.empty()) {
      memcpy(f.data(), magic, f.size() < 4 ? f.size() : 4);
    }
    check(f.data(), f.size(), 3);
  }
  printf("gr_bgzf_scan: %lu calls, all results inside their buffers\n", n_calls);
  return 0;
}
