// Stand-alone check of the DEFLATE decoder and the CRC32 of csrc/grp_inflate.inc on the CPU: the kernels' own text compiled
// as plain C++ with the 64 lanes run one after the other (GRP_INFLATE_HOST), on the cases tools/dev/inflate_host_cases.py
// writes (every text and compressor form of tests/bgzf_cases.py, the hand-written blocks, the refused inputs, 300 streams
// with flipped bits), each confirmed by zlib first.  For the sanitizers; no device is involved.
//   python tools/dev/inflate_host_cases.py /tmp/inflate_cases.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -w tools/dev/inflate_host_check.cpp -o /tmp/inflate_host_check && /tmp/inflate_host_check /tmp/inflate_cases.bin
#define GRP_INFLATE_HOST
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include "../../include/grpath_ingest.h"
#include "../../goldrush_amd/csrc/grp_inflate.inc"
// file: u32 n; per case: u32 comp_len, u32 text_len, u32 expect_ok, u32 crc, u32 pre (bytes in front of payload), payload(pre+comp_len), text
int main(int argc, char** argv)
{
  FILE* f = fopen(argv[1], "rb");
  uint32_t n; fread(&n, 4, 1, f);
  static InfLds s; static CrcLds cs;
  uint32_t tabs[1056]; crc_tables(tabs);
  int bad = 0;
  for (uint32_t c = 0; c < n; ++c) {
    uint32_t h[5]; fread(h, 4, 5, f);
    const uint32_t comp_len = h[0], text_len = h[1], ok = h[2], crc = h[3], pre = h[4];
    // words must be readable up to the aligned end: pad
    std::vector<uint32_t> compw((pre + comp_len + 3) / 4 + 1);
    uint8_t* comp = (uint8_t*)compw.data();
    fread(comp, 1, pre + comp_len, f);
    std::vector<char> text(text_len + 1), outw(text_len + 8 + 3);
    fread(text.data(), 1, text_len, f);
    memset(&s, 0xAA, sizeof s);
    for (int mis = 0; mis < 2; ++mis) {
      char* out = outw.data() + (mis ? 3 : 0);
      memset(outw.data(), 0x55, outw.size());
      const uint32_t st = inf_member(s, comp, pre, comp_len, out, text_len);
      if (ok) {
        if (st != 0 || memcmp(out, text.data(), text_len) != 0) { printf("case %u mis %d: status %u (%s) or text differs\n", c, mis, st, INF_STATUS_TEXT[st]); ++bad; continue; }
        if ((uint8_t)out[text_len] != 0x55) { printf("case %u: wrote behind the text\n", c); ++bad; }
        const uint32_t got = crc_member(cs, tabs, out, text_len);
        if (got != crc) { printf("case %u: crc %08x expected %08x\n", c, got, crc); ++bad; }
      } else if (st == 0) { // the stream itself is good: then the CRC32 must be what refuses it
        if (crc_member(cs, tabs, out, text_len) == crc) { printf("case %u: accepted a bad stream\n", c); ++bad; }
      }
      else if (c < 40 || !ok) { if (mis == 0) printf("case %u refused: %s\n", c, INF_STATUS_TEXT[st]); }
    }
  }
  printf("%u cases, %d bad\n", n, bad);
  return bad != 0;
}
