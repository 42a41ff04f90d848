// Stand-alone check of the DEFLATE decoder and the CRC32 of csrc/grp_inflate.inc on the CPU: the kernels' own text compiled
// as plain C++ with the 64 lanes run one after the other (GRP_INFLATE_HOST), on the cases tools/dev/inflate_host_cases.py
// writes (every text and compressor form of tests/bgzf_cases.py, the hand-written blocks, the refused inputs, 300 streams
// with flipped bits), each confirmed by zlib first.  For the sanitizers; no device is involved.
//   python tools/dev/inflate_host_cases.py /tmp/inflate_cases.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -w tools/dev/inflate_host_check.cpp goldrush_amd/csrc/host/gr_gzidx.cpp goldrush_amd/csrc/host/gr_fastq.cpp -lz -o /tmp/inflate_host_check
//   /tmp/inflate_host_check /tmp/inflate_cases.bin
// The segment form (k_inflate<grp_gzip_segment>) with the index that feeds it, on plain gzip files (tests/gzip_cases.py writes its streams):
//   python tests/gzip_cases.py /tmp/gzip_cases && /tmp/inflate_host_check --gzip /tmp/gzip_cases/*.gz
// every file is read through GzIndexReader (csrc/host/gr_gzidx.cpp) at spans 1, 50 000 and 10^9; every segment is inflated by
// zlib on its own (inflatePrime + inflateSetDictionary) and by the decoder, at two alignments of the output, with buffers
// that end where the engine's end; then damaged forms of it (flipped bits, text_len +- 1, n_bits off, a shorter history,
// the other flag) must be refused, fail the CRC32 or give the same text — and touch nothing outside their buffers.
// The generated corpus (tests/deflate_gen.py: random codes up to 15 bits, the match sweep, the threshold members, the
// hand-made segments) and the libdeflate fixtures, good and refused — what tests/test_gpu_inflate_generated.py gives the device;
// tests/test_deflate_gen_cpu.py runs the same three commands on a build without the sanitizers:
//   python tools/dev/inflate_host_cases.py --generated /tmp/inflate_gen
//   /tmp/inflate_host_check /tmp/inflate_gen/members.bin
//   /tmp/inflate_host_check --segments /tmp/inflate_gen/segments.bin
//   /tmp/inflate_host_check --gzip /tmp/inflate_gen/gzip/*.gz
#define GRP_INFLATE_HOST
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include <zlib.h>
#include "../../include/grpath_ingest.h"
#include "../../goldrush_amd/csrc/host/gr_gzidx.hpp"
#include "../../goldrush_amd/csrc/host/gr_fastq.hpp"
#include "../../goldrush_amd/csrc/grp_inflate.inc"
// file: u32 n; per case: u32 comp_len, u32 text_len, u32 expect_ok, u32 crc, u32 pre (bytes in front of payload), payload(pre+comp_len), text
static InfLds g_s;
static CrcLds g_cs;

// a case file that ends early is an error, not a case
static void must_read(void* to, size_t size, size_t n, FILE* f)
{
  if (fread(to, size, n, f) != n) { printf("the case file ends early\n"); exit(2); }
}

// the segment by zlib alone: the bits from comp_bit on with the history as the dictionary
static bool zlib_segment(const uint8_t* file, size_t n_file, const gr::GzSegment& g, const uint8_t* dict, std::vector<char>& out)
{
  z_stream z; memset(&z, 0, sizeof z);
  if (inflateInit2(&z, -15) != Z_OK) return false;
  size_t at = g.comp_bit >> 3;
  const int skip = (int)(g.comp_bit & 7);
  if (skip) { inflatePrime(&z, 8 - skip, file[at] >> skip); ++at; }
  if (g.dict_len) inflateSetDictionary(&z, dict, g.dict_len);
  out.assign(g.text_len + 1, 0);
  z.next_in = (Bytef*)file + at; z.avail_in = (uInt)(((g.comp_bit + g.n_bits + 7) >> 3) - at);
  z.next_out = (Bytef*)out.data(); z.avail_out = (uInt)out.size();
  bool ok = false;
  for (;;) {
    const int rc = inflate(&z, Z_BLOCK);
    if (rc != Z_OK && rc != Z_STREAM_END) break;
    const uint64_t bit = 8 * (uint64_t)((const uint8_t*)z.next_in - file) - (uint64_t)(z.data_type & 63);
    if ((z.data_type & 128) && bit == g.comp_bit + g.n_bits) { ok = z.total_out == g.text_len && ((z.data_type & 64) != 0) == ((g.flags & 1) != 0); break; }
    if (rc == Z_STREAM_END || z.avail_out == 0 || (z.avail_in == 0 && !(z.data_type & 128))) break;
  }
  inflateEnd(&z);
  (void)n_file;
  return ok;
}

static int gzip_main(int argc, char** argv)
{
  uint32_t tabs[1056]; crc_tables(tabs);
  int bad = 0; uint64_t n_seg = 0, n_dmg = 0, n_refused = 0, n_crc = 0, n_same = 0;
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { printf("%s: cannot open\n", argv[a]); return 2; }
    std::vector<uint8_t> raw; uint8_t tmp[65536]; size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) raw.insert(raw.end(), tmp, tmp + k);
    fclose(f);
    // the engine's buffer: the bytes, 8 bytes of zero padding, nothing behind
    std::vector<uint32_t> compw((raw.size() + 8 + 3) / 4, 0);
    uint8_t* comp = (uint8_t*)compw.data();
    memcpy(comp, raw.data(), raw.size());
    for (uint64_t span : { uint64_t(1), uint64_t(50000), uint64_t(1000000000) }) {
      gr::GzIndexReader rd(argv[a], span, uint64_t(1) << 32);
      std::vector<char> text, piece(1 << 16);
      while ((k = rd.read(piece.data(), piece.size())) > 0) text.insert(text.end(), piece.data(), piece.data() + k);
      std::unique_ptr<gr::GzIndex> ix = rd.take();
      if (!ix) { printf("%s span %llu: no index\n", argv[a], (unsigned long long)span); ++bad; continue; }
      uint64_t off = 0;
      for (size_t i = 0; i < ix->segs.size(); ++i) {
        const gr::GzSegment& g = ix->segs[i];
        ++n_seg;
        // the history in a buffer of its own size (4-byte aligned, as the host program lays them out; 8 bytes of padding as in the engine)
        std::vector<uint32_t> dictw((g.dict_len + 8 + 3) / 4 + 1, 0);
        uint8_t* dict = (uint8_t*)dictw.data();
        if (g.dict_len) memcpy(dict, ix->dict(g), g.dict_len);
        std::vector<char> zt;
        if (!zlib_segment(raw.data(), raw.size(), g, dict, zt) || memcmp(zt.data(), text.data() + off, g.text_len) != 0) { printf("%s span %llu seg %zu: zlib does not confirm the segment\n", argv[a], (unsigned long long)span, i); ++bad; }
        grp_gzip_segment e{ g.comp_bit, g.n_bits, 0, g.dict_len, g.text_len, g.crc32, g.flags };
        std::vector<char> outw((size_t)g.text_len + 3 + 1);
        for (int mis = 0; mis < 2; ++mis) {
          char* out = outw.data() + (mis ? 3 : 0);
          memset(outw.data(), 0x55, outw.size());
          memset(&g_s, 0xAA, sizeof g_s);
          const uint32_t st = inf_entry(g_s, comp, dict, e, out);
          if (st != 0 || memcmp(out, text.data() + off, g.text_len) != 0) { printf("%s span %llu seg %zu mis %d: status %u (%s) or text differs\n", argv[a], (unsigned long long)span, i, mis, st, INF_STATUS_TEXT[st]); ++bad; continue; }
          if ((uint8_t)out[g.text_len] != 0x55 && !(mis == 0 && g.text_len + 1 >= outw.size())) { printf("%s seg %zu: wrote behind the text\n", argv[a], i); ++bad; }
          if (crc_member(g_cs, tabs, out, g.text_len) != g.crc32) { printf("%s span %llu seg %zu: crc differs\n", argv[a], (unsigned long long)span, i); ++bad; }
        }
        // damaged forms (a sample of the segments where there are many)
        if (ix->segs.size() <= 40 || i % 7 == 0) {
          std::vector<grp_gzip_segment> forms;
          std::vector<int> flip; // -1: none, else the bit of the segment that is flipped
          auto add = [&](grp_gzip_segment x, int fb) { forms.push_back(x); flip.push_back(fb); };
          grp_gzip_segment x = e;
          x.text_len = e.text_len + 1; add(x, -1);
          x = e; x.text_len = e.text_len - 1; add(x, -1);
          for (int64_t d : { -1ll, -3ll, -8ll, -17ll, -1000ll }) { x = e; if ((int64_t)e.n_bits + d > 0) { x.n_bits = e.n_bits + d; add(x, -1); } }
          if (g.comp_bit + g.n_bits + 64 <= raw.size() * 8) { x = e; x.n_bits = e.n_bits + 1; add(x, -1); x.n_bits = e.n_bits + 40; add(x, -1); }
          if (i > 0 && !(ix->segs[i - 1].flags & 1)) { x = e; x.comp_bit = ix->segs[i - 1].comp_bit; x.n_bits += ix->segs[i - 1].n_bits; add(x, -1); } // a block too many in front, with this history
          x = e; x.flags ^= 1; add(x, -1);
          if (e.dict_len) { x = e; x.dict_len = e.dict_len - 1; x.dict_off = 1; add(x, -1); x.dict_len = e.dict_len / 2; x.dict_off = e.dict_len - x.dict_len; add(x, -1); x.dict_len = 0; x.dict_off = 0; add(x, -1); }
          uint64_t r = 0x9e3779b97f4a7c15ull * (i + 1) + span;
          for (int t = 0; t < 24; ++t) { r = r * 6364136223846793005ull + 1442695040888963407ull; add(e, (int)((r >> 33) % e.n_bits)); }
          for (size_t q = 0; q < forms.size(); ++q) {
            const grp_gzip_segment& d = forms[q];
            ++n_dmg;
            std::vector<char> o2((size_t)d.text_len + 1, 0x55);
            uint64_t fbit = 0;
            if (flip[q] >= 0) { fbit = d.comp_bit + (uint64_t)flip[q]; comp[fbit >> 3] ^= (uint8_t)(1u << (fbit & 7)); }
            memset(&g_s, 0xAA, sizeof g_s);
            const uint32_t st = inf_entry(g_s, comp, dict, d, o2.data());
            if (flip[q] >= 0) { comp[fbit >> 3] ^= (uint8_t)(1u << (fbit & 7)); }
            if ((uint8_t)o2[d.text_len] != 0x55) { printf("%s seg %zu form %zu: wrote behind the text\n", argv[a], i, q); ++bad; }
            if (st != 0) { ++n_refused; continue; }
            if (crc_member(g_cs, tabs, o2.data(), d.text_len) != d.crc32) { ++n_crc; continue; }
            // accepted: then it must be the segment's own text (a flipped padding bit of a stored block, a history that no distance reaches)
            if (d.text_len != e.text_len || memcmp(o2.data(), text.data() + off, e.text_len) != 0) { printf("%s span %llu seg %zu form %zu: accepted a damaged segment\n", argv[a], (unsigned long long)span, i, q); ++bad; } else { ++n_same; }
          }
        }
        off += g.text_len;
      }
      if (off != text.size()) { printf("%s span %llu: the segments hold %llu bytes of %zu\n", argv[a], (unsigned long long)span, (unsigned long long)off, text.size()); ++bad; }
    }
  }
  printf("%llu segments; %llu damaged forms: %llu refused, %llu failed the CRC32, %llu gave the segment's text; %d bad\n", (unsigned long long)n_seg, (unsigned long long)n_dmg, (unsigned long long)n_refused, (unsigned long long)n_crc, (unsigned long long)n_same, bad);
  return bad != 0;
}

// hand-made segments (inflate_host_cases.py: write_segments): each with its own file and a history at a given alignment
static int segments_main(const char* path)
{
  FILE* f = fopen(path, "rb");
  if (!f) { printf("%s: cannot open\n", path); return 2; }
  uint32_t n = 0; must_read(&n, 4, 1, f);
  uint32_t tabs[1056]; crc_tables(tabs);
  int bad = 0;
  for (uint32_t c = 0; c < n; ++c) {
    uint64_t q[2]; uint32_t h[7]; must_read(q, 8, 2, f); must_read(h, 4, 7, f);
    const uint32_t dict_len = h[0], text_len = h[1], crc = h[2], flags = h[3], ok = h[4], file_len = h[5], pre = h[6];
    // the engine's buffers: the bytes, 8 bytes of zero padding, nothing behind
    std::vector<uint32_t> compw((file_len + 8 + 3) / 4, 0), dictw((pre + dict_len + 8 + 3) / 4, 0);
    uint8_t* comp = (uint8_t*)compw.data(); uint8_t* dict = (uint8_t*)dictw.data();
    must_read(comp, 1, file_len, f); must_read(dict, 1, pre + dict_len, f);
    std::vector<char> text(text_len + 1), outw((size_t)text_len + 3 + 1);
    must_read(text.data(), 1, text_len, f);
    const grp_gzip_segment e{ q[0], q[1], pre, dict_len, text_len, crc, flags };
    for (int mis = 0; mis < 2; ++mis) {
      char* out = outw.data() + (mis ? 3 : 0);
      memset(outw.data(), 0x55, outw.size());
      memset(&g_s, 0xAA, sizeof g_s);
      const uint32_t st = inf_entry(g_s, comp, dict, e, out);
      if ((uint8_t)out[text_len] != 0x55) { printf("segment %u: wrote behind the text\n", c); ++bad; }
      if (ok) {
        if (st != 0 || memcmp(out, text.data(), text_len) != 0) { printf("segment %u mis %d: status %u (%s) or text differs\n", c, mis, st, INF_STATUS_TEXT[st]); ++bad; continue; }
        if (crc_member(g_cs, tabs, out, text_len) != crc) { printf("segment %u: crc differs\n", c); ++bad; }
      } else if (st == 0) { printf("segment %u: accepted a bad segment\n", c); ++bad; }
      else if (mis == 0) { printf("segment %u refused: %s\n", c, INF_STATUS_TEXT[st]); }
    }
  }
  fclose(f);
  printf("%u segments, %d bad\n", n, bad);
  return bad != 0;
}

int main(int argc, char** argv)
{
  if (argc >= 3 && !strcmp(argv[1], "--gzip")) {
    return gzip_main(argc, argv);
  }
  if (argc >= 3 && !strcmp(argv[1], "--segments")) {
    return segments_main(argv[2]);
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("%s: cannot open\n", argv[1]); return 2; }
  uint32_t n; must_read(&n, 4, 1, f);
  static InfLds s; static CrcLds cs;
  uint32_t tabs[1056]; crc_tables(tabs);
  int bad = 0;
  for (uint32_t c = 0; c < n; ++c) {
    uint32_t h[5]; must_read(h, 4, 5, f);
    const uint32_t comp_len = h[0], text_len = h[1], ok = h[2], crc = h[3], pre = h[4];
    // words must be readable up to the aligned end: pad
    std::vector<uint32_t> compw((pre + comp_len + 3) / 4 + 1);
    uint8_t* comp = (uint8_t*)compw.data();
    must_read(comp, 1, pre + comp_len, f);
    std::vector<char> text(text_len + 1), outw(text_len + 8 + 3);
    must_read(text.data(), 1, text_len, f);
    memset(&s, 0xAA, sizeof s);
    for (int mis = 0; mis < 2; ++mis) {
      char* out = outw.data() + (mis ? 3 : 0);
      memset(outw.data(), 0x55, outw.size());
      const uint32_t st = inf_entry(s, comp, nullptr, grp_bgzf_block{ pre, comp_len, text_len, crc, 0 }, out);
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
