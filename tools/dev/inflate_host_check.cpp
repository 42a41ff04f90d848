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
// The open form (k_inflate<InfWalkEntry>) with the rounds that drive it (csrc/host/gr_gzwalk.cpp, compiled into this program): every
// file is indexed through GzIndexReader and through gzip_walk over the host-compiled decoder, at spans 1, 4096 and 262144,
// with the default sizes and with tiny ones (every step repeated until it fits); the two indexes must agree field by field.
// Then one open step per segment of the reader's index and its damaged forms (a shorter history, fewer bits, a room one
// byte short), and damaged copies of the file (flipped bits, cut short, bytes appended): each must be left to zlib or
// indexed as the reader indexes it.
//   /tmp/inflate_host_check --walk /tmp/gzip_cases/*.gz
// The members of a file side by side (GRP_GZIP_WALK_MEMBERS: gr_gzwalk.hpp), on the files tests/gzip_member_cases.py writes: all of
// them in one walk with the switch and without it, against the reader's index; then 10 000 open steps from pseudo-random
// bits of the first file, every buffer in a heap block of exactly its size:
//   python tests/gzip_member_cases.py /tmp/gzip_members && /tmp/inflate_host_check --members /tmp/gzip_members/*.gz
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
#include "../../goldrush_amd/csrc/host/gr_gzwalk.cpp" // (the rounds themselves: the command lines above stay as they are)
#include <unistd.h>
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

// ---- --walk ------------------------------------------------------------------------------------------------------------
static uint64_t g_walk_steps = 0, g_walk_overrun = 0;

// grp_gzip_walk on the host: the engine's buffers (the bytes, 8 bytes of zero padding), a text buffer of exactly `room`
static bool walk_launch(const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n, grp_gzip_walk_result* res, uint8_t* hist)
{
  static uint32_t tabs[1056]; static bool have = false;
  if (!have) { crc_tables(tabs); have = true; }
  std::vector<uint32_t> cw((n_comp + 8 + 3) / 4 + 1, 0), dw((n_dict + 8 + 3) / 4 + 1, 0);
  memcpy(cw.data(), comp, n_comp); memcpy(dw.data(), dict, n_dict);
  for (uint32_t i = 0; i < n; ++i) {
    ++g_walk_steps;
    std::vector<char> out((size_t)steps[i].room + 1, 0x55);
    std::vector<uint8_t> h(32768 + 1, 0x55);
    const InfWalkEntry e{ steps[i], &res[i], h.data() };
    memset(&g_s, 0xAA, sizeof g_s);
    const uint32_t st = inf_entry(g_s, (const uint8_t*)cw.data(), (const uint8_t*)dw.data(), e, out.data());
    if ((uint8_t)out[steps[i].room] != 0x55 || h[32768] != 0x55) ++g_walk_overrun;
    if (st != 0) { res[i] = grp_gzip_walk_result{ 0, 0, 0, 0, st, 0, 0 }; continue; }
    res[i].crc32 = crc_member(g_cs, tabs, out.data(), res[i].text_len);
    memcpy(hist + (size_t)32768 * i, h.data(), res[i].hist_len);
  }
  return true;
}

static std::unique_ptr<gr::GzIndex> reader_index(const char* path, uint64_t span, bool* failed, std::vector<char>* text = nullptr)
{
  gr::GzIndexReader rd(path, span, uint64_t(1) << 32);
  std::vector<char> piece(1 << 16);
  size_t k;
  while ((k = rd.read(piece.data(), piece.size())) > 0) { if (text) text->insert(text->end(), piece.data(), piece.data() + k); }
  *failed = rd.failed();
  return rd.take();
}

static bool same_index(const gr::GzIndex& a, const gr::GzIndex& b, const char* what)
{
  if (a.segs.size() != b.segs.size() || a.text_bytes != b.text_bytes || a.max_text != b.max_text || a.max_comp != b.max_comp || a.bytes() != b.bytes() || a.file_size != b.file_size) {
    printf("%s: totals differ (segments %zu / %zu, text %llu / %llu, bytes %llu / %llu)\n", what, a.segs.size(), b.segs.size(), (unsigned long long)a.text_bytes, (unsigned long long)b.text_bytes, (unsigned long long)a.bytes(), (unsigned long long)b.bytes());
    return false;
  }
  for (size_t i = 0; i < a.segs.size(); ++i) {
    const gr::GzSegment &x = a.segs[i], &y = b.segs[i];
    if (x.comp_bit != y.comp_bit || x.n_bits != y.n_bits || x.dict_at != y.dict_at || x.dict_len != y.dict_len || x.text_len != y.text_len || x.crc32 != y.crc32 || x.flags != y.flags || (x.dict_len != 0 && memcmp(a.dict(x), b.dict(y), x.dict_len) != 0)) {
      printf("%s: segment %zu differs (bit %llu / %llu, bits %llu / %llu, dict %u / %u, text %u / %u, crc %08x / %08x, flags %u / %u)\n", what, i, (unsigned long long)x.comp_bit, (unsigned long long)y.comp_bit, (unsigned long long)x.n_bits,
             (unsigned long long)y.n_bits, x.dict_len, y.dict_len, x.text_len, y.text_len, x.crc32, y.crc32, x.flags, y.flags);
      return false;
    }
  }
  return true;
}

// One open step per segment of the reader's index, asked for the segment's own text in a room of exactly that size: it must
// end where the segment ends.  Then the damaged forms of the --gzip mode that carry over to a step, which has no given end:
// the history shorter by a byte, by half, gone (refused, or the same text where no distance reaches that far), the bits cut
// inside the segment (never the whole text: the input ends, or the step stops at an earlier boundary with a prefix of
// it), a room one byte short (the status of its own) — and nothing written behind the room or the 32 KiB of history.
static void walk_steps(const char* path, const std::vector<uint8_t>& raw, int* bad, uint64_t* n_steps, uint64_t* n_forms, uint64_t* n_refused, uint64_t* n_same)
{
  uint32_t tabs[1056]; crc_tables(tabs);
  std::vector<uint32_t> compw((raw.size() + 8 + 3) / 4 + 1, 0);
  uint8_t* comp = (uint8_t*)compw.data();
  memcpy(comp, raw.data(), raw.size());
  bool failed = false; std::vector<char> text;
  std::unique_ptr<gr::GzIndex> ix = reader_index(path, 4096, &failed, &text);
  if (!ix) return;
  uint64_t off = 0;
  for (size_t i = 0; i < ix->segs.size(); off += ix->segs[i].text_len, ++i) {
    const gr::GzSegment& g = ix->segs[i];
    if (ix->segs.size() > 40 && i % 7 != 0) continue;
    std::vector<uint32_t> dictw((g.dict_len + 8 + 3) / 4 + 1, 0);
    uint8_t* dict = (uint8_t*)dictw.data();
    if (g.dict_len) memcpy(dict, ix->dict(g), g.dict_len);
    struct Form { grp_gzip_walk_step s; int kind; }; // 0 the step itself, 1 a shorter history, 2 fewer bits, 3 a room one byte short
    std::vector<Form> forms;
    const grp_gzip_walk_step e{ g.comp_bit, raw.size() * 8 - g.comp_bit, 0, g.dict_len, g.text_len, g.text_len, 0 };
    forms.push_back({ e, 0 });
    if (g.dict_len) { grp_gzip_walk_step x = e; x.dict_off = 1; x.dict_len = g.dict_len - 1; forms.push_back({ x, 1 }); x.dict_len = g.dict_len / 2; x.dict_off = g.dict_len - x.dict_len; forms.push_back({ x, 1 }); x.dict_len = 0; x.dict_off = 0; forms.push_back({ x, 1 }); }
    for (int64_t d : { 1ll, 3ll, 8ll, 17ll, 1000ll }) { if ((int64_t)g.n_bits > d) { grp_gzip_walk_step x = e; x.n_bits = g.n_bits - (uint64_t)d; forms.push_back({ x, 2 }); } }
    { grp_gzip_walk_step x = e; x.n_bits = g.n_bits; forms.push_back({ x, 0 }); } // exactly the segment's bits: the same answer
    { grp_gzip_walk_step x = e; x.room = g.text_len - 1; forms.push_back({ x, 3 }); }
    for (size_t q = 0; q < forms.size(); ++q) {
      const grp_gzip_walk_step& s = forms[q].s;
      std::vector<char> out((size_t)s.room + 1, 0x55);
      std::vector<uint8_t> h(32768 + 1, 0x55);
      grp_gzip_walk_result r{};
      const InfWalkEntry w{ s, &r, h.data() };
      memset(&g_s, 0xAA, sizeof g_s);
      const uint32_t st = inf_entry(g_s, comp, dict, w, out.data());
      ++*n_steps;
      if (forms[q].kind) ++*n_forms;
      if ((uint8_t)out[s.room] != 0x55 || h[32768] != 0x55) { printf("%s seg %zu form %zu: wrote behind the room or the history\n", path, i, q); ++*bad; }
      if (st != r.status) { printf("%s seg %zu form %zu: the status returned is not the status stored\n", path, i, q); ++*bad; }
      // (a member's last segment may end with blocks without text, which the walk's NEXT step finds: the step then stops in
      // front of them with all of the text, and a step of its own, from there, must end the member without a byte)
      const bool all_text = st == 0 && r.text_len == g.text_len && memcmp(out.data(), text.data() + off, g.text_len) == 0 && crc_member(g_cs, tabs, out.data(), r.text_len) == g.crc32;
      const bool in_front_of_empty_blocks = all_text && (g.flags & 1u) && !r.final && r.bits < g.n_bits && r.bits <= s.n_bits;
      bool whole = all_text && ((r.bits == g.n_bits && r.final == (g.flags & 1u)) || in_front_of_empty_blocks);
      if (whole && in_front_of_empty_blocks && forms[q].kind == 0) {
        std::vector<uint32_t> d2w(32768 / 4 + 3, 0);
        memcpy(d2w.data(), h.data(), r.hist_len);
        std::vector<char> o2(2, 0x55);
        std::vector<uint8_t> h2(32768 + 1, 0x55);
        grp_gzip_walk_result r2{};
        const InfWalkEntry w2{ grp_gzip_walk_step{ g.comp_bit + r.bits, raw.size() * 8 - g.comp_bit - r.bits, 0, r.hist_len, 1, 1, 0 }, &r2, h2.data() };
        const uint32_t st2 = inf_entry(g_s, comp, (const uint8_t*)d2w.data(), w2, o2.data());
        ++*n_steps;
        whole = st2 == 0 && r2.final == 1 && r2.text_len == 0 && r.bits + r2.bits == g.n_bits && r2.hist_len == r.hist_len && memcmp(h2.data(), h.data(), r.hist_len) == 0;
      }
      switch (forms[q].kind) {
        case 0:
          if (!whole) { printf("%s seg %zu form %zu: status %u, the step does not end where the segment ends\n", path, i, q, st); ++*bad; }
          else if (r.hist_len != std::min<uint64_t>(32768, (uint64_t)g.dict_len + g.text_len)) { printf("%s seg %zu: history of %u bytes\n", path, i, r.hist_len); ++*bad; }
          break;
        case 1:
          if (st != 0) ++*n_refused; else if (whole) ++*n_same; else { printf("%s seg %zu form %zu: a shorter history gave another answer\n", path, i, q); ++*bad; }
          break;
        case 2:
          if (st != 0) ++*n_refused;
          else if (in_front_of_empty_blocks) ++*n_same; // (the cut lies in the blocks without text behind it)
          else { printf("%s seg %zu form %zu: fewer bits than the segment has, and the step ended with status 0, %llu bits, %u bytes\n", path, i, q, (unsigned long long)r.bits, r.text_len); ++*bad; }
          break;
        default:
          if (st != INF_NO_ROOM) { printf("%s seg %zu form %zu: a room one byte short gave status %u\n", path, i, q, st); ++*bad; } else ++*n_refused;
      }
    }
  }
}

static int walk_main(int argc, char** argv)
{
  uint64_t n_step_checks = 0, n_step_forms = 0, n_step_refused = 0, n_step_same = 0;
  int bad = 0; uint64_t n_same = 0, n_dmg = 0, n_dmg_left = 0, n_dmg_same = 0, n_repeats = 0;
  gr::GzWalkSizes tiny; tiny.room = 64; tiny.window = 64; tiny.cap = uint64_t(1) << 26;
  const gr::GzWalkSizes sizes[2] = { gr::GzWalkSizes(), tiny };
  char tmp[] = "/tmp/inflate_walk_XXXXXX";
  const int tfd = mkstemp(tmp);
  if (tfd < 0) { printf("no temporary file\n"); return 2; }
  close(tfd);
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { printf("%s: cannot open\n", argv[a]); return 2; }
    std::vector<uint8_t> raw; uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + k);
    fclose(f);
    for (uint64_t span : { uint64_t(1), uint64_t(4096), uint64_t(262144) }) {
      bool failed = false;
      std::unique_ptr<gr::GzIndex> want = reader_index(argv[a], span, &failed);
      if (!want) { printf("%s span %llu: the reader has no index\n", argv[a], (unsigned long long)span); ++bad; continue; }
      for (int z = 0; z < 2; ++z) {
        gr::GzWalkStats st;
        std::vector<gr::GzWalkFile> got = gr::gzip_walk({ argv[a] }, span, uint64_t(1) << 32, sizes[z], walk_launch, &st);
        n_repeats += st.repeats;
        char what[512]; snprintf(what, sizeof what, "%s span %llu sizes %d", argv[a], (unsigned long long)span, z);
        if (!got[0].index) { printf("%s: left to zlib: %s (status %u)\n", what, got[0].left, got[0].status); ++bad; continue; }
        if (!same_index(*want, *got[0].index, what)) { ++bad; continue; }
        ++n_same;
      }
    }
    walk_steps(argv[a], raw, &bad, &n_step_checks, &n_step_forms, &n_step_refused, &n_step_same);
    // damaged copies, at span 4096
    uint64_t r = 0x9e3779b97f4a7c15ull * (uint64_t)(a + 1);
    for (int t = 0; t < 40; ++t) {
      std::vector<uint8_t> d = raw;
      r = r * 6364136223846793005ull + 1442695040888963407ull;
      if (t < 28) { const uint64_t bit = (r >> 20) % (raw.size() * 8); d[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); }
      else if (t < 36) { d.resize((size_t)((r >> 20) % raw.size())); }
      else { d.insert(d.end(), (size_t)(t - 35), (uint8_t)(t == 39 ? 0x1f : 0)); }
      FILE* o = fopen(tmp, "wb");
      if (!o || fwrite(d.data(), 1, d.size(), o) != d.size()) { printf("cannot write %s\n", tmp); return 2; }
      fclose(o);
      ++n_dmg;
      bool failed = false;
      std::unique_ptr<gr::GzIndex> want = reader_index(tmp, 4096, &failed);
      std::vector<gr::GzWalkFile> got = gr::gzip_walk({ tmp }, 4096, uint64_t(1) << 32, sizes[t & 1], walk_launch, nullptr);
      if (!got[0].index) { ++n_dmg_left; continue; }
      char what[512]; snprintf(what, sizeof what, "%s damaged form %d", argv[a], t);
      if (!want || failed) { printf("%s: the walk indexed what the reader %s\n", what, failed ? "refused" : "dropped"); ++bad; continue; }
      if (!same_index(*want, *got[0].index, what)) { ++bad; continue; }
      ++n_dmg_same;
    }
  }
  unlink(tmp);
  if (g_walk_overrun) { printf("%llu steps wrote behind their room or their history\n", (unsigned long long)g_walk_overrun); ++bad; }
  printf("steps: %llu open steps over the reader's segments, %llu damaged forms: %llu refused, %llu gave the segment's text\n", (unsigned long long)n_step_checks, (unsigned long long)n_step_forms, (unsigned long long)n_step_refused,
         (unsigned long long)n_step_same);
  printf("walk: %llu indexes equal the reader's; %llu steps, %llu repeated; %llu damaged files: %llu left to zlib, %llu indexed as the reader does; %d bad\n", (unsigned long long)n_same, (unsigned long long)g_walk_steps,
         (unsigned long long)n_repeats, (unsigned long long)n_dmg, (unsigned long long)n_dmg_left, (unsigned long long)n_dmg_same, bad);
  return bad != 0;
}

// ---- --members ---------------------------------------------------------------------------------------------------------
// The open form from pseudo-random bits of a compressed buffer — what a stream begun at a false candidate gives the decoder.
// The bytes lie in a heap block of exactly their number (a multiple of 4: the decoder loads the words its bits lie in), the
// text goes to a block of exactly `room` bytes, the history comes from and goes to blocks of exactly their sizes: under
// -fsanitize=address a load or store outside any of them ends the program.
static int random_steps(const std::vector<uint8_t>& raw, uint64_t* counts)
{
  const size_t n = raw.size() & ~size_t(3);
  if (n < 64) return 0;
  uint8_t* comp = (uint8_t*)malloc(n);
  memcpy(comp, raw.data(), n);
  int bad = 0;
  uint64_t r = 0x2545f4914f6cdd1dull;
  for (int t = 0; t < 10000; ++t) {
    r = r * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t bit = (r >> 16) % (n * 8);
    r = r * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t left = n * 8 - bit;
    const uint64_t n_bits = (t & 3) == 0 ? (r >> 16) % (left + 1) : left; // to the end of the buffer, or to any bit in front of it
    const uint32_t room = (t & 7) < 3 ? 512u : 1u << 16, dict_len = (t & 1) ? 0u : (uint32_t)((r >> 40) % 32769);
    const uint32_t min_text = (t & 16) ? room / 2 : 1;
    uint8_t* dict = (uint8_t*)malloc(dict_len ? dict_len : 1);
    memset(dict, 'A', dict_len ? dict_len : 1);
    char* out = (char*)malloc(room);
    uint8_t* hist = (uint8_t*)malloc(32768);
    grp_gzip_walk_result res{};
    const InfWalkEntry e{ grp_gzip_walk_step{ bit, n_bits, 0, dict_len, min_text, room, 0 }, &res, hist };
    memset(&g_s, 0xAA, sizeof g_s);
    const uint32_t st = inf_entry(g_s, comp, dict, e, out);
    ++counts[st == 0 ? 0 : st == INF_INPUT_ENDS ? 1 : st == INF_NO_ROOM ? 2 : 3];
    if (st != res.status || (st == 0 && (res.bits == 0 || res.bits > n_bits || res.text_len > room || res.hist_len > 32768 || res.hist_len != std::min<uint64_t>(32768, (uint64_t)dict_len + res.text_len)))) {
      printf("random step %d (bit %llu, %llu bits): status %u, %llu bits, %u bytes, history %u\n", t, (unsigned long long)bit, (unsigned long long)n_bits, st, (unsigned long long)res.bits, res.text_len, res.hist_len);
      ++bad;
    }
    free(hist); free(out); free(dict);
  }
  free(comp);
  return bad;
}

// The members switch of the rounds (csrc/host/gr_gzwalk.hpp: GzWalkMembers) over the host-compiled decoder: all the files in ONE walk,
// with the switch and without it, at spans 1, 50 000 and 10^9; the sizes of a step and the budget of streams come from
// GRP_GZIP_WALK_ROOM and GRP_GZIP_WALK_STREAMS.  A file the serial walk indexes must get the reader's index from both; a file
// it leaves to zlib must be left by both, for the same reason with the same status.  One line of statistics per span (tests/
// test_gzip_members_cpu.py reads them), then the random steps over the first file's bytes.
static int members_main(int argc, char** argv)
{
  int bad = 0;
  gr::GzWalkMembers on = gr::gzip_walk_members();
  on.on = true;
  std::vector<std::string> paths(argv + 2, argv + argc);
  for (uint64_t span : { uint64_t(1), uint64_t(50000), uint64_t(1000000000) }) {
    gr::GzWalkStats s0, s1;
    std::vector<gr::GzWalkFile> off = gr::gzip_walk(paths, span, uint64_t(1) << 32, gr::gzip_walk_sizes(), walk_launch, &s0);
    std::vector<gr::GzWalkFile> got = gr::gzip_walk(paths, span, uint64_t(1) << 32, gr::gzip_walk_sizes(), walk_launch, &s1, nullptr, nullptr, on);
    int span_bad = 0;
    for (size_t i = 0; i < paths.size(); ++i) {
      char what[600]; snprintf(what, sizeof what, "%s span %llu", paths[i].c_str(), (unsigned long long)span);
      if (off[i].index) {
        bool failed = false;
        std::unique_ptr<gr::GzIndex> want = reader_index(paths[i].c_str(), span, &failed);
        if (!want || failed || !same_index(*want, *off[i].index, what)) { printf("%s: the serial walk's index is not the reader's\n", what); ++span_bad; continue; }
        if (!got[i].index) { printf("%s: with the members switch the file is left to zlib: %s (status %u)\n", what, got[i].left, got[i].status); ++span_bad; continue; }
        if (!same_index(*want, *got[i].index, what)) ++span_bad;
      } else if (got[i].index || strcmp(got[i].left, off[i].left) != 0 || got[i].status != off[i].status) {
        printf("%s: left to zlib without the switch (%s, status %u), with it: %s, status %u\n", what, off[i].left, off[i].status, got[i].index ? "indexed" : got[i].left, got[i].status);
        ++span_bad;
      }
    }
    if (s0.candidates || s0.streams || s0.adopted || s0.dropped || s0.max_in_flight || s0.wasted_text) { printf("span %llu: the walk without the switch counts streams\n", (unsigned long long)span); ++span_bad; }
    printf("members: span=%llu files=%llu walked=%llu left_to_zlib=%llu rounds=%llu serial_rounds=%llu text=%llu serial_text=%llu candidates=%llu streams=%llu adopted=%llu dropped=%llu max_in_flight=%llu wasted_text=%llu bad=%d\n",
           (unsigned long long)span, (unsigned long long)s1.files, (unsigned long long)s1.walked, (unsigned long long)s1.left_to_zlib, (unsigned long long)s1.rounds, (unsigned long long)s0.rounds, (unsigned long long)s1.text_bytes,
           (unsigned long long)s0.text_bytes, (unsigned long long)s1.candidates, (unsigned long long)s1.streams, (unsigned long long)s1.adopted, (unsigned long long)s1.dropped, (unsigned long long)s1.max_in_flight,
           (unsigned long long)s1.wasted_text, span_bad);
    bad += span_bad;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) { printf("%s: cannot open\n", argv[2]); return 2; }
  std::vector<uint8_t> raw; uint8_t buf[65536]; size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + k);
  fclose(f);
  uint64_t counts[4] = { 0, 0, 0, 0 };
  bad += random_steps(raw, counts);
  if (g_walk_overrun) { printf("%llu steps wrote behind their room or their history\n", (unsigned long long)g_walk_overrun); ++bad; }
  printf("random: %llu steps ended at a boundary, %llu ran out of input, %llu out of room, %llu were refused; %d bad\n", (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3], bad);
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
  if (argc >= 3 && !strcmp(argv[1], "--walk")) {
    return walk_main(argc, argv);
  }
  if (argc >= 3 && !strcmp(argv[1], "--members")) {
    return members_main(argc, argv);
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
