// Stand-alone check of the BAM record layer (csrc/host/gr_bam.hpp: the header function, the shared walk, the decoder) for
// the sanitizers: good streams, every truncation of one and single-byte damages of another, each in a heap buffer of
// exactly its size, so that a read behind the end is seen.  Every input is either refused or walked to records that lie
// inside the buffer, and every record the walk hands out is decoded.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/dev/bam_host_check.cpp goldrush_amd/csrc/host/gr_bam.cpp -o /tmp/bam_host_check && /tmp/bam_host_check
#include "../../include/grpath_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

typedef std::vector<unsigned char> Bytes;

static void
put32(Bytes& b, uint32_t v)
{
  for (int i = 0; i < 4; ++i) {
    b.push_back((unsigned char)(v >> (8 * i)));
  }
}

static Bytes
header(size_t l_text, unsigned n_ref)
{
  Bytes h = { 'B', 'A', 'M', 1 };
  put32(h, (uint32_t)l_text);
  h.resize(h.size() + l_text, 'h');
  put32(h, n_ref);
  for (unsigned r = 0; r < n_ref; ++r) {
    put32(h, 3 + r);
    h.resize(h.size() + 2 + r, 'r');
    h.push_back(0);
    put32(h, 1000);
  }
  return h;
}

static Bytes
record(const std::string& name, size_t l_seq, unsigned n_cigar, size_t n_tags, unsigned flag, std::mt19937& rng)
{
  Bytes body;
  put32(body, 0xffffffffu); // refID
  put32(body, 0xffffffffu); // pos
  body.push_back((unsigned char)(name.size() + 1));
  body.push_back(0);
  body.push_back(0x48), body.push_back(0x12); // bin
  body.push_back((unsigned char)(n_cigar & 255)), body.push_back((unsigned char)(n_cigar >> 8));
  body.push_back((unsigned char)(flag & 255)), body.push_back((unsigned char)(flag >> 8));
  put32(body, (uint32_t)l_seq);
  put32(body, 0xffffffffu), put32(body, 0xffffffffu), put32(body, 0);
  body.insert(body.end(), name.begin(), name.end());
  body.push_back(0);
  for (unsigned c = 0; c < n_cigar; ++c) {
    put32(body, 16 * (c + 1));
  }
  for (size_t i = 0; i < (l_seq + 1) / 2; ++i) {
    body.push_back((unsigned char)rng());
  }
  for (size_t i = 0; i < l_seq; ++i) {
    body.push_back((unsigned char)(rng() % 94));
  }
  for (size_t i = 0; i < n_tags; ++i) {
    body.push_back((unsigned char)rng());
  }
  Bytes rec;
  put32(rec, (uint32_t)body.size());
  rec.insert(rec.end(), body.begin(), body.end());
  return rec;
}

static unsigned long n_walks = 0, n_refused = 0, n_records = 0;

// header + walk + decode on a copy of exactly n bytes; what they return must lie inside them
static void
check(const unsigned char* src, size_t n, int final_chunk)
{
  unsigned char* buf = (unsigned char*)malloc(n ? n : 1);
  if (n) {
    memcpy(buf, src, n);
  }
  uint64_t hb = ~0ull;
  const int hrc = gr_bam_header(buf, n, &hb);
  if (hrc < -1 || hrc > 1 || (hrc == 1 && hb > n)) {
    fprintf(stderr, "bad header result: n=%zu -> %d, %llu\n", n, hrc, (unsigned long long)hb);
    exit(1);
  }
  if (hrc == 1) {
    const unsigned char* body = buf + hb;
    const uint64_t nb = n - hb;
    std::vector<gr_bam_record> recs(64);
    uint64_t n_rec = ~0ull, used = ~0ull, bad = ~0ull;
    const char* why = nullptr;
    const int rc = gr_bam_walk(body, nb, final_chunk, recs.data(), recs.size(), &n_rec, &used, &bad, &why);
    ++n_walks;
    bool ok = (rc == 0 || rc == -1) && used <= nb && n_rec <= recs.size() && (rc == 0 || (why && bad <= nb && bad == used));
    uint64_t end = 0;
    std::vector<char> seq, qual;
    for (uint64_t i = 0; ok && i < n_rec; ++i) {
      const gr_bam_record& r = recs[i];
      ok = r.off == end && r.name_off == r.off + 36 && r.l_read_name >= 1 && r.id_len < r.l_read_name && r.name_off + r.l_read_name <= r.seq_off &&
           r.seq_off + ((uint64_t)r.l_seq + 1) / 2 == r.qual_off && r.qual_off + r.l_seq <= r.end && r.end <= used && !(r.flag & 0x910);
      end = r.end;
      if (ok) {
        seq.assign(r.l_seq + 1, 0), qual.assign(r.l_seq + 1, 0);
        (void)gr_bam_decode(body, &r, seq.data(), qual.data());
        ++n_records;
      }
    }
    ok = ok && end == used && (rc != 0 || !final_chunk || used == nb);
    if (!ok) {
      fprintf(stderr, "bad walk result: n=%zu final=%d -> rc %d, %llu records, consumed %llu, bad %llu\n", n, final_chunk, rc, (unsigned long long)n_rec, (unsigned long long)used,
              (unsigned long long)bad);
      exit(1);
    }
    n_refused += rc != 0;
  }
  free(buf);
}

int
main()
{
  std::mt19937 rng(7);
  // good streams
  for (size_t l_text : { (size_t)0, (size_t)33, (size_t)200000 }) {
    for (unsigned n_ref : { 0u, 3u }) {
      Bytes f = header(l_text, n_ref);
      for (size_t l_seq : { (size_t)0, (size_t)1, (size_t)2, (size_t)15, (size_t)16, (size_t)17, (size_t)33, (size_t)500 }) {
        const Bytes r = record(std::string(1 + l_seq % 40, 'n'), l_seq, (unsigned)(l_seq % 4), l_seq % 7 * 50, 4, rng);
        f.insert(f.end(), r.begin(), r.end());
      }
      check(f.data(), f.size(), 1);
      check(f.data(), f.size(), 0);
    }
  }
  // every truncation of one
  Bytes small = header(5, 1);
  for (size_t l_seq : { (size_t)0, (size_t)7, (size_t)40 }) {
    const Bytes r = record("name with blank", l_seq, 2, 9, 77, rng);
    small.insert(small.end(), r.begin(), r.end());
  }
  for (size_t n = 0; n <= small.size(); ++n) {
    check(small.data(), n, 0);
    check(small.data(), n, 1);
  }
  // single-byte damages of another: every byte of the header and of the records' fixed parts and names with a few values,
  // and a few thousand random ones
  for (size_t i = 0; i < small.size(); ++i) {
    for (unsigned v : { 0u, 1u, 0x10u, 0x7fu, 0x80u, 0xffu }) {
      Bytes f = small;
      f[i] = (unsigned char)v;
      check(f.data(), f.size(), 1);
    }
  }
  for (int t = 0; t < 5000; ++t) {
    Bytes f = small;
    f[rng() % f.size()] = (unsigned char)rng();
    const size_t n = (t & 3) ? f.size() : rng() % (f.size() + 1);
    check(f.data(), n, t & 1);
  }
  printf("gr_bam: %lu walks (%lu refused), %lu records decoded, all results inside their buffers\n", n_walks, n_refused, n_records);
  return 0;
}
