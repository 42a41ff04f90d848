// Developer check of csrc/host/gr_units.hpp under the sanitizers, without a device and outside Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/dev/units_host_check.cpp -o /tmp/units_host_check && /tmp/units_host_check
// Random files cut into units — empty ones in the middle, at the front and at the end — and random records in them:
// locate_units against a linear search, and the walk gr_writer.cpp's flush makes over its list of pending records (runs of
// records of one file; records of plain files in between are not planned; a compressed file's run goes through plan_fetch
// call after call, under small caps) against the bytes: every record's text must be found at its offset in the
// concatenated text of the units of its call, every unit at most once per call and in file order.
// Then the mapping from a stored record and its decision to what is written of it (written_slice, fetch_record_of): every
// field and the byte count against values written down by hand from include/grpath_ingest.h (grp_fetch_record and the size
// of a record's bytes) — forward and reversed, whole and trimmed, a trim that ends at the last tile, fewer qualities than
// bases and none at the slice, records of no base and of one, FASTA and FASTQ.
#include "../../goldrush_amd/csrc/host/gr_units.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

using namespace gr;

#define CHECK(c)                                                                                                       \
  do {                                                                                                                 \
    if (!(c)) {                                                                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c);                                       \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
  } while (0)

// one case of the mapping: the record at `text_off` of the fetched text, its bytes at out_off 70; `want` in the order of the
// struct's fields from id_len on (out_off and the three text offsets follow from the arguments), and the byte counts
struct SliceCase
{
  uint32_t seq_len, qual_len;
  uint8_t reversed;
  uint32_t kind, trim_start, trim_end, num_tiles;
  uint32_t seq_from, n_seq, qual_from, n_qual, flags;
  uint64_t fasta_bytes, fastq_bytes;
};

static void
check_slices()
{
  // tiles of 10 bases; a record of 47 bases has 4 of them.  id "read1" (5 bytes): '@' id "_untrimmed\n" is 1 + 5 + 11 bytes,
  // "_trimmed\n" 9; then the bases and '\n'; FASTQ: "+\n", the qualities and '\n' more
  const SliceCase cases[] = {
    // forward: whole; tiles 1-2 of 4: bases [10, 30); tiles 2-3, the last tile: to the end, bases [20, 47)
    { 47, 47, 0, 2, 0, 0, 4, /**/ 0, 47, 0, 47, 0, /**/ 65, 115 },
    { 47, 47, 0, 4, 1, 2, 4, /**/ 10, 20, 10, 20, 1, /**/ 36, 59 },
    { 47, 47, 0, 4, 2, 3, 4, /**/ 20, 27, 20, 27, 1, /**/ 43, 73 },
    // reversed: the same slices of the twin are the stored ranges [0, 47), [17, 37), [0, 27), written backwards
    { 47, 47, 1, 2, 0, 0, 4, /**/ 0, 47, 0, 47, 2, /**/ 65, 115 },
    { 47, 47, 1, 4, 1, 2, 4, /**/ 17, 20, 17, 20, 3, /**/ 36, 59 },
    { 47, 47, 1, 4, 2, 3, 4, /**/ 0, 27, 0, 27, 3, /**/ 43, 73 },
    // 25 qualities for 47 bases: whole — all 25; tiles 1-2 — qualities [10, 25), reversed the stored [0, 15)
    { 47, 25, 0, 2, 0, 0, 4, /**/ 0, 47, 0, 25, 0, /**/ 65, 93 },
    { 47, 25, 0, 4, 1, 2, 4, /**/ 10, 20, 10, 15, 1, /**/ 36, 54 },
    { 47, 25, 1, 4, 1, 2, 4, /**/ 17, 20, 0, 15, 3, /**/ 36, 54 },
    // 5 qualities, the slice begins behind them: none, from the end of the qualities (reversed: the stored front)
    { 47, 5, 0, 4, 1, 2, 4, /**/ 10, 20, 5, 0, 1, /**/ 36, 39 },
    { 47, 5, 1, 4, 1, 2, 4, /**/ 17, 20, 0, 0, 3, /**/ 36, 39 },
    { 47, 5, 0, 4, 2, 3, 4, /**/ 20, 27, 5, 0, 1, /**/ 43, 46 },
    // no base; one base
    { 0, 0, 0, 2, 0, 0, 0, /**/ 0, 0, 0, 0, 0, /**/ 18, 21 },
    { 0, 0, 1, 2, 0, 0, 0, /**/ 0, 0, 0, 0, 2, /**/ 18, 21 },
    { 1, 1, 0, 2, 0, 0, 0, /**/ 0, 1, 0, 1, 0, /**/ 19, 23 },
    { 1, 1, 1, 2, 0, 0, 0, /**/ 0, 1, 0, 1, 2, /**/ 19, 23 },
  };
  for (const SliceCase& c : cases) {
    const RecLoc l{ 3, 1000, 5, 6, c.seq_len, 60, c.qual_len, c.reversed };
    const grp_read_decision d{ c.kind, c.num_tiles, 0, c.trim_start, c.trim_end, 0, 0, 0 };
    const WrittenSlice w = written_slice(10, l.seq_len, l.qual_len, d);
    for (int fastq = 0; fastq < 2; ++fastq) {
      uint64_t size = 0;
      const grp_fetch_record r = fetch_record_of(l, w, 300, 70, fastq != 0, &size);
      CHECK(r.id_off == 300 && r.seq_off == 306 && r.qual_off == 360 && r.out_off == 70 && r.id_len == 5);
      CHECK(r.seq_from == c.seq_from && r.n_seq == c.n_seq && r.qual_from == c.qual_from && r.n_qual == c.n_qual && r.flags == c.flags);
      CHECK(size == (fastq ? c.fastq_bytes : c.fasta_bytes));
      // the stored ranges lie inside the record
      CHECK((uint64_t)r.seq_from + r.n_seq <= c.seq_len && (uint64_t)r.qual_from + r.n_qual <= c.qual_len);
    }
  }
}

struct File
{
  std::string text;
  std::vector<uint64_t> text_off; // empty: a plain file
};

int
main()
{
  std::mt19937_64 rng(20260102);
  auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
  size_t n_located = 0, n_calls = 0, n_straddling = 0, n_refused = 0;
  for (int round = 0; round < 300; ++round) {
    // a run's files: some plain, some cut into units
    std::vector<File> files(1 + below(5));
    for (File& f : files) {
      f.text.resize(1 + below(3000));
      for (char& c : f.text) {
        c = (char)('A' + below(26));
      }
      if (below(3) == 0) {
        continue; // plain
      }
      BgzfMap m;
      uint64_t at = 0;
      for (uint64_t e = below(3); e; --e) {
        m.add(0, 0, 0, 0); // empty units at the front
      }
      while (at < f.text.size()) {
        const uint64_t n = below(4) == 0 ? 0 : std::min<uint64_t>(1 + below(round % 2 ? 40 : 700), f.text.size() - at);
        m.add(at, (uint32_t)n, (uint32_t)n, 0);
        at += n;
      }
      for (uint64_t e = below(3); e; --e) {
        m.add(0, 0, 0, 0); // ... and at the end
      }
      CHECK(m.text_off.size() == m.blocks.size() + 1 && m.text_off.back() == f.text.size());
      f.text_off = m.text_off;
    }
    // locate_units against the definition
    for (const File& f : files) {
      if (f.text_off.empty()) {
        continue;
      }
      const size_t n = f.text_off.size() - 1;
      for (int k = 0; k < 200; ++k) {
        const uint64_t off = below(f.text.size() + 3), len = below(4) == 0 ? 0 : below(f.text.size() / 2 + 2);
        UnitRun r;
        const bool ok = locate_units(f.text_off, off, len, r);
        const bool inside = off < f.text.size() && len <= f.text.size() - off;
        CHECK(ok == inside);
        if (!ok) {
          ++n_refused;
          continue;
        }
        ++n_located;
        // the first unit holds `off`, the last the range's last byte; nothing of the range lies outside them
        CHECK(r.first < n && r.count >= 1 && r.first + r.count <= n);
        CHECK(f.text_off[r.first] <= off && off < f.text_off[r.first + 1] && r.inside == off - f.text_off[r.first]);
        const uint64_t last = off + (len ? len - 1 : 0);
        const size_t lu = r.first + r.count - 1;
        CHECK(f.text_off[lu] <= last && last < f.text_off[lu + 1]);
      }
    }
    // the pending list: records in commit order — ascending in a file, the files one after the other, now and then a
    // record of an earlier file (another batch of it)
    struct Rec
    {
      size_t file;
      uint64_t off, len;
    };
    std::vector<Rec> pend;
    for (size_t f = 0; f < files.size(); ++f) {
      uint64_t at = 0;
      while (at < files[f].text.size()) {
        const uint64_t len = 1 + below(300), skip = below(200);
        if (at + skip + len > files[f].text.size()) {
          break;
        }
        pend.push_back(Rec{ f, at + skip, len });
        at += skip + len;
        if (below(40) == 0 && f > 0) {
          pend.push_back(Rec{ f - 1, 0, std::min<uint64_t>(5, files[f - 1].text.size()) });
        }
      }
    }
    const uint64_t text_cap = 200 + below(2000);
    const size_t max_units = 1 + below(30);
    size_t i = 0, n_written = 0;
    FetchPlan pl;
    std::vector<FetchItem> items;
    while (i < pend.size()) {
      const size_t f = pend[i].file;
      size_t e = i + 1;
      while (e < pend.size() && pend[e].file == f) {
        ++e;
      }
      if (files[f].text_off.empty()) { // plain: read back one by one
        n_written += e - i;
        i = e;
        continue;
      }
      while (i < e) {
        items.clear();
        for (size_t j = i; j < e; ++j) {
          items.push_back(FetchItem{ pend[j].off, pend[j].len });
        }
        CHECK(plan_fetch(files[f].text_off, items.data(), items.size(), text_cap, max_units, pl));
        CHECK(pl.n_recs >= 1 && pl.n_recs <= e - i && pl.rec_text_off.size() == pl.n_recs);
        CHECK(pl.n_recs == 1 || (pl.text_bytes <= text_cap && pl.units.size() <= max_units));
        std::string cat;
        for (size_t k = 0; k < pl.units.size(); ++k) {
          CHECK(k == 0 || pl.units[k] > pl.units[k - 1]);
          const size_t u = pl.units[k];
          cat.append(files[f].text, (size_t)files[f].text_off[u], (size_t)(files[f].text_off[u + 1] - files[f].text_off[u]));
        }
        CHECK(cat.size() == pl.text_bytes);
        for (size_t j = 0; j < pl.n_recs; ++j) {
          const Rec& r = pend[i + j];
          CHECK(pl.rec_text_off[j] + r.len <= cat.size());
          CHECK(cat.compare((size_t)pl.rec_text_off[j], (size_t)r.len, files[f].text, (size_t)r.off, (size_t)r.len) == 0);
        }
        n_straddling += pl.straddling;
        n_written += pl.n_recs;
        i += pl.n_recs;
        ++n_calls;
      }
    }
    CHECK(n_written == pend.size());
    // a record outside the text is refused, and named by the plan that would begin with it
    for (const File& f : files) {
      if (!f.text_off.empty()) {
        const FetchItem bad[2] = { { 0, 1 }, { f.text.size(), 1 } };
        CHECK(plan_fetch(f.text_off, bad, 2, 1 << 20, 100, pl) && pl.n_recs == 1);
        CHECK(!plan_fetch(f.text_off, bad + 1, 1, 1 << 20, 100, pl));
      }
    }
  }
  CHECK(n_located > 10000 && n_calls > 1000 && n_straddling > 1000 && n_refused > 100);
  check_slices();
  std::printf("units_host_check ok: %zu ranges located, %zu refused, %zu fetch calls planned, %zu records in two or more units\n", n_located, n_refused, n_calls, n_straddling);
  return 0;
}
