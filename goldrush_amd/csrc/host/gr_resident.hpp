// Reads kept on the device between the passes (round 3).
// The reference reads its input three times (Phred median, fill, classification:
// goldrush_path.cpp:79-107, 235-339, 1210-1256).  Here the fill pass is the only full parse:
// the packed reads it uploads stay in HBM (2 bits per base: 62.5 GB for C2's 10 M reads) and
// the classification pass runs over those batches; the text of a read that is written out
// (an inserted read) is fetched from the input file by offset.  Plain, seekable input without
// a -f list only (gzip / pipes / --debug take the two-pass form); GRP_RESIDENT=off switches it
// off, GRP_RESIDENT_MAX_GB caps the packed bytes kept (default 100).  GRP_RESIDENT=all: BGZF, indexed gzip and BAM inputs
// stay too, their written records are fetched through the units that hold them (gr_writer.hpp: Deferred).
#pragma once
#include "gr_source.hpp"

#include <algorithm>
#include <unistd.h>

namespace gr {

struct ResidentBatch
{
  void* reads = nullptr;
  std::vector<uint32_t> lens, skipped_before;
  uint32_t skipped_after = 0;
  std::vector<RecLoc> loc;         // (gr_units.hpp)
  std::vector<uint64_t> name_hash; // FNV-1a of the id: candidates for filter_out_reads (names are compared through the file ...
  std::string ids;                 // ... or, the records of a compressed file, here: their ids one after the other,
  std::vector<uint64_t> id_at;     //     read i's at ids[id_at[i]], loc[i].id_len long)
};

inline uint64_t
fnv1a(const char* p, size_t n)
{
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) {
    h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
  }
  return h;
}

// the record at `l`, whose id lies at text[t0], as a record of a batch with that text
inline Rec
rec_of(const RecLoc& l, size_t t0)
{
  return Rec{ t0, l.id_len, t0 + l.seq_rel, l.seq_len, t0 + (size_t)l.qual_rel, l.qual_len, l.reversed != 0 };
}

struct Resident
{
  bool on = false;
  uint64_t packed_bytes = 0, max_bytes = 0;
  std::vector<ResidentBatch> batches;
  // GRP_RESIDENT=all: files that are not plain may stay too.  Per file: how its records are read back — PLAIN by pread;
  // the members of a BGZF file or the segments of a gzip file's index through the fetch (UNKNOWN until the fill pass has
  // read the file to its end: resolve_units) — and whether its text is BAM records
  bool all = false;
  enum Kind : uint8_t { PLAIN = 0, BGZF = 1, GZIP = 2, UNKNOWN = 3 };
  std::vector<uint8_t> kind, bam;
  std::vector<std::vector<uint64_t>> gz_text_off; // a GZIP file: the running text offset of its index's segments (n + 1)
  static constexpr uint64_t kTextCap = 64ull << 20; // text of the units of one fetch call (a file with a larger unit is not resident)
  bool any_compressed() const { return std::any_of(kind.begin(), kind.end(), [](uint8_t k) { return k != PLAIN; }); }
  // GRP_RESIDENT / GRP_RESIDENT_MAX_GB, in front of the fill pass: on, if every input is a plain seekable file — else the
  // whole run takes the two-pass form; GRP_RESIDENT=all: or a file of gzip members, whose records can be fetched through
  // its BGZF members or the segments of its gzip index
  void decide(const PathRun& run);
  // ... and gave up (the run goes on in the two-pass form): the line that says why
  void say_dropped(const PathRun& run, const std::string& why, const std::string& file = std::string()) const
  {
    if (all && run.rank == 0) {
      std::cerr << "GRP_RESIDENT=all: the reads are not kept on the device" << (file.empty() ? "" : " (" + file + ")") << ": " << why << std::endl;
    }
  }
  // Behind the fill pass: the units of every compressed file, as the pass left them in the run.  false (the reads are
  // dropped, the run goes on in two passes): a file without them — a BGZF file that fell over to zlib at a member that is
  // not BGZF, a gzip file whose index was not built, was dropped or is not complete — or with a unit larger than a fetch takes,
  // or an engine without the entry point that inflates them.
  bool resolve_units(PathRun& run);
  // The files the records are read back from, opened when a record of theirs is asked for: at most kMaxOpen descriptors at
  // once (a run may have more files than a process may have descriptors; at the limit all are closed and opened again as
  // they are asked for — the records come file after file).
  static constexpr size_t kMaxOpen = 64;
  std::vector<int> fds; // per file, -1: not open
  size_t n_open = 0;
  int fd_of(const PathRun& run, uint32_t file); // -1: the file cannot be opened (any more)
  void close_files()
  {
    for (int& fd : fds) {
      if (fd >= 0) {
        close(fd);
        fd = -1;
      }
    }
    n_open = 0;
  }
  void drop(PathRun& run)
  {
    for (ResidentBatch& rb : batches) {
      if (rb.reads) {
        run.vt.reads_free(rb.reads);
      }
    }
    batches.clear();
    on = false;
  }
};

} // namespace gr
