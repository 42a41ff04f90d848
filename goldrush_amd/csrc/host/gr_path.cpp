// goldrush-path as a function: main() of goldrush_path/goldrush_path.cpp:1096-1275
// with the miBF work going through the engine ABI (grpath.h) instead of
// MIBloomFilter / MIBFConstructSupport / multiLensfrHashIterator.
//
// Same flags, same stderr messages, same output files (<prefix>_<n>.fq in
// --silver_path mode, <prefix>.fa otherwise), same exit codes.
#include "../../../include/grpath_host.h"
#include "gr_classifier.hpp"
#include "gr_fastq.hpp"
#include "gr_opts.hpp"
#include "gr_params.hpp"
#include "gr_source.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <deque>
#include <cstddef>
#include <cstring>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <memory>
#include <unordered_set>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#if defined(_OPENMP)
#include <omp.h>
#endif

namespace gr {
namespace {

// goldrush_path.cpp:1109-1112 -> calc_ntcard_genome_size (ntcard.hpp:248-275): the
// hash stream of EVERY record (no read filter) sampled on the device; the host only
// turns the zero-bucket counts into F0.  Returns -1 to continue.
int
calc_ntcard_genome_size(PathRun& run, uint64_t& genome_size)
{
  const Opts& opt = run.opt;
  // windows are counted with the seeds' own spans: seed s spans span0 + s, span0 = k, or k - 1 at odd k (make_seed_pattern)
  const unsigned s0 = (unsigned)run.seeds[0].size(), h = (unsigned)opt.hash_num;
  std::cerr << "Calculating expected entries" << std::endl;
  const double s_time = now_s();
  uint64_t input_bytes = 0; // (several files: the tables are sized from the sum of their sizes)
  for (const std::string& path : run.files) {
    std::ifstream in(path, std::ifstream::ate | std::ifstream::binary); // getInf (:44-49)
    if (in) {
      input_bytes += (uint64_t)in.tellg();
    }
  }
  const unsigned sbits = ntcard_sbits(input_bytes);
  if (run.vt.ntcard_begin(run.ctx, sbits) != GRP_OK) {
    return run.fail_engine("ntcard tables");
  }
  auto src = open_source(run);
  Batch b;
  std::vector<uint32_t> sel, lens, extra, run_extra, packed;
  std::vector<uint64_t> word_off;
  std::vector<std::pair<size_t, size_t>> runs;
  std::string bam_seq; // a BAM record with other codes than A, C, G, T, as text
  // (another format fails in fill_bit_vector, as in the reference; nothing is counted here)
  const bool readable = src->ok() && src->is_fastq();
  while (readable && src->next(b)) {
    src->stats(b, 0, true);
    sel.clear();
    // records with other characters go in as their ACGT runs (rare: host packing)
    lens.clear();
    extra.clear();
    word_off.assign(1, 0);
    packed.clear();
    for (size_t i = 0; i < b.rec.size(); ++i) {
      if (!b.non_acgt[i]) {
        if (b.rec[i].seq_len >= s0) {
          sel.push_back((uint32_t)i);
        }
        continue;
      }
      const char* seq = b.seq_text(b.rec[i], 0, b.rec[i].seq_len, bam_seq);
      ntcard_split(seq, b.rec[i].seq_len, s0, h, runs, run_extra);
      for (size_t r = 0; r < runs.size(); ++r) {
        const size_t w0 = packed.size();
        packed.resize(w0 + (runs[r].second + 15) / 16);
        pack_2bit(seq + runs[r].first, runs[r].second, packed.data() + w0);
        lens.push_back((uint32_t)runs[r].second);
        word_off.push_back(packed.size());
      }
      extra.insert(extra.end(), run_extra.begin(), run_extra.end());
    }
    if (!lens.empty()) {
      void* hr = nullptr;
      if (packed.empty()) {
        packed.push_back(0);
      }
      if (run.vt.reads_upload(run.ctx, packed.data(), word_off.data(), lens.data(), (uint32_t)lens.size(), &hr) != GRP_OK) {
        return run.fail_engine("uploading reads");
      }
      const int rc = run.vt.ntcard_add(run.ctx, hr, 0, (uint32_t)lens.size(), extra.data());
      run.vt.reads_free(hr);
      if (rc != GRP_OK) {
        return run.fail_engine("ntcard");
      }
    }
    if (!sel.empty()) {
      void* hr = nullptr;
      if (src->upload(b, sel, lens, &hr) != GRP_OK) {
        return run.fail_engine("uploading reads");
      }
      // stRead (:96-112): multiLensfrHashIterator over the whole sequence, ntComp per seed
      const int rc = run.vt.ntcard_add(run.ctx, hr, 0, (uint32_t)sel.size(), nullptr);
      run.vt.reads_free(hr);
      if (rc != GRP_OK) {
        return run.fail_engine("ntcard");
      }
    }
  }
  std::vector<uint64_t> zeros((size_t)h * 2, 0);
  if (run.vt.ntcard_finish(run.ctx, zeros.data()) != GRP_OK) {
    return run.fail_engine("ntcard");
  }
  std::cerr << "Reapeat profile estimated using ntCard in (sec): " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  // (setprecision(4) << fixed stay set on std::cerr, as in the reference: the banner
  // below prints "occupancy: 0.1000" after an ntcard pass)
  genome_size = 0;
  for (unsigned i = 0; i < h; ++i) {
    const uint64_t f0 = ntcard_f0(zeros[2 * i], zeros[2 * i + 1], sbits);
    std::cerr << "Expected entries for seed pattern " << run.seeds[i] << " : " << f0 << std::endl;
    genome_size += f0;
  }
  std::cerr << "Total expected entries for seed patterns: " << genome_size << std::endl;
  return -1;
}

// goldrush_path.cpp:79-107.  Deterministic form of the OpenMP loop: the first
// 50000 eligible reads in file order fill the sample; every one of the `jobs`
// threads performs one more fetch_add before it breaks, which only moves the
// median index (calc_median takes vec[n/2] of the descending sort).
int
calc_min_phred_threshold(PathRun& run)
{
  constexpr size_t MEDIAN_SAMPLES_NEEDED = 50000;
  constexpr uint32_t MINIMUM_PHRED_THRESHOLD = 10;
  Opts& opt = run.opt;
  if (opt.phred_min != 0) {
    return -1;
  }
  std::cerr << "Calculating minimum phred score via median" << std::endl;
  std::vector<uint32_t> scores(MEDIAN_SAMPLES_NEEDED, 0);
  size_t taken = 0, over = 0;
  auto src = open_source(run);
  Batch b;
  bool done = false;
  while (!done && src->ok() && src->next(b)) {
    src->stats(b, opt.min_length, false);
    for (size_t i = 0; i < b.rec.size(); ++i) {
      if (b.rec[i].seq_len < opt.min_length) {
        continue;
      }
      if (taken >= MEDIAN_SAMPLES_NEEDED) {
        if (++over >= opt.jobs) {
          done = true;
          break;
        }
        continue;
      }
      scores[taken++] = b.avg[i];
    }
  }
  const size_t n = taken + over;
  std::sort(scores.begin(), scores.end(), std::greater<uint32_t>());
  opt.phred_min = std::max(MINIMUM_PHRED_THRESHOLD, scores[n / 2]);
  if (opt.debug) { // log_phred_calculations (:60-70)
    std::cerr << "Number of reads used to calculate median: " << n << std::endl;
    std::cerr << "Median array: ";
    for (const uint32_t v : scores) {
      std::cerr << v << " ";
    }
    std::cerr << std::endl;
  }
  if (opt.verbose) {
    std::cerr << "Minimum phred score calculated with median: " << opt.phred_min << std::endl;
  }
  return -1;
}

// goldrush_path.cpp:235-339
// ---- reads kept on the device between the passes (round 3) -----------------------
// The reference reads its input three times (Phred median, fill, classification:
// goldrush_path.cpp:79-107, 235-339, 1210-1256).  Here the fill pass is the only full parse:
// the packed reads it uploads stay in HBM (2 bits per base: 62.5 GB for C2's 10 M reads) and
// the classification pass runs over those batches; the text of a read that is written out
// (an inserted read) is fetched from the input file by offset.  Plain, seekable input without
// a -f list only (gzip / pipes / --debug take the two-pass form); GRP_RESIDENT=off switches it
// off, GRP_RESIDENT_MAX_GB caps the packed bytes kept (default 100).  GRP_RESIDENT=all: BGZF, indexed gzip and BAM inputs
// stay too, their written records are fetched through the units that hold them (below: Deferred).
struct RecLoc
{
  uint32_t file;    // which of the run's files
  uint64_t off;     // offset of the record's id in that file
  uint32_t id_len;
  uint32_t seq_rel; // seq / qual relative to `off`
  uint32_t seq_len;
  uint64_t qual_rel;
  uint32_t qual_len;
  uint8_t reversed; // a reverse-strand record of an aligned BAM file: written backwards (seq_rel / qual_rel: the stored bytes)
};

struct ResidentBatch
{
  void* reads = nullptr;
  std::vector<uint32_t> lens, skipped_before;
  uint32_t skipped_after = 0;
  std::vector<RecLoc> loc;
  std::vector<uint64_t> name_hash; // FNV-1a of the id: candidates for filter_out_reads (names are compared through the file ...
  std::string ids;                 // ... or, the records of a compressed file, here: their ids one after the other,
  std::vector<uint64_t> id_at;     //     read i's at ids[id_at[i]], loc[i].id_len long)
};

uint64_t
fnv1a(const char* p, size_t n)
{
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) {
    h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
  }
  return h;
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
  bool any_compressed() const { return std::any_of(kind.begin(), kind.end(), [](uint8_t k) { return k != PLAIN; }); }
  // ... and gave up (the run goes on in the two-pass form): the line that says why
  void say_dropped(const PathRun& run, const std::string& why, const std::string& file = std::string()) const
  {
    if (all && run.rank == 0) {
      std::cerr << "GRP_RESIDENT=all: the reads are not kept on the device" << (file.empty() ? "" : " (" + file + ")") << ": " << why << std::endl;
    }
  }
  // The files the records are read back from: at most kMaxOpen descriptors at once, the others opened when a record of
  // theirs is asked for (the one used longest ago makes room).
  static constexpr size_t kMaxOpen = 64;
  struct Open
  {
    uint32_t file;
    int fd;
    uint64_t used;
  };
  std::vector<Open> open_fds;
  uint64_t clock = 0;
  int fd_of(const PathRun& run, uint32_t file) // -1: the file cannot be opened (any more)
  {
    size_t oldest = 0;
    for (size_t i = 0; i < open_fds.size(); ++i) {
      if (open_fds[i].file == file) {
        open_fds[i].used = ++clock;
        return open_fds[i].fd;
      }
      if (open_fds[i].used < open_fds[oldest].used) {
        oldest = i;
      }
    }
    const int fd = open(run.files[file].c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
      return -1;
    }
    if (open_fds.size() < kMaxOpen) {
      open_fds.push_back(Open{ file, fd, ++clock });
    } else {
      close(open_fds[oldest].fd);
      open_fds[oldest] = Open{ file, fd, ++clock };
    }
    return fd;
  }
  void close_files()
  {
    for (const Open& o : open_fds) {
      close(o.fd);
    }
    open_fds.clear();
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

struct SinkState;

// The insert commits of a resident run with compressed inputs, written in batches (below: "the written records of
// compressed inputs")
struct Deferred
{
  struct Pending
  {
    RecLoc loc;
    uint32_t kind, trim_start, trim_end, num_tiles;
  };
  static constexpr uint64_t kTextCap = 64ull << 20; // text of the units of one fetch call (a file with a larger unit is not resident)
  static constexpr size_t kMaxUnits = size_t(1) << 20;
  std::vector<Pending> pend; // in commit order
  std::deque<double> sums;   // of the records written, not yet asked for by the settle hook
  void flush(SinkState& st);
  bool fetch_some(SinkState& st, size_t& i, size_t e);
  // GRP_TRACE_INGEST
  uint64_t n_flushes = 0, n_units_inflated = 0, n_text_bytes = 0, n_records = 0, n_trimmed = 0, n_straddling = 0, n_out_bytes = 0;

private:
  std::vector<FetchItem> items;
  FetchPlan plan;
  std::vector<uint8_t> comp, dict;
  std::vector<grp_bgzf_block> blocks;
  std::vector<grp_gzip_segment> segs;
  std::vector<grp_fetch_record> recs;
  std::vector<char> out, text;
  std::vector<double> got_sums;
};

// plain regular file (no gzip magic) whose records can be read back with pread?  `may_be_empty`: one of several files
// may hold no byte (no record is ever read back from it).
bool
is_plain_input(const std::string& path, bool may_be_empty)
{
  const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    return false;
  }
  struct stat st;
  unsigned char magic[4] = { 0, 0, 0, 0 }; // (gzip data, or BAM that is not compressed: records are not text to read back)
  bool plain = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
  if (plain && !(may_be_empty && st.st_size == 0)) {
    plain = !(pread(fd, magic, 4, 0) < 2 || (magic[0] == 0x1f && magic[1] == 0x8b) || !memcmp(magic, "BAM\1", 4));
  }
  close(fd);
  return plain;
}

// GRP_RESIDENT=all, a file that is not plain: could its records be fetched through inflatable units?  A regular file of
// gzip members (BGZF among them); whether its units are known is seen behind the fill pass (resolve_units).  Else why not.
bool
compressed_candidate(const std::string& path, std::string& why)
{
  const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    why = "it cannot be opened";
    return false;
  }
  struct stat st;
  unsigned char magic[4] = { 0, 0, 0, 0 };
  const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
  const ssize_t k = regular ? pread(fd, magic, 4, 0) : 0;
  close(fd);
  if (!regular) {
    why = "it is no regular file";
  } else if (k == 4 && !memcmp(magic, "BAM\1", 4)) {
    why = "it is an uncompressed BAM file";
  } else if (!(k >= 2 && magic[0] == 0x1f && magic[1] == 0x8b)) {
    why = "it is neither plain FASTQ nor gzip data";
  }
  return why.empty();
}

// Behind the fill pass: the units of every compressed file, as the pass left them in the run.  false (the reads are
// dropped, the run goes on in two passes): a file without them — a BGZF file that fell over to zlib at a member that is
// not BGZF, a gzip file whose index was not built, was dropped or is not complete — or with a unit larger than a fetch takes,
// or an engine without the entry point that inflates them.
bool
resolve_units(PathRun& run, Resident& res)
{
  res.gz_text_off.assign(run.files.size(), std::vector<uint64_t>());
  for (size_t f = 0; f < run.files.size(); ++f) {
    if (res.kind[f] != Resident::UNKNOWN) {
      continue;
    }
    std::string why;
    if (run.bgzf_map[f]) {
      res.kind[f] = Resident::BGZF;
      if (!run.ext.records_fetch && !run.ext.bgzf_inflate) {
        why = "the engine cannot inflate BGZF members";
      }
    } else if (run.gzidx[f] && run.gzidx[f]->matches(run.files[f])) {
      res.kind[f] = Resident::GZIP;
      const GzIndex& ix = *run.gzidx[f];
      std::vector<uint64_t>& toff = res.gz_text_off[f];
      toff.assign(1, 0);
      for (const GzSegment& g : ix.segs) {
        toff.push_back(toff.back() + g.text_len);
      }
      if (!run.ext.records_fetch && !run.ext.gzip_inflate) {
        why = "the engine cannot inflate gzip segments";
      } else if (ix.max_text > Deferred::kTextCap) {
        why = "a segment of its index holds more text (" + std::to_string(ix.max_text) + " bytes) than a fetch takes";
      }
    } else {
      why = "the fill pass left neither a table of its BGZF members (a member that is not BGZF hands the file to zlib) nor a complete gzip index (GRP_GZIP_INDEX=off, dropped at GRP_GZIP_INDEX_MAX_GB, bytes behind the last member)";
    }
    if (!why.empty()) {
      res.say_dropped(run, why, run.files[f]);
      res.drop(run);
      return false;
    }
  }
  return true;
}

int
fill_bit_vector(PathRun& run, Resident& res)
{
  const Opts& opt = run.opt;
  std::cerr << "inserting bit vector" << std::endl;
  const double s_time = now_s();
  auto src = open_source(run);
  if (!src->ok() || !src->is_fastq()) {
    std::cerr << "Gold Path requires fastq format" << std::endl;
    return 1;
  }
  size_t num_reads = 0, num_passed_reads = 0, by_phred = 0, by_delta = 0, by_length = 0, by_bases = 0;
  Batch b;
  void* prev = nullptr;
  std::vector<uint32_t> sel, lens;
  uint32_t lead_skipped = 0;
  uint64_t n_batches = 0;
  // developer trace (GRP_TRACE_INGEST): where the host's time of this pass goes, per call site
  static const bool trace = getenv("GRP_TRACE_INGEST") != nullptr;
  double t_next = 0, t_filter = 0, t_upload = 0, t_fill = 0, t_keep = 0;
  for (;;) {
    const double tn0 = trace ? now_s() : 0.0;
    if (!src->next(b)) {
      break;
    }
    const double tn1 = trace ? now_s() : 0.0;
    t_next += tn1 - tn0;
    src->stats(b, opt.min_length, true);
    sel.clear();
    ResidentBatch keep;
    uint32_t skipped = 0;
    for (size_t i = 0; i < b.rec.size(); ++i) {
      ++num_reads;
      ++skipped; // (taken back below when the record is selected)
      if (b.rec[i].seq_len < opt.min_length) { // :261-265
        ++by_length;
        continue;
      }
      if (opt.debug) { // :267-273 (file order here; the reference prints from an OpenMP region)
        std::cerr << "phred avg: " << b.avg[i] << "\n"
                  << "phred delta: " << b.delta[i] << std::endl;
      }
      const bool low = b.avg[i] < opt.phred_min, hairpin = b.delta[i] >= opt.phred_delta;
      if (low || hairpin) { // :275-292
        if (opt.verbose) {
          by_phred += low ? 1 : 0;
          by_delta += hairpin ? 1 : 0;
        }
        run.filter_out_reads.insert(b.id_str(i));
        continue;
      }
      if (b.non_acgt[i]) { // :293-301
        ++by_bases;
        run.filter_out_reads.insert(b.id_str(i));
        continue;
      }
      ++num_passed_reads;
      sel.push_back((uint32_t)i);
      if (res.on) {
        // what the classification pass needs of this read: it is classified iff it is long enough and
        // not in filter_out_reads (read_hashing.cpp:35-42) — without a -f list exactly the reads selected here
        const Rec& r = b.rec[i];
        keep.skipped_before.push_back(skipped - 1);
        keep.loc.push_back(RecLoc{ (uint32_t)b.file, b.base_off + r.id_off, (uint32_t)r.id_len, (uint32_t)(r.seq_off - r.id_off), (uint32_t)r.seq_len, (uint64_t)(r.qual_off - r.id_off), (uint32_t)r.qual_len, (uint8_t)(r.reversed ? 1 : 0) });
        keep.name_hash.push_back(fnv1a(b.text + r.id_off, r.id_len));
        res.bam[b.file] = b.bam ? 1 : 0;
        if (res.kind[b.file] != Resident::PLAIN) { // (no pread finds this id again)
          keep.id_at.resize(keep.loc.size(), 0);
          keep.id_at.back() = keep.ids.size();
          keep.ids.append(b.text + r.id_off, r.id_len);
        }
      }
      skipped = 0;
    }
    if (res.on && sel.empty() && !res.batches.empty()) {
      res.batches.back().skipped_after += skipped; // a batch without a single selected read
      skipped = 0;
    }
    const double tf1 = trace ? now_s() : 0.0;
    t_filter += tf1 - tn1;
    if (!sel.empty()) {
      void* h = nullptr;
      if (src->upload(b, sel, lens, &h) != GRP_OK) {
        return run.fail_engine("uploading reads");
      }
      const double tu1 = trace ? now_s() : 0.0;
      t_upload += tu1 - tf1;
      if (prev) {
        run.vt.reads_free(prev); // waits for the previous batch's kernel
        prev = nullptr;
      }
      // multiLensfrHashIterator itr(record.seq, seeds); miBFCS.insertBV(itr)  (:304-305)
      static const bool trace_nofill = trace && getenv("GRP_TRACE_NOFILL") != nullptr; // developer: the pass without its fill kernels (timing only: the filter stays empty)
      const bool mine = !trace_nofill && (!run.shard_fill || (n_batches % run.world) == run.rank);
      ++n_batches;
      if (mine && run.vt.bv_insert(run.ctx, h, 0, (uint32_t)sel.size()) != GRP_OK) {
        return run.fail_engine("bit-vector insert");
      }
      const double tb1 = trace ? now_s() : 0.0;
      t_fill += tb1 - tu1;
      if (res.on) {
        for (uint32_t l : lens) {
          res.packed_bytes += ((uint64_t)l + 15) / 16 * 4;
        }
        if (res.packed_bytes > res.max_bytes) {
          res.say_dropped(run, "the packed reads exceed GRP_RESIDENT_MAX_GB", run.files[b.file]);
          res.drop(run); // too much to keep: the classification pass parses the input again
          prev = h;
        } else {
          keep.reads = h;
          keep.lens = lens;
          keep.skipped_after = skipped;
          res.batches.push_back(std::move(keep));
        }
      } else {
        prev = h;
      }
    } else if (res.on && res.batches.empty()) {
      lead_skipped += skipped; // records in front of the first selected read of the input
    }
  }
  if (res.on && !res.batches.empty() && lead_skipped) {
    res.batches.front().skipped_before.front() += lead_skipped;
  }
  if (prev) {
    run.vt.reads_free(prev);
  }
  if (opt.verbose) {
    std::cerr << "num_passed_reads: " << num_passed_reads << "\n"
              << "num_reads: " << num_reads << "\n"
              << "num_reads - num_passed_reads: " << num_reads - num_passed_reads << "\n"
              << "num_reads - num_passed_reads / num_reads: " << floor((double)(num_reads - num_passed_reads) / num_reads) << "\n"
              << "num_reads_skipped_by_phred: " << by_phred << "\n"
              << "num_reads_skipped_by_delta: " << by_delta << "\n"
              << "num_reads_skipped_by_length: " << by_length << "\n"
              << "num_reads_skipped_by_invalid_bases: " << by_bases << "\n"
              << "Total reads skipped: " << by_phred + by_delta + by_length + by_bases << std::endl;
  }
  if (num_passed_reads == 0 && input_failed()) {
    return -1; // (not an input without usable reads: one that could not be read — the caller reports that)
  }
  if (num_passed_reads == 0) {
    std::cerr << "Error: no reads passed the Phred score and min length requirements\n"
              << "Try again with a lower Phred threshold or lower min length" << std::endl;
    return 1;
  }
  const double ts0 = trace ? now_s() : 0.0;
  if (run.vt.sync(run.ctx) != GRP_OK) {
    return run.fail_engine("bit-vector insert");
  }
  if (trace) {
    (void)t_keep;
    std::cerr << "GRP_TRACE_INGEST fill pass: " << n_batches << " batches; host seconds in next() (read + parse) " << t_next << ", filter " << t_filter << ", upload (pack) " << t_upload << ", bv_insert call " << t_fill
              << ", final sync " << now_s() - ts0 << std::endl;
  }
  if (run.shard_fill) {
    // the bitwise OR of the ranks' vectors (the fill is order-free; csrc/host/gr_ranks.cpp)
    const int mrc = gr_fill_merge_run(&run.vt, run.ctx, run.shm, run.world, run.rank, run.merge_rccl ? GR_MERGE_RCCL : GR_MERGE_STAGED);
    if (mrc == 1) {
      return run.fail_engine(run.merge_rccl ? "merging the bit vectors of the ranks (RCCL)" : "merging the bit vectors of the ranks");
    }
    if (mrc != 0) {
      std::cerr << "goldrush-path: the exchange between the ranks failed" << std::endl;
      return 1;
    }
  }
  std::cerr << "finished inserting bit vector" << std::endl;
  std::cerr << "in " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  return -1;
}

// classification sink: writes one committed read (goldrush_path.cpp:996-1002, 1055-1070)
struct SinkState
{
  PathRun* run = nullptr;
  const Batch* batch = nullptr;
  const std::vector<uint32_t>* sel = nullptr;
  // reads kept on the device: the record's text comes from the input file
  const ResidentBatch* resident = nullptr;
  Resident* res = nullptr;
  Deferred* deferred = nullptr; // the resident run has compressed inputs: the commits are written in batches
  std::vector<char> text;
  std::string upper;
  std::string bam_seq, bam_qual; // a BAM record's written slice as text
  // --debug: the records that are not classified, in file order ({record, 1 = too short / 2 = filtered}),
  // and for every classified read the number of them in front of it
  const std::vector<std::pair<uint32_t, uint8_t>>* skipped = nullptr;
  const std::vector<uint32_t>* skipped_before = nullptr;
  size_t skipped_done = 0;
};

// --debug: what process_read prints for the records it skips (goldrush_path.cpp:907-932)
void
debug_skipped(const SinkState& st, size_t from, size_t to)
{
  const Batch& b = *st.batch;
  for (size_t i = from; i < to; ++i) {
    const auto& sk = (*st.skipped)[i];
    std::cerr << (sk.second == 1 ? "too short" : "hairpin or quality too low or invalid bases") << std::endl;
    std::cerr << "skipping: " << b.id_str(sk.first) << std::endl;
  }
}

// --debug: in front of a classified read (:907-941)
void
debug_sink(void* user, uint32_t read)
{
  SinkState& st = *static_cast<SinkState*>(user);
  const size_t n = (*st.skipped_before)[read];
  debug_skipped(st, st.skipped_done, st.skipped_done + n);
  st.skipped_done += n;
  const Batch& b = *st.batch;
  const uint32_t i = (*st.sel)[read];
  std::cerr << "name: " << b.id_str(i) << std::endl;
  std::cerr << "num tiles: " << b.rec[i].seq_len / st.run->opt.tile_length << std::endl;
}

// The slice of a committed read that is written (goldrush_path.cpp:996-1002, 1055-1070): bases [off, off + n_seq), qualities
// [qoff, qoff + n_qual); a read inserted whole is written whole
struct WrittenSlice
{
  size_t off, n_seq, qoff, n_qual;
  bool trimmed;
};

WrittenSlice
written_slice(const Opts& opt, size_t seq_len, size_t qual_len, uint32_t kind, uint32_t trim_start, uint32_t trim_end, uint32_t num_tiles)
{
  WrittenSlice w{ 0, seq_len, 0, qual_len, kind == DEC_INSERT_TRIMMED };
  if (w.trimmed) {
    const size_t tile = opt.tile_length;
    w.off = (size_t)trim_start * tile;
    const size_t end_pos = (trim_end == num_tiles - 1) ? std::string::npos : (size_t)(trim_end - trim_start + 1) * tile;
    w.n_seq = std::min(end_pos, seq_len - w.off);
    w.n_qual = (w.off <= qual_len) ? std::min(end_pos, qual_len - w.off) : 0;
  }
  w.qoff = std::min(w.off, qual_len);
  return w;
}

// One committed read, whose text is in `b`, to the output file; returns sum_phred of the qualities it wrote
double
write_record(SinkState& st, const Batch& b, const Rec& r, uint32_t kind, uint32_t trim_start, uint32_t trim_end, uint32_t num_tiles)
{
  PathRun& run = *st.run;
  const char first = run.opt.silver_path ? '@' : '>';
  const WrittenSlice w = written_slice(run.opt, r.seq_len, r.qual_len, kind, trim_start, trim_end, num_tiles);
  const char* suffix = w.trimmed ? "_trimmed\n" : "_untrimmed\n";
  const size_t n_seq = w.n_seq, n_qual = w.n_qual;
  // the written slice (a BAM batch: it alone is decoded — bases through the code table, qualities + 33)
  const char* seq = b.seq_text(r, w.off, n_seq, st.bam_seq);
  const char* qual = b.qual_text(r, w.qoff, n_qual, st.bam_qual);
  std::ofstream& o = run.out;
  o.put(first);
  o.write(b.text + r.id_off, (std::streamsize)r.id_len);
  o << suffix;
  if (b.seq_is_upper || b.bam) { // (the code table is upper case)
    o.write(seq, (std::streamsize)n_seq);
  } else {
    // SeqReader folds the case of what the reference later writes
    st.upper.assign(seq, n_seq);
    for (char& ch : st.upper) {
      if (ch >= 'a' && ch <= 'z') {
        ch = (char)(ch - 32);
      }
    }
    o.write(st.upper.data(), (std::streamsize)n_seq);
  }
  o << std::endl;
  if (run.opt.silver_path) {
    o << "+\n";
    o.write(qual, (std::streamsize)n_qual);
    o << std::endl;
  }
  return sum_phred(qual, n_qual);
}

// resident mode, a plain file: one record read back from the file and written
double
write_plain_record(SinkState& st, const RecLoc& l, uint32_t kind, uint32_t trim_start, uint32_t trim_end, uint32_t num_tiles)
{
  PathRun& run = *st.run;
  const size_t n = (size_t)l.qual_rel + l.qual_len;
  st.text.resize(n);
  size_t got = 0;
  const int fd = st.res->fd_of(run, l.file);
  while (got < n) {
    const ssize_t k = fd < 0 ? -1 : pread(fd, st.text.data() + got, n - got, (off_t)(l.off + got));
    if (k <= 0) {
      // not exit(1) from inside the commit callback (a streaming window may be parked on this thread's word,
      // ADVICE r03): the failure is noted, this and the later records are not written, and the program ends with
      // an error behind the pass
      note_input_failure("cannot read the record at byte " + std::to_string(l.off) + " back from " + run.files[l.file]);
      return 0.0;
    }
    got += (size_t)k;
  }
  Batch fetched;
  fetched.text = st.text.data();
  fetched.seq_is_upper = false;
  const Rec rec{ 0, l.id_len, l.seq_rel, l.seq_len, (size_t)l.qual_rel, l.qual_len };
  return write_record(st, fetched, rec, kind, trim_start, trim_end, num_tiles);
}

// ---- the written records of compressed inputs, fetched in batches (GRP_RESIDENT=all) ------------------------------------
// A record of a plain file is read back with one pread.  The text of a BGZF / gzip / BAM input exists only behind an
// inflate, and one record at a time through zlib is out of the question, so the commits are only written down and the
// records of many of them are fetched together: the units that hold them (gr_units.hpp) are read from the file, and the
// engine inflates them and hands back the formatted records with their Phred sums (grp_records_fetch; without that entry
// point the host inflates the units through bgzf_inflate / gzip_inflate and formats with write_record).
//
// WHERE a flush runs is the one constraint: it launches kernels and waits for them, and a streaming window that is parked
// on this thread's word holds the device with its persistent launch.  A flush therefore runs from the classifier's settle
// hook and from the rollover callback alone — the top of a rolling-over silver_path_check, where the committing read has
// ended the streaming launches in front of its insert (gr_classifier.cpp: `rolls_over` means stream_abort on both; a
// window of several ranks and one that is not resumable were aborted in front of the commit; batch and pipelined windows
// are ordinary launches that end by themselves), and the end of Classifier::run, behind drop_streams — never from
// commit_sink, a timer or the size of the list.  One run is one ingest chunk, which bounds the list.  The rollover
// callback follows the settle hook at once, so the list is empty when the output file changes: it holds no path
// boundaries.  Ranks other than 0 write nothing: they queue nothing and have no hook.
void
Deferred::flush(SinkState& st)
{
  Resident& res = *st.res;
  if (pend.empty()) {
    return;
  }
  ++n_flushes;
  const size_t want = sums.size() + pend.size(); // one sum per record of the list, written or not
  size_t i = 0;
  while (i < pend.size() && !input_failed()) {
    const uint32_t f = pend[i].loc.file;
    size_t e = i + 1;
    while (e < pend.size() && pend[e].loc.file == f) {
      ++e;
    }
    if (res.kind[f] == Resident::PLAIN) {
      for (; i < e && !input_failed(); ++i) {
        sums.push_back(write_plain_record(st, pend[i].loc, pend[i].kind, pend[i].trim_start, pend[i].trim_end, pend[i].num_tiles));
      }
    } else {
      while (i < e && fetch_some(st, i, e)) {
      }
      if (i < e) {
        break; // (the failure is noted)
      }
    }
  }
  while (sums.size() < want) { // (an input failure: what was not written counts nothing)
    sums.push_back(0.0);
  }
  pend.clear();
}

// one call of the fetch for records [i, e) of the list, all of one compressed file: as many as its buffers take; i moves
// behind them.  false: a failure was noted.
bool
Deferred::fetch_some(SinkState& st, size_t& i, size_t e)
{
  PathRun& run = *st.run;
  Resident& res = *st.res;
  const uint32_t f = pend[i].loc.file;
  const bool gz = res.kind[f] == Resident::GZIP, bam = res.bam[f] != 0, fastq = run.opt.silver_path;
  const std::vector<uint64_t>& toff = gz ? res.gz_text_off[f] : run.bgzf_map[f]->text_off;
  items.clear();
  for (size_t j = i; j < e; ++j) {
    items.push_back(FetchItem{ pend[j].loc.off, pend[j].loc.qual_rel + pend[j].loc.qual_len });
  }
  if (!plan_fetch(toff, items.data(), items.size(), kTextCap, kMaxUnits, plan)) {
    note_input_failure("the record at byte " + std::to_string(pend[i].loc.off) + " of the text of " + run.files[f] + " does not lie inside the units the fill pass wrote down");
    return false;
  }
  // the units' compressed bytes (and histories), one after the other
  comp.clear();
  dict.clear();
  blocks.clear();
  segs.clear();
  const int fd = res.fd_of(run, f);
  for (const size_t u : plan.units) {
    uint64_t at, n;
    if (gz) {
      const GzSegment& g = run.gzidx[f]->segs[u];
      at = g.first_byte();
      n = g.end_byte() - at;
      segs.push_back(grp_gzip_segment{ g.comp_bit - at * 8 + (uint64_t)comp.size() * 8, g.n_bits, (uint64_t)dict.size(), g.dict_len, g.text_len, g.crc32, g.flags });
      dict.insert(dict.end(), run.gzidx[f]->dict(g), run.gzidx[f]->dict(g) + g.dict_len);
      dict.resize((dict.size() + 3) & ~size_t(3));
    } else {
      const grp_bgzf_block& b = run.bgzf_map[f]->blocks[u];
      at = b.comp_off;
      n = b.comp_len;
      blocks.push_back(grp_bgzf_block{ (uint64_t)comp.size(), b.comp_len, b.text_len, b.crc32, 0 });
    }
    const size_t have = comp.size();
    comp.resize(have + (size_t)n);
    size_t got = 0;
    while (got < n) {
      const ssize_t k = fd < 0 ? -1 : pread(fd, comp.data() + have + got, (size_t)n - got, (off_t)(at + got));
      if (k <= 0) {
        note_input_failure("cannot read the compressed bytes at byte " + std::to_string(at) + " back from " + run.files[f]);
        return false;
      }
      got += (size_t)k;
    }
  }
  const uint32_t n_units = (uint32_t)plan.units.size();
  const void* units = gz ? static_cast<const void*>(segs.data()) : static_cast<const void*>(blocks.data());
  const auto engine_says = [&](const char* what) {
    note_input_failure(std::string("reading ") + run.files[f] + " failed: " + what + ": " + (run.vt.last_error ? run.vt.last_error(run.ctx) : "the engine refused"));
    return false;
  };
  if (run.ext.records_fetch) {
    recs.clear();
    uint64_t out_n = 0;
    for (size_t j = 0; j < plan.n_recs; ++j) {
      const Pending& p = pend[i + j];
      const RecLoc& l = p.loc;
      const WrittenSlice w = written_slice(run.opt, l.seq_len, l.qual_len, p.kind, p.trim_start, p.trim_end, p.num_tiles);
      const uint64_t t0 = plan.rec_text_off[j];
      // (a reversed record: the written slice counts in the twin's coordinates, the fetch takes the stored range and writes it backwards)
      const uint32_t seq_from = l.reversed ? (uint32_t)(l.seq_len - w.off - w.n_seq) : (uint32_t)w.off, qual_from = l.reversed ? (uint32_t)(l.qual_len - w.qoff - w.n_qual) : (uint32_t)w.qoff;
      recs.push_back(grp_fetch_record{ t0, t0 + l.seq_rel, t0 + l.qual_rel, out_n, l.id_len, seq_from, (uint32_t)w.n_seq, qual_from, (uint32_t)w.n_qual,
                                       (w.trimmed ? GRP_FETCH_REC_TRIMMED : 0u) | (l.reversed ? GRP_FETCH_REC_REVERSED : 0u) });
      out_n += 1 + (uint64_t)l.id_len + (w.trimmed ? 9 : 11) + w.n_seq + 1 + (fastq ? 3 + (uint64_t)w.n_qual : 0);
    }
    out.resize((size_t)out_n);
    got_sums.assign(plan.n_recs, 0.0);
    uint32_t bad_unit = UINT32_MAX, bad_rec = UINT32_MAX;
    if (run.ext.records_fetch(run.ctx, gz ? GRP_FETCH_UNITS_GZIP : GRP_FETCH_UNITS_BGZF, comp.data(), comp.size(), dict.data(), dict.size(), units, n_units, recs.data(), (uint32_t)recs.size(),
                              (fastq ? GRP_FETCH_FASTQ : 0u) | (bam ? GRP_FETCH_BAM : 0u), out.data(), out.size(), got_sums.data(), &bad_unit, &bad_rec) != GRP_OK) {
      return engine_says("the written records could not be fetched");
    }
    run.out.write(out.data(), (std::streamsize)out.size());
    sums.insert(sums.end(), got_sums.begin(), got_sums.end());
    n_out_bytes += out.size();
  } else {
    // the host's own fetch: the units' text through the inflate entry points, formatted by write_record
    text.resize((size_t)plan.text_bytes + 8);
    uint32_t bad = UINT32_MAX;
    const int rc = gz ? run.ext.gzip_inflate(run.ctx, comp.data(), comp.size(), dict.data(), dict.size(), segs.data(), n_units, text.data(), plan.text_bytes, &bad)
                      : run.ext.bgzf_inflate(run.ctx, comp.data(), comp.size(), blocks.data(), n_units, text.data(), plan.text_bytes, &bad);
    if (rc != GRP_OK) {
      return engine_says("the units of the written records could not be inflated");
    }
    Batch b;
    b.text = text.data();
    b.bam = bam;
    const std::streampos before = run.out.tellp();
    for (size_t j = 0; j < plan.n_recs; ++j) {
      const Pending& p = pend[i + j];
      const RecLoc& l = p.loc;
      const size_t t0 = (size_t)plan.rec_text_off[j];
      const Rec rec{ t0, l.id_len, t0 + l.seq_rel, l.seq_len, t0 + (size_t)l.qual_rel, l.qual_len, l.reversed != 0 };
      sums.push_back(write_record(st, b, rec, p.kind, p.trim_start, p.trim_end, p.num_tiles));
    }
    n_out_bytes += (uint64_t)(run.out.tellp() - before);
  }
  n_units_inflated += n_units;
  n_text_bytes += plan.text_bytes;
  n_records += plan.n_recs;
  n_straddling += plan.straddling;
  for (size_t j = 0; j < plan.n_recs; ++j) {
    n_trimmed += pend[i + j].kind == DEC_INSERT_TRIMMED ? 1 : 0;
  }
  i += plan.n_recs;
  return true;
}

// the classifier's settle hook: the sums of the n insert commits since the last call, in commit order
void
settle_sink(void* user, double* out_sums, uint32_t n)
{
  SinkState& st = *static_cast<SinkState*>(user);
  Deferred& d = *st.deferred;
  d.flush(st);
  for (uint32_t k = 0; k < n && !d.sums.empty(); ++k) {
    out_sums[k] = d.sums.front();
    d.sums.pop_front();
  }
}

double
commit_sink(void* user, const gr_commit* c)
{
  SinkState& st = *static_cast<SinkState*>(user);
  if (c->dec.kind != DEC_INSERT_WHOLE && c->dec.kind != DEC_INSERT_TRIMMED) {
    return 0.0;
  }
  if (input_failed()) {
    return 0.0;
  }
  if (st.resident && st.deferred) {
    // (ranks other than 0 write nothing and print nothing: nothing to fetch)
    if (st.run->rank == 0) {
      st.deferred->pend.push_back(Deferred::Pending{ st.resident->loc[c->read], c->dec.kind, c->dec.trim_start, c->dec.trim_end, c->dec.num_tiles });
    }
    return 0.0; // (the sum comes through the settle hook)
  }
  if (st.resident) {
    return write_plain_record(st, st.resident->loc[c->read], c->dec.kind, c->dec.trim_start, c->dec.trim_end, c->dec.num_tiles);
  }
  const Batch& b = *st.batch;
  return write_record(st, b, b.rec[(*st.sel)[c->read]], c->dec.kind, c->dec.trim_start, c->dec.trim_end, c->dec.num_tiles);
}

void
rollover_sink(void* user, uint64_t new_path)
{
  // golden_path_vec.pop_back(); emplace_back(ofstream(prefix + "_" + path + ".fq"))  (:182-184)
  SinkState& st = *static_cast<SinkState*>(user);
  PathRun& run = *st.run;
  if (st.deferred) {
    st.deferred->flush(st); // (the settle hook has run in front of this callback: nothing is left — the records of a path go to its file)
  }
  run.out.close();
  run.out.open(run.rank == 0 ? run.opt.prefix_file + "_" + std::to_string(new_path) + ".fq" : std::string("/dev/null"));
}

} // namespace
} // namespace gr

extern "C" int
gr_path_main(int argc, char** argv, const grp_engine_vt* vt)
{
  return gr_path_main_ext(argc, argv, vt, nullptr);
}

extern "C" int
gr_path_main_ext(int argc, char** argv, const grp_engine_vt* vt, const grp_engine_ext* ext)
{
  using namespace gr;
  PathRun run;
  run.vt = *vt;
  if (ext && ext->struct_size >= offsetof(grp_engine_ext, bgzf_inflate) + sizeof(ext->bgzf_inflate)) {
    run.ext.bgzf_inflate = ext->bgzf_inflate;
  }
  if (ext && ext->struct_size >= offsetof(grp_engine_ext, gzip_inflate) + sizeof(ext->gzip_inflate)) {
    run.ext.gzip_inflate = ext->gzip_inflate;
  }
  if (ext && ext->struct_size >= offsetof(grp_engine_ext, bam_parse) + sizeof(ext->bam_parse)) {
    run.ext.bam_parse = ext->bam_parse;
  }
  if (ext && ext->struct_size >= offsetof(grp_engine_ext, records_fetch) + sizeof(ext->records_fetch)) {
    run.ext.records_fetch = ext->records_fetch;
  }
  if (ext && ext->struct_size >= offsetof(grp_engine_ext, bam_parse_ex) + sizeof(ext->bam_parse_ex)) {
    run.ext.bam_parse_ex = ext->bam_parse_ex;
  }
  Opts& opt = run.opt;
  // Several GPUs of one node: one process per GPU (GRP_WORLD / GRP_RANK, or the launcher's
  // WORLD_SIZE / RANK; LOCAL_RANK picks the device).  Every rank runs the whole program on
  // its own replica of the miBF — the same input, the same passes, every insert — and the
  // ranks share the QUERY work of each classification window (gr_classifier: the window's
  // reads are split / striped over the ranks, the 32-byte decisions all-gathered through
  // /dev/shm).  Rank 0 writes the files and the log; the others are silent.
  auto env_u32 = [](const char* a, const char* b, uint32_t dflt) {
    const char* e = getenv(a);
    if (!e || !*e) {
      e = getenv(b);
    }
    return (e && *e) ? (uint32_t)strtoul(e, nullptr, 10) : dflt;
  };
  run.world = std::max<uint32_t>(1, env_u32("GRP_WORLD", "WORLD_SIZE", 1));
  run.rank = env_u32("GRP_RANK", "RANK", 0);
  if (run.rank >= run.world) {
    std::cerr << "goldrush-path: rank " << run.rank << " outside the world of " << run.world << std::endl;
    return 1;
  }
  struct Quiet // ranks > 0: nothing on stdout / stderr
  {
    std::streambuf *cerr_buf = nullptr, *cout_buf = nullptr;
    std::ofstream null;
    ~Quiet()
    {
      if (cerr_buf) {
        std::cerr.rdbuf(cerr_buf);
        std::cout.rdbuf(cout_buf);
      }
    }
  } quiet;
  if (run.rank != 0) {
    quiet.null.open("/dev/null");
    quiet.cerr_buf = std::cerr.rdbuf(quiet.null.rdbuf());
    quiet.cout_buf = std::cout.rdbuf(quiet.null.rdbuf());
  }
  clear_input_failure();
  // an input that could not be read to its end is an error, not a shorter input (gr_fastq.hpp): checked behind every pass
  auto input_error = [] {
    std::string what;
    if (!input_failed(&what)) {
      return false;
    }
    std::cerr << "ERROR: " << what << std::endl;
    return true;
  };
  int ec = process_options(opt, argc, argv);
  if (ec >= 0) {
    return ec;
  }
  {
    // every -i is an input, a ".fofn" list stands for the files it names (gr_opts.hpp); no -i at all: the reference's empty name
    std::string bad_list;
    if (!expand_inputs(opt.inputs, run.files, bad_list)) {
      std::cerr << "goldrush-path: " << bad_list << std::endl;
      return 1;
    }
    if (run.files.empty()) {
      run.files.push_back(opt.input);
    }
    run.gzidx.resize(run.files.size());
    run.bgzf_map.resize(run.files.size());
    run.bam_aligned.resize(run.files.size());
  }
  {
    // GRP_BAM_ALIGNED=on: a BAM input is read as its aligned twin — what `samtools fastq -n` writes for it with its default
    // filters (gr_bam.hpp).  Read here, once, in front of the first pass; opt-in, because records are dropped
    const char* e = getenv("GRP_BAM_ALIGNED");
    if (e && !strcmp(e, "on")) {
      run.bam_accept = BAM_REFUSED_FLAGS;
    } else if (e && strcmp(e, "off")) {
      std::cerr << "goldrush-path: GRP_BAM_ALIGNED=" << e << ": the switch takes on or off" << std::endl;
      return 1;
    }
  }
  struct ShmGuard
  {
    void* h = nullptr;
    ~ShmGuard() { gr_shm_allgather_close(h); }
  } shm;
  if (run.world > 1) {
    const char* key = getenv("GRP_SHM_KEY");
    std::string k = key && *key ? key : std::string("path_") + (getenv("MASTER_PORT") ? getenv("MASTER_PORT") : "0") + "_" + std::to_string((unsigned long)getppid());
    shm.h = gr_shm_allgather_open(run.world, run.rank, k.c_str(), 120.0);
    if (!shm.h) {
      std::cerr << "goldrush-path: cannot set up the exchange between the " << run.world << " ranks (/dev/shm/grp_" << k << ")" << std::endl;
      return 1;
    }
  }
#if defined(_OPENMP)
  // the reference uses -j for its OpenMP regions; here it only drives the host
  // side (parsing, Phred, packing, decisions) and is capped at the machine size
  omp_set_num_threads((int)std::max<size_t>(1, std::min<size_t>(opt.jobs, (size_t)effective_cpus())));
#endif
  run.seeds = make_seed_pattern(opt.seed_preset, (unsigned)opt.kmer_size, (unsigned)opt.weight, (unsigned)opt.hash_num, true);
  const bool use_ntcard = opt.hash_universe == 0 && opt.ntcard;
  if (use_ntcard && !(run.vt.ntcard_begin && run.vt.ntcard_add && run.vt.ntcard_finish && run.vt.set_filter_size)) {
    std::cerr << "goldrush-path: --ntcard needs an engine with the ntcard entry points" << std::endl;
    return 1;
  }
  if (opt.hash_universe == 0 && !use_ntcard) {
    opt.hash_universe = hash_universe(opt.weight, opt.genome_size, opt.hash_num);
  }
  const std::string what = opt.silver_path ? std::to_string(opt.max_paths) + " silver path(s)" : std::string("the golden path");
  // the engine is set up before the first pass over the input (the Phred median
  // pass already uses the GPU ingest); the reference's messages keep their order.
  // With --ntcard the filter size is only known after the ntcard pass.
  uint64_t filter_size = use_ntcard ? 0 : calc_optimal_size(opt.hash_universe, 1, opt.occupancy);
  {
    std::vector<const char*> sp;
    for (const auto& s : run.seeds) {
      sp.push_back(s.c_str());
    }
    grp_params gp{};
    gp.struct_size = sizeof(gp);
    gp.k = (uint32_t)opt.kmer_size;
    gp.h = (uint32_t)opt.hash_num;
    gp.tile = (uint32_t)opt.tile_length;
    gp.m = filter_size;
    gp.seeds = sp.data();
    gp.device = run.world > 1 ? (int32_t)env_u32("GRP_LOCAL_RANK", "LOCAL_RANK", run.rank) : -1;
    run.device = gp.device;
    if (run.vt.create(&gp, &run.ctx) != GRP_OK) {
      std::cerr << "goldrush-path: cannot set up the MI355X engine: " << (run.vt.last_error ? run.vt.last_error(nullptr) : "") << std::endl;
      return 1;
    }
  }
  struct CtxGuard
  {
    PathRun& r;
    ~CtxGuard()
    {
      if (r.ctx) {
        r.vt.destroy(r.ctx);
      }
    }
  } guard{ run };
  if (run.files.size() > 1) {
    // several inputs: each is looked at before the first pass — a run does not get an hour into the fill before it finds
    // that its last file is missing
    const std::string bad = check_inputs(run);
    if (!bad.empty()) {
      std::cerr << "goldrush-path: " << bad << std::endl;
      std::cerr << "Gold Path requires fastq format" << std::endl;
      return 1;
    }
  }
  if (use_ntcard) {
    uint64_t genome_size = 0;
    ec = calc_ntcard_genome_size(run, genome_size);
    run.say_bam_aligned();
    if (ec >= 0) {
      return ec;
    }
    if (input_error()) {
      return 1;
    }
    opt.hash_universe = genome_size;
    filter_size = calc_optimal_size(opt.hash_universe, 1, opt.occupancy);
    if (run.vt.set_filter_size(run.ctx, filter_size) != GRP_OK) {
      return run.fail_engine("allocating the bit vector");
    }
  }
  if (run.vt.occupancy_hint && opt.occupancy > 0.0 && opt.occupancy < 1.0) {
    // the ID / count tables of phase 2 are sized by the occupancy the fill will reach: -o, by construction of the filter
    // size (:1183-1184) — the engine allocates them beside the fill instead of between the passes (a hint: ignored where wrong)
    (void)run.vt.occupancy_hint(run.ctx, opt.occupancy);
  }
  if (run.world > 1 && shm.h && gr_ranks_share_device(shm.h, run.world, run.device) == 1) {
    // ranks on one device (a test box): their windows' launches must all fit it at once — the in-launch inserts of
    // the ranks' windows wait grid-wide (read at the engine's first streaming launch; an explicit setting stands)
    setenv("GRP_STREAM_WGS_PER_CU", "1", 0);
  }
  if (run.world > 1 && !getenv("GRP_REPLICATED_FILL")) {
    // A sharded fill needs a way to merge: RCCL inside the engine (one GPU per rank), else the
    // host-staged form (ranks sharing a device, engines without RCCL).  Every decision below is
    // taken by ALL ranks alike (flags all-gathered through /dev/shm).
    run.shm = shm.h;
    const int plan = gr_fill_merge_plan(&run.vt, run.ctx, shm.h, run.world, run.rank, run.device);
    run.merge_rccl = plan == GR_MERGE_RCCL;
    run.shard_fill = plan != GR_MERGE_NONE;
  }
  ec = calc_min_phred_threshold(run);
  run.say_bam_aligned();
  if (ec >= 0) {
    return ec;
  }
  if (input_error()) {
    return 1;
  }
  std::cerr << "Calculating " << what << "\n"
            << "Using:\n"
            << "\ttile length: " << opt.tile_length << "\n"
            << "\tblock size: " << opt.block_size << "\n"
            << "\tseed patterns: " << opt.hash_num << "\n"
            << "\tthreshold: " << opt.threshold << "\n"
            << "\tbase seed pattern: " << run.seeds[0] << "\n"
            << "\tminimum unassigned tiles: " << opt.unassigned_min << "\n"
            << "\tmaximum assigned tiles: " << opt.assigned_max << "\n"
            << "\texpected hash space: " << opt.hash_universe << "\n"
            << "\tminimum average phred quality score: " << opt.phred_min << "\n"
            << "\tmaximum average phred delta between first and second half of read: " << opt.phred_delta << "\n"
            << "\toccupancy: " << opt.occupancy << "\n"
            << "\tjobs: " << opt.jobs << std::endl;
  if (!opt.filter_file.empty()) {
    std::cerr << "Using only reads not found in: " << opt.filter_file << std::endl;
    std::ifstream in(opt.filter_file);
    std::string name;
    while (in >> name) {
      run.filter_out_reads.insert(name);
    }
  }
  run.out.open(run.rank != 0 ? std::string("/dev/null") : opt.silver_path ? opt.prefix_file + "_1.fq" : opt.prefix_file + ".fa");
  double s_time = now_s();
  std::cerr << "allocating bit vector" << std::endl;
  std::cerr << "m_filterSize: " << filter_size << std::endl;
  std::cerr << "finished allocating bit vector" << std::endl;
  std::cerr << "in " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  for (const std::string& path : run.files) {
    std::cerr << "opening: " << path << std::endl;
  }

  Resident res;
  struct ResGuard
  {
    PathRun& run;
    Resident& res;
    ~ResGuard()
    {
      res.drop(run);
      res.close_files();
    }
  } res_guard{ run, res };
  {
    const char* e = getenv("GRP_RESIDENT");
    const bool gpu_ingest = run.vt.fastq_parse && run.vt.fastq_records && run.vt.fastq_pack && run.vt.fastq_free && !getenv("GRP_HOST_INGEST");
    res.all = e && !strcmp(e, "all");
    res.kind.assign(run.files.size(), Resident::PLAIN);
    res.bam.assign(run.files.size(), 0);
    if (!(e && !strcmp(e, "off")) && gpu_ingest && !opt.debug) {
      // (every input a plain seekable file — else the whole run takes the two-pass form; GRP_RESIDENT=all: or a file of
      // gzip members, whose records can be fetched through its BGZF members or the segments of its gzip index)
      res.on = true;
      for (size_t f = 0; f < run.files.size() && res.on; ++f) {
        const std::string& path = run.files[f];
        if (is_plain_input(path, run.files.size() > 1)) {
          continue;
        }
        std::string why;
        if (res.all && compressed_candidate(path, why)) {
          res.kind[f] = Resident::UNKNOWN;
        } else {
          res.on = false;
          res.say_dropped(run, why, path);
        }
      }
      const char* cap = getenv("GRP_RESIDENT_MAX_GB");
      res.max_bytes = (uint64_t)((cap ? atof(cap) : 100.0) * (double)(1ull << 30));
    } else {
      res.say_dropped(run, opt.debug ? "--debug" : getenv("GRP_HOST_INGEST") ? "GRP_HOST_INGEST" : "the engine has no ingest entry points");
    }
  }
  ec = fill_bit_vector(run, res);
  run.say_bam_aligned();
  if (ec >= 0) {
    return ec;
  }
  if (input_error()) {
    return 1;
  }
  if (res.on && res.any_compressed()) {
    (void)resolve_units(run, res); // (false: dropped, with its reason line)
  }
  uint64_t pop = 0;
  if (run.vt.finalize(run.ctx, &pop) != GRP_OK) {
    return run.fail_engine("building the rank structure");
  }
  if (run.world > 1 && run.shm) {
    // every rank classifies on its own replica: they must hold the same filter (a merge that failed on one rank
    // would otherwise only show as diverging decisions much later)
    if (gr_ranks_same_u64(run.shm, run.world, pop) != 1) {
      std::cerr << "ERROR: the ranks' filters differ after the merge (rank " << run.rank << ": " << pop << " set bits)" << std::endl;
      return 1;
    }
  }

  std::cerr << "assigning tiles" << std::endl;
  s_time = now_s();
  gr_classifier_params cp{};
  cp.struct_size = sizeof(cp);
  cp.tile_length = (uint32_t)opt.tile_length;
  cp.block_size = (uint32_t)opt.block_size;
  cp.threshold = (uint32_t)opt.threshold;
  cp.unassigned_min = (uint32_t)opt.unassigned_min;
  cp.assigned_max = (uint32_t)opt.assigned_max;
  cp.kmer_size = (uint32_t)opt.kmer_size;
  cp.hash_num = (uint32_t)opt.hash_num;
  cp.target_bases = (uint64_t)(opt.ratio * opt.genome_size); // :1223
  cp.max_paths = opt.max_paths;
  cp.silver_path = opt.silver_path;
  cp.verbose = opt.verbose;
  cp.world = run.world;
  cp.rank = run.rank;
  cp.debug = opt.debug;
  cp.seed0_span = (uint32_t)run.seeds[0].size();
  if (opt.debug && run.world > 1) {
    std::cerr << "goldrush-path: --debug runs on one rank" << std::endl;
    return 1;
  }
  Classifier cls(cp, run.vt, run.ctx);
  SinkState sink;
  sink.run = &run;
  cls.set_callbacks(commit_sink, rollover_sink, nullptr, &sink);
  if (run.world > 1) {
    cls.set_allgather(gr_shm_allgather, shm.h);
  }
  if (opt.debug) {
    cls.set_debug(debug_sink);
  }

  Deferred deferred;
  const auto trace_fetch = [&] {
    if (getenv("GRP_TRACE_INGEST") && sink.deferred && run.rank == 0) {
      std::cerr << "GRP_TRACE_INGEST resident fetch: " << deferred.n_flushes << " flushes, units inflated " << deferred.n_units_inflated << ", text bytes inflated " << deferred.n_text_bytes << ", records fetched "
                << deferred.n_records << " (trimmed " << deferred.n_trimmed << ", in two or more units " << deferred.n_straddling << "), output bytes " << deferred.n_out_bytes
                << (run.ext.records_fetch ? " (formatted on the device)" : " (inflated through the engine, formatted on the host)") << std::endl;
    }
  };
  if (res.on) {
    // the classification pass over the batches the fill pass left in HBM: no second parse
    sink.res = &res;
    if (res.any_compressed()) {
      sink.deferred = &deferred;
      if (run.rank == 0) {
        cls.set_settle(settle_sink, &sink);
      }
    }
    std::unordered_set<uint64_t> filtered_hash;
    for (const std::string& name : run.filter_out_reads) {
      filtered_hash.insert(fnv1a(name.data(), name.size()));
    }
    bool finished = false;
    std::vector<uint32_t> sb;
    std::string name;
    for (size_t bi = 0; bi < res.batches.size() && !finished; ++bi) {
      ResidentBatch& rb = res.batches[bi];
      const uint32_t n = (uint32_t)rb.lens.size();
      // reads named in filter_out_reads (a -f list, or a failing read of the same name) are not
      // classified (read_hashing.cpp:35-42): they become skipped records of the run behind them
      std::vector<uint8_t> drop(n, 0);
      bool any_drop = false;
      if (!filtered_hash.empty()) {
        for (uint32_t i = 0; i < n; ++i) {
          if (filtered_hash.count(rb.name_hash[i])) {
            name.resize(rb.loc[i].id_len);
            bool have = false;
            if (res.kind[rb.loc[i].file] != Resident::PLAIN) {
              name.assign(rb.ids, (size_t)rb.id_at[i], rb.loc[i].id_len);
              have = true;
            } else {
              const int fd = res.fd_of(run, rb.loc[i].file);
              have = fd >= 0 && pread(fd, &name[0], name.size(), (off_t)rb.loc[i].off) == (ssize_t)name.size();
            }
            if (have && run.filter_out_reads.count(name)) {
              drop[i] = 1;
              any_drop = true;
            }
          }
        }
      }
      sink.resident = &rb;
      int rc = GRP_OK;
      if (!any_drop) {
        rc = cls.run(rb.reads, rb.lens.data(), 0, n, rb.skipped_before.data(), rb.skipped_after, finished);
      } else {
        // kept reads with the records skipped in front of each (dropped reads included), runs of
        // consecutive kept reads go to the classifier one after the other
        sb.assign(n, 0);
        std::vector<uint32_t> idx;
        uint32_t carry = 0;
        for (uint32_t i = 0; i < n; ++i) {
          if (drop[i]) {
            carry += rb.skipped_before[i] + 1;
          } else {
            sb[i] = rb.skipped_before[i] + carry;
            carry = 0;
            idx.push_back(i);
          }
        }
        const uint32_t trailing = carry + rb.skipped_after;
        if (idx.empty()) {
          rc = cls.run(rb.reads, rb.lens.data(), 0, 0, sb.data(), trailing, finished);
        }
        for (size_t a = 0; a < idx.size() && rc == GRP_OK && !finished;) {
          size_t e = a + 1;
          while (e < idx.size() && idx[e] == idx[e - 1] + 1) {
            ++e;
          }
          rc = cls.run(rb.reads, rb.lens.data(), idx[a], (uint32_t)(e - a), sb.data(), e == idx.size() ? trailing : 0u, finished);
          a = e;
        }
      }
      run.vt.reads_free(rb.reads);
      rb.reads = nullptr;
      if (rc != GRP_OK) {
        std::cerr << "goldrush-path: " << cls.error() << std::endl;
        return 1;
      }
    }
    sink.resident = nullptr;
    trace_fetch();
    if (finished) {
      run.out.flush();
      return sink.deferred && input_error() ? 1 : 0; // exit(0) inside silver_path_check (:173-176); (a fetch that failed is an error)
    }
  } else {
    auto src = open_source(run);
    Batch b;
    std::vector<uint32_t> sel, skipped_before, lens;
    std::vector<std::pair<uint32_t, uint8_t>> skipped_recs;
    bool finished = false;
    while (!finished && src->ok() && src->next(b)) {
      // read_hashing.cpp:35-42 / goldrush_path.cpp:907-932: a read is classified
      // iff it is long enough and not in filter_out_reads
      sel.clear();
      skipped_before.clear();
      skipped_recs.clear();
      uint32_t skipped = 0;
      for (size_t i = 0; i < b.rec.size(); ++i) {
        bool eligible = b.rec[i].seq_len >= opt.min_length;
        uint8_t why = eligible ? 0 : 1;
        if (eligible && !run.filter_out_reads.empty() && run.filter_out_reads.count(b.id_str(i))) {
          eligible = false;
          why = 2;
        }
        if (!eligible && opt.debug) {
          skipped_recs.emplace_back((uint32_t)i, why);
        }
        if (eligible) {
          sel.push_back((uint32_t)i);
          skipped_before.push_back(skipped);
          skipped = 0;
        } else {
          ++skipped;
        }
      }
      void* h = nullptr;
      if (src->upload(b, sel, lens, &h) != GRP_OK) {
        return run.fail_engine("uploading reads");
      }
      sink.batch = &b;
      sink.sel = &sel;
      sink.skipped = &skipped_recs;
      sink.skipped_before = &skipped_before;
      sink.skipped_done = 0;
      const int rc = cls.run(h, lens.data(), 0, (uint32_t)sel.size(), skipped_before.data(), skipped, finished);
      if (opt.debug && rc == GRP_OK && !finished) {
        debug_skipped(sink, sink.skipped_done, skipped_recs.size()); // the records behind the batch's last classified read
      }
      run.vt.reads_free(h);
      if (rc != GRP_OK) {
        std::cerr << "goldrush-path: " << cls.error() << std::endl;
        return 1;
      }
    }
    run.say_bam_aligned();
    if (finished) {
      run.out.flush();
      return input_error() ? 1 : 0; // exit(0) inside silver_path_check (:173-176)
    }
  }
  if (input_error()) {
    return 1;
  }
  if (opt.silver_path && opt.max_paths > cls.curr_path()) {
    std::cerr << "WARNING: Expected " << std::to_string(opt.max_paths) << " silver paths, but only " << std::to_string(cls.curr_path()) << " generated.\n"
              << "Possible reasons include:\n"
              << "\t- Input reads sorted by chromosome/position\n"
              << "\t- Genome size set too large\n";
  }
  if (opt.verbose) {
    cls.log_path_stat();
  }
  std::cerr << "assigned" << std::endl;
  std::cerr << "in " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  return 0;
}
