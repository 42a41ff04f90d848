// The passes over the input (gr_passes.hpp): goldrush_path.cpp:1109-1112, 79-107, 235-339, 1210-1256.
#include "gr_passes.hpp"
#include "gr_fastq.hpp"
#include "gr_golden.hpp"
#include "gr_params.hpp"

#include <cmath>
#include <functional>
#include <iomanip>

namespace gr {

bool
input_error()
{
  std::string what;
  const bool failed = input_failed(&what);
  if (failed) {
    std::cerr << "ERROR: " << what << std::endl;
  }
  return failed;
}

int
after_pass(PathRun& run, int ec)
{
  run.say_bam_aligned();
  return ec >= 0 ? ec : input_error() ? 1 : -1;
}

// goldrush_path.cpp:1109-1112 -> calc_ntcard_genome_size (ntcard.hpp:248-275): the
// hash stream of EVERY record (no read filter) sampled on the device; the host only
// turns the zero-bucket counts into F0.
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
    // the runs, packed here; then the clean records — stRead (:96-112): multiLensfrHashIterator over the whole sequence, ntComp per seed
    for (const bool cut : { true, false }) {
      const uint32_t n = (uint32_t)(cut ? lens.size() : sel.size());
      if (n == 0) {
        continue;
      }
      void* hr = nullptr;
      packed.resize(std::max<size_t>(packed.size(), 1));
      if ((cut ? run.vt.reads_upload(run.ctx, packed.data(), word_off.data(), lens.data(), n, &hr) : src->upload(b, sel, lens, &hr)) != GRP_OK) {
        return run.fail_engine("uploading reads");
      }
      const int rc = run.vt.ntcard_add(run.ctx, hr, 0, n, cut ? extra.data() : nullptr);
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
  // prints "occupancy: 0.1000" after an ntcard pass)
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

namespace {

// The read filters of the fill pass over one batch (goldrush_path.cpp:261-301): the records that pass go to `sel`, and, the
// reads staying on the device, what the classification pass needs of them to `keep`.  Returns the records behind the last
// selected one.
uint32_t
filter_batch(PathRun& run, Resident& res, const Batch& b, FillCounts& n, std::vector<uint32_t>& sel, ResidentBatch& keep)
{
  const Opts& opt = run.opt;
  uint32_t skipped = 0;
  for (size_t i = 0; i < b.rec.size(); ++i) {
    ++n.num_reads;
    ++skipped; // (taken back below when the record is selected)
    if (b.rec[i].seq_len < opt.min_length) { // :261-265
      ++n.by_length;
      continue;
    }
    if (opt.debug) { // :267-273 (file order here; the reference prints from an OpenMP region)
      std::cerr << "phred avg: " << b.avg[i] << "\n"
                << "phred delta: " << b.delta[i] << std::endl;
    }
    const bool low = b.avg[i] < opt.phred_min, hairpin = b.delta[i] >= opt.phred_delta;
    if (low || hairpin) { // :275-292
      if (opt.verbose) {
        n.by_phred += low ? 1 : 0;
        n.by_delta += hairpin ? 1 : 0;
      }
      run.filter_out_reads.insert(b.id_str(i));
      continue;
    }
    if (b.non_acgt[i]) { // :293-301
      ++n.by_bases;
      run.filter_out_reads.insert(b.id_str(i));
      continue;
    }
    ++n.num_passed_reads;
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
  return skipped;
}

} // namespace

// behind the fill pass's loop: its --verbose counts; 1 (said): no read passed; -2: none passed because the input could not
// be read (the caller reports that); -1: go on
int
say_fill_counts(const PathRun& run, const FillCounts& n)
{
  const Opts& opt = run.opt;
  if (opt.verbose) {
    std::cerr << "num_passed_reads: " << n.num_passed_reads << "\n"
              << "num_reads: " << n.num_reads << "\n"
              << "num_reads - num_passed_reads: " << n.num_reads - n.num_passed_reads << "\n"
              << "num_reads - num_passed_reads / num_reads: " << floor((double)(n.num_reads - n.num_passed_reads) / n.num_reads) << "\n"
              << "num_reads_skipped_by_phred: " << n.by_phred << "\n"
              << "num_reads_skipped_by_delta: " << n.by_delta << "\n"
              << "num_reads_skipped_by_length: " << n.by_length << "\n"
              << "num_reads_skipped_by_invalid_bases: " << n.by_bases << "\n"
              << "Total reads skipped: " << n.by_phred + n.by_delta + n.by_length + n.by_bases << std::endl;
  }
  if (n.num_passed_reads == 0) {
    if (input_failed()) {
      return -2; // (not an input without usable reads: one that could not be read — the caller reports that)
    }
    std::cerr << "Error: no reads passed the Phred score and min length requirements\n"
              << "Try again with a lower Phred threshold or lower min length" << std::endl;
    return 1;
  }
  return -1;
}

// goldrush_path.cpp:235-339
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
  FillCounts n;
  Batch b;
  void* prev = nullptr;
  std::vector<uint32_t> sel, lens;
  uint32_t lead_skipped = 0;
  uint64_t n_batches = 0;
  // developer trace (GRP_TRACE_INGEST): where the host's time of this pass goes, per call site
  static const bool trace = getenv("GRP_TRACE_INGEST") != nullptr;
  double t_next = 0, t_filter = 0, t_upload = 0, t_fill = 0, t_keep = 0, t_last = trace ? now_s() : 0.0;
  const auto lap = [&](double& t) { // the time since the last lap goes to t
    const double now = trace ? now_s() : 0.0;
    t += now - t_last;
    t_last = now;
  };
  while (src->next(b)) {
    lap(t_next);
    src->stats(b, opt.min_length, true);
    sel.clear();
    ResidentBatch keep;
    uint32_t skipped = filter_batch(run, res, b, n, sel, keep);
    if (res.on && sel.empty() && !res.batches.empty()) {
      res.batches.back().skipped_after += skipped; // a batch without a single selected read
      skipped = 0;
    }
    lap(t_filter);
    if (!sel.empty()) {
      void* h = nullptr;
      if (src->upload(b, sel, lens, &h) != GRP_OK) {
        return run.fail_engine("uploading reads");
      }
      lap(t_upload);
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
      lap(t_fill);
      for (size_t i = 0; res.on && i < lens.size(); ++i) {
        res.packed_bytes += ((uint64_t)lens[i] + 15) / 16 * 4;
      }
      if (res.on && res.packed_bytes > res.max_bytes) {
        res.say_dropped(run, "the packed reads exceed GRP_RESIDENT_MAX_GB", run.files[b.file]);
        res.drop(run); // too much to keep: the classification pass parses the input again
      }
      if (res.on) {
        keep.reads = h;
        keep.lens = lens;
        keep.skipped_after = skipped;
        res.batches.push_back(std::move(keep));
      } else {
        prev = h;
      }
    } else if (res.on && res.batches.empty()) {
      lead_skipped += skipped; // records in front of the first selected read of the input
    }
    lap(t_keep); // (not said)
  }
  if (res.on && !res.batches.empty() && lead_skipped) {
    res.batches.front().skipped_before.front() += lead_skipped;
  }
  if (prev) {
    run.vt.reads_free(prev);
  }
  const int counted = say_fill_counts(run, n);
  if (counted != -1) {
    return counted == -2 ? -1 : counted;
  }
  const double ts0 = trace ? now_s() : 0.0;
  if (run.vt.sync(run.ctx) != GRP_OK) {
    return run.fail_engine("bit-vector insert");
  }
  if (trace) {
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

int
classify_resident(PathRun& run, Resident& res, Classifier& cls, SinkState& sink)
{
  Deferred deferred;
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
  // is read i of the batch named in filter_out_reads?  (its id: kept beside the batch, or read back from its plain file)
  std::string name;
  const auto filtered = [&](const ResidentBatch& rb, uint32_t i) {
    const RecLoc& l = rb.loc[i];
    if (filtered_hash.empty() || !filtered_hash.count(rb.name_hash[i])) {
      return false;
    }
    if (res.kind[l.file] != Resident::PLAIN) {
      name.assign(rb.ids, (size_t)rb.id_at[i], l.id_len);
    } else {
      int err = 0;
      name.resize(l.id_len);
      const int fd = res.fd_of(run, l.file);
      if (fd < 0 || pread_full(fd, &name[0], name.size(), l.off, &err) != name.size()) {
        return false; // (a name that cannot be read differs)
      }
    }
    return run.filter_out_reads.count(name) != 0;
  };
  bool finished = false;
  std::vector<uint32_t> sb, idx;
  for (size_t bi = 0; bi < res.batches.size() && !finished; ++bi) {
    ResidentBatch& rb = res.batches[bi];
    const uint32_t n = (uint32_t)rb.lens.size();
    // reads named in filter_out_reads (a -f list, or a failing read of the same name) are not classified
    // (read_hashing.cpp:35-42): they become skipped records of the run behind them.  The kept reads, with the records
    // skipped in front of each (dropped reads included); runs of consecutive kept reads go to the classifier one after
    // the other — every read kept: the one run [0, n)
    sb.assign(n, 0);
    idx.clear();
    uint32_t carry = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (filtered(rb, i)) {
        carry += rb.skipped_before[i] + 1;
      } else {
        sb[i] = rb.skipped_before[i] + carry;
        carry = 0;
        idx.push_back(i);
      }
    }
    const uint32_t trailing = carry + rb.skipped_after;
    sink.resident = &rb;
    int rc = GRP_OK;
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
    if (sink.golden) {
      sink.golden->cut(run, rb.reads); // (the settle point: no window is parked, every commit of the batch is written)
    }
    run.vt.reads_free(rb.reads);
    rb.reads = nullptr;
    if (rc != GRP_OK) {
      std::cerr << "goldrush-path: " << cls.error() << std::endl;
      return 1;
    }
  }
  sink.resident = nullptr;
  if (sink.deferred) {
    deferred.say_trace(run);
  }
  if (finished) {
    run.out.flush();
    return sink.deferred && input_error() ? 1 : 0; // exit(0) inside silver_path_check (:173-176); (a fetch that failed is an error)
  }
  return -1;
}

int
classify_source(PathRun& run, Classifier& cls, SinkState& sink)
{
  const Opts& opt = run.opt;
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
      const uint8_t why = b.rec[i].seq_len < opt.min_length ? 1 : !run.filter_out_reads.empty() && run.filter_out_reads.count(b.id_str(i)) ? 2 : 0;
      if (why == 0) {
        sel.push_back((uint32_t)i);
        skipped_before.push_back(skipped);
        skipped = 0;
        continue;
      }
      ++skipped;
      if (opt.debug) {
        skipped_recs.emplace_back((uint32_t)i, why);
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
    if (sink.golden) {
      sink.golden->cut(run, h);
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
  return -1;
}

} // namespace gr
