// --golden_path on the device route (gr_golden.hpp).
#include "gr_golden.hpp"
#include "gr_fastq.hpp"
#include "gr_params.hpp"
#include "gr_passes.hpp"

#include <cstring>
#include <functional>
#include <iomanip>

namespace gr {

void
GoldenCarry::decide(const PathRun& run)
{
  on = true;
  const char* cap = getenv("GRP_RESIDENT_MAX_GB"); // (the cap of the reads kept between the passes holds for the parts too)
  max_bytes = (uint64_t)((cap ? atof(cap) : 100.0) * (double)(1ull << 30));
  const char* e = getenv("GRP_GOLDEN_RESIDENT");
  if (e && !strcmp(e, "off")) {
    give_up(run, "GRP_GOLDEN_RESIDENT=off");
  } else if (run.opt.debug) {
    give_up(run, "--debug");
  } else if (run.opt.ntcard) {
    give_up(run, "--ntcard (the second stage's filter may differ in size from the first's)");
  } else if (!run.ext.reads_gather || !run.ext.rewind) {
    give_up(run, "the engine has no grp_reads_gather / grp_rewind");
  }
}

void
GoldenCarry::free_parts(const PathRun& run)
{
  for (void* p : parts) {
    run.vt.reads_free(p);
  }
  parts.clear();
  part_bytes = 0;
}

void
GoldenCarry::give_up(const PathRun& run, const std::string& reason)
{
  if (on) {
    why = reason;
  }
  on = false;
  free_parts(run);
  pending.clear();
  recs.clear();
  n_cut = 0;
}

void
GoldenCarry::note_commit(const PathRun& run, uint32_t read, uint32_t seq_len, const grp_read_decision& d)
{
  if (!on) {
    return;
  }
  // untrimmed: (read, 0, len); trimmed: the substr of goldrush_path.cpp:1055-1062
  const WrittenSlice w = written_slice(run.opt.tile_length, seq_len, seq_len, d);
  pending.push_back(grp_read_slice{ 0, read, (uint32_t)w.off, (uint32_t)w.n_seq });
}

void
GoldenCarry::note_written(const PathRun& run, uint64_t id_off, const char* id, size_t id_len, bool trimmed, size_t n_seq, const char* qual, size_t n_qual)
{
  ++n_written;
  if (!on) {
    return;
  }
  const char* suffix = trimmed ? "_trimmed" : "_untrimmed";
  const size_t n_suffix = strlen(suffix);
  uint64_t h = fnv1a(id, id_len); // ... continued over the suffix
  for (size_t i = 0; i < n_suffix; ++i) {
    h = (h ^ (unsigned char)suffix[i]) * 1099511628211ull;
  }
  GoldenRec r{};
  r.out_file = (uint32_t)(run.out_files.size() - 1);
  const uint32_t wid = (uint32_t)(id_len + n_suffix);
  // "@<id><suffix>\n<bases>\n+\n<qualities>\n": everything relative to the id
  r.loc = RecLoc{ 0, id_off, wid, wid + 1, (uint32_t)n_seq, (uint64_t)wid + 1 + n_seq + 3, (uint32_t)n_qual, 0 };
  r.name_hash = h;
  r.sum = sum_phred(qual, n_qual);
  r.first = sum_phred(qual, n_qual / 2);
  recs.push_back(r);
}

void
GoldenCarry::cut(const PathRun& run, void* reads)
{
  if (!on || pending.empty()) {
    pending.clear();
    return;
  }
  if (recs.size() - n_cut != pending.size()) {
    give_up(run, "a record of the first stage was not written");
    return;
  }
  void* part = nullptr;
  const void* src = reads;
  const int rc = run.ext.reads_gather(run.ctx, &src, 1, pending.data(), (uint32_t)pending.size(), &part);
  if (rc != GRP_OK) {
    give_up(run, rc == GRP_ERR_NOMEM ? "no device memory for the silver reads (grp_reads_gather)" : std::string("grp_reads_gather failed: ") + (run.vt.last_error ? run.vt.last_error(run.ctx) : ""));
    return;
  }
  for (size_t i = 0; i < pending.size(); ++i) {
    recs[n_cut + i].part = (uint32_t)parts.size();
    recs[n_cut + i].index = (uint32_t)i;
    part_bytes += ((uint64_t)pending[i].n_bases + 15) / 16 * 4;
  }
  parts.push_back(part);
  n_cut = recs.size();
  pending.clear();
  if (part_bytes + recs.size() * sizeof(GoldenRec) > max_bytes) {
    give_up(run, "the silver reads exceed GRP_RESIDENT_MAX_GB");
  }
}

void
golden_order(GoldenCarry& g, const std::vector<std::string>& a_out_files, const std::vector<std::string>& files)
{
  // the records as the files order them: the files by name, commit order inside a file
  std::vector<uint32_t> file_of(a_out_files.size(), UINT32_MAX);
  for (size_t o = 0; o < a_out_files.size(); ++o) {
    for (size_t f = 0; f < files.size(); ++f) {
      if (files[f] == a_out_files[o]) {
        file_of[o] = (uint32_t)f;
      }
    }
  }
  for (GoldenRec& r : g.recs) {
    r.loc.file = file_of[r.out_file];
  }
  std::stable_sort(g.recs.begin(), g.recs.end(), [](const GoldenRec& a, const GoldenRec& b) { return a.loc.file < b.loc.file; });
}

// calc_min_phred_threshold (gr_passes.cpp) over the stored sums: -m 0 excludes nothing
int
golden_phred_threshold(PathRun& run, const GoldenCarry& g)
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
  for (const GoldenRec& r : g.recs) {
    if (r.loc.seq_len < opt.min_length) {
      continue;
    }
    if (taken >= MEDIAN_SAMPLES_NEEDED) {
      if (++over >= opt.jobs) {
        break;
      }
      continue;
    }
    uint32_t avg = 0, delta = 0;
    phred_from_sums(r.sum, r.first, r.loc.qual_len, avg, delta);
    scores[taken++] = avg;
  }
  const size_t n = taken + over;
  std::sort(scores.begin(), scores.end(), std::greater<uint32_t>());
  opt.phred_min = std::max(MINIMUM_PHRED_THRESHOLD, scores[n / 2]);
  if (opt.verbose) {
    std::cerr << "Minimum phred score calculated with median: " << opt.phred_min << std::endl;
  }
  return -1;
}

// fill_bit_vector (gr_passes.cpp) over the stored records
int
golden_fill(PathRun& run, Resident& res, GoldenCarry& g)
{
  const Opts& opt = run.opt;
  std::cerr << "inserting bit vector" << std::endl;
  const double s_time = now_s();
  // the reads stay on the device, their files are plain: what Resident::decide leaves for such inputs
  res.on = true;
  res.all = false;
  res.kind.assign(run.files.size(), Resident::PLAIN);
  res.bam.assign(run.files.size(), 0);
  res.max_bytes = g.max_bytes;
  const char* e = getenv("GRP_INGEST_CHUNK");
  const uint64_t chunk = e && atoll(e) > 0 ? (uint64_t)atoll(e) : (uint64_t)256 << 20; // a batch: the records of one chunk of text, as the ingest cuts them
  FillCounts n;
  std::vector<grp_read_slice> slices;
  std::string name;
  uint32_t lead_skipped = 0;
  for (size_t i = 0; i < g.recs.size();) {
    size_t end = i;
    uint64_t bytes = 0;
    while (end < g.recs.size() && g.recs[end].loc.file == g.recs[i].loc.file) { // (a batch never spans two files)
      const uint64_t rec_bytes = g.recs[end].loc.qual_rel + g.recs[end].loc.qual_len + 2;
      if (end > i && bytes + rec_bytes > chunk) {
        break;
      }
      bytes += rec_bytes;
      ++end;
    }
    slices.clear();
    ResidentBatch keep;
    uint32_t skipped = 0;
    for (; i < end; ++i) { // filter_batch (gr_passes.cpp); other characters than ACGT: the first stage wrote none
      const GoldenRec& r = g.recs[i];
      ++n.num_reads;
      ++skipped;
      if (r.loc.seq_len < opt.min_length) {
        ++n.by_length;
        continue;
      }
      uint32_t avg = 0, delta = 0;
      phred_from_sums(r.sum, r.first, r.loc.qual_len, avg, delta);
      const bool low = avg < opt.phred_min, hairpin = delta >= opt.phred_delta;
      if (low || hairpin) {
        if (opt.verbose) {
          n.by_phred += low ? 1 : 0;
          n.by_delta += hairpin ? 1 : 0;
        }
        int err = 0;
        name.resize(r.loc.id_len);
        const int fd = res.fd_of(run, r.loc.file);
        if (fd < 0 || pread_full(fd, &name[0], name.size(), r.loc.off, &err) != name.size()) {
          note_input_failure("cannot read the record at byte " + std::to_string(r.loc.off) + " back from " + run.files[r.loc.file]);
        } else {
          run.filter_out_reads.insert(name);
        }
        continue;
      }
      ++n.num_passed_reads;
      slices.push_back(grp_read_slice{ r.part, r.index, 0, r.loc.seq_len });
      keep.skipped_before.push_back(skipped - 1);
      keep.loc.push_back(r.loc);
      keep.name_hash.push_back(r.name_hash);
      keep.lens.push_back(r.loc.seq_len);
      skipped = 0;
    }
    if (slices.empty()) {
      if (!res.batches.empty()) {
        res.batches.back().skipped_after += skipped;
      } else {
        lead_skipped += skipped;
      }
      continue;
    }
    // the second use of the gather: whole reads out of many parts
    if (run.ext.reads_gather(run.ctx, g.parts.data(), (uint32_t)g.parts.size(), slices.data(), (uint32_t)slices.size(), &keep.reads) != GRP_OK) {
      return run.fail_engine("gathering the silver reads");
    }
    ++g.n_batches;
    keep.skipped_after = skipped;
    const uint32_t n_sel = (uint32_t)slices.size();
    res.batches.push_back(std::move(keep));
    if (run.vt.bv_insert(run.ctx, res.batches.back().reads, 0, n_sel) != GRP_OK) {
      return run.fail_engine("bit-vector insert");
    }
  }
  if (!res.batches.empty() && lead_skipped) {
    res.batches.front().skipped_before.front() += lead_skipped;
  }
  g.free_parts(run); // (waits for the gathers)
  const int counted = say_fill_counts(run, n);
  if (counted != -1) {
    return counted == -2 ? -1 : counted;
  }
  if (run.vt.sync(run.ctx) != GRP_OK) {
    return run.fail_engine("bit-vector insert");
  }
  std::cerr << "finished inserting bit vector" << std::endl;
  std::cerr << "in " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  return -1;
}

} // namespace gr
