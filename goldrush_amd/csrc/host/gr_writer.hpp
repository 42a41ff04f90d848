// The classification sinks: what writes a committed read (goldrush_path.cpp:996-1002, 1055-1070, 182-184) — from the batch
// in hand, read back from a plain file, or, the written records of compressed inputs, fetched in batches (Deferred).
#pragma once
#include "gr_resident.hpp"

#include <deque>

namespace gr {

struct Deferred;
struct GoldenCarry; // (gr_golden.hpp)

// what the classifier's callbacks get as their user pointer
struct SinkState
{
  PathRun* run = nullptr;
  const Batch* batch = nullptr;
  const std::vector<uint32_t>* sel = nullptr;
  // reads kept on the device: the record's text comes from the input file
  const ResidentBatch* resident = nullptr;
  Resident* res = nullptr;
  Deferred* deferred = nullptr; // the resident run has compressed inputs: the commits are written in batches
  GoldenCarry* golden = nullptr; // --golden_path, the first stage: what is written is remembered for the second
  std::vector<char> text;
  std::string upper;
  std::string bam_seq, bam_qual; // a BAM record's written slice as text
  // --debug: the records that are not classified, in file order ({record, 1 = too short / 2 = filtered}),
  // and for every classified read the number of them in front of it
  const std::vector<std::pair<uint32_t, uint8_t>>* skipped = nullptr;
  const std::vector<uint32_t>* skipped_before = nullptr;
  size_t skipped_done = 0;
};

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
struct Deferred
{
  struct Pending
  {
    RecLoc loc;
    grp_read_decision dec;
  };
  static constexpr size_t kMaxUnits = size_t(1) << 20;
  std::vector<Pending> pend; // in commit order
  std::deque<double> sums;   // of the records written, not yet asked for by the settle hook
  void flush(SinkState& st);
  void say_trace(const PathRun& run) const; // GRP_TRACE_INGEST: the "resident fetch" line

private:
  bool fetch_some(SinkState& st, size_t& i, size_t e);
  uint64_t n_flushes = 0, n_units_inflated = 0, n_text_bytes = 0, n_records = 0, n_trimmed = 0, n_straddling = 0, n_out_bytes = 0;
  std::vector<FetchItem> items;
  FetchPlan plan;
  std::vector<uint8_t> comp, dict;
  std::vector<grp_bgzf_block> blocks;
  std::vector<grp_gzip_segment> segs;
  std::vector<grp_fetch_record> recs;
  std::vector<char> out, text;
  std::vector<double> got_sums;
};

// the classifier's callbacks (grpath_host.h), user = a SinkState
double commit_sink(void* user, const gr_commit* c);
void settle_sink(void* user, double* out_sums, uint32_t n);
void rollover_sink(void* user, uint64_t new_path);
void debug_sink(void* user, uint32_t read);
// --debug: what process_read prints for the records [from, to) of SinkState::skipped (goldrush_path.cpp:907-932)
void debug_skipped(const SinkState& st, size_t from, size_t to);

} // namespace gr
