// The record sources of goldrush-path (gr_passes.cpp): a pass over the input hands out batches of consecutive FASTQ
// records, their Phred statistics and the selected ones as packed reads on the device.  HostSource reads and packs on
// the host (engines without the ingest entry points); GpuSource hands raw text chunks to the engine (grpath_ingest.h),
// from plain text, gzip through zlib, BGZF members or the segments of an indexed gzip file (gr_source.cpp).
// A BAM input (gr_bam.hpp) is read as its FASTQ twin by either source — with GRP_BAM_ALIGNED=on (PathRun::bam_accept) as
// its aligned twin: secondary and supplementary records passed over, reverse-strand records read backwards.
// A run may have several input files (PathRun::files), of any of these formats: one source reads them one after the other
// in a pass, each to its own end, and hands out their records as those of one file that holds them in that order.
#pragma once
#include "../../../include/grpath_host.h"
#include "gr_bam.hpp"
#include "gr_gzidx.hpp"
#include "gr_gzwalk.hpp"
#include "gr_opts.hpp"
#include "gr_units.hpp"

#include <cstddef>
#include <cstdint>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

namespace gr {

double now_s(); // steady clock, seconds

struct PathRun
{
  Opts opt;
  grp_engine_vt vt{};
  grp_engine_ext ext{}; // the optional entry points behind the table's 48 (gr_path_main_ext)
  void* ctx = nullptr;
  std::vector<std::string> seeds;
  std::unordered_set<std::string> filter_out_reads;
  std::ofstream out;
  std::vector<std::string> out_files; // every file `out` was opened on, in order (rank 0): what a --golden_path run reads back
  uint32_t world = 1, rank = 0; // ranks sharing the classification windows (one process per GPU)
  // several ranks: every rank hashes the reads of its share of the batches into its bit vector, the
  // vectors are OR-merged before the rank build (round 3: the CLI's fill is no longer replicated)
  bool shard_fill = false;   // batch b belongs to rank b % world
  bool merge_rccl = false;   // ... merged by RCCL inside the engine (else staged through host memory and /dev/shm)
  void* shm = nullptr;       // gr_shm_allgather handle
  int32_t device = -1;       // HIP device ordinal of this rank
  // the files the run reads, in order: every -i, ".fofn" lists expanded (expand_inputs).  A pass reads them one after the
  // other through ONE source; a batch never spans two of them
  std::vector<std::string> files;
  // a plain gzip input: the restart points the first pass that read that file to its end wrote down (gr_gzidx.hpp); the
  // passes behind it inflate its segments on the device.  One per file, each built, dropped and used on its own
  std::vector<std::shared_ptr<GzIndex>> gzidx;
  // GRP_GZIP_WALK=on (read_options): in front of the first source of the run, the indexes of all its plain gzip files are
  // built on the device, the files side by side (gr_gzwalk.hpp), so that the first pass reads them through segments too
  bool gzip_walk = false, gzip_walked = false; // the switch; the walk has had its turn
  // GRP_GZIP_WALK_MEMBERS=on, GRP_GZIP_WALK_STREAMS (read_options): the walk also begins streams at the members behind a
  // file's first, so that a file of many members (cat *.fastq.gz) is walked side by side like many files
  GzWalkMembers gzip_walk_members;
  // a BGZF input: the members the last pass over that file walked, if it walked them to the file's end (BgzfFeed); a file
  // whose last pass did not go through the member feed, or left it for zlib at a member that is not BGZF, has none
  std::vector<std::shared_ptr<BgzfMap>> bgzf_map;
  // GRP_BAM_ALIGNED=on: BAM_REFUSED_FLAGS, the flags a BAM input is read with instead of refused (0: unaligned BAM only).
  // Per file, what the first pass that read it to its end met of them: said once, on rank 0, behind that pass
  uint32_t bam_accept = 0;
  struct BamAligned
  {
    uint64_t skipped = 0, reversed = 0; // secondary / supplementary records passed over, reverse-strand records read backwards
    bool counted = false, said = false; // a pass has read the file to its end; its line has been written
  };
  std::vector<BamAligned> bam_aligned;
  // a source, at the end of a file it has read from its first byte to its last
  void note_bam_aligned(size_t file, uint64_t skipped, uint64_t reversed);
  // behind a pass: one line per BAM file that held such records (ranks other than 0 are silent)
  void say_bam_aligned();

  int fail_engine(const char* what)
  {
    std::cerr << "goldrush-path: " << what << ": " << (vt.last_error ? vt.last_error(ctx) : "engine error") << std::endl;
    return 1;
  }
};

// A batch of consecutive FASTQ records of one file; offsets are relative to `text`.
struct Rec
{
  size_t id_off, id_len, seq_off, seq_len, qual_off, qual_len;
  bool reversed = false; // a BAM batch: a reverse-strand record of an aligned file, read backwards (seq_off / qual_off: the stored bytes)
};

struct Batch
{
  const char* text = nullptr;
  size_t file = 0;                  // which of PathRun::files the records come from
  uint64_t base_off = 0;            // offset of text[0] in that file's (decompressed) stream
  std::vector<Rec> rec;
  std::vector<uint32_t> avg, delta; // calc_phred_average, valid where stats() ran
  std::vector<uint8_t> non_acgt;    // find_first_not_of("ACGTacgt") != npos
  bool seq_is_upper = false;        // the host reader folds case while copying
  // `text` is a chunk of BAM records (gr_bam.hpp): seq_off = a record's 4-bit bases, qual_off = its raw Phred bytes; the
  // name is text as it stands.  What reads a record's bases or qualities goes through seq_text / qual_text.
  bool bam = false;
  std::string id_str(size_t i) const { return std::string(text + rec[i].id_off, rec[i].id_len); }
  // bases [from, from + n) of a record as the characters of its FASTQ form (`tmp`: where they are decoded to, if they must
  // be); a reversed record: the slice counts in the twin's coordinates
  const char* seq_text(const Rec& r, size_t from, size_t n, std::string& tmp) const
  {
    if (!bam) {
      return text + r.seq_off + from;
    }
    tmp.resize(n);
    if (r.reversed) {
      bam_decode_bases_rev(reinterpret_cast<const uint8_t*>(text + r.seq_off), r.seq_len, from, n, &tmp[0]);
    } else {
      bam_decode_bases(reinterpret_cast<const uint8_t*>(text + r.seq_off), from, n, &tmp[0]);
    }
    return tmp.data();
  }
  const char* qual_text(const Rec& r, size_t from, size_t n, std::string& tmp) const
  {
    if (!bam) {
      return text + r.qual_off + from;
    }
    tmp.resize(n);
    if (r.reversed) {
      (void)bam_decode_quals_rev(reinterpret_cast<const uint8_t*>(text + r.qual_off), r.qual_len, from, n, &tmp[0]);
    } else {
      (void)bam_decode_quals(reinterpret_cast<const uint8_t*>(text + r.qual_off) + from, n, &tmp[0]); // (the parse has refused what has no character)
    }
    return tmp.data();
  }
};

class RecordSource
{
public:
  virtual ~RecordSource() {}
  virtual bool ok() const = 0;
  virtual bool is_fastq() = 0; // a format this program reads: FASTQ, or unaligned BAM (read as its FASTQ twin)
  virtual bool next(Batch& b) = 0;
  // Phred statistics (and the ACGT check) of the records with seq_len >= min_len
  virtual void stats(Batch& b, size_t min_len, bool need_acgt) = 0;
  // the selected records as a batch of packed reads on the device
  virtual int upload(Batch& b, const std::vector<uint32_t>& sel, std::vector<uint32_t>& lens, void** reads) = 0;
};

// GpuSource where the engine has the ingest entry points (GRP_HOST_INGEST: no), else HostSource
std::unique_ptr<RecordSource> open_source(PathRun& run);
// Several inputs: every one of them looked at before the first pass.  Empty: all can be read (FASTQ, BAM, a file without a
// byte, or something that is no regular file and shows what it is when it is read); else the line that names the first
// file that cannot be opened or is neither FASTQ nor BAM.
std::string check_inputs(const PathRun& run);

} // namespace gr
