// --golden_path: what stage A of the run (the silver paths) remembers of the records it writes, so that stage B (the golden
// path over those records) needs neither their text nor a second engine.  Every record A commits is a whole read or a
// tile-aligned slice of one that sits packed on the device at that moment: its slice is cut out of the batch the classifier
// has just run over (grp_reads_gather) and kept as a small part; where the record went in its silver file, the hash of its
// written id and the two Phred sums of its written qualities are kept beside it.  Behind A the engine is rewound
// (grp_rewind) and B's reads are gathered from the parts; the text of what B writes is read back from the silver files.
// Where any of this cannot be done the run reads the silver files back instead, and says why.
#pragma once
#include "gr_resident.hpp"

namespace gr {

struct GoldenRec
{
  uint32_t out_file;    // which of PathRun::out_files of stage A the record went to
  RecLoc loc;           // where it lies there (its file index: set when stage B numbers its inputs)
  uint64_t name_hash;   // FNV-1a of the written id ("<id>_trimmed" / "<id>_untrimmed")
  double sum, first;    // Phred sums of the written qualities: all of them, and the first half (calc_phred_average's chain)
  uint32_t part, index; // its bases: read `index` of parts[part]
};

struct GoldenCarry
{
  bool on = false;  // the device route is still possible
  bool done = false; // stage A has ended well (at the end of its input, or where the reference does exit(0))
  std::string why;  // ... or why not
  std::vector<grp_read_slice> pending; // the slices of the commits since the last cut, in commit order
  std::vector<GoldenRec> recs;         // the records written, in commit order
  size_t n_cut = 0;                    // of which so many have their part
  std::vector<void*> parts;
  uint64_t part_bytes = 0, max_bytes = 0;
  void* ctx = nullptr; // the engine, handed from stage A to stage B
  uint64_t filter_size = 0;
  uint64_t n_batches = 0; // of stage B's fill
  uint64_t n_written = 0; // records stage A wrote (counted on either route)

  // in front of stage A: may the device route be taken at all?
  void decide(const PathRun& run);
  void give_up(const PathRun& run, const std::string& reason);
  void free_parts(const PathRun& run);
  // commit_sink / the writers: a committed read's written slice; the record as it went to the file
  void note_commit(const PathRun& run, uint32_t read, uint32_t seq_len, const grp_read_decision& d);
  void note_written(const PathRun& run, uint64_t id_off, const char* id, size_t id_len, bool trimmed, size_t n_seq, const char* qual, size_t n_qual);
  // behind the classifier's runs over `reads`, in front of its release: the pending slices become a part
  void cut(const PathRun& run, void* reads);
};

// Stage B on the device route, in the places of calc_min_phred_threshold and fill_bit_vector (gr_passes.hpp): the median
// of the first 50 000 records' averages from the stored sums; the fill pass over the stored records — the Phred filters,
// the names of failing records, the --verbose counts — with the passing ones gathered from the parts into batches that
// stay on the device (res).  `files`: stage B's inputs, run.files.
void golden_order(GoldenCarry& g, const std::vector<std::string>& a_out_files, const std::vector<std::string>& files);
int golden_phred_threshold(PathRun& run, const GoldenCarry& g);
int golden_fill(PathRun& run, Resident& res, GoldenCarry& g);

} // namespace gr
