/*
 * grpath_host.h — C ABI of libgrpath_host.so: the host side of GoldRush-Path
 * that sits above the engine ABI (grpath.h).  It mirrors the reference host
 * (the .cpp files under goldrush_path/) function by function so the parity tests can call the
 * product's host logic directly; the `goldrush-path` CLI is built from the
 * same sources.  Pure C++17 (no HIP): the engine is reached through the
 * function table grp_engine_vt, whose members have exactly the signatures of
 * grpath.h (opaque handles as void*).
 */
#ifndef GRPATH_HOST_H
#define GRPATH_HOST_H

#include "grpath.h"
#include "grpath_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- engine function table (filled with the grp_* symbols of grpath.h) ---- */
typedef struct
{
  int (*create)(const grp_params*, void** ctx_out);
  void (*destroy)(void* ctx);
  const char* (*last_error)(const void* ctx);
  int (*reads_upload)(void* ctx, const uint32_t* packed, const uint64_t* word_off, const uint32_t* len, uint32_t n_reads, void** out);
  void (*reads_free)(void* reads);
  int (*bv_insert)(void* ctx, const void* reads, uint32_t first, uint32_t count);
  int (*finalize)(void* ctx, uint64_t* pop);
  int (*query_tiles)(void* ctx, const void* reads, uint32_t first, uint32_t count, grp_tile_summary* tiles, grp_id_count* lists, uint64_t list_cap, uint64_t* list_used, grp_query_stats* stats);
  int (*insert_tiles)(void* ctx, const void* reads, uint32_t read_idx, uint32_t tile_start, uint32_t tile_end, uint32_t id);
  int (*reset_ids)(void* ctx);
  int (*sync)(void* ctx);
  /* optional (may be NULL): query + decision on the device, grp_classify_reads */
  int (*classify_reads)(void* ctx, const void* reads, uint32_t first, uint32_t count, const grp_decide_params* params, grp_read_decision* out);
  /* optional (may be NULL): all ID blocks of one read at once, grp_insert_read */
  int (*insert_read)(void* ctx, const void* reads, uint32_t read_idx, uint32_t tile_start, uint32_t tile_end, uint32_t block_tiles, uint32_t first_id, uint32_t id_offset);
  /* optional (both or none): pipelined windows, grp_classify_reads_begin / _end */
  int (*classify_begin)(void* ctx, const void* reads, uint32_t first, uint32_t count, const grp_decide_params* params, uint32_t slot);
  int (*classify_end)(void* ctx, uint32_t slot, grp_read_decision* out);
  /* optional (all four or none): streaming windows, grp_classify_stream_* */
  int (*stream_begin)(void* ctx, const void* reads, uint32_t first, uint32_t count, const grp_decide_params* params, uint32_t slot, uint32_t stripe_reads, uint32_t n_owners, uint32_t owner, const grp_read_decision** decisions); /* grp_classify_stream_begin_striped */
  int (*stream_abort)(void* ctx, uint32_t slot);
  int (*stream_poll)(void* ctx, uint32_t slot);
  int (*stream_end)(void* ctx, uint32_t slot, uint32_t* reads_decided);
  /* optional (all four or none): a window of reads committed as one batch, grp_batch_* */
  int (*batch_insert)(void* ctx, const void* reads, const grp_batch_insert* inserts, uint32_t n_inserts, uint32_t block_tiles, uint32_t first_read);
  int (*batch_classify)(void* ctx, const void* reads, uint32_t first, uint32_t count, const grp_decide_params* params, const uint32_t* id_floor, grp_read_decision* out);
  int (*batch_undo)(void* ctx, uint32_t from_read, uint32_t id_floor);
  int (*batch_end)(void* ctx);
  /* optional (all four or none): --ntcard on the device, grp_ntcard_* / grp_set_filter_size */
  int (*ntcard_begin)(void* ctx, uint32_t sbits);
  int (*ntcard_add)(void* ctx, const void* reads, uint32_t first, uint32_t count, const uint32_t* stale_extra);
  int (*ntcard_finish)(void* ctx, uint64_t* zero_buckets);
  int (*set_filter_size)(void* ctx, uint64_t m);
  /* optional (all four or none): FASTQ ingest on the device, grpath_ingest.h */
  int (*fastq_parse)(void* ctx, const char* text, uint64_t n_bytes, int final_chunk, void** fq_out, uint64_t* n_records, uint64_t* bytes_consumed, int* stopped);
  int (*fastq_records)(void* fq, grp_fastq_record* out);
  int (*fastq_pack)(void* ctx, void* fq, const uint32_t* sel, uint32_t n_sel, void** reads_out);
  void (*fastq_free)(void* fq);
  /* optional (both, with the stream_* members; round 3): a window that waits where it parks and
   * applies the insert the host commits itself, grp_classify_stream_begin_resumable / _insert;
   * stream_end may then return 1 (the insert posted last was not applied) */
  int (*stream_begin_resumable)(void* ctx, const void* reads, uint32_t first, uint32_t count, const grp_decide_params* params, uint32_t slot, const grp_read_decision** decisions);
  int (*stream_insert)(void* ctx, uint32_t slot, uint32_t read_idx, uint32_t tile_start, uint32_t tile_end, uint32_t block_tiles, uint32_t first_id, uint32_t id_offset, uint32_t* generation);
  /* optional (round 3): the fill sharded over the ranks of one node, the bit vectors OR-merged —
   * through RCCL inside the engine (comm_unique_id / comm_init / bv_merge_ranks, all three or none)
   * or, where the ranks cannot form a communicator, staged through host memory (bv_words /
   * bv_export_words / bv_or_words, all three or none; the host exchanges the words) */
  int (*comm_unique_id)(void* out, size_t cap);
  int (*comm_init)(void* ctx, const void* unique_id, uint32_t world, uint32_t rank);
  int (*bv_merge_ranks)(void* ctx);
  int (*bv_words)(const void* ctx, uint64_t* n_words32);
  int (*bv_export_words)(void* ctx, uint64_t first, uint64_t n_words32, uint32_t* words);
  int (*bv_or_words)(void* ctx, uint64_t first, uint64_t n_words32, const uint32_t* words);
  /* optional: page-lock / release the chunk buffer handed to fastq_parse (grp_fastq_pin / _unpin) */
  int (*fastq_pin)(void* ctx, const char* buffer, uint64_t n_bytes);
  int (*fastq_unpin)(void* ctx);
  /* optional (with the batch_* members; round 4): the second decisions of a batch from the batch's own
   * records instead of a second query, grp_batch_verify */
  int (*batch_verify)(void* ctx, const void* reads, uint32_t first, uint32_t count, uint32_t extra, const grp_decide_params* params, const uint32_t* id_floor, grp_read_decision* out);
  /* optional (round 4): per read of a range the closest read in front of it that it overlaps, grp_window_overlap —
   * where most of the reads insert the classifier ends its batches in front of such reads */
  int (*window_overlap)(void* ctx, const void* reads, uint32_t first, uint32_t count, uint32_t threshold, uint32_t* prev_out);
  /* optional (all three, with stream_insert; round 5): striped windows that apply inserts themselves — the ranks of a
   * multi-GPU run keep their launches across an insert, grp_classify_stream_begin_striped_resumable /
   * grp_classify_stream_resumable; stream_end may then also return 2 (a wait inside the launch timed out) */
  int (*stream_begin_striped_resumable)(void* ctx, const void* reads, uint32_t first, uint32_t count, const grp_decide_params* params, uint32_t slot, uint32_t stripe_reads, uint32_t n_owners, uint32_t owner, const grp_read_decision** decisions);
  int (*stream_resumable)(void* ctx, uint32_t slot);
  int (*stream_insert_done)(void* ctx, uint32_t slot); /* grp_classify_stream_insert_done */
  /* optional (with the fastq_* members; round 5): the next chunk's upload started ahead of its parse, grp_fastq_prefetch */
  int (*fastq_prefetch)(void* ctx, const char* text, uint64_t n_bytes);
  /* optional (round 6): the occupancy the filter was sized for (-o): the phase-2 tables are allocated beside the fill, grp_set_occupancy_hint */
  int (*occupancy_hint)(void* ctx, double occupancy);
} grp_engine_vt;

/* ---- pure functions --------------------------------------------------------- */
/* make_seed_pattern (spaced_seeds.cpp:7-69): h NUL-terminated strings, `stride`
 * bytes apart, into out.  log_to_stderr != 0 prints the reference's messages. */
int gr_make_seed_pattern(const char* preset, unsigned k, unsigned weight, unsigned h, char* out, size_t stride, int log_to_stderr);
/* hash universe (goldrush_path.cpp:1113-1121), single-precision product */
uint64_t gr_hash_universe(uint64_t weight, uint64_t genome_size, uint64_t hash_num);
/* MIBloomFilter::calcOptimalSize (MIBloomFilter.hpp:94-101) */
uint64_t gr_calc_optimal_size(uint64_t entries, unsigned hash_num, double occupancy);
/* calc_phred_average / sum_phred (calc_phred_average.cpp:8-58) */
void gr_calc_phred_average(const char* qual, size_t n, uint32_t* avg, uint32_t* delta);
double gr_sum_phred(const char* qual, size_t n);
/* 2-bit packing of one read into ceil(n/16) words; returns 0, or -1 if the read
 * holds a non-ACGT character */
int gr_pack_2bit(const char* seq, size_t n, uint32_t* out_words);
/* --ntcard host arithmetic (goldrush_path/ntcard.hpp): nts::sBits for the input size
 * (:177-178); compEst's F0 from the zero buckets of the two sample tables (:124-136,
 * :232); and a record with non-ACGT characters cut into the ACGT runs (>= k bases; k = the span of seed 0, -k - 1 at odd -k)
 * grp_ntcard_add takes, with the iterator's stale repeats per run and seed
 * (extra[run*h + s]).  gr_ntcard_split returns the number of runs (writes at most cap). */
unsigned gr_ntcard_sbits(uint64_t input_bytes);
uint64_t gr_ntcard_f0(uint64_t zero0, uint64_t zero1, unsigned sbits);
size_t gr_ntcard_split(const char* seq, size_t n, unsigned k, unsigned h, uint64_t* run_off, uint64_t* run_len, uint32_t* extra, size_t cap);
/* process_options (goldrush_path/opt.cpp:89-217) on argv; writes one "name=value" line per
 * option into out (for the parity tests).  Returns -1 when the run would continue,
 * otherwise the exit code the reference exits with (messages go to stdout / stderr). */
int gr_process_options_dump(int argc, char** argv, char* out, size_t cap);
/* The inputs of a run as process_options and the expansion of ".fofn" lists see them: "input=" (the last -i), one
 * "inputs=" line per -i in command-line order, one "file=" line per file read, in order — or "error=" and the text that
 * names the list that is unreadable, empty or nested.  Returns as above, 1 for such a list. */
int gr_inputs_dump(int argc, char** argv, char* out, size_t cap);
/* CPUs this process may use: min(affinity mask, cgroup cpu.max quota) */
unsigned gr_effective_cpus(void);

/* ---- tile decision (goldrush_path.cpp:628-889, 195-233, 341-527, 960-1040) - */
typedef grp_read_decision gr_read_decision; /* see grpath.h */

/* decision of one read from its tile summaries (list_off indexes `lists`) */
void gr_decide_read(size_t threshold, size_t unassigned_min, size_t assigned_max, size_t num_tiles, const grp_tile_summary* tiles, const grp_id_count* lists, gr_read_decision* out);
/* the intermediate results, for the parity tests: ids/bools have num_tiles entries */
size_t gr_smooth_tiles(size_t num_tiles, const grp_tile_summary* tiles, const grp_id_count* lists, size_t threshold, uint32_t* ids_out, uint8_t* bools_out);
void gr_find_longest_stretch(const uint8_t* bools, size_t num_tiles, long* start, long* end);
int gr_eval_flanks(long longest_start, long longest_end, const uint32_t* ids, size_t num_tiles, size_t* trim_start, size_t* trim_end);

/* ---- order-exact classifier (process_read + silver_path_check) ------------- */
typedef struct
{
  uint32_t struct_size;
  uint32_t tile_length;   /* -t */
  uint32_t block_size;    /* -b */
  uint32_t threshold;     /* -x */
  uint32_t unassigned_min; /* -u */
  uint32_t assigned_max;  /* -a */
  uint32_t kmer_size;     /* -k */
  uint32_t hash_num;      /* -h */
  uint64_t target_bases;  /* uint64(r * G), goldrush_path.cpp:1223 */
  uint64_t max_paths;     /* -M */
  int32_t silver_path;    /* --silver_path */
  int32_t verbose;
  uint32_t max_window;    /* speculation window cap (reads); 0 = default */
  uint32_t world, rank;   /* ranks sharing each window (1, 0 = single GPU) */
  int32_t debug;          /* --debug: reads are decided one by one on the host and the reference's per-read
                             lines and per-pass tile-state dumps go to stderr (goldrush_path.cpp:109-124, 938-1086) */
  uint32_t seed0_span;    /* span of seed 0: kmer_size, or kmer_size - 1 at odd k (make_seed_pattern); a tile has
                             tile_length + kmer_size - seed0_span frames (the "Total queries" count).  0 = kmer_size.
                             A struct_size that ends in front of this field is accepted (0). */
} gr_classifier_params;

/* one committed read, in file order */
typedef struct
{
  uint32_t read;        /* index in the batch */
  gr_read_decision dec;
  uint32_t first_id;    /* ids_inserted after its ++ (ID of the first block) */
  uint64_t path;        /* curr_path the read was written to */
} gr_commit;

/* called for every classified read in order; returns sum_phred of what it wrote
 * (only used for the verbose per-path log) */
typedef double (*gr_commit_fn)(void* user, const gr_commit* c);
/* called when a silver path rolls over (new output file) */
typedef void (*gr_rollover_fn)(void* user, uint64_t new_path);
/* all-gather of `bytes` per rank (rank r's block at recv + r*bytes); NULL for world==1 */
typedef int (*gr_allgather_fn)(void* user, const void* send, uint64_t bytes, void* recv);

/* ---- node-local all-gather through /dev/shm (what the ranks of a multi-GPU classification
 * exchange: 32-byte decision records, a few KB per call) ---------------------------------
 * _open   rank 0 creates /dev/shm/grp_<key>, the others attach; returns NULL on failure /
 *         after timeout_s.  All `world` ranks of one node call it with the same key.
 * gr_shm_allgather has the signature of gr_allgather_fn with user = the handle.
 * _close  detaches; rank 0 removes the file. */
void* gr_shm_allgather_open(uint32_t world, uint32_t rank, const char* key, double timeout_s);
int gr_shm_allgather(void* handle, const void* send, uint64_t bytes, void* recv);
void gr_shm_allgather_close(void* handle);

/* ---- the fill of several ranks merged into every rank's bit vector (csrc/host/gr_ranks.cpp) -------
 * One implementation for the goldrush-path binary and bench.py's N > 1 runs.  All three are COLLECTIVE over the ranks of
 * `shm` (gr_shm_allgather_open).  _plan: how the ranks will merge — GR_MERGE_RCCL inside the engine (one GPU per rank:
 * grp_comm_unique_id / grp_comm_init, the communicator is up on return), GR_MERGE_STAGED through host memory and /dev/shm
 * (ranks sharing a device, engines without RCCL), GR_MERGE_NONE (every rank fills every read); every decision is taken by
 * all ranks alike.  _run: the merge, between the ranks' fills and finalize — 0 done, 1 an engine call failed, 2 the
 * exchange failed.  gr_ranks_same_u64: 1 if every rank holds `value` (the population behind the merge), 0 / -1. */
#define GR_MERGE_NONE 0
#define GR_MERGE_STAGED 1
#define GR_MERGE_RCCL 2
int gr_fill_merge_plan(const grp_engine_vt* vt, void* ctx, void* shm, uint32_t world, uint32_t rank, int device);
int gr_fill_merge_run(const grp_engine_vt* vt, void* ctx, void* shm, uint32_t world, uint32_t rank, int plan);
int gr_ranks_same_u64(void* shm, uint32_t world, uint64_t value);
/* 1: at least two ranks run on the same device (then their persistent launches must share it: one workgroup per CU each,
 * GRP_STREAM_WGS_PER_CU), 0: none do, -1: the exchange failed.  Collective. */
int gr_ranks_share_device(void* shm, uint32_t world, int device);

typedef struct gr_classifier gr_classifier;

int gr_classifier_create(const gr_classifier_params* p, const grp_engine_vt* vt, void* engine_ctx, gr_classifier** out);
void gr_classifier_destroy(gr_classifier* c);
void gr_classifier_set_callbacks(gr_classifier* c, gr_commit_fn commit, gr_rollover_fn rollover, gr_allgather_fn allgather, void* user);
/* --debug: called (with the commit callbacks' user pointer) in front of every read that is classified:
 * the host prints what the reference prints there — the skipped records before it, "name:", "num tiles:" */
typedef void (*gr_debug_fn)(void* user, uint32_t read);
void gr_classifier_set_debug(gr_classifier* c, gr_debug_fn fn);
/* The Phred sums of the insert commits handed over later than their commits (a host that writes its records in batches —
 * fetched from a compressed input, say — knows them only once a batch is written).  With `fn` set the commit callback's
 * return value is ignored; the classifier counts the insert commits (kinds 2 and 4: the reads that are written) and calls
 * fn(user, sums, n) for the n of them since the last call, oldest first, wherever the path's sum is looked at or zeroed: at
 * the top of a silver path's rollover (in front of its log line and the rollover callback; the run may finish there) and
 * at the end of every gr_classifier_run[_range].  fn fills sums[0, n) (zeroed before the call); they are added left to
 * right — the additions the undeferred form makes, in its order, so phred_sum_in_path and "Average Phred" are
 * bit-identical to it.  fn == NULL: the commit callback's return value is added at the commit, as before. */
typedef void (*gr_settle_fn)(void* user, double* sums, uint32_t n);
void gr_classifier_set_settle(gr_classifier* c, gr_settle_fn fn, void* user);
/* A witness of the decisions that costs nothing per read: the commits of the reads [first0, first0 + count0) and
 * [first1, first1 + count1) — numbers in the batch of reads handed to gr_classifier_run[_range] — are kept inside
 * the classifier (whether or not a commit callback is set) and handed out by gr_classifier_kept_commits (returns
 * how many there are, writes at most cap).  bench.py compares them with the oracle's serial loop on the same reads. */
void gr_classifier_keep_commits(gr_classifier* c, uint32_t first0, uint32_t count0, uint32_t first1, uint32_t count1);
size_t gr_classifier_kept_commits(const gr_classifier* c, gr_commit* out, size_t cap);
/* the all-gather with its own user pointer (e.g. gr_shm_allgather + its handle) */
void gr_classifier_set_allgather(gr_classifier* c, gr_allgather_fn allgather, void* allgather_user);
/*
 * Classify reads [0, n_reads) of an uploaded batch, in order, exactly as the
 * reference's serial process_read loop would (goldrush_path.cpp:1229-1256):
 * speculative windows are queried on the GPU, committed in order, and
 * everything after a read that inserts is queried again.  skipped_before[i]
 * (may be NULL) = number of non-eligible records (too short / filtered) that
 * precede read i in the file since the previous eligible read — they only
 * advance the read counter (:907-932); skipped_after likewise for the tail.
 * Returns GRP_OK, or a negative grp_status.  *finished is set when the
 * reference would have exit(0)'d (path M complete, :173-176).
 */
int gr_classifier_run(gr_classifier* c, void* reads, const uint32_t* lens, uint32_t n_reads, const uint32_t* skipped_before, uint32_t skipped_after, int* finished);
/* same for reads [first, first+count) of the batch; lens / skipped_before are
 * indexed by the read's number in the batch */
int gr_classifier_run_range(gr_classifier* c, void* reads, const uint32_t* lens, uint32_t first, uint32_t count, const uint32_t* skipped_before, uint32_t skipped_after, int* finished);
const char* gr_classifier_error(const gr_classifier* c);

typedef struct
{
  uint64_t valid_reads, total_tiles, assigned_tiles, unassigned_tiles, queries, hits, misses, num_reads_in_path;
  double phred_sum_in_path;
  uint64_t inserted_bases, curr_path;
  uint32_t id, ids_inserted;
  /* speculation statistics */
  uint64_t windows, reads_queried, reads_committed, inserts;
  /* wall-clock split of gr_classifier_run: engine calls for the windows vs ordered commit */
  double seconds_windows, seconds_commit;
  /* windows committed as batches (grp_batch_*): batches checked, batches ended early, reads committed through them */
  uint64_t batches, batches_undone, batch_reads;
  uint64_t batches_refused; /* batches the engine refused (GRP_ERR_NOMEM): committed the classic way */
  /* round 3: batches whose first decisions came out of the previous batch's second-query launch; inserts a
   * streaming window applied inside its own launch (grp_classify_stream_insert) */
  uint64_t batches_fused, stream_inserts;
  /* round 4: inserts a parked window did not apply (applied the classic way; parked windows are tried again after 64
   * clean windows), windows begun again because their launch had left without deciding a read (idle limit) */
  uint64_t stream_insert_fallbacks, stream_relaunches;
  uint64_t stream_handbacks; /* records a streaming window handed back to the synchronous path (kind 0: a read of more tiles than the
                                in-launch decision holds, a tile that needed the worst-case table) */
  uint64_t stream_rollovers; /* silver mode (round 4): inserts a parked window did not apply itself because the silver path rolls over behind them (the ID array is reset: the launches end there) */
  uint64_t batch_overlap_cuts; /* windows of batches ended in front of a read grp_window_overlap named (round 4) */
  uint64_t overlap_calls;      /* grp_window_overlap calls (one per block of 4096 reads where it is asked) */
} gr_classifier_state;
void gr_classifier_get_state(const gr_classifier* c, gr_classifier_state* out);

/* ---- the input reader (what btllib::SeqReader's file handling is to goldrush_path.cpp:235-339) --
 * Reads `path` (plain text by pread — requests of >= 32 MiB by several threads — or gzip / a pipe
 * through zlib) in requests of `request_bytes` into dst[0..cap).  Returns the bytes delivered
 * (the whole input if it fits cap), UINT64_MAX if the file cannot be opened.  Test hook of the
 * CLI's chunk reader. */
uint64_t gr_input_read(const char* path, uint64_t request_bytes, char* dst, uint64_t cap);

/* ---- BGZF input (csrc/host/gr_bgzf.cpp) ----------------------------------------------------------------------------
 * walk the gzip members in [buf, buf+n): fills blocks (payload offset/len, ISIZE, CRC32) while they are BGZF
 * members (FEXTRA with a 'B','C',SLEN=2 subfield, CM=8) that lie completely inside the buffer; returns their
 * number, *consumed = bytes they span, *why = 0 more data needed / 1 end of buffer (or `cap` blocks found) / 2 a member
 * that is not BGZF (other flags than FEXTRA, no BC subfield, an ISIZE above 65536: zlib's business) */
size_t gr_bgzf_scan(const unsigned char* buf, size_t n, grp_bgzf_block* blocks, size_t cap, size_t* consumed, int* why);

/* ---- plain gzip input (csrc/host/gr_gzidx.cpp): the restart points the first pass over a .gz file writes down -------------
 * gr_gzidx_build reads `path` as the host program's first pass does (zlib, Z_BLOCK), with a point every `span` bytes of
 * text and the index dropped beyond max_bytes; stop_after != 0: it stops once that much text has come out (the index is
 * then incomplete, like the Phred pass's).  The text goes to text_out[0, text_cap) if given.  NULL: the file cannot be
 * opened.  _info: [0] the index is complete, [1] segments, [2] bytes of text read, [3] bytes the index holds,
 * [4] it was dropped (the cap, bytes behind the last member), [5] the read failed (grp_last_error has no part in this: the
 * failure is the host program's input failure), [6] the longest segment's text, [7] the file's size.
 * _segment: segment i with comp_bit counted from the FILE's first bit and dict_off 0; its dict_len bytes of history go
 * to dict (32768 bytes of room).  _matches: the file at `path` still has the size and time the index was built from. */
typedef struct gr_gzidx gr_gzidx;
gr_gzidx* gr_gzidx_build(const char* path, uint64_t span, uint64_t max_bytes, uint64_t stop_after, char* text_out, uint64_t text_cap);
void gr_gzidx_info(const gr_gzidx* h, uint64_t out[8]);
int gr_gzidx_segment(const gr_gzidx* h, uint64_t i, grp_gzip_segment* seg, unsigned char* dict);
int gr_gzidx_matches(const gr_gzidx* h, const char* path);
void gr_gzidx_free(gr_gzidx* h);

/* ---- unaligned BAM input (csrc/host/gr_bam.hpp) -------------------------------------------------------------------------
 * A BAM file is read as its FASTQ twin: per record "@<name up to its NUL>\n<bases by =ACMGRSVTWYHKDBN>\n+\n<qual + 33>\n".
 * gr_bam_header: the header at the front of buf[0, n): 1 complete (*header_bytes = where the first record begins), 0 more
 * bytes needed, -1 not BAM.  gr_bam_walk: the record chain of buf[0, n), which begins at a record — the walk the engine's
 * grp_bam_parse performs: up to `cap` complete records into recs (all offsets from buf), *n_records of them found,
 * *consumed = the bytes they span; 0, or -1 with *bad_offset = the refused record and *why = the reason: a block_size
 * smaller than the record's fields, l_read_name 0, a name without NUL, flag 0x10 / 0x100 / 0x800, and with final_chunk a
 * stream that ends inside a record.  gr_bam_decode: l_seq bases and l_seq quality characters of one record; -1: a
 * quality without a FASTQ character (0xFF, above 93).
 * The aligned twin (GRP_BAM_ALIGNED=on; what `samtools fastq -n` writes with its default filters, written down from the SAM
 * specification and samtools' documented behaviour): gr_bam_walk_ex is the walk with `accept`, a subset of 0x910 (any other
 * bit: -1) — a record with a flag bit of 0x910 outside `accept` is refused as by gr_bam_walk (accept 0 is gr_bam_walk), one
 * with an accepted 0x100 / 0x800 is checked, consumed, counted in *skipped and not written to recs (*consumed may be > 0
 * with *n_records 0), one with an accepted 0x10 is written with its flag.  gr_bam_decode_twin: bases and quality characters
 * [from, from + n) of one record as the aligned twin has them — flag 0x10: base j = the complement of stored base
 * l_seq-1-j (the 4-bit code bit-reversed), quality j = qual[l_seq-1-j] + 33, the slice in twin coordinates; else the
 * stored order.  -1: a quality without a FASTQ character in the slice, or a slice outside the record. */
typedef struct
{
  uint64_t off, name_off, seq_off, qual_off, end; /* block_size field, name, 4-bit bases, qualities, the next record */
  uint32_t l_read_name, l_seq, flag;
  uint32_t id_len; /* the name up to its NUL, cut at the first whitespace */
} gr_bam_record;
int gr_bam_header(const unsigned char* buf, uint64_t n, uint64_t* header_bytes);
int gr_bam_walk(const unsigned char* buf, uint64_t n, int final_chunk, gr_bam_record* recs, uint64_t cap, uint64_t* n_records, uint64_t* consumed, uint64_t* bad_offset, const char** why);
int gr_bam_decode(const unsigned char* buf, const gr_bam_record* rec, char* seq_out, char* qual_out);
int gr_bam_walk_ex(const unsigned char* buf, uint64_t n, int final_chunk, uint32_t accept, gr_bam_record* recs, uint64_t cap, uint64_t* n_records, uint64_t* consumed, uint64_t* bad_offset, const char** why, uint64_t* skipped);
int gr_bam_decode_twin(const unsigned char* buf, const gr_bam_record* rec, uint64_t from, uint64_t n, char* seq_out, char* qual_out);

/* ---- optional engine entry points that came after grp_engine_vt was frozen at 48 members: a second table, every member
 * optional (NULL, or a struct_size that ends in front of it: the host takes the path it took without it) */
typedef struct
{
  uint32_t struct_size;
  /* grp_bgzf_inflate: with it, a BGZF-compressed input is inflated on the device (GRP_BGZF=off: through zlib as before) */
  int (*bgzf_inflate)(void* ctx, const uint8_t* comp, uint64_t n_comp, const grp_bgzf_block* blocks, uint32_t n_blocks, char* text_out, uint64_t text_cap, uint32_t* bad_block);
  /* grp_gzip_inflate: with it, the passes over a plain gzip input behind the first inflate the segments of the first
   * pass's index on the device (GRP_GZIP_INDEX=off: every pass through zlib as before) */
  int (*gzip_inflate)(void* ctx, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_segment* segs, uint32_t n_segs, char* text_out, uint64_t text_cap, uint32_t* bad_seg);
  /* grp_bam_parse: with it, the records of an unaligned BAM input are parsed and packed on the device, where text goes
   * through fastq_parse (the handle is served by the table's fastq_records / fastq_pack / fastq_free); without it a BAM
   * file takes the host reader */
  int (*bam_parse)(void* ctx, const char* bytes, uint64_t n_bytes, int final_chunk, void** out, uint64_t* n_records, uint64_t* bytes_consumed, uint64_t* bad_offset);
  /* grp_records_fetch: with it (and GRP_RESIDENT=all), the written records of a compressed input whose reads stayed on the
   * device are inflated, cut and formatted there; without it the host inflates their units through bgzf_inflate /
   * gzip_inflate above and formats them itself */
  int (*records_fetch)(void* ctx, int unit_kind, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const void* units, uint32_t n_units, const grp_fetch_record* recs, uint32_t n_recs, uint32_t out_flags,
                       char* out, uint64_t out_cap, double* sums, uint32_t* bad_unit, uint32_t* bad_record);
  /* grp_bam_parse_ex: with it (and GRP_BAM_ALIGNED=on), the records of an aligned BAM input are parsed and packed on the
   * device as the reads of its aligned twin; without it such a run's BAM files take the host reader, as BAM files do on an
   * engine without bam_parse */
  int (*bam_parse_ex)(void* ctx, const char* bytes, uint64_t n_bytes, int final_chunk, uint32_t accept, void** out, uint64_t* n_records, uint64_t* bytes_consumed, uint64_t* bad_offset, uint64_t* n_skipped);
  /* grp_reads_gather and grp_rewind (both or none): what a --golden_path run needs to hand the silver reads to its second
   * stage on the device and to build that stage's filter in the place of the first; without them the second stage reads
   * the silver files */
  int (*reads_gather)(void* ctx, const void* const* srcs, uint32_t n_srcs, const grp_read_slice* slices, uint32_t n_slices, void** out);
  int (*rewind)(void* ctx);
  /* grp_gzip_walk: with it (and GRP_GZIP_WALK=on), the restart points of the run's plain gzip files are found on the
   * device in front of the first pass, all files side by side (csrc/host/gr_gzwalk.hpp), and the first pass over them
   * inflates their segments through gzip_inflate too; without it that pass reads them through zlib and builds the index */
  int (*gzip_walk)(void* ctx, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n_steps, grp_gzip_walk_result* results, uint8_t* hist_out, char* text_out,
                   uint64_t text_cap, uint32_t* bad_step);
} grp_engine_ext;

/* The same index built by the engine's walk (csrc/host/gr_gzwalk.hpp; ext->gzip_walk on engine_ctx), the n files side by
 * side: out[i] is a handle like gr_gzidx_build's (_info: [2] the text the index describes, [4] the file was left to zlib,
 * [5] 0; _segment / _matches as above) — NULL where the file cannot be read as a regular file.  The sizes come from
 * GRP_GZIP_WALK_ROOM.  stats, if not NULL: files, walked, left to zlib, rounds, bytes of text decoded, launches, repeated
 * steps, microseconds.  -1: no walk in the table, or a bad argument.  _build_device: one file; NULL also without a walk.
 * _left: why the file was left to zlib (NULL: it was not), *status = the decoder's status where that was the reason. */
int gr_gzidx_build_device_many(const grp_engine_ext* ext, void* engine_ctx, const char* const* paths, uint32_t n, uint64_t span, uint64_t max_bytes, gr_gzidx** out, uint64_t stats[8]);
gr_gzidx* gr_gzidx_build_device(const grp_engine_ext* ext, void* engine_ctx, const char* path, uint64_t span, uint64_t max_bytes);
/* _many with the members of a file side by side (csrc/host/gr_gzwalk.hpp: GzWalkMembers; what GRP_GZIP_WALK_MEMBERS=on does in
 * the host program): members != 0 begins a stream at every gzip header found behind byte 0 of a file, ahead of the chain of
 * members from byte 0, which adopts the streams it arrives at and drops the others; at most GRP_GZIP_WALK_STREAMS (1024)
 * streams take steps at a time.  The indexes are those of _many, word for word.  members == 0 is _many.  stats: the eight
 * of _many, then candidates, streams begun, adopted, dropped, the most streams that took a step in one round, the bytes of
 * text dropped streams had decoded, the microseconds of the scan for candidates, 0.  _many itself reads neither variable. */
int gr_gzidx_build_device_many_ex(const grp_engine_ext* ext, void* engine_ctx, const char* const* paths, uint32_t n, uint64_t span, uint64_t max_bytes, int members, gr_gzidx** out, uint64_t stats[16]);
const char* gr_gzidx_left(const gr_gzidx* h, uint32_t* status);
/* The two pieces of the walk that need no engine.  _header_bytes: the gzip header at buf[0, n) as the walk parses it (FEXTRA,
 * FNAME, FCOMMENT, FHCRC with its CRC16): its length; 0: it does not end inside the n bytes; -1: not a header zlib takes
 * (magic, a method other than 8, a reserved flag, a header CRC that does not match).  _switch: GRP_GZIP_WALK as the host
 * program reads it: 1 on, 0 off or unset, -1 any other value (the run ends with status 1 before its first pass). */
long gr_gzip_header_bytes(const unsigned char* buf, size_t n);
int gr_gzip_walk_switch(void);
int gr_gzip_walk_members_switch(void); /* GRP_GZIP_WALK_MEMBERS, read the same way; without GRP_GZIP_WALK=on it has no effect */

/* ---- the CLI as a function (main of goldrush_path.cpp:1096-1275) ----------- */
int gr_path_main(int argc, char** argv, const grp_engine_vt* vt); /* = gr_path_main_ext(argc, argv, vt, NULL) */
int gr_path_main_ext(int argc, char** argv, const grp_engine_vt* vt, const grp_engine_ext* ext);

#ifdef __cplusplus
}
#endif
#endif
