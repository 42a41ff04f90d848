// libgrpath_hip.so — hand-written gfx950 (CDNA4) kernels + the C ABI of
// include/grpath.h.  Integer / bit-vector work, HBM-transaction bound: no MFMA.
// This file: context, launch logic and the exported functions; the kernels live in
// grp_kernels.inc (hot path), grp_ingest.inc (FASTQ), grp_inflate.inc (BGZF input), grp_ntcard.inc (--ntcard).
// The k_query launch is grp_query.inc, the streaming window's host side grp_stream.inc, the words the two sides of
// a launch hand each other grp_stream_proto.h.
//
// Kernels
//   k_fill        spaced-seed ntHash of every read position + test-and-set of
//                 bit (hash % m)           (goldrush_path.cpp:304-305,
//                 MIBFConstructSupport.hpp:134-147)
//   k_bucket_*    popcount prefix scan -> 64-byte buckets {rank, bitmap, IDs}
//                 (MIBFConstructSupport.hpp:165-181)
//   k_query       fused hash -> probe (bit+rank, then ID) -> per-frame ID
//                 dedup -> per-tile LDS count table -> top ID + count>2 list
//                 (read_hashing.cpp:29-54, goldrush_path.cpp:544-626)
//   k_insert      hash -> rank -> exact per-call rank dedup -> reservoir rule
//                 (MIBFConstructSupport.hpp:247-283)
// Seeds of spans 65 .. 256 bases (DevSeeds::wide == 2, long_span) run their own
// instantiation of every hashing kernel, WT == GRP_WT_LONG (DISPATCH_H_SPAN / DISPATCH_HW
// pick it); the forms of spans up to 64 are untouched.
#include "grp_buffers.h"
#include "grp_device.h"
#include "grp_stream_proto.h"
#include "host/gr_stream_stripes.hpp"
#include "host/gr_tile_geom.hpp"
#include "host/gr_tiles_core.hpp"
#include "host/gr_bam.hpp"
#include "host/gr_gather_word.hpp"

#include "../../include/grpath.h"
#include "../../include/grpath_ingest.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <cmath>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// ---------------------------------------------------------------------------
// host-side context
// ---------------------------------------------------------------------------

namespace {

thread_local std::string g_create_error;

struct EventPair
{
  Event a, b;
  int kind = 0;
};

} // namespace


// per-window device / pinned buffers of the query + decision kernels
struct QuerySlot
{
  DevBuf<grp_tile_summary> d_tiles;
  DevBuf<grp_id_count> d_lists;
  DevBuf<uint64_t> d_qctr; // [3] list arena cursor, [4] flagged tiles (kept zero between calls)
  uint64_t* h_qctr = nullptr; // pinned: the first 64 bytes of h_dec_raw (one copy brings counters and decisions, slot_dec_alloc)
  DevBuf<uint32_t> d_flag_idx;
  // decide scratch: one capacity for the three (slot_dec_scratch)
  DevBuf<uint32_t> d_dec_ids;
  DevBuf<uint8_t> d_dec_asg;
  DevBuf<uint64_t> d_dec_scratch;
  uint64_t d_dec_cap = 0;
  std::vector<uint32_t> h_long_reads; // reads of the window of more than 256 tiles: decided by a launch of their own (classify_enqueue_decide)
  DevBuf<uint32_t> d_long_reads;
  grp_read_decision* d_dec = nullptr; // = d_dec_raw + 2: two entries (64 bytes) in front of the decisions carry the window's counters
  grp_read_decision* h_dec = nullptr; // = h_dec_raw + 2, pinned
  DevBuf<grp_read_decision> d_dec_raw;
  HostBuf<grp_read_decision> h_dec_raw;
  // a window in flight (grp_classify_reads_begin)
  Event done;                  // decisions of the window are in h_dec
  Event qdone;                 // the window's query kernel has finished (decide stream waits on it)
  bool side_used = false;      // `done` was last recorded on the decide stream
  // streaming window (grp_classify_stream_*, grp_stream.inc); the words it shares with the launch: grp_stream_proto.h
  struct StreamWindow
  {
    HostBuf<grp_read_decision> h_sdec;      // mapped, coherent: the kernel publishes decisions here
    // abort flag: the host raises the one in mapped host memory (a plain store); every
    // 64th workgroup reads that one when it starts and relays it to the flag in DEVICE
    // memory, which is what all workgroups test (a PCIe round trip in every workgroup
    // costs the kernel 2.4x, measured; a 4-byte hipMemcpyAsync takes ~1.5 ms to land
    // beside a full-device kernel, measured)
    DevBuf<uint32_t> d_abort;               // ABORT_* words
    HostBuf<uint32_t> h_abort;              // mapped, coherent
    DevBuf<uint32_t> d_tiles_done;
    DevBuf<unsigned long long> d_executed;  // EXE_* counters
    HostBuf<unsigned long long> h_executed; // pinned
    bool streaming = false;
    // a streaming window that applies inserts itself (grp_classify_stream_insert)
    DevBuf<uint32_t> d_tile_ver; // round 6: per tile of a resumable window, the generation its summary belongs to (DevStreamCtl::tile_ver)
    DevBuf<uint32_t> d_rel;      // release words of a resumable window's grid-wide waits: a 128-byte line per workgroup (STREAM_REL_WGS of them)
    DevBuf<uint32_t> d_dbg;      // developer (GRP_STREAM_DEBUG): a state word per workgroup of the streaming launch
    DevBuf<uint32_t> d_sctl;     // SCT_* control block
    HostBuf<uint32_t> h_cmd;     // mapped, coherent: CMD_SEQ, then the command's CMD_* fields from CMD_FIELDS on
    HostBuf<uint32_t> h_ack;     // mapped, coherent: ACK_* words
    bool resumable = false;       // the window in flight takes grp_classify_stream_insert
    gr::stripes::Window stripes;  // its reads and whose they are (one owner: the whole window is this launch's)
    uint32_t gen = 1;             // generation of the records the host is waiting for
    uint32_t cmd_seq = 0;         // commands posted to the window in flight
    HostBuf<uint32_t> h_stripe_tiles; // pinned: this rank's tiles of a striped window
    DevBuf<uint32_t> d_stripe_tiles;
  } win;
  bool busy = false;
  const grp_reads* reads = nullptr;
  uint32_t first = 0, count = 0;
  grp_decide_params dp{};
  uint64_t list_cap = 0;
  uint64_t t0 = 0, nt = 0, probes = 0;
};

struct DevBatchView; // grp_kernels.inc

// state of a batch of inserts applied ahead of their reads' queries (grp_batch_*, grp_batch.inc)
struct BatchRun
{
  bool active = false;
  uint32_t n_ins = 0, block_tiles = 0;
  uint64_t n_units = 0, n_rec = 0;
  HostBuf<uint32_t> h_counters;   // page-locked [4]: records that own a chain, chained touches, log entries, error
  std::vector<uint32_t> h_ins;    // [n_ins][6]: read, tile_start, tile_end, first_id, id_offset, first unit
  HostBuf<uint32_t> h_ins_stage;  // page-locked copy of h_ins: the upload does not wait for the stream
  DevBuf<uint32_t> d_counters;    // two sets of 4: a batch's clean-up zeroes the NEXT batch's set (k_batch_clear)
  uint32_t ctr_set = 0;
  DevBuf<uint32_t> d_ins;
  uint32_t epoch = 0; // of the current / last batch: the claim field of the count words (grp_device.h), 1 .. GRP_EPOCH_MAX
  uint64_t tab_cap = 0, cur_cap = 0;    // allocated slots / slots the current batch uses (the three log tables)
  DevBuf<unsigned long long> d_rec_key; // records, one per (frame, seed) of the inserted tiles
  DevBuf<unsigned long long> d_rec_loc;
  DevBuf<unsigned long long> d_rec_old;
  DevBuf<uint32_t> d_rec_chain;
  uint64_t rec_cap = 0;
  DevBuf<uint32_t> d_ovf_next; // touches of a rank by other (read, block)s than its owner's, chained per record
  DevBuf<uint32_t> d_ovf_jb;
  DevBuf<uint32_t> d_chained;  // the records that own a chain (k_batch_apply walks these, not all records)
  uint64_t ovf_cap = 0;
  DevBuf<unsigned long long> d_log_keys;
  DevBuf<uint32_t> d_log_head;
  DevBuf<uint32_t> d_log_bits; // 1 bit per log table slot: something was logged with this home slot
  DevBuf<uint32_t> d_log_old;
  DevBuf<uint32_t> d_log_writer;
  DevBuf<uint32_t> d_log_next;
  DevBuf<uint32_t> d_log_slot; // log entry -> its slot in the log table (to clean it)
  uint64_t log_cap = 0;
  DevBuf<uint32_t> d_floor;    // grp_batch_classify: per read of the window
  // grp_batch_verify: the window's tiles with records, then the tiles queried again; per read its insert entry
  HostBuf<uint32_t> h_vf_stage; // page-locked: per read of the batch its insert entry, then the floors
  DevBuf<uint32_t> d_vf_stage;
  uint32_t first_read = 0;        // reads are numbered from here in the log
};

constexpr int FQ_TEXT_SLOTS = 3; // device text buffers of the FASTQ ingest (grp_ingest.inc)

// The stream handles are a base of the context: a base is destroyed after every member, so the buffers and events
// below free themselves in `delete c` while the streams still exist, and the streams go last.
struct CtxStreams
{
  hipStream_t stream = nullptr;
  // decision kernel + copy-back of a pipelined window run here, next to the following
  // window's query kernel on `stream`
  hipStream_t stream2 = nullptr;
  hipStream_t stream3 = nullptr; // the uploads of coming FASTQ chunks (grp_fastq_prefetch): a copy must not stand in front of the parse of the chunk before it
  ~CtxStreams()
  {
    for (hipStream_t s : { stream3, stream2, stream }) {
      if (s) {
        (void)hipStreamDestroy(s);
      }
    }
  }
};

struct grp_ctx : CtxStreams
{
  int device = 0;
  std::string arch;
  bool coherent_arch = false; // gfx942 / gfx950: agent-scope accesses are served by the memory side
  BatchRun batch;
  grp_params params{};
  std::vector<std::string> seeds;
  DevSeeds h_seeds{};
  DevBuf<DevSeeds> d_seeds;
  DevBuf<uint32_t> d_gtab; // count tables of k_query<..., GT> (query_geom: tiles whose worst case does not fit the LDS)
  DevFilter f{}; // the view the kernels take; the memory belongs to the owners below
  DevBuf<uint32_t> bv;
  DevBuf<uint4> buckets;
  DevBuf<ulonglong2> far;
  DevBuf<unsigned long long> ovf_keys;
  DevBuf<uint32_t> ovf_ids;
  uint64_t nsb = 0;      // superbuckets
  uint64_t n_bv_words = 0;
  uint64_t n_ovf = 0;    // IDs living in the overflow table
  uint64_t n_far = 0;    // count words living in the far table
  uint32_t uniform_weight = 0; // weight shared by all seeds, 0 if they differ

  // Developer switches and test hooks: every one the library reads, read once, when the context is created (read_switches;
  // not on every call of a latency path).  DESIGN.md has the table.
  struct Switches
  {
    bool no_direct = false;          // GRP_NO_DIRECT: grp_query_tiles takes the general path for small windows too
    bool stream_resume_off = false;  // GRP_STREAM_RESUME=off: every streaming window ends where it parks
    bool no_early_park = false;      // GRP_NO_EARLY_PARK (the engine-level API contract assumes it is not set)
    int trace_abort = 0;             // GRP_TRACE_ABORT: 1 = set, 2 = its value begins with '2' (every in-launch insert's phase times)
    uint32_t small_hist = 0;         // GRP_SMALL_HIST: slots of the first-step count table (forces the two-step scheme)
    uint32_t batch_epochs = GRP_EPOCH_MAX; // GRP_BATCH_EPOCHS (tests): batches between two sweeps of the claims
    int stream_keep = 2;             // GRP_STREAM_KEEP: fingerprint buffers per workgroup, 0 .. 2 (0: rounds 3 - 5's form)
    int stream_wgs_per_cu = 0;       // GRP_STREAM_WGS_PER_CU: resident workgroups per CU of a streaming launch (0: three)
    bool stream_debug = false;       // GRP_STREAM_DEBUG: a state word per workgroup of the streaming launch, dumped when a wait times out
    double stream_wait_s = 2.0;      // GRP_STREAM_WAIT_S: time limit of a grid-wide wait (seconds)
    bool verify_strict = false;      // GRP_VERIFY_STRICT: an impossible delta in grp_batch_verify ends the run
    long batch_ovf_cap = 0;          // GRP_BATCH_OVF_CAP (tests): a tiny chain store, so that batches are refused on the device
    uint32_t batch_overlap_shift = 59; // GRP_BATCH_OVERLAP_SHIFT (measurement): 60 = one sampled frame in 16, 59 = one in 32 ...
    bool batch_verify_off = false;   // GRP_BATCH_VERIFY=off: grp_batch_verify always takes the second query
    bool shared_halves_off = false;  // GRP_SHARED_HALVES=off: every seed of a frame hashed on its own
    bool debug_stats = false;        // GRP_DEBUG_STATS: grp_destroy prints the context's path counters
  } sw;
  // grp_window_overlap (grp_batch.inc): samples per tile, their table, the result per read
  struct OverlapBuf
  {
    DevBuf<unsigned long long> d_samples;
    DevBuf<uint32_t> d_n;
    DevBuf<unsigned long long> d_tab;
    DevBuf<uint32_t> d_prev;
  } ovl;
  uint64_t n_overlap_calls = 0;
  uint64_t n_batch_sweeps = 0; // times the batch epochs wrapped and the claims were swept out of the count words
  uint64_t n_stream_keep[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; // grp_debug_stream_stats
  uint64_t n_stream_idle_exits = 0, n_stream_coop_refused = 0; // parked windows that left by themselves (idle limit); resumable windows whose cooperative launch was refused
  uint64_t n_flagged_tiles = 0, n_flagged_distinct = 0, n_flagged_list = 0; // statistics: tiles redone with the worst-case table; why (distinct IDs / list length)
  uint64_t n_verify_impossible = 0;
  uint64_t n_verify_tiles = 0, n_verify_queried = 0, n_verify_flagged = 0, n_verify_fallbacks = 0, n_verify_uncertified = 0, n_verify_unpatched = 0; // grp_batch_verify: tiles patched from records / queried again / patched tiles redone / calls that took the second query
  uint64_t n_direct_windows = 0, n_direct_fallbacks = 0, n_general_windows = 0, n_redo_launches = 0; // GRP_DEBUG_STATS
  uint64_t n_chunks = 0; // rank-build chunks
  DevBuf<uint64_t> d_super;
  // grp_set_occupancy_hint: the phase-2 tables allocated by a helper thread while the fill runs (grp_finalize joins it)
  struct Prealloc
  {
    double occupancy = 0.0;
    bool started = false;
    std::thread worker;
    DevBuf<uint4> units;        // (written by the worker, read behind its join)
    uint64_t units_buckets = 0; // capacity in 128-byte units
    DevBuf<ulonglong2> far;     // slots: a power of two
  } pre;
  double finalize_times[6] = { 0, 0, 0, 0, 0, 0 };
  bool finalized = false;
  int n_cus = 0;
  std::mutex fill_mutex; // grp_bv_insert may be called from several host threads (the reference calls insertBV under `omp parallel`)
  // --ntcard pass (grp_ntcard.inc)
  DevBuf<uint32_t> d_ntc;
  uint32_t ntc_sbits = 0;
  DevBuf<uint2> d_ntc_chunks;
  DevBuf<uint32_t> d_ntc_extra;
  // query scratch: two slots so that a second window can be in flight while the
  // host commits the first (grp_classify_reads_begin / _end)
  QuerySlot slot[2];
  QuerySlot* q = &slot[0];
  // first decisions kept for grp_batch_verify: slot `slot` holds, from tile `tile_off` of its buffers on, the plain
  // tile summaries of reads [first, first + count) of `reads` against the filter as it is (as it was in front of the
  // batch, between grp_batch_insert_reads and grp_batch_end / _undo).  Dropped by whatever changes the filter or the slot.
  struct Carry
  {
    bool valid = false;
    uint32_t slot = 0;
    const grp_reads* reads = nullptr;
    uint32_t first = 0, count = 0;
    uint64_t tile_off = 0;
  } carry;
  const DevBatchView* view = nullptr; // set while grp_batch_classify enqueues its window
  HostBuf<grp_tile_summary> h_tiles; // pinned staging
  HostBuf<grp_id_count> h_lists; // pinned staging of the list prefix
  // small windows: kernel writes straight into mapped host memory
  HostBuf<grp_tile_summary> h_small_tiles;
  HostBuf<grp_id_count> h_small_lists;
  // insert scratch
  DevBuf<unsigned long long> d_dedup;
  uint32_t epoch = 0;
  // whole-read insert table: one capacity (ir_cap slots) for the four tables and the two changed-slot sets
  DevBuf<unsigned long long> d_ir_keys;
  DevBuf<unsigned long long> d_ir_masks;
  DevBuf<unsigned long long> d_ir_locs;
  DevBuf<uint32_t> d_ir_slots;
  DevBuf<uint32_t> d_ir_counter;
  uint32_t dbg_stream_lds = 0, dbg_stream_grid = 0; // developer (GRP_STREAM_DEBUG): the last streaming launch
  DevBuf<uint32_t> d_fp_tab[2]; // changed-slot sets of a streaming window's last two in-launch inserts (ir_cap words each)
  uint64_t ir_cap = 0;
  uint32_t ir_parity = 0;
  // RCCL communicator of a multi-GPU fill (grp_comm.inc), NULL on one GPU
  void* comm = nullptr;
  uint32_t comm_world = 1, comm_rank = 0;
  uint32_t n_comm_merges = 0; // grp_bv_merge_ranks calls that succeeded
  DevBuf<double> d_delog; // 10^(-Q/10) table for the FASTQ ingest
  DevBuf<double> d_delog_raw; // ... and for BAM records, whose quality bytes are Q itself (the same values, 33 entries apart)
  // buffers of the FASTQ ingest, kept between chunks (round 4: a chunk used to pay seven hipMalloc / hipFree pairs,
  // 256 MiB of text among them — every hipFree waits for the device)
  struct IngestPool
  {
    DevBuf<uint8_t> text[FQ_TEXT_SLOTS]; // the chunk being packed, the next one (uploaded ahead) and the one after (uploading)
    bool text_used[FQ_TEXT_SLOTS] = {};
    int last_slot = FQ_TEXT_SLOTS - 1; // the slot handed out last (the next one takes the one after it)
    // grp_fastq_prefetch: bodies of coming chunks on their way into slots, oldest first
    struct Pre
    {
      int slot = -1;
      const char* body = nullptr;
      uint64_t n_body = 0;
    } pre[2];
    int n_pre = 0;
    uint64_t n_dropped = 0; // prefetched bodies that were not followed by their parse (uploaded for nothing)
    DevBuf<uint32_t> d_counts;
    DevBuf<uint64_t> d_base, d_super, d_total, d_nl;
    DevBuf<uint8_t> d_rec; // grp_fastq_record[], in bytes
    HostBuf<uint64_t> h_bam_off; // ... page-locked, device-mapped staging of that table
    Event uploaded; // the chunk's text has arrived (copied on the side stream, beside the fill of the chunk before)
    // page-locked, device-mapped staging of a parse (grp_ingest.inc: ingest_stage): [0] newlines, [1] end of the last record
    HostBuf<uint64_t> h_scal;
    HostBuf<uint8_t> h_front; // the bytes in front of a prefetched body
    HostBuf<uint8_t> h_rec; // the record table
    Event text_up[FQ_TEXT_SLOTS];   // the slot's prefetched body has arrived (recorded on the copy stream)
    Event text_done[FQ_TEXT_SLOTS]; // the main stream's last use of the slot's text (grp_fastq_free records it: the next upload into the slot waits for it, not the host)
  } ingest;
  // grp_bgzf_inflate / grp_gzip_inflate (grp_inflate.inc): the compressed bytes, the histories (segments only), the
  // table with the text offsets, the text and the per-entry status words of one call; grown, never shrunk
  template <class Entry>
  struct InflatePool
  {
    DevBuf<uint8_t> d_comp, d_dict, d_text;
    DevBuf<Entry> d_entries;
    DevBuf<uint64_t> d_toff;
    DevBuf<uint32_t> d_status;
    HostBuf<Entry> h_entries; // page-locked staging
    HostBuf<uint64_t> h_toff;
    HostBuf<uint32_t> h_status;
    Event ev0, ev1; // around the two kernels
    uint64_t n_entries = 0, n_comp = 0, n_text = 0; // grp_debug_bgzf_stats / grp_debug_gzip_stats
    double kernel_us = 0.0;
  };
  InflatePool<grp_bgzf_block> bgzf;
  InflatePool<grp_gzip_segment> gzip;
  // grp_gzip_walk (grp_inflate.inc): beside the buffers above (its entries are InfWalkEntry, kept as bytes here) the
  // per-step answers and the 32 KiB of new history of every step; grown, never shrunk
  struct WalkPool
  {
    InflatePool<uint8_t> io;
    DevBuf<grp_gzip_walk_result> d_res;
    DevBuf<uint8_t> d_hist;
    HostBuf<grp_gzip_walk_result> h_res;
  } walk;
  // grp_records_fetch: the record table, the formatted records and their Phred sums of one call; grown, never shrunk
  struct FetchPool
  {
    DevBuf<grp_fetch_record> d_recs;
    DevBuf<uint8_t> d_out;
    DevBuf<double> d_sums;
  } fetch;
  DevBuf<uint32_t> d_crc_tab; // CRC32 slicing tables and x^(2^k), of both (inflate_crc_tables)
  const char* reg_text = nullptr; // the caller's text buffer, page-locked by grp_fastq_pin
  size_t reg_bytes = 0;
  uint32_t timing_mask = (1u << GRP_K_FILL) | (1u << GRP_K_RANK) | (1u << GRP_K_QUERY) | (1u << GRP_K_DECIDE) | (1u << GRP_K_QUERY_LAT) | (1u << GRP_K_VERIFY) | (1u << GRP_K_BATCH);
  // timing
  bool timing = true;
  std::vector<EventPair> pending;
  std::vector<EventPair> free_events;
  grp_kernel_stat kstat[GRP_K_COUNT]{};
  mutable std::string err;
};

// a source batch of grp_reads_gather as its kernel sees it (grp_gather.inc)
struct GatherSrc
{
  const uint32_t* packed;
  const uint64_t* word_off;
};

struct grp_reads
{
  grp_ctx* ctx = nullptr;
  uint32_t n_reads = 0;
  uint64_t n_words = 0;
  // what the batch owns: empty where the memory is the caller's (grp_reads_wrap_device: the bases) or a part of
  // d_slab (grp_fastq_pack: the index arrays); `dev` has the addresses either way
  DevBuf<uint32_t> d_packed;
  DevBuf<uint64_t> d_word_off;
  DevBuf<uint32_t> d_len;
  DevBuf<uint64_t> d_tile0;
  DevBuf<uint32_t> d_tile_read;
  DevBuf<uint64_t> d_chunk0;
  DevBuf<uint32_t> d_chunk_read;
  std::vector<uint64_t> tile0;  // host copy
  std::vector<uint64_t> chunk0; // host copy
  std::vector<uint32_t> len;    // host copy
  // grp_fastq_pack (round 5): one device allocation behind all index arrays, filled by asynchronous copies out of these
  // vectors — they live as long as the batch, so no call has to wait for a copy
  DevBuf<uint8_t> d_slab;
  std::vector<uint64_t> h_word_off, h_seq_off;
  std::vector<uint32_t> h_tile_read, h_chunk_read;
  // grp_reads_gather: the slices and the sources' addresses, likewise
  std::vector<grp_read_slice> h_slices;
  std::vector<GatherSrc> h_srcs;
  DevReads dev{};
};

namespace {

void comm_release(grp_ctx* c); // grp_comm.inc

int
set_err(const grp_ctx* ctx, int code, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) {
    ctx->err = buf;
  } else {
    g_create_error = buf;
  }
  return code;
}

#define HIP_TRY(ctx, expr)                                                                                             \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      return set_err(ctx, GRP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
    }                                                                                                                  \
  } while (0)

constexpr uint32_t FILL_CHUNK = 2048; // read positions per fill workgroup
constexpr uint64_t LIST_PREFIX = 8192; // list entries copied back together with the tile summaries
constexpr uint32_t SMALL_TILES = 512;  // windows up to this many tiles use the direct (zero-copy) path
constexpr uint32_t SMALL_STRIDE = 32;  // list entries per tile in the direct path
constexpr int THREADS = gr::geom::WG_THREADS;
// A HIP grid holds fewer than 2^32 work-items per dimension (larger ones are truncated
// modulo 2^32 without an error): no launch of 256-lane workgroups exceeds this many
constexpr uint32_t MAX_GRID_WGS = 1u << 22;

// ---- ntHash (btllib::SeedNtHash, restated; see DESIGN.md "Hash") -----------

uint64_t
srol_n(uint64_t x, unsigned d)
{
  const uint64_t M33 = 0x1FFFFFFFFULL, M31 = 0x7FFFFFFFULL;
  uint64_t lo = x & M33, hi = (x >> 33) & M31;
  unsigned rl = d % 33, rh = d % 31;
  if (rl) {
    lo = ((lo << rl) | (lo >> (33 - rl))) & M33;
  }
  if (rh) {
    hi = ((hi << rh) | (hi >> (31 - rh))) & M31;
  }
  return (hi << 33) | lo;
}

const uint64_t BASE_SEED[4] = { 0x3c8bfbb395c60474ULL, 0x3193c18562a02b4cULL, 0x20323ed082572324ULL, 0x295549f54be24456ULL };

} // namespace

#include "grp_kernels.inc"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

namespace {

struct Timer
{
  grp_ctx* c;
  EventPair ep;
  bool on = false;
  hipStream_t st;
  Timer(grp_ctx* ctx, int kind, uint64_t units, hipStream_t on_stream = nullptr)
    : c(ctx)
    , st(on_stream ? on_stream : ctx->stream)
  {
    c->kstat[kind].launches += 1;
    c->kstat[kind].units += units;
    if (!c->timing || !(c->timing_mask & (1u << kind))) {
      return;
    }
    if (!c->free_events.empty()) {
      ep = std::move(c->free_events.back());
      c->free_events.pop_back();
    } else if (ep.a.create(hipEventDefault) != hipSuccess || ep.b.create(hipEventDefault) != hipSuccess) {
      return;
    }
    ep.kind = kind;
    on = true;
    (void)hipEventRecord(ep.a, st);
  }
  ~Timer()
  {
    if (on) {
      (void)hipEventRecord(ep.b, st);
      c->pending.push_back(std::move(ep));
    }
  }
};

// accumulate the durations of the launches that have completed; launches still in
// flight (a pipelined next window) stay pending
void
drain_events(grp_ctx* c)
{
  std::vector<EventPair> keep;
  for (auto& ep : c->pending) {
    if (hipEventQuery(ep.b) != hipSuccess) {
      keep.push_back(std::move(ep));
      continue;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
      c->kstat[ep.kind].ms += (double)ms;
    }
    c->free_events.push_back(std::move(ep));
  }
  c->pending.swap(keep);
}

uint64_t
next_pow2_64(uint64_t v)
{
  uint64_t p = 1;
  while (p < v) {
    p <<= 1;
  }
  return p;
}

uint32_t
next_pow2(uint64_t v)
{
  uint32_t p = 1;
  while (p < v) {
    p <<= 1;
  }
  return p;
}

size_t
tab_bytes(const grp_ctx* c)
{
  return (size_t)c->h_seeds.h * c->h_seeds.wmax * 4u * sizeof(ulonglong2);
}

constexpr size_t
bases_bytes(uint32_t nbases)
{
  // words covering nbases at any 16-base phase + 2 pad words, rounded to 16 B
  size_t words = (nbases + 15u) / 16u + 1u + 4u;
  return ((words * 4u + 15u) / 16u) * 16u;
}

// seeds of spans beyond 64 bases (DevSeeds::wide == 2): every hashing kernel runs its long-span form (WT ==
// GRP_WT_LONG), the only code that reads bases past the 64th of a frame
inline bool
long_span(const grp_ctx* c)
{
  return c->h_seeds.wide > 1u;
}

// span of seed 0, the shortest seed: k, or k - 1 at odd k.  The tile geometry that follows from it is
// host/gr_tile_geom.hpp's; these are its functions for a context.
inline uint32_t
span0(const grp_ctx* c)
{
  return c->h_seeds.span[0];
}

inline uint32_t
tile_frames(const grp_ctx* c)
{
  return gr::geom::frames_per_tile(c->params.tile, c->params.k, span0(c));
}

// (k_insert, k_insert_collect, k_batch_collect walk a tile in these units)
inline uint32_t
tile_parts(const grp_ctx* c)
{
  return gr::geom::tile_parts(tile_frames(c));
}

inline gr::geom::TileExtent
tile_extent(const grp_ctx* c, uint32_t len, uint32_t ti)
{
  return gr::geom::tile_extent(c->params.tile, c->params.k, span0(c), len, ti);
}

template<typename K>
int
ensure_lds(grp_ctx* c, K kernel, size_t bytes)
{
  if (bytes > 64 * 1024) {
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  }
  return GRP_OK;
}

// k_decide's LDS work space: reads of more than 256 tiles (register forms above) up to DECIDE_LDS_MAX_TILES
inline uint32_t
decide_lds_tiles(const uint64_t* tile0, uint32_t count)
{
  uint64_t most = 0;
  for (uint32_t i = 0; i < count; ++i) {
    most = std::max(most, tile0[i + 1] - tile0[i]);
  }
  return most <= 4 * LANE_TILES ? 0u : (uint32_t)std::min<uint64_t>((most + 63) / 64 * 64, DECIDE_LDS_MAX_TILES);
}

inline size_t
decide_lds_bytes(uint32_t lds_tiles)
{
  return (size_t)lds_tiles * DECIDE_LDS_BYTES_PER_TILE;
}

// The kernel form of h seeds per frame: one instantiation per h up to 8, the many-seed form (GRP_H_MANY, grp_kernels.inc
// frame_seeds) for 9 .. 16.  Any other h has no kernel: an error (grp_create refuses it first).  Used inside functions
// that return a grp_status and have the context `c` at hand.
#define DISPATCH_H_CASES_FEW(CALL)                                                                                     \
    case 1: { constexpr int HH = 1; CALL; } break;                                                                     \
    case 2: { constexpr int HH = 2; CALL; } break;                                                                     \
    case 3: { constexpr int HH = 3; CALL; } break;                                                                     \
    case 4: { constexpr int HH = 4; CALL; } break;                                                                     \
    case 5: { constexpr int HH = 5; CALL; } break;                                                                     \
    case 6: { constexpr int HH = 6; CALL; } break;                                                                     \
    case 7: { constexpr int HH = 7; CALL; } break;                                                                     \
    case 8: { constexpr int HH = 8; CALL; } break;
#define DISPATCH_H(hval, CALL)                                                                                         \
  switch (hval) {                                                                                                      \
    DISPATCH_H_CASES_FEW(CALL)                                                                                         \
    case 9: case 10: case 11: case 12: case 13: case 14: case 15:                                                      \
    case 16: { constexpr int HH = GRP_H_MANY; CALL; } break;                                                           \
    default: return set_err(c, GRP_ERR_INVALID, "h=%u has no kernel form", (unsigned)(hval));                         \
  }
// the forms of h <= 8 only (the developer prototypes of grp_pshard.inc, which refuse more seeds first)
#define DISPATCH_H_FEW(hval, CALL)                                                                                     \
  switch (hval) {                                                                                                      \
    DISPATCH_H_CASES_FEW(CALL)                                                                                         \
    default: return set_err(c, GRP_ERR_INVALID, "h=%u has no kernel form here", (unsigned)(hval));                    \
  }

// The hash form of a launch, the kernels' WT parameter: GRP_WT_LONG for seeds of spans beyond 64 bases, the only form
// that reads them; else 16 for seeds that all have make_seed_pattern's default weight, where the kernel has that form —
// the care loop unrolled, in the kernels whose launches are latency-bound (k_insert_collect, k_batch_collect,
// k_batch_delta, k_ovl_sample); else 0, run-time weights.
inline int
hash_form(const grp_ctx* c, bool has_16)
{
  return long_span(c) ? GRP_WT_LONG : (has_16 && c->uniform_weight == 16) ? 16 : 0;
}

// CALL with WW, the hash form: DISPATCH_W_SPAN for the kernels of forms {0, LONG}, DISPATCH_W for those that have the
// weight-16 form as well (only the forms named here are compiled).  DISPATCH_H_SPAN / DISPATCH_HW: with HH beside it.
#define DISPATCH_W_SPAN(cc, CALL)                                                                                      \
  switch (hash_form(cc, false)) {                                                                                      \
    case GRP_WT_LONG: { constexpr int WW = GRP_WT_LONG; CALL; } break;                                                 \
    default: { constexpr int WW = 0; CALL; } break;                                                                    \
  }
#define DISPATCH_W(cc, CALL)                                                                                           \
  switch (hash_form(cc, true)) {                                                                                       \
    case GRP_WT_LONG: { constexpr int WW = GRP_WT_LONG; CALL; } break;                                                 \
    case 16: { constexpr int WW = 16; CALL; } break;                                                                   \
    default: { constexpr int WW = 0; CALL; } break;                                                                    \
  }
#define DISPATCH_H_SPAN(cc, CALL) DISPATCH_W_SPAN(cc, DISPATCH_H((cc)->params.h, CALL))
#define DISPATCH_HW(cc, CALL) DISPATCH_W(cc, DISPATCH_H((cc)->params.h, CALL))

// decision buffers of a slot: [64 bytes of counters][cap decisions], on the device and page-locked on the host
int
slot_dec_alloc(grp_ctx* c, QuerySlot& sl, uint64_t cap)
{
  static_assert(2 * sizeof(grp_read_decision) == 8 * sizeof(uint64_t), "the counters take two decision entries");
  clear_all(sl.d_dec_raw, sl.h_dec_raw);
  sl.d_dec = sl.h_dec = nullptr;
  sl.h_qctr = nullptr;
  HIP_TRY(c, sl.d_dec_raw.reset(cap + 2));
  HIP_TRY(c, sl.h_dec_raw.reset(cap + 2, hipHostMallocDefault));
  memset(sl.h_dec_raw, 0, 2 * sizeof(grp_read_decision));
  sl.d_dec = sl.d_dec_raw + 2;
  sl.h_dec = sl.h_dec_raw + 2;
  sl.h_qctr = reinterpret_cast<uint64_t*>(sl.h_dec_raw.p);
  return GRP_OK;
}

// room for `want` elements (DevBuf::ensure), a failure reported through the context
template<typename T>
int
ensure_dev(grp_ctx* c, DevBuf<T>& b, uint64_t want)
{
  HIP_TRY(c, b.ensure(want));
  return GRP_OK;
}

constexpr size_t LDS_PER_WORKGROUP = 160 * 1024 - 512; // gfx950, less the kernels' static shared variables
// The kernels that stage a fill chunk or one tile beside the seed tables (fill, ntCard, insert, batch records, overlap
// samples, tile-hash inspection): their LDS grows with the span, and fits at the longest span and tile there are
static_assert(GRP_DEV_MAX_H * GRP_DEV_MAX_W * 4u * sizeof(ulonglong2) + bases_bytes(GRP_MAX_TILE + GRP_MAX_SPAN + GRP_DEV_MAX_H) <= LDS_PER_WORKGROUP,
              "a tile of the longest span does not fit the LDS beside the seed tables");
} // namespace

#include "grp_query.inc"

namespace {

// the environment's switches (grp_ctx::Switches): the library's only getenv calls
grp_ctx::Switches
read_switches()
{
  grp_ctx::Switches s;
  const auto set = [](const char* name) { return getenv(name) != nullptr; };
  const auto off = [](const char* name) {
    const char* e = getenv(name);
    return e && !strcmp(e, "off");
  };
  s.no_direct = set("GRP_NO_DIRECT");
  s.stream_resume_off = off("GRP_STREAM_RESUME");
  s.no_early_park = set("GRP_NO_EARLY_PARK");
  if (const char* e = getenv("GRP_TRACE_ABORT")) {
    s.trace_abort = e[0] == '2' ? 2 : 1;
  }
  if (const char* e = getenv("GRP_SMALL_HIST")) {
    s.small_hist = (uint32_t)atoi(e) / 2u * 2u;
  }
  if (const char* e = getenv("GRP_BATCH_EPOCHS")) { // the claims are swept every n batches instead of every 1023
    s.batch_epochs = (uint32_t)std::min<long>(std::max<long>(atol(e), 1), (long)GRP_EPOCH_MAX);
  }
  if (const char* e = getenv("GRP_STREAM_KEEP")) {
    s.stream_keep = std::max(0, std::min(2, atoi(e)));
  }
  if (const char* e = getenv("GRP_STREAM_WGS_PER_CU")) {
    s.stream_wgs_per_cu = atoi(e);
  }
  s.stream_debug = set("GRP_STREAM_DEBUG");
  if (const char* e = getenv("GRP_STREAM_WAIT_S")) {
    s.stream_wait_s = atof(e);
  }
  s.verify_strict = set("GRP_VERIFY_STRICT");
  if (const char* e = getenv("GRP_BATCH_OVF_CAP")) {
    s.batch_ovf_cap = atol(e);
  }
  if (const char* e = getenv("GRP_BATCH_OVERLAP_SHIFT")) {
    s.batch_overlap_shift = (uint32_t)std::min(63, std::max(52, atoi(e)));
  }
  s.batch_verify_off = off("GRP_BATCH_VERIFY");
  s.shared_halves_off = off("GRP_SHARED_HALVES");
  s.debug_stats = set("GRP_DEBUG_STATS");
  return s;
}

int
build_seed_tables(grp_ctx* c)
{
  DevSeeds& sd = c->h_seeds;
  memset(&sd, 0, sizeof(sd));
  sd.h = c->params.h;
  sd.k = c->params.k;
  sd.wmax = 0;
  // seed s spans span0 + s bases, span0 = k or k - 1 (odd k: make_seed_pattern's halves are k/2 positions each,
  // spaced_seeds.cpp:27-66); the tile string is tile + k - 1 bases either way
  const size_t sp0 = c->seeds[0].size();
  if (sp0 == 0 || (sp0 != c->params.k && sp0 + 1 != c->params.k)) {
    return set_err(c, GRP_ERR_INVALID, "seed 0 has span %zu, expected k = %u or k-1 = %u", sp0, c->params.k, c->params.k - 1);
  }
  for (uint32_t s = 0; s < sd.h; ++s) {
    const std::string& p = c->seeds[s];
    if (p.size() != sp0 + s) {
      return set_err(c, GRP_ERR_INVALID, "seed %u has span %zu, expected k+%u = %u or k-1+%u = %u", s, p.size(), s, c->params.k + s, s, c->params.k - 1 + s);
    }
    sd.span[s] = (uint32_t)p.size();
    uint32_t w = 0;
    for (uint32_t q = 0; q < p.size(); ++q) {
      if (p[q] == '1') {
        if (w >= GRP_DEV_MAX_W) {
          return set_err(c, GRP_ERR_INVALID, "seed weight > %d unsupported", GRP_DEV_MAX_W);
        }
        sd.shift[s][w] = 2u * q;
        for (uint32_t b = 0; b < 4; ++b) {
          sd.tab[s][w][b].x = srol_n(BASE_SEED[b], sd.span[s] - 1u - q);
          sd.tab[s][w][b].y = srol_n(BASE_SEED[3u - b], q);
        }
        ++w;
      } else if (p[q] != '0') {
        return set_err(c, GRP_ERR_INVALID, "seed %u contains '%c'", s, p[q]);
      }
    }
    sd.weight[s] = w;
    sd.wmax = std::max(sd.wmax, w);
  }
  if (sd.wmax == 0) {
    return set_err(c, GRP_ERR_INVALID, "seeds have weight 0");
  }
  c->uniform_weight = sd.wmax;
  for (uint32_t s2 = 0; s2 < sd.h; ++s2) {
    if (sd.weight[s2] != sd.wmax) {
      c->uniform_weight = 0;
    }
  }
  // spans beyond 32 bases (round 4): the generic hash reads a second 64-bit window; the unrolled weight-16 form and
  // the shared halves are 32-base forms and stay off.  Beyond 64 bases (up to GRP_MAX_SPAN): the long-span
  // instantiations, which read each care position from the staged bases (long_span, grp_kernels.inc seed_hash_long).
  // The class comes from the longest actual span, span0 + h - 1 (k + h - 2 at odd k): k = 33 with one seed of 32 bases
  // hashes from the 32-base window, k = 65 with one seed of 64 from the 64-base one.
  const uint32_t span = sd.span[sd.h - 1];
  sd.wide = (span > 64) ? 2u : (span > 32) ? 1u : 0u;
  if (sd.wide) {
    c->uniform_weight = 0;
  }
  // make_seed_pattern's family (spaced_seeds.cpp:58-66): seed i = left || "0" x i || right with
  // left = the first k/2 positions of seed 0.  The query kernel then evaluates the halves once per
  // frame (GRP_SHARED_HALVES=off: developer switch, every seed on its own as before).
  sd.n_left = 0;
  {
    const std::string& s0 = c->seeds[0];
    const size_t cut = s0.size() / 2;
    bool family = sd.h >= 2 && !c->sw.shared_halves_off;
    for (uint32_t s2 = 1; s2 < sd.h && family; ++s2) {
      family = c->seeds[s2] == s0.substr(0, cut) + std::string(s2, '0') + s0.substr(cut);
    }
    uint32_t nl = 0;
    for (size_t q = 0; q < cut; ++q) {
      nl += s0[q] == '1';
    }
    if (family && nl > 0 && nl < sd.weight[0] && !sd.wide) {
      sd.n_left = nl;
    }
  }
  return GRP_OK;
}

} // namespace

extern "C" {

const char*
grp_last_error(const grp_ctx* ctx)
{
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int
grp_create(const grp_params* p, grp_ctx** out)
{
  if (!p || !out || p->struct_size != sizeof(grp_params)) {
    return set_err(nullptr, GRP_ERR_INVALID, "grp_create: bad params / struct_size");
  }
  *out = nullptr;
  if (p->h < 1 || p->h > GRP_MAX_SEEDS) {
    return set_err(nullptr, GRP_ERR_INVALID, "h=%u: this implementation supports 1 to %d spaced seeds", p->h, GRP_MAX_SEEDS);
  }
  if (p->k < 1 || p->k > GRP_MAX_SPAN || p->k + p->h - 1 > GRP_MAX_SPAN) {
    return set_err(nullptr, GRP_ERR_INVALID, "k=%u h=%u: the longest seed spans k+h-1=%u bases, this implementation supports spans of 1 to %d bases", p->k, p->h, p->k + p->h - 1, GRP_MAX_SPAN);
  }
  if (p->tile < p->k + p->h - 1) {
    return set_err(nullptr, GRP_ERR_INVALID, "tile length %u shorter than the longest seed span %u", p->tile, p->k + p->h - 1);
  }
  if (p->tile > GRP_MAX_TILE) {
    return set_err(nullptr, GRP_ERR_INVALID, "tile length %u: a tile holds at most 65 535 frames (an ID's count per tile is 16 bits)", p->tile);
  }
  // m = 0: the size is not known yet (--ntcard estimates it from the reads);
  // grp_set_filter_size() must follow before the first grp_bv_insert
  if (p->m != 0 && (p->m < 64 || p->m >= (1ULL << 50))) {
    return set_err(nullptr, GRP_ERR_INVALID, "filter size m=%llu unsupported", (unsigned long long)p->m);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    return set_err(nullptr, GRP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  }
  grp_ctx* c = new grp_ctx();
  c->params = *p;
  for (uint32_t s = 0; s < p->h; ++s) {
    c->seeds.emplace_back(p->seeds[s] ? p->seeds[s] : "");
  }
  c->params.seeds = nullptr;
  auto fail = [&](int code) {
    g_create_error = c->err;
    grp_destroy(c);
    return code;
  };
  if (p->device >= 0) {
    if (hipSetDevice(p->device) != hipSuccess) {
      set_err(c, GRP_ERR_NO_DEVICE, "hipSetDevice(%d) failed", p->device);
      return fail(GRP_ERR_NO_DEVICE);
    }
    c->device = p->device;
  } else if (hipGetDevice(&c->device) != hipSuccess) {
    set_err(c, GRP_ERR_NO_DEVICE, "hipGetDevice failed");
    return fail(GRP_ERR_NO_DEVICE);
  }
  c->sw = read_switches();
  int rc = build_seed_tables(c);
  if (rc != GRP_OK) {
    return fail(rc);
  }
  if (tile_frames(c) > GRP_MAX_TILE) { // odd k: a full tile has tile + 1 frames
    set_err(c, GRP_ERR_INVALID, "tile length %u with k=%u and a shortest seed of %u bases: %u frames per tile, at most 65 535 (an ID's count per tile is 16 bits)", p->tile, p->k, span0(c), tile_frames(c));
    return fail(GRP_ERR_INVALID);
  }
  // LDS geometry of the query kernel's worst-case launch must fit one workgroup
  {
    const QueryGeom g = query_geom(c, true), g1 = query_geom(c, false);
    if (g.lds > LDS_PER_WORKGROUP || g1.lds > LDS_PER_WORKGROUP || g1.hist_cap <= (uint32_t)THREADS * p->h + 64) {
      set_err(c, GRP_ERR_INVALID, "tile=%u h=%u needs %zu B of LDS per workgroup beside the count table (limit 160 KiB)", p->tile, p->h, std::max(g.lds, g1.lds));
      return fail(GRP_ERR_INVALID);
    }
  }
#define CREATE_TRY(expr)                                                                                               \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      set_err(c, GRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                                          \
      return fail(e_ == hipErrorOutOfMemory ? GRP_ERR_NOMEM : GRP_ERR_HIP);                                            \
    }                                                                                                                  \
  } while (0)
  {
    hipDeviceProp_t prop;
    CREATE_TRY(hipGetDeviceProperties(&prop, c->device));
    c->n_cus = prop.multiProcessorCount;
    c->arch = prop.gcnArchName;
    c->coherent_arch = c->arch.compare(0, 5, "gfx94") == 0 || c->arch.compare(0, 5, "gfx95") == 0;
  }
  CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  {
    // The side stream runs what must not queue behind a device-filling launch of the main stream: the parse of the
    // next FASTQ chunk beside the fill of the chunk before (the fill's grid holds ~10^6 workgroups: at equal priority
    // the parse kernels were dispatched behind them and the chunk's chain was fill + parse, round 5), the decisions and
    // copy-back of a pipelined window beside the next window's query.  Highest priority the device offers.
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) {
      lo = hi = 0;
      (void)hipGetLastError();
    }
    CREATE_TRY(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, hi));
    // the copy stream at the LOWEST priority: streams of one priority may share a hardware queue, and the barrier packets
    // around a 5 ms DMA copy then hold back whatever else that queue carries (round 5: with both side streams at the
    // highest priority the parse kernels of a chunk started exactly when the copy of the chunk after next ended)
    CREATE_TRY(hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, lo));
  }
  CREATE_TRY(c->d_seeds.reset(1));
  CREATE_TRY(hipMemcpyAsync(c->d_seeds, &c->h_seeds, sizeof(DevSeeds), hipMemcpyHostToDevice, c->stream));
  if (p->m != 0) {
    c->f.m = p->m;
    c->f.m_inv = ~0ULL / p->m;
    // phase 1: plain bit vector (+3 zero pad words for the bucket builder)
    c->n_bv_words = (p->m + 31) / 32;
    CREATE_TRY(c->bv.reset(c->n_bv_words + 3));
    c->f.bv = c->bv;
    CREATE_TRY(hipMemsetAsync(c->f.bv, 0, (c->n_bv_words + 3) * sizeof(uint32_t), c->stream));
  }
  for (QuerySlot& sl : c->slot) {
    CREATE_TRY(sl.d_qctr.reset(QCTR_WORDS));
    if (const int arc = slot_dec_alloc(c, sl, 1024); arc != GRP_OK) {
      return fail(arc);
    }
    CREATE_TRY(hipMemsetAsync(sl.d_qctr, 0, QCTR_WORDS * sizeof(uint64_t), c->stream));
    CREATE_TRY(sl.done.create(hipEventDisableTiming));
    CREATE_TRY(sl.qdone.create(hipEventDisableTiming));
    QuerySlot::StreamWindow& w = sl.win;
    CREATE_TRY(w.d_abort.reset(ABORT_WORDS));
    CREATE_TRY(hipMemsetAsync(w.d_abort, 0, ABORT_BYTES, c->stream));
    CREATE_TRY(w.h_abort.reset(16, hipHostMallocMapped | hipHostMallocCoherent));
    *w.h_abort = 0;
    CREATE_TRY(w.d_sctl.reset(SCT_WORDS));
    CREATE_TRY(w.d_rel.reset((uint64_t)STREAM_REL_WGS * 32u));
    CREATE_TRY(w.h_cmd.reset(CMD_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
    CREATE_TRY(w.h_ack.reset(ACK_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
    memset(w.h_cmd, 0, CMD_WORDS * sizeof(uint32_t));
    memset(w.h_ack, 0, ACK_WORDS * sizeof(uint32_t));
    CREATE_TRY(w.d_executed.reset(EXE_WORDS));
    CREATE_TRY(w.h_executed.reset(EXE_WORDS, hipHostMallocDefault));
  }
  CREATE_TRY(c->h_lists.reset(LIST_PREFIX, hipHostMallocDefault));
  CREATE_TRY(c->h_small_tiles.reset(SMALL_TILES, hipHostMallocMapped | hipHostMallocCoherent));
  CREATE_TRY(c->h_small_lists.reset((uint64_t)SMALL_TILES * SMALL_STRIDE, hipHostMallocMapped | hipHostMallocCoherent));
  CREATE_TRY(hipStreamSynchronize(c->stream));
#undef CREATE_TRY
  *out = c;
  return GRP_OK;
}

void
grp_destroy(grp_ctx* c)
{
  if (!c) {
    return;
  }
  if (c->sw.debug_stats) {
    fprintf(stderr, "grp stats: direct windows %llu (fallbacks %llu), general windows %llu, redo launches %llu, flagged tiles %llu, FASTQ prefetches dropped %llu\n", (unsigned long long)c->n_direct_windows,
            (unsigned long long)c->n_direct_fallbacks, (unsigned long long)c->n_general_windows, (unsigned long long)c->n_redo_launches, (unsigned long long)c->n_flagged_tiles, (unsigned long long)c->ingest.n_dropped);
  }
  if (c->stream3) {
    (void)hipStreamSynchronize(c->stream3);
  }
  if (c->stream2) {
    (void)hipStreamSynchronize(c->stream2);
  }
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
  }
  if (c->pre.worker.joinable()) {
    c->pre.worker.join();
  }
  comm_release(c);
  if (c->reg_text) {
    (void)hipHostUnregister(const_cast<char*>(c->reg_text));
  }
  drain_events(c);
  delete c; // (the members free themselves, the streams go behind them: CtxStreams)
}

// ---- reads -------------------------------------------------------------------------

static int
reads_build(grp_ctx* c, grp_reads* r, const uint64_t* word_off, const uint32_t* len, uint32_t n)
{
  const uint32_t tile = c->params.tile;
  const uint32_t s0 = span0(c);
  const uint32_t min_len = s0 + c->params.h - 1;
  r->ctx = c;
  r->n_reads = n;
  r->n_words = word_off[n];
  r->len.assign(len, len + n);
  r->tile0.resize((size_t)n + 1);
  r->chunk0.resize((size_t)n + 1);
  uint64_t t = 0, ch = 0;
  for (uint32_t i = 0; i < n; ++i) {
    r->tile0[i] = t;
    r->chunk0[i] = ch;
    t += len[i] / tile;
    // reads shorter than the longest span are outside the reference's defined
    // behaviour (SeedNtHash on a too-short string); they contribute nothing
    if (len[i] >= min_len) {
      uint64_t npos = (uint64_t)len[i] - s0 + 1;
      ch += (npos + FILL_CHUNK - 1) / FILL_CHUNK;
    }
    if ((uint64_t)(len[i] + 15u) / 16u > word_off[i + 1] - word_off[i]) {
      return set_err(c, GRP_ERR_INVALID, "read %u: %u bases do not fit its %llu words", i, len[i], (unsigned long long)(word_off[i + 1] - word_off[i]));
    }
  }
  r->tile0[n] = t;
  r->chunk0[n] = ch;
  std::vector<uint32_t> tile_read(t), chunk_read(ch);
  for (uint32_t i = 0; i < n; ++i) {
    for (uint64_t j = r->tile0[i]; j < r->tile0[i + 1]; ++j) {
      tile_read[j] = i;
    }
    for (uint64_t j = r->chunk0[i]; j < r->chunk0[i + 1]; ++j) {
      chunk_read[j] = i;
    }
  }
  HIP_TRY(c, r->d_word_off.reset((uint64_t)n + 1));
  HIP_TRY(c, r->d_len.reset(std::max<uint64_t>(n, 1)));
  HIP_TRY(c, r->d_tile0.reset((uint64_t)n + 1));
  HIP_TRY(c, r->d_chunk0.reset((uint64_t)n + 1));
  HIP_TRY(c, r->d_tile_read.reset(std::max<uint64_t>(t, 1)));
  HIP_TRY(c, r->d_chunk_read.reset(std::max<uint64_t>(ch, 1)));
  HIP_TRY(c, hipMemcpy(r->d_word_off, word_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(r->d_len, len, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(r->d_tile0, r->tile0.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(r->d_chunk0, r->chunk0.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(r->d_tile_read, tile_read.data(), t * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(r->d_chunk_read, chunk_read.data(), ch * 4, hipMemcpyHostToDevice));
  r->dev.word_off = r->d_word_off;
  r->dev.len = r->d_len;
  r->dev.tile0 = r->d_tile0;
  r->dev.tile_read = r->d_tile_read;
  r->dev.chunk0 = r->d_chunk0;
  r->dev.chunk_read = r->d_chunk_read;
  return GRP_OK;
}

// the host half of reads_build for grp_fastq_pack: lengths, tile / fill-chunk prefixes and the tile -> read, chunk -> read
// maps, kept in the batch (its asynchronous uploads read them)
int
reads_index(grp_ctx* c, grp_reads* r, const uint64_t* word_off, const uint32_t* len, uint32_t n)
{
  const uint32_t tile = c->params.tile;
  const uint32_t s0 = span0(c);
  const uint32_t min_len = s0 + c->params.h - 1;
  r->ctx = c;
  r->n_reads = n;
  r->n_words = word_off[n];
  r->len.assign(len, len + n);
  r->tile0.resize((size_t)n + 1);
  r->chunk0.resize((size_t)n + 1);
  uint64_t t = 0, ch = 0;
  for (uint32_t i = 0; i < n; ++i) {
    r->tile0[i] = t;
    r->chunk0[i] = ch;
    t += len[i] / tile;
    if (len[i] >= min_len) { // (see reads_build)
      const uint64_t npos = (uint64_t)len[i] - s0 + 1;
      ch += (npos + FILL_CHUNK - 1) / FILL_CHUNK;
    }
  }
  r->tile0[n] = t;
  r->chunk0[n] = ch;
  r->h_tile_read.resize(t);
  r->h_chunk_read.resize(ch);
  for (uint32_t i = 0; i < n; ++i) {
    for (uint64_t j = r->tile0[i]; j < r->tile0[i + 1]; ++j) {
      r->h_tile_read[j] = i;
    }
    for (uint64_t j = r->chunk0[i]; j < r->chunk0[i + 1]; ++j) {
      r->h_chunk_read[j] = i;
    }
  }
  return GRP_OK;
}

int
grp_reads_upload(grp_ctx* c, const uint32_t* packed, const uint64_t* word_off, const uint32_t* len, uint32_t n, grp_reads** out)
{
  if (!c || !out || !word_off || (!len && n) || (!packed && n && word_off[n])) {
    return set_err(c, GRP_ERR_INVALID, "grp_reads_upload: null argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_reads* r = new grp_reads();
  hipError_t e = r->d_packed.reset(std::max<uint64_t>(word_off[n], 1) + 4);
  if (e != hipSuccess) {
    delete r;
    return set_err(c, GRP_ERR_NOMEM, "allocating %llu words of device memory failed: %s", (unsigned long long)word_off[n], hipGetErrorString(e));
  }
  e = hipMemcpy(r->d_packed, packed, word_off[n] * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    grp_reads_free(r);
    return set_err(c, GRP_ERR_HIP, "hipMemcpy(packed) failed: %s", hipGetErrorString(e));
  }
  r->dev.packed = r->d_packed;
  int rc = reads_build(c, r, word_off, len, n);
  if (rc != GRP_OK) {
    grp_reads_free(r);
    return rc;
  }
  *out = r;
  return GRP_OK;
}

int
grp_reads_wrap_device(grp_ctx* c, const void* d_packed, const uint64_t* word_off, const uint32_t* len, uint32_t n, grp_reads** out)
{
  if (!c || !out || !word_off || (!len && n) || !d_packed) {
    return set_err(c, GRP_ERR_INVALID, "grp_reads_wrap_device: null argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_reads* r = new grp_reads();
  r->dev.packed = static_cast<const uint32_t*>(d_packed); // borrowed: r->d_packed stays empty
  int rc = reads_build(c, r, word_off, len, n);
  if (rc != GRP_OK) {
    grp_reads_free(r);
    return rc;
  }
  *out = r;
  return GRP_OK;
}

void
grp_reads_free(grp_reads* r)
{
  if (!r) {
    return;
  }
  if (r->ctx) {
    // a pipelined window that was abandoned may still run its decision kernel and copy-back on
    // the second stream; both read this batch's arrays
    if (r->ctx->stream2) {
      (void)hipStreamSynchronize(r->ctx->stream2);
    }
    if (r->ctx->stream) {
      (void)hipStreamSynchronize(r->ctx->stream);
    }
    for (QuerySlot& sl : r->ctx->slot) {
      if (sl.reads == r && !sl.busy) {
        sl.reads = nullptr;
      }
    }
  }
  delete r;
}

const uint64_t*
grp_reads_tile0(const grp_reads* r)
{
  return r ? r->tile0.data() : nullptr;
}

// ---- fill ---------------------------------------------------------------------------

// buckets (128-byte units) and far-table slots a filter of m bits at occupancy `occ` needs: W as grp_finalize picks it
// from the measured occupancy, the far entries from the binomial bucket population (E[max(c - 8, 0)] per bucket)
static void
prealloc_sizes(uint64_t m, double occ, uint64_t& n_buckets, uint64_t& far_cap)
{
  // a W slightly below what the hinted occupancy gives: a measured occupancy a few percent above the hint still fits
  const double w = 6.0 / (occ * 1.04);
  const uint32_t W = std::max<uint32_t>(GRP_BUCKET_IDS, std::min<uint32_t>(w >= 64.0 ? 64u : (uint32_t)w, 64u));
  n_buckets = (m + W - 1) / W;
  double pk = std::pow(1.0 - occ, (double)W), tail = 0.0; // P(c = 0)
  for (uint32_t k = 0; k <= W; ++k) {
    if (k > GRP_NEAR_CW) {
      tail += pk * (double)(k - GRP_NEAR_CW);
    }
    pk = pk * (double)(W - k) / (double)(k + 1) * occ / (1.0 - occ);
  }
  const uint64_t expect_far = (uint64_t)(tail * (double)n_buckets * 1.10) + 1024;
  far_cap = 1024;
  while (far_cap < 2 * expect_far) {
    far_cap <<= 1;
  }
}

// called with the first fill launches enqueued: the allocations run beside them
static void
prealloc_start(grp_ctx* c)
{
  if (c->pre.started || c->pre.occupancy <= 0.0 || c->f.m == 0 || c->finalized) {
    return;
  }
  c->pre.started = true;
  uint64_t nb = 0, fc = 0;
  prealloc_sizes(c->f.m, c->pre.occupancy, nb, fc);
  const int device = c->device;
  grp_ctx::Prealloc* p = &c->pre;
  const uint64_t bv_bytes = c->f.m / 8;
  c->pre.worker = std::thread([p, nb, fc, device, bv_bytes] {
    if (hipSetDevice(device) != hipSuccess) {
      return;
    }
    // Only where the tables fit BESIDE what phase 1 may still need: two more bit vectors (the ranks' merge,
    // grp_bv_merge_ranks) and 16 GB for the batches of reads that pass through — C2 has the room, C4's 246 GB of tables
    // have not (grp_finalize then allocates when the fill is through, as it did until round 5).
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    const uint64_t need = nb * (uint64_t)GRP_UNIT_U4 * 16 + fc * sizeof(ulonglong2);
    if ((uint64_t)free_b < need + 2 * bv_bytes + (16ull << 30)) {
      return;
    }
    DevBuf<uint4> u;
    if (u.reset(nb * (uint64_t)GRP_UNIT_U4) != hipSuccess) {
      (void)hipGetLastError();
      return; // grp_finalize allocates what it needs (and reports the failure if there is one)
    }
    DevBuf<ulonglong2> f;
    if (f.reset(fc) != hipSuccess) {
      (void)hipGetLastError();
    }
    p->units = std::move(u);
    p->units_buckets = nb;
    p->far = std::move(f);
  });
}

int
grp_set_occupancy_hint(grp_ctx* c, double occupancy)
{
  if (!c || !(occupancy > 0.0 && occupancy < 1.0)) {
    return set_err(c, GRP_ERR_INVALID, "grp_set_occupancy_hint: occupancy must lie in (0, 1)");
  }
  if (c->finalized || c->pre.started) {
    return set_err(c, GRP_ERR_STATE, "grp_set_occupancy_hint: the tables are being prepared already (call it before the first grp_bv_insert)");
  }
  c->pre.occupancy = occupancy;
  return GRP_OK;
}

int
grp_debug_finalize_times(const grp_ctx* c, double out[6])
{
  if (!c || !out) {
    return GRP_ERR_INVALID;
  }
  memcpy(out, c->finalize_times, sizeof(c->finalize_times));
  return GRP_OK;
}

int
grp_set_filter_size(grp_ctx* c, uint64_t m)
{
  if (!c || m < 64 || m >= (1ULL << 50)) {
    return set_err(c, GRP_ERR_INVALID, "grp_set_filter_size: filter size m=%llu unsupported", (unsigned long long)m);
  }
  if (c->f.m != 0) {
    return set_err(c, GRP_ERR_STATE, "grp_set_filter_size: the filter already has m=%llu bits", (unsigned long long)c->f.m);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t words = (m + 31) / 32;
  HIP_TRY(c, c->bv.reset(words + 3));
  c->f.bv = c->bv;
  HIP_TRY(c, hipMemsetAsync(c->f.bv, 0, (words + 3) * sizeof(uint32_t), c->stream));
  c->params.m = m;
  c->f.m = m;
  c->f.m_inv = ~0ULL / m;
  c->n_bv_words = words;
  return GRP_OK;
}

int
grp_bv_insert(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count)
{
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads) {
    return set_err(c, GRP_ERR_INVALID, "grp_bv_insert: bad range");
  }
  if (c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_insert after grp_finalize: the bit vector is immutable");
  }
  if (c->f.m == 0) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_insert: the filter size is not set (grp_set_filter_size)");
  }
  // re-entrant: the enqueue (stream, event bookkeeping) is serialised here; the launches of
  // different callers may interleave on the stream in any order — the fill is order-free
  std::lock_guard<std::mutex> lock(c->fill_mutex);
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t ch0 = r->chunk0[first], ch1 = r->chunk0[first + count];
  if (ch1 == ch0) {
    return GRP_OK;
  }
  const size_t lds = tab_bytes(c) + bases_bytes(FILL_CHUNK + c->params.k + c->params.h);
  uint64_t probes = 0;
  for (uint32_t i = first; i < first + count; ++i) {
    for (uint32_t s = 0; s < c->params.h; ++s) {
      const uint32_t span = c->h_seeds.span[s];
      if (r->len[i] >= span0(c) + c->params.h - 1) {
        probes += r->len[i] - span + 1;
      }
    }
  }
  // launch in slices of at most MAX_GRID_WGS workgroups
  for (uint64_t b = ch0; b < ch1;) {
    uint32_t nb = (uint32_t)std::min<uint64_t>(ch1 - b, MAX_GRID_WGS);
    Timer t(c, GRP_K_FILL, b == ch0 ? probes : 0);
    DISPATCH_H_SPAN(c, (k_fill<HH, WW><<<dim3(nb), dim3(THREADS), lds, c->stream>>>(c->f, r->dev, c->d_seeds, b)));
    HIP_TRY(c, hipGetLastError());
    b += nb;
  }
  prealloc_start(c); // (the first call with work: the phase-2 tables are allocated beside the fill, grp_set_occupancy_hint)
  return GRP_OK;
}

int
grp_bv_words(const grp_ctx* c, uint64_t* n_words32)
{
  if (!c || !n_words32) {
    return GRP_ERR_INVALID;
  }
  *n_words32 = c->n_bv_words;
  return GRP_OK;
}

int
grp_bv_export_device(grp_ctx* c, void* d_dst)
{
  if (!c || !d_dst) {
    return GRP_ERR_INVALID;
  }
  if (c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_export_device after grp_finalize");
  }
  if (c->f.m == 0) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_export_device: the filter size is not set (grp_set_filter_size)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(d_dst, c->f.bv, c->n_bv_words * 4, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_bv_merge_device(grp_ctx* c, const void* d_src)
{
  if (!c || !d_src) {
    return GRP_ERR_INVALID;
  }
  if (c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_merge_device after grp_finalize: the bit vector is immutable");
  }
  if ((reinterpret_cast<uintptr_t>(d_src) & 15u) != 0) {
    return set_err(c, GRP_ERR_INVALID, "grp_bv_merge_device: source must be 16-byte aligned");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n4 = c->n_bv_words / 4;
  const uint32_t tail = (uint32_t)(c->n_bv_words - n4 * 4);
  k_bv_or<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(reinterpret_cast<uint4*>(c->f.bv), static_cast<const uint4*>(d_src), n4, c->f.bv + n4 * 4, static_cast<const uint32_t*>(d_src) + n4 * 4, tail);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_words_or_device(grp_ctx* c, void* d_dst, const void* d_src, uint64_t n_words32)
{
  if (!c || !d_dst || !d_src || ((reinterpret_cast<uintptr_t>(d_dst) | reinterpret_cast<uintptr_t>(d_src)) & 15u) != 0) {
    return set_err(c, GRP_ERR_INVALID, "grp_words_or_device: null or unaligned buffer");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n4 = n_words32 / 4;
  const uint32_t tail = (uint32_t)(n_words32 - n4 * 4);
  k_bv_or<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(static_cast<uint4*>(d_dst), static_cast<const uint4*>(d_src), n4, static_cast<uint32_t*>(d_dst) + n4 * 4, static_cast<const uint32_t*>(d_src) + n4 * 4, tail);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_bv_import_device(grp_ctx* c, const void* d_src)
{
  if (!c || !d_src) {
    return GRP_ERR_INVALID;
  }
  if (c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_import_device after grp_finalize: the bit vector is immutable");
  }
  if (c->f.m == 0) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_import_device: the filter size is not set (grp_set_filter_size)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(c->f.bv, d_src, c->n_bv_words * 4, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_finalize(grp_ctx* c, uint64_t* pop)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_finalize called twice");
  }
  if (c->f.m == 0) {
    return set_err(c, GRP_ERR_STATE, "grp_finalize: the filter size is not set (grp_set_filter_size)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  const auto t_begin = now();
  for (double& v : c->finalize_times) {
    v = 0.0;
  }
  DevBuf<unsigned long long> d_scalars; // [0] pop (popcount), [1] pop (scan), [2] overflow entries (IDs), [3] far entries (count words)
  HIP_TRY(c, d_scalars.reset(4));
  HIP_TRY(c, hipMemsetAsync(d_scalars, 0, 4 * sizeof(unsigned long long), c->stream));
  Timer* t = new Timer(c, GRP_K_RANK, c->n_bv_words);
  k_popcount<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(c->f.bv, c->n_bv_words, d_scalars);
  unsigned long long h_scalars[4] = { 0, 0, 0, 0 };
  HIP_TRY(c, hipMemcpyAsync(h_scalars, d_scalars, sizeof(h_scalars), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const auto t_pop = now();
  c->finalize_times[0] = secs(t_begin, t_pop);
  const uint64_t h_pop = h_scalars[0];
  // bucket width: ~6 set bits per bucket on average at the measured occupancy;
  // with W <= 13 a bucket can never overflow its 13 ID slots
  // (floor(6 m / pop) in integers, m < 2^50: the quotient in double precision came out one below at exact ratios —
  // 6.0 / (pop / m) = 58.99999999999999 where 6 m = 59 pop)
  uint32_t W = 64;
  if (h_pop > 0) {
    W = (uint32_t)std::min<uint64_t>(6 * c->f.m / h_pop, 64);
  }
  W = std::max<uint32_t>(GRP_BUCKET_IDS, W);
  c->f.W = W;
  c->f.w_magic = (uint64_t)((((unsigned __int128)1) << 64) / W) + 1;
  c->f.n_buckets = (c->f.m + W - 1) / W;
  for (uint64_t q : { (uint64_t)0, (uint64_t)1, c->f.n_buckets / 2, c->f.n_buckets - 1 }) { // the division shortcut is exact
    for (uint64_t d : { (uint64_t)0, (uint64_t)W - 1 }) {
      const uint64_t pos = q * W + d;
      if (grp_div_w(pos, c->f.w_magic) != q) {
        delete t;
        return set_err(c, GRP_ERR_INVALID, "internal: bucket division is not exact for W=%u", W);
      }
    }
  }
  c->n_chunks = (c->f.n_buckets + GRP_CHUNK_BUCKETS - 1) / GRP_CHUNK_BUCKETS;
  c->nsb = ((c->f.n_buckets - 1) >> GRP_SUPER_SHIFT) + 1;
  if (c->n_chunks > MAX_GRID_WGS) {
    delete t;
    return set_err(c, GRP_ERR_INVALID, "filter of %llu buckets exceeds the rank builder's launch size", (unsigned long long)c->f.n_buckets);
  }
  DevBuf<uint32_t> d_chunk_sum;
  DevBuf<uint64_t> d_chunk_base;
  // a bucket is a 128-byte unit since round 5: its query line {rel, bitmap, 13 IDs} and its insert line (8 count words);
  // the count words of the ranks beyond a bucket's 8th set bit come on top (the far table below, ~5 % of the ranks x 32 B)
  const uint64_t unit_bytes = (uint64_t)GRP_UNIT_U4 * 16;
  // Round 6: the tables prepared beside the fill (grp_set_occupancy_hint) are taken where they are large enough — the
  // measured occupancy picks W and the bucket count as ever, a prepared table only has to hold them.  hipMalloc of
  // 130 GB + 8 GB took ~4 s of host time here, with the device idle.
  if (c->pre.worker.joinable()) {
    c->pre.worker.join();
  }
  bool used_prepared = false;
  if (c->pre.units && c->pre.units_buckets >= c->f.n_buckets) {
    c->buckets = std::move(c->pre.units);
    used_prepared = true;
  } else {
    c->pre.units.clear(); // prepared for another geometry (the occupancy came out far above the hint): released first
    const hipError_t e = c->buckets.reset(c->f.n_buckets * GRP_UNIT_U4);
    if (e != hipSuccess) {
      delete t;
      return set_err(c, GRP_ERR_NOMEM, "hipMalloc of %llu bucket units (%.1f GB: 128 B per %u filter bits, IDs and insert counts included) failed: %s", (unsigned long long)c->f.n_buckets, c->f.n_buckets * unit_bytes / 1e9, W,
                     hipGetErrorString(e));
    }
  }
  c->f.buckets = c->buckets;
  HIP_TRY(c, c->d_super.reset(c->nsb));
  c->f.super = c->d_super;
  HIP_TRY(c, d_chunk_sum.reset(c->n_chunks));
  HIP_TRY(c, d_chunk_base.reset(c->n_chunks));
  const auto t_alloc = now();
  c->finalize_times[1] = secs(t_pop, t_alloc);
  k_bucket_chunk_sums<<<dim3((uint32_t)c->n_chunks), dim3(THREADS), 0, c->stream>>>(c->f.bv, c->f.m, W, c->f.n_buckets, d_chunk_sum);
  k_scan_chunks<<<dim3(1), dim3(1024), 0, c->stream>>>(d_chunk_sum, c->n_chunks, d_chunk_base, c->d_super, reinterpret_cast<uint64_t*>(d_scalars.p + 1));
  k_bucket_write<<<dim3((uint32_t)c->n_chunks), dim3(THREADS), 0, c->stream>>>(c->f.bv, c->f.m, W, c->f.n_buckets, c->f.buckets, d_chunk_base, c->d_super, d_scalars + 2);
  delete t;
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(h_scalars, d_scalars, sizeof(h_scalars), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (h_scalars[1] != h_pop) {
    // the popcount runs over whole words, the buckets end at m: an imported or merged vector with bits behind m (grpath.h)
    uint32_t last = 0;
    if ((c->f.m & 31u) != 0 && hipMemcpy(&last, c->f.bv + (c->n_bv_words - 1), sizeof(last), hipMemcpyDeviceToHost) == hipSuccess) {
      const uint32_t stray = (uint32_t)__builtin_popcount(last >> (c->f.m & 31u));
      if (stray != 0 && h_scalars[1] + stray == h_pop) {
        return set_err(c, GRP_ERR_INVALID, "grp_finalize: the bit vector holds %u set bits at positions >= m=%llu (a vector given to grp_bv_import_device / grp_bv_merge_device must be zero there); grp_rewind starts over", stray,
                       (unsigned long long)c->f.m);
      }
    }
    return set_err(c, GRP_ERR_HIP, "internal: bucket scan counted %llu set bits, popcount %llu", h_scalars[1], (unsigned long long)h_pop);
  }
  {
    // the bits now live in the buckets.  (Measured in round 6 before deciding where this belongs: hipFree waits for the
    // device — idle here — and unmaps 7.6 GB at C2; finalize_times[5] has what it takes.  A helper thread would free it
    // behind the caller's back, but hipFree synchronises with EVERY later launch too: a parked streaming window that waits
    // for the host while the host's next HIP call waits for the free is a deadlock this engine has met before)
    const auto t_free = now();
    c->bv.clear();
    c->f.bv = nullptr;
    clear_all(d_chunk_sum, d_chunk_base, d_scalars);
    c->finalize_times[5] = secs(t_free, now());
  }
  c->f.pop = h_pop;
  const auto t_rank = now();
  c->finalize_times[2] = secs(t_alloc, t_rank);
  {
    // the count words beyond a bucket's 8th set bit: {rank + 1, word}, open addressing at load <= 1/2, keys written now
    const uint64_t far_cap = next_pow2_64(std::max<uint64_t>(2 * h_scalars[3], 1024));
    if (c->pre.far.cap >= far_cap) {
      // (a prepared table larger than needed keeps its size: the load only drops)
      c->far = std::move(c->pre.far);
    } else {
      used_prepared = false;
      c->pre.far.clear();
      const hipError_t e = c->far.reset(far_cap);
      if (e != hipSuccess) {
        return set_err(c, GRP_ERR_NOMEM, "hipMalloc of the far count table (%llu ranks beyond their bucket's 8th set bit, %.1f GB) failed: %s", h_scalars[3], far_cap * sizeof(ulonglong2) / 1e9, hipGetErrorString(e));
      }
    }
    c->f.far = c->far;
    c->f.far_mask = c->far.cap - 1;
    HIP_TRY(c, hipMemsetAsync(c->f.far, 0, (c->f.far_mask + 1) * sizeof(ulonglong2), c->stream));
    c->n_far = h_scalars[3];
    if (h_scalars[3]) {
      k_far_build<<<dim3((uint32_t)std::min<uint64_t>((c->f.n_buckets + THREADS - 1) / THREADS, 65536)), dim3(THREADS), 0, c->stream>>>(c->f);
      HIP_TRY(c, hipGetLastError());
    }
  }
  const uint64_t ovf_cap = next_pow2_64(std::max<uint64_t>(2 * h_scalars[2], 1024));
  HIP_TRY(c, c->ovf_keys.reset(ovf_cap));
  HIP_TRY(c, c->ovf_ids.reset(ovf_cap));
  c->f.ovf_keys = c->ovf_keys;
  c->f.ovf_ids = c->ovf_ids;
  HIP_TRY(c, hipMemsetAsync(c->f.ovf_keys, 0, ovf_cap * sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipMemsetAsync(c->f.ovf_ids, 0, ovf_cap * sizeof(uint32_t), c->stream));
  c->f.ovf_mask = ovf_cap - 1;
  c->n_ovf = h_scalars[2];
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->finalize_times[3] = secs(t_rank, now());
  c->finalize_times[4] = used_prepared ? 1.0 : 0.0;
  c->finalized = true;
  if (pop) {
    *pop = h_pop;
  }
  return GRP_OK;
}

} // extern "C"

namespace {

int
classify_enqueue_decide(grp_ctx* c, QuerySlot& sl, hipStream_t st)
{
  Timer t(c, GRP_K_DECIDE, sl.count, st);
  // Reads of more than 256 tiles keep their state in LDS (up to 148 KB at 4096 tiles): sized for the longest read and
  // applied to the whole launch, ONE such read used to drop every workgroup of the window to about one per CU (ADVICE
  // r04).  They get a launch of their own over an index list; the common launch carries no dynamic LDS.
  const uint64_t* tile0 = sl.reads->tile0.data() + sl.first;
  std::vector<uint32_t>& longs = sl.h_long_reads;
  longs.clear();
  uint64_t most = 0;
  for (uint32_t i = 0; i < sl.count; ++i) {
    const uint64_t n = tile0[i + 1] - tile0[i];
    if (n > 4 * LANE_TILES) {
      longs.push_back(i);
      most = std::max(most, n);
    }
  }
  k_decide<<<dim3(sl.count), dim3(DECIDE_THREADS), 0, st>>>(sl.reads->dev, sl.first, sl.count, sl.dp, sl.d_tiles, sl.d_lists, sl.list_cap, sl.d_dec_ids, sl.d_dec_asg, sl.d_dec_scratch, sl.d_dec, 0u, nullptr,
                                                            longs.empty() ? 0u : 4u * LANE_TILES, reinterpret_cast<unsigned long long*>(sl.d_qctr.p), reinterpret_cast<unsigned long long*>(sl.d_dec_raw.p));
  HIP_TRY(c, hipGetLastError());
  if (!longs.empty()) {
    const uint32_t lds_tiles = (uint32_t)std::min<uint64_t>((most + 63) / 64 * 64, DECIDE_LDS_MAX_TILES);
    const size_t lds = decide_lds_bytes(lds_tiles);
    if (const int rc = ensure_lds(c, k_decide, lds); rc != GRP_OK) {
      return rc;
    }
    if (const int rc = ensure_dev(c, sl.d_long_reads, longs.size()); rc != GRP_OK) {
      return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(sl.d_long_reads, longs.data(), longs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st)); // (pageable: staged before the call returns)
    k_decide<<<dim3((uint32_t)longs.size()), dim3(DECIDE_THREADS), lds, st>>>(sl.reads->dev, sl.first, sl.count, sl.dp, sl.d_tiles, sl.d_lists, sl.list_cap, sl.d_dec_ids, sl.d_dec_asg, sl.d_dec_scratch, sl.d_dec, lds_tiles,
                                                                            sl.d_long_reads, 0u);
    HIP_TRY(c, hipGetLastError());
  }
  return GRP_OK;
}

// counters + decisions to pinned memory, completion event.  ONE copy: the window's k_decide has moved the counters into the
// 64 bytes in front of the decisions and zeroed them (round 5: this was two copies and a fill, each with its gap on the stream,
// behind every window and every batch).
int
classify_enqueue_fetch(grp_ctx* c, QuerySlot& sl, hipStream_t st)
{
  if (sl.count == 0) { // no decide launch: the counters alone
    HIP_TRY(c, hipMemcpyAsync(sl.h_qctr, sl.d_qctr, QCTR_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemsetAsync(sl.d_qctr, 0, QCTR_WORDS * sizeof(uint64_t), st));
  } else {
    HIP_TRY(c, hipMemcpyAsync(sl.h_dec_raw, sl.d_dec_raw, ((size_t)sl.count + 2) * sizeof(grp_read_decision), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipEventRecord(sl.done, st));
  sl.side_used = (st != c->stream);
  return GRP_OK;
}

// query + decide + fetch of the slot's window, all asynchronous
int
classify_enqueue(grp_ctx* c, QuerySlot& sl, bool side)
{
  c->q = &sl;
  QueryRun q;
  if (sl.nt) {
    int rc = enqueue_query(c, sl.reads, sl.first, sl.count, sl.list_cap, q);
    if (rc != GRP_OK) {
      return rc;
    }
  }
  sl.t0 = q.t0;
  // optimistic: decide right behind the query, one round trip in the common case.
  // `side`: decision + copy-back go to the second stream, so that the next window's
  // query kernel (already queued on the main stream) starts at once.
  hipStream_t st = c->stream;
  if (side) {
    HIP_TRY(c, hipEventRecord(sl.qdone, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, sl.qdone, 0));
    st = c->stream2;
  }
  int rc = classify_enqueue_decide(c, sl, st);
  if (rc == GRP_OK) {
    rc = classify_enqueue_fetch(c, sl, st);
  }
  return rc;
}

} // namespace

extern "C" {

// the slot's buffers and fields for a window of reads [first, first + count); nothing is enqueued
static int
classify_setup(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot)
{
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads || !dp || slot > 1) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_reads_begin: bad argument");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_reads before grp_finalize");
  }
  QuerySlot& sl = c->slot[slot];
  if (sl.busy) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_reads_begin: slot %u still has a window in flight", slot);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t nt = r->tile0[first + count] - r->tile0[first];
  if (nt > MAX_GRID_WGS) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_reads: %llu tiles in one call (limit 2^22)", (unsigned long long)nt);
  }
  sl.reads = r;
  sl.first = first;
  sl.count = count;
  sl.dp = *dp;
  sl.nt = nt;
  sl.busy = true;
  if (count == 0) {
    return GRP_OK;
  }
  c->q = &sl;
  // decision buffers + scratch for reads too long for the LDS path
  if ((uint64_t)count + 2 > sl.h_dec_raw.cap) { // (the pinned half is allocated last: a pair that failed half-way grows again)
    if (const int rc = slot_dec_alloc(c, sl, std::max<uint64_t>((uint64_t)count + count / 4, 1024)); rc != GRP_OK) {
      return rc;
    }
  }
  if (const int rc = slot_dec_scratch(c, sl, nt); rc != GRP_OK) {
    return rc;
  }
  sl.list_cap = std::max<uint64_t>(sl.d_lists.cap, 4 * nt + 4096);
  return GRP_OK;
}

static int
classify_begin(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, bool side)
{
  int rc = classify_setup(c, r, first, count, dp, slot);
  if (rc != GRP_OK || count == 0) {
    return rc;
  }
  if (c) {
    c->carry.valid = false; // the slot's summaries are about to be replaced
  }
  return classify_enqueue(c, c->slot[slot], side);
}

int
grp_classify_reads_begin(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot)
{
  return classify_begin(c, r, first, count, dp, slot, true);
}


int
grp_classify_reads_end(grp_ctx* c, uint32_t slot, grp_read_decision* out)
{
  if (!c || slot > 1 || !c->slot[slot].busy || c->slot[slot].win.streaming) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_reads_end: no window in flight in this slot");
  }
  QuerySlot& sl = c->slot[slot];
  sl.busy = false;
  if (sl.count == 0) {
    return GRP_OK;
  }
  if (!out) {
    // abandoned window: nothing to wait for, the slot's next use is ordered behind it
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  c->q = &sl;
  HIP_TRY(c, hipEventSynchronize(sl.done));
  for (int attempt = 0; attempt < 8; ++attempt) {
    if (sl.h_qctr[QCTR_LIST_CURSOR] > sl.list_cap) { // list arena too small: grow (with room for the lists of tiles that are redone) and redo the window
      sl.list_cap = 2 * sl.h_qctr[QCTR_LIST_CURSOR] + 4096;
      int rc = classify_enqueue(c, sl, false);
      if (rc != GRP_OK) {
        return rc;
      }
      HIP_TRY(c, hipEventSynchronize(sl.done));
      continue;
    }
    if (sl.h_qctr[QCTR_FLAGGED]) { // some tiles needed the worst-case table: redo them, decide again
      QueryRun q;
      q.t0 = sl.t0;
      int rc = enqueue_redo_flagged(c, sl.reads, sl.list_cap, q);
      if (rc == GRP_OK) {
        rc = classify_enqueue_decide(c, sl, c->stream);
      }
      if (rc == GRP_OK) {
        rc = classify_enqueue_fetch(c, sl, c->stream);
      }
      if (rc != GRP_OK) {
        return rc;
      }
      HIP_TRY(c, hipEventSynchronize(sl.done));
      continue;
    }
    if (c->pending.size() > 64) {
      drain_events(c);
    }
    memcpy(out, sl.h_dec, (size_t)sl.count * sizeof(grp_read_decision));
    return GRP_OK;
  }
  return set_err(c, GRP_ERR_NOMEM, "grp_classify_reads: list arena kept overflowing");
}

int
grp_classify_reads(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, grp_read_decision* out)
{
  if (!out && count) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_reads: out is NULL");
  }
  int rc = classify_begin(c, r, first, count, dp, 0, false);
  if (rc != GRP_OK) {
    if (c && r && r->ctx == c) {
      c->slot[0].busy = false;
    }
    return rc;
  }
  rc = grp_classify_reads_end(c, 0, out);
  if (rc == GRP_OK && !c->view && count) {
    // plain summaries of [first, first + count) stay in slot 0: grp_batch_verify patches them instead of asking again
    c->carry.valid = true;
    c->carry.slot = 0;
    c->carry.reads = r;
    c->carry.first = first;
    c->carry.count = count;
    c->carry.tile_off = 0;
  }
  return rc;
}

} // extern "C"

#include "grp_stream.inc"

extern "C" {

// ---- insert -------------------------------------------------------------------------

int
grp_insert_tiles(grp_ctx* c, const grp_reads* r, uint32_t read_idx, uint32_t tile_start, uint32_t tile_end, uint32_t id)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !r || r->ctx != c || read_idx >= r->n_reads) {
    return set_err(c, GRP_ERR_INVALID, "grp_insert_tiles: bad read index");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_insert_tiles before grp_finalize");
  }
  const uint64_t ntile = r->tile0[read_idx + 1] - r->tile0[read_idx];
  if (tile_start > tile_end || tile_end > ntile) {
    return set_err(c, GRP_ERR_INVALID, "grp_insert_tiles: tiles [%u,%u) outside the read's %llu tiles", tile_start, tile_end, (unsigned long long)ntile);
  }
  if (tile_start == tile_end) {
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t nt = tile_end - tile_start;
  const uint64_t max_ranks = (uint64_t)nt * tile_frames(c) * c->params.h;
  const uint64_t want = next_pow2(max_ranks * 2);
  if (want > c->d_dedup.cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, c->d_dedup.reset(want));
    HIP_TRY(c, hipMemsetAsync(c->d_dedup, 0, want * 8, c->stream));
    c->epoch = 0;
  }
  c->epoch += 1;
  if (c->epoch >= (1u << 24)) {
    HIP_TRY(c, hipMemsetAsync(c->d_dedup, 0, c->d_dedup.cap * 8, c->stream));
    c->epoch = 1;
  }
  const unsigned long long epoch_tag = (unsigned long long)c->epoch << 40;
  const size_t lds = tab_bytes(c) + bases_bytes(c->params.tile + c->params.k + c->params.h);
  {
    Timer t(c, GRP_K_INSERT, max_ranks);
    DISPATCH_H_SPAN(c, (k_insert<HH, WW><<<dim3(nt * tile_parts(c)), dim3(THREADS), lds, c->stream>>>(c->f, r->dev, c->d_seeds, c->params.tile, read_idx, tile_start, id, c->d_dedup, c->d_dedup.cap - 1, epoch_tag)));
  }
  HIP_TRY(c, hipGetLastError());
  return GRP_OK;
}

int
grp_insert_read(grp_ctx* c, const grp_reads* r, uint32_t read_idx, uint32_t tile_start, uint32_t tile_end, uint32_t block_tiles, uint32_t first_id, uint32_t id_offset)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !r || r->ctx != c || read_idx >= r->n_reads || block_tiles == 0 || id_offset > 1) {
    return set_err(c, GRP_ERR_INVALID, "grp_insert_read: bad argument");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_insert_read before grp_finalize");
  }
  const uint64_t ntile = r->tile0[read_idx + 1] - r->tile0[read_idx];
  if (tile_start > tile_end || tile_end > ntile) {
    return set_err(c, GRP_ERR_INVALID, "grp_insert_read: tiles [%u,%u) outside the read's %llu tiles", tile_start, tile_end, (unsigned long long)ntile);
  }
  if (tile_start == tile_end) {
    return GRP_OK;
  }
  const uint32_t nt = tile_end - tile_start;
  const uint32_t n_blocks = (nt + block_tiles - 1) / block_tiles;
  if (n_blocks > 64) { // more ID blocks than mask bits: one launch per block
    for (uint32_t j = 0; j < n_blocks; ++j) {
      const uint32_t bs = tile_start + j * block_tiles;
      int rc = grp_insert_tiles(c, r, read_idx, bs, std::min(bs + block_tiles, tile_end), first_id + (j * block_tiles + id_offset) / block_tiles);
      if (rc != GRP_OK) {
        return rc;
      }
    }
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t max_ranks = (uint64_t)nt * tile_frames(c) * c->params.h;
  {
    const int trc = ensure_insert_table(c, max_ranks);
    if (trc != GRP_OK) {
      return trc;
    }
  }
  InsertTable tb{ c->d_ir_keys, c->d_ir_masks, c->d_ir_locs, c->d_ir_slots, c->d_ir_counter, c->ir_cap - 1 };
  const uint32_t parity = c->ir_parity;
  c->ir_parity ^= 1u;
  const size_t lds = tab_bytes(c) + bases_bytes(c->params.tile + c->params.k + c->params.h);
  {
    Timer t(c, GRP_K_INSERT, max_ranks);
    DISPATCH_HW(c, (k_insert_collect<HH, WW><<<dim3(nt * tile_parts(c)), dim3(THREADS), lds, c->stream>>>(c->f, r->dev, c->d_seeds, c->params.tile, read_idx, tile_start, block_tiles, tb, parity)));
    k_insert_apply<<<dim3((uint32_t)((max_ranks + THREADS - 1) / THREADS)), dim3(THREADS), 0, c->stream>>>(c->f, tb, parity, block_tiles, first_id, id_offset);
  }
  HIP_TRY(c, hipGetLastError());
  return GRP_OK;
}

int
grp_reset_ids(grp_ctx* c)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_reset_ids before grp_finalize");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  k_reset_bucket_ids<<<dim3(65536), dim3(THREADS), 0, c->stream>>>(c->f.buckets, c->f.n_buckets);
  HIP_TRY(c, hipGetLastError());
  k_far_reset<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(c->f.far, c->f.far_mask + 1); // (the insert lines went with the IDs above)
  c->batch.epoch = 0; // (the claims are gone with the counts)
  HIP_TRY(c, hipMemsetAsync(c->f.ovf_keys, 0, (c->f.ovf_mask + 1) * sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipMemsetAsync(c->f.ovf_ids, 0, (c->f.ovf_mask + 1) * sizeof(uint32_t), c->stream));
  return GRP_OK;
}

int
grp_sync(grp_ctx* c)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream3));
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

// ---- inspection -------------------------------------------------------------------

uint64_t
grp_filter_bits(const grp_ctx* c)
{
  return c ? c->f.m : 0;
}

uint64_t
grp_pop(const grp_ctx* c)
{
  return c ? c->f.pop : 0;
}

int
grp_export_bits(grp_ctx* c, uint64_t* words, uint64_t n_words)
{
  if (!c || !words || n_words != (c->f.m + 63) / 64) {
    return set_err(c, GRP_ERR_INVALID, "grp_export_bits: n_words must be ceil(m/64)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  memset(words, 0, n_words * 8);
  if (!c->finalized) {
    // phase 1: the device words ARE the sdsl layout (little-endian 32-bit halves)
    HIP_TRY(c, hipMemcpyAsync(words, c->f.bv, c->n_bv_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GRP_OK;
  }
  DevBuf<uint32_t> d;
  HIP_TRY(c, d.reset(n_words * 2 + 3));
  HIP_TRY(c, hipMemsetAsync(d, 0, (n_words * 2 + 3) * 4, c->stream));
  k_export_bits<<<dim3((uint32_t)std::min<uint64_t>((c->f.n_buckets + 255) / 256, MAX_GRID_WGS)), dim3(256), 0, c->stream>>>(c->f.buckets, c->f.n_buckets, c->f.W, d);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(words, d, n_words * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_rank(grp_ctx* c, const uint64_t* pos, uint64_t n, uint8_t* bit, uint64_t* rank)
{
  if (!c || !c->finalized || !pos || !bit || !rank) {
    return set_err(c, GRP_ERR_STATE, "grp_rank: needs a finalized filter and non-null arrays");
  }
  for (uint64_t i = 0; i < n; ++i) {
    if (pos[i] >= c->f.m) {
      return set_err(c, GRP_ERR_INVALID, "grp_rank: position %llu >= m", (unsigned long long)pos[i]);
    }
  }
  if (n == 0) {
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf<uint64_t> d_pos, d_rank;
  DevBuf<uint8_t> d_bit;
  HIP_TRY(c, d_pos.reset(n));
  HIP_TRY(c, d_rank.reset(n));
  HIP_TRY(c, d_bit.reset(n));
  HIP_TRY(c, hipMemcpyAsync(d_pos, pos, n * 8, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_rank_positions, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, c->f, d_pos, n, d_bit, d_rank);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(bit, d_bit, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(rank, d_rank, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_export_ids(grp_ctx* c, uint64_t first, uint64_t n, uint32_t* ids, uint32_t* counts)
{
  if (!c || !c->finalized || first + n > c->f.pop || !ids || !counts) {
    return set_err(c, GRP_ERR_INVALID, "grp_export_ids: bad range");
  }
  if (n == 0) {
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf<uint32_t> d_ids, d_cnt;
  HIP_TRY(c, d_ids.reset(n));
  HIP_TRY(c, d_cnt.reset(n));
  k_export_ids<<<dim3((uint32_t)std::min<uint64_t>((c->f.n_buckets + 255) / 256, MAX_GRID_WGS)), dim3(256), 0, c->stream>>>(c->f, first, n, d_ids, d_cnt);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(ids, d_ids, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(counts, d_cnt, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_import_ids(grp_ctx* c, uint64_t first, uint64_t n, const uint32_t* ids, const uint32_t* counts)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !c->finalized || first + n > c->f.pop) {
    return set_err(c, GRP_ERR_INVALID, "grp_import_ids: bad range");
  }
  if (n == 0 || (!ids && !counts)) {
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf<uint32_t> d_ids, d_cnt;
  if (ids) {
    HIP_TRY(c, d_ids.reset(n));
    HIP_TRY(c, hipMemcpyAsync(d_ids, ids, n * 4, hipMemcpyHostToDevice, c->stream));
  }
  if (counts) {
    HIP_TRY(c, d_cnt.reset(n));
    HIP_TRY(c, hipMemcpyAsync(d_cnt, counts, n * 4, hipMemcpyHostToDevice, c->stream));
  }
  k_import_ids<<<dim3((uint32_t)std::min<uint64_t>((c->f.n_buckets + 255) / 256, MAX_GRID_WGS)), dim3(256), 0, c->stream>>>(c->f, first, n, d_ids, d_cnt);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_debug_tile_hashes(grp_ctx* c, const grp_reads* r, uint32_t read_idx, uint32_t tile_idx, uint64_t* out, uint64_t cap, uint64_t* n_values)
{
  if (!c || !r || r->ctx != c || read_idx >= r->n_reads || !out || !n_values) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_tile_hashes: bad argument");
  }
  const uint32_t tile = c->params.tile, k = c->params.k;
  if (tile_idx >= r->len[read_idx] / tile) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_tile_hashes: tile index out of range");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t nv = (uint64_t)tile_extent(c, r->len[read_idx], tile_idx).frames * c->params.h;
  *n_values = nv;
  if (nv > cap) {
    return set_err(c, GRP_ERR_NOMEM, "grp_debug_tile_hashes: %llu values, capacity %llu", (unsigned long long)nv, (unsigned long long)cap);
  }
  DevBuf<uint64_t> d;
  HIP_TRY(c, d.reset(nv));
  const size_t lds = tab_bytes(c) + bases_bytes(tile + k + c->params.h);
  DISPATCH_H_SPAN(c, (k_debug_tile_hashes<HH, WW><<<dim3(1), dim3(THREADS), lds, c->stream>>>(r->dev, c->d_seeds, tile, read_idx, tile_idx, d, nv)));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d, nv * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_debug_locate(grp_ctx* c, const uint64_t* x, uint64_t n, uint64_t m, uint32_t W, int on_device, uint64_t* mod_out, uint64_t* div_out)
{
  if (!x || !mod_out || !div_out || m == 0 || W < GRP_BUCKET_IDS || W > 64 || (on_device && !c)) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_locate: bad argument");
  }
  const uint64_t m_inv = ~0ULL / m;                                               // as grp_create
  const uint64_t w_magic = (uint64_t)((((unsigned __int128)1) << 64) / W) + 1;   // as grp_finalize
  if (!on_device) {
    for (uint64_t i = 0; i < n; ++i) {
      mod_out[i] = grp_mod_m(x[i], m, m_inv);
      div_out[i] = grp_div_w(mod_out[i], w_magic);
    }
    return GRP_OK;
  }
  if (n == 0) {
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf<uint64_t> d_x, d_mod, d_div;
  HIP_TRY(c, d_x.reset(n));
  HIP_TRY(c, d_mod.reset(n));
  HIP_TRY(c, d_div.reset(n));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * 8, hipMemcpyHostToDevice, c->stream));
  k_debug_locate<<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream>>>(d_x, n, m, m_inv, W, w_magic, d_mod, d_div);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(mod_out, d_mod, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(div_out, d_div, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_debug_tile_states(grp_ctx* c, uint64_t n_tiles, uint32_t* ids, uint8_t* assigned)
{
  if (!c || !ids || !assigned || n_tiles > c->q->d_dec_cap) { // c->q: the slot of the last window
    return set_err(c, GRP_ERR_INVALID, "grp_debug_tile_states: no such window");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(ids, c->q->d_dec_ids, n_tiles * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(assigned, c->q->d_dec_asg, n_tiles, hipMemcpyDeviceToHost));
  return GRP_OK;
}

// ---- measurement ---------------------------------------------------------------

// k_decide on caller-provided tile summaries (inspection: the decision kernel against the
// reference's own smoothing / stretch / flank vectors, tests/golden/reference_funcs.json)
int
grp_debug_decide(grp_ctx* c, uint32_t n_reads, const uint64_t* tile0, const grp_tile_summary* tiles, const grp_id_count* lists, uint64_t n_lists, const grp_decide_params* dp, grp_read_decision* out, uint32_t* ids_out, uint8_t* asg_out)
{
  if (!c || !tile0 || !dp || !out || n_reads == 0) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_decide: bad argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t nt = tile0[n_reads];
  DevBuf<uint64_t> d_tile0, d_scr;
  DevBuf<grp_tile_summary> d_tiles;
  DevBuf<grp_id_count> d_lists;
  DevBuf<uint32_t> d_ids;
  DevBuf<uint8_t> d_asg;
  DevBuf<grp_read_decision> d_out;
  HIP_TRY(c, d_tile0.reset((uint64_t)n_reads + 1));
  HIP_TRY(c, d_tiles.reset(std::max<uint64_t>(nt, 1)));
  HIP_TRY(c, d_lists.reset(std::max<uint64_t>(n_lists, 1)));
  HIP_TRY(c, d_ids.reset(std::max<uint64_t>(nt, 1)));
  HIP_TRY(c, d_asg.reset(std::max<uint64_t>(nt, 1)));
  HIP_TRY(c, d_scr.reset(std::max<uint64_t>(nt, 1)));
  HIP_TRY(c, d_out.reset(n_reads));
  HIP_TRY(c, hipMemcpy(d_tile0, tile0, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (nt) {
    HIP_TRY(c, hipMemcpy(d_tiles, tiles, nt * sizeof(grp_tile_summary), hipMemcpyHostToDevice));
  }
  if (n_lists) {
    HIP_TRY(c, hipMemcpy(d_lists, lists, n_lists * sizeof(grp_id_count), hipMemcpyHostToDevice));
  }
  HIP_TRY(c, hipMemset(d_ids, 0, std::max<uint64_t>(nt, 1) * 4));
  HIP_TRY(c, hipMemset(d_asg, 0, std::max<uint64_t>(nt, 1)));
  DevReads rd{};
  rd.tile0 = d_tile0;
  const uint32_t lds_tiles = decide_lds_tiles(tile0, n_reads);
  HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_decide), hipFuncAttributeMaxDynamicSharedMemorySize, (int)decide_lds_bytes(DECIDE_LDS_MAX_TILES)));
  k_decide<<<dim3(n_reads), dim3(DECIDE_THREADS), decide_lds_bytes(lds_tiles), c->stream>>>(rd, 0, n_reads, *dp, d_tiles, d_lists, std::max<uint64_t>(n_lists, 1), d_ids, d_asg, d_scr, d_out, lds_tiles);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, d_out, n_reads * sizeof(grp_read_decision), hipMemcpyDeviceToHost));
  if (ids_out && nt) {
    HIP_TRY(c, hipMemcpy(ids_out, d_ids, nt * 4, hipMemcpyDeviceToHost));
  }
  if (asg_out && nt) {
    HIP_TRY(c, hipMemcpy(asg_out, d_asg, nt, hipMemcpyDeviceToHost));
  }
  return GRP_OK;
}

int
grp_debug_stream_stats(const grp_ctx* c, uint64_t out[8])
{
  if (!c || !out) {
    return GRP_ERR_INVALID;
  }
  memcpy(out, c->n_stream_keep, sizeof(c->n_stream_keep));
  out[0] = c->n_stream_coop_refused;
  return GRP_OK;
}

int
grp_set_timing(grp_ctx* c, int enabled)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  c->timing = enabled != 0;
  if (enabled >= 2) {
    c->timing_mask = ~0u; // also the latency-critical insert launches
  }
  return GRP_OK;
}

int
grp_get_kernel_stats(grp_ctx* c, grp_kernel_stat out[GRP_K_COUNT])
{
  if (!c || !out) {
    return GRP_ERR_INVALID;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drain_events(c);
  memcpy(out, c->kstat, sizeof(c->kstat));
  return GRP_OK;
}

int
grp_reset_kernel_stats(grp_ctx* c)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drain_events(c);
  memset(c->kstat, 0, sizeof(c->kstat));
  return GRP_OK;
}

void*
grp_stream(grp_ctx* c)
{
  return c ? (void*)c->stream : nullptr;
}

} // extern "C"

extern "C" int
grp_dev_hooks(void)
{
#ifdef GRP_DEV_HOOKS
  return 1;
#else
  return 0;
#endif
}
#include "grp_batch.inc"
#include "grp_verify.inc"
#include "grp_ingest.inc"
#include "grp_inflate.inc"
#include "grp_gather.inc"
#include "grp_ntcard.inc"
#include "grp_comm.inc"
#ifdef GRP_DEV_HOOKS // priced-and-rejected prototypes, measurement only (make DEV=1; include/grpath_dev.h)
#include "grp_pshard.inc"
#endif
