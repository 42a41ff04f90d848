// Order-exact read classification on top of the engine ABI.
//
// The reference classifies reads strictly one after the other
// (goldrush_path.cpp:1229-1256): read N is queried after the inserts of every
// accepted read < N.  Here a *window* of consecutive reads is queried
// speculatively in one kernel launch, the decisions are committed in file
// order, and as soon as one read inserts (which changes the miBF) the rest of
// the window is discarded and queried again.  The window size adapts to the
// observed insert rate, so the result is identical to the serial loop while
// the insert-free stretches run as large GPU batches.
//
// The class is the reference's loop state with commit() — process_read() behind
// the tile query — plus three kinds of round, each with its own state and file:
//   gr_classifier.cpp         construction, commit, the window plan (cost model), run();
//                             synchronous / pipelined windows (WindowState): with an engine that has
//                             classify_begin / classify_end the window after the current one is already
//                             on the GPU while the host commits (two slots); an insert abandons it
//   gr_classifier_stream.cpp  streaming windows (StreamState): one long launch, its decisions
//                             consumed while it runs; a parked launch applies inserts itself
//   gr_classifier_batch.cpp   windows committed as batches (BatchState): decided at once, inserted
//                             at once, confirmed by a second query
// run() chooses the kind per round; every kind commits through commit_one().
#pragma once
#include "../../../include/grpath_host.h"
#include "gr_tiles.hpp"

#include <chrono>
#include <string>
#include <vector>

namespace gr {

class Classifier
{
public:
  Classifier(const gr_classifier_params& p, const grp_engine_vt& vt, void* ctx);
  void set_callbacks(gr_commit_fn commit, gr_rollover_fn rollover, gr_allgather_fn allgather, void* user);
  void set_allgather(gr_allgather_fn allgather, void* allgather_user);
  void set_debug(gr_debug_fn fn) { debug_cb_ = fn; }
  // The Phred sums of the insert commits come later, through `fn`, instead of from the commit callback (a host that writes
  // its records in batches knows them only then): asked for where the sum is looked at or zeroed — in front of a rollover's
  // log and callback, where the run finishes, at the end of run() — and added in commit order, the same additions
  void set_settle(gr_settle_fn fn, void* user)
  {
    settle_cb_ = fn;
    settle_user_ = user;
  }
  // commits of the reads [first0, first0 + count0) and [first1, first1 + count1) (numbers in the batch of reads) are kept
  void keep_commits(uint32_t first0, uint32_t count0, uint32_t first1, uint32_t count1);
  const std::vector<gr_commit>& kept_commits() const { return kept_; }
  // classifies reads [first, first+n) of the batch; lens / skipped_before are indexed by absolute read number
  int run(void* reads, const uint32_t* lens, uint32_t first, uint32_t n, const uint32_t* skipped_before, uint32_t skipped_after, bool& finished);
  void get_state(gr_classifier_state& s) const;
  // tail of main(): verbose per-path statistics (goldrush_path.cpp:1266-1270)
  void log_path_stat() const;
  const std::string& error() const { return err_; }
  uint64_t curr_path() const { return curr_path_; }
  bool finished() const { return finished_; }

private:
  // The engine takes at most 2^22 tiles per synchronous / pipelined window or batch (grp_classify_reads /
  // grp_query_tiles / grp_batch_* take no more per call: a HIP grid holds fewer than 2^32 work-items) and
  // 2^30 per streaming window: windows are capped in reads by the plan, clamp_tiles caps them in tiles
  static constexpr uint64_t kMaxWindowTiles = 1ull << 22;
  static constexpr uint64_t kMaxStreamTiles = 1ull << 30;
  // wait_record / stream_decision: the launch has left without the record (not an error: the round ends, the window is begun again)
  static constexpr int STREAM_LOST = 100;

  // ---- what every kind of round shares (gr_classifier.cpp) ----
  int query_window(void* reads, uint32_t first, uint32_t count);
  // engine_inserted: the engine has applied the read's ID blocks already (a window committed as a batch: grp_batch_insert_reads)
  bool commit(void* reads, const uint32_t* lens, uint32_t r, const gr_read_decision& d, int& rc, bool engine_inserted = false, uint32_t engine_first_id = 0);
  bool commit_one(uint32_t r, const gr_read_decision& d, int& rc, bool engine_inserted = false, uint32_t engine_first_id = 0);
  void silver_path_check(int& rc);
  void skip_reads(uint32_t n);
  void bump_id();
  double emit_commit(const gr_commit& ev);
  void add_phred(double ph); // an insert commit's sum: added now, or counted for settle()
  void settle();
  int engine_failed(const char* what, int rc); // err_ = "<what>: <the engine's last error>"; returns rc
  struct Plan
  {
    uint32_t S;     // reads in the next window
    bool pipelined; // worth keeping a second window in flight
    bool streaming; // one long launch, decisions consumed while it runs (single rank)
  };
  Plan window_plan() const;
  bool can_stream() const;
  bool can_resume() const;
  uint32_t stripe_reads() const; // reads per stripe of a window shared by several ranks (0: one rank)
  uint32_t clamp_tiles(uint32_t pos, uint32_t S, uint64_t max_tiles) const;
  int gather_decisions(uint32_t q);

  // ---- synchronous / pipelined windows (gr_classifier.cpp) ----
  struct Flight
  {
    bool active = false;
    uint32_t pos = 0, S = 0, slot = 0, q = 0, my_count = 0;
  };
  int launch_window(void* reads, uint32_t pos, uint32_t S, uint32_t slot, Flight& f);
  int finish_window(Flight& f);
  void abandon_window(Flight& f);
  int window_round(uint32_t& pos);

  // ---- streaming windows (gr_classifier_stream.cpp) ----
  struct StreamFlight
  {
    bool active = false;
    uint32_t pos = 0, S = 0, slot = 0;
    const gr_read_decision* dec = nullptr;
    bool resumable = false;   // begun with stream_begin_resumable: it waits where it parks, for stream_abort or stream_insert
    uint32_t gen = 1;         // generation (.pad) of the records that count: +1 per insert the window applied itself
    bool ins_posted = false;  // an insert was handed to the launch (stream_insert); its arguments, should the launch end without it:
    uint32_t ins_read = 0, ins_ts = 0, ins_te = 0, ins_first_id = 0, ins_off = 0;
  };
  int launch_stream(void* reads, uint32_t pos, uint32_t S, uint32_t slot, StreamFlight& f);
  int end_stream(StreamFlight& f);
  int wait_record(const StreamFlight& f, uint32_t j);
  int drop_streams();
  int stream_decision(uint32_t j, gr_read_decision& d);
  int queue_next_stream(uint32_t pos, bool& refused);
  int await_insert_taken();
  int confirm_last_insert(bool& lost);
  int stream_round(uint32_t& pos);

  // ---- windows committed as batches (gr_classifier_batch.cpp) ----
  bool can_batch() const;
  bool want_batch() const; // the insert rate calls for windows committed as batches
  void batch_feedback(uint32_t reads, uint32_t bad, double exposure);
  int batch_query_striped(uint32_t pos, uint32_t count, const uint32_t* floor, std::vector<gr_read_decision>& out, int& engine_rc);
  uint32_t batch_plan_inserts(uint32_t pos, uint32_t B, uint32_t& first_ins);
  uint32_t batch_reads_behind(uint32_t pos, uint32_t cnt);
  uint32_t batch_first_difference(uint32_t cnt, bool& undecided) const;
  double batch_exposure(uint32_t pos, uint32_t cnt, uint32_t bad) const;
  int batch_commit_first(uint32_t& pos, uint32_t upto);
  int batch_round(uint32_t& pos);

  gr_classifier_params p_;
  grp_engine_vt vt_;
  void* ctx_;
  // the behaviour switches, as found when the classifier was created
  struct
  {
    std::string pipeline, stream, batch;       // GRP_PIPELINE / GRP_STREAM / GRP_BATCH
    uint64_t max_window_tiles = 0;             // GRP_MAX_WINDOW_TILES (0: unset)
    double spec_factor = 1.0;                  // GRP_SPEC_FACTOR: scales the synchronous / pipelined window the plan picks
    bool plan_fast_p = false;                  // GRP_PLAN_FAST_P (developer hook): the plan prices inserts with the 32-read average
    double t_abort = 0.0;                      // GRP_T_ABORT_US (developer hook): what an insert costs a streaming launch, in seconds (0: the model's)
    uint32_t stripe = 0;                       // GRP_STRIPE: reads per stripe of a window of several ranks (0: by the number of ranks)
    bool resume_ranks_off = false;             // GRP_STREAM_RESUME_RANKS=off (developer switch): windows of several ranks end at inserts
    double batch_enter = 0.0, batch_leave = 0.0; // GRP_BATCH_ENTER / _LEAVE: insert rates at which the batches take over / hand back (0: the model's)
    uint32_t batch_reads = 0;                  // GRP_BATCH_READS (developer hook): a fixed batch size (0: batch_feedback chooses)
    uint32_t batch_max = 4096;                 // GRP_BATCH_MAX (developer hook)
    uint32_t batch_stripe_min = 32;            // GRP_BATCH_STRIPE_MIN (developer hook / tests): reads per rank from which a batch's queries are striped
    bool batch_fuse_off = false;               // GRP_BATCH_FUSE=off: the second query of a batch does not run on past its window
    bool overlap_fixed = false;                // GRP_BATCH_OVERLAP was given: the threshold stays what it says (else it adapts, OverlapHints)
    uint32_t overlap_samples = 4;              // GRP_BATCH_OVERLAP=<n> / off: windows of batches end in front of a read sharing >= n sampled k-mers with a read in front of it (0: not asked)
    double overlap_min_insert = 0.3;           // GRP_BATCH_OVERLAP_P: ... where at least this share of the reads inserts
    bool trace_abort = false, trace_abort_each = false; // GRP_TRACE_ABORT=1 / 2 (developer hook): AbortTrace, 2 = a line per in-launch insert
  } env_;
  gr_commit_fn commit_cb_ = nullptr;
  uint32_t keep_first_[2] = { 0, 0 }, keep_count_[2] = { 0, 0 };
  std::vector<gr_commit> kept_;
  gr_rollover_fn rollover_cb_ = nullptr;
  gr_allgather_fn allgather_cb_ = nullptr;
  void* user_ = nullptr;
  void* ag_user_ = nullptr;
  gr_debug_fn debug_cb_ = nullptr;
  gr_settle_fn settle_cb_ = nullptr;
  void* settle_user_ = nullptr;
  uint32_t unsettled_ = 0; // insert commits since the last settle()
  std::vector<double> settle_sums_;
  std::vector<std::string> debug_text_; // --debug: the tile-state dumps of the window's reads
  uint32_t debug_window_pos_ = 0;       // ... and the window's first read

  // main()'s loop state (goldrush_path.cpp:1222-1227) + log_info_struct (:41-51)
  uint64_t inserted_bases_ = 0;
  uint64_t curr_path_ = 1;
  uint32_t id_ = 1;
  uint32_t ids_inserted_ = 0;
  uint64_t valid_reads_ = 0, total_tiles_ = 0, assigned_tiles_ = 0, unassigned_tiles_ = 0;
  uint64_t queries_ = 0, hits_ = 0, misses_ = 0, num_reads_in_path_ = 0;
  double phred_sum_in_path_ = 0;
  bool finished_ = false;
  bool last_insert_shares_id_ = false; // the last insert was a trimmed read whose last ID block carries the next insert's first ID

  // speculation control: the estimates the plan and the choice of the round kind share
  double p_insert_ = 1.0;        // EMA over ~32 reads
  double p_insert_slow_ = 0.0;   // EMA over ~8192 reads
  double p_insert_mid_ = 1.0;    // EMA over ~256 reads: chooses between the batches and the windows
  double p_redo_ = 0.0;          // streaming records handed back to the synchronous path (EMA over ~64 reads)
  double avg_probes_per_read_ = 75000.0;

  // statistics: the fields of get_state that are not the loop state above, counted into directly
  gr_classifier_state stat_{};

  // the range being classified (run)
  struct Range
  {
    void* reads = nullptr;
    const uint32_t* lens = nullptr;           // indexed from the range's first read
    const uint32_t* skipped_before = nullptr; // same, or null
    uint32_t n = 0;
  } rg_;
  uint32_t base_ = 0;           // the range's first read in the batch of reads
  std::vector<uint64_t> tile0_; // tile prefix of the current range, relative to base_

  struct WindowState
  {
    Flight next; // pipelined: the window after the current one
  } win_;

  // GRP_TRACE_ABORT (developer hook): where the time of an insert goes in the streaming rounds of this classifier —
  // launch call, first record, drain + insert, and from an insert record a launch applied itself to the first record
  // behind it.  Every mark does nothing unless `on`.
  struct AbortTrace
  {
    using Clock = std::chrono::steady_clock;
    bool on = false, each = false;
    double t_launch = 0, t_first = 0, t_commit_ins = 0, t_drop = 0, t_resume = 0;
    uint64_t n_rounds = 0, n_stale = 0, n_resumed = 0;
    Clock::time_point enter{}, after_launch{}, commit0{}, drop0{}, resume0{};
    bool resume_pending = false;
    static double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
    void round_begins() { if (on) { enter = Clock::now(); resume_pending = false; } }
    void launched() { if (on) { after_launch = Clock::now(); t_launch += secs(enter, after_launch); ++n_rounds; } }
    void record(uint32_t j, uint32_t S) { if (on) { on_record(j, S); } } // record j of a window of S reads has come
    void commit_begins() { if (on) { commit0 = Clock::now(); } }
    // the record is committed; in_launch: it was an insert and the launch took it; stale: the launches were ended for it
    void committed(bool in_launch, bool stale) { if (on) { on_committed(in_launch, stale); } }
    void drop_begins() { if (on) { drop0 = Clock::now(); } }
    void dropped() { if (on) { on_dropped(); } }

  private:
    void on_record(uint32_t j, uint32_t S);
    void on_committed(bool in_launch, bool stale);
    void on_dropped();
  };

  struct StreamState
  {
    StreamFlight cur, next;         // the current window and the one queued behind it
    StreamFlight* ins = nullptr;    // set while stream_round commits an insert record: commit() hands the insert to this window's launch
    bool ins_ok = false;            // ... and the engine took it
    bool resume_disabled = false;   // a launch could not apply an insert itself (shared device): windows end at inserts again
    uint32_t resume_clean_windows = 0; // windows ended without a refused insert since resume_disabled was set (64: tried again)
    uint64_t lost_at = UINT64_MAX;  // read at which a window was last begun again because its launch had left without deciding it
    // several ranks
    bool ranks_resume_ok = true;    // the last window begun was one every rank's launch applies inserts in (what the window plan prices an insert with: the same on every rank)
    uint32_t group_base = UINT32_MAX; // first read of the stripe group held in stripe_recv
    uint32_t group_from = 0;        // reads of the window below this one are committed: a group gathered again behind an insert the launches applied themselves starts here
    bool ins_unconfirmed = false;   // an insert went to the launches and no exchange has followed yet (the ranks have not told each other whether every launch took it)
    bool ins_lost = false;          // this rank's launch had left before the insert command reached it — said in the next exchange, the ranks end the round together
    std::vector<gr_read_decision> stripe_send, stripe_recv;
    AbortTrace trace;
  } stream_;

  // Overlap hints for the windows of batches.  Where most reads insert, a read that overlaps ANY read in front of it in
  // its window will decide differently behind that read's insert and take the rest of the batch back.  The engine tells
  // for blocks of 4096 reads which reads overlap which read in front of them (a hash-only pass, grp_window_overlap: one
  // call per block, nothing per batch) and a window ends in front of the first read that overlaps one of ITS reads — it
  // becomes the next window's first read.  Only a hint; one rank (the ranks would have to agree on it).
  struct OverlapHints
  {
    std::vector<uint32_t> prev;  // grp_window_overlap's answer for reads [lo, hi) of the range that starts at base_ == base
    uint32_t lo = 0, hi = 0;
    uint64_t base = UINT64_MAX;
    // the overlap threshold adapts (round 5): on a repeat-rich genome nearly every read shares a few sampled k-mers with a
    // read in front of it, the windows end after ~50 reads and the batches' fixed cost (~70 reads) is what the run pays
    uint32_t thr = 0;            // the threshold in use (0: not started, env_.overlap_samples)
    int dir = 1;                 // the way the last change went (x 2 / / 2)
    double last_eff = 0.0;       // committed reads per unit of cost over the block before
    uint64_t s_batches = 0, s_reads = 0, s_queried = 0; // counters at the last block's start
    void adapt_threshold(const Classifier& c);
    uint32_t ends_at_overlap(Classifier& c, uint32_t at, uint32_t count); // reads [at, at + count) of the range: how many to keep
  };

  struct BatchState
  {
    bool in_batch = false;    // the last round was a batch (hysteresis)
    bool bypass = false;      // the read in front cannot be part of a batch: one classic round
    uint32_t reads = 128;     // reads per batch, chosen by batch_feedback
    double fail = 1.0, expo = 5e4; // first reads that decided differently / (inserted read, later read) pairs exposed (decaying sums)
    std::vector<gr_read_decision> dec0, dec1; // the window's first and second decisions
    std::vector<grp_batch_insert> ins;        // the inserts the first decisions ask for ...
    std::vector<uint32_t> floor, first;       // ... per read: the floor of its second query, the first ID of its insert (0: none)
    // decisions of the reads behind the last batch, taken by its second query's launch (batch_round)
    struct
    {
      std::vector<gr_read_decision> dec;
      bool valid = false;
      uint32_t base = 0, pos = 0;
      uint64_t inserts = 0, path = 0;
    } next;
    OverlapHints ovl;
  } batch_;

  // scratch of the queries
  std::vector<grp_tile_summary> tiles_;
  std::vector<grp_id_count> lists_;
  std::vector<gr_read_decision> dec_, dec_all_;
  std::vector<TileWorkspace> ws_;
  int decide_cpus_ = 1; // threads for the host's decisions of a large window
  std::string err_;
};

} // namespace gr
