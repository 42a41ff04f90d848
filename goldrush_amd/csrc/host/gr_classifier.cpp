// See gr_classifier.hpp: construction, the commit, the window plan, the synchronous / pipelined windows and
// run().  commit() is process_read() after the tile query (goldrush_path.cpp:960-1094);
// silver_path_check() is :156-187.  The streaming windows are in gr_classifier_stream.cpp, the windows
// committed as batches in gr_classifier_batch.cpp.
#include "gr_classifier.hpp"
#include "gr_params.hpp"
#include "gr_tile_geom.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#if defined(_OPENMP)
#include <omp.h>
#endif

namespace gr {

Classifier::Classifier(const gr_classifier_params& p, const grp_engine_vt& vt, void* ctx)
  : p_(p)
  , vt_(vt)
  , ctx_(ctx)
{
  // the behaviour switches are read ONCE per classifier, here, not per window
  auto env = [](const char* name) { const char* e = getenv(name); return std::string(e ? e : ""); };
  auto env_real = [](const char* name) { const char* e = getenv(name); return e ? atof(e) : 0.0; };
  auto env_count = [](const char* name, long floor, uint32_t unset) { const char* e = getenv(name); return e ? (uint32_t)std::max(floor, atol(e)) : unset; };
  env_.pipeline = env("GRP_PIPELINE");
  env_.stream = env("GRP_STREAM");
  env_.batch = env("GRP_BATCH");
  {
    const std::string t = env("GRP_MAX_WINDOW_TILES");
    env_.max_window_tiles = t.empty() ? 0 : (uint64_t)std::max(1l, atol(t.c_str()));
  }
  env_.spec_factor = env_real("GRP_SPEC_FACTOR") > 0.0 ? env_real("GRP_SPEC_FACTOR") : 1.0;
  env_.plan_fast_p = getenv("GRP_PLAN_FAST_P") != nullptr;
  env_.t_abort = env_real("GRP_T_ABORT_US") * 1e-6;
  env_.stripe = env_count("GRP_STRIPE", 0, 0);
  env_.resume_ranks_off = env("GRP_STREAM_RESUME_RANKS") == "off";
  env_.batch_enter = env_real("GRP_BATCH_ENTER");
  env_.batch_leave = env_real("GRP_BATCH_LEAVE");
  env_.batch_reads = env_count("GRP_BATCH_READS", 2, 0);
  env_.batch_max = env_count("GRP_BATCH_MAX", 2, 4096);
  env_.batch_stripe_min = env_count("GRP_BATCH_STRIPE_MIN", 1, 32);
  env_.batch_fuse_off = env("GRP_BATCH_FUSE") == "off";
  if (const char* e = getenv("GRP_TRACE_ABORT")) {
    env_.trace_abort = true;
    env_.trace_abort_each = e[0] == '2';
  }
  stream_.trace.on = env_.trace_abort;
  stream_.trace.each = env_.trace_abort_each;
  decide_cpus_ = (int)std::min<unsigned>(effective_cpus(), 32);
  {
    const std::string t = env("GRP_BATCH_OVERLAP");
    if (t == "off") {
      env_.overlap_samples = 0;
    } else if (!t.empty()) {
      env_.overlap_samples = (uint32_t)std::max(1l, atol(t.c_str()));
      env_.overlap_fixed = t.find('+') == std::string::npos; // "4+": the base threshold, still adapting (developer: with GRP_BATCH_OVERLAP_SHIFT)
    }
    const std::string pmin = env("GRP_BATCH_OVERLAP_P");
    if (!pmin.empty()) {
      env_.overlap_min_insert = atof(pmin.c_str());
    }
  }
  if (p_.world == 0) {
    p_.world = 1;
  }
  if (p_.max_window == 0) {
    p_.max_window = 8192;
  }
  if (p_.max_window < p_.world) {
    p_.max_window = p_.world;
  }
}

void
Classifier::set_callbacks(gr_commit_fn commit, gr_rollover_fn rollover, gr_allgather_fn allgather, void* user)
{
  commit_cb_ = commit;
  rollover_cb_ = rollover;
  allgather_cb_ = allgather;
  user_ = user;
  ag_user_ = user;
}

// every committed read goes to the host's callback (the CLI writes its files there) and, inside the ranges
// asked for with keep_commits, into kept_: a witness of what was decided, cheap enough to leave on in a
// measured run (bench.py compares it with the oracle's serial loop on the same reads)
double
Classifier::emit_commit(const gr_commit& ev)
{
  for (int i = 0; i < 2; ++i) {
    if (ev.read >= keep_first_[i] && ev.read - keep_first_[i] < keep_count_[i]) {
      kept_.push_back(ev);
      break;
    }
  }
  return commit_cb_ ? commit_cb_(user_, &ev) : 0.0;
}

void
Classifier::add_phred(double ph)
{
  if (settle_cb_) {
    ++unsettled_; // (what the commit callback returned is not looked at)
  } else {
    phred_sum_in_path_ += ph;
  }
}

// the sums of the insert commits since the last call, from the host, added left to right as add_phred would have
void
Classifier::settle()
{
  if (!settle_cb_ || unsettled_ == 0) {
    return;
  }
  settle_sums_.assign(unsettled_, 0.0);
  settle_cb_(settle_user_, settle_sums_.data(), unsettled_);
  for (const double ph : settle_sums_) {
    phred_sum_in_path_ += ph;
  }
  unsettled_ = 0;
}

int
Classifier::engine_failed(const char* what, int rc)
{
  err_ = std::string(what) + ": " + (vt_.last_error ? vt_.last_error(ctx_) : "failed");
  return rc;
}

void
Classifier::keep_commits(uint32_t first0, uint32_t count0, uint32_t first1, uint32_t count1)
{
  keep_first_[0] = first0;
  keep_count_[0] = count0;
  keep_first_[1] = first1;
  keep_count_[1] = count1;
  kept_.clear();
}

void
Classifier::set_allgather(gr_allgather_fn allgather, void* allgather_user)
{
  allgather_cb_ = allgather;
  ag_user_ = allgather_user;
}

void
Classifier::get_state(gr_classifier_state& s) const
{
  s = stat_; // the statistics are counted into it directly; the loop state:
  s.valid_reads = valid_reads_;
  s.total_tiles = total_tiles_;
  s.assigned_tiles = assigned_tiles_;
  s.unassigned_tiles = unassigned_tiles_;
  s.queries = queries_;
  s.hits = hits_;
  s.misses = misses_;
  s.num_reads_in_path = num_reads_in_path_;
  s.phred_sum_in_path = phred_sum_in_path_;
  s.inserted_bases = inserted_bases_;
  s.curr_path = curr_path_;
  s.id = id_;
  s.ids_inserted = ids_inserted_;
}

void
Classifier::log_path_stat() const
{
  // goldrush_path.cpp:126-154
  const uint64_t cp = curr_path_;
  std::cerr << "Visited " << valid_reads_ << " reads to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Saw: " << total_tiles_ << " tiles to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Assigned: " << assigned_tiles_ << " tiles to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Unassigned: " << unassigned_tiles_ << " tiles to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Total queries: " << queries_ << " to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Total hits: " << hits_ << " to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Total misses: " << misses_ << " to generate " << cp << " silver paths" << std::endl;
  std::cerr << "Num reads: " << num_reads_in_path_ << " in silver path " << cp << std::endl;
  const uint32_t avg_phred = (uint32_t)(-10 * std::log10(phred_sum_in_path_ / inserted_bases_));
  std::cerr << "Average Phred: " << avg_phred << " in silver path " << cp << std::endl;
}

void
Classifier::bump_id()
{
  ++id_;
  if (id_ % 10000 == 0 && p_.rank == 0) {
    std::cerr << "processed " << id_ << " reads" << std::endl;
  }
}

void
Classifier::skip_reads(uint32_t n)
{
  // too short / filtered reads only advance the counter (goldrush_path.cpp:907-932)
  for (uint32_t i = 0; i < n; ++i) {
    bump_id();
  }
}

Classifier::Plan
Classifier::window_plan() const
{
  if (p_.debug) {
    return Plan{ p_.world, false, false }; // one read per rank and round, decided on the host (the dumps are per read, in file order)
  }
  // Choose the speculation window S that maximises committed reads per second
  // under a cost model of one round.  p = insert probability per read, estimated
  // on two time scales (a burst of inserts shrinks the window at once; the long
  // average keeps it from growing to the cap between rare inserts, where every
  // insert would discard half a huge window).
  //   committed(S) = (1 - (1-p)^S) / p        reads up to and including the first insert
  // synchronous round (query, decide, fetch, commit one after the other):
  //   time(S) = t_fixed(S) + S * (t_read / world + t_host)
  // pipelined rounds (the next window runs on the GPU during decide + commit): the
  // slower of GPU and host per window, plus the abandoned next window whenever the
  // current one holds an insert:
  //   time(S) = max(g_fix + S * t_read / world, h_fix + S * t_host) * (1 + P_ins(S))
  // GRP_PIPELINE=off: synchronous rounds only; =force: pipelined whenever the window
  // cap allows (tests)
  const bool no_pipeline = env_.pipeline == "off";
  const bool force_pipeline = env_.pipeline == "force";
  const bool force_stream = env_.stream == "force";
  // With the batches of batch_round taking every stretch where more than ~1 % of the reads insert,
  // the windows only see isolated inserts: the 32-read average (one insert = 3 %) would answer
  // each of them with a handful of small synchronous windows (~0.8 ms per insert, measured on
  // C2); the 256-read average follows a real change of regime within a few inserts.
  const double p_recent = (can_batch() && !env_.plan_fast_p) ? p_insert_mid_ : p_insert_;
  const double p = std::min(1.0, std::max(std::max(p_recent, p_insert_slow_), 1e-7));
  const double world = (double)p_.world;
  // measured on MI355X (bench.py --trace): a synchronous round costs ~70 us when it
  // takes the latency path (host decision, < 16 reads), ~170 us with the decision
  // kernel, plus ~0.15 us of ordered host commit per read; multi-rank rounds add the
  // all-gather.  Pipelined: ~40 us of ramp-up / tail per query launch on the GPU,
  // ~60 us of launches and waits per window on the host.
  const double t_gather = p_.world > 1 ? 200e-6 : 0.0;
  const double t_small = 70e-6, t_large = 170e-6 + t_gather;
  const double g_fix = 40e-6, h_fix = 60e-6 + t_gather;
  const double t_host = 0.15e-6;
  const double t_read = std::max(1e-9, avg_probes_per_read_ / 46e9); // query kernel ~46 G probes/s
  const bool can_pipe = vt_.classify_begin && vt_.classify_end && !no_pipeline;
  double best_rate = 0.0;
  uint32_t best = 1;
  bool best_pipe = false;
  const double lq = std::log1p(-std::min(p, 0.999999));
  for (uint32_t S = 1;; S = (S < 8) ? S + 1 : S + S / 4) {
    if (S > p_.max_window) {
      S = p_.max_window;
    }
    const double p_ins = 1.0 - std::exp(lq * S);
    const double committed = p_ins / p;
    const double t_sync = (S < 16 * p_.world ? t_small : t_large) + S * (t_read / world + t_host);
    if (committed / t_sync > best_rate && !(force_pipeline && best_pipe)) {
      best_rate = committed / t_sync;
      best = S;
      best_pipe = false;
    }
    if (can_pipe && S >= (force_pipeline ? 1 : 16) * p_.world) {
      const double t_pipe = std::max(g_fix + S * t_read / world, h_fix + S * t_host) * (1.0 + p_ins);
      if (committed / t_pipe > best_rate || (force_pipeline && !best_pipe)) {
        best_rate = committed / t_pipe;
        best = S;
        best_pipe = true;
      }
    }
    if (S == p_.max_window) {
      break;
    }
  }
  uint32_t w = (uint32_t)std::min<double>(std::max(best * env_.spec_factor, 1.0), (double)p_.max_window);
  if (p_.world > 1) {
    w = ((w + p_.world - 1) / p_.world) * p_.world;
  }
  if (can_stream() && p_.max_window >= 32) {
    // streaming launch: no per-window round trip and a stale window is cut short by the
    // abort flag, so an insert costs one drain + relaunch (~120 us: resident workgroups
    // finish, insert kernels, ramp-up) whatever the window size
    // a window that ends at the insert: drain + insert kernels + relaunch, ~400 us on C2 (tools/abort_matrix.sh);
    // a window that applies the insert itself (round 3): ~240 us until the first record behind it, ~100 us of
    // device time — 200 us fitted on C2's transition zone (tools/dev/r3_thresholds.sh)
    // (several ranks: what the RANKS agreed on for the last window, not this rank's own view — the plan must come out the same on every rank)
    const bool resume_plan = p_.world == 1 ? can_resume() : (stream_.ranks_resume_ok && vt_.stream_begin_striped_resumable && vt_.stream_resumable && vt_.stream_insert_done && vt_.stream_insert && vt_.insert_read);
    const double t_abort = env_.t_abort > 0.0 ? env_.t_abort : (resume_plan ? 200e-6 : 400e-6);
    // the window size does not matter to an abort (only the resident workgroups are lost),
    // so the launches are as long as allowed.  Several ranks: every rank works on its own
    // stripe of the current group, an insert also discards about half a group; the
    // stripe exchange (~150 us per group) is hidden behind the launches unless it is the
    // longer of the two.
    // (round 5: a window of several ranks that applies inserts itself only leaves on the host's word — the GPUs idle for
    // the host's lag behind them at every window's end, ~100 us — and a rank's launch covers 1 / world of it: the
    // windows grow with the number of ranks)
    const uint32_t S = (p_.world > 1 && resume_plan) ? (uint32_t)std::min<uint64_t>((uint64_t)p_.max_window * std::min<uint32_t>(p_.world, 8u), 1u << 16) : p_.max_window;
    // a record handed back (a tile needed the worst-case table) costs an abort plus a
    // synchronous single-read round: where that is frequent (large h on repeat-rich
    // data) the windows that redo flagged tiles in bulk win
    const double t_redo = t_abort + t_small + t_read;
    double per_read = t_read / world + t_host + p * t_abort + p_redo_ * t_redo + g_fix / S;
    if (p_.world > 1) {
      const double group = (double)stripe_reads() * world;
      per_read = std::max(t_read / world, 150e-6 / group + t_host) + p * (t_abort + 0.5 * group * t_read / world) + p_redo_ * t_redo + g_fix / S;
    }
    if (force_stream || 1.0 / per_read > best_rate) {
      return Plan{ S, false, true };
    }
  }
  return Plan{ w, best_pipe, false };
}

bool
Classifier::can_stream() const
{
  return vt_.stream_begin && vt_.stream_abort && vt_.stream_poll && vt_.stream_end && (p_.world == 1 || allgather_cb_) && env_.stream != "off";
}

// one rank, an engine with the entry points: streaming windows apply inserts inside their launch (round 4: in silver
// mode too — the insert behind which the path rolls over is known to the host in front of it and ends the launches)
bool
Classifier::can_resume() const
{
  // (round 5: several ranks too — every rank's launch applies the insert on its replica, parked by the command where the
  // inserting read is another rank's; the ranks agree per window that all of them can, launch_stream)
  const bool entry = p_.world == 1 ? vt_.stream_begin_resumable != nullptr : (vt_.stream_begin_striped_resumable && vt_.stream_resumable && vt_.stream_insert_done && !env_.resume_ranks_off);
  return entry && vt_.stream_insert && vt_.insert_read && !stream_.resume_disabled;
}

uint32_t
Classifier::stripe_reads() const
{
  if (p_.world == 1) {
    return 0;
  }
  // Ranks exchange finished stripes (one all-gather per group of `world` stripes) while
  // their launches run: long enough to hide the exchange behind the stripe's GPU time
  // (~1.6 us per 25 kb read), short enough that an insert discards little.
  // The all-gather of a group takes ~100 us + ~30 us per rank on a CPU group; a stripe
  // must cover it with GPU time: 128 reads for 2 ranks, 224 for 8.
  return env_.stripe ? env_.stripe : 96u + 16u * p_.world;
}

// Windows are capped in reads by the plan; this caps them in tiles (kMaxWindowTiles / kMaxStreamTiles:
// small -t, very long reads).  At least one read.
uint32_t
Classifier::clamp_tiles(uint32_t pos, uint32_t S, uint64_t max_tiles) const
{
  if (env_.max_window_tiles) { // tests: a tiny cap (GRP_MAX_WINDOW_TILES)
    max_tiles = std::min<uint64_t>(max_tiles, env_.max_window_tiles);
  }
  if (S <= 1 || tile0_[(size_t)pos + S] - tile0_[pos] <= max_tiles) {
    return S;
  }
  const auto first = tile0_.begin() + pos;
  const auto it = std::upper_bound(first, first + S + 1, tile0_[pos] + max_tiles); // first prefix value beyond the cap
  return (uint32_t)std::max<ptrdiff_t>(1, (it - first) - 1);
}

int
Classifier::gather_decisions(uint32_t q)
{
  const uint32_t world = p_.world;
  if (world > 1) {
    dec_all_.resize((size_t)q * world);
    if (!allgather_cb_) {
      err_ = "world > 1 but no allgather callback";
      return GRP_ERR_INVALID;
    }
    int rc = allgather_cb_(ag_user_, dec_.data(), (uint64_t)q * sizeof(gr_read_decision), dec_all_.data());
    if (rc != 0) {
      err_ = "allgather callback failed";
      return GRP_ERR_INVALID;
    }
  } else {
    dec_all_.swap(dec_);
  }
  ++stat_.windows;
  return GRP_OK;
}

// enqueue this rank's slice of the window [pos, pos+S) in an engine slot
int
Classifier::launch_window(void* reads, uint32_t pos, uint32_t S, uint32_t slot, Flight& f)
{
  const uint32_t world = p_.world;
  const uint32_t q = (S + world - 1) / world;
  const uint32_t my_first = std::min<uint64_t>((uint64_t)pos + (uint64_t)p_.rank * q, (uint64_t)pos + S);
  const uint32_t my_count = std::min<uint32_t>(q, pos + S - my_first);
  const grp_decide_params dp{ p_.threshold, p_.unassigned_min, p_.assigned_max, 0 };
  int rc = vt_.classify_begin(ctx_, reads, base_ + my_first, my_count, &dp, slot);
  if (rc != GRP_OK) {
    return engine_failed("classify_begin", rc);
  }
  stat_.reads_queried += my_count;
  f.active = true;
  f.pos = pos;
  f.S = S;
  f.slot = slot;
  f.q = q;
  f.my_count = my_count;
  return GRP_OK;
}

int
Classifier::finish_window(Flight& f)
{
  f.active = false;
  dec_.assign(f.q, gr_read_decision{});
  int rc = vt_.classify_end(ctx_, f.slot, dec_.data());
  if (rc != GRP_OK) {
    return engine_failed("classify_end", rc);
  }
  return gather_decisions(f.q);
}

void
Classifier::abandon_window(Flight& f)
{
  if (f.active) {
    (void)vt_.classify_end(ctx_, f.slot, nullptr); // results are stale: do not wait for them
    f.active = false;
  }
}

int
Classifier::query_window(void* reads, uint32_t first, uint32_t count)
{
  const uint32_t world = p_.world;
  const uint32_t q = (count + world - 1) / world; // reads per rank
  const uint32_t my_first = std::min<uint64_t>((uint64_t)first + (uint64_t)p_.rank * q, (uint64_t)first + count);
  const uint32_t my_count = std::min<uint32_t>(q, first + count - my_first);
  dec_.assign(q, gr_read_decision{});
  // tiny windows (insert-heavy phases) are latency-bound: one kernel + host decision
  // is shorter than two kernels
  if (my_count >= 16 && vt_.classify_reads) {
    // query + decision on the device: 32 bytes per read come back
    const grp_decide_params dp{ p_.threshold, p_.unassigned_min, p_.assigned_max, 0 };
    int rc = vt_.classify_reads(ctx_, reads, base_ + my_first, my_count, &dp, dec_.data());
    if (rc != GRP_OK) {
      return engine_failed("classify_reads", rc);
    }
    stat_.reads_queried += my_count;
  } else if (my_count) {
    const uint64_t nt = tile0_[my_first + my_count] - tile0_[my_first];
    tiles_.resize(nt ? nt : 1);
    if (lists_.size() < 4 * nt + 1024) {
      lists_.resize(4 * nt + 1024);
    }
    for (;;) {
      uint64_t used = 0;
      int rc = vt_.query_tiles(ctx_, reads, base_ + my_first, my_count, tiles_.data(), lists_.data(), lists_.size(), &used, nullptr);
      if (rc == GRP_ERR_NOMEM && used > lists_.size()) {
        lists_.resize(used + used / 4);
        continue;
      }
      if (rc != GRP_OK) {
        return engine_failed("query_tiles", rc);
      }
      break;
    }
    stat_.reads_queried += my_count;
    const DecideParams dp{ p_.threshold, p_.unassigned_min, p_.assigned_max };
    const uint64_t t_base = tile0_[my_first];
#if defined(_OPENMP)
    const int nthreads = (my_count >= 256) ? std::max(1, std::min(omp_get_max_threads(), decide_cpus_)) : 1;
#else
    const int nthreads = 1;
#endif
    if ((int)ws_.size() < nthreads) {
      ws_.resize(nthreads);
    }
#if defined(_OPENMP)
#pragma omp parallel for schedule(static) num_threads(nthreads)
#endif
    for (uint32_t j = 0; j < my_count; ++j) {
#if defined(_OPENMP)
      TileWorkspace& ws = ws_[omp_get_thread_num()];
#else
      TileWorkspace& ws = ws_[0];
#endif
      const uint64_t a = tile0_[my_first + j] - t_base;
      const uint64_t b = tile0_[my_first + j + 1] - t_base;
      ReadDecision rd;
      if (p_.debug) { // single-threaded here (windows of one read): the dumps are kept until the read is committed
        char* buf = nullptr;
        size_t len = 0;
        FILE* mem = open_memstream(&buf, &len);
        decide_read(dp, (size_t)(b - a), tiles_.data() + a, lists_.data(), ws, rd, mem);
        fclose(mem);
        if (debug_text_.size() <= j) {
          debug_text_.resize((size_t)j + 1);
        }
        debug_text_[j].assign(buf ? buf : "", len);
        free(buf);
      } else {
        decide_read(dp, (size_t)(b - a), tiles_.data() + a, lists_.data(), ws, rd);
      }
      static_assert(sizeof(ReadDecision) == sizeof(gr_read_decision), "decision layout");
      std::memcpy(&dec_[j], &rd, sizeof(rd));
    }
  }
  return gather_decisions(q);
}

void
Classifier::silver_path_check(int& rc)
{
  // goldrush_path.cpp:156-187
  if (p_.target_bases < inserted_bases_) {
    settle(); // (in front of the log, the callback and the path's zeroed sum; the run may finish here)
    if (p_.verbose && p_.rank == 0) {
      log_path_stat();
    }
    ++curr_path_;
    if (p_.max_paths < curr_path_) {
      finished_ = true; // exit(0) in the reference
      return;
    }
    inserted_bases_ = 0;
    num_reads_in_path_ = 0;
    phred_sum_in_path_ = 0;
    int e = vt_.reset_ids(ctx_);
    if (e != GRP_OK) {
      rc = engine_failed("reset_ids", e);
      return;
    }
    if (rollover_cb_) {
      rollover_cb_(user_, curr_path_);
    }
    ids_inserted_ = 0;
    last_insert_shares_id_ = false;
  }
}

// returns true when the read changed the miBF (everything queried after it is stale)
bool
Classifier::commit(void* reads, const uint32_t* lens, uint32_t r, const gr_read_decision& d, int& rc, bool engine_inserted, uint32_t engine_first_id)
{
  const uint32_t len = lens[r];
  const uint32_t tile = p_.tile_length, block = p_.block_size, k = p_.kmer_size, s0 = p_.seed0_span ? p_.seed0_span : k;
  const uint32_t nt = d.num_tiles;
  total_tiles_ += nt;
  if (nt) {
    // one query per frame (:567-568); only the last tile can be clipped
    queries_ += (uint64_t)(nt - 1) * geom::frames_per_tile(tile, k, s0) + geom::tile_extent(tile, k, s0, len, nt - 1).frames;
  }
  hits_ += d.hits;
  misses_ += d.misses;
  assigned_tiles_ += d.num_assigned;
  unassigned_tiles_ += nt - d.num_assigned;

  gr_commit ev{};
  ev.read = base_ + r;
  ev.dec = d;
  ev.path = curr_path_;
  bool inserted = false;

  auto insert_block = [&](uint32_t ts, uint32_t te, uint32_t id) {
    if (rc != GRP_OK || engine_inserted) {
      return;
    }
    int e = vt_.insert_tiles(ctx_, reads, base_ + r, ts, te, id);
    if (e != GRP_OK) {
      rc = engine_failed("insert_tiles", e);
    }
  };

  // all ID blocks of the read in one engine call (same result as the block loop)
  // `bases`: what the insert adds to the path (silver mode: the host knows in front of the insert whether the path
  // rolls over behind it, :156-187 — the ID array is reset there, a parked window has nothing to carry on with)
  auto insert_read = [&](uint32_t ts, uint32_t te_excl, uint32_t id_offset, uint64_t bases) {
    if (engine_inserted) {
      // the batch applied the insert ahead of this commit, with the ID this counter allocates now
      if (engine_first_id != ids_inserted_) {
        rc = GRP_ERR_STATE;
        err_ = "batch: the engine inserted block ID " + std::to_string(engine_first_id) + ", the host allocates " + std::to_string(ids_inserted_);
      }
      return;
    }
    if (stream_.ins) {
      // the record comes out of a streaming window that is parked at it: the launch applies the
      // insert itself and carries on behind the read (no launch boundary)
      StreamFlight& f = *stream_.ins;
      uint32_t gen = 0;
      const bool rolls_over = p_.silver_path && p_.target_bases < inserted_bases_ + bases;
      if (rolls_over) {
        ++stat_.stream_rollovers;
      }
      if (!rolls_over && vt_.stream_insert(ctx_, f.slot, base_ + r, ts, te_excl, block, ids_inserted_, id_offset, &gen) == GRP_OK) {
        f.gen = gen;
        f.ins_posted = true;
        f.ins_read = base_ + r;
        f.ins_ts = ts;
        f.ins_te = te_excl;
        f.ins_first_id = ids_inserted_;
        f.ins_off = id_offset;
        stream_.ins_ok = true;
        ++stat_.stream_inserts;
        return;
      }
      // this window cannot: end the launches, then the insert behind them as before
      (void)vt_.stream_abort(ctx_, stream_.cur.slot);
      if (stream_.next.active) {
        (void)vt_.stream_abort(ctx_, stream_.next.slot);
      }
    }
    int e = vt_.insert_read(ctx_, reads, base_ + r, ts, te_excl, block, ids_inserted_, id_offset);
    if (e != GRP_OK) {
      rc = engine_failed("insert_read", e);
    }
  };

  if (p_.debug && p_.rank == 0) { // :979, :1016, :1037, :1084
    std::cerr << (d.kind == DEC_INSERT_WHOLE ? "unassigned" : d.kind == DEC_ASSIGNED_ALL ? "complete assignment" : d.kind == DEC_INSERT_TRIMMED ? "trimmed" : "assigned") << std::endl;
  }
  switch (d.kind) {
    case DEC_INSERT_WHOLE: {
      // :978-1011
      ++ids_inserted_;
      ev.first_id = ids_inserted_;
      if (vt_.insert_read || engine_inserted) {
        insert_read(0, nt, 0, len);
      } else {
        for (uint32_t bs = 0; bs < nt; bs += block) {
          insert_block(bs, std::min(bs + block, nt), ids_inserted_ + (uint32_t)(bs / block));
        }
      }
      ids_inserted_ = ids_inserted_ + (uint32_t)(len / ((size_t)tile * block));
      last_insert_shares_id_ = false;
      const double ph = emit_commit(ev);
      inserted_bases_ += len;
      ++num_reads_in_path_;
      add_phred(ph);
      if (p_.silver_path) {
        silver_path_check(rc);
      }
      inserted = true;
      break;
    }
    case DEC_ASSIGNED_ALL: {
      // :1013-1023
      (void)emit_commit(ev);
      ++valid_reads_;
      bump_id();
      return false;
    }
    case DEC_INSERT_TRIMMED: {
      // :1038-1080
      const uint32_t ts = d.trim_start, te = d.trim_end;
      ++ids_inserted_;
      ev.first_id = ids_inserted_;
      // new_seq = seq.substr(ts*tile, te == nt-1 ? npos : (te-ts+1)*tile)
      const uint64_t off = (uint64_t)ts * tile;
      uint64_t n_out = len - off;
      if (te != nt - 1) {
        n_out = std::min<uint64_t>(n_out, (uint64_t)(te - ts + 1) * tile);
      }
      if (vt_.insert_read || engine_inserted) {
        insert_read(ts, te + 1, 1, n_out);
      } else {
        for (uint64_t bs = ts; bs <= te; bs += block) {
          const uint64_t be = std::min<uint64_t>(bs + block - 1, te);
          insert_block((uint32_t)bs, (uint32_t)be + 1, ids_inserted_ + (uint32_t)((bs - ts + 1) / block));
        }
      }
      ids_inserted_ = ids_inserted_ + (uint32_t)((te - ts) / block);
      // The blocks of a trimmed read are numbered from (0 + 1) / block (:1048-1049) while the counter
      // advances by (te - ts) / block (:1074): with block == 1 the LAST block holds ID ids_inserted_ + 1,
      // the next insert's first; with block > 1 block j holds first + j and the counter ends on the
      // last of them, nothing is shared (the rule used to be (te - ts + 1) % block == 0,
      // exact but needlessly wide — every probe with ID == floor then took the slow look-up)
      last_insert_shares_id_ = block == 1;
      inserted_bases_ += n_out;
      const double ph = emit_commit(ev);
      ++num_reads_in_path_;
      add_phred(ph);
      if (p_.silver_path) {
        silver_path_check(rc);
      }
      inserted = true;
      break;
    }
    default: // DEC_ASSIGNED (:1083-1088)
      (void)emit_commit(ev);
      break;
  }
  if (finished_) {
    return inserted; // exit(0) inside silver_path_check: no ++id
  }
  ++valid_reads_;
  bump_id();
  return inserted;
}

// one read of the current range: the reads filtered out before it only advance the
// counter, then process_read's tail; keeps the insert-rate estimates up to date
bool
Classifier::commit_one(uint32_t r, const gr_read_decision& d, int& rc, bool engine_inserted, uint32_t engine_first_id)
{
  if (rg_.skipped_before) {
    skip_reads(rg_.skipped_before[r]);
  }
  if (p_.debug && p_.rank == 0) {
    if (debug_cb_) {
      debug_cb_(user_, base_ + r); // skipped records in front of it, "name:", "num tiles:" (:907-941)
    }
    if (debug_window_pos_ <= r && r - debug_window_pos_ < debug_text_.size()) {
      std::cerr << debug_text_[r - debug_window_pos_];
    }
    std::cerr << "num assigned tiles: " << d.num_assigned << "\n"
              << "num unassigned tiles: " << d.num_tiles - d.num_assigned << std::endl; // :957-964
  }
  const uint64_t path_before = curr_path_;
  const bool ins = commit(rg_.reads, rg_.lens, r, d, rc, engine_inserted, engine_first_id);
  if (rc != GRP_OK) {
    return ins;
  }
  ++stat_.reads_committed;
  p_insert_ += (1.0 / 32.0) * ((ins ? 1.0 : 0.0) - p_insert_);
  p_insert_mid_ += (1.0 / 256.0) * ((ins ? 1.0 : 0.0) - p_insert_mid_);
  if (curr_path_ != path_before) {
    p_insert_ = p_insert_mid_ = 1.0; // a new silver path starts on an empty ID array: every read inserts
  }
  p_insert_slow_ += (1.0 / 8192.0) * ((ins ? 1.0 : 0.0) - p_insert_slow_);
  p_redo_ -= p_redo_ / 4096.0; // forgotten slowly where no streaming window measures it
  stat_.inserts += ins ? 1 : 0;
  return ins;
}

// ---- synchronous / pipelined window: all decisions of the window, then the commit -----
int
Classifier::window_round(uint32_t& pos)
{
  const uint32_t n = rg_.n;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = GRP_OK;
  Flight cur;
  uint32_t S;
  if (win_.next.active) {
    cur = win_.next; // starts at pos: an insert would have abandoned it
    win_.next.active = false;
    S = cur.S;
  } else {
    const Plan plan = window_plan();
    S = clamp_tiles(pos, std::min<uint32_t>(plan.S, n - pos), kMaxWindowTiles);
    debug_window_pos_ = pos;
    rc = plan.pipelined ? launch_window(rg_.reads, pos, S, 0, cur) : query_window(rg_.reads, pos, S);
    if (rc != GRP_OK) {
      return rc;
    }
  }
  if (cur.active) {
    if (pos + S < n) {
      const Plan plan = window_plan();
      const uint32_t S2 = clamp_tiles(pos + S, std::min<uint32_t>(plan.S, n - pos - S), kMaxWindowTiles);
      if (plan.pipelined && (S2 >= 16 * p_.world || S2 == plan.S)) {
        rc = launch_window(rg_.reads, pos + S, S2, cur.slot ^ 1u, win_.next);
      }
    }
    if (rc == GRP_OK) {
      rc = finish_window(cur);
    }
    if (rc != GRP_OK) {
      abandon_window(win_.next);
      return rc;
    }
  }
  const auto t1 = std::chrono::steady_clock::now();
  stat_.seconds_windows += std::chrono::duration<double>(t1 - t0).count();
  uint32_t j = 0;
  bool stale = false;
  while (j < S && !stale && !finished_) {
    stale = commit_one(pos + j, dec_all_[j], rc); // an insert changes the miBF: later speculative results are stale
    if (rc != GRP_OK) {
      abandon_window(win_.next);
      return rc;
    }
    ++j;
  }
  if (stale || finished_) {
    abandon_window(win_.next);
  }
  pos += j;
  stat_.seconds_commit += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  return GRP_OK;
}

int
Classifier::run(void* reads, const uint32_t* lens, uint32_t first, uint32_t n, const uint32_t* skipped_before, uint32_t skipped_after, bool& finished)
{
  finished = finished_;
  if (finished_) {
    return GRP_OK;
  }
  base_ = first;
  stream_.lost_at = UINT64_MAX;  // (reads are numbered from the range's own first: an index of the range before means nothing here)
  batch_.ovl.base = UINT64_MAX; // (the overlap hints of the range before are another batch's)
  rg_.reads = reads;
  rg_.lens = lens + first;
  rg_.skipped_before = skipped_before ? skipped_before + first : nullptr;
  rg_.n = n;
  tile0_.resize((size_t)n + 1);
  tile0_[0] = 0;
  for (uint32_t i = 0; i < n; ++i) {
    tile0_[i + 1] = tile0_[i] + rg_.lens[i] / p_.tile_length;
  }
  if (n) {
    // frames x seeds per read of this range (every tile has ~tile_length frames)
    avg_probes_per_read_ = (double)tile0_[n] * p_.tile_length * p_.hash_num / n;
  }
  uint32_t pos = 0;
  int rc = GRP_OK;
  while (rc == GRP_OK && pos < n && !finished_) {
    if (!win_.next.active && !stream_.next.active && want_batch()) {
      const auto t0 = std::chrono::steady_clock::now();
      rc = batch_round(pos);
      stat_.seconds_windows += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      continue;
    }
    batch_.in_batch = false;
    batch_.bypass = false;
    if (!win_.next.active && (stream_.next.active || window_plan().streaming)) {
      const auto t0 = std::chrono::steady_clock::now();
      rc = stream_round(pos);
      stat_.seconds_windows += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } else {
      rc = window_round(pos);
    }
  }
  abandon_window(win_.next);
  {
    const int drc = drop_streams();
    if (rc == GRP_OK) {
      rc = drc;
    }
  }
  if (rc != GRP_OK) {
    return rc;
  }
  if (!finished_) {
    skip_reads(skipped_after);
  }
  settle();
  finished = finished_;
  return GRP_OK;
}

} // namespace gr
