// The windows of gr::Classifier that are committed as batches (gr_classifier.hpp).
#include "gr_classifier.hpp"

#include <algorithm>
#include <cmath>

namespace gr {

// ---- windows committed as batches ------------------------------------------------------
// Where many reads insert, a classic window ends at its first insert: one round trip (~80 us)
// per inserting read.  Two reads of a window hardly ever influence each other (they would have
// to overlap on the genome), so the whole window is decided against the state in front of it,
// its inserts are applied at once, and a second query — every read against the state in front of
// its own insert, through the engine's log — confirms the decisions or names the first read
// where the serial loop would have gone another way (include/grpath.h, grp_batch_*).
bool
Classifier::can_batch() const
{
  return vt_.batch_insert && vt_.batch_classify && vt_.batch_undo && vt_.batch_end && vt_.classify_reads && vt_.insert_read && !p_.debug && p_.max_window >= 2 && env_.batch != "off";
}

bool
Classifier::want_batch() const
{
  if (!can_batch() || batch_.bypass) {
    return false;
  }
  if (env_.batch == "force") {
    return true;
  }
  // a batch costs two queries per read whatever the insert rate (~4.5 us on C2); the classic
  // windows cost one query per read plus ~80-400 us per insert: measured on C2 (bench.py --trace)
  // the batch wins down to ~1 % inserting reads
  // (windows that apply inserts themselves are cheaper per insert: the batches take over later)
  const double p_in = env_.batch_enter > 0.0 ? env_.batch_enter : (can_resume() ? 0.020 : 0.012);
  const double p_out = env_.batch_leave > 0.0 ? env_.batch_leave : (can_resume() ? 0.012 : 0.007);
  return p_insert_mid_ >= (batch_.in_batch ? p_out : p_in);
}

// The size of the next batch.  A read decides differently in a batch when it overlaps a read
// INSERTED in front of it in the same batch: with a fraction p of inserting reads the chance that
// read x is the first one grows like c * p * x, so a batch of B reads is confirmed with
// probability exp(-c p B^2 / 2).  c is estimated from what the batches did (first differing
// reads over (inserted read, later read) pairs exposed, both decaying); B maximises reads
// committed per unit of time, a batch costing a fixed part (launches, waits: worth ~70 reads,
// measured) plus its reads, and a batch taken back its undo pass on top.
void
Classifier::batch_feedback(uint32_t reads, uint32_t bad, double exposure)
{
  const bool failed = bad < reads;
  batch_.fail = 0.98 * batch_.fail + (failed ? 1.0 : 0.0);
  batch_.expo = 0.98 * batch_.expo + exposure;
  if (env_.batch_reads) { // developer hook: a fixed batch size
    batch_.reads = env_.batch_reads;
    return;
  }
  const double p = std::min(1.0, std::max(p_insert_mid_, 1e-3));
  const double c = std::max(batch_.fail, 0.05) / std::max(batch_.expo, 1.0) * p;
  const double fixed_cost = 70.0;
  double best_rate = 0.0, area = 0.0, prev = 0.0;
  uint32_t best = 8;
  for (double b = 8.0; b <= 16384.0; b *= 1.125) {
    // area = integral of the survival function up to b = expected reads confirmed
    const int steps = 8;
    for (int i = 0; i < steps; ++i) {
      const double t = prev + (b - prev) * (i + 0.5) / steps;
      area += std::exp(-0.5 * c * t * t) * (b - prev) / steps;
    }
    prev = b;
    const double p_fail = 1.0 - std::exp(-0.5 * c * b * b);
    const double rate = (area + p_fail) / (fixed_cost + b * (1.0 + 0.35 * p_fail));
    if (rate > best_rate) {
      best_rate = rate;
      best = (uint32_t)b;
    }
  }
  batch_.reads = best;
}

// The threshold of the block asked for next.  How many shared samples end a window: 4 (of the one frame in 32 the
// engine samples; rounds 4 - 5: 8 of one in 16) tells every true overlap of a uniform genome (an error-free kilobase
// is ~30 samples, unrelated reads share ~0.005) — and, on a genome with repeats, nearly every read: the windows end
// after ~50 reads and the batches' fixed cost (worth ~70 reads) is what the run pays (bench.py --repeat-frac 0.4,
// measured with one frame in 16: 75 k reads/s at 8, 103 k at 64; uniform genome: 127 k at 8, 123 k at 64).  So the
// threshold climbs the block-by-block efficiency — reads committed per (70 x batches + reads queried), from the
// classifier's own counters: deterministic — while the batches are short; where they are long already (>= 128 reads
// at the base threshold) it stays.  A hint either way: every batch is still confirmed by its second decisions.
void
Classifier::OverlapHints::adapt_threshold(const Classifier& c)
{
  const uint32_t base_thr = c.env_.overlap_samples;
  if (thr != 0) {
    const uint64_t db = c.stat_.batches - s_batches, dr = c.stat_.batch_reads - s_reads, dq = c.stat_.reads_queried - s_queried;
    if (db < 8) {
      // (the snapshots move only when a block of >= 8 batches has been judged — short hint windows
      // accumulate until there are 8, instead of never adapting)
      return;
    }
    const double eff = (double)dr / (70.0 * (double)db + (double)dq);
    if (!(thr == base_thr && dr >= 128 * db)) {
      if (eff < last_eff) {
        dir = -dir;
      }
      uint32_t next = dir > 0 ? thr * 2u : thr / 2u;
      if (next < base_thr) {
        next = base_thr;
        dir = 1;
      } else if (next > 32u * base_thr) {
        next = 32u * base_thr;
        dir = -1;
      }
      thr = next;
    }
    last_eff = eff;
  } else {
    thr = base_thr;
  }
  s_batches = c.stat_.batches;
  s_reads = c.stat_.batch_reads;
  s_queried = c.stat_.reads_queried;
}

uint32_t
Classifier::OverlapHints::ends_at_overlap(Classifier& c, uint32_t at, uint32_t count)
{
  const bool ask = c.vt_.window_overlap && c.env_.overlap_samples && c.p_.world == 1 && c.p_insert_mid_ >= c.env_.overlap_min_insert;
  if (!ask || count < 3) {
    return count;
  }
  const uint32_t n = c.rg_.n;
  if (base != c.base_ || at < lo || at >= hi || (at + count > hi && hi < n)) {
    // the block that starts at this window (overlaps with reads in front of `at` do not matter to it); a window
    // that would reach beyond the block's end begins the next block (its tail would go unexamined)
    constexpr uint32_t kBlock = 4096;
    const uint32_t nb = c.clamp_tiles(at, std::min<uint32_t>(kBlock, n - at), 1ull << 19);
    prev.assign(nb, UINT32_MAX);
    base = c.base_;
    lo = at;
    hi = at + nb;
    ++c.stat_.overlap_calls;
    if (!c.env_.overlap_fixed) {
      adapt_threshold(c);
    }
    const uint32_t threshold = c.env_.overlap_fixed || thr == 0 ? c.env_.overlap_samples : thr;
    if (nb >= 3 && c.vt_.window_overlap(c.ctx_, c.rg_.reads, c.base_ + at, nb, threshold, prev.data()) != GRP_OK) {
      prev.assign(nb, UINT32_MAX); // no hints from this engine call
    }
  }
  const uint32_t end = std::min(at + count, hi);
  for (uint32_t j = at + 1; j < end; ++j) {
    const uint32_t p = prev[j - lo];
    if (p != UINT32_MAX && lo + p >= at) {
      ++c.stat_.batch_overlap_cuts;
      return j - at;
    }
  }
  return count;
}

// One query of a batch striped over the ranks (every one holds a replica and applies the whole batch to it): this
// rank decides its stripe of the `count` reads at `pos` — the first query plainly, the second against `floor` (also
// with an empty stripe: the call tells every rank alike whether the batch was refused) — and the 32-byte decisions
// are all-gathered into `out`.  engine_rc: what the engine's call returned; nothing is exchanged unless it is GRP_OK.
int
Classifier::batch_query_striped(uint32_t pos, uint32_t count, const uint32_t* floor, std::vector<gr_read_decision>& out, int& engine_rc)
{
  // reads [lo, lo + my) of the window are this rank's; q = reads per rank
  const uint32_t q = (count + p_.world - 1) / p_.world;
  const uint32_t lo = std::min<uint64_t>((uint64_t)p_.rank * q, count);
  const uint32_t my = std::min<uint32_t>(q, count - lo);
  const grp_decide_params dp{ p_.threshold, p_.unassigned_min, p_.assigned_max, 0 };
  dec_.assign(q, gr_read_decision{});
  engine_rc = GRP_OK;
  if (floor) {
    engine_rc = vt_.batch_classify(ctx_, rg_.reads, base_ + pos + lo, my, &dp, floor + lo, dec_.data());
  } else if (my) {
    engine_rc = vt_.classify_reads(ctx_, rg_.reads, base_ + pos + lo, my, &dp, dec_.data());
  }
  if (engine_rc != GRP_OK) {
    return engine_rc;
  }
  stat_.reads_queried += my;
  const int rc = gather_decisions(q);
  if (rc != GRP_OK) {
    return rc;
  }
  --stat_.windows; // batch_round has counted the round
  std::copy(dec_all_.begin(), dec_all_.begin() + count, out.begin()); // rank r's block starts at read r * q
  return GRP_OK;
}

// The inserts the first decisions of reads [pos, pos + B) ask for, with the IDs commit() will allocate: fills
// batch_.ins and, per read, batch_.floor (the ID floor of its second query) and batch_.first (its insert's first ID).
// Returns how many reads the batch takes (it ends in front of a read that cannot be part of one) and, in first_ins,
// the first inserting read (UINT32_MAX: none).
uint32_t
Classifier::batch_plan_inserts(uint32_t pos, uint32_t B, uint32_t& first_ins)
{
  const uint32_t tile = p_.tile_length, block = p_.block_size;
  batch_.ins.clear();
  batch_.floor.assign(B, 0);
  batch_.first.assign(B, 0);
  uint32_t ids = ids_inserted_;
  uint64_t bases = inserted_bases_;
  first_ins = UINT32_MAX;
  // the last insert so far was a trimmed read whose last ID block carries the next first ID (:1048-1049, :1074; block == 1 only)
  bool shared_id = last_insert_shares_id_;
  // a batch holds 2^26 (frame, seed) records (frames in units of 256 per tile): the window ends
  // in front of the insert that would not fit (the engine refuses larger batches, GRP_ERR_NOMEM)
  const uint64_t rec_per_tile = (uint64_t)((tile + 255u) / 256u) * 256u * p_.hash_num;
  uint64_t rec = 0;
  for (uint32_t j = 0; j < B; ++j) {
    const gr_read_decision& d = batch_.dec0[j];
    const uint32_t len = rg_.lens[pos + j];
    batch_.floor[j] = (ids + 1) | (shared_id ? 0x80000000u : 0u);
    bool ins = false;
    uint32_t ts = 0, te_excl = 0, off = 0, next_ids = ids;
    if (d.kind == DEC_INSERT_WHOLE) {
      ins = true;
      te_excl = d.num_tiles;
      next_ids = ids + 1 + (uint32_t)(len / ((size_t)tile * block));
      bases += len;
    } else if (d.kind == DEC_INSERT_TRIMMED) {
      ins = true;
      ts = d.trim_start;
      te_excl = d.trim_end + 1;
      off = 1;
      next_ids = ids + 1 + (d.trim_end - d.trim_start) / block;
      uint64_t n_out = len - (uint64_t)ts * tile;
      if (d.trim_end != d.num_tiles - 1) {
        n_out = std::min<uint64_t>(n_out, (uint64_t)(te_excl - ts) * tile);
      }
      bases += n_out;
    } else if (d.kind != DEC_ASSIGNED_ALL && d.kind != DEC_ASSIGNED) {
      return j; // a read the engine hands back to the host's decision: the classic path takes it
    }
    if (ins) {
      if ((te_excl - ts + block - 1) / block > 256 || te_excl <= ts) {
        return j; // more ID blocks than a batch entry holds
      }
      rec += (uint64_t)(te_excl - ts) * rec_per_tile;
      if (rec > (60ull << 20) && !batch_.ins.empty()) {
        return j;
      }
      batch_.ins.push_back(grp_batch_insert{ base_ + pos + j, ts, te_excl, ids + 1, off });
      batch_.first[j] = ids + 1;
      ids = next_ids;
      shared_id = off == 1 && block == 1; // see commit(): only ID blocks of one tile share the next insert's first ID
      if (first_ins == UINT32_MAX) {
        first_ins = j;
      }
      if (p_.silver_path && p_.target_bases < bases) {
        return j + 1; // the silver path rolls over behind this read: the ID array is reset there
      }
    }
  }
  return B;
}

// One rank: the second query runs on past the window — the reads behind it are decided in the
// same launch (their floor is the largest ID: they see the filter as it is, with this batch's
// inserts) and become the next window's first decisions when this batch is confirmed in full.
// The launch is twice as large (better filled), and a confirmed batch costs one round trip less.
// How many reads behind the batch [pos, pos + cnt) the second query takes along.
uint32_t
Classifier::batch_reads_behind(uint32_t pos, uint32_t cnt)
{
  const uint32_t n = rg_.n;
  if (p_.world != 1 || env_.batch_fuse_off || pos + cnt >= n) {
    return 0;
  }
  uint32_t extra = clamp_tiles(pos, std::min<uint32_t>({ batch_.reads, n - pos - cnt, p_.max_window, env_.batch_max }) + cnt, kMaxWindowTiles);
  extra = extra > cnt ? extra - cnt : 0;
  // worth it while the query time thrown away with a batch that ends early (probability from the
  // decayed count of such batches, ~50 batches of memory) stays below the round trip saved (~0.1 ms)
  const double p_fail = std::min(1.0, batch_.fail / 50.0);
  const double t_query = (double)extra * avg_probes_per_read_ / 40e9;
  if (p_fail * t_query > 1.0e-4) {
    extra = 0;
  }
  if (extra) {
    extra = batch_.ovl.ends_at_overlap(*this, pos + cnt, extra); // the reads behind the batch are the next window
  }
  return extra;
}

// The first of the batch's `cnt` reads whose second decision is not its first (cnt: none).  undecided: the engine
// handed that read back in its second decision — the classic path takes it.
uint32_t
Classifier::batch_first_difference(uint32_t cnt, bool& undecided) const
{
  undecided = false;
  for (uint32_t j = 0; j < cnt; ++j) {
    const gr_read_decision &a = batch_.dec0[j], &b = batch_.dec1[j];
    if (a.kind != b.kind || a.num_tiles != b.num_tiles || (a.kind == DEC_INSERT_TRIMMED && (a.trim_start != b.trim_start || a.trim_end != b.trim_end))) {
      undecided = b.kind != DEC_INSERT_WHOLE && b.kind != DEC_INSERT_TRIMMED && b.kind != DEC_ASSIGNED_ALL && b.kind != DEC_ASSIGNED;
      return j;
    }
  }
  return cnt;
}

// (inserted read, later read) pairs of the batch that had the chance to differ, for batch_feedback
double
Classifier::batch_exposure(uint32_t pos, uint32_t cnt, uint32_t bad) const
{
  double exposure = 0.0;
  uint32_t seen = 0, k = 0;
  const uint32_t upto = bad < cnt ? bad + 1 : cnt;
  for (uint32_t j = 0; j < upto; ++j) {
    exposure += seen;
    if (k < batch_.ins.size() && batch_.ins[k].read == base_ + pos + j) {
      ++seen;
      ++k;
    }
  }
  return exposure;
}

// the classic way out of a batch: up to and including the first insert the first decisions ARE the serial loop's
int
Classifier::batch_commit_first(uint32_t& pos, uint32_t upto)
{
  int rc = GRP_OK;
  uint32_t j = 0;
  bool stale = false;
  while (j < upto && !stale && !finished_ && rc == GRP_OK) {
    stale = commit_one(pos + j, batch_.dec0[j], rc);
    ++j;
  }
  pos += j;
  return rc;
}

// One window committed as a batch: size, first decisions, plan, insert, second decisions, confirm or undo, commit.
int
Classifier::batch_round(uint32_t& pos)
{
  const uint32_t n = rg_.n, block = p_.block_size, world = p_.world;
  const grp_decide_params dp{ p_.threshold, p_.unassigned_min, p_.assigned_max, 0 };
  uint32_t B = clamp_tiles(pos, std::min<uint32_t>({ batch_.reads, n - pos, p_.max_window, env_.batch_max }), kMaxWindowTiles);
  // The second query of the previous batch ran on past its window (round 3): the reads behind
  // it were decided in the same launch, against the state that batch left — this window's first
  // decisions, if nothing has touched the filter since (the batch was confirmed in full).
  const bool have_first = batch_.next.valid && batch_.next.base == base_ && batch_.next.pos == pos && batch_.next.inserts == stat_.inserts && batch_.next.path == curr_path_ && !batch_.next.dec.empty();
  batch_.next.valid = false;
  B = have_first ? std::min<uint32_t>(B, (uint32_t)batch_.next.dec.size()) : batch_.ovl.ends_at_overlap(*this, pos, B);
  batch_.in_batch = true;
  ++stat_.windows;

  // the first decisions: every read against the state in front of the window.  Several ranks: the two queries
  // of a batch are striped over the ranks like any other window; small batches are not worth the two exchanges.
  batch_.dec0.resize(B);
  int rc = GRP_OK;
  const bool striped = world > 1 && allgather_cb_ && B >= env_.batch_stripe_min * world;
  if (have_first) {
    std::copy(batch_.next.dec.begin(), batch_.next.dec.begin() + B, batch_.dec0.begin());
    ++stat_.batches_fused;
  } else if (striped) {
    int engine_rc;
    rc = batch_query_striped(pos, B, nullptr, batch_.dec0, engine_rc);
    if (engine_rc != GRP_OK) {
      return engine_failed("classify_reads", engine_rc);
    }
    if (rc != GRP_OK) {
      return rc;
    }
  } else {
    rc = vt_.classify_reads(ctx_, rg_.reads, base_ + pos, B, &dp, batch_.dec0.data());
    if (rc != GRP_OK) {
      return engine_failed("classify_reads", rc);
    }
    stat_.reads_queried += B;
  }

  // the inserts they ask for, applied at once
  uint32_t first_ins;
  const uint32_t cnt = batch_plan_inserts(pos, B, first_ins);
  if (cnt == 0) {
    batch_.bypass = true;
    return GRP_OK;
  }
  if (batch_.ins.size() <= 1) {
    return batch_commit_first(pos, batch_.ins.empty() ? cnt : first_ins + 1);
  }
  rc = vt_.batch_insert(ctx_, rg_.reads, batch_.ins.data(), (uint32_t)batch_.ins.size(), block, base_ + pos);
  if (rc == GRP_ERR_NOMEM) {
    batch_.reads = std::max<uint32_t>(2, cnt / 2); // more records than a batch holds
    ++stat_.batches_refused;
    return batch_commit_first(pos, first_ins + 1);
  }
  if (rc != GRP_OK) {
    return engine_failed("batch_insert", rc);
  }

  // the second decisions: every read against the state in front of its own insert
  const uint32_t extra = (!striped && cnt == B) ? batch_reads_behind(pos, cnt) : 0;
  batch_.dec1.resize((size_t)cnt + extra);
  if (extra) {
    batch_.floor.resize((size_t)cnt + extra);
    std::fill(batch_.floor.begin() + cnt, batch_.floor.end(), 0x7FFFFFFFu);
  }
  uint32_t queried = cnt + extra;
  if (striped) {
    int engine_rc;
    rc = batch_query_striped(pos, cnt, batch_.floor.data(), batch_.dec1, engine_rc);
    queried = 0; // (counted there)
    if (engine_rc == GRP_OK && rc != GRP_OK) {
      (void)vt_.batch_undo(ctx_, base_ + pos, batch_.floor[0] & 0x7FFFFFFFu);
      return rc;
    }
  } else if (vt_.batch_verify) {
    // round 4: the inserted tiles are patched from the batch's own records, only the tiles the batch did
    // not insert are queried again; the reads behind the batch take the plain query (include/grpath.h)
    rc = vt_.batch_verify(ctx_, rg_.reads, base_ + pos, cnt, extra, &dp, batch_.floor.data(), batch_.dec1.data());
  } else {
    rc = vt_.batch_classify(ctx_, rg_.reads, base_ + pos, cnt + extra, &dp, batch_.floor.data(), batch_.dec1.data());
  }
  if (rc == GRP_ERR_NOMEM) {
    // found on the device: the window's reads share too many ranks (they overlap each other);
    // nothing was inserted, the batch is over — a smaller one next time
    batch_.reads = std::max<uint32_t>(2, cnt / 2);
    ++stat_.batches_refused;
    return batch_commit_first(pos, first_ins + 1);
  }
  if (rc != GRP_OK) {
    (void)vt_.batch_undo(ctx_, base_ + pos, batch_.floor[0] & 0x7FFFFFFFu);
    return engine_failed("batch_classify", rc);
  }
  stat_.reads_queried += queried;
  ++stat_.batches;

  // confirm, or undo from the first read that decided differently
  bool bad_undecided;
  const uint32_t bad = batch_first_difference(cnt, bad_undecided), confirmed = bad;
  if (bad == cnt) {
    rc = vt_.batch_end(ctx_);
    if (rc != GRP_OK) {
      return engine_failed("batch_end", rc);
    }
  } else {
    // from read `bad` on the batch was not the serial loop: its insert and the ones behind it are
    // taken back, the confirmed ones in front of it stay
    ++stat_.batches_undone;
    rc = vt_.batch_undo(ctx_, base_ + pos + bad, batch_.floor[bad] & 0x7FFFFFFFu);
    if (rc != GRP_OK) {
      return engine_failed("batch_undo", rc);
    }
  }
  batch_feedback(cnt, bad, batch_exposure(pos, cnt, bad));

  // commit: the second decisions are the records (hits / misses against the state in front of each read)
  const uint64_t path_at_query = curr_path_; // a rollover while committing resets the ID array: the decisions behind the window would be stale
  for (uint32_t j = 0; j < confirmed && rc == GRP_OK && !finished_; ++j) {
    (void)commit_one(pos + j, batch_.dec1[j], rc, batch_.first[j] != 0, batch_.first[j]);
  }
  if (rc != GRP_OK) {
    return rc;
  }
  stat_.batch_reads += confirmed;
  pos += confirmed;
  if (extra && bad == cnt && !finished_ && curr_path_ == path_at_query) {
    batch_.next.dec.assign(batch_.dec1.begin() + cnt, batch_.dec1.end());
    batch_.next.valid = true;
    batch_.next.base = base_;
    batch_.next.pos = pos;
    batch_.next.inserts = stat_.inserts;
    batch_.next.path = curr_path_;
  }
  if (bad != cnt && !finished_) {
    if (bad_undecided) {
      batch_.bypass = true;
    } else {
      // `bad` itself: its second decision was taken against exactly the state it now sees
      (void)commit_one(pos, batch_.dec1[bad], rc);
      ++pos;
    }
  }
  return rc;
}

} // namespace gr
