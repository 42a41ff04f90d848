// The streaming windows of gr::Classifier (gr_classifier.hpp): one long launch per window, its decision records
// consumed while it runs; a parked launch applies the insert the host commits and carries on behind it.
#include "gr_classifier.hpp"

#include <algorithm>
#include <cstdio>

namespace gr {

int
Classifier::launch_stream(void* reads, uint32_t pos, uint32_t S, uint32_t slot, StreamFlight& f)
{
  S = clamp_tiles(pos, S, kMaxStreamTiles);
  const grp_decide_params dp{ p_.threshold, p_.unassigned_min, p_.assigned_max, 0 };
  const gr_read_decision* dec = nullptr;
  // One rank: a window that waits where it parks and applies the insert the host commits inside its own
  // launch (stream_round; a silver-path run resets the ID array at a rollover: commit() ends the launches in
  // front of that insert); several ranks share a window in stripes: those windows end where they park.
  bool resumable = can_resume();
  int rc;
  if (p_.world == 1) {
    rc = resumable ? vt_.stream_begin_resumable(ctx_, reads, base_ + pos, S, &dp, slot, &dec) : vt_.stream_begin(ctx_, reads, base_ + pos, S, &dp, slot, 0, 1, 0, &dec);
  } else {
    rc = resumable ? vt_.stream_begin_striped_resumable(ctx_, reads, base_ + pos, S, &dp, slot, stripe_reads(), p_.world, p_.rank, &dec)
                   : vt_.stream_begin(ctx_, reads, base_ + pos, S, &dp, slot, stripe_reads(), p_.world, p_.rank, &dec);
    if (vt_.stream_begin_striped_resumable && vt_.stream_resumable) {
      // What the window can do is the RANKS' matter: one rank whose launch ends where it parks (the runtime refused the
      // cooperative launch, parked windows switched off after a refused insert) or that cannot begin the window now
      // (GRP_ERR_BUSY) — and every rank takes that form, or they would walk different stripes of different windows.
      // Every rank calls this at the same point of the same sequence of records, whatever its own call returned.
      uint32_t mine[2] = { rc == GRP_OK ? 0u : rc == GRP_ERR_BUSY ? 1u : 2u, (rc == GRP_OK && resumable && vt_.stream_resumable(ctx_, slot) == 1) ? 1u : 0u };
      std::vector<uint32_t> all((size_t)2 * p_.world);
      if (!allgather_cb_ || allgather_cb_(ag_user_, mine, sizeof(mine), all.data()) != 0) {
        err_ = "allgather callback failed";
        if (rc == GRP_OK) {
          (void)vt_.stream_abort(ctx_, slot);
          (void)vt_.stream_end(ctx_, slot, nullptr);
        }
        return GRP_ERR_INVALID;
      }
      uint32_t worst = 0;
      bool all_resumable = true;
      for (uint32_t q = 0; q < p_.world; ++q) {
        worst = std::max(worst, all[(size_t)2 * q]);
        all_resumable = all_resumable && all[(size_t)2 * q + 1] != 0;
      }
      if (worst != 0) {
        if (rc == GRP_OK) { // another rank could not: this rank's window goes as well
          (void)vt_.stream_abort(ctx_, slot);
          (void)vt_.stream_end(ctx_, slot, nullptr);
        }
        if (worst == 1 && (rc == GRP_OK || rc == GRP_ERR_BUSY)) {
          return GRP_ERR_BUSY;
        }
        if (rc == GRP_OK) {
          err_ = "stream_begin failed on another rank";
          return GRP_ERR_STATE;
        }
      }
      resumable = all_resumable;
      stream_.ranks_resume_ok = all_resumable;
    }
  }
  if (rc != GRP_OK) {
    return engine_failed("stream_begin", rc);
  }
  f.active = true;
  f.pos = pos;
  f.S = S;
  f.slot = slot;
  f.dec = dec;
  f.resumable = resumable;
  f.gen = 1;
  f.ins_posted = false;
  ++stat_.windows;
  return GRP_OK;
}

int
Classifier::end_stream(StreamFlight& f)
{
  if (!f.active) {
    return GRP_OK;
  }
  f.active = false;
  uint32_t decided = 0;
  int rc = vt_.stream_end(ctx_, f.slot, &decided);
  if (rc == 1 || rc == 2) {
    // the launch ended without the insert it had been handed: nothing was inserted; the classic call applies it,
    // stream-ordered behind whatever is queued.  2 (one rank: also 1): its workgroups were not all resident — a shared
    // device — and windows end at inserts again for a while; 1 with several ranks: the launch had left before the
    // command came (its own stripes were decided, the inserting read was another rank's) — nothing is wrong
    if (rc == 2 || p_.world == 1) {
      stream_.resume_disabled = true;
      stream_.resume_clean_windows = 0;
    }
    ++stat_.stream_insert_fallbacks;
    rc = GRP_OK;
    if (f.ins_posted) {
      rc = vt_.insert_read(ctx_, rg_.reads, f.ins_read, f.ins_ts, f.ins_te, p_.block_size, f.ins_first_id, f.ins_off);
      if (rc != GRP_OK) {
        (void)engine_failed("insert_read", rc);
      }
    }
  } else if (rc != GRP_OK) {
    return engine_failed("stream_end", rc);
  }
  f.ins_posted = false;
  stat_.reads_queried += decided;
  if (stream_.resume_disabled && rc == GRP_OK && ++stream_.resume_clean_windows >= 64) {
    stream_.resume_disabled = false; // 64 windows ended cleanly since the last refused insert: parked windows are tried again
  }
  return rc;
}

int
Classifier::wait_record(const StreamFlight& f, uint32_t j)
{
  const uint32_t* flag = &f.dec[j].pad;
  uint32_t spins = 0;
  bool finished_seen = false;
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != f.gen) { // (an older generation: decided before an insert in front of the read, stale)
    __builtin_ia32_pause();
    if ((++spins & 0x3FFFu) == 0) {
      if (finished_seen) {
        // The launch is over and this record never came.  With an insert posted: the launch gave up on it
        // (end_stream applies it).  Without: a parked window that was told nothing for its idle limit (a host
        // stopped by a debugger, SIGSTOP, a stalled file system) has left by itself — nothing was modified, the
        // window is ended and begun again at this read.  Twice in a row at the same read is an error.
        if (!f.ins_posted && stream_.lost_at == (uint64_t)base_ + f.pos + j) {
          err_ = "streaming window finished without deciding one of its reads";
          return GRP_ERR_STATE;
        }
        stream_.lost_at = f.ins_posted ? UINT64_MAX : (uint64_t)base_ + f.pos + j;
        if (!f.ins_posted) {
          ++stat_.stream_relaunches;
        }
        return STREAM_LOST;
      }
      const int st = vt_.stream_poll(ctx_, f.slot);
      if (st < 0) {
        return engine_failed("stream_poll", st);
      }
      finished_seen = st == 1; // one more round of spinning for the last store to land
    }
  }
  if (stream_.lost_at == (uint64_t)base_ + f.pos + j) {
    stream_.lost_at = UINT64_MAX; // the window begun again has decided the read: a later idle exit at the same index of ANOTHER run() is a new event
  }
  return GRP_OK;
}

int
Classifier::drop_streams()
{
  int rc = GRP_OK;
  for (StreamFlight* f : { &stream_.cur, &stream_.next }) { // both flags first: the window queued behind must not start on a state an insert is still missing from
    if (f->active) {
      (void)vt_.stream_abort(ctx_, f->slot);
    }
  }
  for (StreamFlight* f : { &stream_.cur, &stream_.next }) {
    if (f->active) {
      const int e = end_stream(*f);
      if (rc == GRP_OK) {
        rc = e;
      }
    }
  }
  return rc;
}

// Decision of read j of the streaming window stream_.cur.  One rank reads its own record as
// soon as it is complete; several ranks exchange the stripes of a group (`world`
// consecutive stripes = world * stripe consecutive reads) once each has finished its own.
int
Classifier::stream_decision(uint32_t j, gr_read_decision& d)
{
  const uint32_t W = p_.world, S = stream_.cur.S;
  if (W == 1) {
    const int e = wait_record(stream_.cur, j);
    if (e == GRP_OK) {
      d = stream_.cur.dec[j];
      stream_.cur.ins_posted = false; // a record of the generation behind the posted insert: the launch has applied it
    }
    return e;
  }
  // A rank's block of the exchange: its stripe's C records behind one header record — .kind of the header != 0: this
  // rank's launch has left without a record it owes (wait_record: STREAM_LOST).  Every rank then ends the round at this
  // read, together: the ranks walk one sequence of records, whatever happens to one launch (round 5; a window of
  // several ranks used to end at every insert, so a launch could not be lost behind one).
  const uint32_t C = stripe_reads(), GW = C * W, CB = C + 1;
  if (stream_.group_base == UINT32_MAX || j < stream_.group_base || j >= stream_.group_base + GW) {
    stream_.group_base = (j / GW) * GW;
    const uint32_t lo = std::min(stream_.group_base + p_.rank * C, S), hi = std::min(lo + C, S);
    stream_.stripe_send.assign(CB, gr_read_decision{});
    int lost = GRP_OK;
    if (stream_.ins_lost) {
      stream_.stripe_send[0].kind = 1;
      lost = STREAM_LOST;
    }
    for (uint32_t q = std::max(lo, stream_.group_from); q < hi && lost == GRP_OK; ++q) { // (reads below stream_.group_from are committed: the group is gathered again behind an insert the launches applied)
      const int e = wait_record(stream_.cur, q);
      if (e == STREAM_LOST) {
        lost = e;
        stream_.stripe_send[0].kind = 1;
        break;
      }
      if (e != GRP_OK) {
        return e;
      }
      stream_.stripe_send[1 + q - lo] = stream_.cur.dec[q];
      const uint32_t kind = stream_.cur.dec[q].kind;
      if (kind == DEC_INSERT_WHOLE || kind == DEC_INSERT_TRIMMED || kind == 0) {
        break; // the launch parks itself behind such a record: later records of the stripe never come, and no rank reads them
      }
    }
    stream_.stripe_recv.resize((size_t)CB * W);
    if (allgather_cb_(ag_user_, stream_.stripe_send.data(), (uint64_t)CB * sizeof(gr_read_decision), stream_.stripe_recv.data()) != 0) {
      err_ = "allgather callback failed";
      return GRP_ERR_INVALID;
    }
    stream_.ins_unconfirmed = false;
    for (uint32_t q = 0; q < W; ++q) {
      if (stream_.stripe_recv[(size_t)q * CB].kind != 0) {
        lost = STREAM_LOST;
      }
    }
    if (lost != GRP_OK) {
      stream_.group_base = UINT32_MAX;
      return lost;
    }
  }
  const uint32_t g = j - stream_.group_base;
  d = stream_.stripe_recv[(size_t)(g / C) * CB + 1 + g % C];
  return GRP_OK;
}

void
Classifier::AbortTrace::on_record(uint32_t j, uint32_t S)
{
  if (j == 0) {
    t_first += secs(after_launch, Clock::now());
  }
  if (resume_pending) { // the first record behind an insert the launch applied itself
    resume_pending = false;
    t_resume += secs(resume0, Clock::now());
    if (each) {
      fprintf(stderr, "insert behind read %u of a window of %u (launched %.1f us ago): %.1f us to the first record behind it\n", j - 1, S, 1e6 * secs(after_launch, resume0), 1e6 * secs(resume0, Clock::now()));
    }
    if ((++n_resumed & 511u) == 0) {
      fprintf(stderr, "in-launch inserts %llu: %.1f us from the insert record to the first record behind it\n", (unsigned long long)n_resumed, 1e6 * t_resume / n_resumed);
    }
  }
}

void
Classifier::AbortTrace::on_committed(bool in_launch, bool stale)
{
  if (in_launch) {
    resume0 = Clock::now();
    resume_pending = true;
  }
  if (stale) {
    t_commit_ins += secs(commit0, Clock::now());
  }
}

void
Classifier::AbortTrace::on_dropped()
{
  t_drop += secs(drop0, Clock::now());
  ++n_stale;
  if ((n_stale & 1023u) == 0) {
    fprintf(stderr, "stream rounds %llu, ended by an insert %llu: per round launch call %.1f us, first record %.1f us; per insert commit+insert call %.1f us, drop (drain + insert kernels) %.1f us\n",
            (unsigned long long)n_rounds, (unsigned long long)n_stale, 1e6 * t_launch / n_rounds, 1e6 * t_first / n_rounds, 1e6 * t_commit_ins / n_stale, 1e6 * t_drop / n_stale);
  }
}

// The next window goes in shortly before the current launch runs out of work (stream_round asks from 256 reads per
// rank before its end): early enough to start back to back (the GPU is at most ~100 reads ahead of the host), late
// enough that an insert rarely has to abort it.  `pos`: the read behind the current window.
int
Classifier::queue_next_stream(uint32_t pos, bool& refused)
{
  const Plan plan = window_plan();
  if (!plan.streaming) {
    return GRP_OK;
  }
  // queued right behind the current launch
  const int rc = launch_stream(rg_.reads, pos, std::min<uint32_t>(plan.S, rg_.n - pos), stream_.cur.slot ^ 1u, stream_.next);
  if (rc == GRP_ERR_BUSY) {
    // the engine would have to wait for the device (buffers to grow) while the current window
    // may be waiting for this thread: the next window is begun when this one has ended
    refused = true;
    return GRP_OK;
  }
  return rc;
}

// Several ranks, behind an insert handed to the launches: this rank's launch may have left before the command came
// (its own stripes were decided; the read is another rank's) — then the window queued behind it must not go on
// unnoticed on a replica without the insert.  The launch answers within the time the owner's launch takes to apply
// it (the ranks wait for its next record anyway).
int
Classifier::await_insert_taken()
{
  for (;;) {
    const int st = vt_.stream_insert_done(ctx_, stream_.cur.slot);
    if (st == 1) {
      return GRP_OK;
    }
    if (st == 2) {
      stream_.ins_lost = true; // said in the next exchange: every rank ends the round there (end_stream applies the insert the classic way)
      return GRP_OK;
    }
    if (st < 0) {
      return engine_failed("stream_insert_done", st);
    }
    __builtin_ia32_pause();
  }
}

// Several ranks: the window's last record was an insert the launches took — one more exchange, of the headers alone:
// a rank whose launch had left before the command must not begin the next window by itself while the others carry on
// with theirs
int
Classifier::confirm_last_insert(bool& lost)
{
  int rc = GRP_OK;
  gr_read_decision mine{};
  mine.kind = stream_.ins_lost ? 1u : 0u;
  std::vector<gr_read_decision> all(p_.world);
  if (allgather_cb_(ag_user_, &mine, sizeof(mine), all.data()) != 0) {
    err_ = "allgather callback failed";
    rc = GRP_ERR_INVALID;
  }
  for (uint32_t q = 0; q < p_.world && rc == GRP_OK; ++q) {
    lost = lost || all[q].kind != 0;
  }
  stream_.ins_unconfirmed = false;
  return rc;
}

// ---- streaming window: consume the decisions while the launch is running ----------
// A round ends with the window (every record committed) or early: `stale` — a record inserted and the launches were
// ended for it; `redo` — the engine handed the read back (kind 0), the synchronous path takes it; `lost` — a launch
// had left without a record it owed, the window is begun again at this read.  An insert the parked launch applies
// itself (`resume`) ends nothing: the records behind it come under the next generation.
int
Classifier::stream_round(uint32_t& pos)
{
  const uint32_t n = rg_.n;
  AbortTrace& trace = stream_.trace;
  int rc = GRP_OK;
  trace.round_begins();
  if (stream_.next.active) {
    stream_.cur = stream_.next; // starts at pos: an insert would have aborted it
    stream_.next.active = false;
  } else {
    const Plan plan = window_plan();
    rc = launch_stream(rg_.reads, pos, std::min<uint32_t>(plan.S, n - pos), 0, stream_.cur);
    if (rc != GRP_OK) {
      return rc;
    }
  }
  const uint32_t S = stream_.cur.S;
  stream_.group_base = UINT32_MAX;
  stream_.group_from = 0;
  stream_.ins_lost = false;
  stream_.ins_unconfirmed = false;
  uint32_t j = 0;
  bool stale = false, redo = false, lost = false, next_refused = false;
  trace.launched();
  while (j < S) {
    if (!stream_.next.active && !next_refused && j + 256 * p_.world >= S && pos + S < n) {
      rc = queue_next_stream(pos + S, next_refused);
      if (rc != GRP_OK) {
        break;
      }
    }
    gr_read_decision d;
    rc = stream_decision(j, d);
    if (rc == STREAM_LOST) {
      rc = GRP_OK;
      lost = true;
      break;
    }
    if (rc != GRP_OK) {
      break;
    }
    trace.record(j, S);
    d.pad = 0;
    // (1 / 1024: a record handed back is priced as what it is over the last ~1000 reads.  With 1 / 64 a SINGLE read of
    // more than 256 tiles — one in 70 000 with a realistic ONT length tail — made the streaming windows look 2.6 x as
    // expensive as they are and the plan left them for ~45 synchronous windows: 146 such reads cost the C2 stream 5 s,
    // bench.py --len-sigma 0.6, profiles/r04_long_tail.txt)
    p_redo_ += (1.0 / 1024.0) * ((d.kind == 0 ? 1.0 : 0.0) - p_redo_);
    stat_.stream_handbacks += d.kind == 0 ? 1 : 0;
    if (d.kind == 0) {
      redo = true; // needs the worst-case table / a larger arena: synchronous path below
      break;
    }
    bool resume = false;
    if (d.kind == DEC_INSERT_WHOLE || d.kind == DEC_INSERT_TRIMMED) {
      // One rank: the parked launch applies the insert itself and carries on behind the read
      // (commit() hands it over).  Otherwise everything behind this read is
      // stale: stop the launches before the insert is queued.
      resume = stream_.cur.resumable;
      if (resume) {
        stream_.ins = &stream_.cur;
        stream_.ins_ok = false;
      } else {
        (void)vt_.stream_abort(ctx_, stream_.cur.slot);
        if (stream_.next.active) {
          (void)vt_.stream_abort(ctx_, stream_.next.slot);
        }
        stale = true;
      }
    }
    trace.commit_begins();
    commit_one(pos + j, d, rc);
    if (resume) {
      stream_.ins = nullptr;
      stale = !stream_.ins_ok; // the engine refused (the launches were aborted, the insert queued behind them)
      if (!stale && p_.world > 1) {
        // the launches carry on behind the read under the next generation: the rest of its stripe group is exchanged again
        stream_.group_base = UINT32_MAX;
        stream_.group_from = j + 1;
        stream_.ins_unconfirmed = true;
        const int e = await_insert_taken();
        if (e != GRP_OK) {
          rc = e;
        }
      }
    }
    trace.committed(resume && !stale, stale);
    if (rc != GRP_OK) {
      break;
    }
    ++j;
    if (stale || finished_) {
      break;
    }
  }
  pos += j;
  if (rc == GRP_OK && p_.world > 1 && stream_.ins_unconfirmed && !lost) {
    rc = confirm_last_insert(lost);
  }
  if (rc != GRP_OK || stale || finished_ || redo || lost) {
    trace.drop_begins();
    const int drc = drop_streams();
    if (rc == GRP_OK) {
      rc = drc;
    }
    trace.dropped();
  } else {
    if (p_.world > 1) {
      (void)vt_.stream_abort(ctx_, stream_.cur.slot); // every read of the window is committed: a striped window that takes inserts stays until it is told
    }
    rc = end_stream(stream_.cur); // completed: returns at once
    if (rc != GRP_OK) {
      drop_streams();
    }
  }
  if (rc == GRP_OK && redo && !finished_) {
    // one read through the synchronous path (it redoes flagged tiles / grows the arena)
    rc = query_window(rg_.reads, pos, 1);
    if (rc == GRP_OK) {
      commit_one(pos, dec_all_[0], rc);
      ++pos;
    }
  }
  return rc;
}

} // namespace gr
