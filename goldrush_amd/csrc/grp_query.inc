// libgrpath_hip.so: the k_query launch — the count table's geometry, the launch's description and argument pack
// (QueryLaunch, query_args), the choice of the kernel form, and grp_query_tiles.  Included by grpath_hip.hip; the words
// the launch shares with the host are grp_stream_proto.h's.

namespace {

constexpr uint32_t GT_SLICE = 256;                     // workgroups of one launch with global count tables

struct QueryGeom
{
  uint32_t hist_cap;       // slots of the per-tile count table (even; 6 bytes each: a key and a 16-bit count)
  uint32_t distinct_limit; // distinct IDs it takes (the rest is room for the claims in flight)
  size_t lds;
  bool global_table = false; // the worst-case table does not fit the LDS: it lives in global memory (k_query<..., GT>; the redo launches only)
};

// The per-tile count table (k_query).  full = worst case: every probe of the tile a different ID — tile * h slots
// plus one claim per lane and seed in flight.  Round 4: at 6 bytes per slot and without power-of-two rounding the
// worst case of the default geometries fits the LDS share that lets three workgroups (h = 5: 48 KB) or four (h = 3:
// 27 KB) onto a CU, so it is what every launch uses and no tile is flagged; only geometries beyond that (h = 8 with
// tiles of 1000: 69 KB; long tiles) keep the two-step scheme: a table of the budget's size first, the tiles whose
// distinct IDs do not fit flagged and recomputed by the same kernel with the worst-case table.
QueryGeom
query_geom(const grp_ctx* c, bool full)
{
  const uint32_t h = c->params.h, tile = c->params.tile;
  const uint64_t max_ids = (uint64_t)tile_frames(c) * h; // (tile + 1 frames at odd k)
  auto lds_of = [&](uint32_t cap) { return tab_bytes(c) + (size_t)cap * 6 + bases_bytes(tile + c->params.k + h); };
  const uint32_t cap_full = (uint32_t)((max_ids + (uint64_t)THREADS * h + 2 + 1023) / 1024 * 1024);
  const uint32_t forced_small = c->sw.small_hist; // developer hook / tests (GRP_SMALL_HIST, read when the context is created): slots of the first-step table — forces the two-step scheme
  QueryGeom g;
  g.hist_cap = cap_full;
  if (!full) {
    if (forced_small && forced_small < cap_full && forced_small > (uint32_t)THREADS * h + 64) {
      g.hist_cap = forced_small;
    } else if (lds_of(cap_full) > 52 * 1024) {
      // the largest table that still lets three workgroups share a CU's 160 KB
      const size_t fixed = lds_of(0);
      const uint32_t cap = (uint32_t)((52 * 1024 - std::min<size_t>(fixed, 40 * 1024)) / 6 / 1024 * 1024);
      if (cap > (uint32_t)THREADS * h + 1024 && cap < cap_full) {
        g.hist_cap = cap;
      }
    }
    if (g.hist_cap == cap_full && lds_of(cap_full) > LDS_PER_WORKGROUP) {
      // no room for the three-workgroups table beside large seed tables (h > 8 of heavy seeds): the largest table
      // the LDS takes, the tiles it cannot hold redone with the worst-case one
      const size_t fixed = lds_of(0);
      const uint32_t cap = fixed < LDS_PER_WORKGROUP ? (uint32_t)((LDS_PER_WORKGROUP - fixed) / 6 / 1024 * 1024) : 0u;
      if (cap > (uint32_t)THREADS * h + 64) {
        g.hist_cap = cap;
      }
    }
  }
  g.distinct_limit = g.hist_cap - THREADS * h - 1;
  g.lds = lds_of(g.hist_cap);
  if (full && g.lds > LDS_PER_WORKGROUP) {
    // Round 5: tiles beyond ~9 000 frames at h = 3 (the reference has no such limit).  The first step's table is LDS-sized
    // (above: the three-workgroups budget); what it cannot hold is redone with the worst-case table in global memory.
    g.global_table = true;
    g.lds = lds_of(0);
  }
  return g;
}

// One k_query launch as the host describes it: QueryLaunch{ n, t0, g, list_cap } is tiles [0, n) of a window into the
// slot's buffers, and a call site names what differs from that.
struct QueryLaunch
{
  uint64_t n_launch = 0;                 // workgroups: tiles of the launch
  uint64_t t0 = 0;                       // the window's first tile in the batch
  QueryGeom g{};
  uint64_t list_cap = 0;
  const uint32_t* d_tile_idx = nullptr;  // a tile list (window indices); none: the launch covers tiles [blk0, blk0 + n_launch) of the window
  grp_tile_summary* out_tiles = nullptr; // none: the slot's d_tiles / d_lists
  grp_id_count* out_lists = nullptr;
  uint32_t direct_stride = 0;            // list entries per tile of the zero-copy path
  const DevStreamCtl* stream_ctl = nullptr;
  uint32_t blk0 = 0;
  bool list_flags = false;               // a tile list that is NOT the redo of flagged tiles: flagged tiles are collected as without a list
  bool plain = false;                    // the plain query even while a batch view is set (the reads behind the batch)
};

// k_query's arguments, in its parameters' order
struct QueryArgs
{
  DevFilter f;
  DevReads rd;
  const DevSeeds* sd;
  uint32_t tile;
  uint64_t t0;
  const uint32_t* idx;
  uint32_t cap, lim;
  grp_tile_summary* tiles;
  grp_id_count* lists;
  uint64_t lcap;
  unsigned long long* ctr;
  uint32_t* flag;
  uint32_t fcap, ds, blk0;
  DevStreamCtl sc;
  DevBatchView bv;
  uint32_t* gtab;

  template<typename K>
  void launch(K kern, uint32_t grid, size_t lds, hipStream_t stream) const
  {
    kern<<<dim3(grid), dim3(THREADS), lds, stream>>>(f, rd, sd, tile, t0, idx, cap, lim, tiles, lists, lcap, ctr, flag, fcap, ds, blk0, sc, bv, gtab);
  }
  template<typename K>
  hipError_t launch_cooperative(K kern, uint32_t grid, size_t lds, hipStream_t stream)
  {
    void* args[] = { &f, &rd, &sd, &tile, &t0, &idx, &cap, &lim, &tiles, &lists, &lcap, &ctr, &flag, &fcap, &ds, &blk0, &sc, &bv, &gtab };
    return hipLaunchCooperativeKernel(reinterpret_cast<const void*>(kern), dim3(grid), dim3(THREADS), args, (unsigned int)lds, stream);
  }
};

// The argument pack of a launch: which flag buffer, which view of the ID array and which stream control it gets is
// decided here, for every form of the launch.
QueryArgs
query_args(const grp_ctx* c, const grp_reads* r, const QueryLaunch& q)
{
  const QuerySlot& sl = *c->q;
  QueryArgs a{};
  a.f = c->f;
  a.rd = r->dev;
  a.sd = c->d_seeds;
  a.tile = c->params.tile;
  a.t0 = q.t0;
  a.idx = q.d_tile_idx;
  a.cap = q.g.hist_cap;
  a.lim = q.g.distinct_limit;
  a.tiles = q.out_tiles ? q.out_tiles : sl.d_tiles.p;
  a.lists = q.out_tiles ? q.out_lists : sl.d_lists.p;
  a.lcap = q.list_cap;
  a.ctr = reinterpret_cast<unsigned long long*>(sl.d_qctr.p);
  a.flag = (q.d_tile_idx && !q.list_flags) ? nullptr : sl.d_flag_idx.p; // the redo of flagged tiles flags nothing
  a.fcap = (uint32_t)sl.d_flag_idx.cap;
  a.ds = q.direct_stride;
  a.blk0 = q.blk0;
  a.sc = q.stream_ctl ? *q.stream_ctl : DevStreamCtl{};
  a.bv = (c->view && !q.plain) ? *c->view : DevBatchView{}; // grp_batch_classify: every read sees the state in front of its own insert
  a.gtab = q.g.global_table ? c->d_gtab.p : nullptr;
  return a;
}

template<int HH, int QWT>
int
launch_query_wt(grp_ctx* c, const grp_reads* r, QueryLaunch q)
{
  const QueryGeom& g = q.g;
  size_t launch_lds = g.lds; // dynamic LDS of the launch (the streaming form adds its fingerprint buffers)
  auto go = [&](auto kern) -> int {
    int rc = ensure_lds(c, kern, launch_lds);
    if (rc != GRP_OK) {
      return rc;
    }
    QueryArgs a = query_args(c, r, q);
    if (q.stream_ctl && q.stream_ctl->ctl) {
      // A window that applies inserts itself: its workgroups wait for each other inside the launch.  The grid is sized
      // from the occupancy query below and launched cooperatively — the runtime checks that it fits the device (or
      // refuses: another process on it; ADVICE r03).  That is a check of sizes, not of residency: now and then a few
      // workgroups begin only when others leave, so the waits count the workgroups that have begun (stream_register).
      // GRP_ERR_BUSY: refused — the caller begins the window in its classic form (it ends where it parks).
      const hipError_t e = a.launch_cooperative(kern, (uint32_t)q.n_launch, launch_lds, c->stream);
      if (e == hipSuccess) {
        return GRP_OK;
      }
      (void)hipGetLastError();
      return set_err(c, GRP_ERR_BUSY, "cooperative launch of a resumable window refused: %s", hipGetErrorString(e));
    }
    a.launch(kern, (uint32_t)q.n_launch, launch_lds, c->stream);
    return GRP_OK;
  };
  // The synchronous forms (large windows, the two queries of a batch): two frames per lane and pass
  // up to h = 3; from h = 4 on one frame per lane with the software-pipelined pass (222 -> 171 VGPRs
  // at h = 5; C4 geometry +4 %, h = 3 -3 %: measured, tools/dev/r3_fr1.sh of round 3; round 4 again with the 24 KB count table:
  // the head of C2 2.94 - 3.04 s against 2.94 - 2.96 s, no gain, the switch is gone)
  constexpr int SFR = (HH <= 3) ? 2 : 1;
  if (g.global_table) {
    // the worst-case table in global memory, GT_SLICE workgroups (and tables) per launch
    if (q.stream_ctl || q.direct_stride) {
      return set_err(c, GRP_ERR_STATE, "launch_query: a global count table in a streaming / zero-copy launch");
    }
    const uint64_t words = (uint64_t)g.hist_cap + g.hist_cap / 2u;
    if (const int rc = ensure_dev(c, c->d_gtab, words * GT_SLICE); rc != GRP_OK) {
      return rc;
    }
    const bool ver = c->view && !q.plain;
    QueryArgs a = query_args(c, r, q);
    for (uint64_t off = 0; off < q.n_launch; off += GT_SLICE) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(GT_SLICE, q.n_launch - off);
      a.idx = q.d_tile_idx ? q.d_tile_idx + off : nullptr;
      a.blk0 = q.d_tile_idx ? q.blk0 : q.blk0 + (uint32_t)off;
      if (ver) {
        if (a.bv.redo_count && off) {
          break; // (a launch sized before its list was known covers one slice: longer lists take the host's way)
        }
        auto kern = k_query<HH, 1, QWT, false, true, true>;
        if (const int rc = ensure_lds(c, kern, g.lds); rc != GRP_OK) {
          return rc;
        }
        a.launch(kern, nb, g.lds, c->stream);
      } else {
        auto kern = k_query<HH, 1, QWT, false, false, true>;
        if (const int rc = ensure_lds(c, kern, g.lds); rc != GRP_OK) {
          return rc;
        }
        a.launch(kern, nb, g.lds, c->stream);
      }
    }
    return GRP_OK;
  }
  if (c->view && !q.stream_ctl && !q.plain) { // grp_batch_classify: every read sees the state in front of its own insert
    return go(k_query<HH, SFR, QWT, false, true>);
  }
  if (q.stream_ctl) {
    // persistent workgroups: exactly what is resident at once
    // one frame per lane and pass: fewer registers, more resident workgroups — measured
    // better than two for the persistent form (h = 3: +3 %, h = 5: +19 %)
    auto kern = k_query<HH, 1, QWT, true>;
    int per_cu = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, THREADS, g.lds));
    // Round 6: a window that applies inserts itself keeps the probes' fingerprints of the tile in progress and of the
    // tile before it in LDS (DevStreamCtl::n_fp) — as many of the two buffers as fit WITHOUT costing a resident workgroup
    // (three per CU is what the launch runs at, below — or fewer, where the kernel's registers allow no more): C2's geometry
    // 27.9 + 2 x 12.3 KB, three of them in the CU's 160 KB; h = 5 with tiles of 1000 (48 KB of count table) would have no
    // room beside three, but it does keep on the MI355X (its instance must be resident twice per CU there: ONE buffer, 25 KB,
    // fits beside that).  h = 5 with tiles of 1500 (one buffer: 36 KB) has no room: such a window hands everything behind an insert out
    // again (tests/test_gpu_stream_striped.py holds both).
    DevStreamCtl sc_fit = *q.stream_ctl;
    QueryGeom g_fit = g;
    sc_fit.n_fp = 0;
    if (q.stream_ctl->ctl && q.stream_ctl->n_fp) {
      const int keep_env = c->sw.stream_keep; // GRP_STREAM_KEEP, developer switch / tests: fingerprint buffers per workgroup (0: rounds 3 - 5's form)
      const uint32_t fb = gr::geom::helper_pass_frames(HH); // frames per pass at least (k_query: the helper-lane layout)
      const uint32_t passes = (tile_frames(c) + fb - 1u) / fb;
      const uint32_t words = passes * (uint32_t)THREADS * (uint32_t)HH;
      const int want_cu = std::min(per_cu, 3);
      for (int nf = std::min<int>(keep_env, (int)q.stream_ctl->n_fp); nf >= 1; --nf) {
        const size_t lds = g.lds + (size_t)nf * words * 4u;
        int fit = 0;
        if (lds <= LDS_PER_WORKGROUP && ensure_lds(c, kern, lds) == GRP_OK && hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kern, THREADS, lds) == hipSuccess && fit >= want_cu) {
          sc_fit.n_fp = (uint32_t)nf;
          sc_fit.fp_off = (uint32_t)g.lds;
          sc_fit.fp_words = words;
          g_fit.lds = lds;
          break;
        }
        (void)hipGetLastError();
      }
    }
    q.stream_ctl = &sc_fit;
    launch_lds = g_fit.lds; // (the launch takes the geometry with the fingerprint buffers)
    int rc = ensure_lds(c, kern, launch_lds);
    if (rc != GRP_OK) {
      return rc;
    }
    const int cap_per_cu = c->sw.stream_wgs_per_cu; // GRP_STREAM_WGS_PER_CU, developer hook
    // 3 .. 6 resident workgroups per CU run equally fast (the kernel is bound by the DRAM
    // access rate, not by occupancy); 4 keeps the amount of work in flight — what an abort
    // throws away — small and leaves room on every CU for other kernels (copies, a
    // collective) beside the persistent launch
    // Round 4: THREE, not four.  With the 24 KB count table a fourth workgroup fits a CU by LDS and VGPRs (128: four
    // waves per SIMD, every wave slot of the device), and the occupancy query — and hipLaunchCooperativeKernel — say
    // so; but the launch then is NOT fully resident in practice (the kernel keeps 4 VGPRs in scratch, and the
    // dispatcher admits fewer scratch waves than wave slots): on the C1 stream the grid-wide waits of the in-launch
    // insert timed out (inserts handed back to the host: 243 k reads/s instead of 489 k, or code 2 with the
    // cooperative launch), profiles/r04_c1_workgroups_per_cu.txt.  Rounds 1 - 3 ran three (the 43.6 KB table allowed
    // no more); three leave a wave slot per SIMD free, and are as fast (C1 559 k reads/s in the steady state, two: 500 k).
    per_cu = std::min(per_cu, cap_per_cu > 0 ? cap_per_cu : 3);
    const uint64_t resident = std::min<uint64_t>((uint64_t)std::max(per_cu, 1) * (uint64_t)std::max(c->n_cus, 1), STREAM_REL_WGS);
    q.n_launch = std::min<uint64_t>(q.n_launch, resident);
    c->dbg_stream_lds = (uint32_t)launch_lds;
    c->dbg_stream_grid = (uint32_t)q.n_launch;
    return go(kern);
  }
  // (round 2 had a second form for windows of a few reads, the care loop unrolled for weight-16
  // seeds: 346 VGPRs + 14 spilled at h = 3.  With the shared halves the hash is a third of the
  // instructions it was and the batches took the insert-heavy phases over: the form is gone — the
  // CLI's silver run takes the same time with and without it, tools/dev/r3_latform.sh.)
  return go(k_query<HH, SFR, QWT, false>);
}

// The query of `n_launch` tiles in the form of the context's h and hash form (QWT of launch_query_wt: 0, or GRP_WT_LONG
// for seeds of spans beyond 64 bases)
int
launch_query(grp_ctx* c, const grp_reads* r, const QueryLaunch& q)
{
  int rc = GRP_OK;
  DISPATCH_H_SPAN(c, (rc = launch_query_wt<HH, WW>(c, r, q)));
  return rc;
}

struct QueryRun
{
  uint64_t t0 = 0, nt = 0, probes = 0;
  uint64_t used = 0;    // list arena entries
  uint64_t flagged = 0; // tiles redone with the worst-case geometry
};

// a slot's tile summaries, list arena and flagged-tile indices for a window of `nt` tiles
int
slot_query_bufs(grp_ctx* c, QuerySlot& sl, uint64_t nt, uint64_t lists)
{
  HIP_TRY(c, sl.d_tiles.ensure(nt));
  HIP_TRY(c, sl.d_lists.ensure(lists));
  HIP_TRY(c, sl.d_flag_idx.ensure(nt));
  return GRP_OK;
}

// a slot's decide scratch for a window of `nt` tiles: three arrays of one capacity
int
slot_dec_scratch(grp_ctx* c, QuerySlot& sl, uint64_t nt)
{
  if (nt + 1 > sl.d_dec_cap) {
    clear_all(sl.d_dec_ids, sl.d_dec_asg, sl.d_dec_scratch);
    sl.d_dec_cap = 0;
    const uint64_t cap = nt + nt / 4 + 64;
    HIP_TRY(c, sl.d_dec_ids.reset(cap));
    HIP_TRY(c, sl.d_dec_asg.reset(cap));
    HIP_TRY(c, sl.d_dec_scratch.reset(cap));
    sl.d_dec_cap = cap;
  }
  return GRP_OK;
}

uint64_t
count_probes(const grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count)
{
  uint64_t probes = 0;
  for (uint32_t i = first; i < first + count; ++i) {
    const uint32_t ntile = r->len[i] / c->params.tile;
    if (ntile == 0) {
      continue;
    }
    // all tiles but the last are full; the last may be clipped
    probes += ((uint64_t)(ntile - 1) * tile_frames(c) + tile_extent(c, r->len[i], ntile - 1).frames) * c->params.h;
  }
  return probes;
}

// Enqueue the query kernel for the window (results stay in c->q->d_tiles /
// c->q->d_lists).  No synchronisation.
int
enqueue_query(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, uint64_t list_cap, QueryRun& q)
{
  q.t0 = r->tile0[first];
  q.nt = r->tile0[first + count] - q.t0;
  q.probes = count_probes(c, r, first, count);
  if (const int rc = slot_query_bufs(c, *c->q, q.nt, std::max<uint64_t>(list_cap, 1)); rc != GRP_OK) {
    return rc;
  }
  if (c->q->side_used) {
    // the slot's previous window may still be in its decision kernel on the other stream
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->q->done, 0));
    c->q->side_used = false;
  }
  const QueryGeom g = query_geom(c, false);
  Timer t(c, GRP_K_QUERY, q.probes);
  int lrc = launch_query(c, r, QueryLaunch{ q.nt, q.t0, g, list_cap });
  if (lrc != GRP_OK) {
    return lrc;
  }
  HIP_TRY(c, hipGetLastError());
  return GRP_OK;
}

// tiles whose ID set did not fit the small LDS table (indices collected on the
// device): redo them with the worst-case geometry — same kernel, same arithmetic.
// Expects h_qctr to hold the counters of the first launch.
int
enqueue_redo_flagged(grp_ctx* c, const grp_reads* r, uint64_t list_cap, QueryRun& q)
{
  q.flagged = c->q->h_qctr[QCTR_FLAGGED];
  c->n_flagged_tiles += q.flagged;
  c->n_flagged_distinct += c->q->h_qctr[QCTR_FLAGGED_DISTINCT];
  c->n_flagged_list += c->q->h_qctr[QCTR_FLAGGED_LIST];
  ++c->n_redo_launches;
  // continue the list arena where the first launch stopped
  uint64_t cursor[QCTR_WORDS] = {};
  cursor[QCTR_LIST_CURSOR] = c->q->h_qctr[QCTR_LIST_CURSOR];
  HIP_TRY(c, hipMemcpyAsync(c->q->d_qctr, cursor, sizeof(cursor), hipMemcpyHostToDevice, c->stream));
  Timer t(c, GRP_K_QUERY, 0);
  QueryLaunch ql{ q.flagged, q.t0, query_geom(c, true), list_cap };
  ql.d_tile_idx = c->q->d_flag_idx;
  int lrc = launch_query(c, r, ql);
  if (lrc != GRP_OK) {
    return lrc;
  }
  HIP_TRY(c, hipGetLastError());
  return GRP_OK;
}

} // namespace

extern "C" {

int
grp_query_tiles(grp_ctx* c,
                const grp_reads* r,
                uint32_t first,
                uint32_t count,
                grp_tile_summary* tiles_out,
                grp_id_count* lists_out,
                uint64_t list_cap,
                uint64_t* list_used,
                grp_query_stats* stats)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads) {
    return set_err(c, GRP_ERR_INVALID, "grp_query_tiles: bad range");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_query_tiles before grp_finalize");
  }
  if (c->slot[0].busy) {
    return set_err(c, GRP_ERR_STATE, "grp_query_tiles while an asynchronous window is in flight in slot 0");
  }
  c->q = &c->slot[0];
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->q->side_used) {
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->q->done, 0));
    c->q->side_used = false;
  }
  const uint64_t nt = r->tile0[first + count] - r->tile0[first];
  if (list_used) {
    *list_used = 0;
  }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
  }
  if (nt == 0) {
    return GRP_OK;
  }
  if (nt > MAX_GRID_WGS) {
    return set_err(c, GRP_ERR_INVALID, "grp_query_tiles: %llu tiles in one call (limit 2^22)", (unsigned long long)nt);
  }
  if (!tiles_out) {
    return set_err(c, GRP_ERR_INVALID, "grp_query_tiles: tiles_out is NULL");
  }
  if (nt <= SMALL_TILES && !c->sw.no_direct) { // (GRP_NO_DIRECT, developer hook: force the general path)
    // latency path (insert-heavy phases query one read at a time): the kernel
    // writes summaries and lists straight into mapped host memory, no copies,
    // no counters; one stream synchronisation
    const uint64_t t0 = r->tile0[first];
    const uint64_t probes = count_probes(c, r, first, count);
    constexpr uint32_t PENDING = 0xFFFFFFFEu; // list_n of a summary the kernel has not written yet
    for (uint64_t i = 0; i < nt; ++i) {
      c->h_small_tiles[i].list_n = PENDING;
    }
    {
      QueryLaunch ql{ nt, t0, query_geom(c, false), (uint64_t)SMALL_TILES * SMALL_STRIDE };
      ql.out_tiles = c->h_small_tiles.dev;
      ql.out_lists = c->h_small_lists.dev;
      ql.direct_stride = SMALL_STRIDE;
      Timer t(c, GRP_K_QUERY_LAT, probes);
      int lrc = launch_query(c, r, ql);
      if (lrc != GRP_OK) {
        return lrc;
      }
    }
    HIP_TRY(c, hipGetLastError());
    // the summaries arrive in host memory while the launch runs (lists first, the word with
    // list_n last): spin on them instead of waiting for the end-of-kernel signal; a launch
    // that never delivers falls back to the stream synchronisation
    {
      uint64_t i = 0;
      uint32_t spins = 0;
      while (i < nt) {
        if (__atomic_load_n(&c->h_small_tiles[i].list_n, __ATOMIC_ACQUIRE) != PENDING) {
          ++i;
          continue;
        }
        __builtin_ia32_pause();
        if ((++spins & 0xFFFFu) == 0 && hipStreamQuery(c->stream) != hipErrorNotReady) {
          HIP_TRY(c, hipStreamSynchronize(c->stream));
          for (uint64_t j = i; j < nt; ++j) {
            if (__atomic_load_n(&c->h_small_tiles[j].list_n, __ATOMIC_ACQUIRE) == PENDING) {
              return set_err(c, GRP_ERR_HIP, "grp_query_tiles: the launch ended without delivering tile %llu", (unsigned long long)j);
            }
          }
          break;
        }
      }
    }
    ++c->n_direct_windows;
    bool any_flagged = false;
    uint64_t used = 0;
    for (uint64_t i = 0; i < nt; ++i) {
      any_flagged = any_flagged || c->h_small_tiles[i].list_n == GRP_TILE_FLAGGED;
      used += c->h_small_tiles[i].list_n;
    }
    if (!any_flagged) {
      if (list_used) {
        *list_used = used;
      }
      if (used > list_cap) {
        return set_err(c, GRP_ERR_NOMEM, "grp_query_tiles: %llu list entries needed, capacity %llu", (unsigned long long)used, (unsigned long long)list_cap);
      }
      uint64_t off = 0;
      for (uint64_t i = 0; i < nt; ++i) {
        grp_tile_summary ts = c->h_small_tiles[i];
        grp_id_count* src = c->h_small_lists + i * SMALL_STRIDE;
        if (ts.list_n) {
          memcpy(lists_out + off, src, ts.list_n * sizeof(grp_id_count));
          if (ts.list_n > 1) {
            std::sort(lists_out + off, lists_out + off + ts.list_n, [](const grp_id_count& a, const grp_id_count& b) {
              return a.count != b.count ? a.count > b.count : a.id < b.id;
            });
          }
        }
        ts.list_off = (uint32_t)off;
        off += ts.list_n;
        tiles_out[i] = ts;
        if (stats) {
          stats->hits += ts.hits;
          stats->misses += ts.misses;
        }
      }
      if (stats) {
        stats->queries = probes / c->params.h;
      }
      return GRP_OK;
    }
    // a tile needs the worst-case table or a longer list: take the general path
    ++c->n_direct_fallbacks;
  }
  if (nt > c->h_tiles.cap) {
    HIP_TRY(c, c->h_tiles.reset(std::max<uint64_t>(nt + nt / 4, 4096), hipHostMallocDefault));
  }
  ++c->n_general_windows;
  QueryRun q;
  int rc = enqueue_query(c, r, first, count, list_cap, q);
  if (rc != GRP_OK) {
    return rc;
  }
  const uint64_t prefix = std::min<uint64_t>(list_cap, LIST_PREFIX);
  // one round trip: counters, tile summaries and the first LIST_PREFIX list
  // entries come back together; the counters are re-zeroed for the next call
  auto fetch = [&]() -> int {
    HIP_TRY(c, hipMemcpyAsync(c->q->h_qctr, c->q->d_qctr, QCTR_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_tiles, c->q->d_tiles, nt * sizeof(grp_tile_summary), hipMemcpyDeviceToHost, c->stream));
    if (prefix) {
      HIP_TRY(c, hipMemcpyAsync(c->h_lists, c->q->d_lists, prefix * sizeof(grp_id_count), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(c->q->d_qctr, 0, QCTR_WORDS * sizeof(uint64_t), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GRP_OK;
  };
  rc = fetch();
  if (rc != GRP_OK) {
    return rc;
  }
  if (c->q->h_qctr[QCTR_FLAGGED]) {
    rc = enqueue_redo_flagged(c, r, list_cap, q);
    if (rc == GRP_OK) {
      rc = fetch();
    }
    if (rc != GRP_OK) {
      return rc;
    }
  }
  drain_events(c);
  memcpy(tiles_out, c->h_tiles, nt * sizeof(grp_tile_summary));
  const uint64_t used = c->q->h_qctr[QCTR_LIST_CURSOR];
  if (list_used) {
    *list_used = used;
  }
  if (stats) {
    stats->queries = q.probes / c->params.h; /* one query per frame (goldrush_path.cpp:567-568) */
    for (uint64_t i = 0; i < nt; ++i) {
      stats->hits += tiles_out[i].hits;
      stats->misses += tiles_out[i].misses;
    }
  }
  if (used > list_cap) {
    return set_err(c, GRP_ERR_NOMEM, "grp_query_tiles: %llu list entries needed, capacity %llu", (unsigned long long)used, (unsigned long long)list_cap);
  }
  if (used) {
    if (!lists_out) {
      return set_err(c, GRP_ERR_INVALID, "grp_query_tiles: lists_out is NULL");
    }
    if (used <= prefix) {
      memcpy(lists_out, c->h_lists, used * sizeof(grp_id_count));
    } else {
      HIP_TRY(c, hipMemcpy(lists_out, c->q->d_lists, used * sizeof(grp_id_count), hipMemcpyDeviceToHost));
    }
    // canonical order inside each tile's list: count descending, id ascending
    for (uint64_t i = 0; i < nt; ++i) {
      grp_tile_summary& ts = tiles_out[i];
      if (ts.list_n > 1) {
        std::sort(lists_out + ts.list_off, lists_out + ts.list_off + ts.list_n, [](const grp_id_count& a, const grp_id_count& b) {
          return a.count != b.count ? a.count > b.count : a.id < b.id;
        });
      }
    }
  }
  return GRP_OK;
}

} // extern "C"
