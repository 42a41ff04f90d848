// libgrpath_hip.so: the streaming window's host side (grp_classify_stream_*) — the persistent k_query<.., ST> launch that
// publishes decisions while it runs and takes in-launch inserts.  Included by grpath_hip.hip.  What the launch and this
// thread hand each other is named in grp_stream_proto.h, the launch itself is grp_query.inc's, the stripes of a shared
// window host/gr_stream_stripes.hpp's.

extern "C" {

// ---- streaming window --------------------------------------------------------------

// the scratch table of a whole-read insert (k_insert_collect / k_insert_apply and the in-launch
// insert of a streaming window): room for `max_ranks` distinct ranks at load <= 1/2.  Growing it
// waits for the stream (never while a window that holds its address is in flight: see the caller).
static int
ensure_insert_table(grp_ctx* c, uint64_t max_ranks)
{
  const uint64_t want = next_pow2_64(max_ranks * 2);
  if (want <= c->ir_cap) {
    return GRP_OK;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  clear_all(c->d_ir_keys, c->d_ir_masks, c->d_ir_locs, c->d_ir_slots, c->d_fp_tab[0], c->d_fp_tab[1]);
  c->ir_cap = 0;
  HIP_TRY(c, c->d_fp_tab[0].reset(want));
  HIP_TRY(c, c->d_fp_tab[1].reset(want));
  HIP_TRY(c, c->d_ir_keys.reset(want));
  HIP_TRY(c, c->d_ir_masks.reset(want));
  HIP_TRY(c, c->d_ir_locs.reset(want));
  HIP_TRY(c, c->d_ir_slots.reset(want));
  HIP_TRY(c, hipMemsetAsync(c->d_ir_keys, 0, want * 8, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_ir_masks, 0, want * 8, c->stream));
  if (!c->d_ir_counter) {
    HIP_TRY(c, c->d_ir_counter.reset(2));
    HIP_TRY(c, hipMemsetAsync(c->d_ir_counter, 0, 2 * sizeof(uint32_t), c->stream));
  }
  c->ir_cap = want;
  return GRP_OK;
}

static int
stream_begin_impl(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, uint32_t stripe_reads, uint32_t n_owners, uint32_t owner, const grp_read_decision** decisions, bool want_resumable);

int
grp_classify_stream_begin(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, const grp_read_decision** decisions)
{
  return stream_begin_impl(c, r, first, count, dp, slot, 0, 1, 0, decisions, false);
}

int
grp_classify_stream_begin_striped(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, uint32_t stripe_reads, uint32_t n_owners, uint32_t owner, const grp_read_decision** decisions)
{
  return stream_begin_impl(c, r, first, count, dp, slot, stripe_reads, n_owners, owner, decisions, false);
}

int
grp_classify_stream_begin_resumable(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, const grp_read_decision** decisions)
{
  return stream_begin_impl(c, r, first, count, dp, slot, 0, 1, 0, decisions, true);
}

int
grp_classify_stream_begin_striped_resumable(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, uint32_t stripe_reads, uint32_t n_owners, uint32_t owner, const grp_read_decision** decisions)
{
  return stream_begin_impl(c, r, first, count, dp, slot, stripe_reads, n_owners, owner, decisions, true);
}

int
grp_classify_stream_insert_done(grp_ctx* c, uint32_t slot)
{
  if (!c || slot > 1 || !c->slot[slot].busy || !c->slot[slot].win.streaming) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_insert_done: no streaming window in this slot");
  }
  QuerySlot& sl = c->slot[slot];
  if (__atomic_load_n(&sl.win.h_ack[ACK_APPLIED], __ATOMIC_ACQUIRE) == sl.win.cmd_seq) {
    return 1;
  }
  if (__atomic_load_n(&sl.win.h_ack[ACK_CODE], __ATOMIC_ACQUIRE) != ACK_CODE_NONE) {
    return 2;
  }
  const hipError_t e = hipEventQuery(sl.done);
  if (e == hipSuccess) {
    return __atomic_load_n(&sl.win.h_ack[ACK_APPLIED], __ATOMIC_ACQUIRE) == sl.win.cmd_seq ? 1 : 2;
  }
  if (e != hipErrorNotReady) {
    return set_err(c, GRP_ERR_HIP, "grp_classify_stream_insert_done: %s", hipGetErrorString(e));
  }
  return 0;
}

int
grp_classify_stream_resumable(grp_ctx* c, uint32_t slot)
{
  if (!c || slot > 1 || !c->slot[slot].busy || !c->slot[slot].win.streaming) {
    return 0;
  }
  return c->slot[slot].win.resumable ? 1 : 0;
}

// What a streaming window of `count` reads and `nt` tiles needs of its slot's buffers, in elements.  stream_begin_impl
// asks whether any of them exceeds its buffer (the no-grow guard) and allocates by the same numbers.  The tile list of a
// striped window (h_ / d_stripe_tiles) is sized by ownership and is NOT among them: it still grows behind the guard.
struct StreamNeeds
{
  uint64_t sdec, tiles_done, dec_tiles, tiles, lists, tile_ver; // (tiles: d_tiles and d_flag_idx; dec_tiles: slot_dec_scratch takes one more)
  bool exceed(const QuerySlot& sl) const
  {
    return sdec > sl.win.h_sdec.cap || tiles_done > sl.win.d_tiles_done.cap || dec_tiles + 1 > sl.d_dec_cap || tiles > sl.d_tiles.cap || lists > sl.d_lists.cap ||
           tiles > sl.d_flag_idx.cap || tile_ver > sl.win.d_tile_ver.cap;
  }
};

static StreamNeeds
stream_needs(uint32_t count, uint64_t nt, bool want_resumable)
{
  const uint64_t tiles = std::max<uint64_t>(nt, 1);
  // (lists: a window that keeps tiles across its inserts does not start its list arena over at each of them: twice the room)
  return { count, std::max<uint64_t>(count, 1), nt, tiles, (want_resumable ? 8 : 4) * nt + 4096, want_resumable ? tiles : 0 };
}

static int
stream_begin_impl(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, uint32_t slot, uint32_t stripe_reads, uint32_t n_owners, uint32_t owner, const grp_read_decision** decisions, bool want_resumable)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads || !dp || slot > 1 || !decisions || n_owners == 0 || owner >= n_owners ||
      (n_owners > 1 && stripe_reads == 0)) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_stream_begin: bad argument");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_begin before grp_finalize");
  }
  if (!c->coherent_arch) {
    // the hand-over between workgroups inside the launch relies on agent-scope accesses being
    // served by the memory side, in issue order (gfx942 / gfx950); not a portable guarantee
    return set_err(c, GRP_ERR_INVALID, "grp_classify_stream_begin: streaming windows are only enabled on gfx942 / gfx950 (this device is %s)", c->arch.c_str());
  }
  QuerySlot& sl = c->slot[slot];
  if (sl.busy) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_begin: slot %u still has a window in flight", slot);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t t0 = r->tile0[first];
  const uint64_t nt = r->tile0[first + count] - t0;
  if (nt > (1u << 30)) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_stream_begin: %llu tiles in one call (limit 2^30)", (unsigned long long)nt);
  }
  const StreamNeeds need = stream_needs(count, nt, want_resumable);
  {
    // Growing a buffer frees the old one, and hipFree / hipHostFree wait for the device.  A
    // resumable window in the other slot may be parked, waiting for THIS thread's answer — the
    // wait would never end (found on C2: a window with a record number of tiles, begun while
    // the current one still had an insert to take; the launch gave up after its idle limit).
    // Not now, then: the caller begins this window once the other one has ended.
    const QuerySlot& other = c->slot[slot ^ 1u];
    if (need.exceed(sl) && other.busy && other.win.streaming && other.win.resumable) {
      return set_err(c, GRP_ERR_BUSY, "grp_classify_stream_begin: the slot's buffers must grow while a resumable window is in flight in the other slot: begin this window when that one has ended");
    }
  }
  c->q = &sl;
  if (need.sdec > sl.win.h_sdec.cap) {
    HIP_TRY(c, sl.win.h_sdec.reset(std::max<uint64_t>(need.sdec + need.sdec / 2, 1024), hipHostMallocMapped | hipHostMallocCoherent));
  }
  int rc = ensure_dev(c, sl.win.d_tiles_done, need.tiles_done);
  if (rc != GRP_OK) {
    return rc;
  }
  if (rc = slot_dec_scratch(c, sl, need.dec_tiles); rc != GRP_OK) {
    return rc;
  }
  sl.list_cap = std::max<uint64_t>(sl.d_lists.cap, need.lists);
  rc = slot_query_bufs(c, sl, need.tiles, sl.list_cap);
  if (rc == GRP_OK && want_resumable) { // (round 6) what a window keeps across an in-launch insert: a mark per tile (DevStreamCtl::tile_ver)
    rc = ensure_dev(c, sl.win.d_tile_ver, need.tile_ver);
  }
  if (rc != GRP_OK) {
    return rc;
  }
  // striped window (several ranks share it): this launch draws only the owner's tiles (host/gr_stream_stripes.hpp)
  gr::stripes::Window stripes;
  stripes.tile0 = r->tile0.data();
  stripes.first = first;
  stripes.count = count;
  stripes.stripe_reads = stripe_reads;
  stripes.n_owners = n_owners;
  stripes.owner = owner;
  const bool striped = stripes.striped();
  // n_decidable: of THIS launch — a striped window completes when its own stripes' reads are decided
  const gr::stripes::Totals tot = gr::stripes::totals(stripes);
  const uint64_t n_mine = tot.n_mine;
  if (striped) {
    if (n_mine > sl.win.d_stripe_tiles.cap) {
      clear_all(sl.win.h_stripe_tiles, sl.win.d_stripe_tiles);
      const uint64_t cap = n_mine + n_mine / 4 + 1024;
      HIP_TRY(c, sl.win.h_stripe_tiles.reset(cap, hipHostMallocDefault));
      HIP_TRY(c, sl.win.d_stripe_tiles.reset(cap));
    }
    gr::stripes::tile_list(stripes, sl.win.h_stripe_tiles);
  }
  // reads without a single tile are never completed by a workgroup: decided here
  memset(sl.win.h_sdec, 0, (size_t)count * sizeof(grp_read_decision));
  for (uint32_t j = 0; j < count; ++j) {
    if (stripes.tiles_of(j) == 0) {
      grp_read_decision d{};
      gr::core::decide(dp->threshold, dp->unassigned_min, dp->assigned_max, 0, nullptr, nullptr, nullptr, nullptr, nullptr, d);
      d.pad = 1;
      sl.win.h_sdec[j] = d;
    }
  }
  // A resumable window (grp_classify_stream_begin_resumable) does not end where it parks: it
  // waits for the host's word — _abort, or _insert: the insert the host has committed, applied
  // inside the launch.  Not when the scratch table would have to grow while the other slot's
  // window holds its address (the window is then an ordinary one; _insert says so).
  const bool resume_off = c->sw.stream_resume_off; // GRP_STREAM_RESUME=off (developer switch / tests): every window ends where it parks
  sl.win.resumable = false;
  if (want_resumable && !resume_off && n_mine != 0) {
    const uint64_t need_ranks = tot.max_tiles_read * tile_frames(c) * c->params.h;
    const bool other_streaming = c->slot[slot ^ 1u].busy && c->slot[slot ^ 1u].win.streaming;
    if (next_pow2_64(need_ranks * 2) <= c->ir_cap || !other_streaming) {
      rc = ensure_insert_table(c, need_ranks);
      if (rc != GRP_OK) {
        return rc;
      }
      sl.win.resumable = true;
    }
  }
  sl.win.gen = 1;
  sl.win.cmd_seq = 0;
  sl.win.stripes = stripes;
  __atomic_store_n(sl.win.h_abort.p, 0u, __ATOMIC_RELEASE);
  sl.reads = r;
  sl.first = first;
  sl.count = count;
  sl.dp = *dp;
  sl.nt = nt;
  sl.t0 = t0;
  sl.busy = true;
  sl.win.streaming = true;
  *decisions = sl.win.h_sdec;
  if (sl.side_used) {
    HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.done, 0));
    sl.side_used = false;
  }
  if (n_mine) {
    if (striped) {
      HIP_TRY(c, hipMemcpyAsync(sl.win.d_stripe_tiles, sl.win.h_stripe_tiles, n_mine * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(sl.win.d_abort, 0, ABORT_BYTES, c->stream));
    HIP_TRY(c, hipMemsetAsync(sl.win.d_abort + ABORT_PARK, 0xFF, sizeof(uint32_t), c->stream)); // park: nothing stale yet
    HIP_TRY(c, hipMemsetAsync(sl.win.d_tiles_done, 0, (size_t)count * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(sl.win.d_executed, 0, EXE_WORDS * sizeof(unsigned long long), c->stream));
    if (sl.win.resumable) {
      HIP_TRY(c, hipMemsetAsync(sl.win.d_sctl, 0, SCT_WORDS * sizeof(uint32_t), c->stream));
      HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sl.win.d_sctl + SCT_GEN), 1, 1, c->stream));
      HIP_TRY(c, hipMemsetAsync(sl.win.d_tile_ver, 0, std::max<uint64_t>(nt, 1) * sizeof(uint32_t), c->stream));
      HIP_TRY(c, hipMemsetAsync(sl.win.d_rel, 0, (size_t)STREAM_REL_WGS * 32u * sizeof(uint32_t), c->stream));
      // the changed-slot sets of the window's inserts start empty (the sets of the window before may hold its last two)
      HIP_TRY(c, hipMemsetAsync(c->d_fp_tab[0], 0, c->ir_cap * sizeof(uint32_t), c->stream));
      HIP_TRY(c, hipMemsetAsync(c->d_fp_tab[1], 0, c->ir_cap * sizeof(uint32_t), c->stream));
      __atomic_store_n(&sl.win.h_cmd[CMD_SEQ], 0u, __ATOMIC_RELEASE);
      sl.win.h_ack[ACK_APPLIED] = 0;
      sl.win.h_ack[ACK_CODE] = ACK_CODE_NONE;
    }
    DevStreamCtl sc;
    sc.first = first;
    sc.tiles_done = sl.win.d_tiles_done;
    sc.abort = sl.win.d_abort;
    sc.abort_host = sl.win.h_abort.dev;
    sc.next_tile = sl.win.d_abort + ABORT_NEXT_TILE;
    sc.park = sl.win.d_abort + ABORT_PARK;
    sc.early_park = c->sw.no_early_park ? 0u : 1u; // GRP_NO_EARLY_PARK, developer hook (the engine-level API contract assumes 1)
    sc.n_tiles = (uint32_t)n_mine;
    sc.dec = sl.win.h_sdec.dev;
    sc.executed = sl.win.d_executed;
    sc.dp = *dp;
    sc.g_ids = sl.d_dec_ids;
    sc.g_asg = sl.d_dec_asg;
    sc.g_scratch = sl.d_dec_scratch;
    sc.n_reads = count;
    sc.n_decidable = tot.n_decidable;
    if (sl.win.resumable) {
      sc.ctl = sl.win.d_sctl;
      sc.cmd_while_busy = striped ? 1u : 0u;
      sc.cmd_host = sl.win.h_cmd.dev;
      sc.ack_host = sl.win.h_ack.dev;
      sc.tb = InsertTable{ c->d_ir_keys, c->d_ir_masks, c->d_ir_locs, c->d_ir_slots, c->d_ir_counter, c->ir_cap - 1 };
      if (c->sw.stream_debug) { // GRP_STREAM_DEBUG
        if (!sl.win.d_dbg) {
          HIP_TRY(c, sl.win.d_dbg.reset(8192));
        }
        HIP_TRY(c, hipMemsetAsync(sl.win.d_dbg, 0, 8192 * sizeof(uint32_t), c->stream));
        sc.dbg = sl.win.d_dbg;
      }
      sc.rel = sl.win.d_rel;
      sc.tile_ver = sl.win.d_tile_ver;
      sc.fp_tab[0] = c->d_fp_tab[0];
      sc.fp_tab[1] = c->d_fp_tab[1];
      sc.fp_mask = (uint32_t)(c->ir_cap - 1);
      sc.n_fp = 2; // asked for; launch_query gives what this geometry's LDS has room for beside three workgroups per CU (0: nothing is kept)
      sc.timeout_ticks = (unsigned long long)(c->sw.stream_wait_s * 1e8); // GRP_STREAM_WAIT_S, developer hook: time limit of a grid-wide wait; wall_clock64 counts at 100 MHz
    }
    QueryLaunch ql{ n_mine, t0, query_geom(c, false), sl.list_cap };
    ql.d_tile_idx = striped ? sl.win.d_stripe_tiles.p : nullptr;
    ql.stream_ctl = &sc;
    {
      Timer t(c, GRP_K_QUERY, 0); // the probes actually executed are added at _end
      int lrc = launch_query(c, r, ql);
      if (lrc == GRP_ERR_BUSY && sl.win.resumable) {
        // the runtime cannot keep every workgroup of the window resident (the device is shared): the window is
        // begun in its classic form — it ends where it parks, grp_classify_stream_insert says GRP_ERR_STATE
        sl.win.resumable = false;
        sc.ctl = nullptr;
        ++c->n_stream_coop_refused;
        lrc = launch_query(c, r, ql);
      }
      if (lrc != GRP_OK) {
        sl.busy = false;
        sl.win.streaming = false;
        return lrc;
      }
      HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(sl.win.h_executed, sl.win.d_executed, EXE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(sl.d_qctr, 0, QCTR_WORDS * sizeof(uint64_t), c->stream));
  } else {
    memset(sl.win.h_executed, 0, EXE_WORDS * sizeof(unsigned long long));
  }
  HIP_TRY(c, hipEventRecord(sl.done, c->stream));
  return GRP_OK;
}

int
grp_classify_stream_abort(grp_ctx* c, uint32_t slot)
{
  if (!c || slot > 1 || !c->slot[slot].busy || !c->slot[slot].win.streaming) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_abort: no streaming window in this slot");
  }
  __atomic_store_n(c->slot[slot].win.h_abort.p, 1u, __ATOMIC_RELEASE);
  return GRP_OK;
}

int
grp_classify_stream_poll(grp_ctx* c, uint32_t slot)
{
  if (!c || slot > 1 || !c->slot[slot].busy || !c->slot[slot].win.streaming) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_poll: no streaming window in this slot");
  }
  hipError_t e = hipEventQuery(c->slot[slot].done);
  if (e == hipSuccess) {
    return 1;
  }
  if (e == hipErrorNotReady) {
    return 0;
  }
  return set_err(c, GRP_ERR_HIP, "grp_classify_stream_poll: %s", hipGetErrorString(e));
}

// developer (GRP_STREAM_DEBUG): where every workgroup of the launch was when a grid-wide wait of it timed out
static void
stream_dump_workgroups(const grp_ctx* c, const QuerySlot& sl, uint32_t code)
{
  const uint32_t who = sl.win.h_ack[ACK_GAVE_UP_WHO], arrived = sl.win.h_ack[ACK_GAVE_UP_COUNT];
  std::vector<uint32_t> st(8192);
  if (hipMemcpy(st.data(), sl.win.d_dbg, st.size() * 4, hipMemcpyDeviceToHost) == hipSuccess) {
    std::string line;
    for (size_t i = 0; i < st.size(); ++i) {
      if (i < 1024 && st[i] != 0 && ((st[i] >> 28) != 5u || (st[i] & 0xFFFFu) != ((sl.win.cmd_seq << 1) & 0xFFFFu))) {
        char b[64];
        snprintf(b, sizeof(b), " %zu:%08x", i, st[i]);
        line += b;
      }
    }
    {
      // when the workgroups came to the event and reached the first wait (100 MHz ticks, relative to the earliest)
      const uint32_t grid = std::min<uint32_t>(st[4095], 1000u);
      uint32_t t_min = 0xFFFFFFFFu;
      for (uint32_t i = 0; i < grid; ++i) {
        t_min = std::min(t_min, st[2048 + i]);
      }
      std::vector<std::pair<uint32_t, uint32_t>> late;
      for (uint32_t i = 0; i < grid; ++i) {
        late.push_back({ st[2048 + i] - t_min, i });
      }
      std::sort(late.begin(), late.end());
      char b[200];
      snprintf(b, sizeof(b), " | grid %u; reached the first wait (us behind the earliest): median %.1f", st[4095], late[grid / 2].first * 1e-2);
      line += b;
      for (uint32_t q = grid >= 6 ? grid - 6 : 0; q < grid; ++q) {
        const uint32_t w = late[q].second;
        snprintf(b, sizeof(b), "; wg %u %.1f us (came to the event %.1f us earlier; began %.1f us before that; xcc %u se %u cu %u)", w, late[q].first * 1e-2, (st[2048 + w] - st[1024 + w]) * 1e-2,
                 (st[1024 + w] - st[4096 + w]) * 1e-2, st[5120 + w] >> 16, (st[5120 + w] >> 13) & 7u, (st[5120 + w] >> 8) & 15u);
        line += b;
      }
      uint32_t t_start = 0xFFFFFFFFu, t_last = 0;
      for (uint32_t i = 0; i < grid; ++i) {
        t_start = std::min(t_start, st[4096 + i]);
      }
      uint32_t n_late = 0;
      for (uint32_t i = 0; i < grid; ++i) {
        t_last = std::max(t_last, st[4096 + i] - t_start);
        n_late += (st[4096 + i] - t_start) > 100000u ? 1u : 0u; // more than a millisecond behind the first
      }
      snprintf(b, sizeof(b), " | the last workgroup began %.1f us behind the first, %u of them more than 1 ms behind", t_last * 1e-2, n_late);
      line += b;
    }
    fprintf(stderr, "  last streaming launch: %u workgroups, %u bytes of LDS each\n", c->dbg_stream_grid, c->dbg_stream_lds);
    const uint32_t* cmd = sl.win.h_cmd + CMD_FIELDS;
    fprintf(stderr, "  window: reads [%u, %u), %llu tiles; command: read %u tiles [%u, %u) block %u first id %u offset %u resume read %u tile %u decided base %u gen %u\n", sl.first, sl.first + sl.count, (unsigned long long)sl.nt,
            cmd[CMD_READ], cmd[CMD_TILE_START], cmd[CMD_TILE_END], cmd[CMD_BLOCK_TILES], cmd[CMD_FIRST_ID], cmd[CMD_ID_OFFSET], cmd[CMD_RESUME_READ], cmd[CMD_RESUME_TILE], cmd[CMD_DECIDED_BASE], cmd[CMD_GEN]);
    fprintf(stderr, "grp_classify_stream_end: code %u, first to give up: wait %u, workgroup %u, %u of the insert's %u workgroups had arrived; workgroups not inside insert %u (index:state):%s\n", code, who & 0xFFFFu, who >> 16, arrived & 0xFFFFu, arrived >> 16, sl.win.cmd_seq, line.c_str());
  }
}

int
grp_classify_stream_end(grp_ctx* c, uint32_t slot, uint32_t* reads_decided)
{
  if (!c || slot > 1 || !c->slot[slot].busy || !c->slot[slot].win.streaming) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_end: no streaming window in this slot");
  }
  QuerySlot& sl = c->slot[slot];
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipEventSynchronize(sl.done));
  sl.busy = false;
  sl.win.streaming = false;
  c->kstat[GRP_K_QUERY].units += sl.win.h_executed[EXE_PROBES];
  for (uint32_t i = EXE_PROBES + 1; i < EXE_WORDS; ++i) { // what the window's in-launch inserts kept and redid (grp_debug_stream_stats)
    c->n_stream_keep[i] += sl.win.h_executed[i];
  }
  if (reads_decided) {
    uint32_t n = 0;
    for (uint32_t j = 0; j < sl.count; ++j) {
      n += sl.win.h_sdec[j].pad != 0;
    }
    *reads_decided = n;
  }
  if (c->pending.size() > 64) {
    drain_events(c);
  }
  if (sl.win.resumable) {
    sl.win.resumable = false;
    const uint32_t code = __atomic_load_n(&sl.win.h_ack[ACK_CODE], __ATOMIC_ACQUIRE);
    const uint32_t applied = __atomic_load_n(&sl.win.h_ack[ACK_APPLIED], __ATOMIC_ACQUIRE);
    const uint32_t who = sl.win.h_ack[ACK_GAVE_UP_WHO], arrived = sl.win.h_ack[ACK_GAVE_UP_COUNT]; // (for the messages: wait [15:0] workgroup [31:16]; arrived [15:0] of [31:16])
    if ((code == ACK_CODE_WAIT_TIMEOUT || code == ACK_CODE_NOT_APPLIED) && sl.win.d_dbg) {
      stream_dump_workgroups(c, sl, code);
    }
    if (code == ACK_CODE_WAIT_TIMEOUT) {
      return set_err(c, GRP_ERR_STATE, "grp_classify_stream_end: a grid-wide wait timed out in the middle of an insert (the ID array may be inconsistent); first to give up: wait %u, workgroup %u, %u of the insert's %u workgroups had arrived",
                     who & 0xFFFFu, who >> 16, arrived & 0xFFFFu, arrived >> 16);
    }
    if (code == ACK_CODE_IDLE_EXIT) {
      // The parked window was told nothing for its idle limit (16 x GRP_STREAM_WAIT_S: a host stopped by a
      // debugger or SIGSTOP, a stalled file system) and left by itself.  It had modified nothing: not an error
      // (ADVICE r03) — the records it did not produce stay open and the caller begins the window again behind
      // the last one it has; what the launch was waiting on is kept as the context's last message.
      uint32_t first_open = sl.count;
      for (uint32_t j = 0; j < sl.count; ++j) {
        if (sl.win.h_sdec[j].pad != sl.win.gen) {
          first_open = j;
          break;
        }
      }
      ++c->n_stream_idle_exits;
      (void)set_err(c, GRP_OK,
                    "grp_classify_stream_end: the parked window was never told how to go on (idle time limit) and left; launch: park %u decided %u next tile %u / %llu event %u command seen %u "
                    "generation %u; host: %u reads, generation %u, commands posted %u applied %u, first open record %u",
                    sl.win.h_ack[ACK_IDLE_PARK], sl.win.h_ack[ACK_IDLE_DECIDED], sl.win.h_ack[ACK_IDLE_NEXT_TILE], (unsigned long long)sl.nt, sl.win.h_ack[ACK_IDLE_EVENT], sl.win.h_ack[ACK_IDLE_CMD_SEQ], sl.win.h_ack[ACK_IDLE_GEN],
                    sl.count, sl.win.gen, sl.win.cmd_seq, applied, first_open);
      if (c->sw.trace_abort) {
        fprintf(stderr, "%s\n", c->err.c_str());
      }
    }
    if (applied != sl.win.cmd_seq) {
      // The launch ended without the insert posted last (an abort overtook it or the launch had left already: 1; the
      // first grid-wide wait timed out, the device is shared: 2).  Only the scratch table may have been
      // touched; the caller applies the insert with grp_insert_read.
      HIP_TRY(c, hipMemsetAsync(c->d_ir_keys, 0, c->ir_cap * 8, c->stream));
      HIP_TRY(c, hipMemsetAsync(c->d_ir_masks, 0, c->ir_cap * 8, c->stream));
      return stream_end_unapplied(code);
    }
  }
  return GRP_OK;
}

int
grp_classify_stream_insert(grp_ctx* c, uint32_t slot, uint32_t read_idx, uint32_t tile_start, uint32_t tile_end, uint32_t block_tiles, uint32_t first_id, uint32_t id_offset, uint32_t* generation)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || slot > 1 || !c->slot[slot].busy || !c->slot[slot].win.streaming || block_tiles == 0 || id_offset > 1 || !generation) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_insert: no streaming window in this slot / bad argument");
  }
  QuerySlot& sl = c->slot[slot];
  const grp_reads* r = sl.reads;
  if (!sl.win.resumable) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_insert: this window ends where it parks (not begun with grp_classify_stream_begin_resumable, or GRP_STREAM_RESUME=off)");
  }
  if (read_idx < sl.first || read_idx >= sl.first + sl.count) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_stream_insert: read %u is not in the window", read_idx);
  }
  const uint64_t ntile = r->tile0[read_idx + 1] - r->tile0[read_idx];
  if (tile_start >= tile_end || tile_end > ntile) {
    return set_err(c, GRP_ERR_INVALID, "grp_classify_stream_insert: tiles [%u,%u) outside the read's %llu tiles", tile_start, tile_end, (unsigned long long)ntile);
  }
  if ((tile_end - tile_start + block_tiles - 1) / block_tiles > 64) {
    return set_err(c, GRP_ERR_STATE, "grp_classify_stream_insert: more than 64 ID blocks (the caller ends the window and uses grp_insert_read)");
  }
  if (sl.win.cmd_seq != 0 && c->sw.trace_abort) { // GRP_TRACE_ABORT, developer trace: phase times of the previous in-launch insert (100 MHz ticks)
    static double t_ph[ACK_PHASES] = { 0, 0, 0, 0 };
    static uint64_t n_tr = 0;
    const uint32_t* ph = sl.win.h_ack + ACK_PHASE;
    for (uint32_t i = 0; i < ACK_PHASES; ++i) {
      t_ph[i] += ph[i] * 1e-2;
    }
    if (c->sw.trace_abort == 2) {
      fprintf(stderr, "  previous in-launch insert, workgroup 0: collect %.1f us, first wait %.1f us, apply %.1f us, second wait %.1f us\n", ph[0] * 1e-2, ph[1] * 1e-2, ph[2] * 1e-2, ph[3] * 1e-2);
    }
    if ((++n_tr & 511u) == 0) {
      fprintf(stderr, "in-launch inserts %llu: workgroup 0 spent %.1f us collecting, %.1f us in the first wait, %.1f us applying, %.1f us in the second wait\n", (unsigned long long)n_tr, t_ph[0] / n_tr,
              t_ph[1] / n_tr, t_ph[2] / n_tr, t_ph[3] / n_tr);
    }
  }
  // (records of the new generation can overtake the launch's acknowledgement of the insert in front of them by a moment)
  for (uint32_t spins = 0; __atomic_load_n(&sl.win.h_ack[ACK_APPLIED], __ATOMIC_ACQUIRE) != sl.win.cmd_seq; ++spins) {
    if (spins > (1u << 26) || __atomic_load_n(&sl.win.h_ack[ACK_CODE], __ATOMIC_ACQUIRE) != ACK_CODE_NONE) {
      return set_err(c, GRP_ERR_STATE, "grp_classify_stream_insert: the previous insert of this window has not been applied");
    }
    __builtin_ia32_pause();
  }
  const uint32_t x = read_idx - sl.first;
  // this launch's decidable reads up to the insert, and its tiles up to there (= where its dispenser starts over)
  const gr::stripes::Resume at = gr::stripes::resume_at(sl.win.stripes, x);
  const uint32_t gen = ++sl.win.gen;
  for (uint32_t j = x + 1; j < sl.count; ++j) { // the host's own records (reads without tiles) move to the new generation
    if (sl.win.stripes.tiles_of(j) == 0) {
      __atomic_store_n(&sl.win.h_sdec[j].pad, gen, __ATOMIC_RELEASE);
    }
  }
  uint32_t* cmd = sl.win.h_cmd + CMD_FIELDS;
  cmd[CMD_READ] = read_idx;
  cmd[CMD_TILE_START] = tile_start;
  cmd[CMD_TILE_END] = tile_end;
  cmd[CMD_BLOCK_TILES] = block_tiles;
  cmd[CMD_FIRST_ID] = first_id;
  cmd[CMD_ID_OFFSET] = id_offset;
  cmd[CMD_RESUME_READ] = x + 1;
  cmd[CMD_RESUME_TILE] = (uint32_t)at.resume_tile;
  cmd[CMD_DECIDED_BASE] = at.decided_base;
  cmd[CMD_GEN] = gen;
  __atomic_store_n(&sl.win.h_cmd[CMD_SEQ], ++sl.win.cmd_seq, __ATOMIC_RELEASE);
  c->kstat[GRP_K_INSERT].launches += 1;
  c->kstat[GRP_K_INSERT].units += (uint64_t)(tile_end - tile_start) * tile_frames(c) * c->params.h;
  *generation = gen;
  return GRP_OK;
}

} // extern "C"
