// The second decisions of a batch WITHOUT a second query of the tiles the batch inserted
// (grp_batch_verify, include/grpath.h; round 4).
//
// grp_batch_classify asks the filter again for every probe of the window (k_query<.., VER>): 75 k
// random bucket lines per read to find the ~100 probes whose rank an earlier read of the batch wrote.
// But the collect pass of grp_batch_insert_reads has already visited every probe of every INSERTED
// tile and knows which of their ranks have a second toucher in the batch: the rank's record carries a
// chain (k_batch_collect).  A probe whose rank has ONE toucher — the probe's own (read, ID block) — reads
// in front of its read's insert exactly what the first query read in front of the batch.  So, per
// inserted tile, k_batch_delta
//   1. streams over the tile's records (12 bytes per probe, coalesced) and keeps the frames with a
//      probe on a multi-touch rank (a few per tile);
//   2. evaluates those frames twice through the batch's log — the IDs the frame held in front of the
//      batch, and the IDs it holds in front of its own read's insert (batch_view, the same function the
//      second query uses) — and tabulates what the frame's ID SET lost and gained, and its hits / misses;
//   3. patches the first query's tile summary with that: the count of every ID of the tile's count > 2
//      list and of its top ID is known, an ID the batch allocated had count 0, every other ID had a
//      count <= 2 that can only have gone down — so the new list is exact, and the new top ID is exact
//      unless the old top lost frames and nothing with more than two frames is left (then an ID whose
//      count is not known could lead): such a tile, and a tile whose dirty frames touch more than
//      VF_DCAP IDs, is FLAGGED and queried again through the log like any flagged tile.
// Tiles the batch did not insert (reads that do not insert, the rest of a trimmed read) have no records:
// they go through k_query<.., VER> as before, in the same call (the kernel leaves the tiles with records at
// once), and the reads behind the batch through the plain query.  The decisions are those of grp_batch_classify bit for bit
// (tests/test_gpu_batch.py runs both on every batch).
// Included by grpath_hip.hip behind grp_batch.inc (same translation unit).

namespace {

constexpr uint32_t VF_DCAP = 256; // slots of a tile's delta table (IDs its dirty frames lose or gain)
// (Measured and removed in round 4: the tiles WITHOUT records patched the same way, their dirty frames found by
// hashing the tile and looking every probe's bucket up in a 2 MiB bitmap of the buckets the batch touched — small
// enough for the L2, 241 G look-ups/s.  A frame has h probes, so with a fraction f of the bits set 1 - (1 - f)^h of
// the clean frames are looked at for nothing: the bitmap only pays below ~1 M records per batch, where the batches
// are about to hand over to the streaming windows anyway; at the batch sizes of the head it cost what the second
// query of those tiles costs.  profiles/r04_bitmap_mode_measured.txt)

struct DevVerify
{
  const grp_tile_summary* t0_tiles = nullptr; // the first decisions' tile summaries: tile i of the window at t0_off + i ...
  const grp_id_count* t0_lists = nullptr;     // ... and their count > 2 lists
  uint64_t t0_lists_cap = 0;
  uint64_t t0_off = 0;
  const uint32_t* read_ins = nullptr; // [reads of the window]: the read's entry in the batch's insert list, BATCH_NONE: none
  uint32_t n_reads = 0;               // reads of the window with an entry in read_ins (the batch's reads)
};

// `d` more (fewer) frames of the tile hold `id`; false: the table is full
__device__ inline bool
delta_add(uint32_t* keys, int* vals, uint32_t id, int d)
{
  uint32_t slot = (id * 2654435761u) & (VF_DCAP - 1u);
  for (uint32_t probe = 0; probe < VF_DCAP / 2u; ++probe) {
    const uint32_t old = atomicCAS(&keys[slot], 0u, id);
    if (old == 0u || old == id) {
      atomicAdd(&vals[slot], d);
      return true;
    }
    slot = (slot + 1u) & (VF_DCAP - 1u);
  }
  return false;
}

// slot of `id` in the delta table, VF_DCAP: not there
__device__ inline uint32_t
delta_find(const uint32_t* keys, uint32_t id)
{
  uint32_t slot = (id * 2654435761u) & (VF_DCAP - 1u);
  for (uint32_t probe = 0; probe < VF_DCAP / 2u; ++probe) {
    const uint32_t k = keys[slot];
    if (k == id) {
      return slot;
    }
    if (k == 0u) {
      return VF_DCAP;
    }
    slot = (slot + 1u) & (VF_DCAP - 1u);
  }
  return VF_DCAP;
}

// one frame with a probe on a multi-touch rank: its ID set in front of the batch and in front of read
// `reader`'s insert (calc_num_assigned_tiles :571-604 on both states), the difference into the delta table
template<int H, int WT>
__device__ inline bool
verify_frame(const DevFilter& f, const DevSeeds* __restrict__ sd, const ulonglong2* sTab, const uint32_t* sBases, uint32_t boff, uint32_t fr, uint32_t Lp, const DevBatchView& bv, uint32_t reader, uint32_t fl0,
             uint32_t flj, uint32_t* dKeys, int* dVals, int& dh, int& dm)
{
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t cur[H];
  uint64_t rank[H], bl[H];
  bool all = true;
#pragma unroll
  for (int s = 0; s < H; ++s) {
    if (!seed_on<H>(s, hn)) { // (the many-seed form: no probe; its IDs below are 0, which nothing counts)
      cur[s] = 0u;
      rank[s] = bl[s] = 0;
      continue;
    }
    // a seed that can no longer roll keeps its last value (multiLensfrHashIterator.hpp:49-68)
    const uint32_t fs = min(fr, Lp - sd->span[s]);
    const Probe pr = grp_locate(f, seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs)));
    const uint4 hd = f.buckets[pr.b * GRP_UNIT_U4];
    const uint64_t bm = grp_bitmap(hd);
    const uint32_t lr = grp_local_rank(bm, pr.off);
    all = all && ((bm >> pr.off) & 1ull); // atRank (MIBloomFilter.hpp:465-476): all or nothing
    rank[s] = f.super[pr.b >> GRP_SUPER_SHIFT] + hd.x + lr;
    bl[s] = pr.b * 64ull + lr;
    cur[s] = 0u;
    if ((bm >> pr.off) & 1ull) {
      cur[s] = (lr < GRP_BUCKET_IDS) ? reinterpret_cast<const uint32_t*>(f.buckets)[grp_id_loc(pr.b, lr)] : grp_ovf_get(f, rank[s]);
    }
  }
  if (!all) {
    return true; // (a frame with a clear bit counts nothing, in either state)
  }
  const uint32_t id0 = fl0 & 0x7FFFFFFFu, idj = flj & 0x7FFFFFFFu;
  uint32_t a[H], z[H]; // the frame's IDs in front of the batch / in front of the reader's insert, saturation bit stripped (:573-594)
#pragma unroll
  for (int s = 0; s < H; ++s) {
    if (!seed_on<H>(s, hn)) {
      a[s] = z[s] = 0u;
      continue;
    }
    const uint32_t c = cur[s], ci = c & 0x7FFFFFFFu;
    const uint32_t v0 = (ci >= id0) ? batch_view(bv, rank[s], bl[s], 0u, c, (fl0 >> 31) != 0u && ci == id0) : c;
    const uint32_t vj = (ci >= idj) ? batch_view(bv, rank[s], bl[s], reader, c, (flj >> 31) != 0u && ci == idj) : c;
    a[s] = (v0 > 0x80000000u) ? (v0 & 0x7FFFFFFFu) : v0;
    z[s] = (vj > 0x80000000u) ? (vj & 0x7FFFFFFFu) : vj;
    dh += (z[s] != 0u ? 1 : 0) - (a[s] != 0u ? 1 : 0);
    dm += (z[s] == 0u ? 1 : 0) - (a[s] == 0u ? 1 : 0);
  }
  bool ok = true;
#pragma unroll
  for (int s = 0; s < H; ++s) {
    bool dup_a = false, dup_z = false, in_z = false, in_a = false;
#pragma unroll
    for (int u = 0; u < H; ++u) {
      dup_a = dup_a || (u < s && a[u] == a[s]);
      dup_z = dup_z || (u < s && z[u] == z[s]);
      in_z = in_z || z[u] == a[s];
      in_a = in_a || a[u] == z[s];
    }
    if (a[s] != 0u && !dup_a && !in_z) {
      ok = delta_add(dKeys, dVals, a[s], -1) && ok; // the frame no longer holds this ID
    }
    if (z[s] != 0u && !dup_z && !in_a) {
      ok = delta_add(dKeys, dVals, z[s], 1) && ok; // the frame holds this ID now
    }
  }
  return ok;
}

template<int H, int WT>
__global__ void __launch_bounds__(THREADS)
k_batch_delta(DevFilter f, DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint64_t tile_begin, DevBatch b, DevBatchView bv, DevVerify vf,
              grp_tile_summary* __restrict__ tiles_out, grp_id_count* __restrict__ lists_out, uint64_t lists_cap, unsigned long long* __restrict__ ctr, uint32_t* __restrict__ flagged_out, uint32_t flagged_cap)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);
  __shared__ uint32_t dKeys[VF_DCAP];
  __shared__ int dVals[VF_DCAP];
  __shared__ uint32_t dSeen[VF_DCAP];
  __shared__ int sDH, sDM, sDTop;
  __shared__ uint32_t sBad, sOutN, sListOff, sDirty;
  __shared__ uint32_t sBest[2 * (THREADS / 64)];

  const uint32_t out_idx = blockIdx.x; // every tile of the batch's reads
  const uint64_t t = tile_begin + out_idx;
  const uint32_t r = rd.tile_read[t];
  const uint32_t ti = (uint32_t)(t - rd.tile0[r]);
  const uint32_t reader = r - bv.first;
  const uint32_t parts = gr::geom::tile_parts(frames_per_tile(sd, tile_len));
  // only the tiles this batch inserted have records; the others are k_query<.., VER>'s
  uint32_t unit0 = 0;
  {
    const uint32_t ji = vf.read_ins[reader];
    if (ji == BATCH_NONE) {
      return;
    }
    const uint32_t* e = b.ins + (size_t)ji * 6;
    if (ti < e[1] || ti >= e[2]) {
      return;
    }
    unit0 = e[5] + (ti - e[1]) * parts;
  }
  const uint32_t len = rd.len[r];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, ti);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;

  for (uint32_t i = threadIdx.x; i < VF_DCAP; i += THREADS) {
    dKeys[i] = 0u;
    dVals[i] = 0;
    dSeen[i] = 0u;
  }
  if (threadIdx.x == 0) {
    sDH = sDM = sDTop = 0;
    sBad = sOutN = sDirty = sListOff = 0u;
  }
  __syncthreads();
  // 1) the tile's records: the frames with a probe on a rank with a second toucher
  uint32_t dirty = 0; // bit `part`: this lane's frame of that part
  for (uint32_t part = 0; part < parts; ++part) {
    bool d = false;
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (!seed_on<H>(s, hn)) {
        continue;
      }
      const uint32_t idx = ((unit0 + part) * hn + (uint32_t)s) * THREADS + threadIdx.x;
      const unsigned long long key = b.rec_key[idx];
      uint32_t owner = idx;
      bool touch = (key >> 26) != 0ull;
      if (!touch) {
        const uint32_t c = (uint32_t)(key & BATCH_LOW26);
        touch = c >= 2u; // a duplicate inside its (read, block) or a touch chained to another record: the owner knows
        owner = touch ? c - 2u : idx;
      }
      d = d || (touch && b.rec_chain[owner] != BATCH_NONE);
    }
    if (d && part * THREADS + threadIdx.x < frames) {
      if (part < 32u) {
        dirty |= 1u << part;
      } else {
        atomicOr(&sBad, 1u); // (tiles of more than 8192 frames: queried again instead)
      }
    }
  }
  if (__syncthreads_or(dirty != 0u)) {
    // 2) the dirty frames, in front of the batch and in front of this read's insert
    load_tab(sTab, sd);
    const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, start, Lp);
    __syncthreads();
    const uint32_t fl0 = bv.floor[0], flj = bv.floor[r - bv.floor_first];
    int dh = 0, dm = 0;
    bool ok = true;
    while (dirty) {
      const uint32_t part = (uint32_t)__ffs((int)dirty) - 1u;
      dirty &= dirty - 1u;
      ok = verify_frame<H, WT>(f, sd, sTab, sBases, boff, part * THREADS + threadIdx.x, Lp, bv, reader, fl0, flj, dKeys, dVals, dh, dm) && ok;
    }
    if (dh != 0) {
      atomicAdd(&sDH, dh);
    }
    if (dm != 0) {
      atomicAdd(&sDM, dm);
    }
    if (!ok) {
      atomicOr(&sBad, 1u);
    }
    if (threadIdx.x == 0) {
      sDirty = 1u;
    }
  }
  __syncthreads();

  // 3) the first query's summary, patched
  const grp_tile_summary T0 = vf.t0_tiles[vf.t0_off + out_idx];
  const uint32_t fl0 = bv.floor[0];
  const uint32_t id0 = fl0 & 0x7FFFFFFFu;
  bool bad = sBad != 0u || T0.list_n == GRP_TILE_FLAGGED || (uint64_t)T0.list_off + T0.list_n > vf.t0_lists_cap;
  if (!bad && threadIdx.x == 0) {
    uint32_t n_max = T0.list_n; // room for the old list and for every ID the dirty frames gained
    if (sDirty) {
      for (uint32_t i = 0; i < VF_DCAP; ++i) {
        n_max += dKeys[i] != 0u ? 1u : 0u;
      }
    }
    sListOff = n_max ? (uint32_t)atomicAdd(&ctr[QCTR_LIST_CURSOR], (unsigned long long)n_max) : 0u;
  }
  __syncthreads();
  uint32_t bc = 0, bid = 0;
  const uint64_t lo = sListOff;
  if (!bad) {
    for (uint32_t i = threadIdx.x; i < T0.list_n; i += THREADS) {
      const grp_id_count en = vf.t0_lists[T0.list_off + i];
      const uint32_t slot = delta_find(dKeys, en.id);
      int c = (int)en.count;
      if (slot != VF_DCAP) {
        c += dVals[slot];
        dSeen[slot] = 1u;
      }
      if (c > 2) {
        const uint32_t at = atomicAdd(&sOutN, 1u);
        if (lo + at < lists_cap) {
          lists_out[lo + at].id = en.id;
          lists_out[lo + at].count = (uint32_t)c;
        }
      }
      if (c > 0 && better((uint32_t)c, en.id, bc, bid)) { // its count is known whether it stays in the list or not
        bc = (uint32_t)c;
        bid = en.id;
      }
      if (c < 0) {
        atomicOr(&sBad, 2u); // cannot happen: counted fewer frames than the tile lost
      }
    }
  }
  __syncthreads();
  if (!bad) {
    for (uint32_t i = threadIdx.x; i < VF_DCAP; i += THREADS) {
      const uint32_t key = dKeys[i];
      const int d = dVals[i];
      if (key == 0u || dSeen[i] != 0u || d == 0) {
        continue;
      }
      if (key == T0.top_id && T0.top_count != 0u) {
        continue; // the old top outside the list: below
      }
      if (key >= id0) {
        // an ID this batch allocated: no frame held it in front of the batch — unless it is the ID the
        // last block of the trimmed read in front of the batch shares with the batch's first insert
        if (d < 0 || ((fl0 >> 31) != 0u && key == id0)) {
          atomicOr(&sBad, 1u);
          continue;
        }
        if (d > 2) {
          const uint32_t at = atomicAdd(&sOutN, 1u);
          if (lo + at < lists_cap) {
            lists_out[lo + at].id = key;
            lists_out[lo + at].count = (uint32_t)d;
          }
        }
        if (better((uint32_t)d, key, bc, bid)) {
          bc = (uint32_t)d;
          bid = key;
        }
      } else if (d > 0) {
        atomicOr(&sBad, 2u); // cannot happen: an older ID gained a frame
      }
      // (an older ID outside the list that is not the top: at most two frames held it, fewer now —
      // it can neither enter the list nor lead)
    }
  }
  if (!bad && threadIdx.x == 0 && T0.top_count != 0u) {
    const uint32_t slot = delta_find(dKeys, T0.top_id);
    const int d = slot != VF_DCAP ? dVals[slot] : 0;
    sDTop = d;
    if (T0.top_count <= 2u) { // not in the list: a candidate by itself
      const int c = (int)T0.top_count + d;
      if (c > 0 && better((uint32_t)c, T0.top_id, bc, bid)) {
        bc = (uint32_t)c;
        bid = T0.top_id;
      }
      if (c < 0) {
        atomicOr(&sBad, 2u);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t oc = __shfl_xor(bc, o, 64);
    const uint32_t oid = __shfl_xor(bid, o, 64);
    if (better(oc, oid, bc, bid)) {
      bc = oc;
      bid = oid;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sBest[2 * (threadIdx.x >> 6)] = bc;
    sBest[2 * (threadIdx.x >> 6) + 1] = bid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < THREADS / 64; ++w) {
      if (better(sBest[2 * w], sBest[2 * w + 1], bc, bid)) {
        bc = sBest[2 * w];
        bid = sBest[2 * w + 1];
      }
    }
    // the old top lost frames and nothing with more than two frames is left: an ID outside the list
    // (count <= 2, not known) may lead now — the tile is queried again
    bad = bad || sBad != 0u || (sDTop < 0 && bc <= 2u);
    grp_tile_summary ts;
    ts.top_id = bid;
    ts.top_count = bc;
    ts.list_off = (uint32_t)lo;
    ts.list_n = sOutN;
    ts.hits = (uint32_t)((int)T0.hits + sDH);
    ts.misses = (uint32_t)((int)T0.misses + sDM);
    if (bad) {
      ts.list_n = GRP_TILE_FLAGGED;
      const unsigned long long fi = atomicAdd(&ctr[QCTR_FLAGGED], 1ull);
      if (fi < flagged_cap) {
        flagged_out[fi] = out_idx;
      }
      if (sBad & 2u) {
        atomicAdd(&ctr[QCTR_IMPOSSIBLE], 1ull); // an impossible delta: reported by the host (the tile is still redone exactly)
      }
      // why the patch was given up (statistics): uncertified — the old top lost frames and no count > 2 is left; unpatched — anything
      // else (delta table full, the batch's first ID shared with the read in front, a first summary that was itself flagged)
      atomicAdd(&ctr[(sBad == 0u && !(T0.list_n == GRP_TILE_FLAGGED)) ? QCTR_UNCERTIFIED : QCTR_UNPATCHED], 1ull);
    }
    tiles_out[out_idx] = ts;
  }
}

constexpr uint32_t VERIFY_REDO_ON_DEVICE = 128; // workgroups of the redo launch that is enqueued before the list's length is known

} // namespace

extern "C" {

int
grp_batch_verify(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, uint32_t extra, const grp_decide_params* dp, const uint32_t* id_floor, grp_read_decision* out)
{
  if (!c || !r || r->ctx != c || !id_floor || !dp || !out || !c->batch.active || first != c->batch.first_read || (uint64_t)first + count + extra > r->n_reads || count == 0) {
    return set_err(c, GRP_ERR_STATE, "grp_batch_verify: no batch on this window");
  }
  BatchRun& br = c->batch;
  const grp_ctx::Carry cy = c->carry;
  const bool off = c->sw.batch_verify_off; // GRP_BATCH_VERIFY=off, developer switch / tests: always the second query
  if (off || !cy.valid || cy.reads != r || cy.first > first || (uint64_t)first + count > (uint64_t)cy.first + cy.count || c->slot[0].busy || c->slot[1].busy) {
    // the first decisions' summaries are gone (or never were this engine's): the window is queried again
    ++c->n_verify_fallbacks;
    return grp_batch_classify(c, r, first, count + extra, dp, id_floor, out);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t total = count + extra;
  const uint32_t out_slot = 1u - cy.slot;
  const QuerySlot& si = c->slot[cy.slot];
  const uint64_t t0 = r->tile0[first];
  const uint64_t nt_batch = r->tile0[first + count] - t0, nt_all = r->tile0[first + total] - t0;
  int rc = classify_setup(c, r, first, total, dp, out_slot);
  if (rc != GRP_OK) {
    c->slot[out_slot].busy = false;
    return rc;
  }
  QuerySlot& so = c->slot[out_slot];
  so.busy = false; // (synchronous call: the slot is never left in flight)
  so.t0 = t0;
  c->carry.valid = false;
  // Per read of the batch: its entry in the insert list (the kernels tell from it which tiles have records).  The
  // floors travel in the same page-locked block: one copy per call, nothing per tile on the host.
  const uint32_t h = c->params.h, ftile = tile_frames(c);
  if ((uint64_t)count + total > br.h_vf_stage.cap) {
    HIP_TRY(c, br.h_vf_stage.reset(2 * ((uint64_t)count + total) + 4096, hipHostMallocDefault));
  }
  rc = ensure_dev(c, br.d_vf_stage, (uint64_t)count + total);
  if (rc != GRP_OK) {
    return rc;
  }
  uint32_t* rins = br.h_vf_stage;
  uint64_t r_records = 0, recorded_tiles = 0;
  {
    uint32_t ji = 0;
    for (uint32_t j = 0; j < count; ++j) {
      const uint32_t rd_i = first + j;
      while (ji < br.n_ins && br.h_ins[(size_t)ji * 6] < rd_i) {
        ++ji;
      }
      rins[j] = BATCH_NONE;
      if (ji < br.n_ins && br.h_ins[(size_t)ji * 6] == rd_i) {
        rins[j] = ji;
        const uint32_t ts = br.h_ins[(size_t)ji * 6 + 1], te = br.h_ins[(size_t)ji * 6 + 2];
        const uint32_t ntile = (uint32_t)(r->tile0[rd_i + 1] - r->tile0[rd_i]);
        uint64_t fr = (uint64_t)(te - ts) * ftile; // only a read's last tile can be clipped
        if (te == ntile && ntile) {
          fr -= ftile - tile_extent(c, r->len[rd_i], ntile - 1).frames;
        }
        r_records += fr * h;
        recorded_tiles += te - ts;
      }
    }
  }
  memcpy(br.h_vf_stage + count, id_floor, (size_t)total * sizeof(uint32_t));
  HIP_TRY(c, hipMemcpyAsync(br.d_vf_stage, br.h_vf_stage, ((size_t)count + total) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  const uint32_t* d_read_ins = br.d_vf_stage;
  const uint32_t* d_floor = br.d_vf_stage + count;
  const uint64_t n_r = recorded_tiles, n_q = nt_batch - recorded_tiles;
  const uint64_t q_probes = count_probes(c, r, first, count) - r_records;
  DevBatchView bv = batch_view_of(c);
  bv.floor = d_floor;
  bv.floor_first = first;
  bv.first = br.first_read;
  const uint64_t x_probes = extra ? count_probes(c, r, first + count, extra) : 0;
  const size_t lds_delta = tab_bytes(c) + bases_bytes(c->params.tile + c->params.k + c->params.h);

  bool redo_on_device = false;
  auto enqueue = [&]() -> int {
    c->q = &so;
    redo_on_device = false;
    if (const int erc = slot_query_bufs(c, so, nt_all, std::max<uint64_t>(so.list_cap, 1)); erc != GRP_OK) {
      return erc;
    }
    if (so.side_used) {
      HIP_TRY(c, hipStreamWaitEvent(c->stream, so.done, 0));
      so.side_used = false;
    }
    if (n_r) {
      // a workgroup per tile of the batch's reads: the ones with records are patched, the others leave at once
      const DevBatch b = batch_dev(c);
      DevVerify vf;
      vf.t0_tiles = si.d_tiles;
      vf.t0_lists = si.d_lists;
      vf.t0_lists_cap = si.list_cap;
      vf.t0_off = cy.tile_off + (r->tile0[first] - r->tile0[cy.first]);
      vf.read_ins = d_read_ins;
      vf.n_reads = count;
      Timer t(c, GRP_K_VERIFY, r_records);
      DISPATCH_HW(c, (k_batch_delta<HH, WW><<<dim3((uint32_t)nt_batch), dim3(THREADS), lds_delta, c->stream>>>(c->f, r->dev, c->d_seeds, c->params.tile, t0, b, bv, vf, so.d_tiles, so.d_lists, so.list_cap,
                                                                                                             reinterpret_cast<unsigned long long*>(so.d_qctr.p), so.d_flag_idx, (uint32_t)so.d_flag_idx.cap)));
      HIP_TRY(c, hipGetLastError());
    }
    const QueryGeom g = query_geom(c, false);
    int lrc = GRP_OK;
    if (n_q) { // tiles without records: through the log, as grp_batch_classify (the tiles with records leave at once)
      Timer t(c, GRP_K_QUERY, q_probes);
      DevBatchView bq = bv;
      bq.skip_read_ins = d_read_ins;
      bq.skip_reads = count;
      c->view = &bq;
      lrc = launch_query(c, r, QueryLaunch{ nt_batch, t0, g, so.list_cap });
      c->view = nullptr;
      if (lrc != GRP_OK) {
        return lrc;
      }
      HIP_TRY(c, hipGetLastError());
    }
    if (extra) { // the reads behind the batch: the plain query (the next window's first decisions)
      Timer t(c, GRP_K_QUERY, x_probes);
      QueryLaunch ql{ nt_all - nt_batch, t0, g, so.list_cap };
      ql.blk0 = (uint32_t)nt_batch;
      ql.plain = true;
      lrc = launch_query(c, r, ql);
      if (lrc != GRP_OK) {
        return lrc;
      }
      HIP_TRY(c, hipGetLastError());
    }
    if (n_r || n_q) {
      // Tiles whose patch was given up (and tiles a small first-step table could not hold) are redone through the log by a
      // launch enqueued HERE, behind the patch: it reads the list's length on the device (workgroups beyond it leave at
      // once), so the window is decided once and the host is asked once.  Round 5: half of the batches of the
      // insert-heavy regime flag a tile or two, and each paid a second round trip — wait, redo, decide again, wait.
      // A list longer than the launch takes the old way below.
      Timer t(c, GRP_K_QUERY, 0);
      DevBatchView bf = bv;
      bf.redo_count = reinterpret_cast<const unsigned long long*>(so.d_qctr.p) + QCTR_FLAGGED;
      c->view = &bf;
      QueryLaunch ql{ VERIFY_REDO_ON_DEVICE, t0, query_geom(c, true), so.list_cap };
      ql.d_tile_idx = so.d_flag_idx;
      lrc = launch_query(c, r, ql);
      c->view = nullptr;
      if (lrc != GRP_OK) {
        return lrc;
      }
      HIP_TRY(c, hipGetLastError());
      redo_on_device = true;
    }
    int erc = classify_enqueue_decide(c, so, c->stream);
    if (erc == GRP_OK) {
      erc = classify_enqueue_fetch(c, so, c->stream);
    }
    return erc;
  };

  rc = enqueue();
  if (rc != GRP_OK) {
    return rc;
  }
  HIP_TRY(c, hipEventSynchronize(so.done));
  bool done = false;
  for (int attempt = 0; attempt < 8 && !done; ++attempt) { // (worst case 5: arena too small for the window, then for the redone tiles' lists)
    if (so.h_qctr[QCTR_IMPOSSIBLE] && attempt == 0) {
      // the patch's self-check (an older ID gained a frame / a count below zero): such a tile is flagged like any tile
      // whose patch was given up and is queried again through the log below — exact — so the run goes on; the count is
      // kept and said once (ADVICE r04: this used to end the run with the carry and the slot half updated)
      c->n_verify_impossible += so.h_qctr[QCTR_IMPOSSIBLE];
      if (c->sw.verify_strict) { // GRP_VERIFY_STRICT, developer switch: a logic error of the patch ends the run (the GPU tests assert the count is 0)
        (void)grp_batch_undo(c, br.first_read, id_floor[0] & 0x7FFFFFFFu);
        return set_err(c, GRP_ERR_STATE, "grp_batch_verify: %llu tiles with an impossible delta (GRP_VERIFY_STRICT; the batch was taken back)", (unsigned long long)so.h_qctr[QCTR_IMPOSSIBLE]);
      }
      static bool said = false;
      if (!said) {
        said = true;
        fprintf(stderr, "grp_batch_verify: %llu tiles with an impossible delta (patch given up, the tiles are queried again; grp_verify_stats counts them)\n", (unsigned long long)so.h_qctr[QCTR_IMPOSSIBLE]);
      }
    }
    if (so.h_qctr[QCTR_LIST_CURSOR] > so.list_cap) { // list arena too small: grow and redo the window (the inputs are untouched)
      so.list_cap = 2 * so.h_qctr[QCTR_LIST_CURSOR] + 4096; // (room for the lists of tiles that are redone: they are not in this count yet)
      rc = enqueue();
      if (rc != GRP_OK) {
        return rc;
      }
      HIP_TRY(c, hipEventSynchronize(so.done));
      continue;
    }
    c->n_verify_uncertified += so.h_qctr[QCTR_UNCERTIFIED];
    c->n_verify_unpatched += so.h_qctr[QCTR_UNPATCHED];
    if (so.h_qctr[QCTR_FLAGGED] && redo_on_device && so.h_qctr[QCTR_FLAGGED] <= VERIFY_REDO_ON_DEVICE && so.h_qctr[QCTR_FLAGGED] <= so.d_flag_idx.cap) {
      // redone behind the patch, inside the launches that have just been waited for
      c->n_verify_flagged += so.h_qctr[QCTR_FLAGGED];
      c->n_flagged_tiles += so.h_qctr[QCTR_FLAGGED];
      c->n_flagged_distinct += so.h_qctr[QCTR_FLAGGED_DISTINCT];
      c->n_flagged_list += so.h_qctr[QCTR_FLAGGED_LIST];
      ++c->n_redo_launches;
    } else if (so.h_qctr[QCTR_FLAGGED]) { // tiles that could not be patched / needed the worst-case table: through the log, decide again
      c->n_verify_flagged += so.h_qctr[QCTR_FLAGGED];
      QueryRun q;
      q.t0 = t0;
      c->q = &so;
      c->view = &bv;
      rc = enqueue_redo_flagged(c, r, so.list_cap, q);
      c->view = nullptr;
      if (rc == GRP_OK) {
        rc = classify_enqueue_decide(c, so, c->stream);
      }
      if (rc == GRP_OK) {
        rc = classify_enqueue_fetch(c, so, c->stream);
      }
      if (rc != GRP_OK) {
        return rc;
      }
      HIP_TRY(c, hipEventSynchronize(so.done));
      continue;
    }
    done = true;
  }
  if (!done) {
    // GRP_ERR_NOMEM means "nothing of the batch is in the filter and the batch is over" to the caller (it commits the
    // window's first insert the classic way and halves the batch): make that true
    (void)grp_batch_undo(c, br.first_read, id_floor[0] & 0x7FFFFFFFu);
    return set_err(c, GRP_ERR_NOMEM, "grp_batch_verify: list arena kept overflowing (the batch was taken back)");
  }
  if (c->pending.size() > 64) {
    drain_events(c);
  }
  memcpy(out, so.h_dec, (size_t)total * sizeof(grp_read_decision));
  c->n_verify_tiles += n_r;
  c->n_verify_queried += n_q;
  if (extra) {
    // the plain summaries of the reads behind the batch stay: the next window's first decisions
    // (valid as long as nothing changes the filter: the caller ends the batch confirmed in full)
    c->carry.valid = true;
    c->carry.slot = out_slot;
    c->carry.reads = r;
    c->carry.first = first + count;
    c->carry.count = extra;
    c->carry.tile_off = nt_batch;
  }
  return batch_check(c);
}

int
grp_debug_verify_stats(const grp_ctx* c, uint64_t out[12])
{
  if (!c || !out) {
    return GRP_ERR_INVALID;
  }
  out[0] = c->n_verify_tiles;
  out[1] = c->n_verify_queried;
  out[2] = c->n_verify_flagged;
  out[3] = c->n_verify_fallbacks;
  out[4] = c->n_verify_uncertified;
  out[5] = c->n_verify_unpatched;
  out[6] = c->n_flagged_tiles;
  out[7] = c->n_flagged_distinct;
  out[8] = c->n_flagged_list;
  out[9] = c->n_batch_sweeps;
  out[10] = c->n_verify_impossible; // tiles whose patch failed its self-check (queried again through the log)
  out[11] = c->n_far;               // count words living in the far table (ranks beyond their bucket's 8th set bit)
  return GRP_OK;
}

int
grp_debug_filter_geometry(const grp_ctx* c, uint64_t out[4])
{
  if (!c || !out) {
    return GRP_ERR_INVALID;
  }
  if (!c->finalized) {
    return GRP_ERR_STATE; // (a const context: no message is kept)
  }
  out[0] = c->f.W;
  out[1] = c->f.n_buckets;
  out[2] = c->n_ovf;
  out[3] = c->n_far;
  return GRP_OK;
}

} // extern "C"
