// The POSITION-SHARDED query, priced on one device (round 5, VERDICT r04 item 3; SURVEY 8(e) "if a replica does not
// fit"): the miBF cut into N contiguous ranges of buckets, one per owner GPU; a window's probes travel to the owners
// of their buckets and the IDs travel back.  On N GPUs that turns the replicated insert work (every rank applies every
// insert on its replica: the Amdahl term of DESIGN 7) into sharded work, and 1 / N of the filter per GPU.  What it costs
// the QUERY is measured here with N virtual owners on ONE device — the partition pass, the gather in owner order and the
// return pass need no xGMI to be timed (the links carry 8 B out and 4 B back per probe: DESIGN 7 has the arithmetic):
//   k_ps_partition  one workgroup per tile (k_query's staging and hashes, goldrush_path.cpp:559-566 /
//                   multiLensfrHashIterator.hpp:49-68): every (frame, seed) probe becomes a record
//                   {bucket * 64 + bit offset} in ITS OWNER's bin, the tile's records of one owner contiguous (the
//                   workgroup counts per owner in LDS and reserves the eight segments with eight atomics); the
//                   probe's place in its tile (frame * h + seed, 16 bits) stays behind in a tag array of the same
//                   shape — what the owner sends back comes in the order it was sent
//   k_ps_gather     the owner's side: its bin in order, the bucket line of every record read by the lane's quad
//                   (atRank + getData, MIBloomFilter.hpp:465-476, 614-621), 4 bytes back per record: the ID, or
//                   PS_CLEAR where the filter bit is not set
//   k_ps_vote       one workgroup per tile: the eight segments of answers and tags (sequential) scattered into the
//                   tile's frame x seed array in LDS, then k_query's vote on it: all-or-nothing per frame, saturation bit
//                   stripped, ID 0 a miss, distinct IDs of the frame counted once (goldrush_path.cpp:571-604), top ID
//                   (ties to the smallest) and the count > 2 list (:607-625)
// A developer entry point (grp_pshard_query, tools/pshard_bench.py): the product's query stays k_query.
// Included by grpath_hip.hip (same translation unit).

namespace {

constexpr uint32_t PS_CLEAR = 0xFFFFFFFFu; // "the probe's filter bit is not set" (no ID has all 32 bits set: bit 31 is the saturation flag of a 31-bit ID)
constexpr uint32_t PS_MAX_OWNERS = 16;

struct DevPshard
{
  uint32_t n_owners;
  uint64_t per_owner;      // buckets per owner (the last one may hold fewer)
  uint64_t owner_magic;    // floor(2^64 / per_owner) + 1
  unsigned long long* bin_fill; // [n_owners] records reserved per bin
  uint64_t bin_cap;        // records per bin
  unsigned long long* keys;  // [n_owners][bin_cap] bucket * 64 + bit offset
  uint16_t* tags;          // [n_owners][bin_cap] frame * h + seed inside the record's tile
  uint32_t* answers;       // [n_owners][bin_cap]
  uint2* segs;             // [tiles][n_owners] {first record in the owner's bin (low 32 bits), count}: bins hold < 2^32 records
};

template<int H, int WT>
__global__ void __launch_bounds__(THREADS)
k_ps_partition(DevFilter f, DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint64_t tile_begin, DevPshard ps)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + H * sd->wmax * 4u);
  __shared__ uint32_t sCnt[PS_MAX_OWNERS], sPos[PS_MAX_OWNERS];
  __shared__ unsigned long long sOff[PS_MAX_OWNERS];
  const uint64_t t = tile_begin + blockIdx.x;
  const uint32_t r = rd.tile_read[t];
  const uint32_t ti = (uint32_t)(t - rd.tile0[r]);
  const uint32_t len = rd.len[r];
  const uint32_t k = sd->k;
  const gr::geom::TileExtent ext = gr::geom::tile_extent(tile_len, k, k, len, ti); // (seed 0 spans k here: the launch refuses anything else)
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;
  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, start, Lp);
  if (threadIdx.x < PS_MAX_OWNERS) {
    sCnt[threadIdx.x] = 0;
    sPos[threadIdx.x] = 0;
  }
  __syncthreads();
  // pass 1: how many of the tile's probes go to each owner (the hashes are computed twice: they are cheap beside
  // the traffic, and a tile of any length needs no per-lane record store)
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t fr = threadIdx.x; fr < frames; fr += THREADS) {
#pragma unroll
      for (int s = 0; s < H; ++s) {
        const uint32_t fs = min(fr, Lp - sd->span[s]); // a seed that can no longer roll keeps its last value
        const Probe pr = grp_locate(f, seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs)));
        const uint32_t owner = min((uint32_t)__umul64hi(pr.b, ps.owner_magic), ps.n_owners - 1u);
        if (pass == 0) {
          atomicAdd(&sCnt[owner], 1u);
        } else {
          const unsigned long long at = sOff[owner] + atomicAdd(&sPos[owner], 1u);
          if (at < ps.bin_cap) {
            ps.keys[(size_t)owner * ps.bin_cap + at] = (unsigned long long)pr.b * 64ull + pr.off;
            ps.tags[(size_t)owner * ps.bin_cap + at] = (uint16_t)(fr * (uint32_t)H + (uint32_t)s);
          }
        }
      }
    }
    __syncthreads();
    if (pass == 0) {
      if (threadIdx.x < ps.n_owners) {
        const uint32_t n = sCnt[threadIdx.x];
        const unsigned long long at = n ? atomicAdd(&ps.bin_fill[threadIdx.x], (unsigned long long)n) : 0ull;
        sOff[threadIdx.x] = at;
        ps.segs[(size_t)blockIdx.x * ps.n_owners + threadIdx.x] = make_uint2((uint32_t)at, n);
      }
      __syncthreads();
    }
  }
}

// the owner's side: records [0, n) of one bin
__global__ void __launch_bounds__(THREADS)
k_ps_gather(DevFilter f, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ answers, uint64_t n)
{
  const QuadLane ql = quad_lane();
  const uint32_t pbytes = quad_piece_bytes(ql.sub);
  for (uint64_t i0 = (uint64_t)blockIdx.x * THREADS; i0 < n; i0 += (uint64_t)gridDim.x * THREADS) {
    const uint64_t i = i0 + threadIdx.x;
    const unsigned long long key = i < n ? keys[i] : 0ull; // (lanes beyond the bin read bucket 0: the quad exchange needs every lane)
    const uint64_t b = key >> 6;
    const uint32_t off = (uint32_t)(key & 63ull);
    uint4 pc[4];
    pc[0] = quad_load<0>(f.buckets, b, pbytes);
    pc[1] = quad_load<1>(f.buckets, b, pbytes);
    pc[2] = quad_load<2>(f.buckets, b, pbytes);
    pc[3] = quad_load<3>(f.buckets, b, pbytes);
    const QuadAnswer mine = quad_decode(pc, off, ql);
    uint32_t d = mine.id;
    if (mine.lr >= GRP_BUCKET_IDS && mine.bit) { // 14th.. set bit of its bucket: rare side table
      d = grp_ovf_get(f, f.super[b >> GRP_SUPER_SHIFT] + mine.rel + mine.lr);
    }
    if (i < n) {
      answers[i] = mine.bit ? d : PS_CLEAR;
    }
  }
}

// k_query's vote on the answers that came back; hist_cap / limit as query_geom(full)
template<int H>
__global__ void __launch_bounds__(THREADS)
k_ps_vote(DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint64_t tile_begin, DevPshard ps, uint32_t hist_cap, uint32_t distinct_limit, grp_tile_summary* __restrict__ tiles_out,
          grp_id_count* __restrict__ lists_out, uint64_t lists_cap, unsigned long long* __restrict__ list_ctr)
{
  extern __shared__ uint4 smem4[];
  uint32_t* sKeys = reinterpret_cast<uint32_t*>(smem4);
  uint32_t* sCnts = sKeys + hist_cap; // 16-bit counts, two per word
  uint32_t* sAns = sCnts + hist_cap / 2u; // [frames * H]
  __shared__ uint32_t sDistinct, sOverflow, sListN, sListW, sBest[2 * (THREADS / 64)], sRed[2 * (THREADS / 64)], sListOff;
  const uint64_t t = tile_begin + blockIdx.x;
  const uint32_t r = rd.tile_read[t];
  const uint32_t ti = (uint32_t)(t - rd.tile0[r]);
  const uint32_t len = rd.len[r];
  const uint32_t k = sd->k;
  const uint32_t frames = gr::geom::tile_extent(tile_len, k, k, len, ti).frames; // (seed 0 spans k here: the launch refuses anything else)
  for (uint32_t i = threadIdx.x; i < hist_cap; i += THREADS) {
    sKeys[i] = 0u;
    if (i < hist_cap / 2u) {
      sCnts[i] = 0u;
    }
  }
  if (threadIdx.x == 0) {
    sDistinct = 0;
    sOverflow = 0;
    sListN = 0;
    sListW = 0;
  }
  // the answers of the tile's probes, owner by owner, back to their places
  for (uint32_t o = 0; o < ps.n_owners; ++o) {
    const uint2 sg = ps.segs[(size_t)blockIdx.x * ps.n_owners + o];
    const size_t base = (size_t)o * ps.bin_cap + sg.x;
    for (uint32_t i = threadIdx.x; i < sg.y; i += THREADS) {
      sAns[ps.tags[base + i]] = ps.answers[base + i];
    }
  }
  __syncthreads();
  uint32_t n_hit = 0, n_miss = 0;
  for (uint32_t fr = threadIdx.x; fr < frames; fr += THREADS) {
    uint32_t idv[H];
    bool all = true;
#pragma unroll
    for (int s = 0; s < H; ++s) {
      idv[s] = sAns[fr * (uint32_t)H + (uint32_t)s];
      all = all && idv[s] != PS_CLEAR; // atRank (MIBloomFilter.hpp:465-476): all or nothing
    }
    if (!all) {
      continue;
    }
    uint32_t ids[H];
#pragma unroll
    for (int s = 0; s < H; ++s) {
      const uint32_t d = idv[s];
      const uint32_t id = (d > 0x80000000u) ? (d & 0x7FFFFFFFu) : d; // saturation bit stripped exactly as goldrush_path.cpp:573-594
      if (id == 0u) {
        ++n_miss;
      } else {
        ++n_hit;
      }
      bool dup = false;
#pragma unroll
      for (int u = 0; u < s; ++u) {
        dup = dup || ids[u] == id;
      }
      ids[s] = id;
      if (id != 0u && !dup) {
        hist_add16(sKeys, sCnts, hist_cap, id, &sDistinct, distinct_limit, &sOverflow);
      }
    }
  }
  __syncthreads();
  uint32_t bc = 0, bid = 0, my_n = 0;
  for (uint32_t i = threadIdx.x; i < hist_cap; i += THREADS) {
    const uint32_t key = sKeys[i];
    if (key != 0u) {
      const uint32_t c = (sCnts[i >> 1] >> ((i & 1u) << 4)) & 0xFFFFu;
      if (better(c, key, bc, bid)) {
        bc = c;
        bid = key;
      }
      my_n += c > 2u ? 1u : 0u;
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
  n_hit = wave_sum(n_hit);
  n_miss = wave_sum(n_miss);
  my_n = wave_sum(my_n);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sBest[2 * wave] = bc;
    sBest[2 * wave + 1] = bid;
    sRed[2 * wave] = n_hit;
    sRed[2 * wave + 1] = n_miss;
    if (my_n) {
      atomicAdd(&sListN, my_n);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t hsum = 0, msum = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
      if (better(sBest[2 * w], sBest[2 * w + 1], bc, bid)) {
        bc = sBest[2 * w];
        bid = sBest[2 * w + 1];
      }
      hsum += sRed[2 * w];
      msum += sRed[2 * w + 1];
    }
    const uint32_t n = sListN;
    const uint64_t lo = n ? atomicAdd(list_ctr, (unsigned long long)n) : 0ull;
    sListOff = (uint32_t)lo;
    grp_tile_summary ts;
    ts.top_id = bid;
    ts.top_count = bc;
    ts.list_off = (uint32_t)lo;
    ts.list_n = sOverflow ? GRP_TILE_FLAGGED : n; // (cannot happen: the table holds the worst case)
    ts.hits = hsum;
    ts.misses = msum;
    tiles_out[blockIdx.x] = ts;
  }
  __syncthreads();
  if (sListN != 0u) {
    const uint64_t lo = sListOff;
    for (uint32_t i = threadIdx.x; i < hist_cap; i += THREADS) {
      const uint32_t key = sKeys[i];
      if (key == 0u) {
        continue;
      }
      const uint32_t c = (sCnts[i >> 1] >> ((i & 1u) << 4)) & 0xFFFFu;
      if (c <= 2u) {
        continue;
      }
      const uint64_t at = lo + atomicAdd(&sListW, 1u);
      if (at < lists_cap) {
        lists_out[at].id = key;
        lists_out[at].count = c;
      }
    }
  }
}

// ---- a hashed filter of the ranks a batch touched, in front of the second query (VERDICT r04 item 4) ----------------
// The second decisions of the tiles nobody inserted ask the filter again for every probe (grp_verify.inc) to find the
// few whose rank an insert of the batch wrote.  Would a small hashed set of the touched (bucket, bit) positions — 8 /
// 16 MiB: the L2s and the memory-side cache serve it — answer "this frame is clean" faster than the bucket lines do?
// This kernel is that pass alone: every (frame, seed) of a window's tiles hashed as the query hashes them, `n_hash`
// bits of a table of `table_words` words tested per probe, a frame counted dirty when any of its h probes hits.  The
// table is filled by the caller to the share of set bits a batch of the head leaves.  Measurement only.
template<int H, int WT>
__global__ void __launch_bounds__(THREADS)
k_touch_probe(DevFilter f, DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint64_t tile_begin, const uint32_t* __restrict__ table, uint32_t table_mask, uint32_t n_hash,
              unsigned long long* __restrict__ dirty_frames)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + H * sd->wmax * 4u);
  const uint64_t t = tile_begin + blockIdx.x;
  const uint32_t r = rd.tile_read[t];
  const uint32_t ti = (uint32_t)(t - rd.tile0[r]);
  const uint32_t len = rd.len[r];
  const uint32_t k = sd->k;
  const gr::geom::TileExtent ext = gr::geom::tile_extent(tile_len, k, k, len, ti); // (seed 0 spans k here: the launch refuses anything else)
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;
  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, start, Lp);
  __syncthreads();
  uint32_t dirty = 0;
  for (uint32_t fr = threadIdx.x; fr < frames; fr += THREADS) {
    uint32_t w[H * 2];
    uint32_t bit[H * 2];
#pragma unroll
    for (int s = 0; s < H; ++s) {
      const uint32_t fs = min(fr, Lp - sd->span[s]);
      const Probe pr = grp_locate(f, seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs)));
      const uint64_t key = (pr.b * 64ull + pr.off) * 0x9E3779B97F4A7C15ULL;
      const uint32_t h0 = (uint32_t)(key >> 32), h1 = (uint32_t)key * 0x85EBCA6Bu;
      w[2 * s] = table[(h0 >> 5) & table_mask];
      bit[2 * s] = h0 & 31u;
      w[2 * s + 1] = n_hash > 1 ? table[(h1 >> 5) & table_mask] : 0xFFFFFFFFu;
      bit[2 * s + 1] = h1 & 31u;
    }
    bool any = false;
#pragma unroll
    for (int s = 0; s < H; ++s) {
      any = any || (((w[2 * s] >> bit[2 * s]) & 1u) && ((w[2 * s + 1] >> bit[2 * s + 1]) & 1u));
    }
    dirty += any ? 1u : 0u;
  }
  dirty = wave_sum(dirty);
  if ((threadIdx.x & 63) == 0 && dirty) {
    atomicAdd(dirty_frames, (unsigned long long)dirty);
  }
}

__global__ void __launch_bounds__(THREADS)
k_touch_fill(uint32_t* __restrict__ table, uint64_t n_words, uint32_t threshold_20bit)
{
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * THREADS) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 32; ++b) {
      uint64_t x = (i * 32 + b) * 0xD6E8FEB86659FD93ULL + 0x9E3779B97F4A7C15ULL;
      x ^= x >> 32;
      x *= 0xD6E8FEB86659FD93ULL;
      x ^= x >> 29;
      v |= ((uint32_t)(x & 0xFFFFFu) < threshold_20bit ? 1u : 0u) << b;
    }
    table[i] = v;
  }
}

} // namespace

extern "C" {

// Measurement (VERDICT r04 item 4): the hash-and-test pass of a touched-rank filter of `table_mib` MiB with a share
// `fill` of its bits set and `n_hash` (1 or 2) bits tested per probe, over the tiles of reads [first, first + count).
// *ms = the kernel (HIP events, best of 3), *dirty = frames with at least one probe that hits (what would be
// evaluated through the log), *frames = all frames.
int
grp_debug_touch_filter(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, uint32_t table_mib, double fill, uint32_t n_hash, float* ms, uint64_t* dirty, uint64_t* frames_out)
{
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads || table_mib == 0 || table_mib > 8192 || (table_mib & (table_mib - 1)) || n_hash < 1 || n_hash > 2 || !ms || !dirty) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_touch_filter: bad argument (the table size is a power of two of MiB)");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_debug_touch_filter before grp_finalize");
  }
  if (long_span(c)) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_touch_filter: the prototype hashes seeds of spans up to 64 bases only (k+h-1=%u)", c->params.k + c->params.h - 1);
  }
  if (span0(c) != c->params.k) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_touch_filter: the prototype takes tiles of `tile` frames only (seed 0 spans %u bases, k=%u)", span0(c), c->params.k);
  }
  if (c->params.h > GRP_H_GROUP) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_touch_filter: the prototype hashes up to %d seeds per frame only (h=%u)", GRP_H_GROUP, c->params.h);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t H = c->params.h, tile = c->params.tile;
  const uint64_t t0 = r->tile0[first];
  const uint64_t nt = r->tile0[first + count] - t0;
  if (nt == 0 || nt > MAX_GRID_WGS) {
    return set_err(c, GRP_ERR_INVALID, "grp_debug_touch_filter: %llu tiles", (unsigned long long)nt);
  }
  const uint64_t n_words = (uint64_t)table_mib << 18;
  DevBuf<uint32_t> d_table; // (developer entry points: what they allocate lives for one call)
  DevBuf<unsigned long long> d_dirty;
  Event e0, e1;
  HIP_TRY(c, d_table.reset(n_words));
  HIP_TRY(c, d_dirty.reset(1));
  k_touch_fill<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(d_table, n_words, (uint32_t)(fill * 1048576.0));
  const size_t lds = tab_bytes(c) + bases_bytes(tile + c->params.k + H);
  HIP_TRY(c, e0.create(hipEventDefault));
  HIP_TRY(c, e1.create(hipEventDefault));
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {
    HIP_TRY(c, hipMemsetAsync(d_dirty, 0, 8, c->stream));
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    if (c->uniform_weight == 16) {
      DISPATCH_H_FEW(H, (k_touch_probe<HH, 16><<<dim3((uint32_t)nt), dim3(THREADS), lds, c->stream>>>(c->f, r->dev, c->d_seeds, tile, t0, d_table, (uint32_t)(n_words - 1), n_hash, d_dirty)));
    } else {
      DISPATCH_H_FEW(H, (k_touch_probe<HH, 0><<<dim3((uint32_t)nt), dim3(THREADS), lds, c->stream>>>(c->f, r->dev, c->d_seeds, tile, t0, d_table, (uint32_t)(n_words - 1), n_hash, d_dirty)));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    HIP_TRY(c, hipEventSynchronize(e1));
    float t = 0;
    (void)hipEventElapsedTime(&t, e0, e1);
    best = std::min(best, t);
  }
  unsigned long long h_dirty = 0;
  HIP_TRY(c, hipMemcpy(&h_dirty, d_dirty, 8, hipMemcpyDeviceToHost));
  *ms = best;
  *dirty = h_dirty;
  if (frames_out) {
    *frames_out = nt * tile; // (full tiles: the bench's reads end behind their last tile)
  }
  return GRP_OK;
}

// Tile summaries of reads [first, first + count) through the position-sharded form with `n_owners` virtual owners
// (the result grp_query_tiles gives: same fields, lists in any order).  times_ms[3]: partition, gather (all owners'
// bins), vote — HIP events around the kernels.  gather_span: 0 = the owners' bins one after the other (each confined
// to its 1 / n_owners of the table: what an owner GPU does), as measured.
int
grp_pshard_query(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, uint32_t n_owners, grp_tile_summary* tiles, grp_id_count* lists, uint64_t list_cap, uint64_t* list_used, float* times_ms)
{
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads || !tiles || (!lists && list_cap) || n_owners == 0 || n_owners > PS_MAX_OWNERS) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: bad argument");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_pshard_query before grp_finalize");
  }
  if (long_span(c)) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: the prototype hashes seeds of spans up to 64 bases only (k+h-1=%u)", c->params.k + c->params.h - 1);
  }
  if (span0(c) != c->params.k) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: the prototype takes tiles of `tile` frames only (seed 0 spans %u bases, k=%u)", span0(c), c->params.k);
  }
  if (c->params.h > GRP_H_GROUP) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: the prototype hashes up to %d seeds per frame only (h=%u)", GRP_H_GROUP, c->params.h);
  }
  const uint32_t H = c->params.h, tile = c->params.tile;
  if ((uint64_t)tile * H > 65535u) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: more than 65535 probes per tile (the tags are 16 bits)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t t0 = r->tile0[first];
  const uint64_t nt = r->tile0[first + count] - t0;
  if (nt == 0) {
    if (list_used) {
      *list_used = 0;
    }
    return GRP_OK;
  }
  if (nt > MAX_GRID_WGS) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: %llu tiles in one call (limit %u)", (unsigned long long)nt, MAX_GRID_WGS);
  }
  if (query_geom(c, true).global_table) { // (before anything is allocated: ADVICE r05)
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: the prototype keeps a tile's count table in LDS (tile x h too large)");
  }
  const uint64_t probes = nt * tile * H;
  DevPshard ps{};
  ps.n_owners = n_owners;
  ps.per_owner = (c->f.n_buckets + n_owners - 1) / n_owners;
  ps.owner_magic = (uint64_t)((((unsigned __int128)1) << 64) / ps.per_owner) + 1;
  ps.bin_cap = probes / n_owners + probes / (4 * n_owners) + 65536; // uniform hashes: a bin holds its share +- a little
  if (ps.bin_cap >= (1ull << 32)) {
    return set_err(c, GRP_ERR_INVALID, "grp_pshard_query: window too large (a bin holds < 2^32 records)");
  }
  DevBuf<unsigned long long> bin_fill, keys, d_ctr; // (the views go into `ps`)
  DevBuf<uint16_t> tags;
  DevBuf<uint32_t> answers;
  DevBuf<uint2> segs;
  DevBuf<grp_tile_summary> d_tiles;
  DevBuf<grp_id_count> d_lists;
  Event ev[5];
  const uint64_t lcap = std::max<uint64_t>(list_cap, 1);
  if (bin_fill.reset(PS_MAX_OWNERS) != hipSuccess || keys.reset(n_owners * ps.bin_cap) != hipSuccess || tags.reset(n_owners * ps.bin_cap) != hipSuccess || answers.reset(n_owners * ps.bin_cap) != hipSuccess ||
      segs.reset(nt * n_owners) != hipSuccess || d_tiles.reset(nt) != hipSuccess || d_lists.reset(lcap) != hipSuccess || d_ctr.reset(1) != hipSuccess) {
    return set_err(c, GRP_ERR_NOMEM, "grp_pshard_query: no memory for the bins of %llu probes", (unsigned long long)probes);
  }
  ps.bin_fill = bin_fill;
  ps.keys = keys;
  ps.tags = tags;
  ps.answers = answers;
  ps.segs = segs;
  for (Event& e : ev) {
    HIP_TRY(c, e.create(hipEventDefault));
  }
  HIP_TRY(c, hipMemsetAsync(ps.bin_fill, 0, PS_MAX_OWNERS * 8, c->stream));
  HIP_TRY(c, hipMemsetAsync(d_ctr, 0, 8, c->stream));
  const QueryGeom g = query_geom(c, true);
  const size_t lds_part = tab_bytes(c) + bases_bytes(tile + c->params.k + H);
  const size_t lds_vote = (size_t)g.hist_cap * 6 + (size_t)tile * H * 4 + 64;
  HIP_TRY(c, hipEventRecord(ev[0], c->stream));
  if (c->uniform_weight == 16) {
    DISPATCH_H_FEW(H, (k_ps_partition<HH, 16><<<dim3((uint32_t)nt), dim3(THREADS), lds_part, c->stream>>>(c->f, r->dev, c->d_seeds, tile, t0, ps)));
  } else {
    DISPATCH_H_FEW(H, (k_ps_partition<HH, 0><<<dim3((uint32_t)nt), dim3(THREADS), lds_part, c->stream>>>(c->f, r->dev, c->d_seeds, tile, t0, ps)));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(ev[1], c->stream));
  unsigned long long fill[PS_MAX_OWNERS];
  HIP_TRY(c, hipMemcpyAsync(fill, ps.bin_fill, sizeof(fill), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint32_t o = 0; o < n_owners; ++o) {
    if (fill[o] > ps.bin_cap) {
      return set_err(c, GRP_ERR_NOMEM, "grp_pshard_query: owner %u was sent %llu records, its bin holds %llu", o, fill[o], (unsigned long long)ps.bin_cap);
    }
  }
  HIP_TRY(c, hipEventRecord(ev[2], c->stream));
  for (uint32_t o = 0; o < n_owners; ++o) {
    if (fill[o]) {
      k_ps_gather<<<dim3((uint32_t)std::min<uint64_t>((fill[o] + THREADS - 1) / THREADS, 256 * 32)), dim3(THREADS), 0, c->stream>>>(c->f, ps.keys + (size_t)o * ps.bin_cap, ps.answers + (size_t)o * ps.bin_cap, fill[o]);
    }
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(ev[3], c->stream));
  DISPATCH_H_FEW(H, (k_ps_vote<HH><<<dim3((uint32_t)nt), dim3(THREADS), lds_vote, c->stream>>>(r->dev, c->d_seeds, tile, t0, ps, g.hist_cap, g.distinct_limit, d_tiles, d_lists, lcap, d_ctr)));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(ev[4], c->stream));
  unsigned long long used = 0;
  HIP_TRY(c, hipMemcpyAsync(&used, d_ctr, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(tiles, d_tiles, nt * sizeof(grp_tile_summary), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (list_cap) {
    HIP_TRY(c, hipMemcpy(lists, d_lists, std::min<uint64_t>(used, list_cap) * sizeof(grp_id_count), hipMemcpyDeviceToHost));
  }
  if (list_used) {
    *list_used = used;
  }
  if (times_ms) {
    (void)hipEventElapsedTime(&times_ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&times_ms[1], ev[2], ev[3]);
    (void)hipEventElapsedTime(&times_ms[2], ev[3], ev[4]);
  }
  return GRP_OK;
}

} // extern "C"
