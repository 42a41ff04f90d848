// Batches of inserts applied AHEAD of their reads' queries (grp_batch_*, include/grpath.h).
//
// The reference's loop is serial: read j is queried after the inserts of every accepted read
// < j (goldrush_path.cpp:1229-1256), and in the insert-heavy start of a path nearly every read
// inserts, so a window is one read and a round costs ~77 us of dependent small launches.  But
// two reads share ~1 rank (75 k probes each over 6e9 ranks), so the DECISIONS of the reads of a
// window taken against one state almost always hold.  A batch does this, exactly:
//   1. the window is decided against the state in front of it (grp_classify_reads);
//   2. grp_batch_insert_reads applies the inserts those decisions ask for, all at once, in the
//      reference's order per rank (read by read, block by block), and keeps what a later read of
//      the window must not see: per rank what was there before the batch, and for a rank that is
//      touched more than once in the batch a log of its writes ({old value, writing read});
//   3. grp_batch_classify queries the window again THROUGH THE LOG: IDs grow with the read
//      order, so a probe that returns an ID >= the first ID read j could allocate was written by
//      read j or a later one, and read j sees the old value of the earliest such write instead
//      (0 if that write went into an empty slot and is not logged) — the state in front of its
//      own insert, hits / misses counters included;
//   4. the caller compares the two sets of decisions in order: where they agree the batch was
//      the serial loop; at the first read that differs, grp_batch_undo takes back the inserts
//      of that read and the ones behind it (the same log tells what was there).
//
// Data: one RECORD per (frame, seed) of the inserted tiles at a fixed index (no reservation:
// record (unit * H + seed) * THREADS + lane, unit = 1024 frames of one tile), filled by the lane
// that is the first of the batch to touch the rank (its owner).  The claim lives in the rank's COUNT word
// (round 4, grp_device.h: count | epoch of the batch | record): one compare-and-swap both claims the rank and
// counts the owner's touch, on the line the count has to be read from anyway — the hash table rank -> record of
// rounds 2-3 (a third random line per record) is gone, and with it its clearing after every batch: a claim of
// an older epoch is no claim (the epochs wrap after 1023 batches, then the words are swept once).
// Touches of the rank by OTHER (read, block)s are chained to the
// owner's record.  The owner applies its touch at once (the ID slot is in the bucket line it
// has just read for the rank) and keeps what was there; the second pass only logs, and replays
// in the reference's order the few ranks that ended up with a chain.  Undo streams over the
// records.
// Included by grpath_hip.hip (same translation unit).

namespace {

constexpr uint32_t BATCH_MAX_INS = 1u << 17;    // inserting reads per batch (17 bits of a record word)
constexpr uint32_t BATCH_MAX_BLOCKS = 256;      // ID blocks per read (8 bits)
constexpr uint64_t BATCH_MAX_REC = 1ull << 26;  // records per batch (26 bits of a table word)
constexpr unsigned long long BATCH_LOW26 = (1ull << 26) - 1ull;

struct DevBatch
{
  uint32_t epoch = 0;                    // of this batch, 1 .. GRP_EPOCH_MAX (the claim field of f.counts)
  uint32_t* bits = nullptr;              // per hash slot: a rank with this home slot has something to restore
  uint64_t cap_mask = 0;
  uint32_t* counters = nullptr;          // [0] records that own a chain [1] chained touches [2] log entries [3] error
  uint32_t* chained = nullptr;           // [counters[0]] those records (the first touch chained to a record enters it)
  const uint32_t* ins = nullptr;         // [n_ins][6]
  uint32_t n_ins = 0, block_tiles = 0;
  uint32_t n_rec = 0;
  unsigned long long* rec_key = nullptr; // (rank + 1) << 26 | read-of-the-batch << 8 | block; 0: no record here
  unsigned long long* rec_loc = nullptr; // grp_id_loc: bucket * 32 + dword of the ID slot inside the bucket's unit (= its dword index); dword 0: the ID lives in the overflow table
  unsigned long long* rec_old = nullptr; // wrote << 63 | count before << 32 | ID before
  uint32_t* rec_chain = nullptr;         // newest touch by another (read, block), BATCH_NONE: none
  uint32_t* ovf_next = nullptr;
  uint32_t* ovf_jb = nullptr;
  uint32_t ovf_cap = 0;
  unsigned long long* log_keys = nullptr;
  uint32_t* log_head = nullptr;
  uint32_t* log_old = nullptr;
  uint32_t* log_writer = nullptr;
  uint32_t* log_next = nullptr;
  uint32_t* log_slot = nullptr;
  uint64_t log_mask = 0;
  uint32_t log_cap = 0;
  uint32_t first_read = 0; // reads are numbered from here in the log
};

__device__ inline uint32_t
batch_block_id(const DevBatch& b, uint32_t jb)
{
  const uint32_t j = jb >> 8, blk = jb & 255u;
  const uint32_t* e = b.ins + (size_t)j * 6;
  return e[3] + (blk * b.block_tiles + e[4]) / b.block_tiles; // grp_insert_read's rule
}

// ctr += 1 for every lane that is here, one atomic for all of them; returns the lane's own value of the counter
__device__ inline uint32_t
wave_counter_take(uint32_t* ctr)
{
  const unsigned long long here = __ballot(1);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t leader = (uint32_t)__ffsll((long long)here) - 1u;
  uint32_t base = 0;
  if (lane == leader) {
    base = atomicAdd(ctr, (uint32_t)__popcll(here));
  }
  base = __shfl(base, (int)leader, 64);
  return base + (uint32_t)__popcll(here & ((1ull << lane) - 1ull));
}

// (insert of the batch) << 8 | ID block of the unit's tile
__device__ inline uint32_t
batch_unit_jb(const DevBatch& b, uint32_t unit, uint32_t parts)
{
  uint32_t lo = 0, hi = b.n_ins;
  while (hi - lo > 1) { // the last insert whose first unit is <= unit
    const uint32_t mid = (lo + hi) >> 1;
    if (b.ins[(size_t)mid * 6 + 5] <= unit) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const uint32_t tj = (unit - b.ins[(size_t)lo * 6 + 5]) / parts;
  return (lo << 8) | (tj / b.block_tiles);
}

// collect: every distinct rank of the batch gets ONE record, written by the lane whose CAS
// claims the rank; a touch by another (read, block) is chained to that record.  One workgroup =
// THREADS frames of one tile under ONE seed (blockIdx = unit * H + seed): a lane has a single
// probe, so the claim loop and the owner's touch are straight-line code around one loop.
// CLAIM-LOOP RULE (DESIGN.md 5b "the lost touches of round 2"): ONE seed per claim loop, its hash / bucket header
// computed right in front of the loop, nothing but the frame position live across it.  Keeping the triples of
// several seeds live across unrolled claim loops loses touches of the last seed with this hipcc.  The guard:
// tests/test_gpu_batch.py::test_claim_loops_keep_every_touch (this kernel: [batch]).
// The query line of a probe's unit is read by the lane's QUAD — one 64-byte request that brings header AND ID slot
// (the query's access, quad_decode; rounds 2 - 4 loaded 16 bytes of header and 4 bytes of slot per lane: round 5's matrix,
// profiles/r05_collect_matrix.txt).
template<int H, int WT>
__global__ void __launch_bounds__(THREADS)
k_batch_collect(DevFilter f, DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, DevBatch b, uint32_t gunit0)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  const uint32_t hn = frame_seeds<H>(sd); // (one seed per workgroup: the many-seed form differs in its strides only)
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);

  const uint32_t gunit = gunit0 + blockIdx.x;
  const uint32_t unit = gunit / hn;
  const uint32_t s = gunit - unit * hn;
  const uint32_t parts = gr::geom::tile_parts(frames_per_tile(sd, tile_len));
  const uint32_t jb = batch_unit_jb(b, unit, parts);
  const uint32_t* e = b.ins + (size_t)(jb >> 8) * 6;
  const uint32_t read_idx = e[0], tile_start = e[1];
  const uint32_t u = unit - e[5];
  const uint32_t tj = u / parts, part = u - tj * parts;
  const uint32_t ti = tile_start + tj;
  // the units of this unit's (read, block): a record of one of them is the same dedup scope (no search per chained touch:
  // an insert's units are consecutive)
  const uint32_t blk_unit0 = e[5] + (tj / b.block_tiles) * b.block_tiles * parts;
  const uint32_t blk_unit1 = min(blk_unit0 + b.block_tiles * parts, e[5] + (e[2] - e[1]) * parts);
  const uint32_t len = rd.len[read_idx];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, ti);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;

  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[read_idx], len, start, Lp);
  __syncthreads();

  const uint32_t fr = part * THREADS + threadIdx.x;
  const bool live = fr < frames;
  const uint32_t fs = min(min(fr, frames ? frames - 1u : 0u), Lp - sd->span[s]);
  const Probe pr = grp_locate(f, seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs)));
  uint32_t lr, rel, bit, qid = 0;
  {
    const QuadLane ql = quad_lane();
    const uint32_t pbytes = quad_piece_bytes(ql.sub);
    uint4 pc[4];
    pc[0] = quad_load<0>(f.buckets, pr.b, pbytes);
    pc[1] = quad_load<1>(f.buckets, pr.b, pbytes);
    pc[2] = quad_load<2>(f.buckets, pr.b, pbytes);
    pc[3] = quad_load<3>(f.buckets, pr.b, pbytes);
    const QuadAnswer mine = quad_decode(pc, pr.off, ql);
    lr = mine.lr;
    rel = mine.rel;
    bit = mine.bit;
    qid = mine.id;
  }
  const uint64_t rank = f.super[pr.b >> GRP_SUPER_SHIFT] + rel + lr;
  const bool valid = live && rank < f.pop && bit; // see k_insert
  const uint32_t idx = gunit * THREADS + threadIdx.x;
  const uint64_t home = ((rank + 1) * 0x9E3779B97F4A7C15ULL) >> 20 & b.cap_mask;
  bool claimed = false;
  uint32_t count0 = 0;
  uint32_t* idp = nullptr;
  uint32_t id0 = 0;
  // what a slot that is no record holds (word >> 26 == 0): 0 no frame, 1 no set bit, owner + 2: the rank
  // belongs to record `owner` (a duplicate inside one (read, block), or a touch chained to it) — the
  // verify pass (grp_verify.inc) finds out through it whether this probe's rank has a second toucher
  uint32_t why = !live ? 0u : 1u;
  if (valid) {
    unsigned long long* cwp = grp_cw_ptr(f, pr.b, lr, rank); // the insert line of the bucket's unit: the same 128-byte block as the header just read
    // The kernel pays per memory REQUEST of a lane, whether it hits the L2 or not (tools/gather_bench.hip mode 50,
    // profiles/r05_collect_matrix.txt: header + count word + CAS + ID read + ID write 13.4 G records/s; without the load
    // of the count word 15.0; with the ID read issued in front of the CAS as well 16.3; the ID by atomicExch instead
    // of load + store 12.4).  So the ID slot is read first — the owner's touch needs it anyway — and it tells whether
    // the count word has to be loaded: a rank that holds no ID has never been inserted (the first touch of a rank
    // always writes: c = 1), its word is 0 and the compare-and-swap starts from that; a word that is not what was
    // guessed comes back with the failed attempt.  (Starting EVERY rank from 0 lost 20 %: on a human-scale path
    // half of the touched ranks have been touched before — 4^16 spaced k-mers against 3 G bases per path.)
    idp = (lr < GRP_BUCKET_IDS) ? &reinterpret_cast<uint32_t*>(f.buckets)[grp_id_loc(pr.b, lr)] : nullptr;
    id0 = idp ? qid : 1u; // only the claim's winner uses it (and only the winner writes the slot)
    unsigned long long cur = (id0 == 0u) ? 0ull : __hip_atomic_load(cwp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
      if (grp_claim_epoch(cur) == b.epoch) { // a rank of this batch already: whose
        const uint32_t owner = grp_claim_record(cur);
        const uint32_t owner_unit = owner / (hn * THREADS);
        why = owner + 2u;
        // the same unit is the same (read, block): one dedup scope, one touch
        if (owner_unit < blk_unit0 || owner_unit >= blk_unit1) {
          // (one atomic per wave and counter, not per lane.  Measured on the repeat-rich genome, where a third of a batch's
          // records are chained touches: no difference — the collect pass there is 4 x slower per record than on a uniform
          // genome with or without it, and with or without the search this replaced below; what is left is the ranks of
          // the repeat families themselves, the same few units asked for by many lanes at once; round 5,
          // tools/dev/r5_repeats_prof.sh)
          const uint32_t at = wave_counter_take(&b.counters[1]);
          if (at < b.ovf_cap) {
            b.ovf_jb[at] = jb;
            const uint32_t before = atomicExch(&b.rec_chain[owner], at);
            b.ovf_next[at] = before;
            if (before == BATCH_NONE) { // the owner's first chained touch: k_batch_apply's work list (one entry per such record; never more than chain entries)
              b.chained[wave_counter_take(&b.counters[0])] = owner;
            }
          }
        }
        break;
      }
      // the claim and the owner's touch of the count in one word: c = ++count
      count0 = grp_cnt(cur);
      const unsigned long long prev = atomicCAS(cwp, cur, grp_cnt_with(grp_claim_word(idx, b.epoch, 0u), count0 + 1u));
      if (prev == cur) {
        claimed = true;
        break;
      }
      cur = prev;
    }
  }
  b.rec_key[idx] = claimed ? (((unsigned long long)(rank + 1) << 26) | jb) : (unsigned long long)why;
  if (claimed) {
    // the owner's touch, as if it were the rank's only one (k_batch_apply replays the ranks
    // where it was not): c = ++count; if (uint32(rank ^ id) % c == c - 1) the ID is written
    const unsigned long long loc = grp_id_loc(pr.b, lr);
    uint32_t* p = idp;
    const uint32_t cur = p ? id0 : grp_ovf_get(f, rank);
    const uint32_t cnt = count0 + 1u;
    const uint32_t id = batch_block_id(b, jb);
    const bool wrote = (uint32_t)(rank ^ (uint64_t)id) % cnt == cnt - 1u;
    if (wrote && cur != 0u) {
      atomicOr(&b.bits[home >> 5], 1u << (home & 31u));
    }
    if (wrote) {
      const uint32_t nv = (cur > 0x80000000u) ? (id | 0x80000000u) : id;
      if (p) {
        *p = nv;
      } else {
        grp_ovf_put(f, rank, nv);
      }
    }
    b.rec_loc[idx] = loc;
    b.rec_old[idx] = ((unsigned long long)(wrote ? 1u : 0u) << 63) | ((unsigned long long)count0 << 32) | cur;
  }
}



// the next touch of a rank, in the reference's order: the smallest (read, block) above `last`
// among the owner's own and the record's chain (the same (read, block) may be chained more
// than once: one dedup scope, one touch)
__device__ inline uint32_t
batch_next_touch(const DevBatch& b, uint32_t chain, uint32_t own_jb, uint32_t last)
{
  uint32_t best = BATCH_NONE;
  if (last == BATCH_NONE || own_jb > last) {
    best = own_jb;
  }
  for (uint32_t e = chain; e != BATCH_NONE; e = b.ovf_next[e]) {
    const uint32_t jb = b.ovf_jb[e];
    if ((last == BATCH_NONE || jb > last) && jb < best) {
      best = jb;
    }
  }
  return best;
}

__device__ inline void
batch_log(const DevBatch& b, uint64_t rank, uint32_t old, uint32_t writer)
{
  const unsigned long long key = rank + 1;
  uint64_t slot = (key * 0x9E3779B97F4A7C15ULL) >> 18 & b.log_mask;
  for (;;) {
    unsigned long long k = b.log_keys[slot];
    if (k == 0) {
      k = atomicCAS(&b.log_keys[slot], 0ull, key);
      if (k == 0) {
        k = key;
      }
    }
    if (k == key) {
      break;
    }
    slot = (slot + 1) & b.log_mask;
  }
  const uint32_t e = atomicAdd(&b.counters[2], 1u);
  if (e >= b.log_cap) {
    atomicOr(&b.counters[3], 2u);
    return;
  }
  b.log_old[e] = old;
  b.log_writer[e] = writer;
  b.log_slot[e] = (uint32_t)slot;
  b.log_next[e] = atomicExch(&b.log_head[slot], e); // one lane per rank: the chain is pushed in writer order
}

// second pass.  A rank without a chain: its only touch has been applied by the owner, the
// record holds what was there.  A rank with a chain: back to what the owner found, then the
// touches in the reference's order — c = ++count; if (uint32(rank ^ id)
// % c == c - 1) the ID is written (MIBFConstructSupport.hpp:274-282, setData
// MIBloomFilter.hpp:593-602) — every write logged.
__global__ void __launch_bounds__(THREADS)
k_batch_apply(DevFilter f, DevBatch b)
{
  // more touches than the chains hold: the host is told (counters[1]) and takes the batch back
  // (the owners' touches are undone from the records, the ranks with a chain stay as the owners
  // left them until then: nothing may be queried in between)
  // (round 5: over the records that OWN a chain — the collect pass lists them — instead of over all records: the scan of
  // ~11 M records per batch for the few hundred that matter was a quarter of the batches' insert time)
  const bool broken = b.counters[1] > b.ovf_cap;
  const uint32_t n_chained = broken ? 0u : b.counters[0];
  for (uint32_t q = blockIdx.x * THREADS + threadIdx.x; q < n_chained; q += gridDim.x * THREADS) {
    const uint32_t i = b.chained[q];
    const unsigned long long word = b.rec_key[i];
    const uint32_t chain = b.rec_chain[i];
    if ((word >> 26) == 0ull || chain == BATCH_NONE) {
      continue; // (cannot be: a chain hangs on a record)
    }
    const unsigned long long old = b.rec_old[i];
    const uint64_t rank = (word >> 26) - 1;
    const uint32_t own_jb = (uint32_t)(word & BATCH_LOW26);
    const unsigned long long loc = b.rec_loc[i];
    uint32_t* p = (loc & (GRP_UNIT_DW - 1u)) ? &reinterpret_cast<uint32_t*>(f.buckets)[loc] : nullptr;
    // what the rank held in front of the batch: in the record if its owner wrote, else still in the slot
    uint32_t cur = (old >> 63) ? (uint32_t)old : (p ? *p : grp_ovf_get(f, rank));
    {
      const uint64_t home = ((rank + 1) * 0x9E3779B97F4A7C15ULL) >> 20 & b.cap_mask;
      atomicOr(&b.bits[home >> 5], 1u << (home & 31u));
    }
    uint32_t count = (uint32_t)(old >> 32) & 0x7FFFFFFFu;
    uint32_t last = BATCH_NONE;
    for (;;) {
      const uint32_t jb = batch_next_touch(b, chain, own_jb, last);
      if (jb == BATCH_NONE) {
        break;
      }
      last = jb;
      ++count;
      const uint32_t id = batch_block_id(b, jb);
      if ((uint32_t)(rank ^ (uint64_t)id) % count == count - 1u) {
        batch_log(b, rank, cur, b.ins[(size_t)(jb >> 8) * 6] - b.first_read);
        cur = (cur > 0x80000000u) ? (id | 0x80000000u) : id;
      }
    }
    unsigned long long* cwp = grp_cw_ptr_loc(f, loc, rank);
    *cwp = grp_cnt_with(*cwp, count); // (the claim stays: the views look the record up through it)
    if (p) {
      *p = cur;
    } else {
      grp_ovf_put(f, rank, cur);
    }
  }
}

// the chains overflowed: every owner's touch is taken back from its record
__global__ void __launch_bounds__(THREADS)
k_batch_revert(DevFilter f, DevBatch b)
{
  for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < b.n_rec; i += gridDim.x * THREADS) {
    const unsigned long long word = b.rec_key[i];
    if ((word >> 26) == 0ull) {
      continue;
    }
    const unsigned long long old = b.rec_old[i];
    const unsigned long long loc = b.rec_loc[i];
    const uint64_t rank = (word >> 26) - 1;
    *grp_cw_ptr_loc(f, loc, rank) = (unsigned long long)((uint32_t)(old >> 32) & 0x7FFFFFFFu); // (no claim left: the batch is over)
    if (!(old >> 63)) {
      continue; // the owner did not write: the slot is as it was
    }
    if (loc & (GRP_UNIT_DW - 1u)) {
      reinterpret_cast<uint32_t*>(f.buckets)[loc] = (uint32_t)old;
    } else {
      grp_ovf_put(f, rank, (uint32_t)old);
    }
  }
}

// undo: the inserts [from_ins, n_ins) of the batch are taken back.  A rank with one touch goes
// back to its record.  A rank with a chain: the count goes back by the number of their touches;
// an ID written by one of them (>= floor_id, the first ID insert from_ins allocated) goes back to
// what read from_read saw, the old value of the first logged write by a read >= from_read.
__global__ void __launch_bounds__(THREADS)
k_batch_undo(DevFilter f, DevBatch b, DevBatchView bv, uint32_t from_ins, uint32_t from_read, uint32_t floor_id)
{
  for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < b.n_rec; i += gridDim.x * THREADS) {
    const unsigned long long word = b.rec_key[i];
    if ((word >> 26) == 0ull) {
      continue;
    }
    const uint32_t chain = b.rec_chain[i];
    const uint32_t own_jb = (uint32_t)(word & BATCH_LOW26);
    const uint64_t rank = (word >> 26) - 1;
    if (chain == BATCH_NONE) {
      // one touch, its owner's: the record holds what was there
      if ((own_jb >> 8) >= from_ins) {
        const unsigned long long old = b.rec_old[i];
        const unsigned long long loc = b.rec_loc[i];
        *grp_cw_ptr_loc(f, loc, rank) = (unsigned long long)((uint32_t)(old >> 32) & 0x7FFFFFFFu); // (the claim goes too: nobody looks this rank up any more, the batch ends behind this kernel)
        if (old >> 63) {
          if (loc & (GRP_UNIT_DW - 1u)) {
            reinterpret_cast<uint32_t*>(f.buckets)[loc] = (uint32_t)old;
          } else {
            grp_ovf_put(f, rank, (uint32_t)old);
          }
        }
      }
      continue;
    }
    uint32_t touches = 0, last = BATCH_NONE;
    for (;;) {
      const uint32_t jb = batch_next_touch(b, chain, own_jb, last);
      if (jb == BATCH_NONE) {
        break;
      }
      last = jb;
      touches += (jb >> 8) >= from_ins ? 1u : 0u;
    }
    if (touches == 0) {
      continue;
    }
    const unsigned long long loc = b.rec_loc[i];
    {
      unsigned long long* cwp = grp_cw_ptr_loc(f, loc, rank);
      const unsigned long long w = *cwp;
      *cwp = grp_cnt_with(w, grp_cnt(w) - touches); // (the claim stays: batch_view below goes through it)
    }
    uint32_t* p = (loc & (GRP_UNIT_DW - 1u)) ? &reinterpret_cast<uint32_t*>(f.buckets)[loc] : nullptr;
    const uint32_t cur = p ? *p : grp_ovf_get(f, rank);
    if ((cur & 0x7FFFFFFFu) >= floor_id) {
      const uint32_t dw = (uint32_t)(loc & (GRP_UNIT_DW - 1u));
      const uint32_t orig = batch_view(bv, rank, (loc / GRP_UNIT_DW) * 64ull + (dw ? dw - 3u : 63u), from_read, cur, (cur & 0x7FFFFFFFu) == floor_id);
      if (p) {
        *p = orig;
      } else {
        grp_ovf_put(f, rank, orig);
      }
    }
  }
}

// Everything a batch leaves behind, in one launch (round 5: these were a kernel and four fills / batch, each with its
// own gap on the stream): the log table (only the slots that were used), the bits of the hash slots, the chain heads
// of the batch's records, and the counters of the NEXT batch (the other set: this batch's are still being read here).
__global__ void __launch_bounds__(THREADS)
k_batch_clear(DevBatch b, uint32_t* __restrict__ next_counters, uint32_t bits_u4)
{
  const uint32_t nl = min(b.counters[2], b.log_cap);
  const uint32_t tid = blockIdx.x * THREADS + threadIdx.x, nthr = gridDim.x * THREADS;
  for (uint32_t e = tid; e < nl; e += nthr) {
    const uint32_t slot = b.log_slot[e];
    b.log_keys[slot] = 0ull;
    b.log_head[slot] = BATCH_NONE;
  }
  uint4* bits4 = reinterpret_cast<uint4*>(b.bits);
  for (uint32_t i = tid; i < bits_u4; i += nthr) {
    bits4[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  uint4* chain4 = reinterpret_cast<uint4*>(b.rec_chain);
  const uint32_t n4 = (b.n_rec + 3u) / 4u; // (the array holds n_rec + n_rec / 4 + 1024 entries)
  for (uint32_t i = tid; i < n4; i += nthr) {
    chain4[i] = make_uint4(BATCH_NONE, BATCH_NONE, BATCH_NONE, BATCH_NONE);
  }
  if (tid < 4u) {
    next_counters[tid] = 0u;
  }
}

// the epochs have wrapped: every claim is dropped, the counts stay.  `units`: the filter as 64-bit words, the count
// words are words 8..15 of every 16; then the far table's words (stride 2, offset 1: its odd words)
__global__ void __launch_bounds__(THREADS)
k_batch_sweep(unsigned long long* __restrict__ cw, uint64_t n, uint32_t group, uint32_t skip)
{
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS) {
    if ((i & (group - 1u)) < skip) {
      continue;
    }
    const unsigned long long w = cw[i];
    if (w > GRP_CNT_MASK) {
      cw[i] = w & GRP_CNT_MASK;
    }
  }
}

// ---- overlaps inside a window, known BEFORE it is queried (round 4; grp_window_overlap) ------------
// A batch is the serial loop unless one of its reads decides differently behind the inserts of the reads in front
// of it — which happens when it OVERLAPS a read of its own window that inserts.  Then the rest of the batch is taken
// back: 14 - 19 % of the batches, ~10 % of the work of the insert-heavy regime.  Hashing is free beside the
// memory-bound kernels, so a pre-pass hashes the reads of the window that is about to be queried under seed 0 only,
// keeps one frame in 32 (the canonical hash: the same on either strand) and names the FIRST read that shares more
// than a handful of those with a read in front of it; the host ends its window there.  (Found the hard way: naming
// such reads behind the window's query instead, and cutting the batch in front of them, throws the rest of the
// window's first query away and loses — profiles/r04_overlap_hints_measured.txt.)  A hint: exactness never
// depends on it, the second decisions still confirm every batch.
constexpr uint32_t OVL_CAP_T = 128; // samples kept per tile (31 expected at 1000 frames; 62 with the developer hook's one in 16)

__device__ inline bool
ovl_sampled(uint64_t hv, uint32_t shift)
{
  return ((hv * 0x9E3779B97F4A7C15ULL) >> shift) == 0ull; // shift 59: one frame in 32
}

__device__ inline uint32_t
ovl_key(unsigned long long hv)
{
  const uint32_t k = (uint32_t)((hv * 0xD6E8FEB86659FD93ULL) >> 32);
  return k ? k : 1u;
}

// one workgroup per tile of the window: the sampled frames' hashes under seed 0
template<int WT>
__global__ void __launch_bounds__(THREADS)
k_ovl_sample(DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint64_t tile_begin, unsigned long long* __restrict__ samples, uint32_t* __restrict__ n_out, uint32_t shift)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + sd->h * sd->wmax * 4u);
  __shared__ uint32_t sN;
  const uint64_t t = tile_begin + blockIdx.x;
  const uint32_t r = rd.tile_read[t];
  const uint32_t ti = (uint32_t)(t - rd.tile0[r]);
  const uint32_t len = rd.len[r];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, ti);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;
  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, start, Lp);
  if (threadIdx.x == 0) {
    sN = 0;
  }
  __syncthreads();
  for (uint32_t fr = threadIdx.x; fr < frames; fr += THREADS) {
    const uint64_t hv = seed_hash_t<WT>(sTab, sd, 0, window_at(sBases, boff + fr));
    if (ovl_sampled(hv, shift)) {
      const uint32_t at = atomicAdd(&sN, 1u);
      if (at < OVL_CAP_T) {
        samples[(uint64_t)blockIdx.x * OVL_CAP_T + at] = hv;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    n_out[blockIdx.x] = min(sN, OVL_CAP_T);
  }
}

// one workgroup per read of the window: its samples into the table (open addressing, key << 32 | read: the smallest read wins)
__global__ void __launch_bounds__(THREADS)
k_ovl_mark(DevReads rd, uint32_t first, uint64_t tile_begin, const unsigned long long* __restrict__ samples, const uint32_t* __restrict__ n_in, unsigned long long* __restrict__ tab, uint32_t tab_mask)
{
  const uint32_t j = blockIdx.x;
  const uint64_t t_read = rd.tile0[first + j] - tile_begin;
  const uint32_t nt = (uint32_t)(rd.tile0[first + j + 1] - rd.tile0[first + j]);
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t n = n_in[t_read + t];
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) {
      const unsigned long long hv = samples[(t_read + t) * OVL_CAP_T + i];
      const uint32_t key = ovl_key(hv);
      const unsigned long long word = ((unsigned long long)key << 32) | j;
      uint32_t slot = (uint32_t)(hv >> 20) & tab_mask;
      for (uint32_t step = 0; step < 64u; ++step) { // (a full neighbourhood loses the sample: a hint)
        unsigned long long cur = tab[slot];
        if (cur == ~0ull) {
          cur = atomicCAS(&tab[slot], ~0ull, word);
          if (cur == ~0ull) {
            break;
          }
        }
        if ((uint32_t)(cur >> 32) == key) {
          atomicMin(&tab[slot], word);
          break;
        }
        slot = (slot + 1u) & tab_mask;
      }
    }
  }
}

// one workgroup per read j: its samples attributed to their owners (the first read of the range that holds them);
// prev[j] = the CLOSEST read in front of j that owns at least `threshold` of them, OVL_NONE if there is none
constexpr uint32_t OVL_NONE = 0xFFFFFFFFu;
constexpr uint32_t OVL_OWNERS = 256; // distinct owners counted per read (the rest is dropped: a hint)

__global__ void __launch_bounds__(THREADS)
k_ovl_count(DevReads rd, uint32_t first, uint64_t tile_begin, const unsigned long long* __restrict__ samples, const uint32_t* __restrict__ n_in, const unsigned long long* __restrict__ tab, uint32_t tab_mask, uint32_t threshold,
            uint32_t* __restrict__ prev)
{
  __shared__ uint32_t sOwner[OVL_OWNERS], sCount[OVL_OWNERS], sBest;
  const uint32_t j = blockIdx.x;
  for (uint32_t i = threadIdx.x; i < OVL_OWNERS; i += THREADS) {
    sOwner[i] = OVL_NONE;
    sCount[i] = 0;
  }
  if (threadIdx.x == 0) {
    sBest = OVL_NONE;
  }
  __syncthreads();
  const uint64_t t_read = rd.tile0[first + j] - tile_begin;
  const uint32_t nt = (uint32_t)(rd.tile0[first + j + 1] - rd.tile0[first + j]);
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t n = n_in[t_read + t];
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) {
      const unsigned long long hv = samples[(t_read + t) * OVL_CAP_T + i];
      const uint32_t key = ovl_key(hv);
      uint32_t slot = (uint32_t)(hv >> 20) & tab_mask;
      uint32_t owner = OVL_NONE;
      for (uint32_t step = 0; step < 64u; ++step) {
        const unsigned long long cur = tab[slot];
        if (cur == ~0ull) {
          break;
        }
        if ((uint32_t)(cur >> 32) == key) {
          owner = (uint32_t)cur;
          break;
        }
        slot = (slot + 1u) & tab_mask;
      }
      if (owner < j) {
        uint32_t o = (owner * 2654435761u) >> 24; // 8 bits
        for (uint32_t step = 0; step < OVL_OWNERS; ++step) {
          const uint32_t cur = atomicCAS(&sOwner[o], OVL_NONE, owner);
          if (cur == OVL_NONE || cur == owner) {
            atomicAdd(&sCount[o], 1u);
            break;
          }
          o = (o + 1u) & (OVL_OWNERS - 1u);
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < OVL_OWNERS; i += THREADS) {
    if (sOwner[i] != OVL_NONE && sCount[i] >= threshold) {
      // the closest one in front of j: the largest index (OVL_NONE is the largest value: start from a max over valid owners)
      atomicMin(&sBest, j - 1u - sOwner[i]); // distance - 1, so that the smallest wins
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    prev[j] = (sBest == OVL_NONE) ? OVL_NONE : j - 1u - sBest;
  }
}

DevBatch
batch_dev(const grp_ctx* c)
{
  const BatchRun& r = c->batch;
  DevBatch b;
  b.epoch = r.epoch;
  b.cap_mask = r.cur_cap - 1;
  b.counters = r.d_counters + 4u * r.ctr_set;
  b.ins = r.d_ins;
  b.n_ins = r.n_ins;
  b.block_tiles = r.block_tiles;
  b.n_rec = (uint32_t)r.n_rec;
  b.rec_key = r.d_rec_key;
  b.rec_loc = r.d_rec_loc;
  b.rec_old = r.d_rec_old;
  b.rec_chain = r.d_rec_chain;
  b.ovf_next = r.d_ovf_next;
  b.ovf_jb = r.d_ovf_jb;
  b.chained = r.d_chained;
  b.ovf_cap = (uint32_t)r.ovf_cap;
  b.log_keys = r.d_log_keys;
  b.log_head = r.d_log_head;
  b.bits = r.d_log_bits;
  b.log_old = r.d_log_old;
  b.log_writer = r.d_log_writer;
  b.log_next = r.d_log_next;
  b.log_slot = r.d_log_slot;
  b.log_mask = r.cur_cap - 1;
  b.log_cap = (uint32_t)r.log_cap;
  b.first_read = r.first_read;
  return b;
}

DevBatchView
batch_view_of(const grp_ctx* c)
{
  const BatchRun& br = c->batch;
  DevBatchView bv;
  bv.first = br.first_read;
  bv.units = reinterpret_cast<const unsigned long long*>(c->f.buckets);
  bv.far = c->f.far;
  bv.far_mask = c->f.far_mask;
  bv.epoch = br.epoch;
  bv.bits_mask = br.cur_cap - 1;
  bv.bits = br.d_log_bits;
  bv.rec_old = br.d_rec_old;
  bv.rec_chain = br.d_rec_chain;
  bv.rec_key = br.d_rec_key;
  bv.ins = br.d_ins;
  bv.log_keys = br.d_log_keys;
  bv.log_head = br.d_log_head;
  bv.log_old = br.d_log_old;
  bv.log_writer = br.d_log_writer;
  bv.log_next = br.d_log_next;
  bv.log_mask = br.cur_cap - 1;
  return bv;
}

int
batch_release(grp_ctx* c)
{
  BatchRun& r = c->batch;
  if (!r.active) {
    return GRP_OK;
  }
  const DevBatch b = batch_dev(c);
  k_batch_clear<<<dim3(512), dim3(THREADS), 0, c->stream>>>(b, r.d_counters + 4u * (r.ctr_set ^ 1u), (uint32_t)(std::max<uint64_t>(r.cur_cap / 8, 64) / 16));
  HIP_TRY(c, hipGetLastError());
  r.ctr_set ^= 1u;
  r.active = false; // (the claims in the count words need no clearing: the next batch has another epoch)
  return GRP_OK;
}

} // namespace

extern "C" {

int
grp_batch_insert_reads(grp_ctx* c, const grp_reads* r, const grp_batch_insert* ins, uint32_t n_ins, uint32_t block_tiles, uint32_t first_read)
{
  if (!c || !r || r->ctx != c || !ins || n_ins == 0 || block_tiles == 0 || n_ins > BATCH_MAX_INS) {
    return set_err(c, GRP_ERR_INVALID, "grp_batch_insert_reads: bad argument");
  }
  if (!c->finalized) {
    return set_err(c, GRP_ERR_STATE, "grp_batch_insert_reads before grp_finalize");
  }
  BatchRun& br = c->batch;
  if (br.active) {
    return set_err(c, GRP_ERR_STATE, "grp_batch_insert_reads: the previous batch has not been ended");
  }
  if (c->f.pop >= (1ull << 38) - 1) {
    return set_err(c, GRP_ERR_INVALID, "grp_batch_insert_reads: more than 2^38 set bits (a table word holds rank + 1 in 38 bits)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t parts = tile_parts(c);
  std::vector<uint32_t>& h_ins = br.h_ins;
  h_ins.resize((size_t)n_ins * 6);
  uint64_t units = 0;
  for (uint32_t j = 0; j < n_ins; ++j) {
    const grp_batch_insert& e = ins[j];
    if (e.read >= r->n_reads || e.read < first_read || (j && e.read <= ins[j - 1].read) || e.id_offset > 1) {
      return set_err(c, GRP_ERR_INVALID, "grp_batch_insert_reads: inserts must name reads of the batch in ascending order");
    }
    const uint64_t ntile = r->tile0[e.read + 1] - r->tile0[e.read];
    if (e.tile_start >= e.tile_end || e.tile_end > ntile) {
      return set_err(c, GRP_ERR_INVALID, "grp_batch_insert_reads: tiles [%u,%u) outside read %u's %llu tiles", e.tile_start, e.tile_end, e.read, (unsigned long long)ntile);
    }
    if ((e.tile_end - e.tile_start + block_tiles - 1) / block_tiles > BATCH_MAX_BLOCKS) {
      return set_err(c, GRP_ERR_INVALID, "grp_batch_insert_reads: read %u has more than %u ID blocks", e.read, BATCH_MAX_BLOCKS);
    }
    uint32_t* d = &h_ins[(size_t)j * 6];
    d[0] = e.read;
    d[1] = e.tile_start;
    d[2] = e.tile_end;
    d[3] = e.first_id;
    d[4] = e.id_offset;
    d[5] = (uint32_t)units;
    units += (uint64_t)(e.tile_end - e.tile_start) * parts;
  }
  const uint64_t n_rec = units * c->params.h * THREADS;
  if (n_rec + 2 >= BATCH_MAX_REC) { // (owner + 2 must fit the low 26 bits of a slot that is no record)
    return set_err(c, GRP_ERR_NOMEM, "grp_batch_insert_reads: %llu (frame, seed) records, a batch holds 2^26: nothing was inserted, use a smaller batch", (unsigned long long)n_rec);
  }
  // tables (grown, never shrunk; every batch leaves them clean)
  const uint64_t want = std::max<uint64_t>(next_pow2_64(n_rec + n_rec / 2), 1u << 16);
  if (want > br.tab_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    clear_all(br.d_log_keys, br.d_log_head, br.d_log_bits);
    br.tab_cap = 0;
    HIP_TRY(c, br.d_log_keys.reset(want));
    HIP_TRY(c, br.d_log_head.reset(want));
    HIP_TRY(c, br.d_log_bits.reset(std::max<uint64_t>(want / 8, 64) / 4)); // (in words)
    HIP_TRY(c, hipMemsetAsync(br.d_log_keys, 0, want * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(br.d_log_head, 0xFF, want * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(br.d_log_bits, 0, std::max<uint64_t>(want / 8, 64), c->stream));
    br.tab_cap = want;
  }
  if (!br.d_counters) {
    HIP_TRY(c, br.d_counters.reset(8));
    HIP_TRY(c, hipMemsetAsync(br.d_counters, 0, 8 * sizeof(uint32_t), c->stream));
    HIP_TRY(c, br.h_counters.reset(4, hipHostMallocDefault));
    memset(br.h_counters, 0, 4 * sizeof(uint32_t));
    br.ctr_set = 0;
  }
  if (h_ins.size() > br.h_ins_stage.cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, br.h_ins_stage.reset(2 * h_ins.size() + 6 * 1024, hipHostMallocDefault));
  }
  int rc = ensure_dev(c, br.d_ins, (uint64_t)n_ins * 6);
  if (rc == GRP_OK && n_rec > br.rec_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    clear_all(br.d_rec_key, br.d_rec_loc, br.d_rec_old, br.d_rec_chain, br.d_ovf_next, br.d_ovf_jb, br.d_chained, br.d_log_old, br.d_log_writer, br.d_log_next, br.d_log_slot);
    br.rec_cap = br.log_cap = br.ovf_cap = 0;
    const uint64_t n = n_rec + n_rec / 4 + 1024;
    HIP_TRY(c, br.d_rec_key.reset(n));
    HIP_TRY(c, br.d_rec_loc.reset(n));
    HIP_TRY(c, br.d_rec_old.reset(n));
    HIP_TRY(c, br.d_rec_chain.reset(n));
    HIP_TRY(c, hipMemsetAsync(br.d_rec_chain, 0xFF, n * sizeof(uint32_t), c->stream)); // every batch leaves it clean (k_batch_clear)
    // touches of a rank by a second (read, block): ~ranks^2 / (2 pop) for independent reads,
    // more where reads of the batch overlap (then the batch is taken back anyway)
    const long ovf_test = c->sw.batch_ovf_cap; // GRP_BATCH_OVF_CAP, tests: a tiny chain store, so that batches are refused on the device
    const uint64_t no = ovf_test > 0 ? (uint64_t)ovf_test : n / 4 + 65536;
    HIP_TRY(c, br.d_ovf_next.reset(no));
    HIP_TRY(c, br.d_ovf_jb.reset(no));
    HIP_TRY(c, br.d_chained.reset(no));
    const uint64_t nl = n + no; // one entry per write at most
    HIP_TRY(c, br.d_log_old.reset(nl));
    HIP_TRY(c, br.d_log_writer.reset(nl));
    HIP_TRY(c, br.d_log_next.reset(nl));
    HIP_TRY(c, br.d_log_slot.reset(nl));
    br.rec_cap = n;
    br.ovf_cap = no;
    br.log_cap = nl;
  }
  if (rc != GRP_OK) {
    return rc;
  }
  br.n_ins = n_ins;
  br.block_tiles = block_tiles;
  br.n_units = units;
  br.n_rec = n_rec;
  br.cur_cap = want; // this batch uses the first `want` slots of the tables
  br.first_read = first_read;
  if (br.epoch >= c->sw.batch_epochs) {
    // 1023 batches since the claims were last dropped: once over the count words (the insert lines of all units)
    k_batch_sweep<<<dim3(16384), dim3(THREADS), 0, c->stream>>>(reinterpret_cast<unsigned long long*>(c->f.buckets), c->f.n_buckets * GRP_UNIT_QW, GRP_UNIT_QW, 8u);
    k_batch_sweep<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(reinterpret_cast<unsigned long long*>(c->f.far), (c->f.far_mask + 1) * 2, 2u, 1u);
    HIP_TRY(c, hipGetLastError());
    br.epoch = 0;
    ++c->n_batch_sweeps;
  }
  ++br.epoch;
  memcpy(br.h_ins_stage, h_ins.data(), h_ins.size() * sizeof(uint32_t)); // (the previous batch's upload is long through: its decisions were waited for)
  HIP_TRY(c, hipMemcpyAsync(br.d_ins, br.h_ins_stage, h_ins.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  br.active = true;
  const DevBatch b = batch_dev(c);
  const size_t lds = tab_bytes(c) + bases_bytes(c->params.tile + c->params.k + c->params.h);
  {
    Timer t(c, GRP_K_BATCH, n_rec);
    const uint64_t gunits = units * c->params.h;
    for (uint64_t u0 = 0; u0 < gunits; u0 += MAX_GRID_WGS) {
      const uint32_t nb = (uint32_t)std::min<uint64_t>(gunits - u0, MAX_GRID_WGS);
      DISPATCH_HW(c, (k_batch_collect<HH, WW><<<dim3(nb), dim3(THREADS), lds, c->stream>>>(c->f, r->dev, c->d_seeds, c->params.tile, b, (uint32_t)u0)));
    }
    HIP_TRY(c, hipGetLastError());
    // k_batch_apply does nothing when the chains overflowed (counters[1] > ovf_cap): the caller
    // learns it from grp_batch_classify / grp_batch_end (batch_check takes the owners' touches back)
    // (grid from a host-known bound on the chained records — the loop is grid-stride and stops at counters[0], so workgroups
    // beyond the list cost nothing on a uniform genome; on a repeat-rich one a third of a batch's records own a chain and
    // 256 workgroups were one per CU for a latency-bound chain walk, ADVICE r05)
    k_batch_apply<<<dim3((uint32_t)std::min<uint64_t>((std::min<uint64_t>(n_rec, br.ovf_cap) + THREADS - 1) / THREADS, 4096)), dim3(THREADS), 0, c->stream>>>(c->f, b);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(br.h_counters, br.d_counters + 4u * br.ctr_set, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  }
  return GRP_OK;
}

// For every read j of [first, first + count): prev_out[j] = the closest read in front of it in that range (index relative
// to first) that it overlaps — that owns at least `threshold` of j's sampled k-mers — or 0xFFFFFFFF; see "overlaps inside a
// window" above.  One call covers many windows (a window [s, e) of the range should end in front of the first j with
// prev_out[j] >= s).  Reads nothing of the filter; synchronous.
int
grp_window_overlap(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, uint32_t threshold, uint32_t* prev_out)
{
  if (!c || !r || r->ctx != c || (!prev_out && count) || (uint64_t)first + count > r->n_reads) {
    return set_err(c, GRP_ERR_INVALID, "grp_window_overlap: bad argument");
  }
  std::fill(prev_out, prev_out + count, OVL_NONE);
  const uint64_t t0 = r->tile0[first];
  const uint64_t nt = r->tile0[first + count] - t0;
  if (count < 2 || nt == 0 || nt > (1u << 19) || threshold == 0) {
    return GRP_OK; // nothing to compare / a range too large for one call: no overlap named
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_ctx::OverlapBuf& ob = c->ovl;
  const uint64_t tab = std::max<uint64_t>(next_pow2_64(nt * 128), 1u << 16); // ~62 samples per tile: load < 1/2
  if (nt * OVL_CAP_T > ob.d_samples.cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, ob.d_samples.reset((nt + nt / 4 + 64) * OVL_CAP_T));
  }
  int rc = ensure_dev(c, ob.d_n, nt);
  if (rc == GRP_OK) {
    rc = ensure_dev(c, ob.d_tab, tab);
  }
  if (rc == GRP_OK) {
    rc = ensure_dev(c, ob.d_prev, count);
  }
  if (rc != GRP_OK) {
    return rc;
  }
  HIP_TRY(c, hipMemsetAsync(ob.d_tab, 0xFF, tab * sizeof(unsigned long long), c->stream));
  // one frame in 32 (round 5; one in 16 before): with the threshold halved the same overlaps are named and the pass's table
  // work is half (tools/dev/r5_ovl_sampling.sh: silver pass over C2's reads 138.2 -> 140.3 k reads/s, repeat-rich genome 97.9 -> 99.9 k;
  // one in 64 with a threshold of 2 names unrelated reads)
  const uint32_t ovl_shift = c->sw.batch_overlap_shift; // GRP_BATCH_OVERLAP_SHIFT, developer hook (measurement): 60 = one sampled frame in 16, 59 = one in 32 ...
  const size_t lds = tab_bytes(c) + bases_bytes(c->params.tile + c->params.k + c->params.h);
  for (uint64_t b0 = 0; b0 < nt; b0 += MAX_GRID_WGS) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(nt - b0, MAX_GRID_WGS);
    DISPATCH_W(c, (k_ovl_sample<WW><<<dim3(nb), dim3(THREADS), lds, c->stream>>>(r->dev, c->d_seeds, c->params.tile, t0 + b0, ob.d_samples + b0 * OVL_CAP_T, ob.d_n + b0, ovl_shift)));
  }
  k_ovl_mark<<<dim3(count), dim3(THREADS), 0, c->stream>>>(r->dev, first, t0, ob.d_samples, ob.d_n, ob.d_tab, (uint32_t)(tab - 1));
  k_ovl_count<<<dim3(count), dim3(THREADS), 0, c->stream>>>(r->dev, first, t0, ob.d_samples, ob.d_n, ob.d_tab, (uint32_t)(tab - 1), threshold, ob.d_prev);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(prev_out, ob.d_prev, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ++c->n_overlap_calls;
  return GRP_OK;
}

// the batch's counters, once its kernels are through: chains overflowed -> nothing was applied
static int
batch_check(grp_ctx* c)
{
  BatchRun& br = c->batch;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (br.h_counters[1] > br.ovf_cap) {
    const DevBatch b = batch_dev(c);
    k_batch_revert<<<dim3((uint32_t)std::min<uint64_t>((br.n_rec + THREADS - 1) / THREADS, 16384)), dim3(THREADS), 0, c->stream>>>(c->f, b);
    (void)batch_release(c);
    return set_err(c, GRP_ERR_NOMEM, "grp_batch: %u ranks are touched by several ID blocks of the batch (limit %llu): nothing was inserted, use a smaller batch", br.h_counters[1], (unsigned long long)br.ovf_cap);
  }
  if (br.h_counters[3]) {
    return set_err(c, GRP_ERR_STATE, "grp_batch: the batch's log overflowed");
  }
  return GRP_OK;
}

int
grp_batch_classify(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const grp_decide_params* dp, const uint32_t* id_floor, grp_read_decision* out)
{
  if (!c || !r || r->ctx != c || !id_floor || !c->batch.active || first < c->batch.first_read) {
    return set_err(c, GRP_ERR_STATE, "grp_batch_classify: no batch on this window");
  }
  BatchRun& br = c->batch;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure_dev(c, br.d_floor, std::max<uint64_t>(count, 1));
  if (rc != GRP_OK) {
    return rc;
  }
  HIP_TRY(c, hipMemcpyAsync(br.d_floor, id_floor, (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  DevBatchView bv = batch_view_of(c);
  bv.floor = br.d_floor;
  bv.floor_first = first;
  bv.first = br.first_read;
  c->view = &bv;
  rc = grp_classify_reads(c, r, first, count, dp, out); // `id_floor` may be pageable: the call is synchronous
  c->view = nullptr;
  if (rc != GRP_OK) {
    return rc;
  }
  return batch_check(c);
}

int
grp_batch_undo(grp_ctx* c, uint32_t from_read, uint32_t id_floor)
{
  if (c) {
    c->carry.valid = false;
  }
  if (!c || !c->batch.active) {
    return set_err(c, GRP_ERR_STATE, "grp_batch_undo: no batch");
  }
  BatchRun& br = c->batch;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = batch_check(c);
  if (rc != GRP_OK) {
    return rc == GRP_ERR_NOMEM && !br.active ? GRP_OK : rc; // nothing had been applied
  }
  uint32_t from_ins = 0;
  while (from_ins < br.n_ins && br.h_ins[(size_t)from_ins * 6] < from_read) {
    ++from_ins;
  }
  if (from_ins < br.n_ins) {
    const DevBatch b = batch_dev(c);
    k_batch_undo<<<dim3((uint32_t)std::min<uint64_t>((br.n_rec + THREADS - 1) / THREADS, 16384)), dim3(THREADS), 0, c->stream>>>(c->f, b, batch_view_of(c), from_ins, from_read >= br.first_read ? from_read - br.first_read : 0u, id_floor);
    HIP_TRY(c, hipGetLastError());
  }
  return batch_release(c);
}

int
grp_batch_end(grp_ctx* c)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (!c->batch.active) {
    return GRP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = batch_check(c);
  if (rc != GRP_OK) {
    return rc;
  }
  return batch_release(c);
}

} // extern "C"
