// Device code of the engine: every kernel of the hot path (fill, rank build, query with
// its streaming form, decision, insert, inspection).  Included by grpath_hip.hip (same
// translation unit: uses the context types declared there and grp_device.h).
// ---------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------

// 64-bit window of 2-bit bases (32 bases) starting at base index `b` of the staged words
__device__ inline uint64_t
window_lo(const uint32_t* sBases, uint32_t b)
{
  uint32_t bit = b * 2u;
  uint32_t wi = bit >> 5;
  uint32_t sh = bit & 31u;
  uint64_t lo = (uint64_t)sBases[wi] | ((uint64_t)sBases[wi + 1] << 32);
  uint64_t w = lo >> sh;
  if (sh) {
    w |= (uint64_t)sBases[wi + 2] << (64u - sh);
  }
  return w;
}

// The window a hash is taken from: its first 32 bases, and where it lies — seeds whose span exceeds 32 bases
// (k + h - 1 up to 64; round 4, DevSeeds::wide) fetch the 32 bases behind them from there.  The default geometries
// (span <= 26) never do: the wide path costs them one wave-uniform branch per hash.  Spans beyond 64 (up to 256,
// DevSeeds::wide == 2) read every care position from the staged words themselves (seed_hash_long) and run in
// instantiations of their own (WT == GRP_WT_LONG), which nothing else launches.
struct Win
{
  uint64_t lo;
  const uint32_t* src;
  uint32_t b;
};

__device__ inline Win
window_at(const uint32_t* sBases, uint32_t b)
{
  return Win{ window_lo(sBases, b), sBases, b };
}

// hash of seed s on window w (closed form: XOR of per-position table entries,
// fwd + rev); tab is the LDS copy [s][i][b]
__device__ inline uint64_t
seed_hash(const ulonglong2* sTab, const DevSeeds* __restrict__ sd, uint32_t s, const Win& w)
{
  uint64_t fwd = 0, rev = 0;
  const uint32_t wt = sd->weight[s];
  const ulonglong2* t = sTab + (size_t)s * sd->wmax * 4u;
  if (sd->wide) {
    const uint64_t hi = window_lo(w.src, w.b + 32u); // bases 32 .. 63 of the window (the staging pads cover the read-ahead)
    for (uint32_t i = 0; i < wt; ++i) {
      const uint32_t sh = sd->shift[s][i];
      const uint32_t b = (uint32_t)((sh < 64u ? w.lo >> sh : hi >> (sh - 64u)) & 3u);
      const ulonglong2 e = t[i * 4u + b];
      fwd ^= e.x;
      rev ^= e.y;
    }
    return fwd + rev;
  }
  for (uint32_t i = 0; i < wt; ++i) {
    uint32_t b = (uint32_t)(w.lo >> sd->shift[s][i]) & 3u;
    ulonglong2 e = t[i * 4u + b];
    fwd ^= e.x;
    rev ^= e.y;
  }
  return fwd + rev;
}

// The long-span class of the kernels' WT parameter: seeds whose span exceeds 64 bases (k + h - 1 up to GRP_MAX_SPAN =
// 256).  The host launches these instantiations instead of the WT == 0 ones when DevSeeds::wide == 2; the forms of
// spans up to 64 keep their code.
constexpr int GRP_WT_LONG = -1;

// The seeds of a frame.  Every kernel that hashes a frame's seeds is compiled once per h up to GRP_H_GROUP (H = h: the
// seed loops unroll to exactly h); h = 9 .. 16 share ONE many-seed form (H = GRP_H_MANY), whose loops run over 16 seeds
// and drop the seeds >= sd->h at run time (a wave-uniform test).  Its per-lane arrays are sized for 16 seeds: where
// that would not fit the registers (the query's bucket lines, the fill's frames in flight) the form walks a frame's
// seeds in groups of GRP_H_GROUP, or keeps fewer frames in flight.
constexpr int GRP_H_GROUP = 8;
constexpr int GRP_H_MANY = 16;
static_assert(GRP_H_MANY == GRP_DEV_MAX_H && GRP_H_MANY <= 2 * GRP_H_GROUP, "the many-seed form covers the device tables in two groups");

template<int H>
__device__ __forceinline__ uint32_t
frame_seeds(const DevSeeds* __restrict__ sd)
{
  if constexpr (H <= GRP_H_GROUP) {
    return (uint32_t)H;
  } else {
    return sd->h;
  }
}

// seed s takes part in a frame of this form (always true, and folded away, in the forms of h <= GRP_H_GROUP)
template<int H>
__device__ __forceinline__ bool
seed_on(int s, uint32_t hn)
{
  return H <= GRP_H_GROUP || (uint32_t)s < hn;
}

// seed_hash for spans beyond 64 bases: each care position's 2-bit base is read from the staged words
// (one LDS dword per care position; a base never straddles two words).  No window is built — a per-lane array
// of the span would live in scratch — and every position read lies inside the seed's span, so inside the bases
// a kernel stages for its frames (a frame's seeds end at or before the last staged base).
__device__ inline uint64_t
seed_hash_long(const ulonglong2* sTab, const DevSeeds* __restrict__ sd, uint32_t s, const Win& w)
{
  uint64_t fwd = 0, rev = 0;
  const uint32_t wt = sd->weight[s];
  const ulonglong2* t = sTab + (size_t)s * sd->wmax * 4u;
  const uint32_t bit0 = w.b * 2u;
  for (uint32_t i = 0; i < wt; ++i) {
    const uint32_t bit = bit0 + sd->shift[s][i];
    const uint32_t b = (w.src[bit >> 5] >> (bit & 31u)) & 3u;
    const ulonglong2 e = t[i * 4u + b];
    fwd ^= e.x;
    rev ^= e.y;
  }
  return fwd + rev;
}

// WT > 0: every seed has weight WT (make_seed_pattern's seeds do) and the care
// loop is fully unrolled; WT == 0: run-time weights; WT == GRP_WT_LONG: run-time
// weights, spans beyond 64 bases
template<int WT>
__device__ inline uint64_t
seed_hash_t(const ulonglong2* sTab, const DevSeeds* __restrict__ sd, uint32_t s, const Win& win)
{
  const uint64_t w = win.lo; // (WT > 0 is only dispatched for seeds of span <= 32: the engine clears uniform_weight otherwise)
  if constexpr (WT == 0) {
    return seed_hash(sTab, sd, s, win);
  } else if constexpr (WT == GRP_WT_LONG) {
    return seed_hash_long(sTab, sd, s, win);
  } else {
    uint64_t fwd = 0, rev = 0;
    const ulonglong2* t = sTab + (size_t)s * WT * 4u;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)WT; ++i) {
      const uint32_t b = (uint32_t)(w >> sd->shift[s][i]) & 3u;
      const ulonglong2 e = t[i * 4u + b];
      fwd ^= e.x;
      rev ^= e.y;
    }
    return fwd + rev;
  }
}

__device__ inline void
load_tab(ulonglong2* sTab, const DevSeeds* __restrict__ sd)
{
  const uint32_t n = sd->h * sd->wmax * 4u;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    uint32_t s = i / (sd->wmax * 4u);
    uint32_t r = i - s * sd->wmax * 4u;
    sTab[i] = sd->tab[s][r >> 2][r & 3u];
  }
}

// stage bases [b0, b0+nb) of a read into LDS words (plus 4 zero pad words);
// returns the base offset of b0 inside the staged words
__device__ inline uint32_t
stage_bases(uint32_t* sBases, const uint32_t* __restrict__ packed, uint64_t word_off, uint32_t len, uint32_t b0, uint32_t nb)
{
  const uint32_t w0 = b0 >> 4;
  const uint32_t w_last = (b0 + nb + 15u) >> 4; // exclusive
  const uint32_t w_read = (len + 15u) >> 4;     // words the read owns
  const uint32_t nw = w_last - w0 + 4u; // + pad: a window reads up to 3 words from its first one, a wide one (span > 32) 5;
                                        // a long one (span > 64) reads its care positions only, all before b0 + nb
  for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) {
    uint32_t w = w0 + i;
    sBases[i] = (w < w_read) ? packed[word_off + w] : 0u;
  }
  return b0 & 15u;
}

// The tile geometry (host/gr_tile_geom.hpp) of the seeds on the device
__device__ __forceinline__ uint32_t
frames_per_tile(const DevSeeds* __restrict__ sd, uint32_t tile_len)
{
  return gr::geom::frames_per_tile(tile_len, sd->k, sd->span[0]);
}

__device__ __forceinline__ gr::geom::TileExtent
tile_extent(const DevSeeds* __restrict__ sd, uint32_t tile_len, uint32_t len, uint32_t ti)
{
  return gr::geom::tile_extent(tile_len, sd->k, sd->span[0], len, ti);
}

// ---- wave / block reductions -------------------------------------------------

__device__ inline uint32_t
wave_sum(uint32_t v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v += __shfl_xor(v, o, 64);
  }
  return v;
}

// ---- fill ------------------------------------------------------------------------

// WT: 0, or GRP_WT_LONG for seeds of spans beyond 64 bases (DevSeeds::wide == 2)
template<int H, int WT = 0>
__global__ void __launch_bounds__(THREADS)
k_fill(DevFilter f, DevReads rd, const DevSeeds* __restrict__ sd, uint64_t chunk_begin)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);

  const uint64_t chunk = chunk_begin + blockIdx.x;
  const uint32_t r = rd.chunk_read[chunk];
  const uint32_t ci = (uint32_t)(chunk - rd.chunk0[r]);
  const uint32_t len = rd.len[r];
  const uint32_t s0 = sd->span[0];     // the shortest seed: k, or k - 1 at odd k
  const uint32_t npos = len - s0 + 1u; // chunk exists => len >= s0 + h - 1
  const uint32_t p0 = ci * FILL_CHUNK;
  const uint32_t np = min(FILL_CHUNK, npos - p0);

  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, p0, np + s0 + hn - 2u);
  __syncthreads();

  uint32_t* words = f.bv;
  constexpr int FR = (H <= GRP_H_GROUP) ? 4 : 2; // the many-seed form: 2 x 16 probes in flight per lane (4 x 16 spill)
  for (uint32_t i0 = threadIdx.x; i0 < np; i0 += THREADS * FR) {
    uint64_t widx[FR][H];
    uint32_t mask[FR][H];
    uint32_t val[FR][H];
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      const uint32_t i = i0 + j * THREADS;
      const uint32_t p = p0 + i;
#pragma unroll
      for (int s = 0; s < H; ++s) {
        // seed s is valid at read position p iff p + span_s <= len
        // (stale re-inserts of the iterator set the same bit again)
        const bool ok = seed_on<H>(s, hn) && (i < np) && (p + sd->span[s] <= len);
        mask[j][s] = 0;
        widx[j][s] = 0;
        if (ok) {
          uint64_t hv = seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + i));
          uint64_t pos = grp_mod_m(hv, f.m, f.m_inv);
          widx[j][s] = pos >> 5;
          mask[j][s] = 1u << (uint32_t)(pos & 31u);
        }
      }
    }
    // test first (plain load), set only where needed: the filter saturates and
    // most probes find their bit already set
#pragma unroll
    for (int j = 0; j < FR; ++j) {
#pragma unroll
      for (int s = 0; s < H; ++s) {
        val[j][s] = mask[j][s] ? words[widx[j][s]] : 0xFFFFFFFFu;
      }
    }
#pragma unroll
    for (int j = 0; j < FR; ++j) {
#pragma unroll
      for (int s = 0; s < H; ++s) {
        if (mask[j][s] & ~val[j][s]) {
          atomicOr(&words[widx[j][s]], mask[j][s]);
        }
      }
    }
  }
}

// dst |= src, 16 bytes per lane (streaming)
__global__ void __launch_bounds__(THREADS)
k_bv_or(uint4* __restrict__ dst, const uint4* __restrict__ src, uint64_t n4, uint32_t* __restrict__ dst_tail, const uint32_t* __restrict__ src_tail, uint32_t n_tail)
{
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * THREADS) {
    const uint4 a = dst[i], b = src[i];
    dst[i] = make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < n_tail) {
    dst_tail[threadIdx.x] |= src_tail[threadIdx.x];
  }
}

// ---- finalize: plain bit vector -> 64-byte buckets -----------------------------

__global__ void __launch_bounds__(THREADS)
k_popcount(const uint32_t* __restrict__ bv, uint64_t n_words, unsigned long long* __restrict__ out)
{
  __shared__ uint32_t sW[THREADS / 64];
  uint32_t acc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * THREADS) {
    acc += __popc(bv[i]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) {
    sW[threadIdx.x >> 6] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
      t += sW[w];
    }
    atomicAdd(out, t);
  }
}

// the W filter bits of bucket b (bv is padded with 3 zero words)
__device__ inline uint64_t
bucket_bits(const uint32_t* __restrict__ bv, uint64_t b, uint32_t W, uint64_t m)
{
  const uint64_t s = b * W;
  const uint64_t w = s >> 5;
  const uint32_t sh = (uint32_t)(s & 31u);
  uint64_t v = ((uint64_t)bv[w] | ((uint64_t)bv[w + 1] << 32)) >> sh;
  if (sh) {
    v |= (uint64_t)bv[w + 2] << (64u - sh);
  }
  const uint64_t n = (s + W <= m) ? W : (m - s); // the last bucket may be short
  if (n < 64) {
    v &= (1ull << n) - 1ull;
  }
  return v;
}

__global__ void __launch_bounds__(THREADS)
k_bucket_chunk_sums(const uint32_t* __restrict__ bv, uint64_t m, uint32_t W, uint64_t n_buckets, uint32_t* __restrict__ chunk_sum)
{
  __shared__ uint32_t sW[THREADS / 64];
  const uint64_t b0 = (uint64_t)blockIdx.x * GRP_CHUNK_BUCKETS;
  uint32_t acc = 0;
  for (uint32_t i = threadIdx.x; i < GRP_CHUNK_BUCKETS; i += THREADS) {
    const uint64_t b = b0 + i;
    if (b < n_buckets) {
      acc += (uint32_t)__popcll(bucket_bits(bv, b, W, m));
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) {
    sW[threadIdx.x >> 6] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
      t += sW[w];
    }
    chunk_sum[blockIdx.x] = t;
  }
}

// single workgroup: exclusive scan of the chunk sums (uint64), superbucket table, pop
__global__ void __launch_bounds__(1024)
k_scan_chunks(const uint32_t* __restrict__ chunk_sum, uint64_t n_chunks, uint64_t* __restrict__ chunk_base, uint64_t* __restrict__ super, uint64_t* __restrict__ pop_out)
{
  __shared__ uint64_t sScan[1024];
  __shared__ uint64_t sCarry;
  if (threadIdx.x == 0) {
    sCarry = 0;
  }
  __syncthreads();
  const uint32_t chunks_per_super = (1u << GRP_SUPER_SHIFT) / GRP_CHUNK_BUCKETS;
  for (uint64_t c0 = 0; c0 < n_chunks; c0 += 1024) {
    uint64_t c = c0 + threadIdx.x;
    uint64_t v = (c < n_chunks) ? chunk_sum[c] : 0;
    sScan[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) { // Hillis-Steele inclusive scan
      uint64_t t = (threadIdx.x >= o) ? sScan[threadIdx.x - o] : 0;
      __syncthreads();
      sScan[threadIdx.x] += t;
      __syncthreads();
    }
    uint64_t excl = sCarry + sScan[threadIdx.x] - v;
    if (c < n_chunks) {
      chunk_base[c] = excl;
      if (c % chunks_per_super == 0) {
        super[c / chunks_per_super] = excl;
      }
    }
    __syncthreads();
    if (threadIdx.x == 1023) {
      sCarry += sScan[1023];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *pop_out = sCarry;
  }
}

// write every bucket unit of a chunk: {rel, bitmap, ids = 0}, {count words = 0}; count the overflow entries (n_ovf[0]:
// IDs beyond a bucket's 13th set bit, n_ovf[1]: count words beyond its 8th)
__global__ void __launch_bounds__(THREADS)
k_bucket_write(const uint32_t* __restrict__ bv, uint64_t m, uint32_t W, uint64_t n_buckets, uint4* __restrict__ buckets, const uint64_t* __restrict__ chunk_base, const uint64_t* __restrict__ super, unsigned long long* __restrict__ n_ovf)
{
  constexpr uint32_t PER = GRP_CHUNK_BUCKETS / THREADS; // consecutive buckets per thread
  __shared__ uint32_t sScan[THREADS];
  const uint64_t chunk = blockIdx.x;
  const uint64_t b0 = chunk * GRP_CHUNK_BUCKETS + (uint64_t)threadIdx.x * PER;
  uint64_t bm[PER];
  uint32_t tot = 0, ovf = 0, far = 0;
#pragma unroll
  for (uint32_t i = 0; i < PER; ++i) {
    const uint64_t b = b0 + i;
    bm[i] = (b < n_buckets) ? bucket_bits(bv, b, W, m) : 0ull;
    const uint32_t c = (uint32_t)__popcll(bm[i]);
    tot += c;
    ovf += (c > GRP_BUCKET_IDS) ? (c - GRP_BUCKET_IDS) : 0u;
    far += (c > GRP_NEAR_CW) ? (c - GRP_NEAR_CW) : 0u;
  }
  sScan[threadIdx.x] = tot;
  __syncthreads();
  for (uint32_t o = 1; o < THREADS; o <<= 1) {
    uint32_t t = (threadIdx.x >= o) ? sScan[threadIdx.x - o] : 0;
    __syncthreads();
    sScan[threadIdx.x] += t;
    __syncthreads();
  }
  const uint64_t sb = (chunk * GRP_CHUNK_BUCKETS) >> GRP_SUPER_SHIFT;
  uint32_t rel = (uint32_t)(chunk_base[chunk] - super[sb]) + sScan[threadIdx.x] - tot;
#pragma unroll
  for (uint32_t i = 0; i < PER; ++i) {
    const uint64_t b = b0 + i;
    if (b < n_buckets) {
      buckets[b * GRP_UNIT_U4 + 0] = make_uint4(rel, (uint32_t)bm[i], (uint32_t)(bm[i] >> 32), 0u);
#pragma unroll
      for (uint32_t q = 1; q < GRP_UNIT_U4; ++q) {
        buckets[b * GRP_UNIT_U4 + q] = make_uint4(0, 0, 0, 0);
      }
    }
    rel += (uint32_t)__popcll(bm[i]);
  }
  ovf = wave_sum(ovf);
  far = wave_sum(far);
  if ((threadIdx.x & 63) == 0 && ovf) {
    atomicAdd(n_ovf, (unsigned long long)ovf);
  }
  if ((threadIdx.x & 63) == 0 && far) {
    atomicAdd(n_ovf + 1, (unsigned long long)far);
  }
}

// the keys of the far table: every rank beyond its bucket's 8th set bit gets its slot (written once, read-only afterwards)
__global__ void __launch_bounds__(THREADS)
k_far_build(DevFilter f)
{
  for (uint64_t b = (uint64_t)blockIdx.x * THREADS + threadIdx.x; b < f.n_buckets; b += (uint64_t)gridDim.x * THREADS) {
    const uint4 hd = f.buckets[b * GRP_UNIT_U4];
    const uint32_t c = (uint32_t)__popcll(grp_bitmap(hd));
    if (c <= GRP_NEAR_CW) {
      continue;
    }
    const uint64_t base = f.super[b >> GRP_SUPER_SHIFT] + hd.x;
    for (uint32_t lr = GRP_NEAR_CW; lr < c; ++lr) {
      const unsigned long long key = base + lr + 1;
      uint64_t slot = (key * 0x9E3779B97F4A7C15ULL) >> 19 & f.far_mask;
      for (;;) {
        if (f.far[slot].x == 0ull && atomicCAS(&f.far[slot].x, 0ull, key) == 0ull) {
          break;
        }
        slot = (slot + 1) & f.far_mask;
      }
    }
  }
}

// zero the count words of the far table, keep the keys
__global__ void __launch_bounds__(THREADS)
k_far_reset(ulonglong2* __restrict__ far, uint64_t n)
{
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS) {
    far[i].y = 0ull;
  }
}

// zero every ID (bucket slots) and every count word, keep rel + bitmap
__global__ void __launch_bounds__(THREADS)
k_reset_bucket_ids(uint4* __restrict__ buckets, uint64_t n_buckets)
{
  // eight lanes per bucket unit, one 16-byte piece each (grid-stride: 8 * n_buckets may exceed a grid)
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n_buckets * GRP_UNIT_U4; i += (uint64_t)gridDim.x * THREADS) {
    if ((i & (GRP_UNIT_U4 - 1u)) == 0) {
      reinterpret_cast<uint32_t*>(&buckets[i])[3] = 0u;
    } else {
      buckets[i] = make_uint4(0, 0, 0, 0);
    }
  }
}

// ---- quad exchange (DPP) ------------------------------------------------------------

// value of quad lane G in every lane of the quad (v_mov_b32 dpp quad_perm:[G,G,G,G])
template<int G>
__device__ inline uint32_t
quad_bcast(uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, G * 0x55, 0xF, 0xF, true);
}

template<int G>
__device__ inline uint64_t
quad_bcast64(uint64_t v)
{
  return (uint64_t)quad_bcast<G>((uint32_t)v) | ((uint64_t)quad_bcast<G>((uint32_t)(v >> 32)) << 32);
}

struct QuadAnswer
{
  uint32_t bit; // filter bit of the probe
  uint32_t lr;  // set bits below it inside its bucket
  uint32_t id;  // ID slot min(lr, 12) of the bucket
  uint32_t rel; // bucket's relative rank (for the overflow table)
};

// The quad read of a probe's 64-byte line: round G reads the bucket of quad lane G's probe, four lanes x 16 bytes in one
// instruction.  Two piece orders:
//  - ROTATED (quad_load / quad_decode): quad lane L loads piece quad_piece<G>(L) = (L - G) & 3.  The request is the same
//    line, but the header piece (piece 0: {rel, bitmap lo, bitmap hi, ids[0]}) of lane G's probe arrives in lane G
//    ITSELF, in its round-G registers: a lane decodes only its own probe, once, and only the ID word crosses lanes.
//  - STRAIGHT (quad_answer_straight): lane L loads piece L, the header always arrives in quad lane 0 and every lane of
//    the quad runs the whole decode for all four rounds (four DPP broadcasts, shift, popcount, slot arithmetic each) to
//    keep one of the four results.  More instructions, a few registers fewer in some instantiations: quad_rotated()
//    says which k_query forms stay on it.
// The rotated form leans on this hipcc's code generation in three places (bit_select, quad_opaque, quad_load).  When the
// toolchain moves, re-check with tools/dev/kernel_resources.py against profiles/r10_quad_kernel_resources.txt: the row of
// k_query<3, 1, 0, true, false, false> (168 VGPRs, no VGPR spill, no scratch: three workgroups per CU) first, then the
// waves per SIMD of the forms quad_rotated() lists.
template<int G>
__device__ inline uint32_t
quad_piece(uint32_t sub)
{
  return (sub - (uint32_t)G) & 3u;
}

// the four rounds' piece offsets in bytes, one per byte of a word: ONE register across the kernel (quad_load extracts
// its round's byte)
__device__ inline uint32_t
quad_piece_bytes(uint32_t sub)
{
  return (quad_piece<0>(sub) << 4) | (quad_piece<1>(sub) << 12) | (quad_piece<2>(sub) << 20) | (quad_piece<3>(sub) << 28);
}

// Round G's 16 bytes of bucket b's line for this lane, rotated order.  The offset is extracted by a VOLATILE asm so that
// it stays at the load: as four plain values the offsets are hoisted out of the pass loop and held as 64-bit address
// parts in up to eight registers, which the streaming form does not have (VGPRs spilled) and which cost the many-seed
// forms a wave.
template<int G>
__device__ inline uint4
quad_load(const uint4* buckets, uint64_t b, uint32_t piece_bytes)
{
  uint32_t o;
  asm volatile("v_bfe_u32 %0, %1, %2, 8" : "=v"(o) : "v"(piece_bytes), "n"(8 * G));
  return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(buckets) + (quad_bcast64<G>(b) * (GRP_UNIT_U4 * 16u) + o));
}

// (a & m) | (b & ~m) in one instruction.  The selects of the exchange go through lane masks held in registers (0 / ~0):
// written as `c ? a : b` over words that come straight from the bucket loads, hipcc turns each select into a branch
// over exec so as to sink the load's wait into it (four branches a word); written as and / or, it distributes the nest
// into six masks and ten instructions a word.  Hence the instruction itself.
__device__ inline uint32_t
bit_select(uint32_t m, uint32_t a, uint32_t b)
{
  uint32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}

// a mask the optimiser cannot see through (an empty asm): it would otherwise recognise 0 / ~0 as a sign-extended
// condition and turn the bit_select back into the select it replaces
__device__ inline uint32_t
quad_opaque(uint32_t m)
{
  asm("" : "+v"(m));
  return m;
}

// a lane's place in its quad: constants of the kernel
struct QuadLane
{
  uint32_t sub;        // quad lane: threadIdx.x & 3
  uint32_t quad_base;  // first lane of the quad inside the wave
  uint32_t m0, m1, m2; // ~0 where sub == 0 / 1 / 2
};

__device__ inline QuadLane
quad_lane()
{
  QuadLane q;
  q.sub = threadIdx.x & 3u;
  q.quad_base = (threadIdx.x & 63u) & ~3u;
  q.m0 = quad_opaque(q.sub == 0u ? ~0u : 0u);
  q.m1 = quad_opaque(q.sub == 1u ? ~0u : 0u);
  q.m2 = quad_opaque(q.sub == 2u ? ~0u : 0u);
  return q;
}

// the value of round `sub`: a lane's own round (a register select, no exchange)
__device__ inline uint32_t
quad_own(const QuadLane& q, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3)
{
  return bit_select(q.m0, v0, bit_select(q.m1, v1, bit_select(q.m2, v2, v3)));
}

// Round G of the ID exchange: `slot` is the lane's own ID slot (dword index inside its bucket), lane G's is broadcast
// (the one DPP move of the round); every lane picks that component of its round-G piece, and lane G pulls the word
// from the lane that holds the slot's piece (`src`, its own byte address for ds_bpermute).  Lane G keeps the result.
template<int G>
__device__ inline uint32_t
quad_id_round(const uint4& piece, uint32_t slot, int src)
{
  const uint32_t sg = quad_bcast<G>(slot);
  const uint32_t c0 = quad_opaque((uint32_t)((int32_t)(sg << 31) >> 31)); // ~0 where the component's bit 0 / bit 1 is set
  const uint32_t c1 = quad_opaque((uint32_t)((int32_t)(sg << 30) >> 31));
  const uint32_t word = bit_select(c1, bit_select(c0, piece.w, piece.z), bit_select(c0, piece.y, piece.x));
  return (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)word);
}

// `pc[G]` is this lane's piece of round G (loaded in quad_piece order), `off` its OWN probe's bit offset.  The header
// is the piece of the lane's own round; bit, local rank, rel and the slot 3 + min(lr, 12) are computed once.  Only the
// ID word crosses lanes: piece p = slot >> 2 of lane G's line is held by quad lane (G + p) & 3 (for G = sub: `src`,
// the same in all four rounds; slot 3, ids[0], is the lane's own header piece and needs no special case).
__device__ __forceinline__ QuadAnswer
quad_decode(const uint4 (&pc)[4], uint32_t off, const QuadLane& q)
{
  const uint64_t bm = (uint64_t)quad_own(q, pc[0].y, pc[1].y, pc[2].y, pc[3].y) | ((uint64_t)quad_own(q, pc[0].z, pc[1].z, pc[2].z, pc[3].z) << 32);
  QuadAnswer a;
  a.rel = quad_own(q, pc[0].x, pc[1].x, pc[2].x, pc[3].x);
  a.bit = (uint32_t)((bm >> off) & 1ull);
  a.lr = grp_local_rank(bm, off);
  const uint32_t slot = 3u + min(a.lr, GRP_BUCKET_IDS - 1u); // dword index inside the bucket
  const int src = (int)((q.quad_base + ((q.sub + (slot >> 2)) & 3u)) << 2);
  const uint32_t r0 = quad_id_round<0>(pc[0], slot, src);
  const uint32_t r1 = quad_id_round<1>(pc[1], slot, src);
  const uint32_t r2 = quad_id_round<2>(pc[2], slot, src);
  const uint32_t r3 = quad_id_round<3>(pc[3], slot, src);
  a.id = quad_own(q, r0, r1, r2, r3);
  return a;
}

// The straight order.  Round G: `piece` is this lane's 16 bytes (piece `sub`) of the bucket probed by quad lane G, `off`
// this lane's OWN bit offset (lane G's is broadcast).  Every lane of the quad computes lane G's answer; lane G keeps it.
template<int G>
__device__ inline QuadAnswer
quad_answer(const uint4& piece, uint32_t off, uint32_t quad_base)
{
  const uint32_t o = quad_bcast<G>(off);
  // header words live in quad lane 0: {rel, bitmap lo, bitmap hi, ids[0]}
  const uint64_t bm = (uint64_t)quad_bcast<0>(piece.y) | ((uint64_t)quad_bcast<0>(piece.z) << 32);
  QuadAnswer a;
  a.rel = quad_bcast<0>(piece.x);
  a.bit = (uint32_t)((bm >> o) & 1ull);
  a.lr = grp_local_rank(bm, o);
  const uint32_t slot = 3u + min(a.lr, GRP_BUCKET_IDS - 1u); // dword index inside the bucket
  const uint32_t comp = slot & 3u;
  const uint32_t word = (comp == 0u) ? piece.x : (comp == 1u) ? piece.y : (comp == 2u) ? piece.z : piece.w;
  a.id = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((quad_base + (slot >> 2)) << 2), (int)word);
  return a;
}

__device__ __forceinline__ QuadAnswer
quad_answer_straight(const uint4 (&pc)[4], uint32_t off, const QuadLane& q)
{
  const QuadAnswer a0 = quad_answer<0>(pc[0], off, q.quad_base);
  const QuadAnswer a1 = quad_answer<1>(pc[1], off, q.quad_base);
  const QuadAnswer a2 = quad_answer<2>(pc[2], off, q.quad_base);
  const QuadAnswer a3 = quad_answer<3>(pc[3], off, q.quad_base);
  const uint32_t sub = q.sub;
  QuadAnswer a; // (field by field: a select between whole structs ends in scratch memory here)
  a.bit = (sub == 0) ? a0.bit : (sub == 1) ? a1.bit : (sub == 2) ? a2.bit : a3.bit;
  a.lr = (sub == 0) ? a0.lr : (sub == 1) ? a1.lr : (sub == 2) ? a2.lr : a3.lr;
  a.id = (sub == 0) ? a0.id : (sub == 1) ? a1.id : (sub == 2) ? a2.id : a3.id;
  a.rel = (sub == 0) ? a0.rel : (sub == 1) ? a1.rel : (sub == 2) ? a2.rel : a3.rel;
  return a;
}

// one round's load / a probe's answer in the order a kernel form is compiled for
template<bool ROT, int G>
__device__ __forceinline__ uint4
quad_read(const uint4* buckets, uint64_t b, const QuadLane& q, uint32_t piece_bytes)
{
  if constexpr (ROT) {
    return quad_load<G>(buckets, b, piece_bytes);
  } else {
    return buckets[quad_bcast64<G>(b) * GRP_UNIT_U4 + q.sub];
  }
}

template<bool ROT>
__device__ __forceinline__ QuadAnswer
quad_result(const uint4 (&pc)[4], uint32_t off, const QuadLane& q)
{
  if constexpr (ROT) {
    return quad_decode(pc, off, q);
  } else {
    return quad_answer_straight(pc, off, q);
  }
}

// Which k_query forms read in rotated order.  All do but those that lose a wave per SIMD to it with this hipcc (a few
// VGPRs across an allocation boundary, tools/dev/kernel_resources.py) and were not shown to run faster for it: the
// global-table redo forms <3,1,-1,false,false,true> (96 -> 98 VGPRs), <3,1,0,false,true,true> (128 -> 130),
// <4,1,0,false,false,true> (127 -> 129) and <16,1,0,false,false,true> (247 -> 264), which run for the few flagged
// tiles only and cannot be timed in a workload.  (<4,1,0,false,false,false>, 127 -> 129, and <16,1,0,false,false,false>,
// 246 -> 264, lose a wave as well and run faster rotated: the query kernels of an h = 4 stream by 4 %, of an h = 16
// stream by 6 %, DESIGN.md 4.)
template<int H, int FR, int WT, bool ST, bool VER, bool GT>
constexpr bool
quad_rotated()
{
  if (GT && !ST && FR == 1) {
    if ((H == 3 && WT == -1 && !VER) || (H == 3 && WT == 0 && VER) || (H == 4 && WT == 0 && !VER) || (H > GRP_H_GROUP && WT == 0 && !VER)) {
      return false;
    }
  }
  return true;
}
// ---- query -------------------------------------------------------------------------

// per-tile count table in LDS: open addressing, key = ID (0 = empty).  An
// insert is only attempted while fewer than `limit` distinct IDs are stored
// (limit <= capacity - THREADS*H - 1, so concurrent claims can never fill the
// table and probing always terminates); otherwise the tile is flagged and
// recomputed by the full-capacity launch.
__device__ inline void
hist_add(uint32_t* keys, uint32_t* cnts, uint32_t mask, uint32_t id, uint32_t* sDistinct, uint32_t limit, uint32_t* sOverflow)
{
  if (*reinterpret_cast<volatile uint32_t*>(sDistinct) >= limit) {
    *sOverflow = 1u;
    return;
  }
  uint32_t slot = (id * 2654435761u) & mask;
  for (;;) {
    uint32_t old = atomicCAS(&keys[slot], 0u, id);
    if (old == 0u) {
      atomicAdd(sDistinct, 1u);
    }
    if (old == 0u || old == id) {
      atomicAdd(&cnts[slot], 1u);
      return;
    }
    slot = (slot + 1u) & mask;
  }
}

// Round 4: the same table with 16-bit counts (a tile has at most tile_len <= 65535 frames: two counts per LDS
// word) and any even number of slots (multiply-shift instead of a mask).  At human-genome scale the 4^16 possible
// spaced k-mers of the default seeds are nearly all taken, so about half of a read's error k-mers are some other
// locus's k-mer and return that locus's ID: a tile of 1000 frames x 5 seeds holds ~2500 DISTINCT IDs — the
// 4096-slot table of rounds 1-3 (2815 usable at h = 5) overflowed on 40 % of the tiles of the C4 geometry and every
// one of them was queried twice.  6 bytes per slot instead of 8 and no power-of-two rounding let the worst case
// (tile x h IDs) fit the same LDS: no tile of the default geometries is ever flagged.
__device__ inline void
hist_add16(uint32_t* keys, uint32_t* cnt_words, uint32_t cap, uint32_t id, uint32_t* sDistinct, uint32_t limit, uint32_t* sOverflow)
{
  if (*reinterpret_cast<volatile uint32_t*>(sDistinct) >= limit) {
    *sOverflow = 1u;
    return;
  }
  uint32_t slot = __umulhi(id * 2654435761u, cap);
  for (;;) {
    uint32_t old = atomicCAS(&keys[slot], 0u, id);
    if (old == 0u) {
      atomicAdd(sDistinct, 1u);
    }
    if (old == 0u || old == id) {
      atomicAdd(&cnt_words[slot >> 1], 1u << ((slot & 1u) << 4));
      return;
    }
    slot = (slot + 1u == cap) ? 0u : slot + 1u;
  }
}

// (count, id) ordering of calc_num_assigned_tiles :607-615: larger count wins,
// equal counts -> smaller id (std::map ascending + strict '>')
__device__ inline bool
better(uint32_t c, uint32_t id, uint32_t bc, uint32_t bid)
{
  return (c > bc) || (c == bc && c != 0u && id < bid);
}

// ---- the seeds of one make_seed_pattern family share their halves ---------------------------
// seed i = left || 0^i || right (DevSeeds::n_left).  With seed 0's table entries
//   T[q][b] = { srol(SEED[b], K0-1-q), srol(SEED[comp b], q) }
// and, for a frame p,  L(p) / RL(p) = XOR of the .x / .y entries over the LEFT care positions,
// R(p) / RR(p) over the RIGHT ones:
//   fwd_i(p) = srol^i(L(p)) ^ R(p+i)      (left: K_i-1-q = (K0-1-q) + i; right: position q+i, rotation K0-1-q)
//   rev_i(p) = RL(p) ^ srol^i(RR(p+i))    (left: rotation q; right: rotation q + i)
// — srol rotates the two parts of the word, so it commutes with XOR and srol^a srol^b = srol^(a+b).
// hash_i = fwd_i + rev_i as ever (ntHash2's canonical sum).  A frame costs 16 look-ups instead
// of 16 per seed; R / RR of the frames p+1 .. p+H-1 are the neighbouring lanes' (wave shuffles).
template<int WT, bool LEFT, bool RIGHT>
__device__ inline void
seed_halves(const ulonglong2* sTab, const DevSeeds* __restrict__ sd, uint32_t n_left, const Win& win, uint64_t& L, uint64_t& RL, uint64_t& R, uint64_t& RR)
{
  const uint64_t w = win.lo; // (n_left is 0 for wide seeds: the shared halves are a 32-base form)
  L = RL = R = RR = 0;
  const uint32_t wt = WT > 0 ? (uint32_t)WT : sd->weight[0];
  if (n_left == 8u && wt == 16u) { // the pipeline's seeds (weight 16, palindromic): straight-line code
    if constexpr (LEFT) {
#pragma unroll
      for (uint32_t i = 0; i < 8u; ++i) {
        const ulonglong2 e = sTab[i * 4u + ((uint32_t)(w >> sd->shift[0][i]) & 3u)];
        L ^= e.x;
        RL ^= e.y;
      }
    }
    if constexpr (RIGHT) {
#pragma unroll
      for (uint32_t i = 8u; i < 16u; ++i) {
        const ulonglong2 e = sTab[i * 4u + ((uint32_t)(w >> sd->shift[0][i]) & 3u)];
        R ^= e.x;
        RR ^= e.y;
      }
    }
    return;
  }
  if constexpr (LEFT) {
    for (uint32_t i = 0; i < n_left; ++i) {
      const ulonglong2 e = sTab[i * 4u + ((uint32_t)(w >> sd->shift[0][i]) & 3u)];
      L ^= e.x;
      RL ^= e.y;
    }
  }
  if constexpr (RIGHT) {
    for (uint32_t i = n_left; i < wt; ++i) {
      const ulonglong2 e = sTab[i * 4u + ((uint32_t)(w >> sd->shift[0][i]) & 3u)];
      R ^= e.x;
      RR ^= e.y;
    }
  }
}

// srol^n for small n (split rotation: the low 33 and the high 31 bits rotate on their own)
__device__ inline uint64_t
srol_small(uint64_t x, uint32_t n)
{
  const uint64_t M33 = 0x1FFFFFFFFULL, M31 = 0x7FFFFFFFULL;
  const uint64_t lo = x & M33, hi = x >> 33;
  return ((((hi << n) | (hi >> (31u - n))) & M31) << 33) | (((lo << n) | (lo >> (33u - n))) & M33);
}

#define GRP_TILE_FLAGGED 0xFFFFFFFFu

// Stores / loads that are coherent across the XCDs' L2s inside one launch (agent scope,
// "sc1": written through to / read from the memory side).  The streaming window uses
// them for everything one workgroup hands to another; with them the hand-over needs no
// device-scope fence (whose L2 write-back + invalidate per workgroup costs the query
// kernel 5x, measured).
__device__ inline void
store_coherent(unsigned long long* p, unsigned long long v)
{
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline unsigned long long
load_coherent(const unsigned long long* p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline uint32_t
ldc(const uint32_t* p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void
stc(uint32_t* p, uint32_t v)
{
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static_assert(sizeof(grp_tile_summary) == 24 && sizeof(grp_id_count) == 8, "coherent copies move these as 64-bit words");

// coherent forms of the overflow-table accessors (grp_device.h): the table gains keys while
// a launch that both inserts and probes runs
__device__ inline uint32_t
grp_ovf_get_c(const DevFilter& f, uint64_t rank)
{
  uint64_t slot = (rank * 0x9E3779B97F4A7C15ULL) >> 17 & f.ovf_mask;
  for (;;) {
    const unsigned long long k = load_coherent(&f.ovf_keys[slot]);
    if (k == rank + 1) {
      return ldc(&f.ovf_ids[slot]);
    }
    if (k == 0) {
      return 0u;
    }
    slot = (slot + 1) & f.ovf_mask;
  }
}

__device__ inline void
grp_ovf_put_c(const DevFilter& f, uint64_t rank, uint32_t id)
{
  uint64_t slot = (rank * 0x9E3779B97F4A7C15ULL) >> 17 & f.ovf_mask;
  for (;;) {
    unsigned long long k = load_coherent(&f.ovf_keys[slot]);
    if (k == 0) {
      k = atomicCAS(&f.ovf_keys[slot], 0ull, (unsigned long long)(rank + 1));
      if (k == 0) {
        k = rank + 1;
      }
    }
    if (k == rank + 1) {
      stc(&f.ovf_ids[slot], id);
      return;
    }
    slot = (slot + 1) & f.ovf_mask;
  }
}

// scratch table of a whole-read insert (k_insert_collect / k_insert_apply below, and the
// in-launch insert of a streaming window)
struct InsertTable
{
  unsigned long long* keys;  // rank + 1, 0 = free (left clean by k_insert_apply)
  unsigned long long* masks; // blocks touching the rank
  unsigned long long* locs;  // dword index of the ID slot, or ~0 for the overflow table
  uint32_t* slots;           // claimed slots, in claim order
  uint32_t* counter;         // [2], alternating per call
  uint64_t cap_mask;
};

// (the control block of a streaming window that applies inserts itself, SCT_*, and every other word the launch and the
// host hand each other: grp_stream_proto.h)

// Streaming window (grp_classify_stream_*): persistent k_query<.., true> workgroups draw
// the window's tiles in order; the workgroup that finishes the LAST tile of a read takes
// that read's decision on the spot (first wave, register-resident state: a few
// microseconds) and publishes it in mapped host memory, so the host commits reads while
// the same launch is still working on later ones.  An abort (an insert made the rest of
// the window stale) parks the tile dispenser: the launch ends as soon as the resident
// tiles are done.
// (Measured alternatives: a decision by one lane walking LDS arrays keeps a 141-VGPR wave
// slot for ~100 us per read and costs the query kernel 10 %; resident decision waves in a
// second kernel do not fit beside 3 query workgroups per CU — they either displace one
// (-20 %) or starve until the launch ends.)
struct DevStreamCtl
{
  uint32_t first = 0;                    // batch index of the window's first read
  uint32_t* tiles_done = nullptr;        // [reads of the window] finished tiles, zeroed before the launch
  uint32_t* abort = nullptr;             // device memory: what every workgroup tests
  const uint32_t* abort_host = nullptr;  // mapped host memory: raised by the host, relayed by every 64th workgroup
  grp_read_decision* dec = nullptr;      // mapped host memory [reads]; .pad = 1 once the record is complete
  uint32_t* next_tile = nullptr;         // tile dispenser of the persistent workgroups; >= n_tiles: stop
  uint32_t* park = nullptr;              // first stale read of the window (UINT_MAX: none); tiles of earlier
                                         // reads that were already handed out are still processed
  uint32_t n_tiles = 0;
  uint32_t early_park = 1;               // the deciding wave parks the window at an insert / hand-back record
  unsigned long long* executed = nullptr; // EXE_*: probes of the tiles that were processed; round 6: what the in-launch inserts kept and redid
  grp_decide_params dp{};
  uint32_t* g_ids = nullptr;             // per-tile results (inspection) / scratch of long reads
  uint8_t* g_asg = nullptr;
  uint64_t* g_scratch = nullptr;
  // in-launch inserts: NULL ctl = the window ends at its first insert (striped windows, tests of the classic form)
  uint32_t* ctl = nullptr;            // SCT_* words, device memory
  const uint32_t* cmd_host = nullptr; // mapped host memory: CMD_SEQ the sequence number of the newest command, from CMD_FIELDS on its CMD_* fields
  uint32_t* ack_host = nullptr;       // mapped host memory: ACK_* words
  uint32_t n_reads = 0;               // reads of the window
  uint32_t n_decidable = 0;           // ... of this launch's stripes with at least one tile (the others are decided by the host)
  uint32_t cmd_while_busy = 0;        // a striped window: an insert command parks the launch wherever it is (the relays look for it between tiles)
  InsertTable tb{};
  unsigned long long timeout_ticks = 0; // wall_clock64 ticks a grid-wide wait / an idle workgroup may take
  // Round 6 — what the window has queried behind an inserting read is KEPT where the insert did not touch it: every probe
  // leaves a 32-bit fingerprint of its ID slot in the workgroup's LDS (the tile in progress and the one before), the
  // insert's apply pass collects the fingerprints of the slots it CHANGED, and behind the insert a workgroup holds its
  // tiles against that set — clean: the summary stands and is counted again, dirty: the tile is queried again (DESIGN 5a)
  uint32_t* tile_ver = nullptr;      // [tiles of the window] generation a finished tile's summary belongs to; 0: not begun; STREAM_TILE_BUSY / _HELD
  uint32_t* fp_tab[2] = { nullptr, nullptr }; // changed-slot sets of the last two inserts (open addressing, 0 = empty)
  uint32_t fp_mask = 0;
  uint32_t* rel = nullptr;           // release words of the grid-wide waits: one 128-byte line per workgroup (stream_grid_wait)
  uint32_t* dbg = nullptr;           // developer (GRP_STREAM_DEBUG): where every workgroup is, one word each — read by the host when a grid-wide wait times out
  uint32_t n_fp = 0;                 // fingerprint buffers per workgroup (0: none — every insert hands everything behind it out again, rounds 3-5)
  uint32_t fp_off = 0;               // where they start in the dynamic LDS (bytes)
  uint32_t fp_words = 0;             // words per buffer: passes x THREADS x h
};

constexpr uint32_t STREAM_TILE_HELD = 0xFFFFFFFEu;  // tile_ver: finished, fingerprints in its workgroup's LDS (that workgroup says what becomes of it)
constexpr uint32_t STREAM_TILE_BUSY = 0xFFFFFFFDu;  // tile_ver: one of a workgroup's kept tiles that an insert touched: that workgroup queries it again itself
constexpr uint32_t STREAM_REDO_NONE = 0xFFFFFFFFu;  // no tile
constexpr uint32_t STREAM_FULL_RESET = 0x80000000u; // SCT_SCAN_END, bit 31

// fingerprint of the ID slot a probe reads: the filter position it belongs to — bucket b, bit `off` of it (what grp_locate
// gives, known as soon as the hash is; the insert's side keeps the offset with the slot's location, insert_collect_unit).  Never 0.
__device__ inline uint32_t
slot_fp(uint64_t b, uint32_t off)
{
  const uint32_t x = ((uint32_t)b ^ ((uint32_t)(b >> 32) * 0x85EBCA6Bu)) * 0x9E3779B1u + off;
  return x ? x : 1u;
}

// an insert table entry's location word: the ID slot (grp_id_loc) below, the filter bit's offset inside its bucket on top
constexpr unsigned long long IR_LOC_MASK = (1ull << 58) - 1ull;

__device__ inline uint32_t
fp_home(uint32_t fp, uint32_t mask)
{
  return (fp ^ (fp >> 15)) & mask;
}

// the insert's side (agent-scope: workgroups of every XCD fill one table)
__device__ inline void
fp_put(uint32_t* tab, uint32_t mask, uint32_t fp)
{
  uint32_t slot = fp_home(fp, mask);
  for (;;) {
    uint32_t cur = ldc(&tab[slot]);
    if (cur == 0u) {
      cur = atomicCAS(&tab[slot], 0u, fp);
      if (cur == 0u) {
        return;
      }
    }
    if (cur == fp) {
      return;
    }
    slot = (slot + 1u) & mask;
  }
}

// the query's side, behind the insert's second grid-wide wait (its acquire fence): plain loads
__device__ inline bool
fp_has(const uint32_t* tab, uint32_t mask, uint32_t fp)
{
  uint32_t slot = fp_home(fp, mask);
  for (;;) {
    const uint32_t cur = tab[slot];
    if (cur == 0u) {
      return false;
    }
    if (cur == fp) {
      return true;
    }
    slot = (slot + 1u) & mask;
  }
}

// reads of up to this many tiles are decided inside the streaming launch (37 bytes of the
// idle count-table area per tile: 9.5 KB of the >= 16 KB the small geometry owns)
constexpr uint32_t STREAM_LDS_TILES = 256;

// ---- wave-register state for the decision core (csrc/host/gr_tiles_core.hpp) -------
// Tile i of the read lives in lane i (reads of up to 64 tiles); every access is a
// v_readlane / v_writelane with a wave-uniform index, so the passes run as scalar code
// executed by the whole wave in lockstep.
__device__ inline uint32_t
lane_get(uint32_t v, size_t i)
{
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)i);
}

// v_writelane by hand (this compiler has no builtin for it): value and index are
// wave-uniform, every lane executes — a compare and a select
__device__ inline uint32_t
lane_set(uint32_t v, size_t i, uint32_t reg)
{
  return (__lane_id() == (uint32_t)i) ? v : reg;
}

struct LaneState
{
  uint32_t v_top_id = 0, v_top_count = 0, v_list_n = 0, v_list_off = 0, v_hits = 0, v_misses = 0;
  uint32_t v_id = 0, v_asg = 0, v_lo = 0, v_hi = 0;
  // the first LANE_LIST entries of every tile's count>2 list, fetched by all lanes at once
  // (P1 / P2 walk the lists tile by tile: one dependent global load per entry otherwise,
  // ~40 us per 25-tile read, measured)
  static constexpr uint32_t LANE_LIST = 4;
  uint32_t v_eid[LANE_LIST] = { 0, 0, 0, 0 }, v_ecnt[LANE_LIST] = { 0, 0, 0, 0 };
  const grp_id_count* lists = nullptr;

  __device__ uint32_t top_id(size_t i) const { return lane_get(v_top_id, i); }
  __device__ uint32_t top_count(size_t i) const { return lane_get(v_top_count, i); }
  __device__ uint32_t list_n(size_t i) const { return lane_get(v_list_n, i); }
  __device__ uint32_t list_off(size_t i) const { return lane_get(v_list_off, i); }
  __device__ uint32_t hits(size_t i) const { return lane_get(v_hits, i); }
  __device__ uint32_t misses(size_t i) const { return lane_get(v_misses, i); }
  __device__ grp_id_count list_entry(size_t k) const { return gr::core::load_list_entry(lists + k); }
  __device__ grp_id_count tile_list_entry(size_t i, uint32_t j) const
  {
    grp_id_count e;
    switch (j) { // wave-uniform
      case 0: e.id = lane_get(v_eid[0], i); e.count = lane_get(v_ecnt[0], i); return e;
      case 1: e.id = lane_get(v_eid[1], i); e.count = lane_get(v_ecnt[1], i); return e;
      case 2: e.id = lane_get(v_eid[2], i); e.count = lane_get(v_ecnt[2], i); return e;
      case 3: e.id = lane_get(v_eid[3], i); e.count = lane_get(v_ecnt[3], i); return e;
      default: return gr::core::load_list_entry(lists + lane_get(v_list_off, i) + j);
    }
  }
  // `want` in tile i's count>2 list: the WHOLE wave looks, 64 entries a step (every lane is active here: the passes
  // run as wave-uniform code); see PtrState::find_in_list
  __device__ bool find_in_list(size_t i, uint32_t want, uint32_t& count) const
  {
    const uint32_t ln = list_n(i), off = list_off(i);
    const uint32_t lane = __lane_id();
    for (uint32_t base = 0; base < ln; base += 64u) {
      const uint32_t j = base + lane;
      grp_id_count e;
      e.id = 0u;
      e.count = 0u;
      if (j < ln) {
        e = gr::core::load_list_entry(lists + off + j);
      }
      const unsigned long long m = __ballot(j < ln && e.id == want);
      if (m != 0ull) {
        count = (uint32_t)__builtin_amdgcn_readlane((int)e.count, __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1));
        return true;
      }
    }
    return false;
  }
  // this lane's tile: prefetch its list head (call after load(); only for a valid, unflagged tile)
  __device__ void load_list_head()
  {
#pragma unroll
    for (uint32_t j = 0; j < LANE_LIST; ++j) {
      if (j < v_list_n) {
        const grp_id_count e = gr::core::load_list_entry(lists + v_list_off + j);
        v_eid[j] = e.id;
        v_ecnt[j] = e.count;
      }
    }
  }
  __device__ uint32_t id(size_t i) const { return lane_get(v_id, i); }
  __device__ void set_id(size_t i, uint32_t v) { v_id = lane_set(v, i, v_id); }
  __device__ uint32_t asg(size_t i) const { return lane_get(v_asg, i); }
  __device__ void set_asg(size_t i, uint32_t v) { v_asg = lane_set(v, i, v_asg); }
  __device__ uint64_t scr(size_t i) const { return (uint64_t)lane_get(v_lo, i) | ((uint64_t)lane_get(v_hi, i) << 32); }
  __device__ void set_scr(size_t i, uint64_t v)
  {
    v_lo = lane_set((uint32_t)v, i, v_lo);
    v_hi = lane_set((uint32_t)(v >> 32), i, v_hi);
  }
  __device__ void log_pass(size_t) const {}
  // whole-state operations: tile i in lane i, lanes >= n hold zeros (see load)
  __device__ void init_from_top(size_t n, size_t x)
  {
    v_id = v_top_id;
    v_asg = (__lane_id() < (uint32_t)n && v_list_n != 0u && (size_t)v_top_count > x) ? 1u : 0u;
  }
  __device__ size_t count_asg(size_t) const { return (size_t)__popcll(__ballot(v_asg != 0u)); }
  __device__ void sum_hits_misses(size_t, uint32_t& h, uint32_t& m) const
  {
    h = wave_sum(v_hits);
    m = wave_sum(v_misses);
  }
  // P7's work list (PtrState::sort_assigned): every lane counts the assigned keys below its own while the keys
  // pass by one at a time, then one cross-lane permutation puts key r into lane r (the unassigned lanes take
  // the places behind, so it is a permutation of all 64 lanes)
  __device__ size_t sort_assigned(size_t n)
  {
    const unsigned long long am = __ballot(v_asg != 0u);
    const uint32_t ne = (uint32_t)__popcll(am);
    const uint32_t lane = __lane_id();
    uint32_t rank = 0;
    for (uint32_t j = 0; j < (uint32_t)n; ++j) { // wave-uniform
      if ((am >> j) & 1ull) {
        const uint32_t idj = lane_get(v_id, j);
        rank += (idj < v_id || (idj == v_id && j < lane)) ? 1u : 0u;
      }
    }
    const uint32_t dst = (v_asg != 0u) ? rank : ne + (uint32_t)__popcll(~am & ((1ull << lane) - 1ull));
    v_lo = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)lane);
    v_hi = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)v_id);
    return ne;
  }
  // wave-wide summaries of the state
  __device__ bool any_asg(size_t) const { return __ballot(v_asg != 0u) != 0ull; }
  __device__ bool any_list(size_t) const { return __ballot(v_list_n != 0u) != 0ull; }
  __device__ void load(const grp_tile_summary& t)
  {
    v_top_id = t.top_id;
    v_top_count = t.top_count;
    v_list_n = t.list_n;
    v_list_off = t.list_off;
    v_hits = t.hits;
    v_misses = t.misses;
  }
};
constexpr uint32_t LANE_TILES = 64;

// The same for longer reads: NS register sets, tile i in lane i & 63 of set i >> 6 (the index is wave-uniform, so is
// the choice of the set) — 128 tiles with two sets, 256 with four.  Only k_decide uses it: the streaming kernel has
// no registers to spare (it sits at its 128-VGPR cap) and decides such reads from LDS arrays.  Round 4: with a
// realistic ONT length tail (bench.py --len-sigma 0.6: 3 % of the reads have more than 64 tiles, one read in 300 more
// than 128) the one-lane walk over GLOBAL arrays that k_decide fell back to took ~1 ms per read and every decision
// launch of a batch waited for it (k_decide 0.4 -> 9.4 s over the C2 stream, profiles/r04_long_tail.txt).
template<int NS>
struct LaneStateN
{
  uint32_t v_top_id[NS] = {}, v_top_count[NS] = {}, v_list_n[NS] = {}, v_list_off[NS] = {}, v_hits[NS] = {}, v_misses[NS] = {};
  uint32_t v_id[NS] = {}, v_asg[NS] = {}, v_lo[NS] = {}, v_hi[NS] = {};
  static constexpr uint32_t LANE_LIST = 4;
  uint32_t v_eid[LANE_LIST][NS] = {}, v_ecnt[LANE_LIST][NS] = {}; // [entry][set]
  const grp_id_count* lists = nullptr;

  // Every array index below is a compile-time constant AND every load / store of the state is unconditional: the
  // choice of the set is a select between VALUES.  (A loop the optimizer did not unroll, and later an if-chain whose
  // loads and stores the CFG simplifier merged behind a phi of ADDRESSES, each put the whole state into scratch
  // memory: 304 bytes, ~1.7 ms per decision launch.)
  template<int S = 0>
  __device__ static __attribute__((always_inline)) uint32_t get(const uint32_t (&v)[NS], size_t i)
  {
    const uint32_t mine = lane_get(v[S], i & 63);
    if constexpr (S == NS - 1) {
      return mine;
    } else {
      const uint32_t rest = get<S + 1>(v, i);
      return ((i >> 6) == (size_t)S) ? mine : rest; // wave-uniform choice
    }
  }
  template<int S = 0>
  __device__ static __attribute__((always_inline)) void put(uint32_t (&v)[NS], size_t i, uint32_t x)
  {
    if constexpr (S < NS) {
      const uint32_t old = v[S];
      const uint32_t with = lane_set(x, i & 63, old);
      v[S] = ((i >> 6) == (size_t)S) ? with : old;
      put<S + 1>(v, i, x);
    }
  }
  // entry j < LANE_LIST of tile i: first the choice of j in every set (per lane), then the set and the lane
  template<int S = 0>
  __device__ static __attribute__((always_inline)) void pick_entry(const uint32_t (&v)[LANE_LIST][NS], uint32_t j, uint32_t (&out)[NS])
  {
    if constexpr (S < NS) {
      const uint32_t e0 = v[0][S], e1 = v[1][S], e2 = v[2][S], e3 = v[3][S];
      out[S] = j == 0 ? e0 : j == 1 ? e1 : j == 2 ? e2 : e3;
      pick_entry<S + 1>(v, j, out);
    }
  }
  __device__ __attribute__((always_inline)) grp_id_count head_entry(size_t i, uint32_t j) const
  {
    uint32_t ids[NS], cnts[NS];
    pick_entry(v_eid, j, ids);
    pick_entry(v_ecnt, j, cnts);
    grp_id_count e;
    e.id = get(ids, i);
    e.count = get(cnts, i);
    return e;
  }
  __device__ uint32_t top_id(size_t i) const { return get(v_top_id, i); }
  __device__ uint32_t top_count(size_t i) const { return get(v_top_count, i); }
  __device__ uint32_t list_n(size_t i) const { return get(v_list_n, i); }
  __device__ uint32_t list_off(size_t i) const { return get(v_list_off, i); }
  __device__ uint32_t hits(size_t i) const { return get(v_hits, i); }
  __device__ uint32_t misses(size_t i) const { return get(v_misses, i); }
  __device__ grp_id_count list_entry(size_t k) const { return gr::core::load_list_entry(lists + k); }
  __device__ grp_id_count tile_list_entry(size_t i, uint32_t j) const
  {
    return j < LANE_LIST ? head_entry(i, j) : gr::core::load_list_entry(lists + get(v_list_off, i) + j);
  }
  // `want` in tile i's count>2 list: the WHOLE wave looks, 64 entries a step (every lane is active here: the passes
  // run as wave-uniform code); see PtrState::find_in_list
  __device__ bool find_in_list(size_t i, uint32_t want, uint32_t& count) const
  {
    const uint32_t ln = list_n(i), off = list_off(i);
    const uint32_t lane = __lane_id();
    for (uint32_t base = 0; base < ln; base += 64u) {
      const uint32_t j = base + lane;
      grp_id_count e;
      e.id = 0u;
      e.count = 0u;
      if (j < ln) {
        e = gr::core::load_list_entry(lists + off + j);
      }
      const unsigned long long m = __ballot(j < ln && e.id == want);
      if (m != 0ull) {
        count = (uint32_t)__builtin_amdgcn_readlane((int)e.count, __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1));
        return true;
      }
    }
    return false;
  }
  // this lane's tile of set S: its summary and the head of its list (a valid, unflagged tile)
  template<int S>
  __device__ __attribute__((always_inline)) void load(const grp_tile_summary& t, bool with_list)
  {
    v_top_id[S] = t.top_id;
    v_top_count[S] = t.top_count;
    v_list_n[S] = t.list_n;
    v_list_off[S] = t.list_off;
    v_hits[S] = t.hits;
    v_misses[S] = t.misses;
    if (with_list) {
      if (0 < t.list_n) {
        const grp_id_count e = gr::core::load_list_entry(lists + t.list_off + 0);
        v_eid[0][S] = e.id;
        v_ecnt[0][S] = e.count;
      }
      if (1 < t.list_n) {
        const grp_id_count e = gr::core::load_list_entry(lists + t.list_off + 1);
        v_eid[1][S] = e.id;
        v_ecnt[1][S] = e.count;
      }
      if (2 < t.list_n) {
        const grp_id_count e = gr::core::load_list_entry(lists + t.list_off + 2);
        v_eid[2][S] = e.id;
        v_ecnt[2][S] = e.count;
      }
      if (3 < t.list_n) {
        const grp_id_count e = gr::core::load_list_entry(lists + t.list_off + 3);
        v_eid[3][S] = e.id;
        v_ecnt[3][S] = e.count;
      }
    }
  }
  __device__ uint32_t id(size_t i) const { return get(v_id, i); }
  __device__ void set_id(size_t i, uint32_t v) { put(v_id, i, v); }
  __device__ uint32_t asg(size_t i) const { return get(v_asg, i); }
  __device__ void set_asg(size_t i, uint32_t v) { put(v_asg, i, v); }
  __device__ uint64_t scr(size_t i) const { return (uint64_t)get(v_lo, i) | ((uint64_t)get(v_hi, i) << 32); }
  __device__ void set_scr(size_t i, uint64_t v)
  {
    put(v_lo, i, (uint32_t)v);
    put(v_hi, i, (uint32_t)(v >> 32));
  }
  __device__ void log_pass(size_t) const {}
  template<int S = 0>
  __device__ __attribute__((always_inline)) void init_set(size_t n, size_t x)
  {
    if constexpr (S < NS) {
      v_id[S] = v_top_id[S];
      v_asg[S] = (__lane_id() + 64u * (uint32_t)S < (uint32_t)n && v_list_n[S] != 0u && (size_t)v_top_count[S] > x) ? 1u : 0u;
      init_set<S + 1>(n, x);
    }
  }
  __device__ void init_from_top(size_t n, size_t x) { init_set(n, x); }
  template<int S = 0>
  __device__ __attribute__((always_inline)) size_t count_set() const
  {
    if constexpr (S == NS) {
      return 0;
    } else {
      return (size_t)__popcll(__ballot(v_asg[S] != 0u)) + count_set<S + 1>();
    }
  }
  __device__ size_t count_asg(size_t) const { return count_set(); }
  template<int S = 0>
  __device__ static __attribute__((always_inline)) uint32_t sum_of(const uint32_t (&v)[NS])
  {
    if constexpr (S == NS) {
      return 0u;
    } else {
      return v[S] + sum_of<S + 1>(v);
    }
  }
  template<int S = 0>
  __device__ static __attribute__((always_inline)) uint32_t or_of(const uint32_t (&v)[NS])
  {
    if constexpr (S == NS) {
      return 0u;
    } else {
      return v[S] | or_of<S + 1>(v);
    }
  }
  __device__ void sum_hits_misses(size_t, uint32_t& h, uint32_t& m) const
  {
    h = wave_sum(sum_of(v_hits));
    m = wave_sum(sum_of(v_misses));
  }
  __device__ bool any_asg(size_t) const { return __ballot(or_of(v_asg) != 0u) != 0ull; }
  __device__ bool any_list(size_t) const { return __ballot(or_of(v_list_n) != 0u) != 0ull; }
  // P7's work list (LaneState::sort_assigned): the keys of set S pass by, every lane counts for each of its NS
  // keys; the placement goes through LDS (sort_lds: 64 * NS words of 8 bytes)
  uint64_t* sort_lds = nullptr;
  template<int T = 0>
  __device__ __attribute__((always_inline)) void rank_step(uint32_t idj, uint32_t j, uint32_t (&rank)[NS]) const
  {
    if constexpr (T < NS) {
      const uint32_t mine = v_id[T], me = __lane_id() + 64u * (uint32_t)T;
      rank[T] += (idj < mine || (idj == mine && j < me)) ? 1u : 0u;
      rank_step<T + 1>(idj, j, rank);
    }
  }
  template<int S = 0>
  __device__ __attribute__((always_inline)) uint32_t rank_sets(uint32_t n, uint32_t (&rank)[NS]) const
  {
    if constexpr (S == NS) {
      return 0u;
    } else {
      const unsigned long long am = __ballot(v_asg[S] != 0u);
      for (uint32_t l = 0; l < 64u && l + 64u * (uint32_t)S < n; ++l) { // wave-uniform
        if ((am >> l) & 1ull) {
          rank_step(lane_get(v_id[S], l), l + 64u * (uint32_t)S, rank);
        }
      }
      return (uint32_t)__popcll(am) + rank_sets<S + 1>(n, rank);
    }
  }
  template<int T = 0>
  __device__ __attribute__((always_inline)) void place_keys(const uint32_t (&rank)[NS])
  {
    if constexpr (T < NS) {
      if (v_asg[T] != 0u) {
        sort_lds[rank[T]] = ((uint64_t)v_id[T] << 32) | (uint64_t)(__lane_id() + 64u * (uint32_t)T);
      }
      place_keys<T + 1>(rank);
    }
  }
  template<int T = 0>
  __device__ __attribute__((always_inline)) void fetch_keys()
  {
    if constexpr (T < NS) {
      const uint64_t key = sort_lds[__lane_id() + 64u * (uint32_t)T];
      v_lo[T] = (uint32_t)key;
      v_hi[T] = (uint32_t)(key >> 32);
      fetch_keys<T + 1>();
    }
  }
  __device__ size_t sort_assigned(size_t n)
  {
    uint32_t rank[NS] = {};
    const uint32_t ne = rank_sets((uint32_t)n, rank);
    place_keys(rank);
    __builtin_amdgcn_wave_barrier(); // one wave: its LDS accesses complete in order
    fetch_keys();
    __builtin_amdgcn_wave_barrier();
    return ne;
  }
};

// The state in LDS arrays, walked by ALL lanes of a wave in step (every access at a wave-uniform address: a
// broadcast) — reads too long for the register forms.  The passes stay serial; P7's sort uses the lanes.
struct WaveLdsState : gr::core::PtrState
{
  // `want` in tile i's count>2 list: the WHOLE wave looks, 64 entries a step (every lane is active here: the passes
  // run as wave-uniform code); see PtrState::find_in_list
  __device__ bool find_in_list(size_t i, uint32_t want, uint32_t& count) const
  {
    const uint32_t ln = list_n(i), off = list_off(i);
    const uint32_t lane = __lane_id();
    for (uint32_t base = 0; base < ln; base += 64u) {
      const uint32_t j = base + lane;
      grp_id_count e;
      e.id = 0u;
      e.count = 0u;
      if (j < ln) {
        e = gr::core::load_list_entry(lists + off + j);
      }
      const unsigned long long m = __ballot(j < ln && e.id == want);
      if (m != 0ull) {
        count = (uint32_t)__builtin_amdgcn_readlane((int)e.count, __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1));
        return true;
      }
    }
    return false;
  }
  __device__ size_t sort_assigned(size_t n)
  {
    const uint32_t lane = __lane_id();
    uint32_t mine = 0;
    for (uint32_t i = lane; i < (uint32_t)n; i += 64u) {
      mine += flags[i] ? 1u : 0u;
    }
    const uint32_t ne = wave_sum(mine);
    for (uint32_t i = lane; i < (uint32_t)n; i += 64u) {
      if (flags[i]) {
        const uint32_t my = ids[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < (uint32_t)n; ++j) {
          const uint32_t idj = ids[j];
          rank += (flags[j] && (idj < my || (idj == my && j < i))) ? 1u : 0u;
        }
        scratch[rank] = ((uint64_t)my << 32) | (uint64_t)i;
      }
    }
    __builtin_amdgcn_wave_barrier();
    return (size_t)ne;
  }
};

// one wave, a read of up to NS * 64 tiles [a, a + n) of the window: tiles into the register sets, the shared decision
// core, per-tile results out; false: a tile is flagged / its list lies beyond the arena (decided again later)
template<int NS, int S = 0>
__device__ __attribute__((always_inline)) inline bool
lane_sets_load(LaneStateN<NS>& st, uint32_t lane, uint64_t a, uint64_t n, const grp_tile_summary* __restrict__ tiles, uint64_t lists_cap)
{
  if constexpr (S == NS) {
    return false;
  } else {
    bool bad = false;
    const uint32_t i = lane + 64u * (uint32_t)S;
    if (i < n) {
      const grp_tile_summary t = tiles[a + i];
      bad = t.list_n == GRP_TILE_FLAGGED || (uint64_t)t.list_off + t.list_n > lists_cap;
      st.template load<S>(t, !bad);
    }
    return lane_sets_load<NS, S + 1>(st, lane, a, n, tiles, lists_cap) || bad;
  }
}

template<int NS, int S = 0>
__device__ __attribute__((always_inline)) inline void
lane_sets_store(const LaneStateN<NS>& st, uint32_t lane, uint64_t a, uint64_t n, uint32_t* __restrict__ g_ids, uint8_t* __restrict__ g_asg)
{
  if constexpr (S < NS) {
    const uint32_t i = lane + 64u * (uint32_t)S;
    if (i < n) {
      g_ids[a + i] = st.v_id[S];
      g_asg[a + i] = (uint8_t)st.v_asg[S];
    }
    lane_sets_store<NS, S + 1>(st, lane, a, n, g_ids, g_asg);
  }
}

template<int NS>
__device__ inline bool
decide_in_registers(uint32_t lane, uint64_t a, uint64_t n, const grp_decide_params& dp, const grp_tile_summary* __restrict__ tiles, const grp_id_count* __restrict__ lists, uint64_t lists_cap,
                    uint32_t* __restrict__ g_ids, uint8_t* __restrict__ g_asg, uint64_t* sort_lds, grp_read_decision& d)
{
  LaneStateN<NS> st;
  st.lists = lists;
  st.sort_lds = sort_lds;
  const bool bad = lane_sets_load<NS>(st, lane, a, n, tiles, lists_cap);
  if (__ballot(bad) != 0ull) {
    return false;
  }
  gr::core::decide(dp.threshold, dp.unassigned_min, dp.assigned_max, (size_t)n, st, d);
  lane_sets_store<NS>(st, lane, a, n, g_ids, g_asg);
  return true;
}

// One wave (all 64 lanes), read `rj` of a streaming window complete (tiles [a, a+n) of the
// window): the decision, published to the host.  Summaries and lists were written by other
// workgroups during this launch: coherent loads.  `lds` / cap_tiles: work space for reads
// of more than 64 tiles (the idle count-table area of the workgroup).
__device__ inline void
stream_decide(const DevStreamCtl& sc, uint32_t rj, uint64_t a, uint32_t n, const grp_tile_summary* tiles, const grp_id_count* lists, uint64_t lists_cap, uint32_t* lds, uint32_t cap_tiles)
{
  const uint32_t lane = threadIdx.x;
  grp_read_decision d{};
  auto fetch = [&](uint32_t i) {
    union
    {
      unsigned long long w[3];
      grp_tile_summary t;
    } u;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(tiles + a + i);
    u.w[0] = load_coherent(src);
    u.w[1] = load_coherent(src + 1);
    u.w[2] = load_coherent(src + 2);
    return u.t;
  };
  if (n <= LANE_TILES) {
    LaneState st;
    st.lists = lists;
    bool bad = false;
    if (lane < n) {
      const grp_tile_summary t = fetch(lane);
      st.load(t);
      bad = t.list_n == GRP_TILE_FLAGGED || (uint64_t)t.list_off + t.list_n > lists_cap;
      if (!bad) {
        st.load_list_head();
      }
    }
    if (__ballot(bad) == 0ull) { // else kind stays 0: the host takes this read through the synchronous path
      gr::core::decide(sc.dp.threshold, sc.dp.unassigned_min, sc.dp.assigned_max, (size_t)n, st, d);
      if (lane < n) {
        sc.g_ids[a + lane] = st.v_id;
        sc.g_asg[a + lane] = (uint8_t)st.v_asg;
      }
    }
  } else if (n <= cap_tiles) {
    uint64_t* sScratch = reinterpret_cast<uint64_t*>(lds);
    grp_tile_summary* sTiles = reinterpret_cast<grp_tile_summary*>(sScratch + cap_tiles);
    uint32_t* sIds = reinterpret_cast<uint32_t*>(sTiles + cap_tiles);
    uint8_t* sAsg = reinterpret_cast<uint8_t*>(sIds + cap_tiles);
    bool bad = false;
    for (uint32_t i = lane; i < n; i += 64u) {
      const grp_tile_summary t = fetch(i);
      sTiles[i] = t;
      bad = bad || t.list_n == GRP_TILE_FLAGGED || (uint64_t)t.list_off + t.list_n > lists_cap;
    }
    const bool redo = __ballot(bad) != 0ull;
    __builtin_amdgcn_wave_barrier();
    if (!redo) {
      WaveLdsState st;
      st.tiles = sTiles;
      st.lists = lists;
      st.ids = sIds;
      st.flags = sAsg;
      st.scratch = sScratch;
      gr::core::decide(sc.dp.threshold, sc.dp.unassigned_min, sc.dp.assigned_max, (size_t)n, st, d); // all lanes, in step
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = lane; i < n; i += 64u) {
        sc.g_ids[a + i] = sIds[i];
        sc.g_asg[a + i] = sAsg[i];
      }
    }
  } // longer still: synchronous path (kind stays 0)
  if (lane == 0 && sc.early_park && (d.kind == gr::core::KIND_INSERT_WHOLE || d.kind == gr::core::KIND_INSERT_TRIMMED || d.kind == 0u)) {
    // An insert (or a hand-back) makes every later read of the window stale, whatever the
    // reads before it decide — the host will say so when it reaches this record.
    // Park the window now: all tiles of this and of the earlier reads have been handed out already (in order) and
    // are still processed; nothing new is handed out.
    // (Round 6: what a window that applies inserts itself has in progress behind such a record is FINISHED — it used to be
    // dropped at the next pass — and kept across the insert where the insert changed none of the slots it probed, k_query.
    // Not parking at all was tried: by the time the host's word arrives the dispenser is ~2 800 tiles beyond the read,
    // 1 300 of them finished with their fingerprints gone — more work lost per insert than parking idles away.)
    atomicMin(sc.park, rj + 1u);
    if (sc.ctl == nullptr) {
      atomicMax(sc.next_tile, STREAM_STOP);
    }
    // (a window that applies inserts itself parks by the `park` word alone: a workgroup that draws a tile of a read behind
    // it goes idle — the dispenser itself must stay open, for behind an insert it walks a second time, and a read whose
    // tiles were all kept can be decided, and park the window, while tiles of reads in FRONT of it still wait to be
    // queried again: raising the dispenser then left those reads open for good, found on C2's transition zone)
    __hip_atomic_store(sc.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0) {
    // The record goes to host memory with system-scope stores (no L2 involved); the flag
    // follows once they are acknowledged.  No fence: a system-scope release would write
    // back and invalidate the whole L2 once per read.
    unsigned long long* o = reinterpret_cast<unsigned long long*>(sc.dec + rj);
    __hip_atomic_store(o, (unsigned long long)d.kind | ((unsigned long long)d.num_tiles << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(o + 1, (unsigned long long)d.num_assigned | ((unsigned long long)d.trim_start << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(o + 2, (unsigned long long)d.trim_end | ((unsigned long long)d.hits << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(reinterpret_cast<uint32_t*>(o + 3), d.misses, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // .pad = the generation of the record: 1, or 1 + the inserts this launch has applied itself
    // (records produced before an insert for reads behind it carry an older generation: stale)
    const uint32_t gen = sc.ctl ? ldc(sc.ctl + SCT_GEN) : 1u;
    __builtin_amdgcn_s_waitcnt(0);
    __hip_atomic_store(reinterpret_cast<uint32_t*>(o + 3) + 1, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (sc.ctl) {
      // counted after the park above has been acknowledged: "every read decided and not parked" ends the launch
      __builtin_amdgcn_s_waitcnt(0);
      __hip_atomic_fetch_add(sc.ctl + SCT_DECIDED, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- whole-read insert: the two steps as device functions -------------------------------
// process_read inserts a read as consecutive blocks of `block` tiles, one insertMIBF call
// (= one dedup scope, one ID) per block, in order (goldrush_path.cpp:982-990, 1040-1051).
// Step 1 (collect) gathers, for every distinct rank of the read, the SET of blocks that touch it
// (bit j = block j); step 2 (apply) replays the blocks in ascending order per rank:
// c = ++count; if (uint32(rank ^ id_j) % c == c-1) id = id_j — identical to the sequential
// calls because different ranks never interact.  Used by k_insert_collect / k_insert_apply
// (grp_insert_read: two launches) and, with COH = true, by the workgroups of a streaming
// window that applies an insert itself: everything one workgroup hands to another inside that
// launch, and the ID / count words it writes, moves with agent-scope accesses.
//
// One unit = THREADS frames of one tile (parts units per tile), one frame per lane, all H seeds.
// CLAIM-LOOP RULE (see k_batch_collect, grp_batch.inc): the seeds are walked one at a time, hash first, one claim
// loop per seed.  Guards: tests/test_gpu_batch.py::test_claim_loops_keep_every_touch [read] (k_insert_collect) and
// [stream] (the same unit inside the streaming launch).
template<int H, int WT, bool COH>
__device__ inline void
insert_collect_unit(const DevFilter& f, const DevReads& rd, const DevSeeds* __restrict__ sd, const ulonglong2* sTab, uint32_t* sBases, uint32_t* sWave /* [THREADS / 64 + 1] */, uint32_t tile_len,
                    uint32_t read_idx, uint32_t tile_start, uint32_t block_tiles, const InsertTable& tb, uint32_t* counter, uint32_t unit)
{
  const uint32_t parts = gr::geom::tile_parts(frames_per_tile(sd, tile_len));
  const uint32_t tj = unit / parts; // tile inside the inserted range
  const uint32_t ti = tile_start + tj;
  const uint32_t part = unit % parts;
  const unsigned long long block_bit = 1ull << (tj / block_tiles);
  const uint32_t len = rd.len[read_idx];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, ti);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;

  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[read_idx], len, start, Lp);
  __syncthreads();

  const uint32_t fr = part * THREADS + threadIdx.x;
  const bool live = fr < frames;
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t my_slot[H];
  bool my_claim[H];
  uint32_t n_claimed = 0;
  {
    // Every seed's hash, bucket header and claim loop one after the other: nothing of a seed is
    // live across another seed's claim loop.  (Round 3: the unrolled three-seed form of
    // k_batch_collect, which kept pr[] / hd[] of all seeds in registers across the claim loops in
    // front, lost ~10 % of its third seed's touches — generated code, bisected on C2's filter,
    // profiles/r03_collect3_hunt.txt.  This kernel never showed it, but it had the same shape.)
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (!seed_on<H>(s, hn)) {
        my_claim[s] = false;
        continue;
      }
      Probe pr[H];
      uint4 hd[H];
      {
        const uint32_t fs = min(min(fr, frames ? frames - 1u : 0u), Lp - sd->span[s]);
        pr[s] = grp_locate(f, seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs)));
        hd[s] = f.buckets[pr[s].b * GRP_UNIT_U4]; // rel + bitmap: immutable after grp_finalize
      }
      const uint64_t bm = grp_bitmap(hd[s]);
      const uint32_t lr = grp_local_rank(bm, pr[s].off);
      const uint64_t rank = f.super[pr[s].b >> GRP_SUPER_SHIFT] + hd[s].x + lr;
      const bool valid = live && rank < f.pop && ((bm >> pr[s].off) & 1ull); // see k_insert
      const unsigned long long key = rank + 1;
      uint64_t slot = (key * 0x9E3779B97F4A7C15ULL) >> 20 & tb.cap_mask;
      bool claimed = false;
      if (valid) {
        for (;;) {
          unsigned long long cur = COH ? load_coherent(&tb.keys[slot]) : tb.keys[slot];
          if (cur == 0) {
            cur = atomicCAS(&tb.keys[slot], 0ull, key);
            if (cur == 0) { // claimed: remember where the rank's ID lives
              const unsigned long long loc = grp_id_loc(pr[s].b, lr) | ((unsigned long long)pr[s].off << 58); // (dword 0 of the unit: overflow table)
              if constexpr (COH) {
                store_coherent(&tb.locs[slot], loc);
              } else {
                tb.locs[slot] = loc;
              }
              claimed = true;
              cur = key;
            }
          }
          if (cur == key) {
            break;
          }
          slot = (slot + 1) & tb.cap_mask;
        }
        atomicOr(&tb.masks[slot], block_bit);
      }
      my_slot[s] = (uint32_t)slot;
      my_claim[s] = claimed;
      n_claimed += claimed ? 1u : 0u;
    }
  }
  // the list of claimed slots grows by ONE atomic per workgroup (a counter bumped per wave and
  // seed serialises ~1500 atomics on one address per inserted read, ~11 ns each, measured)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t incl = n_claimed;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
    if (lane >= (uint32_t)o) {
      incl += v;
    }
  }
  if (lane == 63u) {
    sWave[wv] = incl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int w2 = 0; w2 < THREADS / 64; ++w2) {
      const uint32_t v = sWave[w2];
      sWave[w2] = tot;
      tot += v;
    }
    sWave[THREADS / 64] = tot ? atomicAdd(counter, tot) : 0u;
  }
  __syncthreads();
  uint32_t at = sWave[THREADS / 64] + sWave[wv] + incl - n_claimed;
#pragma unroll
  for (int s = 0; s < H; ++s) {
    if (my_claim[s]) {
      if constexpr (COH) {
        stc(&tb.slots[at++], my_slot[s]);
      } else {
        tb.slots[at++] = my_slot[s];
      }
    }
  }
}

// entry i of the claimed-slot list: the rank's blocks replayed in order; the table slot is left clean
template<bool COH>
__device__ inline void
insert_apply_entry(const DevFilter& f, const InsertTable& tb, uint32_t i, uint32_t block_tiles, uint32_t first_id, uint32_t id_offset, uint32_t* changed = nullptr, uint32_t changed_mask = 0)
{
  const uint32_t slot = COH ? ldc(&tb.slots[i]) : tb.slots[i];
  const uint64_t rank = (COH ? load_coherent(&tb.keys[slot]) : tb.keys[slot]) - 1;
  unsigned long long mask = COH ? load_coherent(&tb.masks[slot]) : tb.masks[slot];
  const unsigned long long loc_word = COH ? load_coherent(&tb.locs[slot]) : tb.locs[slot];
  const unsigned long long loc = loc_word & IR_LOC_MASK;
  if constexpr (COH) {
    store_coherent(&tb.keys[slot], 0ull);
    store_coherent(&tb.masks[slot], 0ull);
  } else {
    tb.keys[slot] = 0;
    tb.masks[slot] = 0;
  }
  unsigned long long* cwp = grp_cw_ptr_loc(f, loc, rank);
  const unsigned long long cword = COH ? load_coherent(cwp) : *cwp;
  uint32_t count = grp_cnt(cword);
  uint32_t new_id = 0;
  bool write = false;
  while (mask) {
    const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1u;
    mask &= mask - 1;
    // MIBFConstructSupport.hpp:274-282, block j's call
    ++count;
    const uint32_t id = first_id + (j * block_tiles + id_offset) / block_tiles;
    if ((uint32_t)(rank ^ (uint64_t)id) % count == count - 1u) {
      new_id = id;
      write = true;
    }
  }
  if constexpr (COH) {
    store_coherent(cwp, grp_cnt_with(cword, count));
  } else {
    *cwp = grp_cnt_with(cword, count);
  }
  if (write) {
    uint32_t* p = (loc & (GRP_UNIT_DW - 1u)) ? &reinterpret_cast<uint32_t*>(f.buckets)[loc] : nullptr;
    uint32_t old;
    if constexpr (COH) {
      old = p ? ldc(p) : grp_ovf_get_c(f, rank);
    } else {
      old = p ? *p : grp_ovf_get(f, rank);
    }
    // setData (MIBloomFilter.hpp:593-602): keep a set saturation bit
    const uint32_t nv = (old > 0x80000000u) ? (new_id | 0x80000000u) : new_id;
    if constexpr (COH) {
      if (changed != nullptr && nv != old) { // (round 6) what a query of this slot returns has changed: the window's kept tiles are held against this set
        fp_put(changed, changed_mask, slot_fp(loc / GRP_UNIT_DW, (uint32_t)(loc_word >> 58)));
      }
      if (p) {
        stc(p, nv);
      } else {
        grp_ovf_put_c(f, rank, nv);
      }
    } else {
      if (p) {
        *p = nv;
      } else {
        grp_ovf_put(f, rank, nv);
      }
    }
  }
}

// ---- a streaming window that applies inserts itself (grp_classify_stream_insert) ----------
// The window parks itself at an insert record (stream_decide).  Until round 3 the launch ended
// there: the host queued the insert kernels behind the draining launch and started a new one —
// ~0.5-0.9 ms per insert, 20 % of C2's steady state.  Now the workgroups that run out of tiles
// stay: the host posts the insert (read, tiles, the block IDs it allocated) in mapped memory, a
// relay workgroup copies it to the control block, ALL workgroups collect the read's ranks, wait
// for each other, replay them, reset the window behind the read (tile counters, dispenser,
// generation of the records) and carry on with the next read — no launch boundary.
//
// Coherence: the insert's own hand-overs and the ID / count words use agent-scope (write-through)
// accesses, acknowledged (s_waitcnt) before a workgroup arrives at a grid-wide wait; behind the
// second wait every workgroup issues one acquire fence (buffer_inv: its CU's vector cache and its
// XCD's L2 drop their clean lines), so the plain bucket loads of the queries that follow see the new IDs.  Both waits need
// every workgroup of the grid resident (it is sized from the occupancy query); the first one has
// a time limit — until it has passed only the scratch table was touched, and the host applies the
// insert the classic way when it fails.
constexpr uint32_t STREAM_ACT_EXIT = 0, STREAM_ACT_INSERT = 1;

__device__ inline uint32_t
load_host(const uint32_t* p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// `invalidate`: the workgroup drops its CU's vector cache and its XCD's clean L2 lines behind the
// wait (one wave issues the buffer_inv; 4096 waves doing it cost ~100 us per insert, measured).
// Everything handed over at these waits was written with agent-scope (write-through) stores or
// atomics: a wave only has to see them acknowledged (s_waitcnt) before its workgroup arrives.
__device__ inline bool
stream_grid_wait(const DevStreamCtl& sc, uint32_t k, uint32_t* sFlag, bool invalidate, uint32_t members, uint32_t* bar, uint32_t* rank = nullptr)
{
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t a = __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *sFlag = (a << 1) | (a + 1u == members ? 1u : 0u);
  }
  __syncthreads();
  const uint32_t arrived = *sFlag;
  if (rank) {
    *rank = arrived >> 1; // the order of arrival: this insert's number of the workgroup (its share of the strided loops)
  }
  // Round 6: every workgroup waits on a release word OF ITS OWN (a 128-byte line each, sc.rel), written by all lanes of
  // the workgroup that arrived last.  The 16 words per group of rounds 3 - 5 were polled by every waiting workgroup: an
  // insert of three tiles into a parked window brings 750 workgroups to the wait within a microsecond.
  // The wait is for the insert's MEMBERS — the workgroups that had begun when its event was published — not for the
  // grid: now and then a workgroup or two of a launch sized to what the device holds begin only when others leave (C2:
  // two windows in 3 487, the last workgroups of one XCD; a cooperative launch does not prevent it), and an insert
  // that waited for them waited for its time limit.
  if ((arrived & 1u) != 0u) {
    for (uint32_t w = threadIdx.x; w < gridDim.x; w += THREADS) {
      stc(sc.rel + (size_t)w * 32u, k);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    uint32_t ok = 1u, spins = 0;
    const uint32_t* mine = sc.rel + (size_t)blockIdx.x * 32u;
    while ((int32_t)(ldc(mine) - k) < 0) {
      __builtin_amdgcn_s_sleep(4);
      if ((++spins & 0x3FFu) == 0u) {
        if (ldc(sc.ctl + SCT_ERR) != 0u || wall_clock64() - t0 > sc.timeout_ticks) {
          if (ldc(sc.ctl + SCT_ERR) == 0u) { // the first one to give up: which wait, who, how many had come of how many (the host's message)
            __hip_atomic_store(sc.ack_host + ACK_GAVE_UP_WHO, (k & 0xFFFFu) | (blockIdx.x << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(sc.ack_host + ACK_GAVE_UP_COUNT, (members << 16) | (ldc(bar) & 0xFFFFu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          }
          stc(sc.ctl + SCT_ERR, 1u);
          ok = 0u;
          break;
        }
      }
    }
    if (ok != 0u && ldc(sc.ctl + SCT_ERR) != 0u) {
      ok = 0u; // somebody gave this wait up (and left) before the last one arrived: nobody goes on as if it had held
    }
    *sFlag = ok;
    if (invalidate) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __builtin_amdgcn_s_waitcnt(0); // the other waves are released by the barrier below: not before the invalidate is through
    }
  }
  __syncthreads();
  return *sFlag != 0u;
}

// thread 0 of a workgroup of a resumable window, before it draws its first tile: it is one of the launch's workgroups
// from here on — the inserts published from now on wait for it.  An insert in progress does not (its members were
// counted when its event was published): the workgroup stays out until that insert is through, and picks up the
// event word and the number of waits behind it.  false: the launch is ending (exit event, a wait that timed out).
constexpr uint32_t STREAM_ALIVE_LOCK = 0x80000000u;
constexpr uint32_t STREAM_ALIVE_INS = 0x7FFFF000u;
__device__ inline bool
stream_register(const DevStreamCtl& sc, uint32_t* my_ev, uint32_t* phase)
{
  bool ok = true;
  const uint32_t v = __hip_atomic_fetch_add(sc.ctl + SCT_ALIVE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((v & STREAM_ALIVE_LOCK) != 0u) {
    const unsigned long long t0 = wall_clock64();
    uint32_t spins = 0;
    for (;;) {
      const uint32_t a = ldc(sc.ctl + SCT_ALIVE);
      if ((a & STREAM_ALIVE_LOCK) == 0u || ((a ^ v) & STREAM_ALIVE_INS) != 0u) {
        break;
      }
      __builtin_amdgcn_s_sleep(32);
      if ((++spins & 0xFFu) == 0u && ((ldc(sc.ctl + SCT_EVENT) & 1u) != 0u || ldc(sc.ctl + SCT_ERR) != 0u || wall_clock64() - t0 > 16ull * sc.timeout_ticks)) {
        ok = false;
        break;
      }
    }
  }
  *my_ev = ldc(sc.ctl + SCT_DONE);
  *phase = ldc(sc.ctl + SCT_DONE + 1);
  return ok;
}

// relay (thread 0 of the first 32 workgroups, whenever one of them has nothing to draw): host
// flags -> event word.  (insert commands seen << 1) | exit; whoever advances the master word
// hands the new value to the 16 group copies the idle workgroups poll.
__device__ inline void
stream_relay(const DevStreamCtl& sc)
{
  const uint32_t ev = ldc(sc.ctl + SCT_EVENT);
  if (ev & 1u) {
    return;
  }
  uint32_t nev = ev;
  if (load_host(sc.abort_host)) {
    // the host has consumed every record it wants: nothing is needed any more
    atomicMin(sc.park, 0u);
    atomicMax(sc.next_tile, STREAM_STOP);
    stc(sc.abort, 1u);
    nev = ev | 1u;
  } else {
    const uint32_t hseq = load_host(sc.cmd_host + CMD_SEQ);
    if (hseq != (ev >> 1)) {
      __builtin_amdgcn_s_waitcnt(0);
      uint32_t w[CMD_N_FIELDS];
#pragma unroll
      for (int i = 0; i < (int)CMD_N_FIELDS; ++i) {
        w[i] = load_host(sc.cmd_host + CMD_FIELDS + i);
      }
      __builtin_amdgcn_s_waitcnt(0);
      if (load_host(sc.cmd_host + CMD_SEQ) == hseq) {
        // A striped window: the inserting read may lie in another rank's stripe (this launch knows nothing of it) — every
        // read of the window up to it has been decided by its owner (the ranks have exchanged those records), so nothing
        // this launch still holds in front of it is needed, and everything behind it is held against the insert.
        // (round 6: the command parks nothing — every workgroup takes the event behind the tile it is in, applies the
        // insert and holds the tiles it keeps of the reads behind it against the slots the insert changed)
#pragma unroll
        for (int i = 0; i < (int)CMD_N_FIELDS; ++i) {
          stc(sc.ctl + SCT_CMD + i, w[i]);
        }
        __builtin_amdgcn_s_waitcnt(0);
        nev = hseq << 1;
      }
    } else if (!sc.cmd_while_busy && ldc(sc.park) == 0xFFFFFFFFu) {
      // (a striped window stays when its own stripes are decided: the read that inserts next may be another rank's,
      // and a launch that had left before the command came would cost every rank its window — the host ends it,
      // grp_classify_stream_abort, when it has committed the window's last read)
      const uint32_t d = ldc(sc.ctl + SCT_DECIDED);
      __builtin_amdgcn_s_waitcnt(0);
      if (d >= sc.n_decidable && ldc(sc.park) == 0xFFFFFFFFu) {
        nev = ev | 1u; // every read decided, none of them an insert: the window is complete
      }
    }
  }
  if (nev != ev && atomicCAS(sc.ctl + SCT_EVENT, ev, nev) == ev) {
    if ((nev & 1u) == 0u) {
      // an insert: its members are the workgroups that have begun by now (stream_register); the counters of the insert
      // after it (the other parity's: the insert before this one is through, the host has its answer)
      const uint32_t par = (nev >> 1) & 1u;
      stc(sc.ctl + SCT_UNIT + (par ^ 1u), 0u);
      stc(sc.ctl + SCT_APPLY + (par ^ 1u), 0u);
      stc(sc.ctl + SCT_IRCOUNT + (par ^ 1u), 0u);
      stc(sc.ctl + SCT_BAR + ((par ^ 1u) * 2u) * 32u, 0u);
      stc(sc.ctl + SCT_BAR + ((par ^ 1u) * 2u + 1u) * 32u, 0u);
      const uint32_t members = __hip_atomic_fetch_add(sc.ctl + SCT_ALIVE, STREAM_ALIVE_LOCK + 0x1000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xFFFu;
      stc(sc.ctl + SCT_MEMBERS, members);
      __builtin_amdgcn_s_waitcnt(0);
    }
    const uint32_t ng = min(SCT_GROUPS, gridDim.x);
    for (uint32_t i = 0; i < ng; ++i) {
      stc(sc.ctl + SCT_EV + i * 32u, nev);
    }
  }
}

// thread 0 of a workgroup with nothing to draw: wait for the next event; *my_ev is the last one acted on
__device__ inline uint32_t
stream_idle(const DevStreamCtl& sc, uint32_t* my_ev)
{
  const uint32_t ng = min(SCT_GROUPS, gridDim.x);
  const uint32_t g = blockIdx.x % ng;
  const unsigned long long t0 = wall_clock64();
  uint32_t spins = 0;
  for (;;) {
    const uint32_t ev = ldc(sc.ctl + SCT_EV + g * 32u);
    if (ev != *my_ev) {
      *my_ev = ev;
      return (ev & 1u) ? STREAM_ACT_EXIT : STREAM_ACT_INSERT;
    }
    if (blockIdx.x < 32u) {
      stream_relay(sc);
    }
    __builtin_amdgcn_s_sleep(64); // (~2 us: a parked launch's hundreds of idle workgroups poll 16 words — not at the rate that starves the ones still in a tile)
    if ((++spins & 0xFFFu) == 0u && wall_clock64() - t0 > 16ull * sc.timeout_ticks) {
      // nobody came for the parked window (a host that died?): never hang the device
      // what the launch was waiting on, for the host's error message
      __hip_atomic_store(sc.ack_host + ACK_IDLE_PARK, ldc(sc.park), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(sc.ack_host + ACK_IDLE_DECIDED, ldc(sc.ctl + SCT_DECIDED), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(sc.ack_host + ACK_IDLE_NEXT_TILE, ldc(sc.next_tile), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(sc.ack_host + ACK_IDLE_EVENT, ldc(sc.ctl + SCT_EVENT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(sc.ack_host + ACK_IDLE_CMD_SEQ, load_host(sc.cmd_host + CMD_SEQ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(sc.ack_host + ACK_IDLE_GEN, ldc(sc.ctl + SCT_GEN), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_s_waitcnt(0);
      __hip_atomic_store(sc.ack_host + ACK_CODE, (uint32_t)ACK_CODE_IDLE_EXIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return STREAM_ACT_EXIT;
    }
  }
}

// what an in-launch insert leaves for the workgroups that carry on behind it
struct StreamInsertDone
{
  uint32_t resume_read = 0; // window index of the first read behind the inserted one
  uint32_t resume_tile = 0; // this launch's first tile behind it (dispenser position)
  uint32_t gen = 0;         // generation of the records from here on
  uint32_t scan_end = 0;    // dispenser position the insert found, STREAM_FULL_RESET: everything behind the read is handed out again
  uint32_t par = 0;         // which changed-slot set (sc.fp_tab) is this insert's
  uint32_t rank = 0;        // this workgroup's number among the insert's members (order of arrival at its first wait)
};

// all threads of every workgroup: the insert the event word announces.  false: a wait timed out.
template<int H, int WT>
__device__ inline bool
stream_apply_insert(const DevFilter& f, const DevReads& rd, const DevSeeds* __restrict__ sd, const ulonglong2* sTab, uint32_t* sBases, uint32_t* sWave, uint32_t* sFlag, uint32_t tile_len,
                    const DevStreamCtl& sc, uint32_t ev, uint32_t& phase, unsigned long long* ctr, uint64_t lists_cap, const uint32_t* __restrict__ tile_idx, StreamInsertDone& done)
{
  const uint32_t* cmd = sc.ctl + SCT_CMD;
  const uint32_t read_idx = ldc(cmd + CMD_READ), tile_start = ldc(cmd + CMD_TILE_START), tile_end = ldc(cmd + CMD_TILE_END), block_tiles = ldc(cmd + CMD_BLOCK_TILES);
  const uint32_t first_id = ldc(cmd + CMD_FIRST_ID), id_offset = ldc(cmd + CMD_ID_OFFSET), resume_read = ldc(cmd + CMD_RESUME_READ), resume_tile = ldc(cmd + CMD_RESUME_TILE);
  const uint32_t decided_base = ldc(cmd + CMD_DECIDED_BASE), gen = ldc(cmd + CMD_GEN);
  const uint32_t par = (ev >> 1) & 1u;
  const uint32_t members = ldc(sc.ctl + SCT_MEMBERS); // the workgroups this insert waits for (those that had begun when it was published)
  uint32_t* const bar = sc.ctl + SCT_BAR + (par * 2u) * 32u;
  const uint32_t parts = gr::geom::tile_parts(frames_per_tile(sd, tile_len));
  const uint32_t n_units = (tile_end - tile_start) * parts;
  const unsigned long long t_enter = wall_clock64(); // workgroup 0 leaves the phase times of the insert for the host's trace
  // collect
  for (;;) {
    __syncthreads(); // sWave / sBases of the previous unit are free
    if (threadIdx.x == 0) {
      sWave[THREADS / 64] = __hip_atomic_fetch_add(sc.ctl + SCT_UNIT + par, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const uint32_t u = sWave[THREADS / 64];
    __syncthreads();
    if (u >= n_units) {
      break;
    }
    if (threadIdx.x == 0 && sc.dbg) {
      stc(&sc.dbg[blockIdx.x], 0x40000000u | ((u & 0xFFFu) << 16) | (ev & 0xFFFFu));
    }
    insert_collect_unit<H, WT, true>(f, rd, sd, sTab, sBases, sWave, tile_len, read_idx, tile_start, block_tiles, sc.tb, sc.ctl + SCT_IRCOUNT + par, u);
  }
  const unsigned long long t_collect_own = wall_clock64();
  if (threadIdx.x == 0 && sc.dbg) {
    stc(&sc.dbg[blockIdx.x], 0x50000000u | ((phase & 0xFFFu) << 16) | (ev & 0xFFFFu));
    stc(&sc.dbg[2048 + (blockIdx.x & 1023u)], (uint32_t)wall_clock64()); // when it reached the first wait
  }
  uint32_t rank = 0;
  if (!stream_grid_wait(sc, ++phase, sFlag, false, members, bar, &rank)) {
    if (threadIdx.x == 0) { // nothing but the scratch table was touched: the host applies the insert (every workgroup says so: the same word)
      __hip_atomic_store(sc.ack_host + ACK_CODE, (uint32_t)ACK_CODE_NOT_APPLIED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return false;
  }
  const unsigned long long t_collected = wall_clock64();
  // apply; the ID slots whose value changes go into this insert's set (round 6)
  uint32_t* const changed = sc.n_fp ? sc.fp_tab[par] : nullptr;
  const uint32_t n = ldc(sc.ctl + SCT_IRCOUNT + par);
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) {
      sWave[THREADS / 64] = __hip_atomic_fetch_add(sc.ctl + SCT_APPLY + par, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const uint32_t i = sWave[THREADS / 64] * THREADS + threadIdx.x;
    if (i - threadIdx.x >= n) {
      break;
    }
    if (i < n) {
      insert_apply_entry<true>(f, sc.tb, i, block_tiles, first_id, id_offset, changed, sc.fp_mask);
    }
  }
  if (sc.n_fp) {
    // the set of the insert before this one: every workgroup held its tiles against it before it came here — cleaned for
    // the insert after this one (write-through stores: the next fill goes through the memory side)
    unsigned long long* old = reinterpret_cast<unsigned long long*>(sc.fp_tab[par ^ 1u]);
    const uint32_t n2 = (sc.fp_mask + 1u) / 2u;
    for (uint32_t i = rank * THREADS + threadIdx.x; i < n2; i += members * THREADS) {
      store_coherent(&old[i], 0ull);
    }
  }
  // the reads behind the inserted one are counted (and decided) again: tile counters, and (one lane) park, generation
  for (uint32_t j = resume_read + rank * THREADS + threadIdx.x; j < sc.n_reads; j += members * THREADS) {
    stc(&sc.tiles_done[j], 0u);
  }
  if (rank == 0u && threadIdx.x == 0) {
    uint32_t at = ldc(sc.next_tile);
    at = max(at >= STREAM_STOP ? 0u : at, ldc(sc.ctl + SCT_FRONTIER)); // the furthest the dispenser ever stood (parked: recorded then)
    stc(sc.ctl + SCT_FRONTIER, at);
    at = min(at, sc.n_tiles);
    if (sc.n_fp == 0u || load_coherent(&ctr[QCTR_LIST_CURSOR]) > (lists_cap / 4u) * 3u) {
      // Nothing is kept (no room for fingerprints in this geometry's LDS; or the list arena, which kept tiles pin, is
      // three quarters full): everything behind the read is queried again, the form of rounds 3 - 5.  The list arena
      // starts over with it: every read up to the inserted one has been decided (the lists of its tiles are dead).
      store_coherent(&ctr[QCTR_LIST_CURSOR], 0ull);
      stc(sc.ctl + SCT_SCAN_END, STREAM_FULL_RESET | at);
    } else {
      stc(sc.ctl + SCT_SCAN_END, at);
    }
    // The dispenser walks the tiles behind the read again, in order, in either form: a workgroup that draws one looks
    // at its mark (k_query) — kept under the new generation, held or worked on by somebody: the next one; handed out
    // under the old state and nobody's any more (finished, its fingerprints gone): queried again.
    stc(sc.next_tile, resume_tile);
    stc(sc.ctl + SCT_DECIDED, decided_base);
    stc(sc.ctl + SCT_GEN, gen);
    stc(sc.park, 0xFFFFFFFFu);
    stc(sc.abort, 0u);
  }
  const unsigned long long t_apply_own = wall_clock64();
  if (!stream_grid_wait(sc, ++phase, sFlag, true, members, bar + 32)) {
    if (threadIdx.x == 0) {
      __hip_atomic_store(sc.ack_host + ACK_CODE, (uint32_t)ACK_CODE_WAIT_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return false;
  }
  if (rank == 0u && threadIdx.x == 0) {
    // the insert is through: a workgroup that begins from here on is a member of the next one (before the host is told
    // — its next command finds the word open)
    stc(sc.ctl + SCT_DONE, ev);
    stc(sc.ctl + SCT_DONE + 1, phase);
    __builtin_amdgcn_s_waitcnt(0);
    (void)__hip_atomic_fetch_and(sc.ctl + SCT_ALIVE, ~STREAM_ALIVE_LOCK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    __hip_atomic_store(sc.ack_host + ACK_PHASE + 0, (uint32_t)(t_collect_own - t_enter), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(sc.ack_host + ACK_PHASE + 1, (uint32_t)(t_collected - t_collect_own), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(sc.ack_host + ACK_PHASE + 2, (uint32_t)(t_apply_own - t_collected), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(sc.ack_host + ACK_PHASE + 3, (uint32_t)(wall_clock64() - t_apply_own), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_s_waitcnt(0);
    __hip_atomic_store(sc.ack_host + ACK_APPLIED, ev >> 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  done.resume_read = resume_read;
  done.resume_tile = resume_tile;
  done.gen = gen;
  done.scan_end = ldc(sc.ctl + SCT_SCAN_END);
  done.par = par;
  done.rank = rank;
  return true;
}

// ---- versioned view of the ID array (grp_batch_*, csrc/grp_batch.inc) ---------------------
// A batch of consecutive reads has been inserted AHEAD of their own queries; read j must see
// the state in front of its own insert.  IDs grow with the read order, so a probe whose ID is
// below floor[j] (the first ID read j could allocate) is untouched by reads >= j.  Otherwise
// the batch's log decides: every write that replaced a non-zero ID, and every write to a rank
// written more than once in the batch, is logged as {old value, writing read}; the view of
// read j is the old value of the earliest logged write by a read >= j, or 0 (an unlogged
// first write into an empty slot).
struct DevBatchView
{
  const uint32_t* floor = nullptr;          // [reads queried], from read floor_first on
  uint32_t floor_first = 0;                 // batch index of the first read queried
  // grp_batch_verify: tiles the batch inserted are patched from its records by k_batch_delta — the query skips them
  const uint32_t* skip_read_ins = nullptr;  // [skip_reads] per read of the window its entry in `ins`, BATCH_NONE: none; NULL: nothing is skipped
  uint32_t skip_reads = 0;
  uint32_t first = 0;                       // batch index of the WINDOW's first read: reads are numbered from here in the log
  // what the batch's collect pass left: rank -> record of the rank's owner, in the rank's count word
  // (grp_device.h: the claim is the batch's if the word carries the batch's epoch); the views name a rank's word by
  // bucket * 64 + (its set bit's index inside the bucket)
  const unsigned long long* units = nullptr; // f.buckets as 64-bit words
  const ulonglong2* far = nullptr;
  uint64_t far_mask = 0;
  uint32_t epoch = 0;
  uint64_t bits_mask = 0;
  const uint32_t* bits = nullptr;           // 1 bit per hash slot: a rank with this home slot has something to restore
  const unsigned long long* rec_old = nullptr; // per record: wrote << 63 | count before << 32 | ID before the batch
  const uint32_t* rec_chain = nullptr;      // BATCH_NONE: the owner's touch is the rank's only one
  const unsigned long long* rec_key = nullptr; // low 26 bits: insert of the batch << 8 | ID block
  const uint32_t* ins = nullptr;            // [inserts][6], [0] = the read
  // ranks touched more than once: the log of their writes
  const unsigned long long* log_keys = nullptr; // open addressing: rank + 1
  const uint32_t* log_head = nullptr;       // per table slot: newest entry of the rank's chain
  const uint32_t* log_old = nullptr;
  const uint32_t* log_writer = nullptr;     // read index inside the window
  const uint32_t* log_next = nullptr;
  uint64_t log_mask = 0;
  // a launch over a tile list whose length only the device knows yet (the tiles a batch's patch gave up, redone behind
  // the patch without a round trip to the host): workgroups beyond *redo_count leave at once
  const unsigned long long* redo_count = nullptr;
};

constexpr uint32_t BATCH_NONE = 0xFFFFFFFFu;

// What read `reader` of the window sees at a rank that holds `cur`, an ID >= the first one
// `reader` could allocate: the value in front of the earliest write by a read >= reader.  IDs grow
// with the read order, but the LAST ID block of a trimmed read can carry the ID the next
// inserting read starts with (goldrush_path.cpp:1048-1049 numbers the blocks of a trimmed read
// from (0 + 1) / block_size, :1074 advances by (end - start) / block_size): an ID equal to the
// floor may have been written in front of `reader` — then the rank has no write by a read >=
// reader and `cur` stands.  `ambiguous`: cur is such an ID (the caller says where that can be).
__device__ inline uint32_t batch_view_log(const DevBatchView& bv, unsigned long long key, uint32_t reader, uint32_t cur);

// the count word of the lr-th set bit of bucket b (grp_cw_ptr on the view's copy of the filter's pointers)
__device__ inline unsigned long long
batch_view_cw(const DevBatchView& bv, uint64_t bl, uint64_t rank)
{
  const uint32_t lr = (uint32_t)(bl & 63ull);
  if (lr < GRP_NEAR_CW) {
    return bv.units[(bl >> 6) * GRP_UNIT_QW + 8u + lr];
  }
  uint64_t slot = ((rank + 1) * 0x9E3779B97F4A7C15ULL) >> 19 & bv.far_mask;
  for (;;) {
    const ulonglong2 e = bv.far[slot];
    if (e.x == rank + 1) {
      return e.y;
    }
    if (e.x == 0) {
      return 0ull; // (unreachable: the far table is complete)
    }
    slot = (slot + 1) & bv.far_mask;
  }
}

__device__ inline uint32_t
batch_view(const DevBatchView& bv, uint64_t rank, uint64_t bl, uint32_t reader, uint32_t cur, bool ambiguous)
{
  const unsigned long long key = rank + 1;
  const uint64_t slot = (key * 0x9E3779B97F4A7C15ULL) >> 20 & bv.bits_mask;
  const bool hint = (bv.bits[slot >> 5] >> (slot & 31u) & 1u) != 0u;
  if (!hint && !ambiguous) {
    return 0u; // most probes of an inserting read: its own writes into empty slots
  }
  const unsigned long long w = batch_view_cw(bv, bl, rank);
  if (grp_claim_epoch(w) != bv.epoch) {
    return cur; // not a rank of the batch
  }
  const uint32_t idx = grp_claim_record(w);
  if (bv.rec_chain[idx] == BATCH_NONE) {
    // one touch, its owner's
    const uint32_t j = (uint32_t)(bv.rec_key[idx] & ((1ull << 26) - 1ull)) >> 8;
    const uint32_t writer = bv.ins[(size_t)j * 6] - bv.first;
    return (writer >= reader && (bv.rec_old[idx] >> 63)) ? (uint32_t)bv.rec_old[idx] : cur;
  }
  return batch_view_log(bv, key, reader, cur);
}

// the H probes of one frame at once: the same answers as batch_view, but the loads of a stage are
// issued for all seeds before any is consumed (hint words; table slots; the three record words) —
// the look-ups are chains of dependent loads, and a lane that walks them seed after seed waits
// H times as long (the second query of a batch spent ~40 % of its time there)
template<int H>
__device__ inline void
batch_view_multi(const DevBatchView& bv, const uint64_t (&rank)[H], const uint64_t (&bl)[H], const bool (&need)[H], const bool (&amb)[H], uint32_t reader, uint32_t (&d)[H])
{
  uint64_t slot[H];
  uint32_t hw[H];
#pragma unroll
  for (int s = 0; s < H; ++s) {
    slot[s] = ((rank[s] + 1) * 0x9E3779B97F4A7C15ULL) >> 20 & bv.bits_mask;
    hw[s] = need[s] ? bv.bits[slot[s] >> 5] : 0u;
  }
  bool look[H];
  unsigned long long k[H];
#pragma unroll
  for (int s = 0; s < H; ++s) {
    look[s] = need[s] && ((((hw[s] >> (slot[s] & 31u)) & 1u) != 0u) || amb[s]);
    if (need[s] && !look[s]) {
      d[s] = 0u; // most probes of an inserting read: its own writes into empty slots
    }
    k[s] = look[s] ? batch_view_cw(bv, bl[s], rank[s]) : 0ull;
  }
  bool have[H];
  uint32_t idx[H];
#pragma unroll
  for (int s = 0; s < H; ++s) {
    have[s] = look[s] && grp_claim_epoch(k[s]) == bv.epoch; // else not a rank of the batch: the ID stands
    idx[s] = grp_claim_record(k[s]);
  }
  uint32_t chain[H];
  unsigned long long rk[H], ro[H];
#pragma unroll
  for (int s = 0; s < H; ++s) {
    chain[s] = have[s] ? bv.rec_chain[idx[s]] : BATCH_NONE;
    rk[s] = have[s] ? bv.rec_key[idx[s]] : 0ull;
    ro[s] = have[s] ? bv.rec_old[idx[s]] : 0ull;
  }
#pragma unroll
  for (int s = 0; s < H; ++s) {
    if (have[s]) {
      if (chain[s] == BATCH_NONE) {
        const uint32_t j = (uint32_t)(rk[s] & ((1ull << 26) - 1ull)) >> 8;
        const uint32_t writer = bv.ins[(size_t)j * 6] - bv.first;
        d[s] = (writer >= reader && (ro[s] >> 63)) ? (uint32_t)ro[s] : d[s];
      } else {
        d[s] = batch_view_log(bv, rank[s] + 1, reader, d[s]);
      }
    }
  }
}

// a rank touched more than once: what `reader` sees is in the log of its writes
__device__ inline uint32_t
batch_view_log(const DevBatchView& bv, unsigned long long key, uint32_t reader, uint32_t cur)
{
  uint64_t slot = (key * 0x9E3779B97F4A7C15ULL) >> 18 & bv.log_mask;
  for (;;) {
    const unsigned long long k = bv.log_keys[slot];
    if (k == key) {
      break;
    }
    if (k == 0) {
      return cur; // touched, never written
    }
    slot = (slot + 1) & bv.log_mask;
  }
  uint32_t best_w = BATCH_NONE, best_old = cur;
  for (uint32_t e = bv.log_head[slot]; e != BATCH_NONE; e = bv.log_next[e]) {
    const uint32_t w = bv.log_writer[e];
    if (w >= reader && w <= best_w) { // newest first: of one writer's entries the OLDEST holds what was there before it
      best_w = w;
      best_old = bv.log_old[e];
    }
  }
  return best_old;
}

template<int H, int FR, int WT, bool ST, bool VER = false, bool GT = false>
__global__ void __launch_bounds__(THREADS, (ST && H <= 3) ? 3 : ((!ST && H >= 4 && H <= 5) ? 3 : 1)) // the persistent form at h <= 3: three workgroups per CU is what it is launched at (launch_query; round 6: it was compiled for four — 128 VGPRs, a few of them in scratch — while never more than three ran); the synchronous forms at h = 4, 5: three workgroups per CU (<= 168 VGPRs) —
                                                                                              // the second query of a batch at h = 5 -13 % (its look-ups behind ID >= floor are latency: occupancy helps)
k_query(DevFilter f,
        DevReads rd,
        const DevSeeds* __restrict__ sd,
        uint32_t tile_len,
        uint64_t tile_begin,
        const uint32_t* __restrict__ tile_idx, // NULL: tile = tile_begin + blockIdx.x
        uint32_t hist_cap,       // slots of the per-tile count table (even)
        uint32_t distinct_limit,
        grp_tile_summary* __restrict__ tiles_out,
        grp_id_count* __restrict__ lists_out,
        uint64_t lists_cap,
        unsigned long long* __restrict__ ctr,
        uint32_t* __restrict__ flagged_out, // indices of flagged tiles (NULL in the redo launch)
        uint32_t flagged_cap,
        uint32_t direct_stride, // != 0: tile i owns lists_out[i*stride ..) (no arena, no counters:
                                // small windows write straight into mapped host memory)
        uint32_t blk0,          // synchronous forms without a tile list: workgroup i takes tile blk0 + i of the window
        DevStreamCtl sc,        // ST only
        DevBatchView bv,        // VER only
        uint32_t* __restrict__ gtab = nullptr) // GT only: the count tables in global memory, hist_cap * 3 / 2 words per workgroup of the launch
{
  if constexpr (VER && !ST) {
    if (bv.redo_count != nullptr && blockIdx.x >= *bv.redo_count) {
      return;
    }
  }
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  // GT (round 5): the worst-case table of a geometry whose tile x h IDs do not fit the LDS (tiles beyond ~9 000 frames at h = 3)
  // lives in a slice of a global scratch area — only the redo of the tiles the first step's LDS-sized table could not hold
  // runs this form: same arithmetic, atomics at the L2 instead of the LDS
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t* sKeys;
  uint32_t* sCnts;
  uint32_t* sBases;
  if constexpr (GT) {
    sKeys = gtab + (size_t)blockIdx.x * (hist_cap + hist_cap / 2u);
    sCnts = sKeys + hist_cap;
    sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);
  } else {
    sKeys = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);
    sCnts = sKeys + hist_cap; // 16-bit counts, two per word
    sBases = sCnts + hist_cap / 2u;
  }
  auto tab_word = [&](const uint32_t* p) -> uint32_t { // (GT: what the other waves' atomics left at the L2, not a line this CU may hold)
    if constexpr (GT) {
      return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      return *p;
    }
  };
  __shared__ uint32_t sListN, sDistinct, sOverflow, sListOff, sListW;
  __shared__ uint32_t sRed[2 * (THREADS / 64)];
  __shared__ uint32_t sBest[2 * (THREADS / 64)];
  __shared__ uint32_t sTile;
  __shared__ unsigned long long sDirectWord;
  __shared__ uint32_t sInsWave[THREADS / 64 + 1]; // ST: scratch of an in-launch insert
  __shared__ uint32_t sEv, sAct;                  // ST: event this workgroup acts on / what to do
  // ST, a window that applies inserts itself (round 6): what this workgroup holds across one
  __shared__ uint32_t sHeldTile[2], sHeldPasses[2]; // per fingerprint buffer: the FINISHED tile whose probes it holds (window index; STREAM_REDO_NONE: none) and its passes
  __shared__ uint32_t sBuf;                       // the buffer of the tile in progress
  __shared__ uint32_t sCut;                       // the tile in progress was cut short (a parked window that keeps nothing): its summary is not a whole tile's
  __shared__ uint32_t sOwnRedo[2], sOwnRedoN;     // held tiles an insert touched: this workgroup queries them again itself, before it draws
  __shared__ uint32_t sWalkEnd;                   // dispenser positions below this were handed out before the last insert: their tiles carry marks
  __shared__ uint32_t sGen;                       // the generation of the records (1 + the inserts this launch has applied)

  load_tab(sTab, sd);
  // ST: persistent workgroups (one launch fills the device once) draw tile after tile
  // from a dispenser, in window order; an abort parks the dispenser beyond the last
  // tile, so a stale window ends as soon as the resident tiles are done.  The next
  // index is fetched while the current tile is being processed.
  uint32_t nxt = 0;
  uint32_t stop = 0; // thread 0: the device abort flag, read while the previous tile was finishing
  uint32_t my_ev = 0;   // thread 0: the last event of the control block this workgroup acted on
  uint32_t phase = 0;   // grid-wide waits passed (the same in every workgroup)
  bool host_abort_seen = false; // thread 0
  uint32_t ev_next = 0; // thread 0: its group's copy of the event word, asked for while the previous tile was finishing (a coherent load: its latency lies behind the tile's way out)
  uint32_t pending_event = 0;   // ST, uniform: nothing to draw, or news in the event word — the event is taken at the top of the loop
  uint32_t* const sFp = (ST && sc.ctl && sc.n_fp) ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(smem4) + sc.fp_off) : nullptr;
  if constexpr (ST) {
    if (threadIdx.x == 0) {
      sHeldTile[0] = sHeldTile[1] = STREAM_REDO_NONE;
      sHeldPasses[0] = sHeldPasses[1] = 0u;
      sBuf = 0u;
      sCut = 0u;
      sOwnRedoN = 0u;
      sWalkEnd = 0u;
      sGen = 1u;
      if (sc.dbg) {
        stc(&sc.dbg[blockIdx.x], 0x00000001u);
        stc(&sc.dbg[4095], gridDim.x);
        stc(&sc.dbg[4096 + (blockIdx.x & 1023u)], (uint32_t)wall_clock64()); // when it began
        stc(&sc.dbg[5120 + (blockIdx.x & 1023u)], (__builtin_amdgcn_s_getreg((16 - 1) << 11 | 4) & 0xFFFFu) | (__builtin_amdgcn_s_getreg((4 - 1) << 11 | 20) << 16)); // HW_ID[15:0] | XCC_ID << 16: where
      }
      // a window that was aborted before it started (the host read an insert out of the
      // previous launch) must not begin a single tile: every workgroup asks the host
      // flag once, here — one PCIe read per workgroup and launch
      if (__hip_atomic_load(sc.abort_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
        atomicMin(sc.park, 0u);
        atomicMax(sc.next_tile, STREAM_STOP);
        __hip_atomic_store(sc.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stop = 1u;
        host_abort_seen = true;
      }
      if (sc.ctl) {
        // one of the launch's workgroups from here on: inserts published from now on wait for it (not one in progress)
        uint32_t ph0 = 0;
        if (!stream_register(sc, &my_ev, &ph0)) {
          stop = 1u;
          host_abort_seen = true;
        }
        sEv = ph0;
        sGen = ldc(sc.ctl + SCT_GEN);
        sWalkEnd = ldc(sc.ctl + SCT_SCAN_END) & ~STREAM_FULL_RESET;
        ev_next = my_ev;
      }
      nxt = atomicAdd(sc.next_tile, 1u);
    }
    if (sc.ctl) {
      __syncthreads();
      phase = sEv;
    }
  }
  for (;;) {
  uint32_t out_idx;
  if constexpr (ST) {
    if (__builtin_expect(pending_event != 0u, 0)) {
      // ---- the host's word: leave, or the insert it has committed (round 3), applied by every workgroup of the launch ----
      // Round 6: what this workgroup holds of the reads behind the inserted one when the insert comes — the last two tiles
      // it has finished, fingerprints of their probes' ID slots in LDS — is held against the slots the insert changed:
      // clean tiles stand, dirty ones are queried again (stream_apply_insert; DESIGN 5a).  A workgroup takes the event
      // between two tiles (round 6 tried between two passes as well, the tile suspended and resumed: the same rates and
      // times on C1 and C2, and its state in the tile loop cost every form 3 - 5 % — gone, DESIGN_HISTORY).
      pending_event = 0u;
      if (threadIdx.x == 0 && sc.dbg) {
        stc(&sc.dbg[blockIdx.x], 0x10000000u | (my_ev & 0xFFFFu));
        stc(&sc.dbg[1024 + (blockIdx.x & 1023u)], (uint32_t)wall_clock64()); // when it came to the event
      }
      if (threadIdx.x == 0) {
        sAct = host_abort_seen ? STREAM_ACT_EXIT : stream_idle(sc, &my_ev);
        sEv = my_ev;
        ev_next = my_ev;
      }
      __syncthreads();
      if (sAct == STREAM_ACT_EXIT) {
        return;
      }
      if (sAct == STREAM_ACT_INSERT) {
        if (sFp != nullptr && threadIdx.x < 2u) { // the finished tiles this workgroup holds: nobody else says what becomes of them
          const uint32_t th = sHeldTile[threadIdx.x];
          if (th != STREAM_REDO_NONE) {
            stc(&sc.tile_ver[th], STREAM_TILE_HELD);
          }
        }
        if (threadIdx.x == 0 && sc.dbg) {
          stc(&sc.dbg[blockIdx.x], 0x20000000u | (my_ev & 0xFFFFu));
        }
        StreamInsertDone done;
        if (!stream_apply_insert<H, WT>(f, rd, sd, sTab, sBases, sInsWave, &sAct, tile_len, sc, sEv, phase, ctr, lists_cap, tile_idx, done)) {
          return;
        }
        const bool keep_none = (done.scan_end & STREAM_FULL_RESET) != 0u; // everything behind the read is queried again (rounds 3 - 5's form)
        if (threadIdx.x == 0) {
          sWalkEnd = done.scan_end & ~STREAM_FULL_RESET; // the dispenser's second walk: tiles in front of this position carry marks
          sGen = done.gen;
        }
        if (done.rank == 0u && threadIdx.x == 0) {
          atomicAdd(sc.executed + (keep_none ? EXE_INSERTS_KEPT_NONE : EXE_INSERTS_KEPT), 1ull);
        }
        {
          const uint32_t* const changed = sc.fp_tab[done.par];
          for (uint32_t hb = 0; hb < 2u; ++hb) { // the finished tiles held
            __syncthreads();
            const uint32_t th = sHeldTile[hb];
            if (sFp == nullptr || th == STREAM_REDO_NONE) {
              continue;
            }
            const uint32_t rh = rd.tile_read[tile_begin + th];
            const uint32_t rjh = rh - sc.first;
            if (rjh < done.resume_read) { // a read in front of the insert: decided long ago
              __syncthreads();
              if (threadIdx.x == 0) {
                sHeldTile[hb] = STREAM_REDO_NONE;
              }
              continue;
            }
            bool dirty = keep_none;
            const uint32_t nfp = keep_none ? 0u : sHeldPasses[hb] * (uint32_t)THREADS * (uint32_t)H;
            // (no short cut: a lane's dozen look-ups are independent loads — chained one behind the other they were
            // half of the time between the insert and the first record behind it)
#pragma unroll 4
            for (uint32_t q = threadIdx.x; q < nfp; q += THREADS) {
              const uint32_t fp = sFp[hb * sc.fp_words + q];
              const bool hit = fp != 0u && fp_has(changed, sc.fp_mask, fp);
              dirty = dirty | hit;
            }
            const bool any_dirty = __syncthreads_or(dirty ? 1 : 0) != 0;
            if (any_dirty) {
              if (threadIdx.x == 0) { // one of its probes reads another ID now: this workgroup queries it again, first thing
                atomicAdd(sc.executed + EXE_REDONE_DIRTY, 1ull);
                stc(&sc.tile_ver[th], STREAM_TILE_BUSY);
                sOwnRedo[sOwnRedoN++] = th;
                sHeldTile[hb] = STREAM_REDO_NONE;
              }
              continue;
            }
            // untouched by the insert: the summary stands — counted again for its read, which may be complete with it
            const uint32_t nt_h = (uint32_t)(rd.tile0[rh + 1] - rd.tile0[rh]);
            if (threadIdx.x == 0) {
              atomicAdd(sc.executed + EXE_KEPT, 1ull);
              stc(&sc.tile_ver[th], done.gen);
              __builtin_amdgcn_s_waitcnt(0);
              sTile = (atomicAdd(&sc.tiles_done[rjh], 1u) + 1u == nt_h) ? 1u : 0u;
            }
            __syncthreads();
            if (sTile != 0u && threadIdx.x < 64u) {
              stream_decide(sc, rjh, rd.tile0[rh] - tile_begin, nt_h, tiles_out, lists_out, lists_cap, reinterpret_cast<uint32_t*>(sKeys), min(STREAM_LDS_TILES, hist_cap * 6u / 40u));
            }
          }
          __syncthreads();
          // (tiles handed out under the old state that nobody holds any more — finished in front of the insert, their
          // fingerprints gone — are found by the dispenser's second walk: the selection below)
          if (threadIdx.x == 0) {
            nxt = atomicAdd(sc.next_tile, 1u); // (the position drawn ahead under the old walk is somebody else's now)
          }
          if (threadIdx.x == 0) {
            stop = 0u;
          }
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      uint32_t pick = STREAM_STOP; // window index of the tile to work on
      bool from_dispenser = false;
      if (sc.ctl && ev_next != my_ev) {
        // news in the event word (looked at while the previous tile was finishing): the event first — what is drawn ahead
        // goes back with it (an insert hands everything behind its read out again; nothing in front of it is open)
      } else {
        if (sc.ctl && sOwnRedoN != 0u) { // this workgroup's own tiles that an insert touched come first
          pick = sOwnRedo[--sOwnRedoN];
        }
        while (pick == STREAM_STOP && nxt < sc.n_tiles) {
          const uint32_t cand = tile_idx ? tile_idx[nxt] : nxt; // striped window: this rank's tiles only
          if (sc.ctl && nxt < sWalkEnd) {
            // (round 6) behind an insert the dispenser walks the tiles behind the read a second time: what is kept under
            // the new generation, held by a workgroup that has not said yet, or some workgroup's own to query again is not this one's
            // (beyond where it stood at the insert nothing carries a mark: no look, no coherent load per tile)
            const uint32_t v = ldc(&sc.tile_ver[cand]);
            if (v == STREAM_TILE_HELD || v == STREAM_TILE_BUSY || (v != 0u && v == sGen)) {
              nxt = atomicAdd(sc.next_tile, 1u);
              continue;
            }
            if (v != 0u) {
              atomicAdd(sc.executed + EXE_REDONE_LOST, 1ull); // finished under an older generation, nobody's: queried again
            }
          }
          pick = cand;
          from_dispenser = true;
        }
        if (stop && from_dispenser) {
          // the window is parked: a tile handed out before that is still needed if its read
          // lies before the first stale one (its record may be waited for), dropped otherwise
          // (dropped = not begun: the walk behind the insert finds it again)
          const uint32_t rj = rd.tile_read[tile_begin + pick] - sc.first;
          if (rj >= __hip_atomic_load(sc.park, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            pick = STREAM_STOP;
            from_dispenser = false;
          }
        }
      }
      sTile = pick;
      if (from_dispenser) {
        nxt = atomicAdd(sc.next_tile, 1u);
      }
      if (pick != STREAM_STOP && sc.ctl != nullptr && blockIdx.x < 32u) {
        // relays of the host's words — its abort flag, the insert it has committed (PCIe reads: only a few workgroups pay
        // for them): the launch may be busy when they come (tiles in front of a park; a striped window whose inserting read is another rank's)
        stream_relay(sc);
      } else if (pick != STREAM_STOP && blockIdx.x < 32u) { // relays of the host's abort flag
        if (__hip_atomic_load(sc.abort_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
          // the host has consumed every record before the stale part: nothing is needed any more
          atomicMin(sc.park, 0u);
          atomicMax(sc.next_tile, STREAM_STOP);
          __hip_atomic_store(sc.abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    if (threadIdx.x == 0 && sc.dbg) {
      stc(&sc.dbg[blockIdx.x], 0x30000000u | (sTile & 0x0FFFFFFFu));
    }
    __syncthreads();
    out_idx = sTile;
    if (out_idx == STREAM_STOP) {
      if (!sc.ctl) {
        return; // classic form: the launch ends where its window ends or parks
      }
      // Nothing to draw — the window is complete, aborted, parked at a record the host takes itself, or all of its
      // tiles are handed out — or the host's word has come: abort, or the insert it has committed.
      pending_event = 1u;
      continue;
    }
  } else {
    out_idx = tile_idx ? tile_idx[blockIdx.x] : blockIdx.x + blk0;
  }
  const uint64_t t = tile_begin + out_idx;
  const uint32_t r = rd.tile_read[t];
  const uint32_t ti = (uint32_t)(t - rd.tile0[r]);
  if constexpr (VER && !ST) {
    if (bv.skip_read_ins != nullptr && r - bv.first < bv.skip_reads) {
      const uint32_t ji = bv.skip_read_ins[r - bv.first];
      if (ji != 0xFFFFFFFFu && ti >= bv.ins[(size_t)ji * 6 + 1] && ti < bv.ins[(size_t)ji * 6 + 2]) {
        return; // a tile with records: k_batch_delta writes its summary (grp_verify.inc)
      }
    }
  }
  const uint32_t len = rd.len[r];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, ti);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;

  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, start, Lp);
  for (uint32_t i = threadIdx.x; i < hist_cap; i += THREADS) {
    sKeys[i] = 0u;
    if (i < hist_cap / 2u) {
      sCnts[i] = 0u;
    }
  }
  if (threadIdx.x == 0) {
    sListN = 0;
    sListW = 0;
    sDistinct = 0;
    sOverflow = 0;
    if constexpr (ST) {
      sCut = 0u;
      if (sFp != nullptr) {
        if (sc.n_fp > 1u) {
          sBuf ^= 1u; // a new tile: its fingerprints replace the older of the two tiles held
        }
        sHeldTile[sBuf] = STREAM_REDO_NONE;
      }
    }
  }
  __syncthreads();
  if constexpr (ST) {
    if (threadIdx.x == 0) {
      atomicAdd(sc.executed + EXE_PROBES, (unsigned long long)frames * hn);
    }
  }
  uint32_t* const fp_cur = (ST && sFp != nullptr) ? sFp + sBuf * sc.fp_words : nullptr; // (sBuf is final behind the barrier above)

  uint32_t n_hit = 0, n_miss = 0;
  uint32_t last[H];
#pragma unroll
  for (int s = 0; s < H; ++s) {
    // a seed that can no longer roll keeps its last value
    // (multiLensfrHashIterator.hpp:49-68): its frame index is clamped
    last[s] = Lp - sd->span[s];
  }
  const QuadLane ql = quad_lane();
  constexpr bool ROT = quad_rotated<H, FR, WT, ST, VER, GT>();
  const uint32_t pbytes = quad_piece_bytes(ql.sub); // round g loads piece (sub - g) & 3 of a bucket

  // Every lane owns FR frames per pass; the 64-byte bucket of each probe is
  // read by the lane's quad with ONE coalesced access (4 x 16 B), the pieces
  // rotated so that a probe's header arrives in the lane that owns the probe:
  // the lane decodes bitmap, rank and slot itself, once, and only the ID word
  // is exchanged inside the quad (one DPP move + one bpermute per round,
  // quad_decode).  Random 16-byte loads issued per lane run at ~27 G/s on
  // MI355X, quad-coalesced bucket reads at ~48 G buckets/s, in either piece
  // order (tools/gather_bench.hip modes 7 / 10, 24 / 28).
  // Frames of a pass.  Seeds that share their halves (DevSeeds::n_left): a frame's right halves
  // serve the H - 1 frames in front of it, handed over by wave shuffles — so the first three waves
  // of a workgroup end on H - 1 helper lanes (they compute the halves of the next wave's first
  // frames and own no probe) and the last wave's last lanes evaluate their neighbours' right
  // halves themselves: 3 x (64 - (H-1)) + 64 frames per block of THREADS lanes (250 at h = 3: a
  // 1000-frame tile still takes 4 passes of one frame per lane).  No barrier, no LDS.
  // Where the helper lanes would cost a pass (h = 5: 244 frames per block, a 1000-frame tile
  // would need 5 passes instead of 4) every wave's last lanes evaluate their neighbours' right
  // halves themselves instead (256 frames per block, H - 1 extra half evaluations per wave).
  const uint32_t n_left = (H >= 2 && H <= GRP_H_GROUP && WT != GRP_WT_LONG) ? sd->n_left : 0u; // (0 for long spans: the halves are a 32-base form;
                                                                                                 // 0 in the many-seed form: every seed hashed on its own)
  constexpr uint32_t OV = (uint32_t)H - 1u, USE = 64u - OV;
  static_assert(THREADS == 256, "the helper-lane layout below is written for four waves per workgroup (my_wave == 3 is the last one, FBH = 3 * USE + 64)");
  constexpr uint32_t FBH = gr::geom::helper_pass_frames(H);
  const uint32_t ftile = frames_per_tile(sd, tile_len);
  const bool helper = n_left != 0u && (ftile + FBH * FR - 1u) / (FBH * FR) == (ftile + THREADS * FR - 1u) / (THREADS * FR);
  const uint32_t FB = helper ? FBH : (uint32_t)THREADS; // frames per block of THREADS lanes
  const uint32_t my_wave = threadIdx.x >> 6, my_lane = threadIdx.x & 63u;
  const uint32_t my_off = helper ? (my_wave * USE + my_lane) : threadIdx.x;          // frame of this lane inside a block
  const bool my_real = helper ? (my_wave == 3u || my_lane < USE) : true;             // not a helper lane
  const bool my_tail_wave = helper ? my_wave == 3u : true;                           // its last lanes have no lane to ask
  const uint32_t passes = (frames + FB * FR - 1u) / (FB * FR);
  uint64_t bk[FR][H];
  uint32_t off[FR][H];
  bool live_j[FR];
  // 1) hashes -> positions.  Frames past the end recompute the last frame: all
  //    lanes stay active (the quad exchange needs them) and all addresses valid.
  //    The positions of pass p + 1 are computed while the bucket loads of pass p are in flight
  //    (software pipelining by hand: a wave's hash arithmetic overlaps its own memory latency).
  auto positions = [&](uint32_t pp, uint64_t (&bk_)[FR][H], uint32_t (&off_)[FR][H], bool (&lv)[FR]) {
  if (n_left != 0u) {
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      const uint32_t fr_raw = (pp * FR + j) * FB + my_off;
      const uint32_t fr = min(fr_raw, frames - 1u);
      lv[j] = my_real && fr_raw < frames;
      uint64_t hL, hRL, hR, hRR;
      seed_halves<WT, true, true>(sTab, sd, n_left, window_at(sBases, boff + fr), hL, hRL, hR, hRR);
      const uint64_t hv0 = (hL ^ hR) + (hRL ^ hRR);
#pragma unroll
      for (int s = 0; s < H; ++s) {
        uint64_t hv = hv0;
        if (s != 0) {
          // the right halves of frame fr + s: the lane s places up the wave ...
          uint64_t nR = __shfl_down((unsigned long long)hR, (unsigned)s, 64);
          uint64_t nRR = __shfl_down((unsigned long long)hRR, (unsigned)s, 64);
          if (my_tail_wave && my_lane + (uint32_t)s >= 64u) {
            // ... which the last lanes of a wave without helper lanes behind it do not have: evaluated here
            uint64_t a, b;
            seed_halves<WT, false, true>(sTab, sd, n_left, window_at(sBases, boff + min(fr_raw + (uint32_t)s, frames - 1u)), a, b, nR, nRR);
          }
          if (lv[j]) {
            if (fr <= last[s]) {
              hv = (srol_small(hL, (uint32_t)s) ^ nR) + (hRL ^ srol_small(nRR, (uint32_t)s));
            } else {
              // a seed that can no longer roll keeps its last value (the tile's last s frames)
              hv = seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + last[s]));
            }
          }
        }
        const Probe p = grp_locate(f, hv);
        bk_[j][s] = p.b;
        off_[j][s] = p.off;
        if constexpr (ST) {
          if (fp_cur != nullptr) { // which ID slot this probe reads: held against the slots an insert changes (round 6)
            fp_cur[((pp * FR + (uint32_t)j) * (uint32_t)THREADS + threadIdx.x) * (uint32_t)H + (uint32_t)s] = lv[j] ? slot_fp(p.b, p.off) : 0u;
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      const uint32_t fr_raw = (pp * FR + j) * THREADS + threadIdx.x;
      const uint32_t fr = min(fr_raw, frames - 1u);
      lv[j] = fr_raw < frames;
#pragma unroll
      for (int s = 0; s < H; ++s) {
        if (!seed_on<H>(s, frame_seeds<H>(sd))) {
          bk_[j][s] = 0;
          off_[j][s] = 0;
          if constexpr (ST) {
            if (fp_cur != nullptr) {
              fp_cur[((pp * FR + (uint32_t)j) * (uint32_t)THREADS + threadIdx.x) * (uint32_t)H + (uint32_t)s] = 0u;
            }
          }
          continue;
        }
        const uint64_t hv = seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + min(fr, last[s])));
        const Probe p = grp_locate(f, hv);
        bk_[j][s] = p.b;
        off_[j][s] = p.off;
        if constexpr (ST) {
          if (fp_cur != nullptr) {
            fp_cur[((pp * FR + (uint32_t)j) * (uint32_t)THREADS + threadIdx.x) * (uint32_t)H + (uint32_t)s] = lv[j] ? slot_fp(p.b, p.off) : 0u;
          }
        }
      }
    }
  }
  };
  // (only the persistent form: with two frames per lane the second set of positions costs the
  // synchronous forms a wave of occupancy — 169 VGPRs — and their rate, measured)
  // (the many-seed form computes a pass's positions in front of its loads: 16 probes per lane are latency enough, and the
  // persistent form has no registers left for a second set — measured: 512 VGPRs and 24 spilled with it)
  constexpr bool PIPE = (ST || FR == 1) && H <= GRP_H_GROUP;
  if constexpr (PIPE) {
    if (passes > 0u) {
      positions(0u, bk, off, live_j);
    }
  }
  for (uint32_t pass = 0; pass < passes; ++pass) {
    if constexpr (ST) {
      // A resumable window that has parked: the remaining passes of a tile behind the parking
      // read are dropped (the tile is stale and will be queried again), so the launch is ready
      // for the insert after one pass instead of one tile — the time from the insert record to
      // the resumed query was two tile times (~2 x 190 us on C2), this is the first of them.
      // A hint only: the flag is read with an ordinary cached load (no extra memory traffic;
      // it may trail the park by a few microseconds), results never depend on it.
      if (sc.ctl && sFp == nullptr && pass != 0u && __hip_atomic_load(sc.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u) {
        if (r - sc.first >= ldc(sc.park)) {
          if ((threadIdx.x & 63u) == 0u) {
            sCut = 1u;
          }
          break;
        }
      }
    }
    if constexpr (H <= GRP_H_GROUP) {
      uint4 piece[FR][H][4];
      if constexpr (!PIPE) {
        positions(pass, bk, off, live_j);
      }
      // 2) round g: the quad reads the bucket of its lane g's probe
#pragma unroll
      for (int j = 0; j < FR; ++j) {
#pragma unroll
        for (int s = 0; s < H; ++s) {
          piece[j][s][0] = quad_read<ROT, 0>(f.buckets, bk[j][s], ql, pbytes);
          piece[j][s][1] = quad_read<ROT, 1>(f.buckets, bk[j][s], ql, pbytes);
          piece[j][s][2] = quad_read<ROT, 2>(f.buckets, bk[j][s], ql, pbytes);
          piece[j][s][3] = quad_read<ROT, 3>(f.buckets, bk[j][s], ql, pbytes);
        }
      }
      uint64_t bk_next[PIPE ? FR : 1][PIPE ? H : 1];
      uint32_t off_next[PIPE ? FR : 1][PIPE ? H : 1];
      bool live_next[PIPE ? FR : 1];
      if constexpr (PIPE) {
        if (pass + 1u < passes) {
          positions(pass + 1u, bk_next, off_next, live_next);
        }
      }
      // 3) bit test + ID slot, exchanged inside the quad; per-frame ID set -> tile count table
#pragma unroll
      for (int j = 0; j < FR; ++j) {
        const bool live = live_j[j];
        bool all = live;
        uint32_t idv[H];
        uint64_t vrank[VER ? H : 1], vbl[VER ? H : 1];
        bool vneed[VER ? H : 1], vamb[VER ? H : 1];
#pragma unroll
        for (int s = 0; s < H; ++s) {
          const QuadAnswer mine = quad_result<ROT>(piece[j][s], off[j][s], ql);
          all = all && mine.bit; // atRank (MIBloomFilter.hpp:465-476)
          uint32_t d = mine.id;  // getData (:614-621)

          if (mine.lr >= GRP_BUCKET_IDS && live) { // 14th.. set bit of its bucket: rare side table
            d = grp_ovf_get(f, f.super[bk[j][s] >> GRP_SUPER_SHIFT] + mine.rel + mine.lr);
          }
          if constexpr (VER) {
            const uint32_t fl = bv.floor[r - bv.floor_first]; // bit 31: an ID equal to the floor may have been written in front of this read
            const uint32_t floor_id = fl & 0x7FFFFFFFu;
            vrank[s] = f.super[bk[j][s] >> GRP_SUPER_SHIFT] + mine.rel + mine.lr;
            vbl[s] = bk[j][s] * 64ull + mine.lr;
            vneed[s] = live && mine.bit && (d & 0x7FFFFFFFu) >= floor_id; // written by this or a later read of the batch
            vamb[s] = (fl >> 31) != 0u && (d & 0x7FFFFFFFu) == floor_id;
          }
          idv[s] = d;
        }
        if (!all) {
          continue; // (a frame with a clear bit counts nothing: its IDs need not be looked up)
        }
        if constexpr (VER) {
          // every read sees the state in front of its own insert: the IDs this batch wrote are looked up
          batch_view_multi<H>(bv, vrank, vbl, vneed, vamb, r - bv.first, idv);
        }
        uint32_t ids[H];
#pragma unroll
        for (int s = 0; s < H; ++s) {
          const uint32_t d = idv[s];
          // saturation bit stripped exactly as goldrush_path.cpp:573-594
          const uint32_t id = (d > 0x80000000u) ? (d & 0x7FFFFFFFu) : d;
          if (id == 0u) {
            ++n_miss;
          } else {
            ++n_hit;
          }
          bool dup = false;
#pragma unroll
          for (int u = 0; u < s; ++u) {
            dup = dup || (ids[u] == id);
          }
          ids[s] = id;
          if (id != 0u && !dup) {
            hist_add16(sKeys, sCnts, hist_cap, id, &sDistinct, distinct_limit, &sOverflow);
          }
        }
      }
      if constexpr (PIPE) {
        if (pass + 1u < passes) {
#pragma unroll
          for (int j = 0; j < FR; ++j) {
            live_j[j] = live_next[j];
#pragma unroll
            for (int s = 0; s < H; ++s) {
              bk[j][s] = bk_next[j][s];
              off[j][s] = off_next[j][s];
            }
          }
        }
      }
    } else {
      // The many-seed form (h = 9 .. 16; one frame per lane): the bucket lines of 16 probes x 4 quad pieces would take
      // 256 VGPRs, so the frame's seeds go in two groups of GRP_H_GROUP — a group's lines are read, answered and
      // dropped before the next group's are read.  The FRAME stays one unit across the groups: its hit flag (all h
      // bits set, MIBloomFilter::atRank) and its IDs are collected over both, then counted and de-duplicated over all
      // h probes at once, as below for h <= 8.
      static_assert(FR == 1 && !PIPE, "the many-seed form runs one frame per lane and pass");
      constexpr int NG = (H + GRP_H_GROUP - 1) / GRP_H_GROUP;
      positions(pass, bk, off, live_j);
      const bool live = live_j[0];
      bool all = live;
      uint32_t idv[H];
      uint64_t vrank[VER ? H : 1], vbl[VER ? H : 1];
      bool vneed[VER ? H : 1], vamb[VER ? H : 1];
#pragma unroll
      for (int s = 0; s < H; ++s) {
        idv[s] = 0u;
        if constexpr (VER) {
          vrank[s] = 0;
          vbl[s] = 0;
          vneed[s] = false;
          vamb[s] = false;
        }
      }
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        uint4 piece[GRP_H_GROUP][4];
#pragma unroll
        for (int q = 0; q < GRP_H_GROUP; ++q) {
          const int s = gi * GRP_H_GROUP + q;
          if (seed_on<H>(s, hn)) {
            piece[q][0] = quad_read<ROT, 0>(f.buckets, bk[0][s], ql, pbytes);
            piece[q][1] = quad_read<ROT, 1>(f.buckets, bk[0][s], ql, pbytes);
            piece[q][2] = quad_read<ROT, 2>(f.buckets, bk[0][s], ql, pbytes);
            piece[q][3] = quad_read<ROT, 3>(f.buckets, bk[0][s], ql, pbytes);
          }
        }
#pragma unroll
        for (int q = 0; q < GRP_H_GROUP; ++q) {
          const int s = gi * GRP_H_GROUP + q;
          if (!seed_on<H>(s, hn)) {
            continue;
          }
          const QuadAnswer mine = quad_result<ROT>(piece[q], off[0][s], ql);
          all = all && mine.bit; // atRank (MIBloomFilter.hpp:465-476): over all h seeds of the frame
          uint32_t d = mine.id;  // getData (:614-621)
          if (mine.lr >= GRP_BUCKET_IDS && live) {
            d = grp_ovf_get(f, f.super[bk[0][s] >> GRP_SUPER_SHIFT] + mine.rel + mine.lr);
          }
          if constexpr (VER) {
            const uint32_t fl = bv.floor[r - bv.floor_first];
            const uint32_t floor_id = fl & 0x7FFFFFFFu;
            vrank[s] = f.super[bk[0][s] >> GRP_SUPER_SHIFT] + mine.rel + mine.lr;
            vbl[s] = bk[0][s] * 64ull + mine.lr;
            vneed[s] = live && mine.bit && (d & 0x7FFFFFFFu) >= floor_id;
            vamb[s] = (fl >> 31) != 0u && (d & 0x7FFFFFFFu) == floor_id;
          }
          idv[s] = d;
        }
      }
      if (all) {
        if constexpr (VER) {
          batch_view_multi<H>(bv, vrank, vbl, vneed, vamb, r - bv.first, idv);
        }
        uint32_t ids[H];
#pragma unroll
        for (int s = 0; s < H; ++s) {
          if (!seed_on<H>(s, hn)) {
            continue;
          }
          const uint32_t d = idv[s];
          const uint32_t id = (d > 0x80000000u) ? (d & 0x7FFFFFFFu) : d; // goldrush_path.cpp:573-594
          if (id == 0u) {
            ++n_miss;
          } else {
            ++n_hit;
          }
          bool dup = false; // the frame's IDs de-duplicated over all h probes, both groups
#pragma unroll
          for (int u = 0; u < s; ++u) {
            dup = dup || (ids[u] == id);
          }
          ids[s] = id;
          if (id != 0u && !dup) {
            hist_add16(sKeys, sCnts, hist_cap, id, &sDistinct, distinct_limit, &sOverflow);
          }
        }
      }
    }
  }
  if constexpr (ST) {
    if (sc.ctl && threadIdx.x == 0) {
      // the host's word, if there is one: looked at behind the tile (a COHERENT load — an ordinary one is served by this
      // XCD's L2, where a line that every workgroup reads for every tile never ages out: the launch then learns of an
      // insert when it runs out of tiles, measured); its latency lies behind the tile's way out
      ev_next = ldc(sc.ctl + SCT_EV + (blockIdx.x % min(SCT_GROUPS, gridDim.x)) * 32u);
    }
  }
  __syncthreads();

  // top ID + count>2 list: one pass over the table for the top and the list's length, a second one (behind the
  // arena reservation) that writes the list straight out — no LDS staging area
  uint32_t bc = 0, bid = 0, my_n = 0;
  for (uint32_t i = threadIdx.x; i < hist_cap; i += THREADS) {
    uint32_t key = tab_word(&sKeys[i]);
    if (key != 0u) {
      uint32_t c = (tab_word(&sCnts[i >> 1]) >> ((i & 1u) << 4)) & 0xFFFFu;
      if (better(c, key, bc, bid)) {
        bc = c;
        bid = key;
      }
      my_n += c > 2u ? 1u : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint32_t oc = __shfl_xor(bc, o, 64);
    uint32_t oid = __shfl_xor(bid, o, 64);
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
    const bool flagged = sOverflow != 0u || (direct_stride != 0u && n > direct_stride);
    uint64_t lo = 0;
    if (direct_stride != 0u) {
      lo = (uint64_t)out_idx * direct_stride;
    } else if (n && !flagged) {
      lo = atomicAdd(&ctr[QCTR_LIST_CURSOR], (unsigned long long)n);
    }
    sListOff = (uint32_t)lo;
    if (flagged) {
      sListN = 0; // nothing is copied out; the full-capacity launch redoes this tile
      if (direct_stride == 0u) {
        atomicAdd(&ctr[QCTR_FLAGGED_DISTINCT], 1ull); // statistics: tiles with more distinct IDs than this launch's table takes
        const unsigned long long fi = atomicAdd(&ctr[QCTR_FLAGGED], 1ull);
        if (flagged_out && fi < flagged_cap) {
          flagged_out[fi] = out_idx;
        }
      }
    }
    grp_tile_summary ts;
    ts.top_id = bid;
    ts.top_count = bc;
    ts.list_off = (uint32_t)lo;
    ts.list_n = flagged ? GRP_TILE_FLAGGED : n;
    ts.hits = hsum;
    ts.misses = msum;
    if constexpr (ST) {
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(tiles_out + out_idx);
      store_coherent(dst, (unsigned long long)ts.top_id | ((unsigned long long)ts.top_count << 32));
      store_coherent(dst + 1, (unsigned long long)ts.list_off | ((unsigned long long)ts.list_n << 32));
      store_coherent(dst + 2, (unsigned long long)ts.hits | ((unsigned long long)ts.misses << 32));
      if (sc.ctl) {
        // finished under this generation; its probes' fingerprints stay in this workgroup's LDS until the tile after next
        // (a tile of a parked window that was cut short — the hint above — is not: such a window hands everything out again)
        const bool whole = sCut == 0u;
        stc(&sc.tile_ver[out_idx], whole ? sGen : 0u); // (sGen: this workgroup's copy of the generation — no coherent load on every tile's way out)
        if (sFp != nullptr) {
          sHeldTile[sBuf] = whole ? out_idx : STREAM_REDO_NONE;
          sHeldPasses[sBuf] = passes;
        }
      }
    } else if (direct_stride != 0u) {
      // zero-copy window: the host spins on list_n; the summary goes out after the lists
      // (below), words 0 and 2 here, the word holding list_n last
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(tiles_out + out_idx);
      __hip_atomic_store(dst, (unsigned long long)ts.top_id | ((unsigned long long)ts.top_count << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(dst + 2, (unsigned long long)ts.hits | ((unsigned long long)ts.misses << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      sDirectWord = (unsigned long long)ts.list_off | ((unsigned long long)ts.list_n << 32);
    } else {
      tiles_out[out_idx] = ts;
    }
  }
  __syncthreads();
  if (sListN != 0u) {
    const uint64_t lo = sListOff;
    for (uint32_t i = threadIdx.x; i < hist_cap; i += THREADS) {
      const uint32_t key = tab_word(&sKeys[i]);
      if (key == 0u) {
        continue;
      }
      const uint32_t c = (tab_word(&sCnts[i >> 1]) >> ((i & 1u) << 4)) & 0xFFFFu;
      if (c <= 2u) {
        continue;
      }
      const uint64_t at = lo + atomicAdd(&sListW, 1u);
      if (at < lists_cap) {
        const unsigned long long e = (unsigned long long)key | ((unsigned long long)c << 32);
        if constexpr (ST) {
          store_coherent(reinterpret_cast<unsigned long long*>(lists_out + at), e);
        } else if (direct_stride != 0u) {
          // host memory, read by the spinning host before the launch ends: system scope (a
          // plain store may sit in the L2 until the end-of-kernel write-back)
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(lists_out + at), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
          lists_out[at].id = key;
          lists_out[at].count = c;
        }
      }
    }
  }
  if constexpr (!ST) {
    if (direct_stride != 0u) {
      __builtin_amdgcn_s_waitcnt(0); // lists (and the other summary words) have left
      __syncthreads();
      if (threadIdx.x == 0) {
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(tiles_out + out_idx) + 1, sDirectWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
  if constexpr (ST) {
    // "last block" hand-over without device-scope fences: the summaries and lists went
    // out as coherent stores; once they are acknowledged (vmcnt = 0 in every wave, then
    // the barrier) one lane counts the tile with a device-scope atomic.  The workgroup
    // that sees the read complete reads them back with coherent loads.
    if (threadIdx.x == 0) { // the prefetched tile index is only used if the window is still live
      stop = __hip_atomic_load(sc.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    const uint32_t rj = r - sc.first;
    const uint32_t nt_read = (uint32_t)(rd.tile0[r + 1] - rd.tile0[r]);
    if (threadIdx.x == 0) {
      sTile = (atomicAdd(&sc.tiles_done[rj], 1u) + 1u == nt_read) ? 1u : 0u;
    }
    __syncthreads();
    if (sTile != 0u && threadIdx.x < 64u) {
      stream_decide(sc, rj, rd.tile0[r] - tile_begin, nt_read, tiles_out, lists_out, lists_cap, reinterpret_cast<uint32_t*>(sKeys), min(STREAM_LDS_TILES, hist_cap * 6u / 40u));
    }
    // (the barrier at the top of the loop keeps sTile / the count-table area untouched
    // until the deciding wave is back)
  } else {
    return;
  }
  } // next tile (ST)
}

// ---- read decision --------------------------------------------------------------

// threshold + smoothing passes + flank test + decision of every read of a window (the
// shared host/device core, csrc/host/gr_tiles_core.hpp), one WAVE per read.
//   reads of up to 64 tiles: tile i sits in lane i, the passes run as wave-uniform scalar
//     code on v_readlane / v_writelane (LaneState) — no LDS, no divergence
//   longer reads: lane 0 walks a slice of a global scratch area
// History (profiles/): 64 reads in the lanes of one wave serialised on divergence
// (~300 us per window), one lane per wave over LDS arrays ~120 us, this form ~10 us.
constexpr int DECIDE_THREADS = 64;
constexpr uint32_t DECIDE_LDS_BYTES_PER_TILE = 8 + sizeof(grp_tile_summary) + 4 + 1; // scratch word, summary, ID, flag
constexpr uint32_t DECIDE_LDS_MAX_TILES = 4096;                                       // 148 KB of the 160 KB

__global__ void __launch_bounds__(DECIDE_THREADS)
k_decide(DevReads rd,
         uint32_t first,
         uint32_t count,
         grp_decide_params dp,
         const grp_tile_summary* __restrict__ tiles,
         const grp_id_count* __restrict__ lists,
         uint64_t lists_cap,
         uint32_t* __restrict__ g_ids,
         uint8_t* __restrict__ g_asg,
         uint64_t* __restrict__ g_scratch,
         grp_read_decision* __restrict__ out,
         uint32_t lds_tiles,
         const uint32_t* __restrict__ read_list = nullptr, // the reads of this launch (window indices); NULL: all of them, one per workgroup
         uint32_t skip_above = 0,                          // no list: reads of more tiles than this belong to another launch (0: none do)
         unsigned long long* __restrict__ qctr = nullptr,  // the window's eight counters: moved to `qctr_out` (in front of the decisions: one copy
         unsigned long long* __restrict__ qctr_out = nullptr) // brings both to the host) and zeroed for the next window
{
  extern __shared__ uint4 smem4[];
  __shared__ uint64_t sSort[4 * LANE_TILES]; // LaneStateN::sort_assigned
  const uint32_t lane = threadIdx.x;
  if (qctr != nullptr && blockIdx.x == 0 && lane < 8u) { // (every kernel that counts has finished: the launches of a window are in stream order)
    qctr_out[lane] = qctr[lane];
    qctr[lane] = 0ull;
  }
  const uint32_t j = read_list ? read_list[blockIdx.x] : blockIdx.x;
  const uint64_t t_base = rd.tile0[first];
  const uint64_t a = rd.tile0[first + j] - t_base;
  const uint64_t n = rd.tile0[first + j + 1] - rd.tile0[first + j];
  if (!read_list && skip_above != 0u && n > skip_above) {
    return; // a read whose state lives in LDS: the launch over the window's long reads decides it (classify_enqueue_decide)
  }
  grp_read_decision d{};
  if (n <= LANE_TILES) {
    LaneState st;
    st.lists = lists;
    bool bad = false;
    if (lane < n) {
      const grp_tile_summary t = tiles[a + lane];
      st.load(t);
      // decided again after the flagged tiles have been redone / the list arena enlarged
      bad = t.list_n == GRP_TILE_FLAGGED || (uint64_t)t.list_off + t.list_n > lists_cap;
      if (!bad) {
        st.load_list_head();
      }
    }
    if (__ballot(bad) == 0ull) {
      gr::core::decide(dp.threshold, dp.unassigned_min, dp.assigned_max, (size_t)n, st, d);
      if (lane < n) { // keep the per-tile result inspectable (grp_debug_tile_states)
        g_ids[a + lane] = st.v_id;
        g_asg[a + lane] = (uint8_t)st.v_asg;
      }
    }
    if (lane == 0) {
      out[j] = d;
    }
  } else if (n <= 2 * LANE_TILES) {
    // 65 .. 128 tiles: two tiles per lane, still register-resident
    (void)decide_in_registers<2>(lane, a, n, dp, tiles, lists, lists_cap, g_ids, g_asg, sSort, d);
    if (lane == 0) {
      out[j] = d;
    }
  } else if (n <= 4 * LANE_TILES) {
    // .. 256 tiles: four per lane
    (void)decide_in_registers<4>(lane, a, n, dp, tiles, lists, lists_cap, g_ids, g_asg, sSort, d);
    if (lane == 0) {
      out[j] = d;
    }
  } else if (n <= lds_tiles) {
    // longer reads (the tail of a long-read length distribution): the state in LDS (DECIDE_LDS_BYTES_PER_TILE a
    // tile), staged and walked by the whole wave in step (WaveLdsState) — the passes are serial, but every step is an
    // LDS access instead of a round trip to HBM (a 600-tile read took ~10 ms through the global arrays and held up its launch)
    uint64_t* sScratch = reinterpret_cast<uint64_t*>(smem4);
    grp_tile_summary* sTiles = reinterpret_cast<grp_tile_summary*>(sScratch + lds_tiles);
    uint32_t* sIds = reinterpret_cast<uint32_t*>(sTiles + lds_tiles);
    uint8_t* sAsg = reinterpret_cast<uint8_t*>(sIds + lds_tiles);
    bool bad = false;
    for (uint32_t i = lane; i < n; i += 64u) {
      const grp_tile_summary t = tiles[a + i];
      sTiles[i] = t;
      bad = bad || t.list_n == GRP_TILE_FLAGGED || (uint64_t)t.list_off + t.list_n > lists_cap;
    }
    const bool redo = __ballot(bad) != 0ull;
    __builtin_amdgcn_wave_barrier();
    if (!redo) {
      WaveLdsState st;
      st.tiles = sTiles;
      st.lists = lists;
      st.ids = sIds;
      st.flags = sAsg;
      st.scratch = sScratch;
      gr::core::decide(dp.threshold, dp.unassigned_min, dp.assigned_max, (size_t)n, st, d); // all lanes, in step
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = lane; i < n; i += 64u) {
        g_ids[a + i] = sIds[i];
        g_asg[a + i] = sAsg[i];
      }
    }
    if (lane == 0) {
      out[j] = d;
    }
  } else {
    if (lane != 0) {
      return;
    }
    const grp_tile_summary* my_tiles = tiles + a;
    bool redo = false;
    for (uint64_t i = 0; i < n; ++i) {
      redo = redo || my_tiles[i].list_n == GRP_TILE_FLAGGED || (uint64_t)my_tiles[i].list_off + my_tiles[i].list_n > lists_cap;
    }
    if (!redo) {
      gr::core::decide(dp.threshold, dp.unassigned_min, dp.assigned_max, (size_t)n, my_tiles, lists, g_ids + a, g_asg + a, g_scratch + a, d);
    }
    out[j] = d;
  }
}

// ---- insert ------------------------------------------------------------------------

// claim `key` in the per-call dedup set; true for exactly one caller per key.
// Entries tagged with an older epoch count as empty (no clearing between calls).
__device__ inline bool
dedup_claim(unsigned long long* table, uint64_t cap_mask, unsigned long long key, unsigned long long epoch_tag)
{
  uint64_t slot = (key * 0x9E3779B97F4A7C15ULL) >> 20 & cap_mask;
  for (;;) {
    unsigned long long cur = table[slot];
    for (;;) {
      if (cur == key) {
        return false;
      }
      if ((cur & 0xFFFFFF0000000000ULL) == epoch_tag) {
        break; // occupied by another rank of this call -> next slot
      }
      unsigned long long prev = atomicCAS(&table[slot], cur, key);
      if (prev == cur) {
        return true;
      }
      cur = prev;
    }
    slot = (slot + 1) & cap_mask;
  }
}

template<int H, int WT>
__device__ __forceinline__ void
insert_tiles(const DevFilter& f,
             const DevReads& rd,
             const DevSeeds* __restrict__ sd,
             uint32_t tile_len,
             uint32_t read_idx,
             uint32_t tile_start,
             uint32_t id,
             unsigned long long* __restrict__ dedup,
             uint64_t dedup_mask,
             unsigned long long epoch_tag)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);

  const uint32_t r = read_idx;
  // one frame per thread: `parts` workgroups share a tile
  const uint32_t parts = gr::geom::tile_parts(frames_per_tile(sd, tile_len));
  const uint32_t ti = tile_start + blockIdx.x / parts;
  const uint32_t part = blockIdx.x % parts;
  const uint32_t len = rd.len[r];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, ti);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;

  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, start, Lp);
  __syncthreads();

  for (uint32_t fr = part * THREADS + threadIdx.x; fr < frames; fr += THREADS * parts) {
    Probe pr[H];
    uint4 hd[H];
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (seed_on<H>(s, hn)) {
        const uint32_t fs = min(fr, Lp - sd->span[s]);
        pr[s] = grp_locate(f, seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs)));
      }
    }
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (seed_on<H>(s, hn)) {
        hd[s] = f.buckets[pr[s].b * GRP_UNIT_U4];
      }
    }
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (!seed_on<H>(s, hn)) {
        continue;
      }
      // getRankPos (MIBloomFilter.hpp:488-491): rank only, the bit is not tested
      const uint32_t lr = grp_local_rank(grp_bitmap(hd[s]), pr[s].off);
      const uint64_t rank = f.super[pr[s].b >> GRP_SUPER_SHIFT] + hd[s].x + lr;
      if (rank >= f.pop || !((grp_bitmap(hd[s]) >> pr[s].off) & 1ull)) {
        // an unset bit has no slot of its own; unreachable for reads that went
        // through the fill (it covers a superset of all tile positions)
        continue;
      }
      if (dedup_claim(dedup, dedup_mask, epoch_tag | rank, epoch_tag)) {
        // MIBFConstructSupport.hpp:274-282 ; the only writer of this rank in this call
        unsigned long long* cwp = grp_cw_ptr(f, pr[s].b, lr, rank);
        const unsigned long long cword = *cwp;
        const uint32_t count = grp_cnt(cword) + 1u;
        *cwp = grp_cnt_with(cword, count);
        const uint32_t random_num = (uint32_t)(rank ^ (uint64_t)id) % count;
        if (random_num == count - 1u) {
          uint32_t* slot = (lr < GRP_BUCKET_IDS) ? &reinterpret_cast<uint32_t*>(f.buckets)[grp_id_loc(pr[s].b, lr)] : nullptr;
          const uint32_t old = slot ? *slot : grp_ovf_get(f, rank);
          // setData (MIBloomFilter.hpp:593-602): keep a set saturation bit
          const uint32_t nv = (old > 0x80000000u) ? (id | 0x80000000u) : id;
          if (slot) {
            *slot = nv;
          } else {
            grp_ovf_put(f, rank, nv);
          }
        }
      }
    }
  }
}

// WT: 0, or GRP_WT_LONG for seeds of spans beyond 64 bases (DevSeeds::wide == 2)
template<int H, int WT = 0>
__global__ void __launch_bounds__(THREADS)
k_insert(DevFilter f,
         DevReads rd,
         const DevSeeds* __restrict__ sd,
         uint32_t tile_len,
         uint32_t read_idx,
         uint32_t tile_start,
         uint32_t id,
         unsigned long long* __restrict__ dedup,
         uint64_t dedup_mask,
         unsigned long long epoch_tag)
{
  insert_tiles<H, WT>(f, rd, sd, tile_len, read_idx, tile_start, id, dedup, dedup_mask, epoch_tag);
}

// ---- whole-read insert (all ID blocks of a read in two launches) ------------------
//
// process_read inserts a read as consecutive blocks of `block` tiles, one
// insertMIBF call (= one dedup scope, one ID) per block, in order
// (goldrush_path.cpp:982-990, 1040-1051).  k_insert_collect gathers, for every
// distinct rank of the read, the SET of blocks that touch it (bit j = block j);
// k_insert_apply then replays the blocks in ascending order per rank:
// c = ++count; if (uint32(rank ^ id_j) % c == c-1) id = id_j — identical to the
// sequential calls because different ranks never interact.

template<int H, int WT>
__global__ void __launch_bounds__(THREADS)
k_insert_collect(DevFilter f, DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint32_t read_idx, uint32_t tile_start, uint32_t block_tiles, InsertTable tb, uint32_t parity)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + frame_seeds<H>(sd) * sd->wmax * 4u);
  __shared__ uint32_t sWave[THREADS / 64 + 1];
  load_tab(sTab, sd);
  insert_collect_unit<H, WT, false>(f, rd, sd, sTab, sBases, sWave, tile_len, read_idx, tile_start, block_tiles, tb, &tb.counter[parity], blockIdx.x);
}

__global__ void __launch_bounds__(THREADS)
k_insert_apply(DevFilter f, InsertTable tb, uint32_t parity, uint32_t block_tiles, uint32_t first_id, uint32_t id_offset)
{
  const uint32_t n = tb.counter[parity];
  const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
  if (i == 0) {
    tb.counter[parity ^ 1u] = 0; // the next call's counter
  }
  if (i >= n) {
    return;
  }
  insert_apply_entry<false>(f, tb, i, block_tiles, first_id, id_offset);
}

// ---- inspection kernels ----------------------------------------------------------

// buckets -> plain bit vector (out zeroed by the caller, 32-bit words)
__global__ void
k_export_bits(const uint4* __restrict__ buckets, uint64_t n_buckets, uint32_t W, uint32_t* __restrict__ out)
{
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t bm = grp_bitmap(buckets[b * GRP_UNIT_U4]);
    if (!bm) {
      continue;
    }
    const uint64_t s = b * W;
    const uint64_t w = s >> 5;
    const uint32_t sh = (uint32_t)(s & 31u);
    atomicOr(&out[w], (uint32_t)(bm << sh));
    const uint64_t rest = sh ? (bm >> (32u - sh)) : (bm >> 32);
    if (sh) {
      if ((uint32_t)rest) {
        atomicOr(&out[w + 1], (uint32_t)rest);
      }
      if ((uint32_t)(rest >> 32)) {
        atomicOr(&out[w + 2], (uint32_t)(rest >> 32));
      }
    } else if ((uint32_t)rest) {
      atomicOr(&out[w + 1], (uint32_t)rest);
    }
  }
}

__global__ void
k_rank_positions(DevFilter f, const uint64_t* __restrict__ pos, uint64_t n, uint8_t* __restrict__ bit, uint64_t* __restrict__ rank)
{
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) {
    return;
  }
  const uint64_t p = pos[i];
  const uint64_t b = grp_div_w(p, f.w_magic);
  const uint32_t off = (uint32_t)(p - b * f.W);
  const uint4 hd = f.buckets[b * GRP_UNIT_U4];
  const uint64_t bm = grp_bitmap(hd);
  bit[i] = (uint8_t)((bm >> off) & 1ull);
  rank[i] = f.super[b >> GRP_SUPER_SHIFT] + hd.x + grp_local_rank(bm, off);
}

// ids / counts of ranks [first, first+n): one thread per bucket
__global__ void
k_export_ids(DevFilter f, uint64_t first, uint64_t n, uint32_t* __restrict__ ids, uint32_t* __restrict__ counts)
{
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < f.n_buckets; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 hd = f.buckets[b * GRP_UNIT_U4];
    const uint32_t c = (uint32_t)__popcll(grp_bitmap(hd));
    const uint64_t base = f.super[b >> GRP_SUPER_SHIFT] + hd.x;
    for (uint32_t lr = 0; lr < c; ++lr) {
      const uint64_t rank = base + lr;
      if (rank >= first && rank < first + n) {
        const uint32_t v = (lr < GRP_BUCKET_IDS) ? reinterpret_cast<const uint32_t*>(f.buckets)[grp_id_loc(b, lr)] : grp_ovf_get(f, rank);
        ids[rank - first] = v;
        counts[rank - first] = grp_cnt(*grp_cw_ptr(f, b, lr, rank));
      }
    }
  }
}

__global__ void
k_import_ids(DevFilter f, uint64_t first, uint64_t n, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ counts)
{
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < f.n_buckets; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 hd = f.buckets[b * GRP_UNIT_U4];
    const uint32_t c = (uint32_t)__popcll(grp_bitmap(hd));
    const uint64_t base = f.super[b >> GRP_SUPER_SHIFT] + hd.x;
    for (uint32_t lr = 0; lr < c; ++lr) {
      const uint64_t rank = base + lr;
      if (rank >= first && rank < first + n) {
        if (ids) {
          if (lr < GRP_BUCKET_IDS) {
            reinterpret_cast<uint32_t*>(f.buckets)[grp_id_loc(b, lr)] = ids[rank - first];
          } else {
            grp_ovf_put(f, rank, ids[rank - first]);
          }
        }
        if (counts) {
          unsigned long long* cwp = grp_cw_ptr(f, b, lr, rank);
          *cwp = grp_cnt_with(*cwp, counts[rank - first]);
        }
      }
    }
  }
}

__global__ void
k_debug_locate(const uint64_t* __restrict__ x, uint64_t n, uint64_t m, uint64_t m_inv, uint32_t W, uint64_t w_magic, uint64_t* __restrict__ mod_out, uint64_t* __restrict__ div_out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint64_t r = grp_mod_m(x[i], m, m_inv);
    mod_out[i] = r;
    div_out[i] = grp_div_w(r, w_magic);
  }
}

template<int H, int WT>
__device__ __forceinline__ void
debug_tile_hashes(const DevReads& rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint32_t read_idx, uint32_t tile_idx, uint64_t* __restrict__ out, uint64_t cap)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);
  const uint32_t len = rd.len[read_idx];
  const gr::geom::TileExtent ext = tile_extent(sd, tile_len, len, tile_idx);
  const uint32_t start = ext.start, Lp = ext.Lp, frames = ext.frames;
  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[read_idx], len, start, Lp);
  __syncthreads();
  for (uint32_t fr = threadIdx.x; fr < frames; fr += THREADS) {
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (!seed_on<H>(s, hn)) {
        continue;
      }
      const uint32_t fs = min(fr, Lp - sd->span[s]);
      uint64_t hv = seed_hash_t<WT>(sTab, sd, s, window_at(sBases, boff + fs));
      uint64_t o = (uint64_t)fr * hn + s;
      if (o < cap) {
        out[o] = hv;
      }
    }
  }
}

// WT: 0, or GRP_WT_LONG for seeds of spans beyond 64 bases (DevSeeds::wide == 2)
template<int H, int WT = 0>
__global__ void __launch_bounds__(THREADS)
k_debug_tile_hashes(DevReads rd, const DevSeeds* __restrict__ sd, uint32_t tile_len, uint32_t read_idx, uint32_t tile_idx, uint64_t* __restrict__ out, uint64_t cap)
{
  debug_tile_hashes<H, WT>(rd, sd, tile_len, read_idx, tile_idx, out, cap);
}
