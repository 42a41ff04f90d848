// --ntcard on the GPU (include/grpath.h "ntCard"; SURVEY.md §8(f) N4).  Included at
// the end of grpath_hip.hip (same translation unit: grp_ctx, seed_hash, stage_bases).
//
// Reference: goldrush_path/ntcard.hpp — stRead (:96-112) walks the
// multiLensfrHashIterator over the whole record and feeds every seed's hash to
// ntComp (:81-94), which samples ~3/2^(sBits+1) of the hash space into two tables of
// 2^27 uint16 counters per seed; compEst (:114-154) / calc_ntcard_genome_size
// (:248-275) only consume the number of zero buckets (F0).
//
//   k_ntcard        same hash stream as k_fill; sampled hashes -> atomicAdd on 32-bit
//                   counters (the reference's uint16 wrap is applied when counting zeros)
//   k_ntcard_zeros  buckets whose low 16 bits are zero, per seed and sample table

namespace {

constexpr uint32_t NTC_RBITS = 27; // nts::rBits (ntcard.hpp:34)
constexpr uint32_t NTC_NSAMP = 2;  // nts::nSamp (ntcard.hpp:38)

// WT: 0, or GRP_WT_LONG for seeds of spans beyond 64 bases (DevSeeds::wide == 2)
template<int H, int WT = 0>
__global__ void __launch_bounds__(THREADS)
k_ntcard(DevReads rd,
         const DevSeeds* __restrict__ sd,
         const uint2* __restrict__ chunks, // (read, chunk index inside the read)
         const uint32_t* __restrict__ extra, // [read - first][h] stale repeats of the last window, or nullptr
         uint32_t first,
         uint32_t* __restrict__ counters,
         uint32_t sbits)
{
  extern __shared__ uint4 smem4[];
  ulonglong2* sTab = reinterpret_cast<ulonglong2*>(smem4);
  const uint32_t hn = frame_seeds<H>(sd);
  uint32_t* sBases = reinterpret_cast<uint32_t*>(sTab + hn * sd->wmax * 4u);

  const uint2 ck = chunks[blockIdx.x];
  const uint32_t r = ck.x;
  const uint32_t len = rd.len[r];
  const uint32_t s0 = sd->span[0];     // the shortest seed: k, or k - 1 at odd k
  const uint32_t npos = len - s0 + 1u; // listed => len >= s0
  const uint32_t p0 = ck.y * FILL_CHUNK;
  const uint32_t np = min(FILL_CHUNK, npos - p0);

  load_tab(sTab, sd);
  const uint32_t boff = stage_bases(sBases, rd.packed, rd.word_off[r], len, p0, np + s0 + hn - 2u);
  __syncthreads();

  const uint64_t smask = (1ull << (sbits - 1u)) - 1ull; // ntcard.hpp:182
  for (uint32_t i = threadIdx.x; i < np; i += THREADS) {
    const uint32_t p = p0 + i;
    const Win w = window_at(sBases, boff + i);
#pragma unroll
    for (int s = 0; s < H; ++s) {
      if (!seed_on<H>(s, hn)) {
        continue;
      }
      const uint32_t span = sd->span[s];
      if (p + span > len) {
        continue; // no window of seed s starts here
      }
      const uint64_t hv = seed_hash_t<WT>(sTab, sd, s, w);
      // ntComp (:81-94)
      uint32_t ind = NTC_NSAMP;
      if ((hv >> (63u - sbits)) == 1ull) {
        ind = 0;
      }
      if ((hv >> (64u - sbits)) == smask) {
        ind = 1;
      }
      if (ind < NTC_NSAMP) {
        // the seed's last window is counted again for every frame it stays stale:
        // span_s - span_0 frames for a plain read, or what the host computed
        uint32_t times = 1u;
        if (p + span == len) {
          times += extra ? extra[(size_t)(r - first) * hn + s] : (span - s0);
        }
        const uint64_t slot = (((uint64_t)s * NTC_NSAMP + ind) << NTC_RBITS) | (hv & ((1ull << NTC_RBITS) - 1ull));
        atomicAdd(&counters[slot], times);
      }
    }
  }
}

__global__ void __launch_bounds__(THREADS)
k_ntcard_zeros(const uint32_t* __restrict__ counters, unsigned long long* __restrict__ zeros)
{
  // grid = (blocks per table, tables); a table has 2^27 counters
  const uint32_t table = blockIdx.y;
  const uint4* t = reinterpret_cast<const uint4*>(counters + ((uint64_t)table << NTC_RBITS));
  const uint32_t n4 = 1u << (NTC_RBITS - 2);
  uint32_t z = 0;
  for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < n4; i += gridDim.x * THREADS) {
    const uint4 v = t[i];
    z += ((v.x & 0xFFFFu) == 0u) + ((v.y & 0xFFFFu) == 0u) + ((v.z & 0xFFFFu) == 0u) + ((v.w & 0xFFFFu) == 0u);
  }
  z = wave_sum(z);
  if ((threadIdx.x & 63u) == 0u && z) {
    atomicAdd(&zeros[table], (unsigned long long)z);
  }
}

} // namespace

extern "C" {

int
grp_ntcard_begin(grp_ctx* c, uint32_t sbits)
{
  if (!c || sbits < 2 || sbits > 32) {
    return set_err(c, GRP_ERR_INVALID, "grp_ntcard_begin: bad argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n = ((uint64_t)c->params.h * NTC_NSAMP) << NTC_RBITS;
  if (!c->d_ntc) {
    HIP_TRY(c, c->d_ntc.reset(n));
  }
  HIP_TRY(c, hipMemsetAsync(c->d_ntc, 0, n * sizeof(uint32_t), c->stream));
  c->ntc_sbits = sbits;
  return GRP_OK;
}

int
grp_ntcard_add(grp_ctx* c, const grp_reads* r, uint32_t first, uint32_t count, const uint32_t* stale_extra)
{
  if (!c || !r || r->ctx != c || (uint64_t)first + count > r->n_reads) {
    return set_err(c, GRP_ERR_INVALID, "grp_ntcard_add: bad range");
  }
  if (!c->d_ntc) {
    return set_err(c, GRP_ERR_STATE, "grp_ntcard_add before grp_ntcard_begin");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t s0 = span0(c), h = c->params.h;
  std::vector<uint2> chunks;
  uint64_t hashes = 0;
  for (uint32_t i = first; i < first + count; ++i) {
    const uint32_t len = r->len[i];
    if (len < s0) {
      continue; // no window of any seed
    }
    const uint32_t nch = (len - s0 + 1 + FILL_CHUNK - 1) / FILL_CHUNK;
    for (uint32_t j = 0; j < nch; ++j) {
      chunks.push_back(make_uint2(i, j));
    }
    for (uint32_t s = 0; s < h; ++s) {
      const uint32_t span = c->h_seeds.span[s];
      hashes += len >= span ? len - span + 1 : 0;
    }
  }
  if (chunks.empty()) {
    return GRP_OK;
  }
  if (chunks.size() > MAX_GRID_WGS) { // 2^22 chunks = 8.6 G bases per call
    return set_err(c, GRP_ERR_INVALID, "grp_ntcard_add: too many bases in one call");
  }
  int rc = ensure_dev(c, c->d_ntc_chunks, chunks.size());
  if (rc == GRP_OK && stale_extra) {
    rc = ensure_dev(c, c->d_ntc_extra, (uint64_t)count * h);
  }
  if (rc != GRP_OK) {
    return rc;
  }
  // pageable sources: the copies return once the host buffers have been consumed
  HIP_TRY(c, hipMemcpyAsync(c->d_ntc_chunks, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
  if (stale_extra) {
    HIP_TRY(c, hipMemcpyAsync(c->d_ntc_extra, stale_extra, (size_t)count * h * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  }
  const size_t lds = tab_bytes(c) + bases_bytes(FILL_CHUNK + c->params.k + c->params.h);
  {
    Timer t(c, GRP_K_NTCARD, hashes);
    DISPATCH_H_SPAN(c, (k_ntcard<HH, WW><<<dim3((uint32_t)chunks.size()), dim3(THREADS), lds, c->stream>>>(
                         r->dev, c->d_seeds, c->d_ntc_chunks, stale_extra ? c->d_ntc_extra : nullptr, first, c->d_ntc, c->ntc_sbits)));
    HIP_TRY(c, hipGetLastError());
  }
  // `chunks` (and the caller's array) must outlive the copies
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_ntcard_finish(grp_ctx* c, uint64_t* zero_buckets)
{
  if (!c || !zero_buckets) {
    return set_err(c, GRP_ERR_INVALID, "grp_ntcard_finish: bad argument");
  }
  if (!c->d_ntc) {
    return set_err(c, GRP_ERR_STATE, "grp_ntcard_finish before grp_ntcard_begin");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t tables = c->params.h * NTC_NSAMP;
  DevBuf<unsigned long long> d_z;
  HIP_TRY(c, d_z.reset(tables));
  hipError_t e = hipMemsetAsync(d_z, 0, tables * sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) {
    k_ntcard_zeros<<<dim3(2048, tables), dim3(THREADS), 0, c->stream>>>(c->d_ntc, d_z);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    e = hipMemcpyAsync(zero_buckets, d_z, tables * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess) {
    e = hipStreamSynchronize(c->stream);
  }
  clear_all(d_z, c->d_ntc);
  if (e != hipSuccess) {
    return set_err(c, GRP_ERR_HIP, "grp_ntcard_finish: %s", hipGetErrorString(e));
  }
  return GRP_OK;
}

} // extern "C"
