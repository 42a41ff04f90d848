// Slices of packed reads cut into a new batch on the device (grp_reads_gather), a batch read back (grp_reads_download) and
// a context returned to its fill state (grp_rewind) — the device pieces of a run that hands the reads one stage has
// written to the next stage without their text (include/grpath.h).
//   k_reads_gather   one workgroup per slice: output word j is the funnel shift of two neighbouring source words
//                    (host/gr_gather_word.hpp, which the host check compiles too)

namespace {

// One workgroup per slice, as k_fq_pack takes one per record, not a flat grid over the output words: the slices of a run
// are whole reads or tile-aligned stretches of reads (thousands of bases, hundreds of words: every lane has work for
// several rounds), and a flat grid would have every lane search the slice that owns its word.  (Neither form has been
// timed against the other.)  Lane t of a round loads source words j and j + 1 — both as 32-bit loads that are contiguous
// across the wave, the second one served by the cache line the first one brought — and stores output word j.
__global__ void __launch_bounds__(THREADS)
k_reads_gather(const GatherSrc* __restrict__ srcs, const grp_read_slice* __restrict__ slices, const uint64_t* __restrict__ out_word_off, uint32_t* __restrict__ out_packed, uint32_t slice0)
{
  const uint32_t i = slice0 + blockIdx.x;
  const grp_read_slice sl = slices[i];
  const GatherSrc s = srcs[sl.src];
  const uint32_t* src = s.packed + s.word_off[sl.read] + (sl.first_base >> 4);
  uint32_t* dst = out_packed + out_word_off[i];
  const uint32_t shift = sl.first_base & 15u;
  const uint32_t nw = gr::gather_words(sl.n_bases);
  for (uint32_t j = threadIdx.x; j < nw; j += THREADS) {
    dst[j] = gr::gather_out_word(src, shift, sl.n_bases, j);
  }
}

} // namespace

extern "C" {

int
grp_reads_gather(grp_ctx* c, const grp_reads* const* srcs, uint32_t n_srcs, const grp_read_slice* slices, uint32_t n_slices, grp_reads** out)
{
  if (!c || !out || (!srcs && n_srcs) || (!slices && n_slices)) {
    return set_err(c, GRP_ERR_INVALID, "grp_reads_gather: null argument");
  }
  *out = nullptr;
  // everything is checked here, in front of any launch: the kernel trusts its table
  for (uint32_t s = 0; s < n_srcs; ++s) {
    if (!srcs[s] || srcs[s]->ctx != c) {
      return set_err(c, GRP_ERR_INVALID, "grp_reads_gather: source %u is not a batch of this context", s);
    }
  }
  for (uint32_t i = 0; i < n_slices; ++i) {
    const grp_read_slice& sl = slices[i];
    if (sl.src >= n_srcs) {
      return set_err(c, GRP_ERR_INVALID, "grp_reads_gather: slice %u names source %u of %u", i, sl.src, n_srcs);
    }
    const grp_reads* r = srcs[sl.src];
    if (sl.read >= r->n_reads) {
      return set_err(c, GRP_ERR_INVALID, "grp_reads_gather: slice %u names read %u of a batch of %u", i, sl.read, r->n_reads);
    }
    if (sl.n_bases == 0 || (uint64_t)sl.first_base + sl.n_bases > r->len[sl.read]) {
      return set_err(c, GRP_ERR_INVALID, "grp_reads_gather: slice %u: bases [%u, %llu) of a read of %u", i, sl.first_base, (unsigned long long)sl.first_base + sl.n_bases, r->len[sl.read]);
    }
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_reads* rd = new grp_reads();
  std::vector<uint64_t>& word_off = rd->h_word_off; // (the copies below read these: they stay with the batch)
  rd->h_slices.assign(slices, slices + n_slices);
  rd->h_srcs.resize(n_srcs);
  for (uint32_t s = 0; s < n_srcs; ++s) {
    rd->h_srcs[s] = GatherSrc{ srcs[s]->dev.packed, srcs[s]->dev.word_off };
  }
  word_off.resize((size_t)n_slices + 1);
  std::vector<uint32_t> len(n_slices);
  uint64_t w = 0;
  for (uint32_t i = 0; i < n_slices; ++i) {
    len[i] = slices[i].n_bases;
    word_off[i] = w;
    w += gr::gather_words(slices[i].n_bases);
  }
  word_off[n_slices] = w;
  auto bail = [&](int code) {
    grp_reads_free(rd);
    return code;
  };
  // an ordinary engine-owned batch, laid out as grp_fastq_pack lays its batches out: the packed words (+ 4) and one slab
  // behind all index arrays, here with the slice and source tables at its end
  int rc = reads_index(c, rd, word_off.data(), len.data(), n_slices);
  if (rc != GRP_OK) {
    return bail(rc);
  }
  const uint64_t nt = rd->tile0[n_slices], nch = rd->chunk0[n_slices];
  const auto up8 = [](uint64_t b) { return (b + 15) & ~(uint64_t)15; };
  const uint64_t n1 = (uint64_t)n_slices + 1;
  const uint64_t o_wo = 0, o_t0 = o_wo + up8(n1 * 8), o_c0 = o_t0 + up8(n1 * 8), o_len = o_c0 + up8(n1 * 8);
  const uint64_t o_tr = o_len + up8(std::max<uint64_t>(n_slices, 1) * 4), o_cr = o_tr + up8(std::max<uint64_t>(nt, 1) * 4), o_sl = o_cr + up8(std::max<uint64_t>(nch, 1) * 4);
  const uint64_t o_src = o_sl + up8(std::max<uint64_t>(n_slices, 1) * sizeof(grp_read_slice));
  const uint64_t slab_bytes = o_src + up8(std::max<uint64_t>(n_srcs, 1) * sizeof(GatherSrc));
  if (rd->d_packed.reset(std::max<uint64_t>(w, 1) + 4) != hipSuccess || rd->d_slab.reset(slab_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return bail(set_err(c, GRP_ERR_NOMEM, "grp_reads_gather: allocating %llu words + %llu bytes of device memory failed", (unsigned long long)w, (unsigned long long)slab_bytes));
  }
  uint8_t* const slab = rd->d_slab;
  uint64_t* const d_word_off = reinterpret_cast<uint64_t*>(slab + o_wo);
  uint64_t* const d_tile0 = reinterpret_cast<uint64_t*>(slab + o_t0);
  uint64_t* const d_chunk0 = reinterpret_cast<uint64_t*>(slab + o_c0);
  uint32_t* const d_len = reinterpret_cast<uint32_t*>(slab + o_len);
  uint32_t* const d_tile_read = reinterpret_cast<uint32_t*>(slab + o_tr);
  uint32_t* const d_chunk_read = reinterpret_cast<uint32_t*>(slab + o_cr);
  grp_read_slice* const d_slices = reinterpret_cast<grp_read_slice*>(slab + o_sl);
  GatherSrc* const d_srcs = reinterpret_cast<GatherSrc*>(slab + o_src);
  hipError_t e = hipMemcpyAsync(d_word_off, word_off.data(), n1 * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tile0, rd->tile0.data(), n1 * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_chunk0, rd->chunk0.data(), n1 * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_slices) e = hipMemcpyAsync(d_len, rd->len.data(), (size_t)n_slices * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && nt) e = hipMemcpyAsync(d_tile_read, rd->h_tile_read.data(), nt * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && nch) e = hipMemcpyAsync(d_chunk_read, rd->h_chunk_read.data(), nch * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_slices) e = hipMemcpyAsync(d_slices, rd->h_slices.data(), (size_t)n_slices * sizeof(grp_read_slice), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_slices) e = hipMemcpyAsync(d_srcs, rd->h_srcs.data(), (size_t)n_srcs * sizeof(GatherSrc), hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) {
    return bail(set_err(c, GRP_ERR_HIP, "grp_reads_gather: upload failed: %s", hipGetErrorString(e)));
  }
  for (uint32_t s0 = 0; s0 < n_slices;) { // (a grid holds at most MAX_GRID_WGS workgroups)
    const uint32_t nb = std::min<uint32_t>(n_slices - s0, MAX_GRID_WGS);
    k_reads_gather<<<dim3(nb), dim3(THREADS), 0, c->stream>>>(d_srcs, d_slices, d_word_off, rd->d_packed, s0);
    if (hipGetLastError() != hipSuccess) {
      return bail(set_err(c, GRP_ERR_HIP, "grp_reads_gather: kernel launch failed"));
    }
    s0 += nb;
  }
  rd->dev.packed = rd->d_packed;
  rd->dev.word_off = d_word_off;
  rd->dev.len = d_len;
  rd->dev.tile0 = d_tile0;
  rd->dev.tile_read = d_tile_read;
  rd->dev.chunk0 = d_chunk0;
  rd->dev.chunk_read = d_chunk_read;
  *out = rd;
  return GRP_OK;
}

int
grp_reads_download(const grp_reads* r, uint32_t* packed, uint64_t n_words, uint64_t* word_off, uint32_t* len)
{
  if (!r || !r->ctx) {
    return GRP_ERR_INVALID;
  }
  grp_ctx* c = r->ctx;
  if (packed && n_words < r->n_words) {
    return set_err(c, GRP_ERR_INVALID, "grp_reads_download: room for %llu words, the batch has %llu", (unsigned long long)n_words, (unsigned long long)r->n_words);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a batch may still be on its way: grp_fastq_pack and grp_reads_gather are asynchronous)
  if (packed && r->n_words) {
    HIP_TRY(c, hipMemcpy(packed, r->dev.packed, r->n_words * 4, hipMemcpyDeviceToHost));
  }
  if (word_off) {
    HIP_TRY(c, hipMemcpy(word_off, r->dev.word_off, ((size_t)r->n_reads + 1) * 8, hipMemcpyDeviceToHost));
  }
  if (len && r->n_reads) {
    HIP_TRY(c, hipMemcpy(len, r->dev.len, (size_t)r->n_reads * 4, hipMemcpyDeviceToHost));
  }
  return GRP_OK;
}

int
grp_rewind(grp_ctx* c)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (c->slot[0].busy || c->slot[1].busy) {
    return set_err(c, GRP_ERR_STATE, "grp_rewind: a window is outstanding (end it first)");
  }
  if (c->batch.active) {
    return set_err(c, GRP_ERR_STATE, "grp_rewind: a batch is outstanding (grp_batch_end / grp_batch_undo first)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream3));
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->pre.worker.joinable()) {
    c->pre.worker.join();
  }
  // the phase-2 tables go, prepared or in use: the next grp_finalize sizes its own from the occupancy it measures
  clear_all(c->buckets, c->far, c->ovf_keys, c->ovf_ids, c->d_super, c->pre.units, c->pre.far);
  c->pre.units_buckets = 0;
  c->pre.started = false;
  c->pre.occupancy = 0.0;
  const uint64_t m = c->f.m, m_inv = c->f.m_inv;
  c->f = DevFilter{};
  c->f.m = m;
  c->f.m_inv = m_inv;
  c->nsb = c->n_ovf = c->n_far = c->n_chunks = 0;
  c->finalized = false;
  if (m != 0) {
    // phase 1 again: the bit vector (grp_finalize has released it), zero
    if (!c->bv) {
      if (c->bv.reset(c->n_bv_words + 3) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, GRP_ERR_NOMEM, "grp_rewind: allocating the bit vector of %llu bits failed", (unsigned long long)m);
      }
    }
    c->f.bv = c->bv;
    HIP_TRY(c, hipMemsetAsync(c->f.bv, 0, (c->n_bv_words + 3) * sizeof(uint32_t), c->stream));
  }
  // counters, and what is left of windows and batches
  c->carry.valid = false;
  c->batch.epoch = 0; // (the claims went with the count words)
  for (QuerySlot& sl : c->slot) {
    sl.reads = nullptr;
    sl.win.streaming = sl.win.resumable = false;
  }
  c->ingest.n_pre = 0; // (bodies uploaded ahead of a parse that never came)
  c->n_overlap_calls = c->n_batch_sweeps = 0;
  for (uint64_t& v : c->n_stream_keep) {
    v = 0;
  }
  c->n_stream_idle_exits = c->n_stream_coop_refused = 0;
  c->n_flagged_tiles = c->n_flagged_distinct = c->n_flagged_list = 0;
  c->n_verify_impossible = c->n_verify_tiles = c->n_verify_queried = c->n_verify_flagged = c->n_verify_fallbacks = c->n_verify_uncertified = c->n_verify_unpatched = 0;
  c->n_direct_windows = c->n_direct_fallbacks = c->n_general_windows = c->n_redo_launches = 0;
  for (double& v : c->finalize_times) {
    v = 0.0;
  }
  drain_events(c); // (every launch has ended: its time is taken, then dropped with the rest)
  for (grp_kernel_stat& k : c->kstat) {
    k = grp_kernel_stat{};
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

} // extern "C"
