// extern "C" surface of libgrpath_host.so (include/grpath_host.h).
#include "../../../include/grpath_host.h"
#include "gr_classifier.hpp"
#include "gr_params.hpp"
#include "gr_opts.hpp"
#include <algorithm>
#include <sstream>
#include "gr_tiles.hpp"
#include "gr_fastq.hpp"
#include "gr_gzidx.hpp"
#include "gr_gzwalk.hpp"

#include <cstddef>
#include <cstring>
#include <new>

extern "C" {

int
gr_make_seed_pattern(const char* preset, unsigned k, unsigned weight, unsigned h, char* out, size_t stride, int log_to_stderr)
{
  if (!out || k / 2 == 0) {
    return -1;
  }
  auto seeds = gr::make_seed_pattern(preset ? preset : "", k, weight, h, log_to_stderr != 0);
  for (unsigned i = 0; i < h; ++i) {
    if (seeds[i].size() + 1 > stride) {
      return -1;
    }
    std::memcpy(out + (size_t)i * stride, seeds[i].c_str(), seeds[i].size() + 1);
  }
  return 0;
}

uint64_t
gr_hash_universe(uint64_t weight, uint64_t genome_size, uint64_t hash_num)
{
  return gr::hash_universe(weight, genome_size, hash_num);
}

uint64_t
gr_calc_optimal_size(uint64_t entries, unsigned hash_num, double occupancy)
{
  return gr::calc_optimal_size(entries, hash_num, occupancy);
}

void
gr_calc_phred_average(const char* qual, size_t n, uint32_t* avg, uint32_t* delta)
{
  gr::calc_phred_average(qual, n, *avg, *delta);
}

double
gr_sum_phred(const char* qual, size_t n)
{
  return gr::sum_phred(qual, n);
}

int
gr_process_options_dump(int argc, char** argv, char* out, size_t cap)
{
  gr::Opts o;
  const int rc = gr::process_options(o, argc, argv);
  std::ostringstream ss;
  ss << "assigned_max=" << o.assigned_max << "\n"
     << "unassigned_min=" << o.unassigned_min << "\n"
     << "tile_length=" << o.tile_length << "\n"
     << "block_size=" << o.block_size << "\n"
     << "hash_universe=" << o.hash_universe << "\n"
     << "genome_size=" << o.genome_size << "\n"
     << "kmer_size=" << o.kmer_size << "\n"
     << "phred_min=" << o.phred_min << "\n"
     << "phred_delta=" << o.phred_delta << "\n"
     << "weight=" << o.weight << "\n"
     << "min_length=" << o.min_length << "\n"
     << "hash_num=" << o.hash_num << "\n"
     << "occupancy=" << o.occupancy << "\n"
     << "ratio=" << o.ratio << "\n"
     << "jobs=" << o.jobs << "\n"
     << "max_paths=" << o.max_paths << "\n"
     << "threshold=" << o.threshold << "\n"
     << "prefix_file=" << o.prefix_file << "\n"
     << "input=" << o.input << "\n"
     << "seed_preset=" << o.seed_preset << "\n"
     << "filter_file=" << o.filter_file << "\n"
     << "help=" << o.help << "\n"
     << "ntcard=" << o.ntcard << "\n"
     << "silver_path=" << o.silver_path << "\n"
     << "verbose=" << o.verbose << "\n"
     << "debug=" << o.debug << "\n";
  const std::string t = ss.str();
  if (out && cap) {
    const size_t n = std::min(cap - 1, t.size());
    std::memcpy(out, t.data(), n);
    out[n] = '\0';
  }
  return rc;
}

int
gr_inputs_dump(int argc, char** argv, char* out, size_t cap)
{
  gr::Opts o;
  int rc = gr::process_options(o, argc, argv);
  std::ostringstream ss;
  ss << "input=" << o.input << "\n";
  for (const std::string& i : o.inputs) {
    ss << "inputs=" << i << "\n";
  }
  std::vector<std::string> files;
  std::string err;
  if (gr::expand_inputs(o.inputs, files, err)) {
    for (const std::string& f : files) {
      ss << "file=" << f << "\n";
    }
  } else {
    ss << "error=" << err << "\n";
    rc = rc < 0 ? 1 : rc;
  }
  const std::string t = ss.str();
  if (out && cap) {
    const size_t n = std::min(cap - 1, t.size());
    std::memcpy(out, t.data(), n);
    out[n] = '\0';
  }
  return rc;
}

unsigned
gr_ntcard_sbits(uint64_t input_bytes)
{
  return gr::ntcard_sbits(input_bytes);
}

uint64_t
gr_ntcard_f0(uint64_t zero0, uint64_t zero1, unsigned sbits)
{
  return gr::ntcard_f0(zero0, zero1, sbits);
}

size_t
gr_ntcard_split(const char* seq, size_t n, unsigned k, unsigned h, uint64_t* run_off, uint64_t* run_len, uint32_t* extra, size_t cap)
{
  std::vector<std::pair<size_t, size_t>> runs;
  std::vector<uint32_t> ex;
  gr::ntcard_split(seq, n, k, h, runs, ex);
  for (size_t r = 0; r < runs.size() && r < cap; ++r) {
    run_off[r] = runs[r].first;
    run_len[r] = runs[r].second;
    for (unsigned s = 0; s < h; ++s) {
      extra[r * h + s] = ex[r * h + s];
    }
  }
  return runs.size();
}

unsigned
gr_effective_cpus(void)
{
  return gr::effective_cpus();
}

int
gr_pack_2bit(const char* seq, size_t n, uint32_t* out_words)
{
  return gr::pack_2bit(seq, n, out_words) ? 0 : -1;
}

void
gr_decide_read(size_t threshold, size_t unassigned_min, size_t assigned_max, size_t num_tiles, const grp_tile_summary* tiles, const grp_id_count* lists, gr_read_decision* out)
{
  gr::TileWorkspace ws;
  gr::ReadDecision d;
  gr::decide_read(gr::DecideParams{ threshold, unassigned_min, assigned_max }, num_tiles, tiles, lists, ws, d);
  std::memcpy(out, &d, sizeof(d));
}

size_t
gr_smooth_tiles(size_t num_tiles, const grp_tile_summary* tiles, const grp_id_count* lists, size_t threshold, uint32_t* ids_out, uint8_t* bools_out)
{
  gr::TileWorkspace ws;
  size_t n = gr::smooth_tiles(num_tiles, tiles, lists, threshold, ws);
  for (size_t i = 0; i < num_tiles; ++i) {
    ids_out[i] = ws.ids[i];
    bools_out[i] = ws.asg[i];
  }
  return n;
}

void
gr_find_longest_stretch(const uint8_t* bools, size_t num_tiles, long* start, long* end)
{
  std::vector<uint8_t> b(bools, bools + num_tiles);
  gr::find_longest_stretch(b, num_tiles, *start, *end);
}

int
gr_eval_flanks(long ls, long le, const uint32_t* ids, size_t num_tiles, size_t* trim_start, size_t* trim_end)
{
  return gr::eval_flanks(ls, le, ids, num_tiles, *trim_start, *trim_end) ? 1 : 0;
}

struct gr_classifier
{
  gr::Classifier impl;
  gr_classifier(const gr_classifier_params& p, const grp_engine_vt& vt, void* ctx)
    : impl(p, vt, ctx)
  {}
};

int
gr_classifier_create(const gr_classifier_params* p, const grp_engine_vt* vt, void* engine_ctx, gr_classifier** out)
{
  // (callers built before seed0_span pass the shorter struct: the field is 0 for them)
  if (!p || !vt || !out || (p->struct_size != sizeof(gr_classifier_params) && p->struct_size != offsetof(gr_classifier_params, seed0_span)) || p->tile_length == 0 ||
      p->block_size == 0) {
    return GRP_ERR_INVALID;
  }
  gr_classifier_params q{};
  memcpy(&q, p, p->struct_size);
  q.struct_size = sizeof(q);
  *out = new (std::nothrow) gr_classifier(q, *vt, engine_ctx);
  return *out ? GRP_OK : GRP_ERR_NOMEM;
}

void
gr_classifier_destroy(gr_classifier* c)
{
  delete c;
}

void
gr_classifier_keep_commits(gr_classifier* c, uint32_t first0, uint32_t count0, uint32_t first1, uint32_t count1)
{
  if (c) {
    c->impl.keep_commits(first0, count0, first1, count1);
  }
}

size_t
gr_classifier_kept_commits(const gr_classifier* c, gr_commit* out, size_t cap)
{
  if (!c) {
    return 0;
  }
  const auto& k = c->impl.kept_commits();
  for (size_t i = 0; i < k.size() && i < cap; ++i) {
    out[i] = k[i];
  }
  return k.size();
}

void
gr_classifier_set_debug(gr_classifier* c, gr_debug_fn fn)
{
  if (c) {
    c->impl.set_debug(fn);
  }
}

void
gr_classifier_set_settle(gr_classifier* c, gr_settle_fn fn, void* user)
{
  if (c) {
    c->impl.set_settle(fn, user);
  }
}

void
gr_classifier_set_allgather(gr_classifier* c, gr_allgather_fn allgather, void* allgather_user)
{
  if (c) {
    c->impl.set_allgather(allgather, allgather_user);
  }
}

void
gr_classifier_set_callbacks(gr_classifier* c, gr_commit_fn commit, gr_rollover_fn rollover, gr_allgather_fn allgather, void* user)
{
  c->impl.set_callbacks(commit, rollover, allgather, user);
}

int
gr_classifier_run(gr_classifier* c, void* reads, const uint32_t* lens, uint32_t n_reads, const uint32_t* skipped_before, uint32_t skipped_after, int* finished)
{
  return gr_classifier_run_range(c, reads, lens, 0, n_reads, skipped_before, skipped_after, finished);
}

int
gr_classifier_run_range(gr_classifier* c, void* reads, const uint32_t* lens, uint32_t first, uint32_t count, const uint32_t* skipped_before, uint32_t skipped_after, int* finished)
{
  bool fin = false;
  int rc = c->impl.run(reads, lens, first, count, skipped_before, skipped_after, fin);
  if (finished) {
    *finished = fin ? 1 : 0;
  }
  return rc;
}

const char*
gr_classifier_error(const gr_classifier* c)
{
  return c->impl.error().c_str();
}

void
gr_classifier_get_state(const gr_classifier* c, gr_classifier_state* out)
{
  c->impl.get_state(*out);
}

uint64_t
gr_input_read(const char* path, uint64_t request_bytes, char* dst, uint64_t cap)
{
  gr::InputFile in(path ? path : "");
  if (!in.ok()) {
    return UINT64_MAX;
  }
  uint64_t got = 0;
  while (got < cap) {
    const size_t k = in.read(dst + got, (size_t)std::min<uint64_t>(std::max<uint64_t>(request_bytes, 1), cap - got));
    if (k == 0) {
      break;
    }
    got += k;
  }
  return got;
}

struct gr_gzidx
{
  std::unique_ptr<gr::GzIndexReader> rd; // (none: the handle of gr_gzidx_build_device)
  std::unique_ptr<gr::GzIndex> idx; // the complete index, else rd->partial()
  uint64_t n_text = 0;
  const char* left = nullptr; // the walk: why the file was left to zlib ...
  uint32_t left_status = 0;   // ... and the decoder's status, where that was the reason
  const gr::GzIndex* get() const { return idx ? idx.get() : rd ? rd->partial() : nullptr; }
};

gr_gzidx*
gr_gzidx_build(const char* path, uint64_t span, uint64_t max_bytes, uint64_t stop_after, char* text_out, uint64_t text_cap)
{
  std::unique_ptr<gr_gzidx> h(new (std::nothrow) gr_gzidx);
  if (!h) {
    return nullptr;
  }
  h->rd.reset(new gr::GzIndexReader(path ? path : "", span, max_bytes));
  if (!h->rd->ok()) {
    return nullptr;
  }
  std::vector<char> piece(size_t(1) << 16);
  for (;;) {
    if (stop_after && h->n_text >= stop_after) {
      break;
    }
    const bool direct = text_out && h->n_text < text_cap;
    const size_t k = direct ? h->rd->read(text_out + h->n_text, (size_t)std::min<uint64_t>(text_cap - h->n_text, piece.size())) : h->rd->read(piece.data(), piece.size());
    if (k == 0) {
      break;
    }
    h->n_text += k;
  }
  h->idx = h->rd->take();
  return h.release();
}

void
gr_gzidx_info(const gr_gzidx* h, uint64_t out[8])
{
  const gr::GzIndex* ix = h->get();
  out[0] = h->idx != nullptr;
  out[1] = ix ? ix->segs.size() : 0;
  out[2] = h->n_text;
  out[3] = ix ? ix->bytes() : 0;
  out[4] = (h->rd ? h->rd->dropped() : true) && !h->idx;
  out[5] = h->rd ? h->rd->failed() : false;
  out[6] = ix ? ix->max_text : 0;
  out[7] = ix ? ix->file_size : 0;
}

int
gr_gzidx_segment(const gr_gzidx* h, uint64_t i, grp_gzip_segment* seg, unsigned char* dict)
{
  const gr::GzIndex* ix = h->get();
  if (!ix || i >= ix->segs.size() || !seg) {
    return -1;
  }
  const gr::GzSegment& g = ix->segs[(size_t)i];
  *seg = grp_gzip_segment{ g.comp_bit, g.n_bits, 0, g.dict_len, g.text_len, g.crc32, g.flags };
  if (dict && g.dict_len) {
    std::memcpy(dict, ix->dict(g), g.dict_len);
  }
  return 0;
}

int
gr_gzidx_matches(const gr_gzidx* h, const char* path)
{
  const gr::GzIndex* ix = h->get();
  return ix && path && ix->matches(path) ? 1 : 0;
}

namespace {

int
gzidx_build_device(const grp_engine_ext* ext, void* engine_ctx, const char* const* paths, uint32_t n, uint64_t span, uint64_t max_bytes, const gr::GzWalkMembers& members, gr_gzidx** out, uint64_t* stats, size_t n_stats)
{
  if (!ext || ext->struct_size < offsetof(grp_engine_ext, gzip_walk) + sizeof(ext->gzip_walk) || !ext->gzip_walk || (n && (!paths || !out))) {
    return -1;
  }
  std::vector<std::string> files;
  for (uint32_t i = 0; i < n; ++i) {
    files.push_back(paths[i] ? paths[i] : "");
  }
  const auto launch = [&](const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n_steps, grp_gzip_walk_result* res, uint8_t* hist) {
    return ext->gzip_walk(engine_ctx, comp, n_comp, dict, n_dict, steps, n_steps, res, hist, nullptr, 0, nullptr) == GRP_OK;
  };
  gr::GzWalkStats st;
  std::vector<gr::GzWalkFile> got = gr::gzip_walk(files, span, max_bytes, gr::gzip_walk_sizes(), launch, &st, nullptr, nullptr, members);
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = nullptr;
    if (got[i].unreadable) {
      continue;
    }
    out[i] = new gr_gzidx;
    out[i]->n_text = got[i].index ? got[i].index->text_bytes : 0;
    out[i]->idx = std::move(got[i].index);
    out[i]->left = got[i].left;
    out[i]->left_status = got[i].status;
  }
  if (stats) {
    const uint64_t v[16] = { st.files, st.walked, st.left_to_zlib, st.rounds, st.text_bytes, st.launches, st.repeats, (uint64_t)(st.seconds * 1e6),
                             st.candidates, st.streams, st.adopted, st.dropped, st.max_in_flight, st.wasted_text, (uint64_t)(st.scan_seconds * 1e6), 0 };
    std::memcpy(stats, v, n_stats * sizeof(uint64_t));
  }
  return 0;
}

} // namespace

int
gr_gzidx_build_device_many(const grp_engine_ext* ext, void* engine_ctx, const char* const* paths, uint32_t n, uint64_t span, uint64_t max_bytes, gr_gzidx** out, uint64_t stats[8])
{
  return gzidx_build_device(ext, engine_ctx, paths, n, span, max_bytes, gr::GzWalkMembers(), out, stats, 8);
}

int
gr_gzidx_build_device_many_ex(const grp_engine_ext* ext, void* engine_ctx, const char* const* paths, uint32_t n, uint64_t span, uint64_t max_bytes, int members, gr_gzidx** out, uint64_t stats[16])
{
  gr::GzWalkMembers m = gr::gzip_walk_members(); // (the budget: GRP_GZIP_WALK_STREAMS)
  m.on = members != 0;
  return gzidx_build_device(ext, engine_ctx, paths, n, span, max_bytes, m, out, stats, 16);
}

gr_gzidx*
gr_gzidx_build_device(const grp_engine_ext* ext, void* engine_ctx, const char* path, uint64_t span, uint64_t max_bytes)
{
  gr_gzidx* h = nullptr;
  return gr_gzidx_build_device_many(ext, engine_ctx, &path, 1, span, max_bytes, &h, nullptr) == 0 ? h : nullptr;
}

long
gr_gzip_header_bytes(const unsigned char* buf, size_t n)
{
  return gr::gzip_header_bytes(buf, n);
}

int
gr_gzip_walk_switch(void)
{
  return gr::gzip_walk_switch();
}

int
gr_gzip_walk_members_switch(void)
{
  return gr::gzip_walk_members_switch();
}

const char*
gr_gzidx_left(const gr_gzidx* h, uint32_t* status)
{
  if (status) {
    *status = h ? h->left_status : 0;
  }
  return h ? h->left : nullptr;
}

void
gr_gzidx_free(gr_gzidx* h)
{
  delete h;
}

} // extern "C"
