// The classification sinks (gr_writer.hpp).
#include "gr_writer.hpp"
#include "gr_fastq.hpp"
#include "gr_golden.hpp"
#include "gr_params.hpp"

namespace gr {
namespace {

// One committed read, whose text is in `b`, to the output file; returns sum_phred of the qualities it wrote
double
write_record(SinkState& st, const Batch& b, const Rec& r, const grp_read_decision& d)
{
  PathRun& run = *st.run;
  const WrittenSlice w = written_slice(run.opt.tile_length, r.seq_len, r.qual_len, d);
  const size_t n_seq = w.n_seq, n_qual = w.n_qual;
  // the written slice (a BAM batch: it alone is decoded — bases through the code table, qualities + 33)
  const char* seq = b.seq_text(r, w.off, n_seq, st.bam_seq);
  const char* qual = b.qual_text(r, w.qoff, n_qual, st.bam_qual);
  std::ofstream& o = run.out;
  if (st.golden && run.rank == 0) {
    st.golden->note_written(run, (uint64_t)(std::streamoff)o.tellp() + 1, b.text + r.id_off, r.id_len, w.trimmed, n_seq, qual, n_qual);
  }
  o.put(run.opt.silver_path ? '@' : '>');
  o.write(b.text + r.id_off, (std::streamsize)r.id_len);
  o << (w.trimmed ? "_trimmed\n" : "_untrimmed\n");
  if (b.seq_is_upper || b.bam) { // (the code table is upper case)
    o.write(seq, (std::streamsize)n_seq);
  } else {
    // SeqReader folds the case of what the reference later writes
    st.upper.assign(seq, n_seq);
    for (char& ch : st.upper) {
      if (ch >= 'a' && ch <= 'z') {
        ch = (char)(ch - 32);
      }
    }
    o.write(st.upper.data(), (std::streamsize)n_seq);
  }
  o << std::endl;
  if (run.opt.silver_path) {
    o << "+\n";
    o.write(qual, (std::streamsize)n_qual);
    o << std::endl;
  }
  return sum_phred(qual, n_qual);
}

// resident mode, a plain file: one record read back from the file and written
double
write_plain_record(SinkState& st, const RecLoc& l, const grp_read_decision& d)
{
  PathRun& run = *st.run;
  const size_t n = (size_t)l.qual_rel + l.qual_len;
  st.text.resize(n);
  int err = 0;
  if (pread_full(st.res->fd_of(run, l.file), st.text.data(), n, l.off, &err) < n) {
    // not exit(1) from inside the commit callback (a streaming window may be parked on this thread's word,
    // ADVICE r03): the failure is noted, this and the later records are not written, and the program ends with
    // an error behind the pass
    note_input_failure("cannot read the record at byte " + std::to_string(l.off) + " back from " + run.files[l.file]);
    return 0.0;
  }
  Batch fetched;
  fetched.text = st.text.data();
  return write_record(st, fetched, rec_of(l, 0), d);
}

} // namespace

void
Deferred::flush(SinkState& st)
{
  Resident& res = *st.res;
  if (pend.empty()) {
    return;
  }
  ++n_flushes;
  const size_t want = sums.size() + pend.size(); // one sum per record of the list, written or not
  size_t i = 0;
  while (i < pend.size() && !input_failed()) {
    const uint32_t f = pend[i].loc.file;
    size_t e = i + 1;
    while (e < pend.size() && pend[e].loc.file == f) {
      ++e;
    }
    if (res.kind[f] == Resident::PLAIN) {
      for (; i < e && !input_failed(); ++i) {
        sums.push_back(write_plain_record(st, pend[i].loc, pend[i].dec));
      }
    } else {
      while (i < e && fetch_some(st, i, e)) {
      }
      if (i < e) {
        break; // (the failure is noted)
      }
    }
  }
  while (sums.size() < want) { // (an input failure: what was not written counts nothing)
    sums.push_back(0.0);
  }
  pend.clear();
}

// one call of the fetch for records [i, e) of the list, all of one compressed file: as many as its buffers take; i moves
// behind them.  false: a failure was noted.
bool
Deferred::fetch_some(SinkState& st, size_t& i, size_t e)
{
  PathRun& run = *st.run;
  Resident& res = *st.res;
  const uint32_t f = pend[i].loc.file;
  const bool gz = res.kind[f] == Resident::GZIP, bam = res.bam[f] != 0, fastq = run.opt.silver_path;
  const std::vector<uint64_t>& toff = gz ? res.gz_text_off[f] : run.bgzf_map[f]->text_off;
  items.clear();
  for (size_t j = i; j < e; ++j) {
    items.push_back(FetchItem{ pend[j].loc.off, pend[j].loc.qual_rel + pend[j].loc.qual_len });
  }
  if (!plan_fetch(toff, items.data(), items.size(), Resident::kTextCap, kMaxUnits, plan)) {
    note_input_failure("the record at byte " + std::to_string(pend[i].loc.off) + " of the text of " + run.files[f] + " does not lie inside the units the fill pass wrote down");
    return false;
  }
  // the units' compressed bytes (and histories), one after the other
  comp.clear();
  dict.clear();
  blocks.clear();
  segs.clear();
  const int fd = res.fd_of(run, f);
  for (const size_t u : plan.units) {
    uint64_t at, n;
    if (gz) {
      const GzSegment& g = run.gzidx[f]->segs[u];
      at = g.first_byte();
      n = g.end_byte() - at;
      segs.push_back(grp_gzip_segment{ g.comp_bit - at * 8 + (uint64_t)comp.size() * 8, g.n_bits, (uint64_t)dict.size(), g.dict_len, g.text_len, g.crc32, g.flags });
      dict.insert(dict.end(), run.gzidx[f]->dict(g), run.gzidx[f]->dict(g) + g.dict_len);
      dict.resize((dict.size() + 3) & ~size_t(3));
    } else {
      const grp_bgzf_block& b = run.bgzf_map[f]->blocks[u];
      at = b.comp_off;
      n = b.comp_len;
      blocks.push_back(grp_bgzf_block{ (uint64_t)comp.size(), b.comp_len, b.text_len, b.crc32, 0 });
    }
    const size_t have = comp.size();
    comp.resize(have + (size_t)n);
    int err = 0;
    if (pread_full(fd, comp.data() + have, (size_t)n, at, &err) < n) {
      note_input_failure("cannot read the compressed bytes at byte " + std::to_string(at) + " back from " + run.files[f]);
      return false;
    }
  }
  const uint32_t n_units = (uint32_t)plan.units.size();
  const void* units = gz ? static_cast<const void*>(segs.data()) : static_cast<const void*>(blocks.data());
  const auto engine_says = [&](const char* what) {
    note_input_failure(std::string("reading ") + run.files[f] + " failed: " + what + ": " + (run.vt.last_error ? run.vt.last_error(run.ctx) : "the engine refused"));
    return false;
  };
  if (run.ext.records_fetch) {
    recs.clear();
    uint64_t out_n = 0, size = 0;
    for (size_t j = 0; j < plan.n_recs; ++j) {
      const RecLoc& l = pend[i + j].loc;
      recs.push_back(fetch_record_of(l, written_slice(run.opt.tile_length, l.seq_len, l.qual_len, pend[i + j].dec), plan.rec_text_off[j], out_n, fastq, &size));
      out_n += size;
    }
    out.resize((size_t)out_n);
    got_sums.assign(plan.n_recs, 0.0);
    uint32_t bad_unit = UINT32_MAX, bad_rec = UINT32_MAX;
    if (run.ext.records_fetch(run.ctx, gz ? GRP_FETCH_UNITS_GZIP : GRP_FETCH_UNITS_BGZF, comp.data(), comp.size(), dict.data(), dict.size(), units, n_units, recs.data(), (uint32_t)recs.size(),
                              (fastq ? GRP_FETCH_FASTQ : 0u) | (bam ? GRP_FETCH_BAM : 0u), out.data(), out.size(), got_sums.data(), &bad_unit, &bad_rec) != GRP_OK) {
      return engine_says("the written records could not be fetched");
    }
    if (st.golden) {
      // the formatted records are in hand: "@<id>_[un]trimmed\n<bases>\n+\n<qualities>\n"
      const uint64_t at = (uint64_t)(std::streamoff)run.out.tellp();
      for (const grp_fetch_record& fr : recs) {
        const bool trimmed = (fr.flags & GRP_FETCH_REC_TRIMMED) != 0;
        const char* id = out.data() + fr.out_off + 1;
        st.golden->note_written(run, at + fr.out_off + 1, id, fr.id_len, trimmed, fr.n_seq, id + fr.id_len + (trimmed ? 9 : 11) + fr.n_seq + 3, fr.n_qual);
      }
    }
    run.out.write(out.data(), (std::streamsize)out.size());
    sums.insert(sums.end(), got_sums.begin(), got_sums.end());
    n_out_bytes += out.size();
  } else {
    // the host's own fetch: the units' text through the inflate entry points, formatted by write_record
    text.resize((size_t)plan.text_bytes + 8);
    uint32_t bad = UINT32_MAX;
    const int rc = gz ? run.ext.gzip_inflate(run.ctx, comp.data(), comp.size(), dict.data(), dict.size(), segs.data(), n_units, text.data(), plan.text_bytes, &bad)
                      : run.ext.bgzf_inflate(run.ctx, comp.data(), comp.size(), blocks.data(), n_units, text.data(), plan.text_bytes, &bad);
    if (rc != GRP_OK) {
      return engine_says("the units of the written records could not be inflated");
    }
    Batch b;
    b.text = text.data();
    b.bam = bam;
    const std::streampos before = run.out.tellp();
    for (size_t j = 0; j < plan.n_recs; ++j) {
      sums.push_back(write_record(st, b, rec_of(pend[i + j].loc, (size_t)plan.rec_text_off[j]), pend[i + j].dec));
    }
    n_out_bytes += (uint64_t)(run.out.tellp() - before);
  }
  n_units_inflated += n_units;
  n_text_bytes += plan.text_bytes;
  n_records += plan.n_recs;
  n_straddling += plan.straddling;
  for (size_t j = 0; j < plan.n_recs; ++j) {
    n_trimmed += pend[i + j].dec.kind == DEC_INSERT_TRIMMED ? 1 : 0;
  }
  i += plan.n_recs;
  return true;
}

void
Deferred::say_trace(const PathRun& run) const
{
  if (getenv("GRP_TRACE_INGEST") && run.rank == 0) {
    std::cerr << "GRP_TRACE_INGEST resident fetch: " << n_flushes << " flushes, units inflated " << n_units_inflated << ", text bytes inflated " << n_text_bytes << ", records fetched " << n_records << " (trimmed " << n_trimmed
              << ", in two or more units " << n_straddling << "), output bytes " << n_out_bytes << (run.ext.records_fetch ? " (formatted on the device)" : " (inflated through the engine, formatted on the host)") << std::endl;
  }
}

// the classifier's settle hook: the sums of the n insert commits since the last call, in commit order
void
settle_sink(void* user, double* out_sums, uint32_t n)
{
  SinkState& st = *static_cast<SinkState*>(user);
  Deferred& d = *st.deferred;
  d.flush(st);
  for (uint32_t k = 0; k < n && !d.sums.empty(); ++k) {
    out_sums[k] = d.sums.front();
    d.sums.pop_front();
  }
}

// writes one committed read (goldrush_path.cpp:996-1002, 1055-1070)
double
commit_sink(void* user, const gr_commit* c)
{
  SinkState& st = *static_cast<SinkState*>(user);
  if ((c->dec.kind != DEC_INSERT_WHOLE && c->dec.kind != DEC_INSERT_TRIMMED) || input_failed()) {
    return 0.0;
  }
  if (st.golden && st.run->rank == 0) {
    st.golden->note_commit(*st.run, c->read, st.resident ? st.resident->loc[c->read].seq_len : (uint32_t)st.batch->rec[(*st.sel)[c->read]].seq_len, c->dec);
  }
  if (st.resident && st.deferred) {
    // (ranks other than 0 write nothing and print nothing: nothing to fetch)
    if (st.run->rank == 0) {
      st.deferred->pend.push_back(Deferred::Pending{ st.resident->loc[c->read], c->dec });
    }
    return 0.0; // (the sum comes through the settle hook)
  }
  if (st.resident) {
    return write_plain_record(st, st.resident->loc[c->read], c->dec);
  }
  const Batch& b = *st.batch;
  return write_record(st, b, b.rec[(*st.sel)[c->read]], c->dec);
}

void
rollover_sink(void* user, uint64_t new_path)
{
  // golden_path_vec.pop_back(); emplace_back(ofstream(prefix + "_" + path + ".fq"))  (:182-184)
  SinkState& st = *static_cast<SinkState*>(user);
  PathRun& run = *st.run;
  if (st.deferred) {
    st.deferred->flush(st); // (the settle hook has run in front of this callback: nothing is left — the records of a path go to its file)
  }
  run.out.close();
  run.out.open(run.rank == 0 ? run.opt.prefix_file + "_" + std::to_string(new_path) + ".fq" : std::string("/dev/null"));
  if (run.rank == 0) {
    run.out_files.push_back(run.opt.prefix_file + "_" + std::to_string(new_path) + ".fq");
  }
}

void
debug_skipped(const SinkState& st, size_t from, size_t to)
{
  const Batch& b = *st.batch;
  for (size_t i = from; i < to; ++i) {
    const auto& sk = (*st.skipped)[i];
    std::cerr << (sk.second == 1 ? "too short" : "hairpin or quality too low or invalid bases") << std::endl;
    std::cerr << "skipping: " << b.id_str(sk.first) << std::endl;
  }
}

// --debug: in front of a classified read (:907-941)
void
debug_sink(void* user, uint32_t read)
{
  SinkState& st = *static_cast<SinkState*>(user);
  const size_t n = (*st.skipped_before)[read];
  debug_skipped(st, st.skipped_done, st.skipped_done + n);
  st.skipped_done += n;
  const Batch& b = *st.batch;
  const uint32_t i = (*st.sel)[read];
  std::cerr << "name: " << b.id_str(i) << std::endl;
  std::cerr << "num tiles: " << b.rec[i].seq_len / st.run->opt.tile_length << std::endl;
}

} // namespace gr
