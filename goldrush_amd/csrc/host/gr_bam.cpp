// The C face of gr_bam.hpp (grpath_host.h): the header, the walk and the decoder as the tests and other callers see them.
#include "gr_bam.hpp"
#include "../../../include/grpath_host.h"

extern "C" {

int
gr_bam_header(const unsigned char* buf, uint64_t n, uint64_t* header_bytes)
{
  if (!buf && n) {
    return -1;
  }
  return gr::bam_header(buf, n, header_bytes);
}

int
gr_bam_walk(const unsigned char* buf, uint64_t n, int final_chunk, gr_bam_record* recs, uint64_t cap, uint64_t* n_records, uint64_t* consumed, uint64_t* bad_offset, const char** why)
{
  return gr_bam_walk_ex(buf, n, final_chunk, 0u, recs, cap, n_records, consumed, bad_offset, why, nullptr);
}

int
gr_bam_walk_ex(const unsigned char* buf, uint64_t n, int final_chunk, uint32_t accept, gr_bam_record* recs, uint64_t cap, uint64_t* n_records, uint64_t* consumed, uint64_t* bad_offset, const char** why, uint64_t* skipped)
{
  uint64_t n_rec = 0, used = 0, bad = 0, n_skipped = 0;
  const char* reason = nullptr;
  if (skipped) {
    *skipped = 0;
  }
  if ((!buf && n) || (accept & ~gr::BAM_REFUSED_FLAGS)) {
    return -1;
  }
  const int rc = gr::bam_walk(buf, n, final_chunk != 0, accept, &used, &n_skipped, &bad, &reason, [&](const gr::BamRecord& r) {
    if (recs && n_rec < cap) {
      recs[n_rec] = gr_bam_record{ r.off, r.name_off, r.seq_off, r.qual_off, r.end, r.l_read_name, r.l_seq, r.flag, gr::bam_id_len(buf + r.name_off, r.l_read_name) };
    }
    ++n_rec;
    return true;
  });
  if (n_records) {
    *n_records = n_rec;
  }
  if (consumed) {
    *consumed = used;
  }
  if (bad_offset) {
    *bad_offset = bad;
  }
  if (why) {
    *why = reason;
  }
  if (skipped) {
    *skipped = n_skipped;
  }
  return rc;
}

int
gr_bam_decode(const unsigned char* buf, const gr_bam_record* rec, char* seq_out, char* qual_out)
{
  if (!buf || !rec || !seq_out || !qual_out) {
    return -1;
  }
  gr::bam_decode_bases(buf + rec->seq_off, 0, rec->l_seq, seq_out);
  return gr::bam_decode_quals(buf + rec->qual_off, rec->l_seq, qual_out) ? 0 : -1;
}

int
gr_bam_decode_twin(const unsigned char* buf, const gr_bam_record* rec, uint64_t from, uint64_t n, char* seq_out, char* qual_out)
{
  if (!buf || !rec || !seq_out || !qual_out || from > rec->l_seq || n > rec->l_seq - from) {
    return -1;
  }
  if (rec->flag & gr::BAM_FLAG_REVERSE) {
    gr::bam_decode_bases_rev(buf + rec->seq_off, rec->l_seq, from, n, seq_out);
    return gr::bam_decode_quals_rev(buf + rec->qual_off, rec->l_seq, from, n, qual_out) ? 0 : -1;
  }
  gr::bam_decode_bases(buf + rec->seq_off, from, n, seq_out);
  return gr::bam_decode_quals(buf + rec->qual_off + from, n, qual_out) ? 0 : -1;
}

} // extern "C"
