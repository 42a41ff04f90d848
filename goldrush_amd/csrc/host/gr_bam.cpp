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
  uint64_t n_rec = 0, used = 0, bad = 0;
  const char* reason = nullptr;
  if (!buf && n) {
    return -1;
  }
  const int rc = gr::bam_walk(buf, n, final_chunk != 0, &used, &bad, &reason, [&](const gr::BamRecord& r) {
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

} // extern "C"
