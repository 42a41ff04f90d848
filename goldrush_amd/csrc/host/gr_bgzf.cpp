#include "gr_bgzf.hpp"

#include "../../../include/grpath_host.h"

namespace gr {

namespace {
inline unsigned
le16(const unsigned char* p)
{
  return (unsigned)p[0] | (unsigned)p[1] << 8;
}
inline uint32_t
le32(const unsigned char* p)
{
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
} // namespace

size_t
bgzf_scan(const unsigned char* buf, size_t n, grp_bgzf_block* blocks, size_t cap, size_t* consumed, int* why)
{
  // ID1 ID2 CM FLG: a BGZF member has FEXTRA and nothing else (the payload then starts right behind the extra field)
  static const unsigned char magic[4] = { 0x1f, 0x8b, 8, 4 };
  size_t pos = 0, nb = 0;
  int w = 1;
  while (nb < cap && pos < n) {
    const unsigned char* m = buf + pos;
    const size_t left = n - pos;
    bool other = false;
    for (size_t i = 0; i < 4 && i < left; ++i) {
      other |= m[i] != magic[i];
    }
    if (other) {
      w = 2;
      break;
    }
    if (left < 12) {
      w = 0;
      break;
    }
    const size_t xlen = le16(m + 10);
    if (left < 12 + xlen) {
      w = 0;
      break;
    }
    // the subfields: SI1 SI2 SLEN data
    size_t bsize = 0;
    bool found = false;
    for (size_t at = 12; at + 4 <= 12 + xlen;) {
      const size_t slen = le16(m + at + 2);
      if (m[at] == 'B' && m[at + 1] == 'C' && slen == 2 && at + 6 <= 12 + xlen) {
        bsize = le16(m + at + 4);
        found = true;
        break;
      }
      at += 4 + slen;
    }
    if (!found || bsize + 1 < 12 + xlen + 8) {
      w = 2;
      break;
    }
    if (left < bsize + 1) {
      w = 0;
      break;
    }
    const uint32_t isize = le32(m + bsize + 1 - 4);
    if (isize > BGZF_MAX_TEXT) {
      w = 2;
      break;
    }
    grp_bgzf_block& b = blocks[nb++];
    b.comp_off = pos + 12 + xlen;
    b.comp_len = (uint32_t)(bsize + 1 - 12 - xlen - 8);
    b.text_len = isize;
    b.crc32 = le32(m + bsize + 1 - 8);
    b.reserved = 0;
    pos += bsize + 1;
  }
  if (consumed) {
    *consumed = pos;
  }
  if (why) {
    *why = w;
  }
  return nb;
}

} // namespace gr

extern "C" size_t
gr_bgzf_scan(const unsigned char* buf, size_t n, grp_bgzf_block* blocks, size_t cap, size_t* consumed, int* why)
{
  return gr::bgzf_scan(buf, n, blocks, cap, consumed, why);
}
