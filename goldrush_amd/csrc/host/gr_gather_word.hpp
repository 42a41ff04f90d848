// One output word of a slice cut out of a packed read (grp_reads_gather, csrc/grp_gather.inc): 16 bases per 32-bit word,
// base j at bits 2j, the unused bits of a read's last word zero (grp_reads_upload's layout).  Compiled for the device by
// the engine and for the host by tools/dev/gather_host_check.cpp, which drives it through the kernel's load pattern with
// every source read in a heap block of exactly its words.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GR_GATHER_HD __host__ __device__
#else
#define GR_GATHER_HD
#endif

namespace gr {

// words of n bases
GR_GATHER_HD inline uint32_t
gather_words(uint32_t n_bases)
{
  return n_bases / 16u + ((n_bases & 15u) != 0u);
}

// Output word j of the slice of n_bases bases that begins `shift` (0..15) bases into src[0] — src points at the source
// read's word that holds the slice's first base.  The word is the funnel shift of src[j] and src[j + 1] by 2 * shift
// bits, cut to the bases the slice still has.  src[j] always holds a base of the slice (j < gather_words(n_bases)).
// src[j + 1] is loaded only where the output word takes a base from it — that base is a base of the slice and so of the
// read: no load leaves the source read's own words, whatever lies behind them.
GR_GATHER_HD inline uint32_t
gather_out_word(const uint32_t* src, uint32_t shift, uint32_t n_bases, uint32_t j)
{
  const uint32_t left = n_bases - 16u * j;      // bases of the slice from this word on (>= 1)
  const uint32_t cnt = left < 16u ? left : 16u; // ... that this word holds
  const uint32_t lo = src[j];
  uint32_t v = lo;
  if (shift) {
    const uint32_t hi = cnt > 16u - shift ? src[j + 1] : 0u;
    v = (lo >> (2u * shift)) | (hi << (32u - 2u * shift));
  }
  return cnt < 16u ? v & ((1u << (2u * cnt)) - 1u) : v;
}

} // namespace gr
