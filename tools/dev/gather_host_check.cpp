// Stand-alone check of the word function of grp_reads_gather (csrc/host/gr_gather_word.hpp) for the sanitizers.  It is
// driven exactly as k_reads_gather drives it — src at the source read's word that holds the slice's first base, one call
// per output word, the output in a block of exactly the slice's words — with every source read in a heap block of exactly
// its words, so that a load behind a read's last word or a store behind a slice's is seen.  Every slice is compared with
// the packing of the sliced string.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dev/gather_host_check.cpp -o /tmp/gather_host_check && /tmp/gather_host_check
#include "../../goldrush_amd/csrc/host/gr_gather_word.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

// 2 bits per base as grp_reads_upload expects them, in a block of exactly ceil(n / 16) words
static std::unique_ptr<uint32_t[]>
pack(const std::vector<uint8_t>& codes, size_t first, size_t n)
{
  const size_t nw = (n + 15) / 16;
  std::unique_ptr<uint32_t[]> w(new uint32_t[nw]());
  for (size_t j = 0; j < n; ++j) {
    w[j / 16] |= (uint32_t)codes[first + j] << (2 * (j % 16));
  }
  return w;
}

static unsigned long n_slices = 0;

static void
check(const std::vector<uint8_t>& codes, const uint32_t* read_words, uint32_t first, uint32_t n)
{
  const uint32_t nw = gr::gather_words(n);
  if (nw != (n + 15) / 16) {
    fprintf(stderr, "gather_words(%u) = %u\n", n, nw);
    exit(1);
  }
  std::unique_ptr<uint32_t[]> out(new uint32_t[nw]);
  const uint32_t* src = read_words + (first >> 4);
  for (uint32_t j = 0; j < nw; ++j) {
    out[j] = gr::gather_out_word(src, first & 15u, n, j);
  }
  const std::unique_ptr<uint32_t[]> want = pack(codes, first, n);
  for (uint32_t j = 0; j < nw; ++j) {
    if (out[j] != want[j]) {
      fprintf(stderr, "read of %zu bases, slice [%u, %u): word %u is %08x, expected %08x\n", codes.size(), first, first + n, j, out[j], want[j]);
      exit(1);
    }
  }
  ++n_slices;
}

int
main()
{
  std::mt19937_64 rng(7);
  std::vector<uint32_t> lens;
  for (uint32_t l = 1; l <= 100; ++l) {
    lens.push_back(l);
  }
  for (uint32_t l : { 255u, 256u, 257u, 4095u, 4096u, 4097u, 4111u, 9001u }) {
    lens.push_back(l);
  }
  for (const uint32_t len : lens) {
    std::vector<uint8_t> codes(len);
    for (uint8_t& c : codes) {
      c = (uint8_t)(rng() & 3);
    }
    const std::unique_ptr<uint32_t[]> words = pack(codes, 0, len);
    if (len <= 100) { // every slice of a short read
      for (uint32_t first = 0; first < len; ++first) {
        for (uint32_t n = 1; first + n <= len; ++n) {
          check(codes, words.get(), first, n);
        }
      }
      continue;
    }
    // a long read: every shift against every length residue, at its front and ending exactly at its end; whole; single bases
    for (uint32_t shift = 0; shift < 16; ++shift) {
      for (uint32_t res = 0; res < 16; ++res) {
        const uint32_t n = 48 + res;
        check(codes, words.get(), 32 + shift, n);
        check(codes, words.get(), 32 + shift, len - (32 + shift) - res);
        if (len - n >= 16) {
          const uint32_t first = ((len - n) & ~15u) - 16 + shift; // ... and one that ends short of the end
          check(codes, words.get(), first, n);
          check(codes, words.get(), len - n, n);
        }
      }
      check(codes, words.get(), len - 1 - shift, 1);
      check(codes, words.get(), shift, 1);
    }
    check(codes, words.get(), 0, len);
    for (int k = 0; k < 2000; ++k) {
      const uint32_t first = (uint32_t)(rng() % len);
      check(codes, words.get(), first, 1 + (uint32_t)(rng() % (len - first)));
    }
  }
  printf("gather_host_check: %lu slices of %zu reads agree with the packing of the sliced string\n", n_slices, lens.size());
  return 0;
}
