// Stand-alone driver of goldrush_amd/csrc/host/gr_stream_stripes.hpp for tests/test_stream_stripes_cpu.py (built with the
// address and undefined-behaviour sanitizers).  Reads cases from the file named on the command line, one per line:
//   first count stripe_reads n_owners owner  n_x x...  n_reads tiles_of_read...
// and prints per case one line:
//   n_mine n_decidable max_tiles_read | owns(j) for every j | the tile list | decided_base resume_tile for every x
#include "host/gr_stream_stripes.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

int
main(int argc, char** argv)
{
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  size_t n_cases = 0;
  while (std::getline(in, line)) {
    if (line.empty()) {
      continue;
    }
    std::istringstream ls(line);
    gr::stripes::Window w;
    size_t n_x = 0, n_reads = 0;
    ls >> w.first >> w.count >> w.stripe_reads >> w.n_owners >> w.owner >> n_x;
    std::vector<uint32_t> xs(n_x);
    for (uint32_t& x : xs) {
      ls >> x;
    }
    ls >> n_reads;
    // exactly n_reads + 1 entries: a read past the window's reads of the batch is a heap overflow the sanitizer reports
    std::vector<uint64_t> tile0(n_reads + 1, 0);
    for (size_t i = 0; i < n_reads; ++i) {
      uint64_t t = 0;
      ls >> t;
      tile0[i + 1] = tile0[i] + t;
    }
    if (!ls || (size_t)w.first + w.count > n_reads) {
      fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    w.tile0 = tile0.data();
    const gr::stripes::Totals t = gr::stripes::totals(w);
    printf("%llu %u %llu |", (unsigned long long)t.n_mine, t.n_decidable, (unsigned long long)t.max_tiles_read);
    for (uint32_t j = 0; j < w.count; ++j) {
      printf(" %d", w.owns(j) ? 1 : 0);
    }
    printf(" |");
    std::vector<uint32_t> tiles(t.n_mine); // exactly n_mine entries, likewise
    gr::stripes::tile_list(w, tiles.data());
    for (uint32_t v : tiles) {
      printf(" %u", v);
    }
    printf(" |");
    for (uint32_t x : xs) {
      const gr::stripes::Resume r = gr::stripes::resume_at(w, x);
      printf(" %u %llu", r.decided_base, (unsigned long long)r.resume_tile);
    }
    printf("\n");
    ++n_cases;
  }
  printf("stripes done: %zu cases\n", n_cases);
  return 0;
}
