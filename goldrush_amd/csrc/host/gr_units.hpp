// Random access into a compressed input by DECOMPRESSED offset (gr_path.cpp: the reads of a BGZF / gzip / BAM input kept on
// the device between the passes, whose written records are fetched through their inflatable units).  A file's units are
// the members of a BGZF file (BgzfMap, written down by the pass that walks them to the file's end: BgzfFeed) or the
// segments of a plain gzip file's index (GzIndex::segs); either way unit i holds the text [text_off[i], text_off[i + 1]) of
// the file's decompressed stream.  Header-only and pure (no I/O): tools/dev/units_host_check.cpp drives it under the
// sanitizers.
#pragma once
#include "../../../include/grpath_ingest.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gr {

// The members of one BGZF file: the tables the engine takes (comp_off counts in the FILE: the payload's first byte) and
// the running text offset, n + 1 entries.  32 bytes per member, 0.05 % of the text.
struct BgzfMap
{
  std::vector<grp_bgzf_block> blocks;
  std::vector<uint64_t> text_off{ 0 };
  void add(uint64_t payload_file_off, uint32_t comp_len, uint32_t text_len, uint32_t crc32)
  {
    blocks.push_back(grp_bgzf_block{ payload_file_off, comp_len, text_len, crc32, 0 });
    text_off.push_back(text_off.back() + text_len);
  }
};

// units [first, first + count) cover the text [off, off + len); `inside`: where `off` lies in unit `first`
struct UnitRun
{
  size_t first = 0, count = 0;
  uint64_t inside = 0;
};

// text_off: n + 1 ascending offsets (units without text repeat an offset).  false: the range does not lie inside the
// units' text.  The first unit is the one that HOLDS `off` — an empty unit in front of it begins at the same offset and is
// not taken; empty units between two units of the run are (they hold nothing); a range of no byte takes the unit at `off`.
inline bool
locate_units(const std::vector<uint64_t>& text_off, uint64_t off, uint64_t len, UnitRun& out)
{
  const size_t n = text_off.empty() ? 0 : text_off.size() - 1;
  if (n == 0 || off >= text_off[n] || len > text_off[n] - off) {
    return false;
  }
  const size_t u = (size_t)(std::upper_bound(text_off.begin(), text_off.begin() + (std::ptrdiff_t)n, off) - text_off.begin()) - 1; // the last unit that begins at or in front of `off`
  const uint64_t end = off + std::max<uint64_t>(len, 1);
  const size_t e = (size_t)(std::lower_bound(text_off.begin() + (std::ptrdiff_t)u + 1, text_off.begin() + (std::ptrdiff_t)n, end) - text_off.begin()); // the first unit behind `u` that begins at or behind the end
  out.first = u;
  out.count = e - u;
  out.inside = off - text_off[u];
  return true;
}

// One record to fetch: its text [off, off + len) in the file's decompressed stream
struct FetchItem
{
  uint64_t off, len;
};

// One call of the fetch: the first n_recs of the items, the file's units they need (each once, ascending) and where each
// record begins in the concatenated text of those units
struct FetchPlan
{
  size_t n_recs = 0;
  std::vector<size_t> units;
  std::vector<uint64_t> rec_text_off;
  uint64_t text_bytes = 0;
  size_t straddling = 0; // records that lie in two or more units
};

// Takes items from the front while the units' text stays within text_cap and their number within max_units — always at
// least one item, whatever it needs (the caller has refused files with a unit larger than its buffers) — and while the
// items go forward through the file (an item that begins in front of the last unit taken ends the call: the next one
// takes it).  false: the first item does not lie inside the units' text (nothing is planned).
inline bool
plan_fetch(const std::vector<uint64_t>& text_off, const FetchItem* items, size_t n, uint64_t text_cap, size_t max_units, FetchPlan& pl)
{
  pl.n_recs = 0;
  pl.units.clear();
  pl.rec_text_off.clear();
  pl.text_bytes = 0;
  pl.straddling = 0;
  for (size_t i = 0; i < n; ++i) {
    UnitRun r;
    if (!locate_units(text_off, items[i].off, items[i].len, r)) {
      return i != 0; // (the call ends in front of it; the next plan reports it)
    }
    size_t from = r.first; // the first unit of the run that is not taken yet
    uint64_t at = pl.text_bytes; // where unit r.first begins in the concatenated text
    if (!pl.units.empty()) {
      if (r.first < pl.units.back()) {
        break;
      }
      if (r.first == pl.units.back()) {
        from = r.first + 1;
        at = pl.text_bytes - (text_off[r.first + 1] - text_off[r.first]);
      }
    }
    uint64_t more = 0;
    for (size_t u = from; u < r.first + r.count; ++u) {
      more += text_off[u + 1] - text_off[u];
    }
    if (i != 0 && (pl.text_bytes + more > text_cap || pl.units.size() + (r.first + r.count - from) > max_units)) {
      break;
    }
    for (size_t u = from; u < r.first + r.count; ++u) {
      pl.units.push_back(u);
    }
    pl.text_bytes += more;
    pl.rec_text_off.push_back(at + r.inside);
    pl.straddling += r.count > 1 ? 1 : 0;
    ++pl.n_recs;
  }
  return pl.n_recs != 0;
}

} // namespace gr
