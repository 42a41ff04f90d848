// Random access into a compressed input by DECOMPRESSED offset (gr_writer.cpp: the reads of a BGZF / gzip / BAM input kept on
// the device between the passes, whose written records are fetched through their inflatable units).  A file's units are
// the members of a BGZF file (BgzfMap, written down by the pass that walks them to the file's end: BgzfFeed) or the
// segments of a plain gzip file's index (GzIndex::segs); either way unit i holds the text [text_off[i], text_off[i + 1]) of
// the file's decompressed stream.  Below them: what is written of a stored record, and its entry in a fetch call.
// Header-only and pure (no I/O): tools/dev/units_host_check.cpp drives it under the sanitizers.
#pragma once
#include "../../../include/grpath_ingest.h"
#include "gr_tiles.hpp"

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

// ---- from a stored record to what is written of it ----------------------------------------------------------------------
// A read kept on the device (gr_resident.hpp), as the fill pass wrote it down: where its record lies in its file's text
struct RecLoc
{
  uint32_t file;    // which of the run's files
  uint64_t off;     // offset of the record's id in that file
  uint32_t id_len;
  uint32_t seq_rel; // seq / qual relative to `off`
  uint32_t seq_len;
  uint64_t qual_rel;
  uint32_t qual_len;
  uint8_t reversed; // a reverse-strand record of an aligned BAM file: written backwards (seq_rel / qual_rel: the stored bytes)
};

// The slice of a committed read that is written (goldrush_path.cpp:996-1002, 1055-1070): bases [off, off + n_seq), qualities
// [qoff, qoff + n_qual); a read inserted whole is written whole
struct WrittenSlice
{
  size_t off, n_seq, qoff, n_qual;
  bool trimmed;
};

inline WrittenSlice
written_slice(size_t tile, size_t seq_len, size_t qual_len, const grp_read_decision& d)
{
  WrittenSlice w{ 0, seq_len, 0, qual_len, d.kind == DEC_INSERT_TRIMMED };
  if (w.trimmed) {
    w.off = (size_t)d.trim_start * tile;
    const size_t end_pos = (d.trim_end == d.num_tiles - 1) ? SIZE_MAX : (size_t)(d.trim_end - d.trim_start + 1) * tile;
    w.n_seq = std::min(end_pos, seq_len - w.off);
    w.n_qual = (w.off <= qual_len) ? std::min(end_pos, qual_len - w.off) : 0;
  }
  w.qoff = std::min(w.off, qual_len);
  return w;
}

// The entry of grp_records_fetch (grpath_ingest.h) for a record whose id lies at `text_off` of the fetched text and whose
// bytes go to out_off; *size: how many those are.  A reversed record: the written slice counts in the twin's coordinates,
// the fetch takes the stored range and writes it backwards.
inline grp_fetch_record
fetch_record_of(const RecLoc& l, const WrittenSlice& w, uint64_t text_off, uint64_t out_off, bool fastq, uint64_t* size)
{
  const size_t seq_from = l.reversed ? l.seq_len - w.off - w.n_seq : w.off, qual_from = l.reversed ? l.qual_len - w.qoff - w.n_qual : w.qoff;
  *size = 1 + (uint64_t)l.id_len + (w.trimmed ? 9 : 11) + w.n_seq + 1 + (fastq ? 3 + (uint64_t)w.n_qual : 0);
  return grp_fetch_record{ text_off, text_off + l.seq_rel, text_off + l.qual_rel, out_off, l.id_len, (uint32_t)seq_from, (uint32_t)w.n_seq, (uint32_t)qual_from, (uint32_t)w.n_qual,
                           (w.trimmed ? GRP_FETCH_REC_TRIMMED : 0u) | (l.reversed ? GRP_FETCH_REC_REVERSED : 0u) };
}

} // namespace gr
