// Plain gzip input: one serial DEFLATE stream per member, with no table of its blocks.  Nothing but a pass through zlib
// finds the block boundaries — and the first pass over the input goes through zlib anyway.  GzIndexReader is that pass: it
// hands out the bytes gzread hands out and, while it inflates with Z_BLOCK, writes down exact restart points in the manner
// of zlib's zran example: a block boundary with its bit position in the file, the up to 32 KiB of text in front of it
// (inflateGetDictionary) and the CRC32 of the text up to the next point.  Every later pass over the same file then has a
// table of independent segments, as a BGZF file has a table of members, and the engine inflates them side by side
// (include/grpath_ingest.h: grp_gzip_inflate).  Nothing is guessed: where this reader is not sure to do what gzread does
// (bytes behind the last member that are no gzip member) it does what gzread does and drops the index.
//
// Points: one behind each member's header (bit 0 of the payload, no history); one at the first block boundary where at
// least `span` bytes of text have come out since the last point; none on the boundary behind a final block — the
// member's end closes the segment there (flag 1).  A segment is never empty: blocks without text behind the last point
// of a member go to the segment in front of them, a member without text has no segment.
#pragma once
#include "../../../include/grpath_ingest.h"

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace gr {

struct GzSegment
{
  uint64_t comp_bit; // first bit of the segment in the FILE (bit 0 = LSB of byte 0)
  uint64_t n_bits;
  uint64_t dict_at;  // GzIndex::dict()
  uint32_t dict_len, text_len, crc32, flags;
  uint64_t first_byte() const { return comp_bit >> 3; }
  uint64_t end_byte() const { return (comp_bit + n_bits + 7) >> 3; }
};

class GzIndex
{
public:
  std::vector<GzSegment> segs;
  uint64_t text_bytes = 0;              // of all segments: the whole input
  uint64_t max_text = 0, max_comp = 0;  // the largest segment's text and compressed bytes (first_byte .. end_byte)
  uint64_t file_size = 0;               // the file the index was built from ...
  int64_t mtime_s = 0, mtime_ns = 0;    // ... and when it was last written
  const uint8_t* dict(const GzSegment& g) const { return store_[g.dict_at / kBlock].get() + g.dict_at % kBlock; }
  uint64_t bytes() const { return segs.size() * sizeof(GzSegment) + (uint64_t)store_.size() * kBlock; }
  bool matches(const std::string& path) const; // the file has that size and time still

private:
  friend class GzIndexReader;
  friend class GzWalker; // gr_gzwalk.hpp: the same index from steps of the engine's decoder
  static constexpr uint64_t kBlock = uint64_t(1) << 20; // histories are kept in blocks of this size, none across two
  std::vector<std::unique_ptr<uint8_t[]>> store_;
  uint64_t used_ = kBlock; // of the last block
  uint8_t* reserve(uint32_t n, uint64_t* at);
};

// GRP_GZIP_INDEX (off: no index), GRP_GZIP_SPAN (bytes of text between two points), GRP_GZIP_INDEX_MAX_GB (default 16)
bool gzip_index_enabled();
uint64_t gzip_index_span();
uint64_t gzip_index_max_bytes();

class GzIndexReader
{
public:
  // span: text between two points (at least 1); max_bytes: the index is dropped when it grows beyond that
  GzIndexReader(const std::string& path, uint64_t span, uint64_t max_bytes);
  ~GzIndexReader();
  GzIndexReader(const GzIndexReader&) = delete;
  GzIndexReader& operator=(const GzIndexReader&) = delete;
  bool ok() const { return fd_ >= 0 && z_ != nullptr; }
  // like InputFile::read of a gzip file: 0 at the end of the data or on an error (noted with note_input_failure)
  size_t read(char* dst, size_t n);
  bool complete() const { return complete_; }  // the end of the file was reached and the index describes all of it
  bool dropped() const { return !indexing_; }  // the cap, or a corner this reader leaves to zlib
  bool failed() const { return failed_; }
  const GzIndex* partial() const { return idx_.get(); } // what there is so far (nullptr once dropped)
  std::unique_ptr<GzIndex> take();             // the complete index; nullptr if there is none

private:
  bool fill();
  void on_boundary();
  void commit(uint64_t end_bit, uint32_t crc_now, uint32_t flags);
  void drop();
  void fail(const std::string& what);
  std::string path_;
  int fd_ = -1;
  void* z_ = nullptr; // z_stream
  std::vector<unsigned char> in_;
  uint64_t in_pos_ = 0; // file offset of the stream's next input byte
  bool file_end_ = false, between_ = false, done_ = false, failed_ = false, complete_ = false, indexing_ = true;
  uint64_t span_, max_bytes_;
  std::unique_ptr<GzIndex> idx_;
  // the member being read: its text so far, the open segment (begun at a point, not closed yet)
  uint64_t member_text_ = 0;
  bool open_ = false;
  GzSegment cur_{};
  uint64_t cur_text0_ = 0, cur_used0_ = 0;
  size_t cur_blocks0_ = 0;
  uint32_t cur_crc0_ = 0;
  size_t member_segs_ = 0;
};

} // namespace gr
