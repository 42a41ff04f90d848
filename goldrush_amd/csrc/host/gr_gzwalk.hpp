// Plain gzip input, many files: the restart points of gr_gzidx.hpp found without zlib's serial first pass.  One stream is
// serial, but across files nothing has to be guessed: every file's first member starts at a known bit behind its header,
// with no history, and where a block ends is known the moment a decoder gets there.  gzip_walk walks all the files side
// by side in rounds: per round and file one step of the engine's open decoder form (include/grpath_ingest.h:
// grp_gzip_walk) from the boundary the round before reached, all steps of a round in one launch.  The host parses the
// gzip headers (FEXTRA, FNAME, FCOMMENT, FHCRC), checks the trailers (the CRC32 combined from the rounds' CRCs, ISIZE
// modulo 2^32) and writes down the index GzIndexReader writes, under its rule, word for word:
//   a point behind each member's header (no history); a point at the first block boundary with at least `span` bytes of
//   text since the last point; none behind a final block: the member's end closes the segment (flag 1); a round without
//   text that ends a member goes to the segment in front of it; a member without text has no segment.
// The text is decoded to find the boundaries and thrown away: a pass that then reads the file inflates it a second time,
// through its segments.  The parallelism is the number of files: a single file gains nothing over zlib.
//
// A file is left to zlib (it gets no index, its reader does and says what it does without the walk) when its bytes behind
// the last member are no member, a header is not what zlib takes, a trailer does not match, the stream ends inside a
// block at the end of the file, the decoder refuses it, the index grows beyond max_bytes, or one block needs more room or
// more compressed bytes than the cap: a step that runs out of either is repeated with both doubled up to there.
//
// The steps go through a callback, so that the same rounds run over the engine (gr_source.cpp, gr_capi.cpp) and over the
// decoder compiled for the host (tools/dev/inflate_host_check.cpp --walk).
#pragma once
#include "gr_gzidx.hpp"

#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace gr {

// GRP_GZIP_WALK: 1 on, 0 off or unset, -1 any other value
int gzip_walk_switch();

// GRP_GZIP_WALK_ROOM=room[,window[,cap]] (bytes): the text a step may produce and the compressed bytes it is given at first,
// and how far both may be doubled.  A step is asked for half its first room of text (or what is left of the span)
struct GzWalkSizes
{
  uint64_t room = uint64_t(1) << 20, window = uint64_t(512) << 10, cap = uint64_t(256) << 20;
};
GzWalkSizes gzip_walk_sizes();

// one launch: results[i] and hist_out[32768 i, +hist_len) for every step; false: the launch itself failed (nothing is walked)
using GzWalkLaunch = std::function<bool(const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n_steps, grp_gzip_walk_result* results, uint8_t* hist_out)>;
// the window buffer is about to be read by launches / about to go away (page-locking); either may be empty
using GzWalkBuffer = std::function<void(uint8_t* buf, size_t n)>;

struct GzWalkStats
{
  uint64_t files = 0, walked = 0, left_to_zlib = 0, rounds = 0, text_bytes = 0, launches = 0, repeats = 0;
  double seconds = 0.0;
};

// why a file was left to zlib (tests); nullptr for a file that was walked
struct GzWalkFile
{
  std::unique_ptr<GzIndex> index; // complete, or none
  const char* left = nullptr;
  uint32_t status = 0; // ... the decoder's status, where that was the reason
  bool unreadable = false; // ... it is no regular file that can be looked at: nothing of it was read
};

std::vector<GzWalkFile> gzip_walk(const std::vector<std::string>& paths, uint64_t span, uint64_t max_bytes, const GzWalkSizes& sizes, const GzWalkLaunch& launch, GzWalkStats* stats = nullptr, const GzWalkBuffer& pin = nullptr,
                                  const GzWalkBuffer& unpin = nullptr);

// The gzip header at buf[0, n): its length; 0: more bytes are needed (n < the header's end); -1: not a header zlib takes.
long gzip_header_bytes(const uint8_t* buf, size_t n);

} // namespace gr
