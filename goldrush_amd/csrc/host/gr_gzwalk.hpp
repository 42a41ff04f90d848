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
// through its segments.  The parallelism is the number of files: a single-member file gains nothing over zlib.
//
// The members of one file (GzWalkMembers, GRP_GZIP_WALK_MEMBERS=on): `cat a.gz b.gz ... > reads.gz` is one file of many
// members, and a member depends on nothing in front of it: it starts on a byte, behind a header, with no history, and the
// index rule starts anew there.  With the switch on, every byte behind byte 0 where `1f 8b 08` stands with no reserved flag
// bit is a candidate (one sequential read of the file), and a stream is begun at a candidate whose header parses: it walks
// ONE member, in the same rounds and launches as every other step, keeps its segments to itself, checks the trailer, notes
// where the member ended and stops.  Per file the serial logic stays the authority (the chain): it starts at byte 0, and
// when it arrives behind a trailer at byte p it adopts the stream that was begun at p, if there is one — its segments go
// into the file's index in order, its end is the next arrival, an unfinished one goes on as the chain's head, a failure
// it noted is the file's.  Nothing guessed enters the index: a stream's segments are taken only if the chain of members
// from byte 0 arrives at exactly its first byte, and then the serial walk would have begun there too, with the same empty
// state and the same decoder — the same index by construction, not by a checksum.  A stream the chain never arrives at (a
// `1f 8b 08` inside a header field, inside stored text, in a trailer) is dropped, the moment the chain has passed its
// first byte: guessing costs work, never correctness.  Where the chain arrives at a byte without a stream it does what it
// does without the switch, so every file that is left to zlib is left for the same reason in the same words.
//
// A file is left to zlib (it gets no index, its reader does and says what it does without the walk) when its bytes behind
// the last member are no member, a header is not what zlib takes, a trailer does not match, the stream ends inside a
// block at the end of the file, the decoder refuses it, the index grows beyond max_bytes, or one block needs more room or
// more compressed bytes than the cap: a step that runs out of either is repeated with both doubled up to there.
//
// The steps go through a callback, so that the same rounds run over the engine (gr_source.cpp, gr_capi.cpp) and over the
// decoder compiled for the host (tools/dev/inflate_host_check.cpp --walk, --members).
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

// GRP_GZIP_WALK_MEMBERS: 1 on, 0 off or unset, -1 any other value.  It has no effect without GRP_GZIP_WALK=on
int gzip_walk_members_switch();

// The members of a file side by side (above).  `streams`, GRP_GZIP_WALK_STREAMS: the most streams that take steps at the
// same time, over all files.  Every file's chain head is one of them whatever the number (they are the walk without the
// switch), streams ahead of a chain are begun only while there are fewer: in file order, then offset order.  1024 is a
// bound on memory, not a measured optimum: a stream holds a window (512 KiB) and two histories (32 KiB each) on the host,
// about 0.6 GB for 1024, and its room (1 MiB) on the device.
struct GzWalkMembers
{
  bool on = false;
  uint64_t streams = 1024;
};
GzWalkMembers gzip_walk_members(); // from the two variables (a bad value of the switch reads as off here: the caller has refused it)

struct GzWalkStats
{
  uint64_t files = 0, walked = 0, left_to_zlib = 0, rounds = 0, text_bytes = 0, launches = 0, repeats = 0;
  double seconds = 0.0;
  // GzWalkMembers::on: candidates found, streams begun ahead of a chain, of them adopted by one and dropped, the most streams
  // that took a step in one round (heads included), the text dropped streams had decoded.  text_bytes is text that
  // entered an index or was decoded by a chain's head
  uint64_t candidates = 0, streams = 0, adopted = 0, dropped = 0, max_in_flight = 0, wasted_text = 0;
  double scan_seconds = 0.0;
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
                                  const GzWalkBuffer& unpin = nullptr, const GzWalkMembers& members = GzWalkMembers());

// The gzip header at buf[0, n): its length; 0: more bytes are needed (n < the header's end); -1: not a header zlib takes.
long gzip_header_bytes(const uint8_t* buf, size_t n);

} // namespace gr
