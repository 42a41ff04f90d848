// BGZF: the gzip members bgzip and the htslib tools write — at most 64 KiB of text each, independent of each other, and
// each says its compressed size in an extra subfield of its header ('B','C', SLEN = 2, BSIZE = member size - 1), so the
// members of a chunk can be found without inflating them and inflated side by side (include/grpath_ingest.h:
// grp_bgzf_inflate).  This is the walk over the headers; pure, no I/O.
#pragma once
#include "../../../include/grpath_ingest.h"

#include <cstddef>

namespace gr {

constexpr size_t BGZF_MAX_MEMBER = 65536; // BSIZE is 16 bits wide
constexpr size_t BGZF_MAX_TEXT = 65536;

// gr_bgzf_scan of grpath_host.h
size_t bgzf_scan(const unsigned char* buf, size_t n, grp_bgzf_block* blocks, size_t cap, size_t* consumed, int* why);

} // namespace gr
