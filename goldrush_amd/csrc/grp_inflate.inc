// BGZF members inflated on the device (include/grpath_ingest.h: grp_bgzf_inflate).  A BGZF file is a series of
// independent gzip members of at most 64 KiB of text; each one is a complete RFC 1951 stream, so the members of a
// chunk are inflated side by side: ONE WAVE PER MEMBER, one wave per workgroup.
//
// A DEFLATE stream is serial, so the decode state (bit buffer, table look-ups, the symbol) is the same in all 64 lanes
// — every lane executes the decoder redundantly, nothing diverges — and the lanes share the work that has a width:
// building the Huffman tables, the match copies (out[p + j] = out[p - dist + j % dist]), the copies of stored blocks,
// fetching the compressed bytes and flushing the text.  Everything the lanes hand to each other goes through LDS:
//   ring      the last 32 KiB of text (the longest DEFLATE distance); flushed to HBM 16 KiB at a time as aligned dwords
//   inw       1 KiB window of the compressed bytes, filled 512 B at a time from registers loaded one step ahead
//   tables    a 10-bit (literal/length) and an 8-bit (distance) direct table, codes longer than that through the
//             canonical counts; 37.8 KiB per workgroup in all: 4 workgroups (waves) per CU of 160 KiB — the decoder
//             is bound by the latency of its dependent LDS look-ups, a wave per SIMD keeps the CU's LDS pipe in use
// The lanes of ONE wave execute LDS operations in order, so a wavefront-scope fence (no instruction: it only keeps the
// compiler from moving accesses across it) is all that stands between a lane's store and another lane's load.
//
// The decoder trusts nothing: every read of the compressed bytes is bounded by the member's payload (INF_Reader: words
// outside it read as zero, and no more bits can be consumed than the payload has), every store by the member's
// text_len, a distance may not reach in front of the member's first byte, every loop consumes input or produces output
// in each iteration, no wave waits for another.  A member that is not a valid stream of exactly text_len bytes ends
// with a status word; k_inflate_crc then compares the CRC32 of every good member's text.
//
// The decoder is written against four macros so that the same text compiles as plain C++ with the 64 lanes run one
// after the other (GRP_INFLATE_HOST: tools/dev/inflate_host_check.cpp checks the decoder against zlib under the sanitizers,
// without a device).
#ifndef GRP_INFLATE_HOST
#define INF_FN __device__ __forceinline__
#define INF_LANES for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define INF_LV(x) x
#define INF_LV_DECL(type, x) type x = 0
#define INF_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#else
#define INF_FN inline
#define INF_LANES for (int lane = 0; lane < 64; ++lane)
#define INF_LV(x) x[lane]
#define INF_LV_DECL(type, x) type x[64] = {}
#define INF_FENCE() (void)0
#endif

namespace {

enum InfStatus : uint32_t
{
  INF_OK = 0,
  INF_BAD_BLOCK_TYPE = 1,
  INF_STORED_LEN = 2,
  INF_INPUT_ENDS = 3,
  INF_TEXT_TOO_LONG = 4,
  INF_DIST_TOO_FAR = 5,
  INF_TOO_MANY_SYMBOLS = 6,
  INF_BAD_CODE_LENGTHS = 7,
  INF_BAD_REPEAT = 8,
  INF_NO_END_OF_BLOCK = 9,
  INF_BAD_LITLEN_SET = 10,
  INF_BAD_DIST_SET = 11,
  INF_BAD_LITLEN_CODE = 12,
  INF_BAD_DIST_CODE = 13,
  INF_TEXT_TOO_SHORT = 14,
  INF_BYTES_BEHIND_END = 15,
  INF_CRC_MISMATCH = 16,
  INF_FINAL_INSIDE = 17, // (segments only)
  INF_NO_FINAL = 18,
  INF_STATUS_COUNT = 19,
};
// the open form's own (grp_gzip_walk): it is no word on the stream, so it stands outside the table of a stream's faults
constexpr uint32_t INF_NO_ROOM = 19;
constexpr const char* INF_NO_ROOM_TEXT = "the text of the step's blocks does not fit its room";

const char* const INF_STATUS_TEXT[INF_STATUS_COUNT] = {
  "ok",
  "invalid block type",
  "invalid stored block lengths",
  "the compressed data ends inside the stream",
  "the stream holds more text than the member's ISIZE",
  "invalid distance too far back",
  "too many length or distance symbols",
  "invalid code lengths set",
  "invalid bit length repeat",
  "invalid code -- missing end-of-block",
  "invalid literal/lengths set",
  "invalid distances set",
  "invalid literal/length code",
  "invalid distance code",
  "the stream holds less text than the member's ISIZE",
  "compressed bytes behind the end of the stream",
  "CRC32 of the text differs from the member's",
  "a final block inside a segment that does not end its member",
  "the segment ends its member, its bits end in front of a final block",
};

constexpr uint32_t INF_RING = 32768, INF_RMASK = INF_RING - 1;
constexpr uint32_t INF_FLUSH = 16384;  // text is flushed once this much is waiting
constexpr uint32_t INF_PIECE = 8192;   // a stored block is copied in pieces of this size
constexpr int INF_LBITS = 10, INF_DBITS = 8, INF_CBITS = 7;
constexpr uint32_t INF_MAX_TEXT = 65536; // ISIZE of a BGZF member

struct InfLds
{
  uint8_t ring[INF_RING];
  uint32_t inw[256];
  uint16_t lit_fast[1 << INF_LBITS];
  uint16_t dist_fast[1 << INF_DBITS];
  uint16_t cl_fast[1 << INF_CBITS];
  uint16_t lit_sorted[288];
  uint16_t dist_sorted[32];
  uint16_t cl_sorted[32];
  uint16_t lit_count[16], dist_count[16], cl_count[16];
  uint16_t first[16], offs[16]; // of the table being built
  uint8_t lens[320 + 32];       // literal/length lengths, then the distance lengths; [320, 339): code length code
};

// one Huffman code: a direct table of `bits` bits ((symbol << 4) | length, 0: longer than that or no code), the symbols
// sorted by (length, symbol) and the number of codes of every length
struct InfHuff
{
  uint16_t* fast;
  uint16_t* sorted;
  uint16_t* count;
  int bits;
};

// Builds `h` from n code lengths.  0, or 1: over-subscribed, or incomplete other than zlib accepts (no code at all; one
// code of length 1 where `single_ok`).
INF_FN int
inf_build(InfLds& s, const InfHuff& h, const uint8_t* lens, int n, bool single_ok)
{
  INF_FENCE();
  INF_LANES
  {
    if (lane < 16) { // lane L counts the codes of length L
      uint32_t c = 0;
      for (int i = 0; i < n; ++i) {
        c += lens[i] == lane;
      }
      h.count[lane] = (uint16_t)(lane == 0 ? 0 : c);
    }
    for (int i = lane; i < (1 << h.bits); i += 64) {
      h.fast[i] = 0;
    }
  }
  INF_FENCE();
  int left = 1, max_len = 0;
  uint32_t code = 0, off = 0;
  for (int l = 1; l <= 15; ++l) {
    const uint32_t c = h.count[l];
    left = (left << 1) - (int)c;
    if (left < 0) {
      return 1;
    }
    if (c) {
      max_len = l;
    }
    s.first[l] = (uint16_t)code;
    s.offs[l] = (uint16_t)off;
    code = (code + c) << 1;
    off += c;
  }
  if (left > 0 && max_len != 0 && !(single_ok && max_len == 1)) {
    return 1;
  }
  const int total = (int)off;
  INF_FENCE();
  INF_LANES
  {
    if (lane >= 1 && lane < 16) { // lane L writes the symbols of length L in ascending order
      uint32_t at = s.offs[lane];
      for (int i = 0; i < n; ++i) {
        if (lens[i] == lane) {
          h.sorted[at++] = (uint16_t)i;
        }
      }
    }
  }
  INF_FENCE();
  INF_LANES
  {
    for (int i = lane; i < total; i += 64) {
      const uint32_t sym = h.sorted[i];
      const int l = lens[sym];
      if (l <= h.bits) {
        uint32_t c = (uint32_t)s.first[l] + (uint32_t)(i - (int)s.offs[l]), r = 0;
        for (int b = 0; b < l; ++b) { // DEFLATE sends a code's first bit first: the table is indexed by the bits as they arrive
          r |= ((c >> b) & 1u) << (l - 1 - b);
        }
        for (uint32_t k = r; k < (1u << h.bits); k += 1u << l) {
          h.fast[k] = (uint16_t)((sym << 4) | (uint32_t)l);
        }
      }
    }
  }
  INF_FENCE();
  return 0;
}

// the compressed bytes of one member as a bit stream, least significant bit first
struct InfReader
{
  const uint32_t* words; // the call's compressed bytes (4-byte aligned)
  uint32_t lo, hi;       // the words that hold bytes of this member's payload: [lo, hi)
  uint32_t di;           // the next word that goes into the bit buffer
  uint32_t loaded_end;   // words [di, loaded_end) are in the LDS window
  uint64_t bb;
  int nb;                // bits in bb (bits of words outside the payload are zero)
  int64_t avail;         // bits of the payload not consumed yet
  bool failed;           // more bits were asked for than the payload has
};

#define INF_READER_LV INF_LV_DECL(uint32_t, in_r0); INF_LV_DECL(uint32_t, in_r1)

// the registers take words [loaded_end, loaded_end + 128): used one step later, so the load's latency is not waited for
#define INF_ISSUE(rd)                                                                                                  \
  INF_LANES                                                                                                            \
  {                                                                                                                    \
    const uint32_t d0_ = (rd).loaded_end + (uint32_t)lane, d1_ = d0_ + 64;                                             \
    INF_LV(in_r0) = (d0_ >= (rd).lo && d0_ < (rd).hi) ? (rd).words[d0_] : 0u;                                          \
    INF_LV(in_r1) = (d1_ >= (rd).lo && d1_ < (rd).hi) ? (rd).words[d1_] : 0u;                                          \
  }

// at least 32 bits in the bit buffer
#define INF_REFILL(rd, s)                                                                                              \
  do {                                                                                                                 \
    if ((rd).nb < 32) {                                                                                                \
      if ((rd).loaded_end - (rd).di < 64) {                                                                            \
        INF_LANES                                                                                                      \
        {                                                                                                              \
          (s).inw[((rd).loaded_end + (uint32_t)lane) & 255u] = INF_LV(in_r0);                                          \
          (s).inw[((rd).loaded_end + (uint32_t)lane + 64) & 255u] = INF_LV(in_r1);                                     \
        }                                                                                                              \
        (rd).loaded_end += 128;                                                                                        \
        INF_ISSUE(rd)                                                                                                  \
        INF_FENCE();                                                                                                   \
      }                                                                                                                \
      (rd).bb |= (uint64_t)(s).inw[(rd).di & 255u] << (rd).nb;                                                         \
      (rd).nb += 32;                                                                                                   \
      (rd).di += 1;                                                                                                    \
    }                                                                                                                  \
  } while (0)

// the stream goes on at byte `at` of the call's compressed bytes
#define INF_SEEK(rd, s, at)                                                                                            \
  do {                                                                                                                 \
    (rd).di = (uint32_t)((at) >> 2);                                                                                   \
    (rd).loaded_end = (rd).di;                                                                                         \
    (rd).bb = 0;                                                                                                       \
    (rd).nb = 0;                                                                                                       \
    INF_ISSUE(rd)                                                                                                      \
    INF_REFILL(rd, s);                                                                                                 \
    (rd).bb >>= 8 * (int)((at) & 3);                                                                                   \
    (rd).nb -= 8 * (int)((at) & 3);                                                                                    \
  } while (0)

// n <= 32 bits; the caller has refilled
INF_FN uint32_t
inf_take(InfReader& rd, int n)
{
  if (n > rd.avail) {
    rd.failed = true;
    rd.avail = 0;
    return 0;
  }
  const uint32_t v = (uint32_t)(rd.bb & ((1ull << n) - 1));
  rd.bb >>= n;
  rd.nb -= n;
  rd.avail -= n;
  return v;
}

// one symbol of `h`; -1: no code of `h` starts the bits (or the payload ended).  The caller has refilled.
INF_FN int
inf_symbol(InfReader& rd, const InfHuff& h)
{
  const uint32_t e = h.fast[(uint32_t)rd.bb & ((1u << h.bits) - 1)];
  if (e) {
    (void)inf_take(rd, (int)(e & 15u));
    return rd.failed ? -1 : (int)(e >> 4);
  }
  // a longer code: canonical decoding, a bit at a time
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((rd.bb >> (l - 1)) & 1u);
    const int c = h.count[l];
    if (code - c < first) {
      (void)inf_take(rd, l);
      return rd.failed ? -1 : (int)h.sorted[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// text [a, b) of the member leaves the ring: bytes up to the first 4-byte boundary of the destination, dwords, bytes
INF_FN void
inf_flush(InfLds& s, char* out, uint32_t a, uint32_t b)
{
  INF_FENCE();
  const uint32_t n = b - a;
  uint32_t head = (uint32_t)((4 - ((uintptr_t)(out + a) & 3)) & 3);
  head = head < n ? head : n;
  const uint32_t n4 = (n - head) >> 2, tail0 = a + head + 4 * n4;
  INF_LANES
  {
    if ((uint32_t)lane < head) {
      out[a + (uint32_t)lane] = (char)s.ring[(a + (uint32_t)lane) & INF_RMASK];
    }
    uint32_t* o4 = reinterpret_cast<uint32_t*>(out + a + head);
    for (uint32_t i = (uint32_t)lane; i < n4; i += 64) {
      const uint32_t q = a + head + 4 * i;
      o4[i] = (uint32_t)s.ring[q & INF_RMASK] | (uint32_t)s.ring[(q + 1) & INF_RMASK] << 8 | (uint32_t)s.ring[(q + 2) & INF_RMASK] << 16 | (uint32_t)s.ring[(q + 3) & INF_RMASK] << 24;
    }
    if (tail0 + (uint32_t)lane < b) { // (fewer than 4)
      out[tail0 + (uint32_t)lane] = (char)s.ring[(tail0 + (uint32_t)lane) & INF_RMASK];
    }
  }
  INF_FENCE();
}

// what the open form of inf_stream reports beside its status: only where the status is INF_OK
struct InfOpenEnd
{
  uint64_t bits;     // consumed, from comp_bit on: the step ended at that block boundary
  uint32_t text_len; // that came out
  uint32_t final;    // 1: the boundary lies behind a final block
};

enum InfForm : int
{
  INF_MEMBER = 0,
  INF_SEGMENT = 1,
  INF_OPEN = 2,
};

// Inflates one stream, text to out[0, text_len), and returns its status.  Three forms, chosen at compile time:
//   a member (SEG false)   the payload is the BYTES comp[start, start + length), it has no history and ends with its final
//                          block; at most 64 KiB of text (the host checks that)
//   a segment (SEG true)   start and length are BITS, comp_bit and n_bits below: a run of whole blocks out of the middle of a serial stream (include/grpath_ingest.h:
//                          grp_gzip_inflate): it starts at BIT comp_bit, which need not lie on a byte; the dict_len <= 32768
//                          bytes of text in front of it are put into the ring in front of text position 0, and a distance
//                          may reach p + dict_len back; it ends at the block boundary where exactly n_bits are consumed —
//                          behind a final block if and only if seg_flags says that it ends its member.  A stored block
//                          aligns to a byte of the FILE, so the padding and the block's address come from the absolute
//                          bit position comp_bit + n_bits - avail.  text_len is any 32-bit number.
//   an open step (OPEN)    a segment whose end is not known (include/grpath_ingest.h: grp_gzip_walk): it starts like a segment,
//                          n_bits are the bits there ARE, text_len the room of `out`, seg_flags the least text it is to
//                          produce (min_text).  It decodes whole blocks and stops behind the first block where at least
//                          min_text bytes have come out, or behind a final block, whichever comes first, and says where
//                          that was (*end).  Text that would not fit the room: INF_NO_ROOM; the bits ending inside a
//                          block or in front of the next one: INF_INPUT_ENDS.  The last min(32768, dict_len + text)
//                          bytes of history and text — the history of the step behind it — go to hist_out, their
//                          number to *hist_len.
template <int FORM>
INF_FN uint32_t
inf_stream(InfLds& s, const uint8_t* comp, uint64_t start, uint64_t length, const uint8_t* dict, uint32_t dict_len, uint32_t seg_flags, char* out, uint32_t text_len, InfOpenEnd* end = nullptr, uint8_t* hist_out = nullptr,
           uint32_t* hist_len = nullptr)
{
  constexpr bool SEG = FORM != INF_MEMBER, OPEN = FORM == INF_OPEN;
  constexpr uint32_t TOO_LONG = OPEN ? INF_NO_ROOM : INF_TEXT_TOO_LONG;
  const uint64_t comp_bit = start, n_bits = length;    // (a segment's)
  const uint64_t comp_off = SEG ? start >> 3 : start;  // a member's payload; a segment's first byte
  const uint32_t comp_len = SEG ? 0u : (uint32_t)length;
  const InfHuff lit{ s.lit_fast, s.lit_sorted, s.lit_count, INF_LBITS };
  const InfHuff dist{ s.dist_fast, s.dist_sorted, s.dist_count, INF_DBITS };
  const InfHuff cl{ s.cl_fast, s.cl_sorted, s.cl_count, INF_CBITS };
  INF_READER_LV;
  InfReader rd;
  rd.words = reinterpret_cast<const uint32_t*>(comp);
  rd.failed = false;
  if constexpr (SEG) {
    rd.lo = (uint32_t)(comp_bit >> 5);
    rd.hi = (uint32_t)((comp_bit + n_bits + 31) >> 5);
    rd.avail = (int64_t)n_bits;
    INF_SEEK(rd, s, comp_off);
    rd.bb >>= (int)(comp_bit & 7); // (the seek leaves at least 8 bits)
    rd.nb -= (int)(comp_bit & 7);
    // the history: ring position (q - dict_len) & INF_RMASK for its byte q, as if it were text [-dict_len, 0)
    if (((dict_len | (uint32_t)(uintptr_t)dict) & 3u) == 0) {
      INF_LANES
      {
        uint32_t* r4 = reinterpret_cast<uint32_t*>(s.ring);
        const uint32_t* d4 = reinterpret_cast<const uint32_t*>(dict);
        for (uint32_t j = (uint32_t)lane; j < dict_len / 4; j += 64) {
          r4[((INF_RING - dict_len) / 4 + j) & (INF_RMASK / 4)] = d4[j];
        }
      }
    } else {
      INF_LANES
      {
        for (uint32_t j = (uint32_t)lane; j < dict_len; j += 64) {
          s.ring[(INF_RING - dict_len + j) & INF_RMASK] = dict[j];
        }
      }
    }
    INF_FENCE();
  } else {
    rd.lo = (uint32_t)(comp_off >> 2);
    rd.hi = (uint32_t)((comp_off + comp_len + 3) >> 2);
    rd.avail = (int64_t)comp_len * 8;
    INF_SEEK(rd, s, comp_off);
  }
  uint32_t p = 0, flushed = 0; // text produced, text that has left the ring

  for (;;) { // a block per iteration: its header consumes three bits
    INF_REFILL(rd, s);
    const uint32_t last = inf_take(rd, 1), type = inf_take(rd, 2);
    if (rd.failed) {
      return INF_INPUT_ENDS;
    }
    if (type == 3) {
      return INF_BAD_BLOCK_TYPE;
    }
    if (type == 0) {
      if constexpr (SEG) {
        (void)inf_take(rd, (int)((0 - (comp_bit + n_bits - (uint64_t)rd.avail)) & 7)); // to the byte boundary of the file
      } else {
        (void)inf_take(rd, (int)(rd.avail & 7)); // to the byte boundary (the payload starts on one)
      }
      INF_REFILL(rd, s);
      const uint32_t len = inf_take(rd, 16), nlen = inf_take(rd, 16);
      if (rd.failed) {
        return INF_INPUT_ENDS;
      }
      if ((len ^ 0xffffu) != nlen) {
        return INF_STORED_LEN;
      }
      if ((int64_t)len * 8 > rd.avail) {
        return INF_INPUT_ENDS;
      }
      if (len > text_len - p) {
        return TOO_LONG;
      }
      uint64_t at = SEG ? (comp_bit + n_bits - (uint64_t)rd.avail) >> 3 : comp_off + comp_len - (uint64_t)(rd.avail >> 3); // the block's bytes inside comp
      rd.avail -= (int64_t)len * 8;
      for (uint32_t left = len; left != 0;) { // every piece produces text
        const uint32_t piece = left < INF_PIECE ? left : INF_PIECE;
        INF_LANES
        {
          for (uint32_t j = (uint32_t)lane; j < piece; j += 64) {
            s.ring[(p + j) & INF_RMASK] = comp[at + j];
          }
        }
        p += piece;
        at += piece;
        left -= piece;
        if (p - flushed >= INF_FLUSH) {
          inf_flush(s, out, flushed, p);
          flushed = p;
        }
      }
      INF_FENCE();
      INF_SEEK(rd, s, at);
    } else {
      if (type == 1) {
        INF_LANES
        {
          for (int i = lane; i < 288; i += 64) {
            s.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
          }
          if (lane < 32) {
            s.lens[288 + lane] = 5;
          }
        }
        (void)inf_build(s, lit, s.lens, 288, false);
        (void)inf_build(s, dist, s.lens + 288, 32, false);
      } else {
        INF_REFILL(rd, s);
        const uint32_t n_lit = inf_take(rd, 5) + 257, n_dist = inf_take(rd, 5) + 1, n_cl = inf_take(rd, 4) + 4;
        if (rd.failed) {
          return INF_INPUT_ENDS;
        }
        if (n_lit > 286 || n_dist > 30) {
          return INF_TOO_MANY_SYMBOLS;
        }
        INF_LANES
        {
          if (lane < 19) {
            s.lens[320 + lane] = 0;
          }
        }
        INF_FENCE();
        for (uint32_t i = 0; i < n_cl; ++i) {
          // the order the code length code's lengths are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
          const uint32_t slot = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
          INF_REFILL(rd, s);
          s.lens[320 + slot] = (uint8_t)inf_take(rd, 3);
        }
        if (rd.failed) {
          return INF_INPUT_ENDS;
        }
        if (inf_build(s, cl, s.lens + 320, 19, false)) {
          return INF_BAD_CODE_LENGTHS;
        }
        // the literal/length and the distance lengths are one sequence: a repeat may run from the first into the second
        const uint32_t n_all = n_lit + n_dist;
        for (uint32_t i = 0; i < n_all;) { // every iteration sets at least one length
          INF_REFILL(rd, s);
          const int sym = inf_symbol(rd, cl);
          if (sym < 0) {
            return rd.failed ? INF_INPUT_ENDS : INF_BAD_CODE_LENGTHS;
          }
          if (sym < 16) {
            s.lens[i++] = (uint8_t)sym;
            continue;
          }
          uint32_t rep, val = 0;
          if (sym == 16) {
            if (i == 0) {
              return INF_BAD_REPEAT;
            }
            INF_FENCE();
            val = s.lens[i - 1];
            rep = 3 + inf_take(rd, 2);
          } else if (sym == 17) {
            rep = 3 + inf_take(rd, 3);
          } else {
            rep = 11 + inf_take(rd, 7);
          }
          if (rd.failed) {
            return INF_INPUT_ENDS;
          }
          if (i + rep > n_all) {
            return INF_BAD_REPEAT;
          }
          for (uint32_t j = 0; j < rep; ++j) {
            s.lens[i++] = (uint8_t)val;
          }
        }
        INF_FENCE();
        if (s.lens[256] == 0) {
          return INF_NO_END_OF_BLOCK;
        }
        // the distance lengths move behind the literal/length table's 288 entries, so that both can be built in place
        INF_LANES
        {
          uint8_t v = 0;
          if ((uint32_t)lane < n_dist) {
            v = s.lens[n_lit + (uint32_t)lane];
          }
          if (lane < 32) {
            s.lens[320 + lane] = (uint32_t)lane < n_dist ? v : (uint8_t)0;
          }
        }
        INF_FENCE();
        if (inf_build(s, lit, s.lens, (int)n_lit, true)) {
          return INF_BAD_LITLEN_SET;
        }
        if (inf_build(s, dist, s.lens + 320, (int)n_dist, true)) {
          return INF_BAD_DIST_SET;
        }
      }
      for (;;) { // a symbol per iteration: it consumes at least one bit
        INF_REFILL(rd, s);
        int sym = inf_symbol(rd, lit);
        if (sym < 0) {
          return rd.failed ? INF_INPUT_ENDS : INF_BAD_LITLEN_CODE;
        }
        if (sym < 256) {
          if (p >= text_len) {
            return TOO_LONG;
          }
          s.ring[p & INF_RMASK] = (uint8_t)sym;
          p += 1;
        } else if (sym == 256) {
          break;
        } else {
          sym -= 257;
          if (sym >= 29) {
            return INF_BAD_LITLEN_CODE;
          }
          uint32_t len;
          if (sym < 8) {
            len = 3 + (uint32_t)sym;
          } else if (sym == 28) {
            len = 258;
          } else {
            const int xb = (sym - 4) >> 2;
            len = ((4u + ((uint32_t)sym & 3u)) << xb) + 3 + inf_take(rd, xb);
          }
          INF_REFILL(rd, s);
          const int ds = inf_symbol(rd, dist);
          if (ds < 0) {
            return rd.failed ? INF_INPUT_ENDS : INF_BAD_DIST_CODE;
          }
          if (ds >= 30) {
            return INF_BAD_DIST_CODE;
          }
          uint32_t d;
          if (ds < 4) {
            d = 1 + (uint32_t)ds;
          } else {
            const int xb = (ds >> 1) - 1;
            d = ((2u + ((uint32_t)ds & 1u)) << xb) + 1 + inf_take(rd, xb);
          }
          if (rd.failed) {
            return INF_INPUT_ENDS;
          }
          if (SEG ? (d > p && d - p > dict_len) : d > p) { // BGZF members share no history, a segment has dict_len bytes of it
            return INF_DIST_TOO_FAR;
          }
          if (len > text_len - p) {
            return TOO_LONG;
          }
          // every source lies in front of p: written before this copy, whatever the overlap
          INF_FENCE();
          for (uint32_t j0 = 0; j0 < len; j0 += 64) { // 64 bytes at a time: all of them read, then all of them written
            INF_LANES
            {
              const uint32_t j = j0 + (uint32_t)lane;
              if (j < len) {
                const uint32_t k = d >= len ? j : j % d;
                s.ring[(p + j) & INF_RMASK] = s.ring[(p - d + k) & INF_RMASK];
              }
            }
          }
          INF_FENCE();
          p += len;
        }
        if (p - flushed >= INF_FLUSH) {
          inf_flush(s, out, flushed, p);
          flushed = p;
        }
      }
    }
    if constexpr (OPEN) {
      if (last || p >= seg_flags) {
        INF_FENCE();
        if (p != flushed) {
          inf_flush(s, out, flushed, p);
        }
        // the ring holds text [p - 32768, p), the history as text [-dict_len, 0)
        const uint32_t keep = dict_len + p < INF_RING ? dict_len + p : INF_RING;
        INF_LANES
        {
          for (uint32_t j = (uint32_t)lane; j < keep; j += 64) {
            hist_out[j] = s.ring[(p - keep + j) & INF_RMASK];
          }
          if (lane == 0) {
            end->bits = n_bits - (uint64_t)rd.avail;
            end->text_len = p;
            end->final = last;
            *hist_len = keep;
          }
        }
        return INF_OK;
      }
    } else if constexpr (SEG) {
      if (last) {
        if (!(seg_flags & 1u)) {
          return INF_FINAL_INSIDE;
        }
        break;
      }
      if (rd.avail == 0) { // the block boundary the segment ends at
        if (seg_flags & 1u) {
          return INF_NO_FINAL;
        }
        break;
      }
    } else {
      if (last) {
        break;
      }
    }
  }
  if (p != text_len) {
    return INF_TEXT_TOO_SHORT;
  }
  if (SEG ? rd.avail != 0 : rd.avail >= 8) {
    return INF_BYTES_BEHIND_END;
  }
  if (p != flushed) {
    inf_flush(s, out, flushed, p);
  }
  return INF_OK;
}

// how an entry of either table decodes: a BGZF member is a whole stream at a byte (it has no history: `dict` is not
// looked at), a segment starts at a bit, behind its history
INF_FN uint32_t
inf_entry(InfLds& s, const uint8_t* comp, const uint8_t*, const grp_bgzf_block& b, char* out)
{
  return inf_stream<INF_MEMBER>(s, comp, b.comp_off, b.comp_len, nullptr, 0, 0, out, b.text_len);
}

INF_FN uint32_t
inf_entry(InfLds& s, const uint8_t* comp, const uint8_t* dict, const grp_gzip_segment& g, char* out)
{
  return inf_stream<INF_SEGMENT>(s, comp, g.comp_bit, g.n_bits, dict + g.dict_off, g.dict_len, g.flags, out, g.text_len);
}

static_assert(GRP_GZIP_WALK_INPUT_ENDS == INF_INPUT_ENDS && GRP_GZIP_WALK_NO_ROOM == INF_NO_ROOM, "the two statuses the walk acts on, as grpath_ingest.h names them");

// a step of grp_gzip_walk: the open form.  The entry says where its answer and the history of the step behind it go
struct InfWalkEntry
{
  grp_gzip_walk_step step;
  grp_gzip_walk_result* res; // one lane writes it
  uint8_t* hist;             // 32768 bytes
};

INF_FN uint32_t
inf_entry(InfLds& s, const uint8_t* comp, const uint8_t* dict, const InfWalkEntry& w, char* out)
{
  InfOpenEnd end{ 0, 0, 0 };
  uint32_t hist_len = 0;
  const uint32_t st = inf_stream<INF_OPEN>(s, comp, w.step.comp_bit, w.step.n_bits, dict + w.step.dict_off, w.step.dict_len, w.step.min_text, out, w.step.room, &end, w.hist, &hist_len);
  INF_LANES
  {
    if (lane == 0) {
      *w.res = grp_gzip_walk_result{ end.bits, end.text_len, 0, end.final, st, hist_len, 0 };
    }
  }
  return st;
}

// what k_inflate_crc does with an entry: the length of its text, and the CRC32 of it — a member and a segment bring the
// CRC32 their text must have, a step of the walk takes the one its text has
INF_FN uint32_t
inf_crc_len(const grp_bgzf_block& b)
{
  return b.text_len;
}
INF_FN uint32_t
inf_crc_len(const grp_gzip_segment& g)
{
  return g.text_len;
}
INF_FN uint32_t
inf_crc_len(const InfWalkEntry& w)
{
  return w.res->text_len;
}
INF_FN uint32_t
inf_crc_done(const grp_bgzf_block& b, uint32_t c)
{
  return c != b.crc32 ? INF_CRC_MISMATCH : INF_OK;
}
INF_FN uint32_t
inf_crc_done(const grp_gzip_segment& g, uint32_t c)
{
  return c != g.crc32 ? INF_CRC_MISMATCH : INF_OK;
}
INF_FN uint32_t
inf_crc_done(const InfWalkEntry& w, uint32_t c)
{
  w.res->crc32 = c;
  return INF_OK;
}

// ---- CRC32 (the gzip polynomial, reflected: 0xedb88320) of a member's text by one wave --------------------------------
// The text is cut into 64 runs of a multiple of 4 bytes; every lane takes the remainder of its run (slicing by 4 with
// tables in LDS where the addresses are aligned), moves it behind the runs after it — a multiplication by x^(8 * bytes)
// modulo the polynomial — and the 64 results are XORed: a CRC is linear.
constexpr uint32_t CRC_POLY = 0xedb88320u;

INF_FN uint32_t
crc_mulmod(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m != 0; m >>= 1) {
    if (a & m) {
      p ^= b;
    }
    b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}

struct CrcLds
{
  uint32_t t[4 * 256 + 32]; // slicing tables t[256 * slice + byte], then x^(2^k) modulo the polynomial at t[1024 + k]
  uint32_t part[64];
};

// tables: tab[4][256] then x2n[32] (crc_tables() on the host)
INF_FN uint32_t
crc_member(CrcLds& s, const uint32_t* tables, const char* text, uint32_t n)
{
  INF_FENCE();
  INF_LANES
  {
    for (int i = lane; i < 1024 + 32; i += 64) {
      s.t[i] = tables[i];
    }
  }
  INF_FENCE();
  const uint32_t per = (((n + 63) >> 6) + 3) & ~3u;
  INF_LANES
  {
    const uint32_t a = (uint32_t)lane * per < n ? (uint32_t)lane * per : n;
    const uint32_t b = a + per < n ? a + per : n;
    uint32_t c = lane == 0 ? 0xffffffffu : 0u;
    uint32_t i = a;
    const uint8_t* t = reinterpret_cast<const uint8_t*>(text);
    for (; i < b && ((uintptr_t)(t + i) & 3) != 0; ++i) {
      c = s.t[(c ^ t[i]) & 0xff] ^ (c >> 8);
    }
    for (; i + 4 <= b; i += 4) {
      c ^= *reinterpret_cast<const uint32_t*>(t + i);
      c = s.t[768 + (c & 0xff)] ^ s.t[512 + ((c >> 8) & 0xff)] ^ s.t[256 + ((c >> 16) & 0xff)] ^ s.t[c >> 24];
    }
    for (; i < b; ++i) {
      c = s.t[(c ^ t[i]) & 0xff] ^ (c >> 8);
    }
    // c * x^(8 * (n - b))
    uint32_t shift = 1u << 31; // x^0
    uint32_t bytes = n - b;
    for (int k = 3; bytes != 0; bytes >>= 1, ++k) {
      if (bytes & 1u) {
        shift = crc_mulmod(s.t[1024 + (k & 31)], shift);
      }
    }
    s.part[lane] = crc_mulmod(c, shift);
  }
  INF_FENCE();
  uint32_t c = 0;
  for (int i = 0; i < 64; ++i) {
    c ^= s.part[i];
  }
  return c ^ 0xffffffffu;
}

#ifndef GRP_INFLATE_HOST
// one workgroup of one wave per entry (Entry: grp_bgzf_block, a member; grp_gzip_segment, a segment of a serial stream);
// toff[i]: where entry i's text starts in `text`
template <class Entry>
__global__ void __launch_bounds__(64)
k_inflate(const uint8_t* __restrict__ comp, const uint8_t* __restrict__ dict, const Entry* __restrict__ entries, const uint64_t* __restrict__ toff, uint32_t n_entries, char* __restrict__ text, uint32_t* __restrict__ status)
{
  __shared__ InfLds s;
  const uint32_t i = blockIdx.x;
  if (i >= n_entries) {
    return;
  }
  const uint32_t st = inf_entry(s, comp, dict, entries[i], text + toff[i]);
  if (threadIdx.x == 0) {
    status[i] = st;
  }
}

template <class Entry>
__global__ void __launch_bounds__(64)
k_inflate_crc(const Entry* __restrict__ entries, const uint64_t* __restrict__ toff, uint32_t n_entries, const char* __restrict__ text, const uint32_t* __restrict__ tables, uint32_t* __restrict__ status)
{
  __shared__ CrcLds s;
  const uint32_t i = blockIdx.x;
  if (i >= n_entries || status[i] != INF_OK) {
    return;
  }
  const uint32_t c = crc_member(s, tables, text + toff[i], inf_crc_len(entries[i]));
  if (threadIdx.x == 0 && inf_crc_done(entries[i], c) != INF_OK) {
    status[i] = INF_CRC_MISMATCH;
  }
}

// ---- grp_records_fetch: records out of the inflated text, formatted as the host program writes them ---------------------
// Copy-and-translate work beside a decoder that costs some 300 cycles per byte: one workgroup per record, no LDS, no
// barrier (no thread reads what another wrote).  Every part of a record — id, bases, qualities — is a span of the output
// that is filled from a span of the text: single bytes up to the destination's first 16-byte boundary, 16-byte stores
// behind it (their source read as 16-byte words where it happens to share the destination's alignment, as bytes where
// not), single bytes for what is left.  No load leaves the record's own id, bases or qualities, no store its output range.
constexpr int EMIT_THREADS = 256;

enum EmitMode
{
  EMIT_COPY = 0,   // ids, qualities of FASTQ text
  EMIT_UPPER = 1,  // bases of FASTQ text: a-z folded to upper case, as SeqReader folds what the reference later writes
  EMIT_PLUS33 = 2, // raw Phred bytes of a BAM record
  EMIT_BAM_SEQ = 3, // 4-bit codes, high half first: src is the byte of base 0, `first` the first base written
  // a reverse-strand BAM record (GRP_FETCH_REC_REVERSED), written last element first: `first` is the LAST element of the
  // stored range, output byte j comes from element first - j
  EMIT_BAM_SEQ_REV = 4, // ... the complement of the code: its bit reversal
  EMIT_PLUS33_REV = 5   // ... raw Phred bytes: src is the record's first quality
};

template <int MODE>
__device__ __forceinline__ uint8_t
emit_byte(const uint8_t* __restrict__ src, uint32_t first, uint32_t j)
{
  if constexpr (MODE == EMIT_BAM_SEQ) {
    const uint32_t b = first + j;
    const uint32_t code = (b & 1u) ? (src[b >> 1] & 15u) : (uint32_t)(src[b >> 1] >> 4);
    // "=ACMGRSVTWYHKDBN", eight characters to a word
    const uint64_t w = code < 8 ? 0x56535247'4d43413dull : 0x4e42444b'48595754ull;
    return (uint8_t)(w >> (8 * (code & 7u)));
  } else if constexpr (MODE == EMIT_BAM_SEQ_REV) {
    const uint32_t b = first - j;
    const uint32_t code = (b & 1u) ? (src[b >> 1] & 15u) : (uint32_t)(src[b >> 1] >> 4);
    // "=TGKCYSBAWRDMHVN": the character of the bit-reversed code
    const uint64_t w = code < 8 ? 0x42535943'4b47543dull : 0x4e56484d'44525741ull;
    return (uint8_t)(w >> (8 * (code & 7u)));
  } else if constexpr (MODE == EMIT_PLUS33_REV) {
    return (uint8_t)(src[first - j] + 33);
  } else {
    const uint8_t ch = src[j];
    if constexpr (MODE == EMIT_UPPER) {
      return (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
    } else if constexpr (MODE == EMIT_PLUS33) {
      return (uint8_t)(ch + 33);
    } else {
      return ch;
    }
  }
}

template <int MODE>
__device__ __forceinline__ uint32_t
emit_word(uint32_t w)
{
  uint32_t r = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint8_t ch = (uint8_t)(w >> (8 * b));
    r |= (uint32_t)emit_byte<MODE>(&ch, 0, 0) << (8 * b);
  }
  return r;
}

// dst[0, n) from src (text modes: its bytes [0, n); EMIT_BAM_SEQ: bases [first, first + n) of the codes at src)
template <int MODE>
__device__ __forceinline__ void
emit_span(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t first, uint32_t n)
{
  const uint32_t tid = threadIdx.x;
  uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15u)) & 15u);
  head = head < n ? head : n;
  const uint32_t n16 = (n - head) >> 4, tail0 = head + 16 * n16;
  for (uint32_t j = tid; j < head; j += EMIT_THREADS) {
    dst[j] = emit_byte<MODE>(src, first, j);
  }
  uint4* d4 = reinterpret_cast<uint4*>(dst + head);
  if (MODE != EMIT_BAM_SEQ && MODE != EMIT_BAM_SEQ_REV && MODE != EMIT_PLUS33_REV && ((uintptr_t)(src + head) & 15u) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head); // (words inside src[head, tail0))
    for (uint32_t i = tid; i < n16; i += EMIT_THREADS) {
      const uint4 v = s4[i];
      d4[i] = make_uint4(emit_word<MODE>(v.x), emit_word<MODE>(v.y), emit_word<MODE>(v.z), emit_word<MODE>(v.w));
    }
  } else {
    for (uint32_t i = tid; i < n16; i += EMIT_THREADS) {
      uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        w[k >> 2] |= (uint32_t)emit_byte<MODE>(src, first, head + 16 * i + (uint32_t)k) << (8 * (k & 3));
      }
      d4[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  for (uint32_t j = tail0 + tid; j < n; j += EMIT_THREADS) {
    dst[j] = emit_byte<MODE>(src, first, j);
  }
}

// out_base: the offset in the caller's buffer that out[0] stands for (a multiple of 16, so that a record's alignment is
// that of its out_off); delog: the ingest's table for the format's quality bytes (ingest_phred_table)
__global__ void __launch_bounds__(EMIT_THREADS)
k_emit_records(const uint8_t* __restrict__ text, const grp_fetch_record* __restrict__ recs, uint32_t n_recs, uint32_t out_flags, uint64_t out_base, uint8_t* __restrict__ out, const double* __restrict__ delog, double* __restrict__ sums)
{
  const uint32_t r = blockIdx.x;
  if (r >= n_recs) {
    return;
  }
  const grp_fetch_record rec = recs[r];
  const bool fastq = (out_flags & GRP_FETCH_FASTQ) != 0, bam = (out_flags & GRP_FETCH_BAM) != 0, trimmed = (rec.flags & GRP_FETCH_REC_TRIMMED) != 0;
  const bool reversed = bam && (rec.flags & GRP_FETCH_REC_REVERSED) != 0; // seq_from / qual_from name the stored range, written backwards
  const uint32_t tid = threadIdx.x;
  uint8_t* o = out + (rec.out_off - out_base);
  if (tid == 0) {
    o[0] = fastq ? '@' : '>';
  }
  emit_span<EMIT_COPY>(o + 1, text + rec.id_off, 0, rec.id_len);
  const char* suffix = trimmed ? "_trimmed\n" : "_untrimmed\n";
  const uint32_t n_suffix = trimmed ? 9u : 11u;
  if (tid < n_suffix) {
    o[1 + rec.id_len + tid] = (uint8_t)suffix[tid];
  }
  uint8_t* ob = o + 1 + rec.id_len + n_suffix;
  if (reversed) {
    emit_span<EMIT_BAM_SEQ_REV>(ob, text + rec.seq_off, rec.seq_from + rec.n_seq - 1u, rec.n_seq); // (n_seq 0: nothing is read)
  } else if (bam) {
    emit_span<EMIT_BAM_SEQ>(ob, text + rec.seq_off, rec.seq_from, rec.n_seq);
  } else {
    emit_span<EMIT_UPPER>(ob, text + rec.seq_off + rec.seq_from, 0, rec.n_seq);
  }
  if (tid == 0) {
    ob[rec.n_seq] = '\n';
  }
  const uint8_t* q = text + rec.qual_off + rec.qual_from;
  if (fastq) {
    uint8_t* oq = ob + rec.n_seq + 1;
    if (tid == 0) {
      oq[0] = '+';
      oq[1] = '\n';
      oq[2 + rec.n_qual] = '\n';
    }
    if (reversed) {
      emit_span<EMIT_PLUS33_REV>(oq + 2, q, rec.n_qual - 1u, rec.n_qual);
    } else if (bam) {
      emit_span<EMIT_PLUS33>(oq + 2, q, 0, rec.n_qual);
    } else {
      emit_span<EMIT_COPY>(oq + 2, q, 0, rec.n_qual);
    }
  }
  if (tid == 0) { // one dependent chain of additions, as in k_fq_phred
    // The chain's loads must be VECTOR loads, so the address goes through a VGPR the compiler cannot see through.  q is
    // the same in every lane, and left to itself the compiler read the qualities through the scalar unit: one
    // s_load_dwordx16 with q as its base and the byte index as its offset, which for a q that is not dword-aligned fetched
    // (q & ~3) + (index & ~3) — the 64 bytes that begin up to 4 in front of the ones asked for (seen on the MI355X: the sum of
    // a slice that begins 1 byte behind a 16-byte boundary; the emitted bytes, all vector loads, were right).
    uintptr_t qa = reinterpret_cast<uintptr_t>(q);
    asm volatile("" : "+v"(qa));
    // (a reversed record: the written line is the stored range read backwards, and so is its chain)
    sums[r] = reversed ? phred_chain_back(reinterpret_cast<const uint8_t*>(qa), 0, rec.n_qual, 0.0, delog) : phred_chain(reinterpret_cast<const uint8_t*>(qa), 0, rec.n_qual, 0.0, delog);
  }
}
#endif

// tab[4][256] (slicing by 4) and x2n[32] of the reflected gzip polynomial
inline void
crc_tables(uint32_t* out)
{
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) {
      c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    }
    out[i] = c;
  }
  for (uint32_t i = 0; i < 256; ++i) {
    for (int t = 1; t < 4; ++t) {
      const uint32_t prev = out[(t - 1) * 256 + i];
      out[t * 256 + i] = (prev >> 8) ^ out[prev & 0xff];
    }
  }
  uint32_t p = 1u << 30; // x^1
  out[1024] = p;
  for (int k = 1; k < 32; ++k) {
    uint32_t a = p, b = p, r = 0;
    for (uint32_t m = 1u << 31; m != 0; m >>= 1) {
      if (a & m) {
        r ^= b;
      }
      b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    out[1024 + k] = p = r;
  }
}

} // namespace

#ifndef GRP_INFLATE_HOST
// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

// What the launcher has to know of a format beside inf_entry: the check of one table entry against the caller's buffers
// (a reason, or nullptr) and the words of its messages.
template <class Entry>
struct InfFormat;

template <>
struct InfFormat<grp_bgzf_block>
{
  static constexpr const char* fn = "grp_bgzf_inflate";
  static constexpr const char* nouns = "blocks";
  static constexpr const char* limits = "at most 4 GiB of compressed bytes and 2^22 blocks per call";

  static const char* check_entry(const grp_bgzf_block& b, uint64_t n_comp, uint64_t)
  {
    return b.comp_off > n_comp || b.comp_len > n_comp - b.comp_off ? "its payload does not lie inside the compressed bytes" : b.text_len > INF_MAX_TEXT ? "more than 65536 bytes of text" : nullptr;
  }
  static int refuse_entry(grp_ctx* c, uint32_t i, const char* why, const grp_bgzf_block& b, uint64_t n_comp, uint64_t)
  {
    return set_err(c, GRP_ERR_INVALID, "grp_bgzf_inflate: block %u: %s (payload [%llu, +%u) of %llu, text %u)", i, why, (unsigned long long)b.comp_off, b.comp_len, (unsigned long long)n_comp, b.text_len);
  }
  static int refuse_stream(grp_ctx* c, uint32_t i, const grp_bgzf_block& b, const char* status)
  {
    return set_err(c, GRP_ERR_INVALID, "grp_bgzf_inflate: block %u is not a valid DEFLATE stream of %u bytes with CRC32 %08x: %s", i, b.text_len, b.crc32, status);
  }
};

template <>
struct InfFormat<grp_gzip_segment>
{
  static constexpr const char* fn = "grp_gzip_inflate";
  static constexpr const char* nouns = "segments";
  static constexpr const char* limits = "at most 4 GiB of compressed bytes, 4 GiB of histories and 2^22 segments per call";

  static const char* check_entry(const grp_gzip_segment& g, uint64_t n_comp, uint64_t n_dict)
  {
    return g.comp_bit > n_comp * 8 || g.n_bits > n_comp * 8 - g.comp_bit    ? "its bits do not lie inside the compressed bytes"
           : g.dict_len > INF_RING                                          ? "a history of more than 32768 bytes"
           : g.dict_off > n_dict || g.dict_len > n_dict - g.dict_off        ? "its history does not lie inside the histories"
           : g.flags & ~GRP_GZIP_SEG_FINAL                                  ? "an unknown flag"
           : g.text_len > 0xffff0000u                                       ? "more than 4 GiB - 64 KiB of text"
                                                                            : nullptr;
  }
  static int refuse_entry(grp_ctx* c, uint32_t i, const char* why, const grp_gzip_segment& g, uint64_t n_comp, uint64_t n_dict)
  {
    return set_err(c, GRP_ERR_INVALID, "grp_gzip_inflate: segment %u: %s (bits [%llu, +%llu) of %llu bytes, history [%llu, +%u) of %llu, text %u, flags %u)", i, why, (unsigned long long)g.comp_bit, (unsigned long long)g.n_bits,
                   (unsigned long long)n_comp, (unsigned long long)g.dict_off, g.dict_len, (unsigned long long)n_dict, g.text_len, g.flags);
  }
  static int refuse_stream(grp_ctx* c, uint32_t i, const grp_gzip_segment& g, const char* status)
  {
    return set_err(c, GRP_ERR_INVALID, "grp_gzip_inflate: segment %u is not %llu bits of valid DEFLATE blocks that hold %u bytes of text with CRC32 %08x: %s", i, (unsigned long long)g.n_bits, g.text_len, g.crc32, status);
  }
};

// the CRC32 tables of both formats, made on the first call of either
int
inflate_crc_tables(grp_ctx* c)
{
  if (!c->d_crc_tab.p) {
    std::vector<uint32_t> tab(4 * 256 + 32);
    crc_tables(tab.data());
    HIP_TRY(c, c->d_crc_tab.reset(tab.size()));
    HIP_TRY(c, hipMemcpy(c->d_crc_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  return GRP_OK;
}

// the checks of a table that are made before anything is launched; *total = the bytes of text its entries hold
template <class Entry>
int
inflate_check_table(grp_ctx* c, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const Entry* entries, uint32_t n, uint32_t* bad, uint64_t* total)
{
  using F = InfFormat<Entry>;
  if ((!comp && n_comp) || (!dict && n_dict) || (!entries && n) || n_comp > (1ull << 32) || n_dict > (1ull << 32) || n > MAX_GRID_WGS) {
    return set_err(c, GRP_ERR_INVALID, "%s: bad argument (%s)", F::fn, F::limits);
  }
  *total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (const char* why = F::check_entry(entries[i], n_comp, n_dict)) {
      if (bad) {
        *bad = i;
      }
      return F::refuse_entry(c, i, why, entries[i], n_comp, n_dict);
    }
    *total += entries[i].text_len;
  }
  return GRP_OK;
}

// What the launches of all three entry types share.  inflate_reserve: the pool's device buffers for n entries of `per`
// elements of the pool's entry type each, grown, never shrunk (like the ingest's buffers) — the kernels read whole words: 8
// bytes of padding behind the compressed bytes, the histories and the text — and its page-locked staging; the caller then
// writes the entries and the text offsets into the staging.  inflate_send: the compressed bytes with their padding, the
// histories, the entries and the offsets go up on `st`.
template <class Pool>
int
inflate_reserve(grp_ctx* c, Pool& p, uint64_t n_comp, uint64_t n_dict, uint64_t total, uint32_t n, uint64_t per = 1)
{
  HIP_TRY(c, p.d_comp.ensure(n_comp + 8));
  HIP_TRY(c, p.d_dict.ensure(n_dict + 8));
  HIP_TRY(c, p.d_text.ensure(total + 8));
  HIP_TRY(c, p.d_entries.ensure((uint64_t)n * per));
  HIP_TRY(c, p.d_toff.ensure(n));
  HIP_TRY(c, p.d_status.ensure(n));
  if (p.h_toff.cap < n) {
    const uint64_t cap = (uint64_t)n + n / 4 + 64;
    HIP_TRY(c, p.h_entries.reset(cap * per, hipHostMallocDefault));
    HIP_TRY(c, p.h_toff.reset(cap, hipHostMallocDefault));
    HIP_TRY(c, p.h_status.reset(cap, hipHostMallocDefault));
  }
  return GRP_OK;
}

template <class Pool>
int
inflate_send(grp_ctx* c, Pool& p, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, uint32_t n, uint64_t per, hipStream_t st)
{
  if (n_comp) {
    HIP_TRY(c, hipMemcpyAsync(p.d_comp, comp, n_comp, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemsetAsync(p.d_comp + n_comp, 0, 8, st));
  if (n_dict) {
    HIP_TRY(c, hipMemcpyAsync(p.d_dict, dict, n_dict, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemcpyAsync(p.d_entries, p.h_entries.p, (size_t)n * per * sizeof(*p.h_entries.p), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(p.d_toff, p.h_toff.p, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  return GRP_OK;
}

// grp_bgzf_inflate and grp_gzip_inflate (a BGZF call has no histories: dict == nullptr, n_dict == 0).  `keep_text`: the
// text is not copied to the caller (text_out and text_cap are not looked at): it is in p.d_text, entry i's at p.h_toff[i],
// when the call returns GRP_OK (grp_records_fetch)
template <class Entry>
int
inflate_entries(grp_ctx* c, grp_ctx::InflatePool<Entry>& p, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const Entry* entries, uint32_t n, char* text_out, uint64_t text_cap, uint32_t* bad, bool keep_text = false)
{
  using F = InfFormat<Entry>;
  // the table is checked before anything is launched
  uint64_t total = 0;
  if (const int rc = inflate_check_table(c, comp, n_comp, dict, n_dict, entries, n, bad, &total)) {
    return rc;
  }
  if (!keep_text && (total > text_cap || (total && !text_out))) {
    return set_err(c, GRP_ERR_INVALID, "%s: the %s hold %llu bytes of text, the caller's buffer %llu", F::fn, F::nouns, (unsigned long long)total, (unsigned long long)text_cap);
  }
  if (n == 0) {
    return GRP_OK;
  }
  hipStream_t st = c->stream2; // (a fill queued on the main stream keeps running beside this)
  if (const int rc = inflate_crc_tables(c)) {
    return rc;
  }
  if (!p.ev0.e) {
    HIP_TRY(c, p.ev0.create(hipEventDefault));
    HIP_TRY(c, p.ev1.create(hipEventDefault));
  }
  if (const int rc = inflate_reserve(c, p, n_comp, n_dict, total, n)) {
    return rc;
  }
  memcpy(p.h_entries.p, entries, (size_t)n * sizeof(Entry));
  uint64_t off = 0;
  for (uint32_t i = 0; i < n; ++i) {
    p.h_toff.p[i] = off;
    off += entries[i].text_len;
  }
  if (const int rc = inflate_send(c, p, comp, n_comp, dict, n_dict, n, 1, st)) {
    return rc;
  }
  HIP_TRY(c, hipEventRecord(p.ev0, st));
  k_inflate<Entry><<<n, 64, 0, st>>>(p.d_comp, p.d_dict, p.d_entries, p.d_toff, n, reinterpret_cast<char*>(p.d_text.p), p.d_status);
  k_inflate_crc<Entry><<<n, 64, 0, st>>>(p.d_entries, p.d_toff, n, reinterpret_cast<const char*>(p.d_text.p), c->d_crc_tab, p.d_status);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(p.ev1, st));
  HIP_TRY(c, hipMemcpyAsync(p.h_status.p, p.d_status, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (total && !keep_text) {
    HIP_TRY(c, hipMemcpyAsync(text_out, p.d_text, total, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, p.ev0, p.ev1) == hipSuccess) {
    p.kernel_us += (double)ms * 1000.0;
  }
  p.n_entries += n;
  p.n_comp += n_comp;
  p.n_text += total;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t s = p.h_status.p[i];
    if (s != INF_OK) {
      if (bad) {
        *bad = i;
      }
      return F::refuse_stream(c, i, entries[i], s < INF_STATUS_COUNT ? INF_STATUS_TEXT[s] : "unknown status");
    }
  }
  return GRP_OK;
}

template <class Pool>
int
inflate_stats(const Pool* p, uint64_t out[4])
{
  if (!p || !out) {
    return GRP_ERR_INVALID;
  }
  out[0] = p->n_entries;
  out[1] = p->n_comp;
  out[2] = p->n_text;
  out[3] = (uint64_t)p->kernel_us;
  return GRP_OK;
}

} // namespace

extern "C" int
grp_bgzf_inflate(grp_ctx* c, const uint8_t* comp, uint64_t n_comp, const grp_bgzf_block* blocks, uint32_t n_blocks, char* text_out, uint64_t text_cap, uint32_t* bad_block)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (bad_block) {
    *bad_block = UINT32_MAX;
  }
  return inflate_entries(c, c->bgzf, comp, n_comp, nullptr, 0, blocks, n_blocks, text_out, text_cap, bad_block);
}

extern "C" int
grp_gzip_inflate(grp_ctx* c, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_segment* segs, uint32_t n_segs, char* text_out, uint64_t text_cap, uint32_t* bad_seg)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (bad_seg) {
    *bad_seg = UINT32_MAX;
  }
  return inflate_entries(c, c->gzip, comp, n_comp, dict, n_dict, segs, n_segs, text_out, text_cap, bad_seg);
}

// One open step per entry: k_inflate<InfWalkEntry>, then k_inflate_crc<InfWalkEntry> for the CRC32 of what came out, over
// the buffers and uploads of inflate_entries (inflate_reserve, inflate_send).  What differs from it is what comes back: a
// step's status is its answer, not the call's, and every step has its answer and its new history.
extern "C" int
grp_gzip_walk(grp_ctx* c, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n, grp_gzip_walk_result* results, uint8_t* hist_out, char* text_out, uint64_t text_cap,
              uint32_t* bad_step)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (bad_step) {
    *bad_step = UINT32_MAX;
  }
  if ((!comp && n_comp) || (!dict && n_dict) || (n && (!steps || !results || !hist_out)) || n_comp > (1ull << 32) || n_dict > (1ull << 32) || n > MAX_GRID_WGS) {
    return set_err(c, GRP_ERR_INVALID, "grp_gzip_walk: bad argument (at most 4 GiB of compressed bytes, 4 GiB of histories and 2^22 steps per call)");
  }
  // the table is checked before anything is launched
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const grp_gzip_walk_step& g = steps[i];
    total += g.room;
    const char* why = g.comp_bit > n_comp * 8 || g.n_bits > n_comp * 8 - g.comp_bit ? "its bits do not lie inside the compressed bytes"
                      : g.dict_len > INF_RING                                       ? "a history of more than 32768 bytes"
                      : g.dict_off > n_dict || g.dict_len > n_dict - g.dict_off     ? "its history does not lie inside the histories"
                      : g.reserved != 0                                             ? "a reserved field that is not 0"
                      : total > (1ull << 34)                                        ? "the rooms up to this step are more than 2^34 bytes"
                      : text_out && total > text_cap                                ? "the rooms up to this step are more than the caller's buffer"
                                                                                    : nullptr;
    if (why) {
      if (bad_step) {
        *bad_step = i;
      }
      return set_err(c, GRP_ERR_INVALID, "grp_gzip_walk: step %u: %s (bits [%llu, +%llu) of %llu bytes, history [%llu, +%u) of %llu, min_text %u, room %u, rooms so far %llu of %llu)", i, why, (unsigned long long)g.comp_bit,
                     (unsigned long long)g.n_bits, (unsigned long long)n_comp, (unsigned long long)g.dict_off, g.dict_len, (unsigned long long)n_dict, g.min_text, g.room, (unsigned long long)total,
                     (unsigned long long)(text_out ? text_cap : 1ull << 34));
    }
  }
  if (n == 0) {
    return GRP_OK;
  }
  hipStream_t st = c->stream2;
  if (const int rc = inflate_crc_tables(c)) {
    return rc;
  }
  grp_ctx::WalkPool& w = c->walk;
  auto& p = w.io;
  // (the pool keeps its entries as bytes: InfWalkEntry is this file's)
  if (const int rc = inflate_reserve(c, p, n_comp, n_dict, total, n, sizeof(InfWalkEntry))) {
    return rc;
  }
  HIP_TRY(c, w.d_res.ensure(n));
  HIP_TRY(c, w.d_hist.ensure((uint64_t)n * INF_RING));
  if (w.h_res.cap < n) {
    HIP_TRY(c, w.h_res.reset((uint64_t)n + n / 4 + 64, hipHostMallocDefault));
  }
  InfWalkEntry* he = reinterpret_cast<InfWalkEntry*>(p.h_entries.p);
  InfWalkEntry* de = reinterpret_cast<InfWalkEntry*>(p.d_entries.p);
  uint64_t off = 0;
  for (uint32_t i = 0; i < n; ++i) {
    he[i] = InfWalkEntry{ steps[i], w.d_res.p + i, w.d_hist.p + (uint64_t)i * INF_RING };
    p.h_toff.p[i] = off;
    off += steps[i].room;
  }
  if (const int rc = inflate_send(c, p, comp, n_comp, dict, n_dict, n, sizeof(InfWalkEntry), st)) {
    return rc;
  }
  k_inflate<InfWalkEntry><<<n, 64, 0, st>>>(p.d_comp, p.d_dict, de, p.d_toff, n, reinterpret_cast<char*>(p.d_text.p), p.d_status);
  k_inflate_crc<InfWalkEntry><<<n, 64, 0, st>>>(de, p.d_toff, n, reinterpret_cast<const char*>(p.d_text.p), c->d_crc_tab, p.d_status);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(w.h_res.p, w.d_res, (size_t)n * sizeof(grp_gzip_walk_result), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(hist_out, w.d_hist, (size_t)n * INF_RING, hipMemcpyDeviceToHost, st));
  if (text_out && total) {
    HIP_TRY(c, hipMemcpyAsync(text_out, p.d_text, total, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  for (uint32_t i = 0; i < n; ++i) {
    results[i] = w.h_res.p[i];
    if (results[i].status != INF_OK) { // (nothing of a step that did not reach a boundary is an answer)
      results[i] = grp_gzip_walk_result{ 0, 0, 0, 0, results[i].status, 0, 0 };
    }
  }
  return GRP_OK;
}

extern "C" const char*
grp_gzip_status_text(uint32_t status)
{
  return status < INF_STATUS_COUNT ? INF_STATUS_TEXT[status] : status == INF_NO_ROOM ? INF_NO_ROOM_TEXT : "unknown status";
}

namespace {

// grp_records_fetch for either kind of unit
template <class Entry>
int
records_fetch(grp_ctx* c, grp_ctx::InflatePool<Entry>& p, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const Entry* units, uint32_t n_units, const grp_fetch_record* recs, uint32_t n_recs,
              uint32_t out_flags, char* out, uint64_t out_cap, double* sums, uint32_t* bad_unit, uint32_t* bad_record)
{
  // both tables are checked before anything is launched
  uint64_t total = 0;
  if (const int rc = inflate_check_table(c, comp, n_comp, dict, n_dict, units, n_units, bad_unit, &total)) {
    return rc;
  }
  if ((!recs && n_recs) || n_recs > MAX_GRID_WGS || (out_flags & ~(GRP_FETCH_FASTQ | GRP_FETCH_BAM)) || (n_recs && (!out || !sums))) {
    return set_err(c, GRP_ERR_INVALID, "grp_records_fetch: bad argument (at most 2^22 records per call, out_flags 0 .. 3)");
  }
  const bool fastq = (out_flags & GRP_FETCH_FASTQ) != 0, bam = (out_flags & GRP_FETCH_BAM) != 0;
  const auto inside = [total](uint64_t off, uint64_t len) { return off <= total && len <= total - off; };
  std::vector<std::pair<uint64_t, uint64_t>> span(n_recs); // [begin, end) in `out`
  for (uint32_t i = 0; i < n_recs; ++i) {
    const grp_fetch_record& r = recs[i];
    // the bytes the written bases are read from (BAM: two bases to a byte)
    const uint64_t seq_first = bam ? r.seq_from / 2 : r.seq_from;
    const uint64_t seq_bytes = !bam ? r.n_seq : r.n_seq ? ((uint64_t)r.seq_from + r.n_seq + 1) / 2 - seq_first : 0;
    const uint64_t size = 1 + (uint64_t)r.id_len + ((r.flags & GRP_FETCH_REC_TRIMMED) ? 9 : 11) + r.n_seq + 1 + (fastq ? 3 + (uint64_t)r.n_qual : 0);
    const char* why = (r.flags & ~(GRP_FETCH_REC_TRIMMED | (bam ? GRP_FETCH_REC_REVERSED : 0u)))  ? "an unknown flag"
                      : !inside(r.id_off, r.id_len)                                               ? "its id does not lie inside the units' text"
                      : r.seq_off > total || !inside(r.seq_off + seq_first, seq_bytes)            ? "its bases do not lie inside the units' text"
                      : r.qual_off > total || !inside(r.qual_off + r.qual_from, r.n_qual)         ? "its qualities do not lie inside the units' text"
                      : r.out_off > out_cap || size > out_cap - r.out_off                         ? "its output does not lie inside the caller's buffer"
                                                                                                  : nullptr;
    if (why) {
      if (bad_record) {
        *bad_record = i;
      }
      return set_err(c, GRP_ERR_INVALID, "grp_records_fetch: record %u: %s (id [%llu, +%u), bases %llu + [%u, +%u), qualities %llu + [%u, +%u) of %llu bytes of text; output [%llu, +%llu) of %llu, flags %u)", i, why,
                     (unsigned long long)r.id_off, r.id_len, (unsigned long long)r.seq_off, r.seq_from, r.n_seq, (unsigned long long)r.qual_off, r.qual_from, r.n_qual, (unsigned long long)total, (unsigned long long)r.out_off,
                     (unsigned long long)size, (unsigned long long)out_cap, r.flags);
    }
    span[i] = { r.out_off, r.out_off + size };
  }
  std::vector<uint32_t> order(n_recs);
  for (uint32_t i = 0; i < n_recs; ++i) {
    order[i] = i;
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return span[a].first != span[b].first ? span[a].first < span[b].first : a < b; });
  for (uint32_t k = 1; k < n_recs; ++k) {
    if (span[order[k]].first < span[order[k - 1]].second) {
      if (bad_record) {
        *bad_record = order[k];
      }
      return set_err(c, GRP_ERR_INVALID, "grp_records_fetch: record %u: its output [%llu, %llu) overlaps that of record %u, [%llu, %llu)", order[k], (unsigned long long)span[order[k]].first, (unsigned long long)span[order[k]].second,
                     order[k - 1], (unsigned long long)span[order[k - 1]].first, (unsigned long long)span[order[k - 1]].second);
    }
  }
  if (n_recs == 0) {
    return GRP_OK; // (nothing is asked for: nothing is inflated)
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (const int rc = inflate_entries(c, p, comp, n_comp, dict, n_dict, units, n_units, nullptr, 0, bad_unit, true)) {
    return rc;
  }
  // the units' text is in p.d_text now, every unit with its CRC32
  if (const int rc = bam ? ingest_phred_table(c, c->d_delog_raw, 0, "grp_records_fetch") : ingest_phred_table(c, c->d_delog, 33, "grp_records_fetch")) {
    return rc;
  }
  hipStream_t st = c->stream2;
  grp_ctx::FetchPool& f = c->fetch;
  const uint64_t out_lo = span[order[0]].first & ~15ull; // (the device buffer begins at a 16-byte boundary of the caller's)
  uint64_t out_hi = 0;
  for (uint32_t i = 0; i < n_recs; ++i) {
    out_hi = std::max(out_hi, span[i].second);
  }
  HIP_TRY(c, f.d_out.ensure(out_hi - out_lo));
  HIP_TRY(c, f.d_recs.ensure(n_recs));
  HIP_TRY(c, f.d_sums.ensure(n_recs));
  HIP_TRY(c, hipMemcpyAsync(f.d_recs, recs, (size_t)n_recs * sizeof(grp_fetch_record), hipMemcpyHostToDevice, st));
  k_emit_records<<<n_recs, EMIT_THREADS, 0, st>>>(p.d_text, f.d_recs, n_recs, out_flags, out_lo, f.d_out, bam ? c->d_delog_raw : c->d_delog, f.d_sums);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(sums, f.d_sums, (size_t)n_recs * sizeof(double), hipMemcpyDeviceToHost, st));
  // the records alone come down: one copy per run of records that lie back to back (a caller that packs them: one copy)
  for (uint32_t k = 0; k < n_recs;) {
    const uint64_t b = span[order[k]].first;
    uint64_t e = span[order[k]].second;
    for (++k; k < n_recs && span[order[k]].first == e; ++k) {
      e = span[order[k]].second;
    }
    HIP_TRY(c, hipMemcpyAsync(out + b, f.d_out + (b - out_lo), e - b, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  return GRP_OK;
}

} // namespace

extern "C" int
grp_records_fetch(grp_ctx* c, int unit_kind, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const void* units, uint32_t n_units, const grp_fetch_record* recs, uint32_t n_recs, uint32_t out_flags, char* out,
                  uint64_t out_cap, double* sums, uint32_t* bad_unit, uint32_t* bad_record)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (bad_unit) {
    *bad_unit = UINT32_MAX;
  }
  if (bad_record) {
    *bad_record = UINT32_MAX;
  }
  if (unit_kind == GRP_FETCH_UNITS_BGZF) {
    return records_fetch(c, c->bgzf, comp, n_comp, nullptr, 0, static_cast<const grp_bgzf_block*>(units), n_units, recs, n_recs, out_flags, out, out_cap, sums, bad_unit, bad_record);
  }
  if (unit_kind == GRP_FETCH_UNITS_GZIP) {
    return records_fetch(c, c->gzip, comp, n_comp, dict, n_dict, static_cast<const grp_gzip_segment*>(units), n_units, recs, n_recs, out_flags, out, out_cap, sums, bad_unit, bad_record);
  }
  return set_err(c, GRP_ERR_INVALID, "grp_records_fetch: unit_kind %d is neither GRP_FETCH_UNITS_BGZF nor GRP_FETCH_UNITS_GZIP", unit_kind);
}

extern "C" int
grp_debug_bgzf_stats(const grp_ctx* c, uint64_t out[4])
{
  return inflate_stats(c ? &c->bgzf : nullptr, out);
}

extern "C" int
grp_debug_gzip_stats(const grp_ctx* c, uint64_t out[4])
{
  return inflate_stats(c ? &c->gzip : nullptr, out);
}
#endif
