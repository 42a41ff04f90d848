// Unaligned BAM (SAM specification §4): the record layer behind the BGZF container.  A BAM stream is a header
// ("BAM\1", l_text, text, n_ref, n_ref x {l_name, name, l_ref}) and then records, each a 4-byte block_size followed by
// that many bytes: 32 fixed bytes, the NUL-terminated read name, the CIGAR, the bases as 4-bit codes (high nibble
// first), the qualities as raw Phred bytes, tags.  The program reads such a file as its FASTQ twin: per record
//   @<name up to its NUL>\n<bases by "=ACMGRSVTWYHKDBN">\n+\n<qual + 33>\n
// With GRP_BAM_ALIGNED=on the twin is the aligned twin, what `samtools fastq -n` writes with its default filters: a
// secondary or supplementary record (flag 0x100 / 0x800) is no read of it, a reverse-strand record (flag 0x10) is read
// in its original orientation — base j = the complement of stored base l_seq-1-j, quality j = qual[l_seq-1-j] + 33.
// Header-only and pure (no I/O): the engine (grp_ingest.inc: grp_bam_parse) and the host library (gr_bam.cpp, the
// host reader of gr_fastq.cpp, the source of gr_source.cpp) walk the record chain with the ONE function below.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace gr {

constexpr uint32_t BAM_FIXED = 32;          // bytes of a record behind block_size and in front of the name
constexpr uint32_t BAM_REFUSED_FLAGS = 0x910; // reverse strand, secondary, supplementary
constexpr uint8_t BAM_MAX_QUAL = 93;          // '~' - 33
constexpr uint32_t BAM_FLAG_REVERSE = 0x10;   // read as its reverse complement where the walk's `accept` holds the bit
constexpr uint32_t BAM_FLAGS_SKIPPED = 0x900; // secondary, supplementary: consumed and not emitted where `accept` holds the bit

#if defined(__HIPCC__)
#define GR_BAM_HD __host__ __device__
#else
#define GR_BAM_HD
#endif

inline uint32_t
bam_le32(const uint8_t* p)
{
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the BAM header at the front of [buf, buf + n): 1 complete (*header_bytes = where the first record begins),
// 0 more bytes needed (nothing in what is there says otherwise), -1 not BAM (the magic, or a negative length)
inline int
bam_header(const uint8_t* buf, uint64_t n, uint64_t* header_bytes)
{
  static const uint8_t magic[4] = { 'B', 'A', 'M', 1 };
  if (memcmp(buf, magic, (size_t)(n < 4 ? n : 4)) != 0) {
    return -1;
  }
  if (n < 8) {
    return 0;
  }
  const uint32_t l_text = bam_le32(buf + 4);
  if (l_text > 0x7fffffffu) {
    return -1;
  }
  uint64_t pos = 8 + (uint64_t)l_text;
  if (n < pos + 4) {
    return 0;
  }
  const uint32_t n_ref = bam_le32(buf + pos);
  if (n_ref > 0x7fffffffu) {
    return -1;
  }
  pos += 4;
  for (uint32_t r = 0; r < n_ref; ++r) {
    if (n < pos + 4) {
      return 0;
    }
    const uint32_t l_name = bam_le32(buf + pos);
    if (l_name > 0x7fffffffu) {
      return -1;
    }
    pos += 4 + (uint64_t)l_name + 4;
  }
  if (n < pos) {
    return 0;
  }
  if (header_bytes) {
    *header_bytes = pos;
  }
  return 1;
}

// what the fixed part of a record says (offsets from the record's block_size field)
struct BamRecord
{
  uint64_t off;      // of block_size
  uint64_t name_off; // l_read_name bytes, the last of them NUL
  uint64_t seq_off;  // (l_seq + 1) / 2 bytes
  uint64_t qual_off; // l_seq bytes
  uint64_t end;      // off + 4 + block_size
  uint32_t l_read_name, l_seq, flag;
};

// The walk over the record chain of [buf, buf + n), which begins at a record: emit(BamRecord) for every COMPLETE
// record whose fields lie inside its block and whose flags the program reads (false: the caller has enough, the walk
// ends in front of that record); *consumed = the bytes of the records taken.
// `accept` (a subset of BAM_REFUSED_FLAGS; 0: unaligned input only) says which of the three flags are read instead of
// refused: a record with an accepted 0x100 / 0x800 is checked like any other, consumed, counted in *skipped and not
// emitted (*consumed may be > 0 with no record emitted); one with an accepted 0x10 is emitted with its flag.
// Returns 0 when the chain is sound as far as it goes (a record that is not complete ends the walk; with `final`
// such a tail is the truncation error), else -1 with *bad_offset = the refused record and *why = the reason.
template<class Emit>
inline int
bam_walk(const uint8_t* buf, uint64_t n, bool final, uint32_t accept, uint64_t* consumed, uint64_t* skipped, uint64_t* bad_offset, const char** why, Emit&& emit)
{
  uint64_t pos = 0;
  *consumed = 0;
  *skipped = 0;
  auto refuse = [&](const char* what) {
    *consumed = pos;
    *bad_offset = pos;
    *why = what;
    return -1;
  };
  while (pos < n) {
    if (n - pos < 4) {
      break;
    }
    const uint32_t block_size = bam_le32(buf + pos);
    if (block_size < BAM_FIXED) {
      return refuse("block_size is smaller than the fixed part of a record");
    }
    if (n - pos - 4 < (uint64_t)block_size) {
      break;
    }
    const uint8_t* r = buf + pos + 4;
    BamRecord rec;
    rec.off = pos;
    rec.l_read_name = r[8];
    const uint32_t n_cigar = (uint32_t)r[12] | ((uint32_t)r[13] << 8);
    rec.flag = (uint32_t)r[14] | ((uint32_t)r[15] << 8);
    rec.l_seq = bam_le32(r + 16);
    const uint64_t need = (uint64_t)BAM_FIXED + rec.l_read_name + 4ull * n_cigar + ((uint64_t)rec.l_seq + 1) / 2 + rec.l_seq;
    if (need > block_size) {
      return refuse("block_size is smaller than the record's name, CIGAR, bases and qualities");
    }
    if (rec.l_read_name == 0) {
      return refuse("l_read_name is 0");
    }
    rec.name_off = pos + 4 + BAM_FIXED;
    if (buf[rec.name_off + rec.l_read_name - 1] != 0) {
      return refuse("the read name does not end in NUL");
    }
    if (rec.flag & BAM_REFUSED_FLAGS & ~accept) {
      return refuse("a reverse-strand, secondary or supplementary record (flag 0x10 / 0x100 / 0x800): convert the file with samtools fastq, or set GRP_BAM_ALIGNED=on");
    }
    rec.seq_off = rec.name_off + rec.l_read_name + 4ull * n_cigar;
    rec.qual_off = rec.seq_off + ((uint64_t)rec.l_seq + 1) / 2;
    rec.end = pos + 4 + (uint64_t)block_size;
    if (rec.flag & BAM_FLAGS_SKIPPED) { // (accepted: no read of the aligned twin; its bases and qualities are not looked at)
      ++*skipped;
      pos = rec.end;
      continue;
    }
    if (!emit(rec)) {
      *consumed = pos;
      return 0;
    }
    pos = rec.end;
  }
  *consumed = pos;
  if (final && pos < n) {
    return refuse(n - pos < 4 + (uint64_t)BAM_FIXED ? "the stream ends inside a record's fixed part (truncated)" : "the stream ends inside a record (truncated)");
  }
  return 0;
}

// the name as the FASTQ reader would take it from the twin's header line: up to the NUL, cut at the first whitespace
inline uint32_t
bam_id_len(const uint8_t* name, uint32_t l_read_name)
{
  uint32_t k = 0;
  while (k + 1 < l_read_name && name[k] != 0 && name[k] != ' ' && !(name[k] >= 9 && name[k] <= 13)) {
    ++k;
  }
  return k;
}

// bases [from, from + n) of a record's 4-bit codes as text
inline void
bam_decode_bases(const uint8_t* seq4, uint64_t from, uint64_t n, char* out)
{
  static const char code[17] = "=ACMGRSVTWYHKDBN";
  for (uint64_t j = 0; j < n; ++j) {
    const uint64_t b = from + j;
    const uint8_t v = seq4[b >> 1];
    out[j] = code[(b & 1) ? (v & 15u) : (v >> 4)];
  }
}

// n raw Phred bytes as FASTQ characters; false: one of them has none (0xFF: the qualities are absent; above 93)
inline bool
bam_decode_quals(const uint8_t* qual, uint64_t n, char* out)
{
  bool ok = true;
  for (uint64_t j = 0; j < n; ++j) {
    ok = ok && qual[j] <= BAM_MAX_QUAL;
    out[j] = (char)(qual[j] + 33);
  }
  return ok;
}

// The same of a reverse-strand record as the aligned twin has it: twin bases [from, from + n) — twin base j is the
// complement of stored base l_seq-1-j, and the complement of a 4-bit code is its bit reversal ('=' stays; A<->T, C<->G,
// M<->K, R<->Y, V<->B, H<->D; S, W and N stay)
inline void
bam_decode_bases_rev(const uint8_t* seq4, uint64_t l_seq, uint64_t from, uint64_t n, char* out)
{
  static const char comp[17] = "=TGKCYSBAWRDMHVN";
  for (uint64_t j = 0; j < n; ++j) {
    const uint64_t b = l_seq - 1 - (from + j);
    const uint8_t v = seq4[b >> 1];
    out[j] = comp[(b & 1) ? (v & 15u) : (v >> 4)];
  }
}

// ... and twin qualities [from, from + n): quality j = qual[l_seq-1-j] + 33 (`qual`: the record's first quality byte)
inline bool
bam_decode_quals_rev(const uint8_t* qual, uint64_t l_seq, uint64_t from, uint64_t n, char* out)
{
  bool ok = true;
  for (uint64_t j = 0; j < n; ++j) {
    const uint8_t q = qual[l_seq - 1 - (from + j)];
    ok = ok && q <= BAM_MAX_QUAL;
    out[j] = (char)(q + 33);
  }
  return ok;
}

// ---- the word functions of the device's pack (grp_ingest.inc: k_bam_pack), written so that they compile for the host too
// 16 bases of 4-bit codes (8 bytes, the first base in the high half of the first byte) as a word of grp_reads: 1, 2, 4, 8
// -> 0, 1, 2, 3, base j at bits 2j
GR_BAM_HD inline uint32_t
bam_pack16(uint64_t x)
{
  const uint64_t c = ((x >> 1) & 0x7777777777777777ull) - ((x >> 3) & 0x1111111111111111ull); // per code: 1, 2, 4, 8 -> 0, 1, 2, 3 (never a borrow: n >> 1 >= n >> 3)
  uint64_t t = ((c >> 4) & 0x0303030303030303ull) | ((c & 0x0303030303030303ull) << 2);      // per byte: its two bases in the low four bits
  t = (t | (t >> 4)) & 0x00FF00FF00FF00FFull;
  t = (t | (t >> 8)) & 0x0000FFFF0000FFFFull;
  return (uint32_t)(t | (t >> 16));
}

// 16 codes that begin at the LOW half of a byte (an odd base index): x = the 8 bytes from that byte on, b8 = the ninth
// -> the 8 bytes bam_pack16 takes, the first code in the high half of the first
GR_BAM_HD inline uint64_t
bam_shift_nibble(uint64_t x, uint8_t b8)
{
  const uint64_t y = (x >> 8) | ((uint64_t)b8 << 56);
  return ((x & 0x0F0F0F0F0F0F0F0Full) << 4) | ((y >> 4) & 0x0F0F0F0F0F0F0F0Full);
}

// A packed word of `cnt` stored bases (base i at bits 2i) as the word of the reversed read: base j = 3 - stored base
// cnt-1-j (A0 C1 G2 T3: the complement is the bitwise not), the bits behind base cnt-1 zero
GR_BAM_HD inline uint32_t
bam_revcomp16(uint32_t v, uint32_t cnt)
{
  uint32_t r = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2); // the sixteen 2-bit groups in reverse order
  r = ((r >> 4) & 0x0F0F0F0Fu) | ((r & 0x0F0F0F0Fu) << 4);
  r = __builtin_bswap32(r);
  r = ~r;
  if (cnt < 16u) {
    r = (r >> (2u * (16u - cnt))) & ((1u << (2u * cnt)) - 1u); // (cnt >= 1)
  }
  return r;
}

} // namespace gr
