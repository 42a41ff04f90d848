// Unaligned BAM (SAM specification §4): the record layer behind the BGZF container.  A BAM stream is a header
// ("BAM\1", l_text, text, n_ref, n_ref x {l_name, name, l_ref}) and then records, each a 4-byte block_size followed by
// that many bytes: 32 fixed bytes, the NUL-terminated read name, the CIGAR, the bases as 4-bit codes (high nibble
// first), the qualities as raw Phred bytes, tags.  The program reads such a file as its FASTQ twin: per record
//   @<name up to its NUL>\n<bases by "=ACMGRSVTWYHKDBN">\n+\n<qual + 33>\n
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
// Returns 0 when the chain is sound as far as it goes (a record that is not complete ends the walk; with `final`
// such a tail is the truncation error), else -1 with *bad_offset = the refused record and *why = the reason.
template<class Emit>
inline int
bam_walk(const uint8_t* buf, uint64_t n, bool final, uint64_t* consumed, uint64_t* bad_offset, const char** why, Emit&& emit)
{
  uint64_t pos = 0;
  *consumed = 0;
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
    if (rec.flag & BAM_REFUSED_FLAGS) {
      return refuse("a reverse-strand, secondary or supplementary record (flag 0x10 / 0x100 / 0x800): convert the file with samtools fastq");
    }
    rec.seq_off = rec.name_off + rec.l_read_name + 4ull * n_cigar;
    rec.qual_off = rec.seq_off + ((uint64_t)rec.l_seq + 1) / 2;
    rec.end = pos + 4 + (uint64_t)block_size;
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

} // namespace gr
