/*
 * grpath_ingest.h — FASTQ ingest on the GPU: record
 * splitting, read filters' inputs and 2-bit packing for goldrush-path's three
 * passes over the input (phred median goldrush_path.cpp:79-107, bit-vector fill
 * :235-339, classification :1229-1256).  Exported by libgrpath_hip.so.
 *
 * The reference gets its records from btllib::SeqReader (external): id = header
 * up to the first whitespace, 4-line records, sequence case-folded to upper case.
 * Here a chunk of raw FASTQ text is uploaded once and parsed on the device; the
 * host keeps the text for the output files and only receives 56 bytes per record.
 *
 * Exactness of the Phred filter: calc_phred_average (calc_phred_average.cpp:8-43)
 * sums 10^(-Q/10) left to right in double precision and truncates
 * -10*log10(sum/n).  The device performs the SAME left-to-right double sums from
 * a 256-entry table of the host's pow() values (IEEE additions, no reassociation),
 * so the sums are bit-identical; log10 and the truncation stay on the host.
 */
#ifndef GRPATH_INGEST_H
#define GRPATH_INGEST_H

#include "grpath.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grp_fastq grp_fastq; /* a parsed chunk of FASTQ text resident in HBM */

typedef struct
{
  uint64_t id_off;    /* byte offset of the id (after '@') inside the chunk */
  uint64_t seq_off;
  uint64_t qual_off;
  uint32_t id_len;    /* up to the first whitespace of the header */
  uint32_t seq_len;   /* trailing CR / blanks trimmed */
  uint32_t qual_len;
  uint32_t flags;     /* GRP_FQ_NON_ACGT: find_first_not_of("ACGTacgt") != npos (goldrush_path.cpp:293); GRP_FQ_REVERSED */
  double phred_sum;   /* sum_{i<qual_len} 10^(-(q_i-33)/10), left to right */
  double phred_first; /* the same sum after i = qual_len/2 - 1 (0 when never reached) */
} grp_fastq_record;

#define GRP_FQ_NON_ACGT 1u
/* grp_bam_parse_ex with flag 0x10 accepted, a reverse-strand record: the read is the reverse complement of what is stored.
 * seq_off / qual_off still name the stored bytes; phred_sum / phred_first are those of the quality line read backwards;
 * grp_fastq_pack packs the reverse complement. */
#define GRP_FQ_REVERSED 2u

/*
 * Upload and parse `n_bytes` of FASTQ text (host memory; pinned memory — grp_fastq_pin — is faster).
 * final_chunk != 0: the text ends the file (a last line without newline is a line).
 * Returns the number of complete records and how many bytes they span; the caller
 * re-submits the unconsumed tail at the start of its next chunk.  *stopped is set
 * when a record's header does not start with '@' (records before it are returned;
 * the reader ends there, like a reader at end of input).
 */
int grp_fastq_parse(grp_ctx* ctx, const char* text, uint64_t n_bytes, int final_chunk, grp_fastq** out, uint64_t* n_records, uint64_t* bytes_consumed, int* stopped);
/*
 * Optional (round 5): start the upload of a COMING chunk now.  `text` is that chunk's body: the later grp_fastq_parse is
 * given a text that ENDS with exactly these bytes at this address — the body itself, or the body with up to GRP_FASTQ_PREFETCH_FRONT bytes (16 MiB) in front
 * of it (the unconsumed tail of the chunk before, which is only known once that chunk has been parsed); it finds the body on
 * the device and uploads what is in front of it alone.  Up to two prefetches may be pending, parsed in the order they were
 * issued.  Why: the copy of a 256 MiB chunk takes ~5 ms and, issued from inside grp_fastq_parse, only began when the fill
 * of the chunk before had ended (the timeline: tools/dev/r5_ingest_timeline.sh); two chunks ahead it is off the path of
 * every chunk.  The body must stay unchanged until its parse returns.  A prefetch that is not followed by the matching
 * parse is simply dropped (with every prefetch behind it).  GRP_ERR_BUSY: no device buffer is free for it right now (not
 * an error: the parse uploads as before).  (NULL, 0): every pending prefetch is forgotten and its copy waited for — call it
 * before the buffers the bodies live in are freed.
 */
#define GRP_FASTQ_PREFETCH_FRONT (16ull << 20) /* bytes a later parse may put in front of a prefetched body (the engine leaves this much room) */
int grp_fastq_prefetch(grp_ctx* ctx, const char* text, uint64_t n_bytes);
/* copy the record table (n_records entries) to the host */
int grp_fastq_records(grp_fastq* fq, grp_fastq_record* out);
/*
 * 2-bit pack the selected records (ascending indices; they must be pure ACGT) into a
 * read batch that lives on the device — no host packing, no second upload.  The
 * batch is independent of `fq` afterwards.
 */
int grp_fastq_pack(grp_ctx* ctx, grp_fastq* fq, const uint32_t* sel, uint32_t n_sel, grp_reads** out);
void grp_fastq_free(grp_fastq* fq);
/*
 * Optional: page-lock the caller's chunk buffer (hipHostRegister) so that grp_fastq_parse's upload
 * of text inside [buffer, buffer + n_bytes) is one DMA.  One buffer per context; _pin replaces the
 * previous one.  The caller MUST call grp_fastq_unpin (or grp_destroy) BEFORE it frees or
 * reallocates the buffer.  GRP_ERR_HIP: the buffer could not be locked — parse works all the same.
 */
int grp_fastq_pin(grp_ctx* ctx, const char* buffer, uint64_t n_bytes);
int grp_fastq_unpin(grp_ctx* ctx);

/*
 * ---- BGZF-compressed FASTQ: the inflate in front of the ingest ------------------------------------------------
 * A BGZF file (what bgzip and the htslib tools write) is a series of independent gzip members of at most 64 KiB of
 * text, each of which says its compressed size in its header: the members of a chunk are inflated side by side on the
 * device (csrc/grp_inflate.inc: one wave per member, a complete RFC 1951 decoder; then the CRC32 of every member's
 * text), where one zlib thread inflates a plain gzip stream serially.  The caller finds the members (the host's
 * gr_bgzf_scan) and hands over their table; the text comes back to host memory, where it is FASTQ text like any other
 * (grp_fastq_prefetch / grp_fastq_parse).
 */
struct grp_bgzf_block
{
  uint64_t comp_off;  /* first byte of the member's DEFLATE payload inside `comp` */
  uint32_t comp_len;  /* payload bytes (BSIZE + 1 - 12 - XLEN - 8) */
  uint32_t text_len;  /* ISIZE of the member's trailer, <= 65536 */
  uint32_t crc32;     /* CRC32 of the trailer */
  uint32_t reserved;
}; /* (the typedef is in grpath.h, which lists every function the engine exports) */

/* Inflate n_blocks independent raw-DEFLATE payloads on the device; the text of block i goes to
 * text_out + sum(text_len[0..i)).  Synchronous.  GRP_ERR_INVALID with *bad_block = the first block that
 * is not a valid stream of exactly text_len bytes with that CRC32 (and a reason in grp_last_error); text_out
 * is then unspecified.  The table is checked before anything is launched (ranges inside comp, text_len <= 65536, the
 * sum of the texts <= text_cap: GRP_ERR_INVALID, *bad_block = the entry).  Pinned memory (grp_fastq_pin) makes both
 * copies one DMA each.  The work runs on the side stream: a fill queued on the main stream keeps running beside it.
 * Same threading / stream rules as grp_fastq_parse. */
int grp_bgzf_inflate(grp_ctx* ctx, const uint8_t* comp, uint64_t n_comp, const grp_bgzf_block* blocks, uint32_t n_blocks, char* text_out, uint64_t text_cap, uint32_t* bad_block);
/* blocks, compressed bytes, text bytes, kernel microseconds (HIP events around the two kernels) since grp_create */
int grp_debug_bgzf_stats(const grp_ctx* ctx, uint64_t out[4]);

/*
 * ---- plain gzip FASTQ: segments of a serial stream ---------------------------------------------------------------
 * An ordinary .gz file is one serial DEFLATE stream (per member) with no block table: only a pass through zlib finds its
 * block boundaries.  The host's first pass over such a file goes through zlib anyway and writes down exact restart
 * points in the manner of zlib's zran example (csrc/host/gr_gzidx.hpp): a block boundary with its bit position, the up to
 * 32 KiB of text in front of it and the CRC32 of the text up to the next point.  Every later pass then has a table of
 * independent segments, as a BGZF file has a table of members, and the same decoder inflates them one wave per segment.
 * A segment differs from a member in that it starts at a bit, starts with a history, ends at a block boundary that need
 * not follow a final block, and may hold any amount of text.
 */
struct grp_gzip_segment
{
  uint64_t comp_bit;   /* first bit of the segment inside `comp` (bit 0 = LSB of byte 0) */
  uint64_t n_bits;     /* its length; it ends on a block boundary */
  uint64_t dict_off;   /* its history inside `dict` */
  uint32_t dict_len;   /* 0 .. 32768 */
  uint32_t text_len;
  uint32_t crc32;      /* of its text_len bytes of text */
  uint32_t flags;      /* 1: the segment ends with a member's final block */
}; /* (the typedef is in grpath.h) */
#define GRP_GZIP_SEG_FINAL 1u

/* Inflate n_segs segments on the device; the text of segment i goes to text_out + sum(text_len[0..i)).  The contract of
 * grp_bgzf_inflate: synchronous, on the side stream; the table is checked before anything is launched (the bits inside
 * comp, the history inside dict, dict_len <= 32768, no flag but 1, the sum of the texts <= text_cap: GRP_ERR_INVALID,
 * *bad_seg = the entry); every segment that is not exactly text_len bytes of valid DEFLATE with that CRC32 — whole blocks
 * that consume exactly n_bits, the last of them a final block if and only if flag 1 is set, no distance that reaches in
 * front of the history — is refused: GRP_ERR_INVALID, *bad_seg = the first such segment, the reason in grp_last_error,
 * text_out unspecified.  At most 4 GiB of compressed bytes, 4 GiB of histories and 2^22 segments per call. */
int grp_gzip_inflate(grp_ctx* ctx, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_segment* segs, uint32_t n_segs, char* text_out, uint64_t text_cap, uint32_t* bad_seg);
/* segments, compressed bytes, text bytes, kernel microseconds (HIP events around the two kernels) since grp_create */
int grp_debug_gzip_stats(const grp_ctx* ctx, uint64_t out[4]);

/*
 * ---- plain gzip FASTQ, many files: the restart points found on the device ---------------------------------------------
 * One gzip stream is serial, but every FILE's first member starts at a known bit behind its header, with no history, and
 * where a block ends is known the moment the decoder gets there.  grp_gzip_walk takes one step in each of many streams
 * side by side, one wave per step (csrc/grp_inflate.inc: the open form of the decoder): from a bit where a block begins,
 * with the history in front of it, whole blocks until at least min_text bytes of text have come out or a final block has
 * ended.  The host (csrc/host/gr_gzwalk.hpp) parses the headers and trailers, strings the steps of a file together and
 * writes down the index GzIndexReader would have written.  Nothing guessed enters the index: a step starts behind a header
 * the host parsed or at a boundary the step in front of it reached, and what the steps of a stream produced is taken only
 * if the chain of members from byte 0 of the file arrives at exactly that header — where the serial walk would have begun
 * too, with the same empty state and the same decoder.  With GRP_GZIP_WALK_MEMBERS=on the host also begins streams at gzip
 * headers it finds behind a file's first member, ahead of that chain; one the chain never arrives at is thrown away, so a
 * step may start at bits that begin no DEFLATE stream: it ends with a status and touches nothing outside its buffers.
 * The text is decoded to find the boundaries and thrown away.
 */
struct grp_gzip_walk_step
{
  uint64_t comp_bit;   /* the step's first bit inside `comp` (`comp` starts on a byte of the file: a stored block aligns to it) */
  uint64_t n_bits;     /* the bits there are from comp_bit on: the step consumes what its blocks take of them */
  uint64_t dict_off;   /* its history inside `dict` */
  uint32_t dict_len;   /* 0 .. 32768 */
  uint32_t min_text;   /* it stops behind the first block where at least this much text has come out (or behind a final block) */
  uint32_t room;       /* ... and may produce this much */
  uint32_t reserved;
};
struct grp_gzip_walk_result
{
  uint64_t bits;       /* consumed: comp_bit + bits is the block boundary the step ended at */
  uint32_t text_len;   /* that came out */
  uint32_t crc32;      /* of that text */
  uint32_t final;      /* 1: the boundary lies behind a final block */
  uint32_t status;     /* 0, or why the step did not end at a boundary (GRP_GZIP_WALK_*, else a damaged stream); then the other fields are 0 */
  uint32_t hist_len;   /* min(32768, dict_len + text_len): the last bytes of history and text, the history of the next step */
  uint32_t reserved;
}; /* (the typedefs are in grpath.h) */
#define GRP_GZIP_WALK_INPUT_ENDS 3u /* n_bits ended inside a block, or in front of the next one: the step needs more compressed bytes */
#define GRP_GZIP_WALK_NO_ROOM 19u   /* the text of the step's blocks does not fit `room` */

/* One step in each of n_steps streams.  results[i] is step i's answer; hist_out + 32768 * i receives its hist_len bytes of
 * new history (host memory, 32768 * n_steps bytes); text_out, if not NULL, the text of step i at the sum of the ROOMS in
 * front of it (tests; the product passes NULL).  Synchronous, on the side stream, with the threading rules of
 * grp_gzip_inflate.  The whole table is checked before anything is launched (the bits inside comp, the history inside
 * dict, dict_len <= 32768, a reserved field that is not 0, the sum of the rooms <= 2^34 and, with text_out, <= text_cap:
 * GRP_ERR_INVALID, *bad_step = the entry).  A step that ends with a status is NOT a failed call: the status is that
 * step's answer, and the other steps of the call are not touched by it.  grp_gzip_status_text: the words of a status.
 * At most 4 GiB of compressed bytes, 4 GiB of histories and 2^22 steps per call. */
int grp_gzip_walk(grp_ctx* ctx, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n_steps, grp_gzip_walk_result* results, uint8_t* hist_out, char* text_out,
                  uint64_t text_cap, uint32_t* bad_step);
const char* grp_gzip_status_text(uint32_t status);

/*
 * ---- unaligned BAM: records instead of four text lines ---------------------------------------------------------------
 * PacBio and Nanopore deliver long reads as unaligned BAM: a BGZF container (grp_bgzf_inflate turns its members into
 * bytes) around a header and records of 4-bit bases and raw Phred bytes.  The program reads a BAM file as its FASTQ twin
 * — per record "@<read_name up to its NUL>\n<bases by =ACMGRSVTWYHKDBN>\n+\n<qual + 33>\n" — and grp_bam_parse is
 * grp_fastq_parse for such bytes, with its contract:
 *  - `bytes` (host memory; pinned is faster) begins at a record: the caller has skipped the BAM header.  Only complete
 *    records are consumed; the caller re-submits the tail.  final_chunk with bytes left over is a truncation error.
 *  - The record chain is walked on the host side of the call (a pointer chase of 4-byte reads over bytes that are in host
 *    memory; csrc/host/gr_bam.hpp, the one walk the host library uses too); the record table, the ACGT test over the
 *    4-bit codes, the quality range test, the Phred sums and the pack run on the device.
 *  - Refused, with GRP_ERR_INVALID, *bad_offset = the record's offset from `bytes` and the reason in grp_last_error:
 *    a block_size smaller than 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq, l_read_name 0, a name that does
 *    not end in NUL, flag 0x10 / 0x100 / 0x800 (convert with samtools fastq), qualities that are absent (0xFF) or above
 *    93 where l_seq > 0, and a stream that ends inside a record.  Nothing is returned then.
 *  - Not refused: l_seq 0, any n_cigar_op and tags (skipped by block_size), paired-end flags, a non-zero padding code
 *    behind an odd l_seq (it does not set GRP_FQ_NON_ACGT), a code other than A, C, G, T (it does).
 *  - The handle is served by grp_fastq_prefetch / _pin / _records / _pack / _free unchanged.  Offsets of the table count
 *    from `bytes`: id_off / id_len = the name without its NUL, cut at a whitespace; seq_off = the first byte of the
 *    4-bit bases (high half first), seq_len = l_seq; qual_off = the first raw quality byte, qual_len = l_seq.
 *    phred_sum / phred_first are the same left-to-right double sums, bit-identical to those of the twin's quality line.
 */
int grp_bam_parse(grp_ctx* ctx, const char* bytes, uint64_t n_bytes, int final_chunk, grp_fastq** out, uint64_t* n_records, uint64_t* bytes_consumed, uint64_t* bad_offset);
/*
 * The same for an ALIGNED BAM file, read as the FASTQ that `samtools fastq -n` writes for it with its default filters
 * (the aligned twin; written down from the SAM specification and samtools' documented behaviour, not pinned against
 * samtools' output).  `accept` is a subset of 0x910 (any other bit: GRP_ERR_INVALID); grp_bam_parse is the call with
 * accept 0.  A record with a flag bit of 0x910 that is not in `accept` is refused as above.
 *  - An accepted 0x100 / 0x800 (secondary, supplementary): the record is no read of the twin.  Its structural fields are
 *    checked like any record's (the chain runs through it), it is consumed and counted in *n_skipped, its bases and
 *    qualities are not looked at (0xFF qualities are fine) and it has no entry in the table.  A chunk may so consume bytes
 *    and return no record.
 *  - An accepted 0x10, and neither of the above: the entry has GRP_FQ_REVERSED.  The read is the complement of stored base
 *    l_seq-1-j at base j (the complement of a 4-bit code is its bit reversal) with quality qual[l_seq-1-j] + 33.
 *    seq_off / qual_off name the stored bytes; GRP_FQ_NON_ACGT does not depend on the order; phred_sum is the
 *    right-to-left sum over the stored bytes and phred_first that sum after the stored bytes l_seq-1 ... l_seq - l_seq/2,
 *    the same additions in the same order as the left-to-right sums of the twin's line: bit-identical to them.
 *    grp_fastq_pack packs such a record as the twin's read.
 *  - Every other record, flag 0x4 or paired-end flags included, is read as by grp_bam_parse.
 */
int grp_bam_parse_ex(grp_ctx* ctx, const char* bytes, uint64_t n_bytes, int final_chunk, uint32_t accept, grp_fastq** out, uint64_t* n_records, uint64_t* bytes_consumed, uint64_t* bad_offset, uint64_t* n_skipped);

/*
 * ---- records of a compressed input, fetched and formatted on the device ----------------------------------------------
 * What the host program writes for an inserted read (goldrush_path.cpp:996-1002, 1055-1070) is
 *     <'@' | '>'> id <"_untrimmed\n" | "_trimmed\n"> bases of the written slice '\n'   [ "+\n" qualities of the slice '\n' ]
 * and the record's text is all it needs of the input.  For a compressed input that text lies inside a few inflatable units
 * (BGZF members, or the segments of a plain gzip file's index): grp_records_fetch inflates those units into device memory
 * and checks their CRC32 as grp_bgzf_inflate / grp_gzip_inflate do, leaves the text there, and emits only the records —
 * formatted, with the Phred sum of each written quality slice — so that neither the text around them nor the records' own
 * text is copied down and formatted by the host.
 *
 * All offsets of a record count in the CONCATENATED text of the call's units (unit i's text begins at the sum of the
 * text_len in front of it); a record may straddle any number of units.
 */
struct grp_fetch_record
{
  uint64_t id_off;    /* the id: text[id_off, id_off + id_len) */
  uint64_t seq_off;   /* the record's first base (BAM: the first byte of its 4-bit codes, high half first) */
  uint64_t qual_off;  /* the record's first quality (FASTQ text: the character; BAM: the raw Phred byte) */
  uint64_t out_off;   /* where the record's bytes go in `out` */
  uint32_t id_len;
  uint32_t seq_from;  /* the written slice: first base written, counted from seq_off in BASES ... */
  uint32_t n_seq;     /* ... and how many */
  uint32_t qual_from; /* first quality written, counted from qual_off ... */
  uint32_t n_qual;    /* ... and how many (ignored for the output without GRP_FETCH_FASTQ; the sum covers them all the same) */
  uint32_t flags;     /* GRP_FETCH_REC_TRIMMED: the id gets "_trimmed", else "_untrimmed"; GRP_FETCH_REC_REVERSED */
}; /* (the typedef is in grpath.h) */
#define GRP_FETCH_REC_TRIMMED 1u
/* With GRP_FETCH_BAM only (without it the flag is refused like any unknown one): a reverse-strand record of an aligned BAM
 * file.  seq_from / n_seq and qual_from / n_qual name the STORED range (the caller computes l_seq - from - n of the twin's
 * slice); it is written last element first, the bases complemented, the qualities + 33, and the sum is that of the
 * written quality characters left to right: the right-to-left chain over the stored bytes. */
#define GRP_FETCH_REC_REVERSED 2u
/* unit_kind: what `units` points at */
#define GRP_FETCH_UNITS_BGZF 0 /* grp_bgzf_block[]; dict is not looked at */
#define GRP_FETCH_UNITS_GZIP 1 /* grp_gzip_segment[] with their histories in dict */
/* out_flags */
#define GRP_FETCH_FASTQ 1u /* '@', and "+\n" with the quality line; without it '>' and no quality lines (FASTA) */
#define GRP_FETCH_BAM 2u   /* the text is BAM: bases through =ACMGRSVTWYHKDBN from any base index, qualities + 33 */
/*
 * The bytes of record r go to out[out_off, out_off + size), size = 1 + id_len + (trimmed ? 9 : 11) + n_seq + 1, and with
 * GRP_FETCH_FASTQ + 2 + n_qual + 1 more; no other byte of `out` is written.  FASTQ text: a-z of the bases folded to upper
 * case, every other byte as it is.  sums[r] = the left-to-right double sum of 10^(-Q/10) over the written quality slice,
 * with the table the ingest uses for the format: bit-identical to the host's gr_sum_phred of the written quality characters
 * (computed without GRP_FETCH_FASTQ too).
 * Synchronous, on the side stream, with the threading rules of grp_bgzf_inflate.  Both tables are checked before anything
 * is launched: the units as grp_bgzf_inflate / grp_gzip_inflate check theirs (GRP_ERR_INVALID, *bad_unit = the entry); of a
 * record the id, the bases' and the qualities' ranges inside the units' text, no flag but GRP_FETCH_REC_TRIMMED (and, with
 * GRP_FETCH_BAM, GRP_FETCH_REC_REVERSED), its output
 * range inside out_cap and disjoint from every other record's (GRP_ERR_INVALID, *bad_record = the entry; of two
 * overlapping records the one that begins later).  A unit that is not a valid stream with its CRC32 is refused as by
 * grp_bgzf_inflate (*bad_unit); `out` and `sums` are then untouched.  The call relies on no padding behind the text or
 * behind `out`.  `out` is host memory (page-locked memory makes its copies DMA), `sums` has one double per record.
 * At most 2^22 units and 2^22 records per call.
 */
int grp_records_fetch(grp_ctx* ctx, int unit_kind, const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const void* units, uint32_t n_units, const grp_fetch_record* recs, uint32_t n_recs, uint32_t out_flags,
                      char* out, uint64_t out_cap, double* sums, uint32_t* bad_unit, uint32_t* bad_record);

#ifdef __cplusplus
}
#endif
#endif
