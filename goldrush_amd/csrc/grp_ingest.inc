// FASTQ ingest on the GPU (include/grpath_ingest.h).  Included at the end of
// grpath_hip.hip (same translation unit: uses grp_ctx, reads_build, set_err).
//
//   k_nl_count / k_nl_scatter   newline positions of the chunk (count, scan, scatter)
//   k_fq_records                one wave per record: line extents, id length, ACGT
//                               check (ballot)
//   k_fq_phred                  one lane per record: left-to-right double Phred sums
//   k_fq_pack                   2 bits per base for the selected records
//   k_bam_records / k_bam_pack  the same table and the same packed words from BAM records
//                               (grp_bam_parse[_ex]: the record chain is walked on the host, host/gr_bam.hpp); a
//                               reverse-strand record of an aligned file is summed and packed backwards

#include "../../include/grpath_ingest.h"

#include <cmath>

namespace {

constexpr uint32_t NL_BYTES_PER_THREAD = 16;
constexpr uint32_t NL_BLOCK_BYTES = THREADS * NL_BYTES_PER_THREAD;
constexpr uint32_t FQ_BAD_HEADER = 0x80000000u;
constexpr uint64_t FQ_FRONT = GRP_FASTQ_PREFETCH_FRONT; // room in front of a prefetched body for the tail of the chunk before it (a multiple of 16; grpath_ingest.h: the caller's carried tail may be this long)

// `lead` (< 16): bytes in front of the text inside its first 16-byte group — the text of a chunk whose body was uploaded before the
// length of what goes in front of it was known begins wherever that leaves it (grp_fastq_prefetch); they are not text
__device__ inline uint32_t
count_nl16(const uint8_t* __restrict__ text, uint64_t base, uint64_t n, uint32_t lead)
{
  uint32_t c = 0;
  if (base + NL_BYTES_PER_THREAD <= n && base >= lead) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + base); // base is 16-byte aligned
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        c += ((w[i] >> (8 * b)) & 0xFFu) == 0x0Au;
      }
    }
  } else {
    const uint64_t end = (base + NL_BYTES_PER_THREAD < n) ? base + NL_BYTES_PER_THREAD : n;
    for (uint64_t i = (base < lead) ? lead : base; i < end; ++i) {
      c += text[i] == 0x0A;
    }
  }
  return c;
}

__global__ void __launch_bounds__(THREADS)
k_nl_count(const uint8_t* __restrict__ text, uint64_t n, uint32_t lead, uint32_t* __restrict__ block_counts)
{
  __shared__ uint32_t sW[THREADS / 64];
  const uint64_t base = (uint64_t)blockIdx.x * NL_BLOCK_BYTES + (uint64_t)threadIdx.x * NL_BYTES_PER_THREAD;
  uint32_t c = (base < n) ? count_nl16(text, base, n, lead) : 0u;
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    sW[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
      t += sW[w];
    }
    block_counts[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(THREADS)
k_nl_scatter(const uint8_t* __restrict__ text, uint64_t n, uint32_t lead, const uint64_t* __restrict__ block_base, uint64_t* __restrict__ nl_pos)
{
  __shared__ uint32_t sScan[THREADS];
  const uint64_t base = (uint64_t)blockIdx.x * NL_BLOCK_BYTES + (uint64_t)threadIdx.x * NL_BYTES_PER_THREAD;
  const uint32_t c = (base < n) ? count_nl16(text, base, n, lead) : 0u;
  sScan[threadIdx.x] = c;
  __syncthreads();
  for (uint32_t o = 1; o < THREADS; o <<= 1) {
    uint32_t t = (threadIdx.x >= o) ? sScan[threadIdx.x - o] : 0;
    __syncthreads();
    sScan[threadIdx.x] += t;
    __syncthreads();
  }
  uint64_t out = block_base[blockIdx.x] + sScan[threadIdx.x] - c;
  if (c) {
    const uint64_t end = (base + NL_BYTES_PER_THREAD < n) ? base + NL_BYTES_PER_THREAD : n;
    for (uint64_t i = (base < lead) ? lead : base; i < end; ++i) {
      if (text[i] == 0x0A) {
        nl_pos[out++] = i;
      }
    }
  }
}

// rtrim of CR / blank / tab, like the host reader
__device__ inline uint64_t
rtrim_end(const uint8_t* __restrict__ text, uint64_t s, uint64_t e)
{
  while (e > s && (text[e - 1] == '\r' || text[e - 1] == ' ' || text[e - 1] == '\t')) {
    --e;
  }
  return e;
}

// all 16 bytes of a group are A / C / G / T in either case?  (goldrush_path.cpp:293 find_first_not_of("ACGTacgt"))
__device__ inline bool
acgt16(uint4 v)
{
  const uint32_t w[4] = { v.x, v.y, v.z, v.w };
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t ch = (w[i] >> (8 * b)) & 0xDFu; // fold case
      ok = ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
    }
  }
  return ok;
}

// one wave per record; offsets in the records count from `text` (the caller takes `lead` off)
__global__ void __launch_bounds__(THREADS)
k_fq_records(const uint8_t* __restrict__ text, const uint64_t* __restrict__ nl_pos, uint64_t n_records, uint32_t lead, grp_fastq_record* __restrict__ out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (r >= n_records) {
    return;
  }
  uint64_t ls[4], le[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t li = 4 * r + i;
    ls[i] = (li == 0) ? lead : nl_pos[li - 1] + 1;
    le[i] = rtrim_end(text, ls[i], nl_pos[li]);
  }
  grp_fastq_record rec;
  rec.flags = 0;
  if (le[0] == ls[0] || text[ls[0]] != '@') {
    rec.flags |= FQ_BAD_HEADER;
  }
  // id = header after '@' up to the first whitespace
  uint64_t ie = ls[0] + 1;
  while (ie < le[0]) {
    const uint8_t ch = text[ie];
    if (ch == ' ' || (ch >= 9 && ch <= 13)) {
      break;
    }
    ++ie;
  }
  rec.id_off = ls[0] + 1;
  rec.id_len = (le[0] > ls[0]) ? (uint32_t)(ie - ls[0] - 1) : 0u;
  rec.seq_off = ls[1];
  rec.seq_len = (uint32_t)(le[1] - ls[1]);
  rec.qual_off = ls[3];
  rec.qual_len = (uint32_t)(le[3] - ls[3]);
  // the ACGT test, 16 bases per lane and load (round 5: one base per lane and load was 1.9 ms per 256 MiB chunk)
  bool bad = false;
  {
    const uint64_t s0 = ls[1], e0 = le[1];
    const uint64_t a0 = (s0 + 15u) & ~(uint64_t)15, a1 = e0 & ~(uint64_t)15; // the aligned middle [a0, a1)
    if (a0 < a1) {
      for (uint64_t b = s0 + lane; b < a0; b += 64) {
        const uint8_t ch = text[b] & 0xDFu;
        bad = bad || !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      }
      for (uint64_t b = a0 + (uint64_t)lane * 16u; b < a1; b += 64u * 16u) {
        bad = bad || !acgt16(*reinterpret_cast<const uint4*>(text + b));
      }
      for (uint64_t b = a1 + lane; b < e0; b += 64) {
        const uint8_t ch = text[b] & 0xDFu;
        bad = bad || !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      }
    } else {
      for (uint64_t b = s0 + lane; b < e0; b += 64) {
        const uint8_t ch = text[b] & 0xDFu;
        bad = bad || !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      }
    }
  }
  if (__ballot(bad) != 0ull) {
    rec.flags |= GRP_FQ_NON_ACGT;
  }
  // (the Phred sums: k_fq_phred, one lane per record)
  rec.phred_sum = 0.0;
  rec.phred_first = 0.0;
  if (lane == 0) {
    out[r] = rec;
  }
}

// calc_phred_average.cpp:15-30: strictly left-to-right double sums, total and the sum after i = n/2 - 1.  A sum is a chain
// of dependent additions: a wave per record spent 64 lanes' issue slots on ONE chain (4.1 ms per 256 MiB chunk: a third of
// the ingest pass's device time); here a lane owns a record and a wave runs 64 chains.  The qualities are read as aligned
// 8-byte words, 10^(-(q-33)/10) comes from the table in LDS.
__device__ inline double
phred_chain(const uint8_t* __restrict__ q, uint32_t from, uint32_t to, double total, const double* sTab)
{
  uint32_t i = from;
  while (i < to && ((uintptr_t)(q + i) & 15u)) {
    total += sTab[q[i]];
    ++i;
  }
  // 64 bytes (one line) per step, the NEXT step's line requested before this step's additions: a lane reads its own
  // record, so every load is a line of its own and its latency — not the additions — was what a record cost
  // (3 000 dependent-looking 8-byte loads per 25 kb record: 1.9 ms per chunk beside the fill)
  if (i + 64 <= to) {
    const uint4* p = reinterpret_cast<const uint4*>(q + i);
    uint4 cur[4] = { p[0], p[1], p[2], p[3] };
    for (;;) {
      const bool more = i + 128 <= to;
      uint4 nxt[4];
      if (more) {
        nxt[0] = p[4];
        nxt[1] = p[5];
        nxt[2] = p[6];
        nxt[3] = p[7];
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t w[4] = { cur[v].x, cur[v].y, cur[v].z, cur[v].w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            total += sTab[(w[k] >> (8 * b)) & 0xFFu];
          }
        }
      }
      i += 64;
      if (!more) {
        break;
      }
      p += 4;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        cur[v] = nxt[v];
      }
    }
  }
  for (; i < to; ++i) {
    total += sTab[q[i]];
  }
  return total;
}

// The same chain from the other end: q[to - 1], q[to - 2] ... q[from], in that order — the left-to-right chain of a line
// that is read backwards (a reverse-strand BAM record, GRP_FQ_REVERSED).  The same table, the same additions, the same
// structure: single bytes down to a 16-byte boundary, lines of 64 bytes downwards with the line below requested ahead,
// single bytes for what is left.  No load leaves q[from, to).
__device__ inline double
phred_chain_back(const uint8_t* __restrict__ q, uint32_t from, uint32_t to, double total, const double* sTab)
{
  uint32_t i = to; // what is left is q[from, i)
  while (i > from && ((uintptr_t)(q + i) & 15u)) {
    --i;
    total += sTab[q[i]];
  }
  if (i - from >= 64) {
    const uint4* p = reinterpret_cast<const uint4*>(q + i) - 4; // the line q[i - 64, i)
    uint4 cur[4] = { p[0], p[1], p[2], p[3] };
    for (;;) {
      const bool more = i - from >= 128;
      uint4 nxt[4];
      if (more) {
        nxt[0] = p[-4];
        nxt[1] = p[-3];
        nxt[2] = p[-2];
        nxt[3] = p[-1];
      }
#pragma unroll
      for (int v = 3; v >= 0; --v) {
        const uint32_t w[4] = { cur[v].x, cur[v].y, cur[v].z, cur[v].w };
#pragma unroll
        for (int k = 3; k >= 0; --k) {
#pragma unroll
          for (int b = 3; b >= 0; --b) {
            total += sTab[(w[k] >> (8 * b)) & 0xFFu];
          }
        }
      }
      i -= 64;
      if (!more) {
        break;
      }
      p -= 4;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        cur[v] = nxt[v];
      }
    }
  }
  while (i > from) {
    --i;
    total += sTab[q[i]];
  }
  return total;
}

// REV: records with GRP_FQ_REVERSED (k_bam_records, where flag 0x10 is accepted) get the sums of the line read backwards
template <bool REV>
__global__ void __launch_bounds__(64)
k_fq_phred(const uint8_t* __restrict__ text, uint64_t n_records, const double* __restrict__ delog, grp_fastq_record* __restrict__ recs)
{
  __shared__ double sTab[256];
  for (uint32_t i = threadIdx.x; i < 256; i += 64) {
    sTab[i] = delog[i];
  }
  __syncthreads();
  const uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= n_records) {
    return;
  }
  const uint8_t* q = text + recs[r].qual_off;
  const uint32_t qn = recs[r].qual_len;
  double first = 0.0, total = 0.0;
  if (REV && (recs[r].flags & GRP_FQ_REVERSED)) {
    // the twin's line is q read backwards: its first half (n/2 qualities) is the stored bytes qn-1 ... qn - qn/2
    if (qn >= 2) {
      first = phred_chain_back(q, qn - qn / 2, qn, 0.0, sTab);
      total = phred_chain_back(q, 0, qn - qn / 2, first, sTab);
    } else {
      total = phred_chain_back(q, 0, qn, 0.0, sTab);
    }
  } else if (qn >= 2) { // (the reference's n/2 - 1 wraps for n < 2: its "first" sum is never taken)
    const uint32_t half = qn / 2 - 1;
    first = phred_chain(q, 0, half + 1, 0.0, sTab);
    total = phred_chain(q, half + 1, qn, first, sTab);
  } else {
    total = phred_chain(q, 0, qn, 0.0, sTab);
  }
  recs[r].phred_sum = total;
  recs[r].phred_first = first;
}

// Small transfers of a parse as KERNELS over page-locked, device-mapped host memory instead of copies (round 5): a copy of a few
// bytes is queued on the same DMA engine as the 256 MiB body of the chunk after next and waited up to 5 ms for it — the tail
// of the chunk before on its way up, the line count and the record table on their way down.
__global__ void __launch_bounds__(THREADS)
k_ing_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n)
{
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS) {
    dst[i] = src[i];
  }
}

__global__ void __launch_bounds__(THREADS)
k_ing_words(unsigned long long* __restrict__ dst_host, const unsigned long long* __restrict__ src, uint64_t n)
{
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS) {
    __hip_atomic_store(dst_host + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// A0 C1 G2 T3 from the ASCII code (either case): (c>>1)&3 gives A0 C1 G3 T2
__device__ inline uint32_t
base_code(uint8_t ch)
{
  const uint32_t x = (ch >> 1) & 3u;
  return x ^ (x >> 1);
}

// one workgroup per selected record
__global__ void __launch_bounds__(THREADS)
k_fq_pack(const uint8_t* __restrict__ text, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ len, const uint64_t* __restrict__ word_off, uint32_t* __restrict__ packed)
{
  const uint32_t r = blockIdx.x;
  const uint64_t so = seq_off[r];
  const uint32_t n = len[r];
  const uint32_t nw = (n + 15u) / 16u;
  uint32_t* dst = packed + word_off[r];
  for (uint32_t w = threadIdx.x; w < nw; w += THREADS) {
    uint32_t v = 0;
    const uint32_t b0 = w * 16u;
    const uint32_t cnt = min(16u, n - b0);
    for (uint32_t j = 0; j < cnt; ++j) {
      v |= base_code(text[so + b0 + j]) << (2u * j);
    }
    dst[w] = v;
  }
}

// ---- unaligned BAM records (host/gr_bam.hpp) ---------------------------------------------------------------------------
// The host has walked the record chain (a pointer chase of 4-byte reads: one lane's work, and the bytes are in host
// memory) and checked every record's fields against its block: these kernels take a record's offset and trust its fixed
// part.  Every load lies inside the record's own name, bases or qualities, at whatever alignment the name left them.
constexpr uint32_t BAM_BAD_QUAL = 0x40000000u; // a quality byte above 93 (0xFF: absent): no FASTQ character

// all eight 4-bit codes of a word are A, C, G or T (1, 2, 4, 8: one bit set)?
__device__ inline bool
bam_acgt8(uint32_t x)
{
  uint32_t p = x - ((x >> 1) & 0x55555555u);
  p = (p & 0x33333333u) + ((p >> 2) & 0x33333333u); // bits set, per code
  return p == 0x11111111u;
}

// one of the four bytes of a word is above 93?
__device__ inline bool
bam_qual4_bad(uint32_t x)
{
  return ((((x & 0x7F7F7F7Fu) + 0x22222222u) | x) & 0x80808080u) != 0u; // (94 + 0x22 = 0x80; no carry between bytes)
}

// this lane's share of a test over the bytes [s0, e0): 16 bytes per lane and load over the aligned middle (as k_fq_records'
// ACGT test), single bytes in front of it and behind it
template<class ByteBad, class WordBad>
__device__ inline bool
bam_scan_bad(const uint8_t* __restrict__ text, uint64_t s0, uint64_t e0, uint32_t lane, ByteBad byte_bad, WordBad word_bad)
{
  bool bad = false;
  const uint64_t a0 = (s0 + 15u) & ~(uint64_t)15, a1 = e0 & ~(uint64_t)15; // the aligned middle [a0, a1)
  if (a0 < a1) {
    for (uint64_t b = s0 + lane; b < a0; b += 64) {
      bad = bad || byte_bad(text[b]);
    }
    for (uint64_t b = a0 + (uint64_t)lane * 16u; b < a1; b += 64u * 16u) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + b);
      bad = bad || word_bad(v.x) || word_bad(v.y) || word_bad(v.z) || word_bad(v.w);
    }
    for (uint64_t b = a1 + lane; b < e0; b += 64) {
      bad = bad || byte_bad(text[b]);
    }
  } else {
    for (uint64_t b = s0 + lane; b < e0; b += 64) {
      bad = bad || byte_bad(text[b]);
    }
  }
  return bad;
}

// one wave per record: the table entry from the fixed 32 bytes, the name's length, the ACGT test over the 4-bit codes and
// the range test over the qualities.  rec_off[r] = the record's block_size field, counted from `text` like every offset
// written here (the caller takes `lead` off).  accept & 0x10: a reverse-strand record gets GRP_FQ_REVERSED (its offsets still
// name the stored bytes; both tests below do not depend on the order).
__global__ void __launch_bounds__(THREADS)
k_bam_records(const uint8_t* __restrict__ text, const uint64_t* __restrict__ rec_off, uint64_t n_records, uint32_t accept, grp_fastq_record* __restrict__ out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (r >= n_records) {
    return;
  }
  const uint64_t o = rec_off[r];
  const uint8_t* f = text + o + 4; // refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, ... (little endian, unaligned)
  const uint32_t l_name = f[8];
  const uint32_t n_cigar = (uint32_t)f[12] | ((uint32_t)f[13] << 8);
  const uint32_t l_seq = (uint32_t)f[16] | ((uint32_t)f[17] << 8) | ((uint32_t)f[18] << 16) | ((uint32_t)f[19] << 24);
  const uint64_t name = o + 4 + gr::BAM_FIXED;
  // id = the name up to its NUL (the host has seen it at l_name - 1), cut at the first whitespace like a FASTQ header
  uint32_t id_len = l_name - 1;
  for (uint32_t base = 0; base < l_name; base += 64) { // (l_read_name is one byte: four rounds at the most)
    const uint32_t i = base + lane;
    bool stop = false;
    if (i < l_name) {
      const uint8_t ch = text[name + i];
      stop = ch == 0 || ch == ' ' || (ch >= 9 && ch <= 13);
    }
    const unsigned long long m = __ballot(stop);
    if (m != 0ull) {
      id_len = base + (uint32_t)__ffsll((long long)m) - 1u;
      break;
    }
  }
  grp_fastq_record rec;
  rec.flags = (accept & f[14] & gr::BAM_FLAG_REVERSE) ? GRP_FQ_REVERSED : 0u;
  rec.id_off = name;
  rec.id_len = id_len;
  rec.seq_off = name + l_name + 4ull * n_cigar;
  rec.seq_len = l_seq;
  rec.qual_off = rec.seq_off + ((uint64_t)l_seq + 1) / 2;
  rec.qual_len = l_seq;
  // the ACGT test over the l_seq / 2 whole bytes; the last base of an odd length is the high code of the byte behind them,
  // whose low code is padding the specification leaves undefined
  const uint64_t whole = rec.seq_off + l_seq / 2;
  bool bad = bam_scan_bad(
    text, rec.seq_off, whole, lane, [](uint8_t b) { return __popc(b >> 4) != 1 || __popc(b & 15u) != 1; }, [](uint32_t w) { return !bam_acgt8(w); });
  if ((l_seq & 1u) && lane == 0) {
    bad = bad || __popc(text[whole] >> 4) != 1;
  }
  const bool qbad = bam_scan_bad(
    text, rec.qual_off, rec.qual_off + l_seq, lane, [](uint8_t b) { return b > gr::BAM_MAX_QUAL; }, [](uint32_t w) { return bam_qual4_bad(w); });
  if (__ballot(bad) != 0ull) {
    rec.flags |= GRP_FQ_NON_ACGT;
  }
  if (__ballot(qbad) != 0ull) {
    rec.flags |= BAM_BAD_QUAL;
  }
  // (the Phred sums: k_fq_phred over qual_off / qual_len, with the table of raw qualities)
  rec.phred_sum = 0.0;
  rec.phred_first = 0.0;
  if (lane == 0) {
    out[r] = rec;
  }
}

// (gr::bam_pack16 and the word functions of the reversed pack: host/gr_bam.hpp, where they compile for the host too)
constexpr uint64_t BAM_PACK_REVERSED = 1ull << 63; // in a seq_off handed to k_bam_pack: the record is packed backwards (a chunk has < 2^36 bytes)

// one workgroup per selected record (k_fq_pack's geometry); a word's 8 source bytes begin wherever the name left them.
// A reversed record (BAM_PACK_REVERSED): word w holds the twin's bases 16w ... 16w + cnt - 1, which are the stored bases
// n - 16w - cnt ... n - 16w - 1, last first and complemented — the 8 bytes that hold them (9 where the first of them is
// the low half of its byte: the parity of n), packed as they stand and turned round as a word.  No load goes in front
// of seq_off or behind the record's last code byte.
__global__ void __launch_bounds__(THREADS)
k_bam_pack(const uint8_t* __restrict__ text, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ len, const uint64_t* __restrict__ word_off, uint32_t* __restrict__ packed)
{
  const uint32_t r = blockIdx.x;
  const bool reversed = (seq_off[r] & BAM_PACK_REVERSED) != 0;
  const uint8_t* src = text + (seq_off[r] & ~BAM_PACK_REVERSED);
  const uint32_t n = len[r];
  const uint32_t nw = (n + 15u) / 16u;
  uint32_t* dst = packed + word_off[r];
  for (uint32_t w = threadIdx.x; w < nw; w += THREADS) {
    const uint32_t cnt = min(16u, n - w * 16u);
    if (reversed) {
      const uint32_t s0 = n - w * 16u - cnt; // the first stored base of the word (0 for the record's last word, where cnt < 16)
      const uint8_t* s = src + (s0 >> 1);
      uint64_t x = 0;
      if (cnt == 16u) {
        __builtin_memcpy(&x, s, 8);
        if (s0 & 1u) {
          x = gr::bam_shift_nibble(x, s[8]); // (base s0 + 15 is the high half of the ninth byte: inside the record)
        }
      } else {
        for (uint32_t j = 0; j < (cnt + 1u) / 2u; ++j) {
          x |= (uint64_t)s[j] << (8u * j);
        }
      }
      dst[w] = gr::bam_revcomp16(gr::bam_pack16(x), cnt);
      continue;
    }
    const uint8_t* s = src + (uint64_t)w * 8u;
    uint64_t x = 0;
    if (cnt == 16u) {
      __builtin_memcpy(&x, s, 8);
    } else { // the record's last word: its (cnt + 1) / 2 bytes and not one more
      for (uint32_t j = 0; j < (cnt + 1u) / 2u; ++j) {
        x |= (uint64_t)s[j] << (8u * j);
      }
    }
    uint32_t v = gr::bam_pack16(x);
    if (cnt < 16u) {
      v &= (1u << (2u * cnt)) - 1u; // (the padding code behind an odd length is not a base)
    }
    dst[w] = v;
  }
}

} // namespace

struct grp_fastq
{
  grp_ctx* ctx = nullptr;
  bool bam = false; // the chunk holds BAM records (grp_bam_parse): seq_off = 4-bit codes, packed by k_bam_pack
  uint8_t* d_text = nullptr; // 16-byte aligned; the text begins `lead` bytes behind it
  DevBuf<uint8_t> own_text;  // what d_text points into where no slot of the context was free
  uint32_t lead = 0;
  int pool_slot = -1; // >= 0: d_text lies in the context's ingest buffer of that slot, given back by grp_fastq_free
  uint64_t n_bytes = 0;
  std::vector<grp_fastq_record> rec; // host copy
};

namespace {

// the parse's page-locked, device-mapped staging: two scalars, the front of a prefetched text, the record table
int
ingest_stage(grp_ctx* c, uint64_t front_bytes, uint64_t rec_bytes)
{
  grp_ctx::IngestPool& ip = c->ingest;
  if (!ip.h_scal) {
    HIP_TRY(c, ip.h_scal.reset(8, hipHostMallocMapped | hipHostMallocCoherent));
  }
  if (front_bytes && !ip.h_front) {
    HIP_TRY(c, ip.h_front.reset(FQ_FRONT + 64, hipHostMallocMapped | hipHostMallocCoherent));
  }
  if (rec_bytes > ip.h_rec.cap) {
    if (ip.h_rec) {
      (void)hipStreamSynchronize(c->stream2);
    }
    HIP_TRY(c, ip.h_rec.reset(rec_bytes + rec_bytes / 4 + 4096, hipHostMallocMapped | hipHostMallocCoherent));
  }
  return GRP_OK;
}

// The bytes of a chunk into one of the context's text buffers, for grp_fastq_parse and grp_bam_parse alike: the slot (or a
// buffer of the handle's own), the body that a prefetch has brought up already, the copy on the side stream, and the
// main stream made to wait for it.  fq->d_text / lead / pool_slot say where the bytes are.
int
ingest_upload(grp_ctx* c, grp_fastq* fq, const char* text, uint64_t n_bytes, const char* who)
{
#define ING_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      return set_err(c, GRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                                   \
    }                                                                                                                  \
  } while (0)
  bool prefetched = false; // the text's body is already on the device (or on its way on the side stream): grp_fastq_prefetch
  uint64_t front_len = 0;  // prefetched: the bytes of `text` in front of that body, uploaded here
  uint64_t dev_off = 0;    // offset of text[0] in its slot
  {
    // one of the context's three text buffers (grown, never shrunk); a fourth chunk alive at once gets its own.
    // The slots take turns (round 5): the chunk in the caller's hands, the next one (its body uploaded ahead) and the one
    // after (uploading) each have one; a slot's last use by the main stream — the pack of its chunk — is three chunks old
    // when its next upload begins, so the copy never waits for the fill queued behind that pack.
    grp_ctx::IngestPool& ip = c->ingest;
    int slot = -1;
    if (ip.n_pre > 0) {
      // prefetches are pending: the oldest is this parse's own body — or another text's, and all of them are dropped
      // (their copies are ahead of anything queued from here on the side stream: the slots can be taken again)
      const grp_ctx::IngestPool::Pre p = ip.pre[0];
      const uint64_t front = n_bytes >= p.n_body ? n_bytes - p.n_body : ~0ull;
      if (front <= FQ_FRONT && text + front == p.body && !ip.text_used[p.slot]) {
        slot = p.slot;
        prefetched = true;
        front_len = front;
        dev_off = FQ_FRONT - front;
        ip.pre[0] = ip.pre[1];
        --ip.n_pre;
      } else {
        // another text's: every pending prefetch is dropped.  Their copies may still be reading the caller's buffers, which
        // the caller is free to reuse once this parse returns: waited for here (ADVICE r05), and counted (GRP_DEBUG_STATS)
        for (int q = 0; q < ip.n_pre; ++q) {
          if (ip.text_up[ip.pre[q].slot]) {
            (void)hipEventSynchronize(ip.text_up[ip.pre[q].slot]);
          }
          ++ip.n_dropped;
        }
        ip.n_pre = 0;
      }
    }
    for (int k2 = 1; k2 <= FQ_TEXT_SLOTS && slot < 0; ++k2) {
      const int i = (ip.last_slot + k2) % FQ_TEXT_SLOTS;
      if (ip.text_used[i]) {
        continue;
      }
      if (ip.text[i].cap < n_bytes + 64) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->stream2);
        (void)hipStreamSynchronize(c->stream3);
        const uint64_t want = FQ_FRONT + n_bytes + n_bytes / 8 + 64;
        if (ip.text[i].reset(want) != hipSuccess) {
          set_err(c, GRP_ERR_NOMEM, "%s: allocating %llu bytes of device memory failed", who, (unsigned long long)want);
          return GRP_ERR_NOMEM;
        }
      }
      slot = i;
      ip.last_slot = slot;
    }
    if (slot >= 0) {
      ip.text_used[slot] = true;
      fq->pool_slot = slot;
      fq->d_text = ip.text[slot] + (dev_off & ~(uint64_t)15);
      fq->lead = (uint32_t)(dev_off & 15u);
    } else if (fq->own_text.reset(n_bytes + 64) != hipSuccess) {
      set_err(c, GRP_ERR_NOMEM, "%s: allocating %llu bytes of device memory failed", who, (unsigned long long)n_bytes);
      return GRP_ERR_NOMEM;
    } else {
      fq->d_text = fq->own_text;
    }
  }
  // The whole parse runs on the SIDE stream (round 5): the caller has usually just queued the fill of the chunk
  // before on the main stream without waiting for it, and the copy (a DMA out of the page-locked chunk buffer), the
  // line scan and the record extraction of this chunk run beside it — the waits below are for the side stream alone,
  // so the host's share of a chunk (records back, filters, selection) overlaps the fill instead of following it
  // (the ingest pass of the binary was GPU 12.5 ms + host 7 ms per 256 MiB chunk, one after the other).  The slot's
  // text may still be read by the main stream (the pack of the chunk before last): the upload waits for that event,
  // not the host.
  hipStream_t ps = c->stream2;
  if (!c->ingest.uploaded) {
    ING_TRY(c->ingest.uploaded.create(hipEventDisableTiming));
  }
  const uint32_t lead = fq->lead;
  if (fq->pool_slot >= 0 && c->ingest.text_up[fq->pool_slot]) {
    // the last body copied into this slot ahead of its parse (this chunk's — or a dropped one's, still on its way)
    ING_TRY(hipStreamWaitEvent(ps, c->ingest.text_up[fq->pool_slot], 0));
  }
  if (!prefetched) {
    if (fq->pool_slot >= 0 && c->ingest.text_done[fq->pool_slot]) {
      ING_TRY(hipStreamWaitEvent(ps, c->ingest.text_done[fq->pool_slot], 0));
    }
    ING_TRY(hipMemcpyAsync(fq->d_text, text, n_bytes, hipMemcpyHostToDevice, ps));
    ING_TRY(hipMemsetAsync(fq->d_text + n_bytes, 0, 64, ps));
  } else if (front_len) {
    // the body is in place (or arriving): the tail of the chunk before goes in front of it — by a kernel out of a mapped
    // staging buffer (see k_ing_bytes)
    if (ingest_stage(c, front_len, 0) != GRP_OK) {
      return GRP_ERR_HIP;
    }
    memcpy(c->ingest.h_front, text, front_len);
    k_ing_bytes<<<dim3((uint32_t)std::min<uint64_t>((front_len + THREADS - 1) / THREADS, 64)), dim3(THREADS), 0, ps>>>(fq->d_text + lead, c->ingest.h_front.dev, front_len);
    ING_TRY(hipGetLastError());
  }
  ING_TRY(hipEventRecord(c->ingest.uploaded, ps));
  ING_TRY(hipStreamWaitEvent(c->stream, c->ingest.uploaded, 0)); // what the main stream does with this chunk (pack) comes behind its text
  return GRP_OK;
#undef ING_TRY
}

// 10^(-q/10) for the byte that stands for quality q: the host's pow() values (calc_phred_average.cpp:21-24).  FASTQ text
// holds q + 33 (shift 33), a BAM record holds q itself (shift 0): the same values, 33 entries apart.
int
ingest_phred_table(grp_ctx* c, DevBuf<double>& d_tab, int shift, const char* who)
{
  if (!d_tab) {
    double tab[256];
    for (int ch = 0; ch < 256; ++ch) {
      const int q = shift ? (int)((char)ch - shift) : ch;
      tab[ch] = std::pow(10.0, -q / 10.0);
    }
    if (d_tab.reset(256) != hipSuccess || hipMemcpy(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) {
      return set_err(c, GRP_ERR_HIP, "%s: cannot set up the Phred table", who);
    }
  }
  return GRP_OK;
}

} // namespace

extern "C" {

int
grp_fastq_parse(grp_ctx* c, const char* text, uint64_t n_bytes, int final_chunk, grp_fastq** out, uint64_t* n_records, uint64_t* bytes_consumed, int* stopped)
{
  if (!c || !out || !n_records || !bytes_consumed || (!text && n_bytes)) {
    return set_err(c, GRP_ERR_INVALID, "grp_fastq_parse: bad argument");
  }
  *out = nullptr;
  *n_records = 0;
  *bytes_consumed = 0;
  if (stopped) {
    *stopped = 0;
  }
  if (n_bytes >= (1ull << 36)) {
    return set_err(c, GRP_ERR_INVALID, "grp_fastq_parse: chunk too large");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_fastq* fq = new grp_fastq();
  fq->ctx = c;
  fq->n_bytes = n_bytes;
  if (n_bytes == 0) {
    *out = fq;
    return GRP_OK;
  }
  auto fail = [&](int code) {
    grp_fastq_free(fq);
    return code;
  };
  if (ingest_phred_table(c, c->d_delog, 33, "grp_fastq_parse") != GRP_OK) {
    return fail(GRP_ERR_HIP);
  }
  const int urc = ingest_upload(c, fq, text, n_bytes, "grp_fastq_parse");
  if (urc != GRP_OK) {
    return fail(urc);
  }
  hipStream_t ps = c->stream2;
  const uint32_t lead = fq->lead;
  const uint64_t n_total = lead + n_bytes; // what the kernels see: the slot's 16-byte group the text begins in, from its start
  const uint64_t n_blocks = (n_total + NL_BLOCK_BYTES - 1) / NL_BLOCK_BYTES;
  grp_ctx::IngestPool& ip = c->ingest; // scratch of this call, kept for the next chunk
  auto cleanup = [&]() {};
  auto fail2 = [&](int code) {
    cleanup();
    return fail(code);
  };
#define FQ_TRY2(expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      set_err(c, GRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                                          \
      return fail2(GRP_ERR_HIP);                                                                                       \
    }                                                                                                                  \
  } while (0)
  if (ensure_dev(c, ip.d_counts, n_blocks) != GRP_OK || ensure_dev(c, ip.d_base, n_blocks) != GRP_OK ||
      ensure_dev(c, ip.d_super, n_blocks / ((1u << GRP_SUPER_SHIFT) / GRP_CHUNK_BUCKETS) + 2) != GRP_OK || ensure_dev(c, ip.d_total, 1) != GRP_OK) {
    return fail2(GRP_ERR_NOMEM);
  }
  uint32_t* const d_counts = ip.d_counts;
  uint64_t *const d_base = ip.d_base, *const d_super = ip.d_super, *const d_total = ip.d_total;
  k_nl_count<<<dim3((uint32_t)n_blocks), dim3(THREADS), 0, ps>>>(fq->d_text, n_total, lead, d_counts);
  k_scan_chunks<<<dim3(1), dim3(1024), 0, ps>>>(d_counts, n_blocks, d_base, d_super, d_total);
  if (ingest_stage(c, 0, 0) != GRP_OK) {
    return fail2(GRP_ERR_HIP);
  }
  k_ing_words<<<dim3(1), dim3(THREADS), 0, ps>>>(reinterpret_cast<unsigned long long*>(ip.h_scal.dev), reinterpret_cast<const unsigned long long*>(d_total), 1);
  FQ_TRY2(hipStreamSynchronize(ps));
  const uint64_t n_nl = ip.h_scal[0];
  if (ensure_dev(c, ip.d_nl, n_nl + 2) != GRP_OK) {
    return fail2(GRP_ERR_NOMEM);
  }
  uint64_t* const d_nl = ip.d_nl;
  k_nl_scatter<<<dim3((uint32_t)n_blocks), dim3(THREADS), 0, ps>>>(fq->d_text, n_total, lead, d_base, d_nl);
  uint64_t n_lines = n_nl;
  if (final_chunk && text[n_bytes - 1] != '\n') {
    // last line without a newline: give it a virtual one behind the text
    FQ_TRY2(hipMemcpyAsync(d_nl + n_nl, &n_total, 8, hipMemcpyHostToDevice, ps));
    n_lines = n_nl + 1;
  }
  uint64_t n_rec = n_lines / 4;
  if (n_rec) {
    if (ingest_stage(c, 0, n_rec * sizeof(grp_fastq_record)) != GRP_OK) {
      return fail2(GRP_ERR_HIP);
    }
    k_ing_words<<<dim3(1), dim3(THREADS), 0, ps>>>(reinterpret_cast<unsigned long long*>(ip.h_scal.dev) + 1, reinterpret_cast<const unsigned long long*>(d_nl + (4 * n_rec - 1)), 1);
    if (n_rec * sizeof(grp_fastq_record) > ip.d_rec.cap) {
      FQ_TRY2(ip.d_rec.reset((n_rec + n_rec / 4 + 64) * sizeof(grp_fastq_record)));
    }
    grp_fastq_record* const d_rec = reinterpret_cast<grp_fastq_record*>(ip.d_rec.p);
    k_fq_records<<<dim3((uint32_t)((n_rec + (THREADS / 64) - 1) / (THREADS / 64))), dim3(THREADS), 0, ps>>>(fq->d_text, d_nl, n_rec, lead, d_rec);
    k_fq_phred<false><<<dim3((uint32_t)((n_rec + 63) / 64)), dim3(64), 0, ps>>>(fq->d_text, n_rec, c->d_delog, d_rec);
    FQ_TRY2(hipGetLastError());
    static_assert(sizeof(grp_fastq_record) % 8 == 0, "the record table goes down as 64-bit words");
    const uint64_t rec_words = n_rec * sizeof(grp_fastq_record) / 8;
    k_ing_words<<<dim3((uint32_t)std::min<uint64_t>((rec_words + THREADS - 1) / THREADS, 256)), dim3(THREADS), 0, ps>>>(reinterpret_cast<unsigned long long*>(ip.h_rec.dev), reinterpret_cast<const unsigned long long*>(d_rec), rec_words);
    FQ_TRY2(hipGetLastError());
    FQ_TRY2(hipStreamSynchronize(ps));
    const uint64_t last_nl = ip.h_scal[1];
    fq->rec.resize(n_rec);
    memcpy(fq->rec.data(), ip.h_rec, n_rec * sizeof(grp_fastq_record));
    *bytes_consumed = std::min<uint64_t>(last_nl + 1 - lead, n_bytes);
    if (lead) { // the caller's offsets count from text[0]
      for (grp_fastq_record& rr : fq->rec) {
        rr.id_off -= lead;
        rr.seq_off -= lead;
        rr.qual_off -= lead;
      }
    }
    for (uint64_t i = 0; i < n_rec; ++i) {
      if (fq->rec[i].flags & FQ_BAD_HEADER) { // not a FASTQ header: the reader ends here
        fq->rec.resize(i);
        if (stopped) {
          *stopped = 1;
        }
        *bytes_consumed = n_bytes;
        break;
      }
    }
  } else {
    FQ_TRY2(hipStreamSynchronize(ps));
  }
  cleanup();
#undef FQ_TRY2
  *n_records = fq->rec.size();
  *out = fq;
  return GRP_OK;
}

int
grp_bam_parse(grp_ctx* c, const char* bytes, uint64_t n_bytes, int final_chunk, grp_fastq** out, uint64_t* n_records, uint64_t* bytes_consumed, uint64_t* bad_offset)
{
  uint64_t n_skipped = 0;
  return grp_bam_parse_ex(c, bytes, n_bytes, final_chunk, 0u, out, n_records, bytes_consumed, bad_offset, &n_skipped);
}

int
grp_bam_parse_ex(grp_ctx* c, const char* bytes, uint64_t n_bytes, int final_chunk, uint32_t accept, grp_fastq** out, uint64_t* n_records, uint64_t* bytes_consumed, uint64_t* bad_offset, uint64_t* n_skipped)
{
  if (!c || !out || !n_records || !bytes_consumed || !bad_offset || !n_skipped || (!bytes && n_bytes)) {
    return set_err(c, GRP_ERR_INVALID, "grp_bam_parse: bad argument");
  }
  *out = nullptr;
  *n_records = 0;
  *bytes_consumed = 0;
  *bad_offset = 0;
  *n_skipped = 0;
  if (accept & ~gr::BAM_REFUSED_FLAGS) {
    return set_err(c, GRP_ERR_INVALID, "grp_bam_parse_ex: accept 0x%x holds other bits than 0x10, 0x100 and 0x800", accept);
  }
  if (n_bytes >= (1ull << 36)) {
    return set_err(c, GRP_ERR_INVALID, "grp_bam_parse: chunk too large");
  }
  // the record chain, on the host (gr_bam.hpp): where the complete records begin, or the record that is refused
  std::vector<uint64_t> offs;
  uint64_t used = 0, bad = 0, skipped = 0;
  const char* why = nullptr;
  if (gr::bam_walk(reinterpret_cast<const uint8_t*>(bytes), n_bytes, final_chunk != 0, accept, &used, &skipped, &bad, &why, [&](const gr::BamRecord& r) {
        offs.push_back(r.off);
        return true;
      }) != 0) {
    *bad_offset = bad;
    return set_err(c, GRP_ERR_INVALID, "%s", why);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_fastq* fq = new grp_fastq();
  fq->ctx = c;
  fq->bam = true;
  fq->n_bytes = n_bytes;
  *bytes_consumed = used;
  *n_skipped = skipped;
  if (n_bytes == 0) {
    *out = fq;
    return GRP_OK;
  }
  auto fail = [&](int code) {
    grp_fastq_free(fq);
    *bytes_consumed = 0;
    *n_skipped = 0;
    return code;
  };
#define BAM_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      set_err(c, GRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                                          \
      return fail(GRP_ERR_HIP);                                                                                        \
    }                                                                                                                  \
  } while (0)
  if (ingest_phred_table(c, c->d_delog_raw, 0, "grp_bam_parse") != GRP_OK) {
    return fail(GRP_ERR_HIP);
  }
  // (all of `bytes` goes up, complete records or not: a body uploaded ahead is this chunk's whatever the walk found)
  const int urc = ingest_upload(c, fq, bytes, n_bytes, "grp_bam_parse");
  if (urc != GRP_OK) {
    return fail(urc);
  }
  hipStream_t ps = c->stream2; // the side stream, as grp_fastq_parse
  const uint64_t n_rec = offs.size();
  if (n_rec) {
    grp_ctx::IngestPool& ip = c->ingest;
    if (n_rec > ip.h_bam_off.cap) {
      BAM_TRY(hipStreamSynchronize(ps));
      BAM_TRY(ip.h_bam_off.reset(n_rec + n_rec / 4 + 512, hipHostMallocMapped | hipHostMallocCoherent));
    }
    if (ingest_stage(c, 0, n_rec * sizeof(grp_fastq_record)) != GRP_OK) {
      return fail(GRP_ERR_HIP);
    }
    if (n_rec * sizeof(grp_fastq_record) > ip.d_rec.cap) {
      BAM_TRY(ip.d_rec.reset((n_rec + n_rec / 4 + 64) * sizeof(grp_fastq_record)));
    }
    // the walk's table goes up beside the bytes: the kernels read it out of page-locked, device-mapped memory (see k_ing_bytes)
    for (uint64_t i = 0; i < n_rec; ++i) {
      ip.h_bam_off[i] = offs[i] + fq->lead;
    }
    grp_fastq_record* const d_rec = reinterpret_cast<grp_fastq_record*>(ip.d_rec.p);
    k_bam_records<<<dim3((uint32_t)((n_rec + (THREADS / 64) - 1) / (THREADS / 64))), dim3(THREADS), 0, ps>>>(fq->d_text, ip.h_bam_off.dev, n_rec, accept, d_rec);
    if (accept & gr::BAM_FLAG_REVERSE) {
      k_fq_phred<true><<<dim3((uint32_t)((n_rec + 63) / 64)), dim3(64), 0, ps>>>(fq->d_text, n_rec, c->d_delog_raw, d_rec);
    } else {
      k_fq_phred<false><<<dim3((uint32_t)((n_rec + 63) / 64)), dim3(64), 0, ps>>>(fq->d_text, n_rec, c->d_delog_raw, d_rec);
    }
    BAM_TRY(hipGetLastError());
    const uint64_t rec_words = n_rec * sizeof(grp_fastq_record) / 8;
    k_ing_words<<<dim3((uint32_t)std::min<uint64_t>((rec_words + THREADS - 1) / THREADS, 256)), dim3(THREADS), 0, ps>>>(reinterpret_cast<unsigned long long*>(ip.h_rec.dev), reinterpret_cast<const unsigned long long*>(d_rec), rec_words);
    BAM_TRY(hipGetLastError());
    BAM_TRY(hipStreamSynchronize(ps));
    fq->rec.resize(n_rec);
    memcpy(fq->rec.data(), ip.h_rec, n_rec * sizeof(grp_fastq_record));
    for (uint64_t i = 0; i < n_rec; ++i) {
      grp_fastq_record& rr = fq->rec[i];
      rr.id_off -= fq->lead; // the caller's offsets count from bytes[0]
      rr.seq_off -= fq->lead;
      rr.qual_off -= fq->lead;
      if (rr.flags & BAM_BAD_QUAL) {
        *bad_offset = offs[i];
        set_err(c, GRP_ERR_INVALID, "a quality without a FASTQ character (absent: 0xFF, or above 93)");
        return fail(GRP_ERR_INVALID);
      }
    }
  } else {
    BAM_TRY(hipStreamSynchronize(ps));
  }
#undef BAM_TRY
  *n_records = n_rec;
  *out = fq;
  return GRP_OK;
}

int
grp_fastq_prefetch(grp_ctx* c, const char* text, uint64_t n_bytes)
{
  if (c && !text && n_bytes == 0) { // the caller's buffers are going away: what was handed over and never parsed is forgotten
    HIP_TRY(c, hipSetDevice(c->device));
    c->ingest.n_pre = 0;
    if (c->stream3) {
      HIP_TRY(c, hipStreamSynchronize(c->stream3));
    }
    return GRP_OK;
  }
  if (!c || !text || n_bytes == 0 || n_bytes >= (1ull << 36)) {
    return set_err(c, GRP_ERR_INVALID, "grp_fastq_prefetch: bad argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_ctx::IngestPool& ip = c->ingest;
  if (ip.n_pre >= 2) {
    return GRP_ERR_BUSY;
  }
  // a slot no chunk holds and no prefetch is heading for, large enough as it is (growing one waits for the device) or not
  // allocated yet; the body goes FQ_FRONT bytes into it: what the parse finds in front of these bytes goes in front of them
  int slot = -1;
  for (int k2 = 1; k2 <= FQ_TEXT_SLOTS && slot < 0; ++k2) {
    const int i = (ip.last_slot + k2) % FQ_TEXT_SLOTS;
    bool pending = false;
    for (int q = 0; q < ip.n_pre; ++q) {
      pending = pending || ip.pre[q].slot == i;
    }
    if (ip.text_used[i] || pending) {
      continue;
    }
    if (!ip.text[i]) {
      const uint64_t want = FQ_FRONT + n_bytes + n_bytes / 8 + 64;
      if (ip.text[i].reset(want) != hipSuccess) {
        (void)hipGetLastError();
        return GRP_ERR_BUSY;
      }
    }
    if (ip.text[i].cap >= FQ_FRONT + n_bytes + 64) {
      slot = i;
    }
  }
  if (slot < 0) {
    return GRP_ERR_BUSY;
  }
  // on the COPY stream: behind the parse kernels of the chunk before (the side stream) the 5 ms of this copy stood in front
  // of every parse — the upload had only moved to another chunk's path
  if (ip.text_done[slot]) {
    HIP_TRY(c, hipStreamWaitEvent(c->stream3, ip.text_done[slot], 0));
  }
  HIP_TRY(c, hipMemcpyAsync(ip.text[slot] + FQ_FRONT, text, n_bytes, hipMemcpyHostToDevice, c->stream3));
  HIP_TRY(c, hipMemsetAsync(ip.text[slot] + FQ_FRONT + n_bytes, 0, 64, c->stream3));
  if (!ip.text_up[slot]) {
    HIP_TRY(c, ip.text_up[slot].create(hipEventDisableTiming));
  }
  HIP_TRY(c, hipEventRecord(ip.text_up[slot], c->stream3));
  ip.pre[ip.n_pre].slot = slot;
  ip.pre[ip.n_pre].body = text;
  ip.pre[ip.n_pre].n_body = n_bytes;
  ++ip.n_pre;
  ip.last_slot = slot;
  return GRP_OK;
}

int
grp_fastq_records(grp_fastq* fq, grp_fastq_record* out)
{
  if (!fq || (!out && !fq->rec.empty())) {
    return GRP_ERR_INVALID;
  }
  if (!fq->rec.empty()) {
    memcpy(out, fq->rec.data(), fq->rec.size() * sizeof(grp_fastq_record));
  }
  return GRP_OK;
}

int
grp_fastq_pack(grp_ctx* c, grp_fastq* fq, const uint32_t* sel, uint32_t n_sel, grp_reads** out)
{
  if (!c || !fq || fq->ctx != c || !out || (!sel && n_sel)) {
    return set_err(c, GRP_ERR_INVALID, "grp_fastq_pack: bad argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  grp_reads* rd = new grp_reads();
  std::vector<uint64_t>&seq_off = rd->h_seq_off, &word_off = rd->h_word_off; // (the copies below read them: they stay with the batch)
  seq_off.resize(n_sel);
  word_off.resize((size_t)n_sel + 1);
  std::vector<uint32_t> len(n_sel);
  uint64_t w = 0;
  for (uint32_t i = 0; i < n_sel; ++i) {
    if (sel[i] >= fq->rec.size() || (i && sel[i] <= sel[i - 1])) {
      delete rd;
      return set_err(c, GRP_ERR_INVALID, "grp_fastq_pack: selection must be ascending record indices");
    }
    const grp_fastq_record& r = fq->rec[sel[i]];
    if (r.flags & GRP_FQ_NON_ACGT) {
      delete rd;
      return set_err(c, GRP_ERR_INVALID, "grp_fastq_pack: record %u holds a non-ACGT base", sel[i]);
    }
    seq_off[i] = r.seq_off | ((fq->bam && (r.flags & GRP_FQ_REVERSED)) ? BAM_PACK_REVERSED : 0ull);
    len[i] = r.seq_len;
    word_off[i] = w;
    w += (r.seq_len + 15u) / 16u;
  }
  word_off[n_sel] = w;
  auto bail = [&](int code) {
    grp_reads_free(rd);
    return code;
  };
  // The batch's host arrays, then ONE device allocation behind the packed bases' (word offsets, lengths, tile and
  // fill-chunk prefixes, the tile -> read and chunk -> read maps, and the selection's sequence offsets for the pack
  // kernel) filled by asynchronous copies on the main stream: seven allocations, nine copies and two waits per chunk
  // used to sit here (round 4: "~7 ms of host time per 256 MiB chunk").
  int rc = reads_index(c, rd, word_off.data(), len.data(), n_sel);
  if (rc != GRP_OK) {
    return bail(rc);
  }
  const uint64_t nt = rd->tile0[n_sel], nch = rd->chunk0[n_sel];
  const auto up8 = [](uint64_t b) { return (b + 15) & ~(uint64_t)15; };
  const uint64_t o_wo = 0, o_t0 = o_wo + up8(((uint64_t)n_sel + 1) * 8), o_c0 = o_t0 + up8(((uint64_t)n_sel + 1) * 8), o_so = o_c0 + up8(((uint64_t)n_sel + 1) * 8);
  const uint64_t o_len = o_so + up8(std::max<uint64_t>(n_sel, 1) * 8), o_tr = o_len + up8(std::max<uint64_t>(n_sel, 1) * 4), o_cr = o_tr + up8(std::max<uint64_t>(nt, 1) * 4);
  const uint64_t slab_bytes = o_cr + up8(std::max<uint64_t>(nch, 1) * 4);
  if (rd->d_packed.reset(std::max<uint64_t>(w, 1) + 4) != hipSuccess || rd->d_slab.reset(slab_bytes) != hipSuccess) {
    return bail(set_err(c, GRP_ERR_NOMEM, "grp_fastq_pack: allocating %llu words + %llu bytes of device memory failed", (unsigned long long)w, (unsigned long long)slab_bytes));
  }
  uint8_t* const slab = rd->d_slab;
  uint64_t* const d_word_off = reinterpret_cast<uint64_t*>(slab + o_wo);
  uint64_t* const d_tile0 = reinterpret_cast<uint64_t*>(slab + o_t0);
  uint64_t* const d_chunk0 = reinterpret_cast<uint64_t*>(slab + o_c0);
  uint64_t* const d_so = reinterpret_cast<uint64_t*>(slab + o_so);
  uint32_t* const d_len = reinterpret_cast<uint32_t*>(slab + o_len);
  uint32_t* const d_tile_read = reinterpret_cast<uint32_t*>(slab + o_tr);
  uint32_t* const d_chunk_read = reinterpret_cast<uint32_t*>(slab + o_cr);
  hipError_t e = hipMemcpyAsync(d_word_off, word_off.data(), ((size_t)n_sel + 1) * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tile0, rd->tile0.data(), ((size_t)n_sel + 1) * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_chunk0, rd->chunk0.data(), ((size_t)n_sel + 1) * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_sel) e = hipMemcpyAsync(d_so, seq_off.data(), (size_t)n_sel * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_sel) e = hipMemcpyAsync(d_len, rd->len.data(), (size_t)n_sel * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && nt) e = hipMemcpyAsync(d_tile_read, rd->h_tile_read.data(), nt * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && nch) e = hipMemcpyAsync(d_chunk_read, rd->h_chunk_read.data(), nch * 4, hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) {
    return bail(set_err(c, GRP_ERR_HIP, "grp_fastq_pack: upload failed: %s", hipGetErrorString(e)));
  }
  if (n_sel) {
    if (fq->bam) {
      k_bam_pack<<<dim3(n_sel), dim3(THREADS), 0, c->stream>>>(fq->d_text + fq->lead, d_so, d_len, d_word_off, rd->d_packed);
    } else {
      k_fq_pack<<<dim3(n_sel), dim3(THREADS), 0, c->stream>>>(fq->d_text + fq->lead, d_so, d_len, d_word_off, rd->d_packed);
    }
    if (hipGetLastError() != hipSuccess) {
      return bail(set_err(c, GRP_ERR_HIP, "grp_fastq_pack: kernel launch failed"));
    }
  }
  rd->dev.packed = rd->d_packed;
  rd->dev.word_off = d_word_off;
  rd->dev.len = d_len;
  rd->dev.tile0 = d_tile0;
  rd->dev.tile_read = d_tile_read;
  rd->dev.chunk0 = d_chunk0;
  rd->dev.chunk_read = d_chunk_read;
  *out = rd;
  return GRP_OK;
}

// The caller's chunk buffer, page-locked for as long as the caller says: the copy of a chunk then
// runs as one DMA (tens of GB/s) instead of being staged through the runtime's bounce buffers.
// Explicit on purpose — a registration the engine kept on its own outlived the buffer (freed,
// and the next allocation at the same address looked "registered": a GPU memory fault).
int
grp_fastq_pin(grp_ctx* c, const char* buffer, uint64_t n_bytes)
{
  if (!c || !buffer || n_bytes == 0) {
    return set_err(c, GRP_ERR_INVALID, "grp_fastq_pin: bad argument");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  (void)grp_fastq_unpin(c);
  if (hipHostRegister(const_cast<char*>(buffer), n_bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(c, GRP_ERR_HIP, "grp_fastq_pin: the buffer cannot be page-locked (it is copied as pageable memory)");
  }
  c->reg_text = buffer;
  c->reg_bytes = n_bytes;
  return GRP_OK;
}

int
grp_fastq_unpin(grp_ctx* c)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  c->ingest.n_pre = 0; // bodies handed over ahead of a parse that never came: their addresses mean nothing once the buffer is gone
  if (c->reg_text) {
    if (c->stream3) { // (such a body may still be on its way out of this buffer)
      (void)hipStreamSynchronize(c->stream3);
    }
    if (c->stream2) {
      (void)hipStreamSynchronize(c->stream2);
    }
    if (c->stream) {
      (void)hipStreamSynchronize(c->stream);
    }
    (void)hipHostUnregister(const_cast<char*>(c->reg_text));
    (void)hipGetLastError();
    c->reg_text = nullptr;
    c->reg_bytes = 0;
  }
  return GRP_OK;
}

void
grp_fastq_free(grp_fastq* fq)
{
  if (!fq) {
    return;
  }
  if (fq->pool_slot >= 0 && fq->ctx) {
    // the buffer stays with the context for the chunk after next; what the main stream still does with its text (the
    // pack of this chunk) is marked by an event the next upload into the slot waits for — the host does not (round 5)
    grp_ctx::IngestPool& ip = fq->ctx->ingest;
    bool marked = false;
    if (fq->ctx->stream) {
      if (!ip.text_done[fq->pool_slot]) {
        (void)ip.text_done[fq->pool_slot].create(hipEventDisableTiming);
      }
      marked = ip.text_done[fq->pool_slot] && hipEventRecord(ip.text_done[fq->pool_slot], fq->ctx->stream) == hipSuccess;
    }
    if (!marked && fq->ctx->stream) {
      (void)hipStreamSynchronize(fq->ctx->stream);
    }
    ip.text_used[fq->pool_slot] = false;
  } else {
    if (fq->ctx && fq->ctx->stream) {
      (void)hipStreamSynchronize(fq->ctx->stream);
    }
  }
  delete fq;
}

} // extern "C"
