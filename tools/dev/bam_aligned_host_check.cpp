// Developer check of csrc/host/gr_bam.hpp's aligned-BAM parts under the sanitizers, without a device and outside Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dev/bam_aligned_host_check.cpp -o /tmp/bam_aligned_host_check && /tmp/bam_aligned_host_check
// Small record streams with secondary, supplementary and reverse-strand records (the cases of tests/bam_aligned_cases.py:
// a skipped record first, last, two in a row, alone; without bases; with 0xFF qualities): bam_walk with every mask of
// accepted flags over EVERY prefix, each prefix in a heap block of exactly its size, against a walk by the definition; the
// twin decoders, whole and sliced, against the byte-wise definition of the aligned twin.  Then the word functions of the
// device's reversed pack (bam_pack16, bam_shift_nibble, bam_revcomp16) through the loads k_bam_pack makes, every record in
// a block of exactly (l_seq + 1) / 2 bytes, for all lengths 1 .. 80 (both parities) against the 2-bit pack of the twin's
// bases; bam_shift_nibble and bam_revcomp16 for all 16 codes / all four bases at every position.
#include "../../goldrush_amd/csrc/host/gr_bam.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

using namespace gr;

#define CHECK(c)                                                                                                       \
  do {                                                                                                                 \
    if (!(c)) {                                                                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c);                                       \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
  } while (0)

static const char CODES[17] = "=ACMGRSVTWYHKDBN";

struct Src
{
  std::string name, bases; // bases over CODES
  std::vector<uint8_t> quals;
  uint32_t flag, n_cigar;
  std::string tags;
};

static int
code_of(char c)
{
  for (int i = 0; i < 16; ++i) {
    if (CODES[i] == c) {
      return i;
    }
  }
  std::abort();
}

static void
put32(std::string& s, uint32_t v)
{
  for (int i = 0; i < 4; ++i) {
    s.push_back((char)(v >> (8 * i)));
  }
}

static std::string
record(const Src& r, uint32_t pad)
{
  std::string body = r.name;
  body.push_back('\0');
  for (uint32_t i = 0; i < r.n_cigar; ++i) {
    put32(body, 16 * (i + 1));
  }
  for (size_t i = 0; i < r.bases.size(); i += 2) {
    const int lo = i + 1 < r.bases.size() ? code_of(r.bases[i + 1]) : (int)pad;
    body.push_back((char)((code_of(r.bases[i]) << 4) | lo));
  }
  body.append(r.quals.begin(), r.quals.end());
  body += r.tags;
  std::string out;
  put32(out, 32 + (uint32_t)body.size());
  put32(out, 0xFFFFFFFFu); // refID
  put32(out, 0xFFFFFFFFu); // pos
  out.push_back((char)(r.name.size() + 1));
  out.push_back(0);
  out.push_back((char)0x48);
  out.push_back((char)0x12);
  out.push_back((char)(r.n_cigar & 255));
  out.push_back((char)(r.n_cigar >> 8));
  out.push_back((char)(r.flag & 255));
  out.push_back((char)(r.flag >> 8));
  put32(out, (uint32_t)r.bases.size());
  put32(out, 0xFFFFFFFFu);
  put32(out, 0xFFFFFFFFu);
  put32(out, 0);
  return out + body;
}

static char
complement(char c)
{
  static const char comp[17] = "=TGKCYSBAWRDMHVN";
  return comp[code_of(c)];
}

// a block of exactly n bytes (n 0: one byte nobody may read)
static std::unique_ptr<uint8_t[]>
exact(const uint8_t* p, size_t n)
{
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  for (size_t i = 0; i < n; ++i) {
    b[i] = p[i];
  }
  return b;
}

// the walk by the definition (tests/bam_aligned_cases.py: walk)
struct Want
{
  std::vector<uint64_t> offs;
  uint64_t consumed = 0, skipped = 0;
  long bad = -1;
};

static Want
walk_by_definition(const std::string& s, size_t n, bool final, uint32_t accept)
{
  Want w;
  uint64_t pos = 0;
  auto u8 = [&](uint64_t i) { return (uint32_t)(uint8_t)s[i]; };
  auto le32 = [&](uint64_t i) { return u8(i) | (u8(i + 1) << 8) | (u8(i + 2) << 16) | (u8(i + 3) << 24); };
  while (pos < n) {
    if (n - pos < 4) {
      break;
    }
    const uint64_t bs = le32(pos);
    if (bs < 32) {
      w.consumed = pos;
      w.bad = (long)pos;
      return w;
    }
    if (n - pos - 4 < bs) {
      break;
    }
    const uint64_t l_name = u8(pos + 12), n_cig = u8(pos + 16) | (u8(pos + 17) << 8), flag = u8(pos + 18) | (u8(pos + 19) << 8), l_seq = le32(pos + 20);
    if (32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs || l_name == 0 || s[pos + 36 + l_name - 1] != 0 || (flag & 0x910 & ~accept)) {
      w.consumed = pos;
      w.bad = (long)pos;
      return w;
    }
    if (flag & 0x900) {
      ++w.skipped;
    } else {
      w.offs.push_back(pos);
    }
    pos += 4 + bs;
  }
  w.consumed = pos;
  if (final && pos < n) {
    w.bad = (long)pos;
  }
  return w;
}

int
main()
{
  std::mt19937_64 rng(20261020);
  auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
  auto mk = [&](const char* name, const char* bases, uint32_t flag, uint32_t n_cigar = 0, const char* tags = "", int ff = 0) {
    Src r{ name, bases, {}, flag, n_cigar, tags };
    for (size_t i = 0; i < r.bases.size(); ++i) {
      r.quals.push_back(ff ? 0xFF : (uint8_t)below(94));
    }
    return r;
  };
  const Src SEC = mk("sec", "", 0x100, 1), SEC_FF = mk("sec ff", "ACGTA", 0x110, 0, "", 1), SUP = mk("sup", "ACGTNACGT", 0x804, 0, "SAZx"), REV_ODD = mk("rev odd", "ACGTNRYKMSWBDHV=A", 0x10),
            REV_EVEN = mk("rev_even", "AACCGGTTACGTAC", 0x51, 2), REV_ONE = mk("r1", "C", 0x10), REV_NONE = mk("r0", "", 0x10), FWD = mk("fwd", "ACGTACGTAA", 4), FWD2 = mk("fwd2 x", "TTGCA", 0x600);
  const std::vector<std::vector<Src>> streams = { { SEC, FWD, REV_ODD, FWD2 }, { FWD, REV_EVEN, SUP }, { REV_ONE, SEC_FF, SUP, REV_NONE, FWD, SEC, SEC, REV_ODD }, { SEC_FF }, { FWD, FWD2 } };
  const uint32_t accepts[5] = { 0, 0x10, 0x100, 0x800, 0x910 };
  size_t n_walks = 0, n_decoded = 0, n_slices = 0, n_words = 0;
  for (const auto& st : streams) {
    std::string s;
    std::vector<const Src*> by_off_src;
    std::vector<uint64_t> by_off;
    for (const Src& r : st) {
      by_off.push_back(s.size());
      by_off_src.push_back(&r);
      s += record(r, (uint32_t)below(16));
    }
    for (size_t cut = 0; cut <= s.size(); ++cut) {
      const auto buf = exact(reinterpret_cast<const uint8_t*>(s.data()), cut);
      for (const uint32_t accept : accepts) {
        for (int final = 0; final < 2; ++final) {
          const Want want = walk_by_definition(s, cut, final != 0, accept);
          uint64_t used = 0, skipped = 0, bad = 0;
          const char* why = nullptr;
          std::vector<BamRecord> got;
          const int rc = bam_walk(buf.get(), cut, final != 0, accept, &used, &skipped, &bad, &why, [&](const BamRecord& r) {
            got.push_back(r);
            return true;
          });
          ++n_walks;
          CHECK(rc == (want.bad < 0 ? 0 : -1) && used == want.consumed && skipped == want.skipped && got.size() == want.offs.size());
          CHECK(rc == 0 || ((long)bad == want.bad && why));
          for (size_t k = 0; k < got.size(); ++k) {
            const BamRecord& r = got[k];
            CHECK(r.off == want.offs[k] && r.end <= cut);
            const Src* src = nullptr;
            for (size_t j = 0; j < by_off.size(); ++j) {
              src = by_off[j] == r.off ? by_off_src[j] : src;
            }
            CHECK(src && r.l_seq == src->bases.size() && r.flag == src->flag && !(r.flag & 0x900) && (!(r.flag & 0x10) || (accept & 0x10)));
            // the twin's read by the definition
            std::string seq = src->bases;
            std::vector<uint8_t> q = src->quals;
            const bool rev = (r.flag & 0x10) != 0;
            if (rev) {
              seq.assign(src->bases.rbegin(), src->bases.rend());
              for (char& c : seq) {
                c = complement(c);
              }
              q.assign(src->quals.rbegin(), src->quals.rend());
            }
            const uint64_t L = r.l_seq;
            for (uint64_t from = 0; from <= L; ++from) {
              for (uint64_t n = 0; from + n <= L; n += (n < 3 || from + n + 1 > L) ? 1 : L - from - n) { // 0, 1, 2, 3 and the rest
                const auto so = exact(nullptr, 0), qo = exact(nullptr, 0);
                std::unique_ptr<char[]> sb(new char[n ? n : 1]), qb(new char[n ? n : 1]);
                bool ok;
                if (rev) {
                  bam_decode_bases_rev(buf.get() + r.seq_off, L, from, n, sb.get());
                  ok = bam_decode_quals_rev(buf.get() + r.qual_off, L, from, n, qb.get());
                } else {
                  bam_decode_bases(buf.get() + r.seq_off, from, n, sb.get());
                  ok = bam_decode_quals(buf.get() + r.qual_off + from, n, qb.get());
                }
                CHECK(ok);
                for (uint64_t j = 0; j < n; ++j) {
                  CHECK(sb[j] == seq[from + j] && (uint8_t)qb[j] == (uint8_t)(q[from + j] + 33));
                }
                ++n_slices;
              }
            }
            ++n_decoded;
          }
        }
      }
    }
  }
  // ---- the word functions, through the loads of k_bam_pack's reversed form (csrc/grp_ingest.inc) -----------------------
  for (uint32_t n = 1; n <= 80; ++n) {
    for (int round = 0; round < 8; ++round) {
      std::vector<uint8_t> base(n); // A0 C1 G2 T3
      std::vector<uint8_t> bytes((n + 1) / 2, 0);
      for (uint32_t i = 0; i < n; ++i) {
        base[i] = (uint8_t)below(4);
        bytes[i >> 1] |= (uint8_t)((1u << base[i]) << ((i & 1) ? 0 : 4));
      }
      if (n & 1) {
        bytes.back() |= (uint8_t)below(16); // the padding code
      }
      const auto src = exact(bytes.data(), bytes.size());
      const uint32_t nw = (n + 15) / 16;
      for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t cnt = std::min(16u, n - w * 16u);
        const uint32_t s0 = n - w * 16u - cnt;
        const uint8_t* s = src.get() + (s0 >> 1);
        uint64_t x = 0;
        if (cnt == 16u) {
          __builtin_memcpy(&x, s, 8);
          if (s0 & 1u) {
            x = bam_shift_nibble(x, s[8]);
          }
        } else {
          CHECK(s0 == 0);
          for (uint32_t j = 0; j < (cnt + 1u) / 2u; ++j) {
            x |= (uint64_t)s[j] << (8u * j);
          }
        }
        const uint32_t got = bam_revcomp16(bam_pack16(x), cnt);
        uint32_t want = 0;
        for (uint32_t j = 0; j < cnt; ++j) {
          want |= (uint32_t)(3u - base[n - 1 - (16u * w + j)]) << (2u * j);
        }
        CHECK(got == want);
        ++n_words;
      }
    }
  }
  for (uint32_t code = 0; code < 16; ++code) { // bam_shift_nibble moves any code, at every position
    for (uint32_t at = 0; at < 16; ++at) {
      uint8_t nine[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
      const uint32_t nib = at + 1; // the codes begin at the low half of byte 0
      nine[nib >> 1] = (uint8_t)(code << ((nib & 1) ? 0 : 4));
      uint64_t x = 0;
      __builtin_memcpy(&x, nine, 8);
      const uint64_t y = bam_shift_nibble(x, nine[8]);
      uint8_t out[8];
      __builtin_memcpy(out, &y, 8);
      for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t c = (j & 1) ? (out[j >> 1] & 15u) : (uint32_t)(out[j >> 1] >> 4);
        CHECK(c == (j == at ? code : 0u));
      }
    }
  }
  for (uint32_t cnt = 1; cnt <= 16; ++cnt) { // bam_revcomp16: every base at every position of every count
    for (uint32_t at = 0; at < cnt; ++at) {
      for (uint32_t b = 0; b < 4; ++b) {
        uint32_t want = 0;
        for (uint32_t j = 0; j < cnt; ++j) {
          want |= (3u - (j == cnt - 1 - at ? b : 0u)) << (2u * j);
        }
        CHECK(bam_revcomp16(b << (2u * at), cnt) == want);
        CHECK(bam_revcomp16((b << (2u * at)) | (cnt < 16 ? 0xFFFFFFFFu << (2u * cnt) : 0u), cnt) == want); // (what lies behind the count does not matter)
      }
    }
  }
  std::printf("bam_aligned_host_check: %zu walks, %zu records decoded in %zu slices, %zu packed words: ok\n", n_walks, n_decoded, n_slices, n_words);
  return 0;
}
