#include "gr_gzidx.hpp"

#include "gr_fastq.hpp"

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>
#include <zlib.h>

namespace gr {

bool
gzip_index_enabled()
{
  const char* e = getenv("GRP_GZIP_INDEX");
  return !(e && !strcmp(e, "off"));
}

uint64_t
gzip_index_span()
{
  const char* e = getenv("GRP_GZIP_SPAN");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? std::min<uint64_t>((uint64_t)v, uint64_t(1) << 31) : uint64_t(256) << 10;
}

uint64_t
gzip_index_max_bytes()
{
  const char* e = getenv("GRP_GZIP_INDEX_MAX_GB");
  const double v = e ? atof(e) : 0.0;
  return (uint64_t)((v > 0.0 ? std::min(v, 1e6) : 16.0) * (double)(uint64_t(1) << 30));
}

namespace {
// CRC32 arithmetic (the reflected gzip polynomial): a * b modulo the polynomial, and x^(8 n).  zlib's crc32_combine does
// the same with 32 x 32 bit matrices that it builds anew in every call — tens of microseconds, once per segment on the
// reader thread; this is a microsecond.
constexpr uint32_t kPoly = 0xedb88320u;
inline uint32_t
crc_mul(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m != 0; m >>= 1) {
    if (a & m) {
      p ^= b;
    }
    b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}
// crc(A B) = crc(A) x^(8 |B|) + crc(B) (the pre- and post-inversions cancel): what crc(A) contributes to crc(A B)
uint32_t
crc_shift(uint32_t crc, uint64_t n_bytes)
{
  static const std::vector<uint32_t> x2n = [] { // x^(2^k)
    std::vector<uint32_t> t(64);
    t[0] = 1u << 30;
    for (int k = 1; k < 64; ++k) {
      t[k] = crc_mul(t[k - 1], t[k - 1]);
    }
    return t;
  }();
  uint32_t shift = 1u << 31; // x^0
  uint64_t bits = n_bytes * 8;
  for (int k = 0; bits != 0; bits >>= 1, ++k) {
    if (bits & 1u) {
      shift = crc_mul(x2n[k], shift);
    }
  }
  return crc_mul(crc, shift);
}
} // namespace

bool
GzIndex::matches(const std::string& path) const
{
  struct stat st;
  return stat(path.c_str(), &st) == 0 && (uint64_t)st.st_size == file_size && (int64_t)st.st_mtim.tv_sec == mtime_s && (int64_t)st.st_mtim.tv_nsec == mtime_ns;
}

uint8_t*
GzIndex::reserve(uint32_t n, uint64_t* at)
{
  if (used_ + n > kBlock) {
    store_.emplace_back(new uint8_t[kBlock]);
    used_ = 0;
  }
  *at = (uint64_t)(store_.size() - 1) * kBlock + used_;
  return store_.back().get() + used_;
}

GzIndexReader::GzIndexReader(const std::string& path, uint64_t span, uint64_t max_bytes)
  : path_(path)
  , span_(std::max<uint64_t>(span, 1))
  , max_bytes_(max_bytes)
{
  fd_ = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd_ < 0) {
    return;
  }
  idx_.reset(new GzIndex);
  struct stat st;
  if (fstat(fd_, &st) == 0) {
    idx_->file_size = (uint64_t)st.st_size;
    idx_->mtime_s = (int64_t)st.st_mtim.tv_sec;
    idx_->mtime_ns = (int64_t)st.st_mtim.tv_nsec;
  } else {
    drop();
  }
  z_stream* z = new z_stream;
  memset(z, 0, sizeof *z);
  if (inflateInit2(z, 31) != Z_OK) { // gzip members, their headers and trailers checked by zlib
    delete z;
    return;
  }
  z_ = z;
  in_.resize(size_t(1) << 20);
}

GzIndexReader::~GzIndexReader()
{
  if (z_) {
    inflateEnd(static_cast<z_stream*>(z_));
    delete static_cast<z_stream*>(z_);
  }
  if (fd_ >= 0) {
    ::close(fd_);
  }
}

void
GzIndexReader::drop()
{
  indexing_ = false;
  idx_.reset();
}

void
GzIndexReader::fail(const std::string& what)
{
  note_input_failure("reading " + path_ + " failed: " + what);
  failed_ = done_ = true;
  drop();
}

std::unique_ptr<GzIndex>
GzIndexReader::take()
{
  if (!complete_ || !indexing_) {
    return nullptr;
  }
  indexing_ = false;
  return std::move(idx_);
}

// the input not consumed yet moves to the front of the buffer, the rest of the buffer is read; false: no byte came
bool
GzIndexReader::fill()
{
  z_stream& z = *static_cast<z_stream*>(z_);
  if (z.avail_in && z.next_in != in_.data()) {
    memmove(in_.data(), z.next_in, z.avail_in);
  }
  z.next_in = in_.data();
  size_t got = 0;
  while (!file_end_ && got == 0) {
    const ssize_t r = ::read(fd_, in_.data() + z.avail_in, in_.size() - z.avail_in);
    if (r < 0 && errno == EINTR) {
      continue;
    }
    if (r < 0) {
      fail(std::string("at byte ") + std::to_string(in_pos_ + z.avail_in) + ": " + strerror(errno));
      return false;
    }
    if (r == 0) {
      file_end_ = true;
    }
    got = (size_t)r;
  }
  z.avail_in += (uInt)got;
  return got != 0;
}

void
GzIndexReader::commit(uint64_t end_bit, uint32_t crc_now, uint32_t flags)
{
  GzIndex& ix = *idx_;
  const uint64_t text = member_text_ - cur_text0_;
  if (text == 0 || text > 0xffff0000ull) { // (never empty; the engine takes 32-bit lengths)
    drop();
    return;
  }
  cur_.n_bits = end_bit - cur_.comp_bit;
  cur_.text_len = (uint32_t)text;
  // zlib keeps the CRC32 of the member's text so far: crc(A B) = crc(A) x^(8 |B|) + crc(B), so B's comes without reading B again
  cur_.crc32 = crc_now ^ crc_shift(cur_crc0_, text);
  cur_.flags = flags;
  ix.segs.push_back(cur_);
  ix.text_bytes += text;
  ix.max_text = std::max(ix.max_text, text);
  ix.max_comp = std::max(ix.max_comp, cur_.end_byte() - cur_.first_byte());
  ++member_segs_;
  if (ix.bytes() > max_bytes_) {
    drop();
  }
}

// inflate() has come back in front of a block's header (or behind a member's header)
void
GzIndexReader::on_boundary()
{
  if (!indexing_) {
    return;
  }
  z_stream& z = *static_cast<z_stream*>(z_);
  const uint64_t bit = in_pos_ * 8 - (uint64_t)(z.data_type & 63); // that many bits of the last byte belong to what follows
  const bool behind_final = (z.data_type & 64) != 0;
  const uint32_t crc_now = (uint32_t)z.adler;
  GzIndex& ix = *idx_;
  if (!open_) { // behind the member's header
    if (behind_final || member_text_ != 0 || (z.data_type & 63) != 0) {
      drop(); // (not what zlib is known to do)
      return;
    }
    cur_ = GzSegment{ bit, 0, 0, 0, 0, 0, 0 };
    cur_text0_ = 0;
    cur_crc0_ = crc_now;
    cur_blocks0_ = ix.store_.size();
    cur_used0_ = ix.used_;
    member_segs_ = 0;
    open_ = true;
    return;
  }
  if (behind_final) { // the member's end closes the segment
    if (member_text_ != cur_text0_) {
      commit(bit, crc_now, GRP_GZIP_SEG_FINAL);
    } else if (member_segs_ != 0) {
      // blocks without text behind the last point: they belong to the segment in front of it, the point is forgotten
      GzSegment& g = ix.segs.back();
      g.n_bits = bit - g.comp_bit;
      g.flags = GRP_GZIP_SEG_FINAL;
      ix.max_comp = std::max(ix.max_comp, g.end_byte() - g.first_byte());
      ix.store_.resize(cur_blocks0_);
      ix.used_ = cur_used0_;
    } // (else: a member without text has no segment)
    open_ = false;
    return;
  }
  if (member_text_ - cur_text0_ < span_) {
    return;
  }
  commit(bit, crc_now, 0);
  if (!indexing_) {
    return;
  }
  cur_blocks0_ = ix.store_.size();
  cur_used0_ = ix.used_;
  uint64_t at = 0;
  uint8_t* d = ix.reserve(32768, &at);
  uInt len = 0;
  if (inflateGetDictionary(&z, d, &len) != Z_OK || len > 32768 || len != std::min<uint64_t>(member_text_, 32768)) {
    drop();
    return;
  }
  ix.used_ += len;
  cur_ = GzSegment{ bit, 0, at, (uint32_t)len, 0, 0, 0 };
  cur_text0_ = member_text_;
  cur_crc0_ = crc_now;
}

size_t
GzIndexReader::read(char* dst, size_t n)
{
  if (!ok()) {
    return 0;
  }
  z_stream& z = *static_cast<z_stream*>(z_);
  size_t got = 0;
  while (got < n && !done_) {
    if (z.avail_in == 0 && !file_end_) {
      fill();
      if (done_) {
        break;
      }
    }
    if (between_) {
      // behind a member: another one (gzread looks for the two magic bytes), the end of the file, or bytes that are no
      // member, which gzread ignores
      if (z.avail_in < 2 && !file_end_) {
        fill();
        if (done_) {
          break;
        }
        continue;
      }
      if (z.avail_in >= 2 && z.next_in[0] == 0x1f && z.next_in[1] == 0x8b) {
        if (inflateReset(&z) != Z_OK) {
          fail("zlib could not be reset");
          break;
        }
        between_ = false;
        member_text_ = 0;
        open_ = false;
        continue;
      }
      done_ = true;
      if (z.avail_in == 0) {
        complete_ = indexing_;
      } else {
        drop(); // the input ends here as it does for gzread; every pass over such a file stays with zlib
      }
      break;
    }
    if (z.avail_in == 0) { // (the file has ended inside a member)
      fail("the compressed stream ends early (truncated gzip data)");
      break;
    }
    z.next_out = reinterpret_cast<Bytef*>(dst + got);
    z.avail_out = (uInt)std::min<size_t>(n - got, size_t(1) << 30);
    const uInt in0 = z.avail_in, out0 = z.avail_out;
    const int rc = inflate(&z, Z_BLOCK);
    in_pos_ += in0 - z.avail_in;
    got += out0 - z.avail_out;
    member_text_ += out0 - z.avail_out;
    if (rc == Z_STREAM_END) {
      if (open_) { // (the boundary behind the final block was not reported: not what zlib is known to do)
        drop();
        open_ = false;
      }
      between_ = true;
      continue;
    }
    if (rc == Z_BUF_ERROR) { // no progress was possible: more input (above) or more room (the caller's next request)
      continue;
    }
    if (rc != Z_OK) {
      fail(std::string(z.msg ? z.msg : "zlib error"));
      break;
    }
    if (z.data_type & 128) {
      on_boundary();
    }
  }
  return got;
}

} // namespace gr
