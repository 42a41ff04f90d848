#include "gr_fastq.hpp"
#include "gr_bam.hpp"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <zlib.h>

namespace gr {

// A plain regular file is read with pread: large requests are cut into slices that several
// threads copy out of the page cache at once (one thread moves ~6 GB/s, the GPU ingest
// behind it parses > 20 GB/s).  Everything else — gzip data, pipes — goes through zlib.
InputFile::InputFile(const std::string& path)
{
  path_ = path;
  const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd >= 0) {
    struct stat st;
    unsigned char magic[2] = { 0, 0 };
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && !getenv("GRP_ZLIB_READER")) {
      const ssize_t k = pread(fd, magic, 2, 0);
      if (k >= 0 && !(k == 2 && magic[0] == 0x1f && magic[1] == 0x8b)) {
        fd_ = fd;
        size_ = (uint64_t)st.st_size;
        opened_ = true;
        return;
      }
    }
    ::close(fd);
  }
  gzFile f = gzopen(path.c_str(), "rb");
  if (f) {
    gzbuffer(f, 1u << 20);
  }
  f_ = f;
  opened_ = f != nullptr;
}

InputFile::InputFile(const std::string& path, int gz_fd)
{
  path_ = path;
  gzFile f = gzdopen(gz_fd, "rb");
  if (f) {
    gzbuffer(f, 1u << 20);
  } else {
    ::close(gz_fd);
  }
  f_ = f;
  opened_ = f != nullptr;
}

InputFile::~InputFile()
{
  if (f_) {
    gzclose(static_cast<gzFile>(f_));
  }
  if (fd_ >= 0) {
    ::close(fd_);
  }
}

namespace {
std::mutex g_fail_mu;
std::string g_fail_what;
bool g_failed = false;
} // namespace

void
note_input_failure(const std::string& what)
{
  std::lock_guard<std::mutex> g(g_fail_mu);
  if (!g_failed) {
    g_failed = true;
    g_fail_what = what;
  }
}

bool
input_failed(std::string* what)
{
  std::lock_guard<std::mutex> g(g_fail_mu);
  if (g_failed && what) {
    *what = g_fail_what;
  }
  return g_failed;
}

void
clear_input_failure()
{
  std::lock_guard<std::mutex> g(g_fail_mu);
  g_failed = false;
  g_fail_what.clear();
}

void
note_bam_failure(const std::string& path, uint64_t off, const char* why)
{
  note_input_failure("reading " + path + " failed: BAM record at byte " + std::to_string(off) + " of the decompressed stream: " + (why ? why : "refused"));
}

int
input_format(const unsigned char* head, size_t n)
{
  if (n >= 4 && !memcmp(head, "BAM\1", 4)) {
    return 2;
  }
  return n >= 1 && head[0] == '@' ? 1 : 0;
}

size_t
pread_full(int fd, void* dst, size_t want, uint64_t off, int* err)
{
  *err = 0;
  size_t k = 0;
  while (k < want) {
    const ssize_t r = pread(fd, static_cast<char*>(dst) + k, want - k, (off_t)(off + k));
    if (r < 0 && errno == EINTR) {
      continue;
    }
    if (r <= 0) {
      *err = r < 0 ? errno : 0;
      break;
    }
    k += (size_t)r;
  }
  return k;
}

FileProbe
probe_file(const std::string& path)
{
  FileProbe p;
  const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  p.opened = fd >= 0;
  p.err = p.opened ? 0 : errno;
  struct stat st;
  if (p.opened && fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
    p.regular = true;
    p.size = (uint64_t)st.st_size;
    unsigned char head[4];
    const size_t k = pread_full(fd, head, sizeof(head), 0, &p.err);
    p.magic = k < 2 ? FileProbe::NONE : (head[0] == 0x1f && head[1] == 0x8b) ? FileProbe::GZIP : input_format(head, k) == 2 ? FileProbe::BAM : FileProbe::OTHER;
  }
  if (p.opened) {
    ::close(fd);
  }
  return p;
}

size_t
InputFile::read(char* dst, size_t n)
{
  if (fd_ >= 0) {
    constexpr size_t kSlice = size_t(16) << 20;
    static const size_t max_threads = [] { // GRP_READ_THREADS: threads copying one request out of the page cache (default 8)
      const char* e = getenv("GRP_READ_THREADS");
      const long v = e ? atol(e) : 0;
      return (size_t)(v > 0 ? std::min(v, 64l) : 8l);
    }();
    size_t threads = std::min<size_t>(n / kSlice, std::min<size_t>(max_threads, std::max(1u, std::thread::hardware_concurrency())));
    size_t got = 0;
    int err = 0;
    if (threads < 2) {
      got = pread_full(fd_, dst, n, off_, &err);
    } else {
      // slice i covers [i * per, (i + 1) * per); the data ends in the first short slice
      const size_t per = (n + threads - 1) / threads;
      std::vector<size_t> part(threads, 0);
      std::vector<int> errs(threads, 0);
      std::vector<std::thread> pool;
      for (size_t i = 1; i < threads; ++i) {
        pool.emplace_back([&, i] { part[i] = pread_full(fd_, dst + i * per, std::min(per, n - i * per), off_ + i * per, &errs[i]); });
      }
      part[0] = pread_full(fd_, dst, per, off_, &errs[0]);
      for (auto& t : pool) {
        t.join();
      }
      for (size_t i = 0; i < threads; ++i) {
        got += part[i];
        if (part[i] < std::min(per, n - i * per)) {
          err = errs[i];
          break;
        }
      }
    }
    // the size is known: a read that failed, or data that ends in front of it, is an error and not the end of the input
    const uint64_t want = std::min<uint64_t>(n, size_ > off_ ? size_ - off_ : 0);
    if (err != 0 || got < want) {
      note_input_failure("reading " + path_ + " failed at byte " + std::to_string(off_ + got) + " of " + std::to_string(size_) + ": " + (err ? strerror(err) : "the file ends early"));
    }
    off_ += got;
    return got;
  }
  size_t got = 0;
  while (f_ && got < n) { // gzread takes an unsigned length
    const unsigned want = (unsigned)std::min<size_t>(n - got, 1u << 30);
    const int r = gzread(static_cast<gzFile>(f_), dst + got, want);
    if (r < 0) {
      int zerr = 0;
      const char* msg = gzerror(static_cast<gzFile>(f_), &zerr);
      note_input_failure("reading " + path_ + " failed: " + (msg ? msg : "zlib error"));
      break;
    }
    if (r == 0) {
      // the end of the data — or of a gzip member that was cut off: zlib hands out what it could inflate and then
      // reports 0 bytes like at a proper end.  gzerror says Z_BUF_ERROR when the cut was met inside this
      // call, gzclose_r when an earlier call swallowed it; a stream that did not end on a complete member is an error.
      int zerr = 0;
      const char* msg = gzerror(static_cast<gzFile>(f_), &zerr);
      const std::string why = (zerr != Z_OK && msg && *msg) ? msg : "";
      const int rc = gzclose_r(static_cast<gzFile>(f_));
      f_ = nullptr;
      if (zerr != Z_OK || rc != Z_OK) {
        note_input_failure("reading " + path_ + " failed: " + (why.empty() ? "the compressed stream ends early (truncated gzip data)" : why));
      }
      break;
    }
    got += (size_t)r;
  }
  return got;
}

int
InputFile::peek()
{
  if (fd_ >= 0) {
    unsigned char c;
    return pread(fd_, &c, 1, (off_t)off_) == 1 ? (int)c : -1;
  }
  if (!f_) {
    return -1;
  }
  const int c = gzgetc(static_cast<gzFile>(f_));
  if (c >= 0) {
    gzungetc(c, static_cast<gzFile>(f_));
  }
  return c;
}

FastqStream::FastqStream(const std::string& path, uint32_t bam_accept)
  : path_(path)
  , bam_accept_(bam_accept)
  , in_(path)
{
  buf_.resize(size_t(8) << 20);
}

FastqStream::~FastqStream() {}

bool
FastqStream::fill()
{
  if (eof_ || !in_.ok()) {
    return false;
  }
  // keep the unread tail, refill the rest
  const size_t tail = end_ - pos_;
  if (tail && pos_) {
    memmove(buf_.data(), buf_.data() + pos_, tail);
  }
  pos_ = 0;
  end_ = tail;
  if (end_ == buf_.size()) {
    buf_.resize(buf_.size() * 2); // a single line longer than the buffer
  }
  const size_t got = in_.read(buf_.data() + end_, buf_.size() - end_);
  if (got == 0) {
    eof_ = true;
    return false;
  }
  end_ += got;
  return true;
}

bool
FastqStream::is_fastq()
{
  if (format_ < 0) {
    while (end_ - pos_ < 4 && fill()) {
    }
    format_ = input_format(reinterpret_cast<const unsigned char*>(buf_.data()) + pos_, end_ - pos_);
  }
  return format_ != 0;
}

// The records of a BAM stream as the records of its FASTQ twin: the shared walk over what the buffer holds, every record
// decoded into the batch.  A refused record, or a stream that ends inside the header or a record, is an input failure.
bool
FastqStream::next_batch_bam(RecordBatch& out, size_t max_records, size_t max_bases)
{
  while (!stopped_ && out.rec.size() < max_records && out.bases < max_bases) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(buf_.data()) + pos_;
    if (!bam_header_done_) {
      uint64_t hb = 0;
      const int rc = bam_header(p, end_ - pos_, &hb);
      if (rc == 0 && fill()) {
        continue;
      }
      if (rc != 1) {
        note_bam_failure(path_, stream_off_, rc == 0 ? "the stream ends inside the BAM header (truncated)" : "not a BAM header");
        stopped_ = true;
        break;
      }
      pos_ += hb;
      stream_off_ += hb;
      bam_header_done_ = true;
      continue;
    }
    uint64_t used = 0, bad = 0, skipped = 0;
    const char* why = nullptr;
    bool full = false;
    int rc = bam_walk(p, end_ - pos_, eof_, bam_accept_, &used, &skipped, &bad, &why, [&](const BamRecord& b) {
      if (out.rec.size() >= max_records || out.bases >= max_bases) {
        full = true;
        return false;
      }
      RecordRef r{};
      r.id_off = out.text.size();
      r.id_len = bam_id_len(p + b.name_off, b.l_read_name);
      out.text.insert(out.text.end(), p + b.name_off, p + b.name_off + r.id_len);
      out.text.push_back('\0');
      r.seq_off = out.text.size();
      r.seq_len = r.qual_len = b.l_seq;
      out.text.resize(r.seq_off + 2 * (size_t)b.l_seq + 2, '\0');
      r.qual_off = r.seq_off + b.l_seq + 1;
      const bool reversed = (b.flag & BAM_FLAG_REVERSE) != 0; // (accepted, or the walk had refused it: the twin's orientation)
      bool quals_ok;
      if (reversed) {
        bam_decode_bases_rev(p + b.seq_off, b.l_seq, 0, b.l_seq, out.text.data() + r.seq_off);
        quals_ok = bam_decode_quals_rev(p + b.qual_off, b.l_seq, 0, b.l_seq, out.text.data() + r.qual_off);
      } else {
        bam_decode_bases(p + b.seq_off, 0, b.l_seq, out.text.data() + r.seq_off);
        quals_ok = bam_decode_quals(p + b.qual_off, b.l_seq, out.text.data() + r.qual_off);
      }
      if (!quals_ok) {
        out.text.resize(r.id_off);
        bad = b.off;
        why = "a quality without a FASTQ character (absent: 0xFF, or above 93)";
        full = true;
        return false;
      }
      out.rec.push_back(r);
      out.bases += r.seq_len;
      bam_reversed_ += reversed ? 1 : 0;
      return true;
    });
    if (rc == 0 && why) {
      rc = -1;
    }
    if (rc != 0) {
      note_bam_failure(path_, stream_off_ + bad, why);
      stopped_ = true;
      break;
    }
    bam_skipped_ += skipped;
    pos_ += used;
    stream_off_ += used;
    if (full || eof_) {
      if (eof_ && !full) {
        stopped_ = true;
      }
      break;
    }
    if (!fill() && pos_ == end_) { // (a tail at the end of the data: walked once more, as the final one)
      stopped_ = true;
      break;
    }
  }
  return !out.rec.empty();
}

bool
FastqStream::get_line(const char*& p, size_t& n)
{
  for (;;) {
    const char* start = buf_.data() + pos_;
    const char* nl = (const char*)memchr(start, '\n', end_ - pos_);
    if (nl) {
      p = start;
      n = (size_t)(nl - start);
      pos_ += n + 1;
      break;
    }
    if (!fill()) {
      if (pos_ == end_) {
        return false;
      }
      p = buf_.data() + pos_; // last line without newline
      n = end_ - pos_;
      pos_ = end_;
      break;
    }
  }
  while (n > 0 && (p[n - 1] == '\r' || p[n - 1] == ' ' || p[n - 1] == '\t')) {
    --n;
  }
  return true;
}

bool
FastqStream::next_batch(RecordBatch& out, size_t max_records, size_t max_bases)
{
  out.clear();
  if (is_fastq() && format_ == 2) {
    return next_batch_bam(out, max_records, max_bases);
  }
  while (!stopped_ && out.rec.size() < max_records && out.bases < max_bases) {
    const char* p;
    size_t n;
    // get_line pointers die at the next refill, so each line is copied at once
    if (!get_line(p, n)) {
      break;
    }
    if (n == 0 || p[0] != '@') {
      stopped_ = true; // not a FASTQ header: stop like a reader at end of input, for good
      break;           // (grp_fastq_parse latches the same state: both sources see the same records)
    }
    RecordRef r{};
    size_t idn = 0;
    while (1 + idn < n && !isspace((unsigned char)p[1 + idn])) {
      ++idn;
    }
    r.id_off = out.text.size();
    r.id_len = idn;
    out.text.insert(out.text.end(), p + 1, p + 1 + idn);
    out.text.push_back('\0');
    if (!get_line(p, n)) {
      out.text.resize(r.id_off);
      break;
    }
    r.seq_off = out.text.size();
    r.seq_len = n;
    out.text.insert(out.text.end(), p, p + n);
    out.text.push_back('\0');
    for (size_t i = 0; i < n; ++i) {
      char& c = out.text[r.seq_off + i];
      if (c >= 'a' && c <= 'z') {
        c = (char)(c - 32);
      }
    }
    if (!get_line(p, n) || !get_line(p, n)) { // '+' line, then qualities
      out.text.resize(r.id_off);
      break;
    }
    r.qual_off = out.text.size();
    r.qual_len = n;
    out.text.insert(out.text.end(), p, p + n);
    out.text.push_back('\0');
    out.rec.push_back(r);
    out.bases += r.seq_len;
  }
  return !out.rec.empty();
}

} // namespace gr
