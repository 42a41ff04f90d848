#include "gr_gzwalk.hpp"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

namespace gr {

int
gzip_walk_switch()
{
  const char* e = getenv("GRP_GZIP_WALK");
  return !e || !strcmp(e, "off") ? 0 : !strcmp(e, "on") ? 1 : -1;
}

GzWalkSizes
gzip_walk_sizes()
{
  GzWalkSizes s;
  if (const char* e = getenv("GRP_GZIP_WALK_ROOM")) {
    unsigned long long v[3] = { 0, 0, 0 };
    const int k = sscanf(e, "%llu,%llu,%llu", &v[0], &v[1], &v[2]);
    s.room = k >= 1 && v[0] ? v[0] : s.room;
    s.window = k >= 2 && v[1] ? v[1] : s.window;
    s.cap = k >= 3 && v[2] ? v[2] : s.cap;
  }
  constexpr uint64_t most = uint64_t(1) << 30; // (a step's room is a 32-bit number, a launch takes 4 GiB of compressed bytes)
  s.room = std::min(std::max<uint64_t>(s.room, 2), most);
  s.window = std::min(std::max<uint64_t>(s.window, 8), most);
  s.cap = std::min(std::max(s.cap, std::max(s.room, s.window)), most);
  return s;
}

long
gzip_header_bytes(const uint8_t* b, size_t n)
{
  if (n >= 1 && b[0] != 0x1f) {
    return -1;
  }
  if (n >= 2 && b[1] != 0x8b) {
    return -1;
  }
  if (n < 10) {
    return 0;
  }
  const unsigned flg = b[3];
  if (b[2] != 8 || (flg & 0xe0)) { // zlib: "unknown compression method", "unknown header flags set"
    return -1;
  }
  size_t p = 10;
  if (flg & 4) { // FEXTRA
    if (p + 2 > n) {
      return 0;
    }
    p += 2 + ((size_t)b[p] | (size_t)b[p + 1] << 8);
    if (p > n) {
      return 0;
    }
  }
  for (const unsigned f : { 8u, 16u }) { // FNAME, FCOMMENT: up to a NUL
    if (flg & f) {
      const void* z = memchr(b + p, 0, n - p);
      if (!z) {
        return 0;
      }
      p = (size_t)(static_cast<const uint8_t*>(z) - b) + 1;
    }
  }
  if (flg & 2) { // FHCRC: the low half of the CRC32 of the header in front of it
    if (p + 2 > n) {
      return 0;
    }
    const uint32_t c = (uint32_t)crc32(crc32(0L, Z_NULL, 0), b, (uInt)p) & 0xffffu;
    if (c != ((uint32_t)b[p] | (uint32_t)b[p + 1] << 8)) {
      return -1;
    }
    p += 2;
  }
  return (long)p;
}

namespace {

// n bytes at `off` of the file, which is opened for this read alone: a walk may have more files than a process may have
// descriptors.  The bytes read; *err != 0: an error
size_t
read_at(const std::string& path, uint8_t* to, size_t n, uint64_t off, int* err)
{
  *err = 0;
  const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    *err = errno ? errno : EIO;
    return 0;
  }
  size_t got = 0;
  while (got < n) {
    const ssize_t r = ::pread(fd, to + got, n - got, (off_t)(off + got));
    if (r < 0 && errno == EINTR) {
      continue;
    }
    if (r < 0) {
      *err = errno ? errno : EIO;
      break;
    }
    if (r == 0) {
      break;
    }
    got += (size_t)r;
  }
  ::close(fd);
  return got;
}

} // namespace

class GzWalker
{
public:
  GzWalker(const std::vector<std::string>& paths, uint64_t span, uint64_t max_bytes, const GzWalkSizes& sizes)
    : span_(std::max<uint64_t>(span, 1))
    , max_bytes_(max_bytes)
    , sizes_(sizes)
    , files_(paths.size())
  {
    for (size_t i = 0; i < paths.size(); ++i) {
      File& f = files_[i];
      f.path = paths[i];
      f.room = sizes_.room;
      f.window = sizes_.window;
      f.hist.resize(32768);
      struct stat st;
      if (stat(f.path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
        f.left = "it cannot be read as a regular file";
        f.unreadable = true;
        continue;
      }
      f.size = (uint64_t)st.st_size;
      f.ix.reset(new GzIndex);
      f.ix->file_size = f.size;
      f.ix->mtime_s = (int64_t)st.st_mtim.tv_sec;
      f.ix->mtime_ns = (int64_t)st.st_mtim.tv_nsec;
      begin_member(f, 0);
    }
  }

  void run(const GzWalkLaunch& launch, GzWalkStats& stats, const GzWalkBuffer& pin, const GzWalkBuffer& unpin)
  {
    std::vector<File*> active;
    for (File& f : files_) {
      if (!f.left && !f.done) {
        active.push_back(&f);
      }
    }
    // the window buffer once, for the first windows of all files; it grows only where a step is repeated with more
    size_t cap = 0;
    for (const File* f : active) {
      cap += (size_t)((f->window + 7) & ~uint64_t(7));
    }
    buf_.resize(cap + 8);
    if (pin && !active.empty()) {
      pin(buf_.data(), buf_.size());
    }
    bool pinned = pin && !active.empty();
    std::vector<grp_gzip_walk_step> steps;
    std::vector<grp_gzip_walk_result> res;
    std::vector<uint8_t> dict, hist_out;
    while (!active.empty()) {
      ++stats.rounds;
      for (size_t first = 0; first < active.size();) {
        // one launch: the files from `first` on that fit its limits (all of them, but for very many or very large windows):
        // 4 GiB of histories at 32 KiB a step are 2^17 steps, the compressed bytes and the rooms as the engine bounds them
        size_t n = 0;
        uint64_t n_comp = 0, rooms = 0;
        for (; first + n < active.size() && n < (size_t(1) << 17); ++n) {
          const File& f = *active[first + n];
          if (n != 0 && (n_comp + f.window > (uint64_t(1) << 31) || rooms + f.room > (uint64_t(1) << 33))) {
            break;
          }
          n_comp += (f.window + 7) & ~uint64_t(7);
          rooms += f.room;
        }
        if (n_comp + 8 > buf_.size()) {
          if (pinned && unpin) {
            unpin(buf_.data(), buf_.size());
          }
          buf_.resize((size_t)n_comp + 8);
          if (pinned) {
            pin(buf_.data(), buf_.size());
          }
        }
        steps.assign(n, grp_gzip_walk_step{});
        res.assign(n, grp_gzip_walk_result{});
        dict.resize(n * 32768);
        hist_out.resize(n * 32768);
        uint64_t slot = 0;
        for (size_t k = 0; k < n; ++k) {
          File& f = *active[first + k];
          const uint64_t byte0 = f.bit >> 3, phase = f.bit & 7;
          const uint64_t want = byte0 < f.size ? std::min(f.window, f.size - byte0) : 0;
          int err = 0;
          const uint64_t got = want ? read_at(f.path, buf_.data() + slot, (size_t)want, byte0, &err) : 0;
          f.at_eof = err == 0 && byte0 + got >= f.size; // (a read that failed: the step runs out of bytes in front of the end)
          f.read_failed = err != 0;
          const uint64_t n_bits = got * 8 > phase ? got * 8 - phase : 0;
          memcpy(dict.data() + k * 32768, f.hist.data(), f.hist_len);
          const uint64_t target = std::max<uint64_t>(1, std::min(span_ - f.seg_text, std::min(sizes_.room / 2, f.room)));
          steps[k] = grp_gzip_walk_step{ slot * 8 + (n_bits ? phase : 0), n_bits, (uint64_t)k * 32768, f.hist_len, (uint32_t)target, (uint32_t)f.room, 0 };
          slot += (f.window + 7) & ~uint64_t(7);
        }
        ++stats.launches;
        if (!launch(buf_.data(), slot, dict.data(), dict.size(), steps.data(), (uint32_t)n, res.data(), hist_out.data())) {
          for (File* f : active) {
            f->left = "a launch of the walk failed";
          }
          break;
        }
        for (size_t k = 0; k < n; ++k) {
          answer(*active[first + k], res[k], hist_out.data() + k * 32768, stats);
        }
        first += n;
      }
      active.erase(std::remove_if(active.begin(), active.end(), [](const File* f) { return f->left || f->done; }), active.end());
    }
    if (pinned && unpin) {
      unpin(buf_.data(), buf_.size());
    }
  }

  std::vector<GzWalkFile> take()
  {
    std::vector<GzWalkFile> out(files_.size());
    for (size_t i = 0; i < files_.size(); ++i) {
      File& f = files_[i];
      if (f.done && !f.left) {
        out[i].index = std::move(f.ix);
      } else {
        out[i].left = f.left ? f.left : "the walk did not come to its end";
        out[i].status = f.status;
        out[i].unreadable = f.unreadable;
      }
    }
    return out;
  }

private:
  struct File
  {
    std::string path;
    uint64_t size = 0;
    std::unique_ptr<GzIndex> ix;
    const char* left = nullptr; // why the file is left to zlib
    uint32_t status = 0;
    bool unreadable = false;    // ... because it is no regular file that can be looked at
    bool done = false;          // the last member's trailer ended the file
    uint64_t bit = 0;           // the block boundary the next step starts at, in the file
    uint64_t room = 0, window = 0;
    bool at_eof = false, read_failed = false; // of the window of the step under way
    // the member being walked: its text and CRC32 so far, its segments; the open segment (begun at a point, not closed
    // yet: a segment may take several steps) with the history at its point; the history at `bit`
    uint64_t member_text = 0;
    uint32_t member_crc = 0;
    size_t member_segs = 0;
    GzSegment cur{};
    uint64_t seg_text = 0;
    uint32_t seg_crc = 0;
    std::vector<uint8_t> seg_dict, hist;
    uint32_t hist_len = 0;
  };

  // the header of the member at byte `at`: the point behind it
  void begin_member(File& f, uint64_t at)
  {
    std::vector<uint8_t> head;
    long h = 0;
    for (size_t n = size_t(1) << 12; h == 0; n *= 16) {
      head.resize((size_t)std::min<uint64_t>(n, f.size - at));
      int err = 0;
      const size_t got = read_at(f.path, head.data(), head.size(), at, &err);
      h = err ? -1 : gzip_header_bytes(head.data(), got);
      if (h == 0 && (at + got >= f.size || got < head.size() || n > (size_t(1) << 28))) {
        h = -1; // (the file ends inside the header)
      }
    }
    if (h < 0) {
      f.left = "a member's header is not one zlib takes";
      return;
    }
    f.bit = (at + (uint64_t)h) * 8;
    f.member_text = 0;
    f.member_crc = 0;
    f.member_segs = 0;
    f.hist_len = 0;
    point(f);
  }

  // a restart point at f.bit, with the history there
  void point(File& f)
  {
    f.cur = GzSegment{ f.bit, 0, 0, f.hist_len, 0, 0, 0 };
    f.seg_dict.assign(f.hist.begin(), f.hist.begin() + f.hist_len);
    f.seg_text = 0;
    f.seg_crc = 0;
  }

  // the open segment ends at f.bit (GzIndexReader::commit)
  void commit(File& f, uint32_t flags)
  {
    GzIndex& ix = *f.ix;
    if (f.seg_text == 0 || f.seg_text > 0xffff0000ull) { // (never empty; the engine takes 32-bit lengths)
      f.left = "a segment of more than 4 GiB - 64 KiB of text";
      return;
    }
    f.cur.n_bits = f.bit - f.cur.comp_bit;
    f.cur.text_len = (uint32_t)f.seg_text;
    f.cur.crc32 = f.seg_crc;
    f.cur.flags = flags;
    if (f.cur.dict_len) {
      uint8_t* d = ix.reserve(32768, &f.cur.dict_at);
      memcpy(d, f.seg_dict.data(), f.cur.dict_len);
      ix.used_ += f.cur.dict_len;
    }
    ix.segs.push_back(f.cur);
    ix.text_bytes += f.seg_text;
    ix.max_text = std::max(ix.max_text, f.seg_text);
    ix.max_comp = std::max(ix.max_comp, f.cur.end_byte() - f.cur.first_byte());
    ++f.member_segs;
    if (ix.bytes() > max_bytes_) {
      f.left = "the index grew beyond its cap";
    }
  }

  // behind the final block at f.bit: the trailer, then another member, the end of the file, or bytes that are no member
  void end_member(File& f)
  {
    const uint64_t at = (f.bit + 7) >> 3;
    uint8_t t[10];
    int err = 0;
    const size_t got = at + 8 <= f.size ? read_at(f.path, t, (size_t)std::min<uint64_t>(10, f.size - at), at, &err) : 0;
    if (got < 8 || err) {
      f.left = "the file ends inside a member's trailer";
      return;
    }
    const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    if (crc != f.member_crc || isize != (uint32_t)f.member_text) {
      f.left = "a member's trailer does not match its text";
      return;
    }
    if (at + 8 == f.size) {
      f.done = true;
    } else if (got == 10 && t[8] == 0x1f && t[9] == 0x8b) {
      begin_member(f, at + 8);
    } else {
      f.left = "bytes behind the last member that are no member"; // (gzread ignores them; every pass over such a file stays with zlib)
    }
  }

  void answer(File& f, const grp_gzip_walk_result& r, const uint8_t* hist, GzWalkStats& stats)
  {
    if (r.status == GRP_GZIP_WALK_NO_ROOM || (r.status == GRP_GZIP_WALK_INPUT_ENDS && !f.at_eof && !f.read_failed)) {
      // the step is repeated with both doubled
      if ((r.status == GRP_GZIP_WALK_NO_ROOM ? f.room : f.window) >= sizes_.cap) {
        f.left = "a block needs more room or more compressed bytes than the cap";
        f.status = r.status;
        return;
      }
      f.room = std::min(2 * f.room, sizes_.cap);
      f.window = std::min(2 * f.window, sizes_.cap);
      ++stats.repeats;
      return;
    }
    if (r.status != 0) {
      f.left = f.read_failed ? "the file could not be read" : r.status == GRP_GZIP_WALK_INPUT_ENDS ? "the stream ends inside a block at the end of the file" : "the decoder refused the stream";
      f.status = r.status;
      return;
    }
    if (r.bits == 0 || r.hist_len > 32768 || (!r.final && r.text_len == 0)) {
      f.left = "a step that made no progress"; // (not what the engine is known to do)
      return;
    }
    f.bit += r.bits;
    f.seg_text += r.text_len;
    f.member_text += r.text_len;
    f.seg_crc = (uint32_t)crc32_combine(f.seg_crc, r.crc32, (z_off_t)r.text_len);
    f.member_crc = (uint32_t)crc32_combine(f.member_crc, r.crc32, (z_off_t)r.text_len);
    memcpy(f.hist.data(), hist, r.hist_len);
    f.hist_len = r.hist_len;
    stats.text_bytes += r.text_len;
    if (r.final) { // the member's end closes the segment
      if (f.seg_text != 0) {
        commit(f, GRP_GZIP_SEG_FINAL);
      } else if (f.member_segs != 0) {
        // blocks without text behind the last point: they belong to the segment in front of it, the point is forgotten
        GzSegment& g = f.ix->segs.back();
        g.n_bits = f.bit - g.comp_bit;
        g.flags = GRP_GZIP_SEG_FINAL;
        f.ix->max_comp = std::max(f.ix->max_comp, g.end_byte() - g.first_byte());
      } // (else: a member without text has no segment)
      if (!f.left) {
        end_member(f);
      }
    } else if (f.seg_text >= span_) {
      commit(f, 0);
      if (!f.left) {
        point(f);
      }
    }
  }

  const uint64_t span_, max_bytes_;
  const GzWalkSizes sizes_;
  std::vector<File> files_;
  std::vector<uint8_t> buf_;
};

std::vector<GzWalkFile>
gzip_walk(const std::vector<std::string>& paths, uint64_t span, uint64_t max_bytes, const GzWalkSizes& sizes, const GzWalkLaunch& launch, GzWalkStats* stats, const GzWalkBuffer& pin, const GzWalkBuffer& unpin)
{
  const auto t0 = std::chrono::steady_clock::now();
  GzWalkStats st;
  GzWalker w(paths, span, max_bytes, sizes);
  w.run(launch, st, pin, unpin);
  std::vector<GzWalkFile> out = w.take();
  st.files = paths.size();
  for (const GzWalkFile& f : out) {
    (f.index ? st.walked : st.left_to_zlib) += 1;
  }
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (stats) {
    *stats = st;
  }
  return out;
}

} // namespace gr
