#include "gr_gzwalk.hpp"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <map>
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

int
gzip_walk_members_switch()
{
  const char* e = getenv("GRP_GZIP_WALK_MEMBERS");
  return !e || !strcmp(e, "off") ? 0 : !strcmp(e, "on") ? 1 : -1;
}

GzWalkMembers
gzip_walk_members()
{
  GzWalkMembers m;
  m.on = gzip_walk_members_switch() == 1;
  if (const char* e = getenv("GRP_GZIP_WALK_STREAMS")) {
    unsigned long long v = 0;
    m.streams = sscanf(e, "%llu", &v) == 1 && v ? v : m.streams;
  }
  return m;
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
  GzWalker(const std::vector<std::string>& paths, uint64_t span, uint64_t max_bytes, const GzWalkSizes& sizes, const GzWalkMembers& members, GzWalkStats& stats)
    : span_(std::max<uint64_t>(span, 1))
    , max_bytes_(max_bytes)
    , sizes_(sizes)
    , members_(members)
    , files_(paths.size())
  {
    for (size_t i = 0; i < paths.size(); ++i) {
      File& f = files_[i];
      f.path = paths[i];
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
      f.head = new_stream(f, false);
      begin_member(*f.head, 0);
      if (f.head->left) {
        f.left = f.head->left;
      } else if (members_.on) {
        scan(f, stats);
      }
    }
  }

  void run(const GzWalkLaunch& launch, GzWalkStats& stats, const GzWalkBuffer& pin, const GzWalkBuffer& unpin)
  {
    // the window buffer once, for the first windows of all streams there can be at a time; it grows only where a step is
    // repeated with more
    size_t cap = 0, ahead = 0;
    for (const File& f : files_) {
      if (live(f)) {
        cap += (size_t)((f.head->window + 7) & ~uint64_t(7));
        ahead += f.cand.size();
      }
    }
    const bool any = cap != 0;
    cap += (size_t)std::min<uint64_t>(ahead, members_.streams) * (size_t)((sizes_.window + 7) & ~uint64_t(7));
    buf_.resize(cap + 8);
    if (pin && any) {
      pin(buf_.data(), buf_.size());
    }
    const bool pinned = pin && any;
    std::vector<Stream*> active;
    std::vector<grp_gzip_walk_step> steps;
    std::vector<grp_gzip_walk_result> res;
    std::vector<uint8_t> dict, hist_out;
    for (bool failed = false; !failed;) {
      if (members_.on) {
        admit(stats);
      }
      active.clear();
      for (File& f : files_) {
        if (live(f)) {
          active.push_back(f.head.get());
          for (auto& s : f.ahead) {
            if (s.second->stepping()) {
              active.push_back(s.second.get());
            }
          }
        }
      }
      if (active.empty()) {
        break;
      }
      ++stats.rounds;
      if (members_.on) {
        stats.max_in_flight = std::max<uint64_t>(stats.max_in_flight, active.size());
      }
      for (size_t first = 0; first < active.size();) {
        // one launch: the streams from `first` on that fit its limits (all of them, but for very many or very large windows):
        // 4 GiB of histories at 32 KiB a step are 2^17 steps, the compressed bytes and the rooms as the engine bounds them
        size_t n = 0;
        uint64_t n_comp = 0, rooms = 0;
        for (; first + n < active.size() && n < (size_t(1) << 17); ++n) {
          const Stream& s = *active[first + n];
          if (n != 0 && (n_comp + s.window > (uint64_t(1) << 31) || rooms + s.room > (uint64_t(1) << 33))) {
            break;
          }
          n_comp += (s.window + 7) & ~uint64_t(7);
          rooms += s.room;
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
          Stream& s = *active[first + k];
          const File& f = *s.file;
          const uint64_t byte0 = s.bit >> 3, phase = s.bit & 7;
          const uint64_t want = byte0 < f.size ? std::min(s.window, f.size - byte0) : 0;
          int err = 0;
          const uint64_t got = want ? read_at(f.path, buf_.data() + slot, (size_t)want, byte0, &err) : 0;
          s.at_eof = err == 0 && byte0 + got >= f.size; // (a read that failed: the step runs out of bytes in front of the end)
          s.read_failed = err != 0;
          const uint64_t n_bits = got * 8 > phase ? got * 8 - phase : 0;
          memcpy(dict.data() + k * 32768, s.hist.data(), s.hist_len);
          const uint64_t target = std::max<uint64_t>(1, std::min(span_ - s.seg_text, std::min(sizes_.room / 2, s.room)));
          steps[k] = grp_gzip_walk_step{ slot * 8 + (n_bits ? phase : 0), n_bits, (uint64_t)k * 32768, s.hist_len, (uint32_t)target, (uint32_t)s.room, 0 };
          slot += (s.window + 7) & ~uint64_t(7);
        }
        ++stats.launches;
        if (!launch(buf_.data(), slot, dict.data(), dict.size(), steps.data(), (uint32_t)n, res.data(), hist_out.data())) {
          for (File& f : files_) {
            if (live(f)) {
              f.left = "a launch of the walk failed";
            }
          }
          failed = true;
          break;
        }
        for (size_t k = 0; k < n; ++k) {
          answer(*active[first + k], res[k], hist_out.data() + k * 32768, stats);
        }
        first += n;
      }
      // behind the answers of ALL the round's steps: a stream that ended in this round is there for the chain that arrives at it
      for (File& f : files_) {
        if (f.head) {
          settle(f, stats);
        }
      }
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
  struct File;

  // a finished segment of a stream ahead of its file's chain, with the history at its point
  struct Kept
  {
    GzSegment g;
    std::vector<uint8_t> dict;
  };

  // One walk through members from a header on.  A file's chain head (ahead false) writes its segments into the file's
  // index and goes from member to member; a stream begun at a candidate (ahead true) keeps them, walks one member and
  // stops behind its trailer, until the chain arrives at its first byte and adopts it — or passes it, and it is dropped
  struct Stream
  {
    File* file = nullptr;
    bool ahead = false;
    uint64_t start = 0;         // the byte the member's header stands at
    const char* left = nullptr; // why the walk through this member stopped (the file's reason, once the chain is here)
    uint32_t status = 0;
    bool ended = false;         // the member's trailer matched ...
    uint64_t end = 0;           // ... and this is the byte behind it
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
    // ahead: the segments so far, the text decoded, the bytes they will take in the index (roughly: a history takes 32 KiB or less)
    std::vector<Kept> kept;
    uint64_t text = 0, kept_bytes = 0;
    bool stepping() const { return !left && !ended; }
  };

  struct File
  {
    std::string path;
    uint64_t size = 0;
    std::unique_ptr<GzIndex> ix;
    const char* left = nullptr; // why the file is left to zlib
    uint32_t status = 0;
    bool unreadable = false;    // ... because it is no regular file that can be looked at
    bool done = false;          // the last member's trailer ended the file
    std::unique_ptr<Stream> head; // the chain: it began at byte 0
    // the members switch: the candidates (ascending), the first one not looked at yet, the streams ahead of the chain by
    // their first byte; no_ahead: the index and the streams ahead together went over the cap, the chain goes on alone
    std::vector<uint64_t> cand;
    size_t next_cand = 0;
    std::map<uint64_t, std::unique_ptr<Stream>> ahead;
    bool no_ahead = false;
  };

  static bool live(const File& f) { return f.head && !f.left && !f.done; }

  std::unique_ptr<Stream> new_stream(File& f, bool ahead) const
  {
    std::unique_ptr<Stream> s(new Stream);
    s->file = &f;
    s->ahead = ahead;
    s->room = sizes_.room;
    s->window = sizes_.window;
    s->hist.resize(32768);
    return s;
  }

  // The candidates of a file: the bytes behind byte 0 where 1f 8b 08 stands with no reserved flag bit, in one sequential
  // read.  (What is a header is decided by gzip_header_bytes when a stream is begun there.)
  void scan(File& f, GzWalkStats& stats)
  {
    const auto t0 = std::chrono::steady_clock::now();
    const int fd = ::open(f.path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
      return;
    }
    constexpr size_t chunk = size_t(4) << 20;
    std::vector<uint8_t> b(chunk + 3); // a chunk and the three bytes behind it: a candidate may lie across two chunks
    for (uint64_t off = 0; off < f.size; off += chunk) {
      size_t got = 0;
      while (got < b.size()) {
        const ssize_t r = ::pread(fd, b.data() + got, b.size() - got, (off_t)(off + got));
        if (r < 0 && errno == EINTR) {
          continue;
        }
        if (r <= 0) {
          break;
        }
        got += (size_t)r;
      }
      if (got < 4) {
        break;
      }
      const size_t last = std::min(chunk, got - 3); // candidates at [0, last) of this chunk
      for (size_t i = 0; i < last;) {
        const void* m = memchr(b.data() + i, 0x1f, last - i);
        if (!m) {
          break;
        }
        i = (size_t)(static_cast<const uint8_t*>(m) - b.data());
        if (b[i + 1] == 0x8b && b[i + 2] == 8 && !(b[i + 3] & 0xe0) && off + i != 0) {
          f.cand.push_back(off + i);
        }
        ++i;
      }
      if (got < b.size()) {
        break;
      }
    }
    ::close(fd);
    stats.candidates += f.cand.size();
    stats.scan_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

  // Streams are begun at candidates while fewer than the budget take steps: in file order, then offset order.  A candidate
  // the chain has passed is forgotten, one whose header does not parse too
  void admit(GzWalkStats& stats)
  {
    uint64_t in_flight = 0;
    for (const File& f : files_) {
      if (live(f)) {
        ++in_flight;
        for (const auto& s : f.ahead) {
          in_flight += s.second->stepping();
        }
      }
    }
    for (File& f : files_) {
      if (!live(f) || f.no_ahead) {
        continue;
      }
      const uint64_t pos = f.head->bit >> 3;
      while (f.next_cand < f.cand.size()) {
        const uint64_t q = f.cand[f.next_cand];
        if (q >= pos && in_flight >= members_.streams) {
          return;
        }
        ++f.next_cand;
        if (q < pos) {
          continue;
        }
        std::unique_ptr<Stream> s = new_stream(f, true);
        begin_member(*s, q);
        if (s->left) {
          continue;
        }
        ++stats.streams;
        ++in_flight;
        f.ahead[q] = std::move(s);
      }
    }
  }

  void drop(File& f, std::map<uint64_t, std::unique_ptr<Stream>>::iterator last, GzWalkStats& stats)
  {
    for (auto it = f.ahead.begin(); it != last; ++it) {
      ++stats.dropped;
      stats.wasted_text += it->second->text;
    }
    f.ahead.erase(f.ahead.begin(), last);
  }

  // Behind a round: the chain.  The head's failure is the file's.  Where the head's member has ended, the chain arrives at the
  // byte behind its trailer: the end of the file, bytes that are no member, a stream begun there (adopted: its segments
  // enter the index in order; ended too, its end is the next arrival) or none (the head begins the member itself, as
  // without the switch).  Then the streams the chain has passed are dropped
  void settle(File& f, GzWalkStats& stats)
  {
    if (!f.left && !f.done && f.head->left) {
      f.left = f.head->left;
      f.status = f.head->status;
    }
    while (!f.left && !f.done && f.head->ended) {
      const uint64_t p = f.head->end;
      if (p == f.size) {
        f.done = true;
        break;
      }
      uint8_t t[2];
      int err = 0;
      if (read_at(f.path, t, (size_t)std::min<uint64_t>(2, f.size - p), p, &err) != 2 || t[0] != 0x1f || t[1] != 0x8b) {
        f.left = "bytes behind the last member that are no member"; // (gzread ignores them; every pass over such a file stays with zlib)
        break;
      }
      const auto it = f.ahead.find(p);
      if (it == f.ahead.end()) {
        f.head->ended = false;
        begin_member(*f.head, p);
      } else {
        std::unique_ptr<Stream> s = std::move(it->second);
        f.ahead.erase(it);
        ++stats.adopted;
        stats.text_bytes += s->text;
        // in the order the serial walk meets them: the segments (the cap), then what stopped the stream
        const char* const noted = s->left;
        s->left = nullptr;
        s->ahead = false;
        for (const Kept& k : s->kept) {
          append(*s, k.g, k.dict.data());
          if (s->left) {
            break;
          }
        }
        s->kept.clear();
        s->kept.shrink_to_fit();
        if (!s->left) {
          s->left = noted;
        } else {
          s->status = 0;
        }
        f.head = std::move(s);
      }
      if (f.head->left) {
        f.left = f.head->left;
        f.status = f.head->status;
      }
    }
    if (f.ahead.empty()) {
      return;
    }
    if (f.left || f.done) {
      drop(f, f.ahead.end(), stats);
      return;
    }
    drop(f, f.ahead.lower_bound(f.head->bit >> 3), stats); // (behind the last consumed bit a member may begin, in front of it none)
    uint64_t bytes = f.ix->bytes();
    for (const auto& s : f.ahead) {
      bytes += s.second->kept_bytes;
    }
    if (bytes > max_bytes_) { // the cap holds for the index and the streams ahead together: the chain goes on alone
      drop(f, f.ahead.end(), stats);
      f.no_ahead = true;
    }
  }

  // the header of the member at byte `at`: the point behind it
  void begin_member(Stream& s, uint64_t at)
  {
    const File& f = *s.file;
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
      s.left = "a member's header is not one zlib takes";
      return;
    }
    s.start = at;
    s.bit = (at + (uint64_t)h) * 8;
    s.member_text = 0;
    s.member_crc = 0;
    s.member_segs = 0;
    s.hist_len = 0;
    point(s);
  }

  // a restart point at s.bit, with the history there
  void point(Stream& s)
  {
    s.cur = GzSegment{ s.bit, 0, 0, s.hist_len, 0, 0, 0 };
    s.seg_dict.assign(s.hist.begin(), s.hist.begin() + s.hist_len);
    s.seg_text = 0;
    s.seg_crc = 0;
  }

  // a finished segment enters the file's index (GzIndexReader::commit)
  void append(Stream& s, GzSegment g, const uint8_t* dict)
  {
    GzIndex& ix = *s.file->ix;
    if (g.dict_len) {
      uint8_t* d = ix.reserve(32768, &g.dict_at);
      memcpy(d, dict, g.dict_len);
      ix.used_ += g.dict_len;
    }
    ix.segs.push_back(g);
    ix.text_bytes += g.text_len;
    ix.max_text = std::max<uint64_t>(ix.max_text, g.text_len);
    ix.max_comp = std::max(ix.max_comp, g.end_byte() - g.first_byte());
    if (ix.bytes() > max_bytes_) {
      s.left = "the index grew beyond its cap";
    }
  }

  // the open segment ends at s.bit
  void commit(Stream& s, uint32_t flags)
  {
    if (s.seg_text == 0 || s.seg_text > 0xffff0000ull) { // (never empty; the engine takes 32-bit lengths)
      s.left = "a segment of more than 4 GiB - 64 KiB of text";
      return;
    }
    s.cur.n_bits = s.bit - s.cur.comp_bit;
    s.cur.text_len = (uint32_t)s.seg_text;
    s.cur.crc32 = s.seg_crc;
    s.cur.flags = flags;
    if (s.ahead) {
      s.kept.push_back(Kept{ s.cur, std::vector<uint8_t>(s.seg_dict.begin(), s.seg_dict.begin() + s.cur.dict_len) });
      s.kept_bytes += sizeof(GzSegment) + s.cur.dict_len;
    } else {
      append(s, s.cur, s.seg_dict.data());
    }
    ++s.member_segs;
  }

  // behind the final block at s.bit: the trailer.  What stands behind it is the chain's to look at (settle)
  void end_member(Stream& s)
  {
    const File& f = *s.file;
    const uint64_t at = (s.bit + 7) >> 3;
    uint8_t t[8];
    int err = 0;
    const size_t got = at + 8 <= f.size ? read_at(f.path, t, 8, at, &err) : 0;
    if (got < 8 || err) {
      s.left = "the file ends inside a member's trailer";
      return;
    }
    const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    if (crc != s.member_crc || isize != (uint32_t)s.member_text) {
      s.left = "a member's trailer does not match its text";
      return;
    }
    s.ended = true;
    s.end = at + 8;
  }

  void answer(Stream& s, const grp_gzip_walk_result& r, const uint8_t* hist, GzWalkStats& stats)
  {
    if (r.status == GRP_GZIP_WALK_NO_ROOM || (r.status == GRP_GZIP_WALK_INPUT_ENDS && !s.at_eof && !s.read_failed)) {
      // the step is repeated with both doubled
      if ((r.status == GRP_GZIP_WALK_NO_ROOM ? s.room : s.window) >= sizes_.cap) {
        s.left = "a block needs more room or more compressed bytes than the cap";
        s.status = r.status;
        return;
      }
      s.room = std::min(2 * s.room, sizes_.cap);
      s.window = std::min(2 * s.window, sizes_.cap);
      ++stats.repeats;
      return;
    }
    if (r.status != 0) {
      s.left = s.read_failed ? "the file could not be read" : r.status == GRP_GZIP_WALK_INPUT_ENDS ? "the stream ends inside a block at the end of the file" : "the decoder refused the stream";
      s.status = r.status;
      return;
    }
    if (r.bits == 0 || r.hist_len > 32768 || (!r.final && r.text_len == 0)) {
      s.left = "a step that made no progress"; // (not what the engine is known to do)
      return;
    }
    s.bit += r.bits;
    s.seg_text += r.text_len;
    s.member_text += r.text_len;
    s.seg_crc = (uint32_t)crc32_combine(s.seg_crc, r.crc32, (z_off_t)r.text_len);
    s.member_crc = (uint32_t)crc32_combine(s.member_crc, r.crc32, (z_off_t)r.text_len);
    memcpy(s.hist.data(), hist, r.hist_len);
    s.hist_len = r.hist_len;
    (s.ahead ? s.text : stats.text_bytes) += r.text_len; // (a stream's text is counted where the chain takes or passes it)
    if (r.final) { // the member's end closes the segment
      if (s.seg_text != 0) {
        commit(s, GRP_GZIP_SEG_FINAL);
      } else if (s.member_segs != 0) {
        // blocks without text behind the last point: they belong to the segment in front of it, the point is forgotten
        GzSegment& g = s.ahead ? s.kept.back().g : s.file->ix->segs.back();
        g.n_bits = s.bit - g.comp_bit;
        g.flags = GRP_GZIP_SEG_FINAL;
        if (!s.ahead) {
          s.file->ix->max_comp = std::max(s.file->ix->max_comp, g.end_byte() - g.first_byte());
        }
      } // (else: a member without text has no segment)
      if (!s.left) {
        end_member(s);
      }
    } else if (s.seg_text >= span_) {
      commit(s, 0);
      if (!s.left) {
        point(s);
      }
    }
  }

  const uint64_t span_, max_bytes_;
  const GzWalkSizes sizes_;
  const GzWalkMembers members_;
  std::vector<File> files_;
  std::vector<uint8_t> buf_;
};

std::vector<GzWalkFile>
gzip_walk(const std::vector<std::string>& paths, uint64_t span, uint64_t max_bytes, const GzWalkSizes& sizes, const GzWalkLaunch& launch, GzWalkStats* stats, const GzWalkBuffer& pin, const GzWalkBuffer& unpin,
          const GzWalkMembers& members)
{
  const auto t0 = std::chrono::steady_clock::now();
  GzWalkStats st;
  GzWalker w(paths, span, max_bytes, sizes, members, st);
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
