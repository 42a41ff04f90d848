// The record sources (gr_source.hpp): the host reader, and the slot pipeline that feeds the engine's ingest from text,
// BGZF members or the segments of an indexed gzip file.
#include "gr_source.hpp"
#include "gr_bgzf.hpp"
#include "gr_fastq.hpp"
#include "gr_params.hpp"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#if defined(_OPENMP)
#include <omp.h>
#endif

namespace gr {

double
now_s()
{
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace {

// records / bases per host batch (one grp_reads upload each).  GRP_BATCH_RECORDS
// overrides the record count (tests use it to exercise the batch boundaries).
size_t
batch_records()
{
  static const size_t n = [] {
    const char* e = getenv("GRP_BATCH_RECORDS");
    const long v = e ? atol(e) : 0;
    return v > 0 ? (size_t)v : (size_t)16384;
  }();
  return n;
}
#define BATCH_RECORDS batch_records()
constexpr size_t BATCH_BASES = size_t(384) << 20;

size_t
ingest_chunk_bytes()
{
  static const size_t n = [] {
    const char* e = getenv("GRP_INGEST_CHUNK");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : (size_t)256 << 20;
  }();
  return n;
}

// host reader + host packing (engines without the ingest entry points)
class HostSource : public RecordSource
{
public:
  HostSource(PathRun& run)
    : run_(run)
    , fq_(run.opt.input)
  {}
  bool ok() const override { return fq_.ok(); }
  bool is_fastq() override { return fq_.is_fastq(); }
  bool next(Batch& b) override
  {
    if (!fq_.next_batch(rb_, BATCH_RECORDS, BATCH_BASES)) {
      return false;
    }
    b.text = rb_.text.data();
    b.rec.resize(rb_.rec.size());
    for (size_t i = 0; i < rb_.rec.size(); ++i) {
      const RecordRef& r = rb_.rec[i];
      b.rec[i] = Rec{ r.id_off, r.id_len, r.seq_off, r.seq_len, r.qual_off, r.qual_len };
    }
    b.seq_is_upper = true;
    return true;
  }
  void stats(Batch& b, size_t min_len, bool need_acgt) override
  {
    const size_t n = b.rec.size();
    b.avg.assign(n, 0);
    b.delta.assign(n, 0);
    b.non_acgt.assign(n, 0);
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic, 8)
#endif
    for (size_t i = 0; i < n; ++i) {
      const Rec& r = b.rec[i];
      if (r.seq_len < min_len) {
        continue;
      }
      calc_phred_average(b.text + r.qual_off, r.qual_len, b.avg[i], b.delta[i]);
      if (need_acgt) {
        const char* s = b.text + r.seq_off; // already upper-cased
        for (size_t j = 0; j < r.seq_len; ++j) {
          const char c = s[j];
          if (c != 'A' && c != 'C' && c != 'G' && c != 'T') {
            b.non_acgt[i] = 1;
            break;
          }
        }
      }
    }
  }
  int upload(Batch& b, const std::vector<uint32_t>& sel, std::vector<uint32_t>& lens, void** reads) override
  {
    const size_t n = sel.size();
    lens.resize(n);
    word_off_.resize(n + 1);
    uint64_t w = 0;
    for (size_t i = 0; i < n; ++i) {
      word_off_[i] = w;
      lens[i] = (uint32_t)b.rec[sel[i]].seq_len;
      w += (b.rec[sel[i]].seq_len + 15) / 16;
    }
    word_off_[n] = w;
    packed_.resize(w ? w : 1);
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic, 16)
#endif
    for (size_t i = 0; i < n; ++i) {
      pack_2bit(b.text + b.rec[sel[i]].seq_off, b.rec[sel[i]].seq_len, packed_.data() + word_off_[i]);
    }
    return run_.vt.reads_upload(run_.ctx, packed_.data(), word_off_.data(), lens.data(), (uint32_t)n, reads);
  }

private:
  PathRun& run_;
  FastqStream fq_;
  RecordBatch rb_;
  std::vector<uint32_t> packed_;
  std::vector<uint64_t> word_off_;
};

// ---- what the slots of a GpuSource are fed from ---------------------------------------------------------------------
// A feed fills the text of a slot, at once (fill) or in two steps: the reader thread reads compressed bytes and their
// table (fill), the consumer has the engine inflate them into the slot's text before its first use (inflate).
// Everything behind that — the carried tail, parse, pack, stats — does not know.
//
// Threading, as GpuSource keeps it: a FREE slot is the reader's, a READY slot the consumer's, so fill and inflate of
// one slot never overlap; inflate runs at most once per filled slot, from next() or from prefetch_next(), whichever
// comes first.  The index a pass publishes (PathRun::gzidx) is read only by the next pass's source, which is
// constructed after this one's reader thread has ended.
struct SlotBuf
{
  char* text;          // Sizes::chunk bytes
  unsigned char* comp; // Sizes::comp bytes
  unsigned char* dict; // Sizes::dict bytes
};

class Feed
{
public:
  // what a slot needs: its text (at least the chunk asked for) and, beside it, compressed bytes and histories
  struct Sizes
  {
    size_t chunk, comp, dict;
  };
  struct Counts // (developer trace)
  {
    uint64_t bgzf_blocks = 0, gzip_segs = 0;
  };
  virtual ~Feed() {}
  // once, before the first fill: the slots will have these sizes (a feed sizes its per-slot tables here)
  virtual Sizes layout(size_t chunk, int /*n_slots*/) { return Sizes{ chunk, 0, 0 }; }
  // reader thread: the next up to `chunk` bytes of text for the slot; eof: the data ends with them
  virtual size_t fill(int slot, const SlotBuf& b, size_t chunk, bool& eof) = 0;
  // consumer thread: the slot's text is there; false: the engine refused it (the failure is noted)
  virtual bool inflate(int /*slot*/, const SlotBuf&, size_t /*chunk*/) { return true; }
  virtual Counts counts() const { return Counts{}; }
};

// `want` bytes at `off`; fewer: the file ends there (*err 0) or the read failed (*err: errno)
size_t
pread_full(int fd, unsigned char* dst, size_t want, uint64_t off, int* err)
{
  *err = 0;
  size_t k = 0;
  while (k < want) {
    const ssize_t r = pread(fd, dst + k, want - k, (off_t)(off + k));
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

// Text: InputFile (parallel pread of a plain file, zlib for gzip data), or GzIndexReader — zlib as before, on the reader
// thread — in the first pass over a plain gzip file, which leaves the index of its restart points in the run when it
// reads the file to its end.  A pass that ends early (the Phred median) leaves no index.
class TextFeed : public Feed
{
public:
  TextFeed(PathRun& run, InputFile& in, std::unique_ptr<GzIndexReader> build)
    : run_(run)
    , in_(in)
    , build_(std::move(build))
  {}
  size_t fill(int, const SlotBuf& b, size_t chunk, bool& eof) override
  {
    size_t got = 0;
    while (!eof && got < chunk) {
      const size_t k = build_ ? build_->read(b.text + got, chunk - got) : in_.read(b.text + got, chunk - got);
      if (k == 0) {
        eof = true;
      }
      got += k;
    }
    if (eof && build_ && build_->complete()) {
      run_.gzidx = build_->take(); // (read by the next pass's source, which begins behind this thread's end)
    }
    return got;
  }

private:
  PathRun& run_;
  InputFile& in_;
  std::unique_ptr<GzIndexReader> build_;
};

// A BGZF-compressed file (gr_bgzf.hpp) whose members the engine can inflate: the reader thread reads COMPRESSED bytes
// and walks the members' headers; a slot is filled with whole members until its text, its compressed bytes or its block
// table is full.  Plain gzip is one serial stream and stays with zlib: from a member in mid-file that is not BGZF on
// (bgzip output followed by gzip output) a text feed reads the rest.
class BgzfFeed : public Feed
{
public:
  BgzfFeed(PathRun& run, int fd)
    : run_(run)
    , fd_(fd)
  {}
  ~BgzfFeed() override { ::close(fd_); }
  Sizes layout(size_t chunk, int n_slots) override
  {
    chunk = std::max<size_t>(chunk, BGZF_MAX_TEXT); // a tiny GRP_INGEST_CHUNK still holds one member
    comp_cap_ = std::max<size_t>(chunk / 2, BGZF_MAX_MEMBER);
    tab_cap_ = std::max<size_t>(chunk / 4096, 64);
    slot_.resize((size_t)n_slots);
    for (Table& t : slot_) {
      t.blocks.resize(tab_cap_);
    }
    return Sizes{ chunk, comp_cap_, 0 };
  }
  size_t fill(int i, const SlotBuf& b, size_t chunk, bool& eof) override
  {
    slot_[i].n_blocks = slot_[i].comp_n = 0; // (also where zlib reads: nothing to inflate)
    size_t got = 0;
    if (!tail_) {
      got = read_members(slot_[i], b.comp, chunk, eof);
    }
    if (got == 0 && !eof && tail_) {
      slot_[i].n_blocks = slot_[i].comp_n = 0; // (empty members in front of the part zlib reads)
      got = tail_->fill(i, b, chunk, eof);
    }
    return got;
  }
  bool inflate(int j, const SlotBuf& b, size_t chunk) override
  {
    const Table& sl = slot_[j];
    if (sl.n_blocks == 0) {
      return true;
    }
    uint32_t bad = UINT32_MAX;
    if (run_.ext.bgzf_inflate(run_.ctx, b.comp, sl.comp_n, sl.blocks.data(), (uint32_t)sl.n_blocks, b.text, chunk, &bad) != GRP_OK) {
      uint64_t at = sl.comp_file_off; // the members of a slot follow each other
      if (bad != UINT32_MAX && bad > 0 && bad < sl.n_blocks) {
        at += sl.blocks[bad - 1].comp_off + sl.blocks[bad - 1].comp_len + 8;
      }
      note_input_failure("reading " + run_.opt.input + " failed: BGZF member " + (bad != UINT32_MAX ? "at byte " + std::to_string(at) : "in the chunk at byte " + std::to_string(at)) + ": " +
                         (run_.vt.last_error ? run_.vt.last_error(run_.ctx) : "the engine could not inflate it"));
      return false;
    }
    n_blocks_ += sl.n_blocks;
    return true;
  }
  Counts counts() const override { return Counts{ n_blocks_, 0 }; }

private:
  // the text of a slot is that of these members, inflated by the consumer before its first use
  struct Table
  {
    std::vector<grp_bgzf_block> blocks; // tab_cap_ entries; comp_off inside the slot's compressed bytes
    size_t n_blocks = 0, comp_n = 0;
    uint64_t comp_file_off = 0; // where the slot's compressed bytes begin in the file
  };
  // Whole members into the slot until its text (chunk), its compressed bytes (comp_cap_) or its table (tab_cap_) is
  // full.  Returns the bytes of text the members hold.  A member that is not BGZF hands the rest of the file to zlib
  // (tail_); a file that ends inside a member is an error, one that ends without the empty end-of-file member is not
  // (zlib accepts it too).
  size_t read_members(Table& sl, unsigned char* comp, size_t chunk, bool& eof)
  {
    constexpr size_t kPiece = size_t(16) << 20;
    for (;;) { // (again only behind a table full of empty members)
      size_t have = 0, pos = 0, text = 0, nb = 0;
      bool full = false, file_end = false, other = false;
      sl.comp_file_off = off_;
      while (!full) {
        if (!file_end && have < comp_cap_ && have - pos < BGZF_MAX_MEMBER) {
          const size_t want = std::min(comp_cap_ - have, kPiece);
          int err = 0;
          const size_t k = pread_full(fd_, comp + have, want, off_ + have, &err);
          if (err) {
            note_input_failure("reading " + run_.opt.input + " failed at byte " + std::to_string(off_ + have + k) + ": " + strerror(err));
          }
          file_end = k < want;
          have += k;
        }
        int why = 1;
        const size_t base = pos;
        const size_t got = bgzf_scan(comp + base, have - base, &sl.blocks[nb], tab_cap_ - nb, nullptr, &why);
        for (size_t t = 0; t < got; ++t) {
          grp_bgzf_block& b = sl.blocks[nb]; // (comp_off: inside what was scanned)
          if (text + b.text_len > chunk) {
            full = true;
            break;
          }
          b.comp_off += base;
          text += b.text_len;
          pos = (size_t)b.comp_off + b.comp_len + 8;
          ++nb;
        }
        if (full) {
          break;
        }
        if (nb == tab_cap_) {
          full = true;
        } else if (why == 2) {
          other = true;
          break;
        } else if (file_end) { // (why 0: bytes of a member are missing; 1: the members end with the file)
          if (have > pos) {
            note_input_failure("reading " + run_.opt.input + " failed: the file ends inside the BGZF member at byte " + std::to_string(off_ + pos) + " (truncated)");
          }
          eof = true;
          break;
        } else if (have == comp_cap_) {
          full = true;
        }
      }
      off_ += pos;
      sl.n_blocks = nb;
      sl.comp_n = pos;
      if (other) {
        // from this member on zlib reads, from a descriptor of its own that stands there
        const int fd = ::open(run_.opt.input.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd >= 0 && lseek(fd, (off_t)off_, SEEK_SET) == (off_t)off_) {
          tail_in_.reset(new InputFile(run_.opt.input, fd));
        } else if (fd >= 0) {
          ::close(fd);
        }
        if (tail_in_ && tail_in_->ok()) {
          tail_.reset(new TextFeed(run_, *tail_in_, nullptr));
        } else {
          note_input_failure("reading " + run_.opt.input + " failed: cannot read on behind the BGZF members at byte " + std::to_string(off_));
          eof = true;
        }
      }
      if (text != 0 || eof || other) {
        return text;
      }
    }
  }
  PathRun& run_;
  int fd_;           // the reader's descriptor ...
  uint64_t off_ = 0; // ... and how far it has come
  size_t comp_cap_ = 0, tab_cap_ = 0;
  std::vector<Table> slot_;
  std::unique_ptr<InputFile> tail_in_; // what follows the BGZF members ...
  std::unique_ptr<TextFeed> tail_;     // ... read as text
  uint64_t n_blocks_ = 0;
};

// A plain gzip file in the passes behind the one that left its index in the run: the reader thread preads whole
// SEGMENTS into a slot until its text, its compressed bytes, its histories or its table is full, and the consumer has
// the engine inflate them, exactly like the members of a BGZF file.  The compressed bytes of a slot are one range of the
// file (with the trailers and headers between two members in it).
class GzipSegFeed : public Feed
{
public:
  GzipSegFeed(PathRun& run, int fd)
    : run_(run)
    , ix_(run.gzidx)
    , fd_(fd)
  {}
  ~GzipSegFeed() override { ::close(fd_); }
  Sizes layout(size_t chunk, int n_slots) override
  {
    comp_cap_ = std::max<size_t>(chunk / 2, (size_t)ix_->max_comp + 8);
    dict_cap_ = chunk / 8 + 32768; // (32 KiB per 256 KiB of text at the default span)
    tab_cap_ = std::max<size_t>(chunk / 4096, 64);
    slot_.resize((size_t)n_slots);
    for (Table& t : slot_) {
      t.segs.resize(tab_cap_);
    }
    return Sizes{ chunk, comp_cap_, dict_cap_ };
  }
  size_t fill(int i, const SlotBuf& b, size_t chunk, bool& eof) override
  {
    const GzIndex& ix = *ix_;
    Table& sl = slot_[i];
    sl.n_segs = sl.comp_n = sl.dict_n = 0;
    if (next_ >= ix.segs.size()) {
      eof = true;
      return 0;
    }
    const uint64_t byte0 = ix.segs[next_].first_byte();
    uint64_t end = byte0;
    size_t text = 0, ns = 0, nd = 0;
    while (next_ + ns < ix.segs.size() && ns < tab_cap_) {
      const GzSegment& g = ix.segs[next_ + ns];
      if (text + g.text_len > chunk || g.end_byte() - byte0 > comp_cap_ || nd + g.dict_len > dict_cap_) {
        break; // (never the slot's first: open_feed has seen to that)
      }
      sl.segs[ns] = grp_gzip_segment{ g.comp_bit - byte0 * 8, g.n_bits, nd, g.dict_len, g.text_len, g.crc32, g.flags };
      if (g.dict_len) {
        memcpy(b.dict + nd, ix.dict(g), g.dict_len);
      }
      nd = (nd + g.dict_len + 3) & ~size_t(3);
      text += g.text_len;
      end = g.end_byte();
      ++ns;
    }
    const size_t want = (size_t)(end - byte0);
    int err = 0;
    const size_t k = pread_full(fd_, b.comp, want, byte0, &err);
    if (k < want) {
      note_input_failure("reading " + run_.opt.input + " failed at byte " + std::to_string(byte0 + k) + ": " + (err ? strerror(err) : "the file ends in front of a segment of its index (it was written during the run)"));
      eof = true;
      return 0;
    }
    sl.comp_file_off = byte0;
    sl.comp_n = want;
    sl.n_segs = ns;
    sl.dict_n = std::min(nd, dict_cap_);
    next_ += ns;
    eof = next_ == ix.segs.size();
    return text;
  }
  bool inflate(int j, const SlotBuf& b, size_t chunk) override
  {
    const Table& sl = slot_[j];
    if (sl.n_segs == 0) {
      return true;
    }
    uint32_t bad = UINT32_MAX;
    if (run_.ext.gzip_inflate(run_.ctx, b.comp, sl.comp_n, b.dict, sl.dict_n, sl.segs.data(), (uint32_t)sl.n_segs, b.text, chunk, &bad) != GRP_OK) {
      const uint64_t bit = sl.comp_file_off * 8 + (bad < sl.n_segs ? sl.segs[bad].comp_bit : 0);
      note_input_failure("reading " + run_.opt.input + " failed: gzip segment " + (bad < sl.n_segs ? "" : "in the chunk ") + "at byte " + std::to_string(bit >> 3) + " (bit " + std::to_string(bit & 7) + "): " +
                         (run_.vt.last_error ? run_.vt.last_error(run_.ctx) : "the engine could not inflate it"));
      return false;
    }
    n_segs_ += sl.n_segs;
    return true;
  }
  Counts counts() const override { return Counts{ 0, n_segs_ }; }

private:
  // the text of a slot is that of these segments (comp_bit inside the slot's compressed bytes, dict_off inside its histories)
  struct Table
  {
    std::vector<grp_gzip_segment> segs; // tab_cap_ entries
    size_t n_segs = 0, comp_n = 0, dict_n = 0;
    uint64_t comp_file_off = 0;
  };
  PathRun& run_;
  std::shared_ptr<GzIndex> ix_; // the run's index, as it was when this pass began
  int fd_;
  size_t next_ = 0; // the first segment of the next slot
  size_t comp_cap_ = 0, dict_cap_ = 0, tab_cap_ = 0;
  std::vector<Table> slot_;
  uint64_t n_segs_ = 0;
};

// Which feed reads run.opt.input (`in` is the source's own view of it, `chunk` the text of a slot as asked for).
//   BGZF (grp_engine_ext::bgzf_inflate; GRP_BGZF=off: no): the first member is a complete BGZF member.
//   A file that is gzip from its first byte and not taken by the BGZF form (grp_engine_ext::gzip_inflate;
//   GRP_GZIP_INDEX=off: no): its segments where the run has an index of it — a file that changed between two passes
//   drops it, an index with a segment larger than a slot is not used — else text through GzIndexReader, which builds one.
//   Everything else: text.
std::unique_ptr<Feed>
open_feed(PathRun& run, InputFile& in, size_t chunk)
{
  const std::string& path = run.opt.input;
  const char* e = getenv("GRP_BGZF");
  if (run.ext.bgzf_inflate && !(e && !strcmp(e, "off"))) {
    // is the first member a complete BGZF member?  (a member is at most 64 KiB; a pipe cannot be pread: zlib)
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd >= 0) {
      std::vector<unsigned char> head(BGZF_MAX_MEMBER);
      const ssize_t k = pread(fd, head.data(), head.size(), 0);
      grp_bgzf_block b;
      if (k > 0 && bgzf_scan(head.data(), (size_t)k, &b, 1, nullptr, nullptr) == 1) {
        return std::unique_ptr<Feed>(new BgzfFeed(run, fd));
      }
      ::close(fd);
    }
  }
  std::unique_ptr<GzIndexReader> build;
  if (run.ext.gzip_inflate && gzip_index_enabled()) {
    if (run.gzidx && !run.gzidx->matches(path)) {
      run.gzidx.reset(); // the file was written since: this pass builds a new one
    }
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    struct stat st;
    unsigned char magic[2] = { 0, 0 };
    const bool gz = fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (gz && run.gzidx && run.gzidx->max_text <= chunk) { // (a larger segment: the whole pass goes through zlib)
      return std::unique_ptr<Feed>(new GzipSegFeed(run, fd));
    }
    if (gz && !run.gzidx) {
      build.reset(new GzIndexReader(path, gzip_index_span(), gzip_index_max_bytes()));
      if (!build->ok()) {
        build.reset();
      }
    }
    if (fd >= 0) {
      ::close(fd);
    }
  }
  return std::unique_ptr<Feed>(new TextFeed(run, in, std::move(build)));
}

// What a regular file's data begins with, decompressed if it is gzip (input_format: 1 FASTQ, 2 BAM, 0 neither), through a
// view of its own on the file; -1: not a regular file — a pipe can only be peeked at, and BAM is not looked for there.
int
probe_format(const std::string& path)
{
  struct stat st;
  if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
    return -1;
  }
  InputFile probe(path);
  unsigned char head[4] = { 0, 0, 0, 0 };
  const size_t n = probe.ok() ? probe.read(reinterpret_cast<char*>(head), sizeof(head)) : 0;
  return input_format(head, n);
}

// Raw text chunks parsed, filtered and packed on the GPU (grpath_ingest.h).  An unaligned BAM input (gr_bam.hpp) takes the
// same way: the feeds deliver its bytes, the header is skipped in front of the first parse — it may span chunks: the
// carry of partial records holds it until it is complete — and grp_engine_ext::bam_parse stands where fastq_parse does.
// A reader thread keeps the NEXT chunk of the input coming (Feed::fill) while the caller works on the current one —
// inflate, upload, parse, pack, fill or classify — so a pass costs max(read, GPU) per chunk instead of their sum.  Four
// slots in ONE page-locked buffer; every slot has room in front of the bytes read for the unconsumed tail of
// the chunk before it (a partial record), which is copied there before the parse.
class GpuSource : public RecordSource
{
public:
  GpuSource(PathRun& run, int format)
    : run_(run)
    , in_(run.opt.input)
    , format_(format)
  {
    chunk_ = std::max<size_t>(ingest_chunk_bytes(), 64);
    feed_ = open_feed(run_, in_, chunk_);
    const Feed::Sizes sz = feed_->layout(chunk_, kSlots);
    chunk_ = sz.chunk;
    comp_cap_ = sz.comp;
    dict_cap_ = sz.dict;
    if (in_.plain_size() != 0) { // a small file: one slot holds it all, no 2 x 256 MiB to allocate and page-lock
      chunk_ = std::min<size_t>(chunk_, std::max<size_t>((size_t)in_.plain_size() + 1, size_t(1) << 16));
    }
    front_ = std::min<size_t>(std::max<size_t>(chunk_ / 16, 4096), (size_t)GRP_FASTQ_PREFETCH_FRONT); // (what a prefetched body may have in front of it, grpath_ingest.h)
    buf_.resize((size_t)kSlots * (front_ + chunk_ + comp_cap_ + dict_cap_)); // (the compressed bytes of the slots behind their texts, the histories behind those: one page-locked buffer)
    const char* pin_min = getenv("GRP_PIN_MIN_BYTES"); // tests: page-lock small buffers too
    if (run_.vt.fastq_pin && run_.vt.fastq_unpin && buf_.size() >= (pin_min ? (size_t)atoll(pin_min) : (size_t(8) << 20))) {
      pinned_ = run_.vt.fastq_pin(run_.ctx, buf_.data(), buf_.size()) == GRP_OK;
    }
  }
  ~GpuSource() override
  {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    if (reader_.joinable()) {
      reader_.join();
    }
    release();
    if (run_.vt.fastq_prefetch) {
      (void)run_.vt.fastq_prefetch(run_.ctx, nullptr, 0); // bodies handed over ahead of a parse that never came (an early end)
    }
    if (getenv("GRP_TRACE_INGEST")) {
      const Feed::Counts n = feed_->counts();
      std::cerr << "GRP_TRACE_INGEST source: " << n_pre_[0] << " chunks, next chunk not ready at " << n_pre_[1] << ", uploads started ahead " << n_pre_[2] << "; seconds waiting for the reader " << t_tr_[0]
                << ", in fastq_parse " << t_tr_[1] << ", in fastq_prefetch " << t_tr_[2] << ", copying tails " << t_tr_[3] << ", BGZF blocks inflated on the device " << n.bgzf_blocks
                << ", gzip segments inflated on the device " << n.gzip_segs << std::endl;
    }
    feed_.reset();
    if (pinned_) {
      run_.vt.fastq_unpin(run_.ctx); // before the buffer goes away: the engine cannot know when the host frees memory
    }
  }
  bool ok() const override { return in_.ok(); }
  bool is_fastq() override { return format_ < 0 ? in_.peek() == '@' : format_ != 0; } // (asked before the first chunk is read)
  bool next(Batch& b) override
  {
    release();
    if (!reader_.joinable() && !done_) {
      reader_ = std::thread([this] { read_loop(); });
    }
    while (!done_) {
      // the slot handed out by the previous call goes back to the reader, the next one is awaited
      Slot* sl = nullptr;
      {
        std::unique_lock<std::mutex> g(mu_);
        if (held_ >= 0) {
          slot_[held_].uploaded = false;
          slot_[held_].state = Slot::FREE;
          held_ = -1;
          cv_.notify_all();
        }
        const double tw0 = now_s();
        cv_.wait(g, [&] { return slot_[take_].state == Slot::READY; });
        t_tr_[0] += now_s() - tw0;
        sl = &slot_[take_];
        held_ = take_;
        take_ = (take_ + 1) % kSlots;
      }
      if (!inflate_slot(held_)) { // (the failure is noted: the run ends with an error behind this pass)
        done_ = true;
        break;
      }
      const bool eof = sl->eof;
      char* data = slot_data(held_);
      // the tail of the chunk before, in front of what was read
      char* text = nullptr;
      size_t fill = carry_.size() + sl->n;
      if (carry_.size() <= front_) {
        text = data - carry_.size();
        if (!carry_.empty()) { // (a prefetch reads the slot's body only: the room in front of it is free to write)
          const double tc0 = now_s();
          memcpy(text, carry_.data(), carry_.size());
          t_tr_[3] += now_s() - tc0;
        }
      } else {
        // a record longer than a chunk: assembled in a buffer of its own (pageable; rare)
        big_.resize(fill);
        memcpy(big_.data(), carry_.data(), carry_.size());
        memcpy(big_.data() + carry_.size(), data, sl->n);
        text = big_.data();
      }
      uint64_t text_off = sl->file_off - carry_.size(); // stream offset of text[0]
      if (fill == 0) {
        done_ = true;
        break;
      }
      uint64_t n_rec = 0, used = 0;
      int stopped = 0;
      const bool bam = format_ == 2;
      if (bam && !bam_header_done_) {
        // the records begin behind the header; one that is not complete yet consumes nothing
        uint64_t hb = 0;
        const int hrc = bam_header(reinterpret_cast<const uint8_t*>(text), fill, &hb);
        if (hrc == 0 && !eof) {
          release();
          carry_.assign(text, text + fill);
          continue;
        }
        if (hrc != 1) {
          note_bam_failure(run_.opt.input, text_off, hrc == 0 ? "the stream ends inside the BAM header (truncated)" : "not a BAM header");
          done_ = true;
          break;
        }
        bam_header_done_ = true;
        text += hb;
        fill -= hb;
        text_off += hb;
        if (fill == 0 && eof) { // a header and no record
          done_ = true;
          break;
        }
      }
      const double tp0 = now_s();
      uint64_t bad_off = 0;
      const int prc = bam ? run_.ext.bam_parse(run_.ctx, text, fill, eof ? 1 : 0, &fq_, &n_rec, &used, &bad_off)
                          : run_.vt.fastq_parse(run_.ctx, text, fill, eof ? 1 : 0, &fq_, &n_rec, &used, &stopped);
      t_tr_[1] += now_s() - tp0;
      if (prc == GRP_ERR_INVALID && bam) { // a refused record: the input's failure, not the engine's
        note_bam_failure(run_.opt.input, text_off + bad_off, run_.vt.last_error ? run_.vt.last_error(run_.ctx) : nullptr);
        done_ = true;
        break;
      }
      if (prc != GRP_OK) {
        std::cerr << "goldrush-path: FASTQ ingest: " << (run_.vt.last_error ? run_.vt.last_error(run_.ctx) : "failed") << std::endl;
        failed_ = true;
        done_ = true;
        break;
      }
      if (n_rec == 0 && !eof && !stopped) {
        // not one complete record yet: everything is carried into the next chunk
        release();
        carry_.assign(text, text + fill);
        continue;
      }
      carry_.assign(text + used, text + fill);
      if (eof || stopped) {
        done_ = true;
      }
      if (n_rec == 0) {
        release();
        continue;
      }
      meta_.resize(n_rec);
      run_.vt.fastq_records(fq_, meta_.data());
      b.text = text;
      b.base_off = text_off;
      b.rec.resize(n_rec);
      for (size_t i = 0; i < n_rec; ++i) {
        const grp_fastq_record& m = meta_[i];
        b.rec[i] = Rec{ (size_t)m.id_off, m.id_len, (size_t)m.seq_off, m.seq_len, (size_t)m.qual_off, m.qual_len };
      }
      b.seq_is_upper = false;
      b.bam = bam;
      prefetch_next();
      return true;
    }
    return false;
  }
  // The uploads of the next TWO chunks' bodies, started as soon as the reader has them (round 5).  A copy issued behind the
  // fill of the current chunk only begins when that has ended (tools/dev/r5_ingest_timeline.sh: fill, then copy, then parse,
  // one after the other); issued one chunk ahead — with the tail of the chunk before copied in front first — it still lay on
  // the path of every chunk (copy 5.5 ms + parse + the host's share against a fill of 7 ms).  The body does not depend on
  // that tail: it goes up two chunks ahead, the engine leaves room in front of it and the parse uploads the tail alone
  // (grpath_ingest.h: grp_fastq_prefetch).
  void prefetch_next()
  {
    ++n_pre_[0];
    if (!run_.vt.fastq_prefetch || done_) {
      return;
    }
    for (int ahead = 0; ahead < 2; ++ahead) {
      const int j = (take_ + ahead) % kSlots;
      size_t n = 0;
      {
        std::lock_guard<std::mutex> g(mu_);
        if (slot_[j].state != Slot::READY) {
          n_pre_[1] += ahead == 0;
          return; // the reader is still at it (and the slots behind it are not ready either)
        }
        if (slot_[j].eof && slot_[j].n == 0) {
          return;
        }
        n = slot_[j].n; // (a READY slot is the consumer's until it releases it)
      }
      if (slot_[j].uploaded || n == 0) {
        continue;
      }
      if (!inflate_slot(j)) {
        return;
      }
      const double tq0 = now_s();
      const int qrc = run_.vt.fastq_prefetch(run_.ctx, slot_data(j), n);
      t_tr_[2] += now_s() - tq0;
      if (qrc != GRP_OK) {
        return; // no free buffer on the device: later
      }
      slot_[j].uploaded = true;
      ++n_pre_[2];
    }
  }
  void stats(Batch& b, size_t min_len, bool) override
  {
    const size_t n = b.rec.size();
    b.avg.assign(n, 0);
    b.delta.assign(n, 0);
    b.non_acgt.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      b.non_acgt[i] = (meta_[i].flags & GRP_FQ_NON_ACGT) ? 1 : 0;
      if (b.rec[i].seq_len >= min_len) {
        // the device summed left to right in double; log10 / truncation happen here
        phred_from_sums(meta_[i].phred_sum, meta_[i].phred_first, b.rec[i].qual_len, b.avg[i], b.delta[i]);
      }
    }
  }
  int upload(Batch& b, const std::vector<uint32_t>& sel, std::vector<uint32_t>& lens, void** reads) override
  {
    lens.resize(sel.size());
    for (size_t i = 0; i < sel.size(); ++i) {
      lens[i] = (uint32_t)b.rec[sel[i]].seq_len;
    }
    return run_.vt.fastq_pack(run_.ctx, fq_, sel.data(), (uint32_t)sel.size(), reads);
  }
  bool failed() const { return failed_; }

private:
  struct Slot
  {
    enum State { FREE, READY } state = FREE;
    size_t n = 0;          // bytes of text
    uint64_t file_off = 0; // stream offset of the first of them
    bool eof = false;      // the data ends with this chunk
    bool uploaded = false; // consumer's: the engine has been handed the body ahead of its parse (prefetch_next)
    bool inflated = false, bad = false; // consumer's: Feed::inflate has run / has failed
  };
  char* slot_data(int i) { return buf_.data() + (size_t)i * (front_ + chunk_) + front_; }
  SlotBuf slot_buf(int i)
  {
    unsigned char* side = reinterpret_cast<unsigned char*>(buf_.data()) + (size_t)kSlots * (front_ + chunk_);
    return SlotBuf{ slot_data(i), side + (size_t)i * comp_cap_, side + (size_t)kSlots * comp_cap_ + (size_t)i * dict_cap_ };
  }
  // the slot's text is there (once); false: the engine refused a part of it
  bool inflate_slot(int j)
  {
    Slot& sl = slot_[j];
    if (!sl.inflated) {
      sl.inflated = true;
      sl.bad = !feed_->inflate(j, slot_buf(j), chunk_);
    }
    return !sl.bad;
  }
  void read_loop()
  {
    uint64_t off = 0;
    for (int i = 0;; i = (i + 1) % kSlots) {
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return stop_ || slot_[i].state == Slot::FREE; });
        if (stop_) {
          return;
        }
      }
      bool eof = false;
      slot_[i].inflated = slot_[i].bad = false; // (a FREE slot is the reader's)
      const size_t got = feed_->fill(i, slot_buf(i), chunk_, eof);
      {
        std::lock_guard<std::mutex> g(mu_);
        slot_[i].n = got;
        slot_[i].file_off = off;
        slot_[i].eof = eof;
        slot_[i].state = Slot::READY;
      }
      cv_.notify_all();
      off += got;
      if (eof) {
        return;
      }
    }
  }
  void release()
  {
    if (fq_) {
      run_.vt.fastq_free(fq_);
      fq_ = nullptr;
    }
  }
  PathRun& run_;
  InputFile in_;
  std::unique_ptr<Feed> feed_;
  std::vector<char> buf_;  // kSlots x [front | chunk], then what the feed asked for beside them
  uint64_t n_pre_[3] = { 0, 0, 0 }; // developer trace: chunks returned, next slot not ready, prefetches the engine took
  double t_tr_[4] = { 0, 0, 0, 0 };  // developer trace: seconds waiting for the reader / in the parse call / in the prefetch calls / copying tails
  std::vector<char> carry_; // unconsumed tail of the chunk before
  std::vector<char> big_;
  size_t chunk_ = 0, front_ = 0;
  size_t comp_cap_ = 0, dict_cap_ = 0; // the capacities of a slot beside its text (Feed::Sizes)
  bool pinned_ = false;
  std::thread reader_;
  std::mutex mu_;
  std::condition_variable cv_;
  // four chunk buffers (round 5; two before): the caller's batch lives in one, the bodies of the next two have been handed to
  // the engine ahead (prefetch_next) and the reader fills the fourth
  static constexpr int kSlots = 4;
  Slot slot_[kSlots];
  int take_ = 0;  // the slot the next chunk arrives in
  int held_ = -1; // the slot the caller's current batch lives in
  bool stop_ = false;
  bool done_ = false, failed_ = false;
  const int format_;             // probe_format of the input
  bool bam_header_done_ = false; // BAM: the header has been skipped
  void* fq_ = nullptr;
  std::vector<grp_fastq_record> meta_;
};

} // namespace

std::unique_ptr<RecordSource>
open_source(PathRun& run)
{
  const bool gpu = run.vt.fastq_parse && run.vt.fastq_records && run.vt.fastq_pack && run.vt.fastq_free && !getenv("GRP_HOST_INGEST");
  const int format = gpu ? probe_format(run.opt.input) : 0;
  if (gpu && !(format == 2 && !run.ext.bam_parse)) { // (a BAM file and an engine without bam_parse: the host reader)
    return std::unique_ptr<RecordSource>(new GpuSource(run, format));
  }
  return std::unique_ptr<RecordSource>(new HostSource(run));
}

} // namespace gr
