// The record sources (gr_source.hpp): the host reader, and the slot pipeline that feeds the engine's ingest from text,
// BGZF members or the segments of an indexed gzip file.
#include "gr_source.hpp"
#include "gr_bgzf.hpp"
#include "gr_fastq.hpp"
#include "gr_gzwalk.hpp"
#include "gr_params.hpp"

#include <algorithm>
#include <atomic>
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

void
PathRun::note_bam_aligned(size_t file, uint64_t skipped, uint64_t reversed)
{
  if (bam_aligned.size() < files.size()) {
    bam_aligned.resize(files.size());
  }
  if (!bam_aligned[file].counted) {
    bam_aligned[file].counted = true;
    bam_aligned[file].skipped = skipped;
    bam_aligned[file].reversed = reversed;
  }
}

void
PathRun::say_bam_aligned()
{
  for (size_t f = 0; f < bam_aligned.size(); ++f) {
    BamAligned& a = bam_aligned[f];
    if (a.counted && !a.said && (a.skipped || a.reversed)) {
      std::cerr << "GRP_BAM_ALIGNED: " << files[f] << ": " << a.skipped << " secondary or supplementary records skipped, " << a.reversed << " reverse-strand records read as their reverse complement" << std::endl;
    }
    a.said = a.said || a.counted;
  }
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
    , fq_(new FastqStream(run.files[0], run.bam_accept))
  {}
  // (several files: check_inputs has looked at every one of them before the first pass)
  bool ok() const override { return run_.files.size() > 1 || fq_->ok(); }
  bool is_fastq() override { return run_.files.size() > 1 || fq_->is_fastq(); }
  bool next(Batch& b) override
  {
    // a file's reader hands out that file's records to its end — as it would on its own — and the next file's takes over
    while (!fq_->next_batch(rb_, BATCH_RECORDS, BATCH_BASES)) {
      if (!input_failed()) { // the file has been read to its end
        run_.note_bam_aligned(file_, fq_->bam_skipped(), fq_->bam_reversed());
      }
      if (file_ + 1 >= run_.files.size() || input_failed()) {
        return false;
      }
      fq_.reset(new FastqStream(run_.files[++file_], run_.bam_accept));
    }
    b.file = file_;
    b.base_off = 0;
    b.bam = false;
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
    lens.reserve(1); // (a file whose every record is filtered out is a batch without a read: still an array to point at)
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
  size_t file_ = 0; // the file being read
  std::unique_ptr<FastqStream> fq_;
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
  // once, before the first fill: the slots have these sizes — what the feeds of all the pass's files asked for
  // (FilePlan::want), so at least what this one did (a feed sizes its per-slot tables here)
  virtual void layout(const Sizes& /*slot*/, int /*n_slots*/) {}
  // reader thread: the next up to `chunk` bytes of text for the slot; eof: the data ends with them
  virtual size_t fill(int slot, const SlotBuf& b, size_t chunk, bool& eof) = 0;
  // consumer thread: the slot's text is there; false: the engine refused it (the failure is noted)
  virtual bool inflate(int /*slot*/, const SlotBuf&, size_t /*chunk*/) { return true; }
  virtual Counts counts() const { return Counts{}; }
  // the first byte of the data without consuming it (-1: none; a feed of compressed bytes does not look: -2)
  virtual int peek() { return -2; }
  virtual bool ok() const { return true; } // the file could be opened
};

// Text: InputFile (parallel pread of a plain file, zlib for gzip data), or GzIndexReader — zlib as before, on the reader
// thread — in the first pass over a plain gzip file, which leaves the index of its restart points in the run when it
// reads the file to its end.  A pass that ends early (the Phred median) leaves no index.
class TextFeed : public Feed
{
public:
  TextFeed(PathRun& run, size_t file, std::unique_ptr<InputFile> in, std::unique_ptr<GzIndexReader> build)
    : run_(run)
    , file_(file)
    , in_(std::move(in))
    , build_(std::move(build))
  {}
  int peek() override { return in_->peek(); }
  bool ok() const override { return in_->ok(); }
  size_t fill(int, const SlotBuf& b, size_t chunk, bool& eof) override
  {
    size_t got = 0;
    while (!eof && got < chunk) {
      const size_t k = build_ ? build_->read(b.text + got, chunk - got) : in_->read(b.text + got, chunk - got);
      if (k == 0) {
        eof = true;
      }
      got += k;
    }
    if (eof && build_ && build_->complete()) {
      run_.gzidx[file_] = build_->take(); // (read by the next pass's source, which begins behind this thread's end)
    }
    return got;
  }

private:
  PathRun& run_;
  const size_t file_; // which of the run's files (its index goes to PathRun::gzidx[file_])
  std::unique_ptr<InputFile> in_;
  std::unique_ptr<GzIndexReader> build_;
};

// A BGZF-compressed file (gr_bgzf.hpp) whose members the engine can inflate: the reader thread reads COMPRESSED bytes
// and walks the members' headers; a slot is filled with whole members until its text, its compressed bytes or its block
// table is full.  Plain gzip is one serial stream and stays with zlib: from a member in mid-file that is not BGZF on
// (bgzip output followed by gzip output) a text feed reads the rest.
class BgzfFeed : public Feed
{
public:
  BgzfFeed(PathRun& run, size_t file, int fd)
    : run_(run)
    , file_(file)
    , path_(run.files[file])
    , fd_(fd)
    , map_(new BgzfMap)
  {}
  ~BgzfFeed() override { ::close(fd_); }
  static Sizes want(size_t chunk)
  {
    chunk = std::max<size_t>(chunk, BGZF_MAX_TEXT); // a tiny GRP_INGEST_CHUNK still holds one member
    return Sizes{ chunk, std::max<size_t>(chunk / 2, BGZF_MAX_MEMBER), 0 };
  }
  void layout(const Sizes& slot, int n_slots) override
  {
    comp_cap_ = slot.comp;
    tab_cap_ = std::max<size_t>(slot.chunk / 4096, 64);
    slot_.resize((size_t)n_slots);
    for (Table& t : slot_) {
      t.blocks.resize(tab_cap_);
    }
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
      note_input_failure("reading " + path_ + " failed: BGZF member " + (bad != UINT32_MAX ? "at byte " + std::to_string(at) : "in the chunk at byte " + std::to_string(at)) + ": " +
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
            note_input_failure("reading " + path_ + " failed at byte " + std::to_string(off_ + have + k) + ": " + strerror(err));
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
            note_input_failure("reading " + path_ + " failed: the file ends inside the BGZF member at byte " + std::to_string(off_ + pos) + " (truncated)");
          }
          eof = true;
          break;
        } else if (have == comp_cap_) {
          full = true;
        }
      }
      for (size_t t = 0; map_ && t < nb; ++t) { // (comp_off: in the slot's bytes, which begin at off_ in the file)
        map_->add(off_ + sl.blocks[t].comp_off, sl.blocks[t].comp_len, sl.blocks[t].text_len, sl.blocks[t].crc32);
      }
      off_ += pos;
      sl.n_blocks = nb;
      sl.comp_n = pos;
      if (other) {
        map_.reset(); // (the rest of the file is zlib's: no random access into it)
      } else if (eof && map_ && !input_failed()) {
        run_.bgzf_map[file_] = std::move(map_); // (read behind this pass, like PathRun::gzidx)
      }
      if (other) {
        // from this member on zlib reads, from a descriptor of its own that stands there
        const int fd = ::open(path_.c_str(), O_RDONLY | O_CLOEXEC);
        std::unique_ptr<InputFile> tail_in;
        if (fd >= 0 && lseek(fd, (off_t)off_, SEEK_SET) == (off_t)off_) {
          tail_in.reset(new InputFile(path_, fd));
        } else if (fd >= 0) {
          ::close(fd);
        }
        if (tail_in && tail_in->ok()) {
          tail_.reset(new TextFeed(run_, file_, std::move(tail_in), nullptr));
        } else {
          note_input_failure("reading " + path_ + " failed: cannot read on behind the BGZF members at byte " + std::to_string(off_));
          eof = true;
        }
      }
      if (text != 0 || eof || other) {
        return text;
      }
    }
  }
  PathRun& run_;
  const size_t file_;
  const std::string path_;
  int fd_;           // the reader's descriptor ...
  uint64_t off_ = 0; // ... and how far it has come
  size_t comp_cap_ = 0, tab_cap_ = 0;
  std::vector<Table> slot_;
  std::unique_ptr<TextFeed> tail_; // what follows the BGZF members, read as text
  std::shared_ptr<BgzfMap> map_;   // the members walked so far; published in the run at the file's end
  uint64_t n_blocks_ = 0;
};

// A plain gzip file in the passes behind the one that left its index in the run: the reader thread preads whole
// SEGMENTS into a slot until its text, its compressed bytes, its histories or its table is full, and the consumer has
// the engine inflate them, exactly like the members of a BGZF file.  The compressed bytes of a slot are one range of the
// file (with the trailers and headers between two members in it).
class GzipSegFeed : public Feed
{
public:
  GzipSegFeed(PathRun& run, size_t file, int fd)
    : run_(run)
    , path_(run.files[file])
    , ix_(run.gzidx[file])
    , fd_(fd)
  {}
  ~GzipSegFeed() override { ::close(fd_); }
  static Sizes want(size_t chunk, const GzIndex& ix)
  {
    return Sizes{ chunk, std::max<size_t>(chunk / 2, (size_t)ix.max_comp + 8), chunk / 8 + 32768 }; // (32 KiB of history per 256 KiB of text at the default span)
  }
  void layout(const Sizes& slot, int n_slots) override
  {
    comp_cap_ = slot.comp;
    dict_cap_ = slot.dict;
    tab_cap_ = std::max<size_t>(slot.chunk / 4096, 64);
    slot_.resize((size_t)n_slots);
    for (Table& t : slot_) {
      t.segs.resize(tab_cap_);
    }
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
      note_input_failure("reading " + path_ + " failed at byte " + std::to_string(byte0 + k) + ": " + (err ? strerror(err) : "the file ends in front of a segment of its index (it was written during the run)"));
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
      note_input_failure("reading " + path_ + " failed: gzip segment " + (bad < sl.n_segs ? "" : "in the chunk ") + "at byte " + std::to_string(bit >> 3) + " (bit " + std::to_string(bit & 7) + "): " +
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
  const std::string path_;
  std::shared_ptr<GzIndex> ix_; // the run's index of this file, as it was when this pass began
  int fd_;
  size_t next_ = 0; // the first segment of the next slot
  size_t comp_cap_ = 0, dict_cap_ = 0, tab_cap_ = 0;
  std::vector<Table> slot_;
  uint64_t n_segs_ = 0;
};

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

// How one file of a pass is read, decided when the pass begins — the slots are allocated once, for what the feeds of all
// its files ask for — and carried out by open_feed when the reader thread comes to the file.  No descriptor is held in
// between: a pass may have more files than a process may have descriptors.
//   BGZF (grp_engine_ext::bgzf_inflate; GRP_BGZF=off: no): the first member is a complete BGZF member.
//   A file that is gzip from its first byte and not taken by the BGZF form (grp_engine_ext::gzip_inflate;
//   GRP_GZIP_INDEX=off: no): its segments where the run has an index of it — a file that changed between two passes
//   drops its index, an index with a segment larger than a slot is not used — else text through GzIndexReader, which
//   builds one.
//   Everything else: text.
struct FilePlan
{
  enum Kind { TEXT, BGZF, GZSEG } kind = TEXT;
  bool build_index = false; // TEXT: a gzip file without an index, read through GzIndexReader
  bool plain = false;       // a plain regular file, read with pread (InputFile) ...
  uint64_t plain_size = 0;  // ... and its bytes
  Feed::Sizes want{ 0, 0, 0 };
};

FilePlan
plan_feed(PathRun& run, size_t file, size_t chunk)
{
  const std::string& path = run.files[file];
  FilePlan pl;
  pl.want = Feed::Sizes{ chunk, 0, 0 };
  const FileProbe p = probe_file(path);
  if (!p.opened) {
    return pl;
  }
  const bool regular = p.regular, gz = p.magic == FileProbe::GZIP;
  const char* e = getenv("GRP_BGZF");
  if (gz && run.ext.bgzf_inflate && !(e && !strcmp(e, "off"))) {
    // is the first member a complete BGZF member?  (a member is at most 64 KiB)
    std::vector<unsigned char> head(BGZF_MAX_MEMBER);
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    int err = 0;
    const size_t k = pread_full(fd, head.data(), head.size(), 0, &err);
    if (fd >= 0) {
      ::close(fd);
    }
    grp_bgzf_block b;
    if (k > 0 && bgzf_scan(head.data(), k, &b, 1, nullptr, nullptr) == 1) {
      pl.kind = FilePlan::BGZF;
      pl.want = BgzfFeed::want(chunk);
    }
  }
  if (pl.kind == FilePlan::TEXT && run.ext.gzip_inflate && gzip_index_enabled()) {
    std::shared_ptr<GzIndex>& ix = run.gzidx[file];
    if (ix && !ix->matches(path)) {
      ix.reset(); // the file was written since: this pass builds a new one
    }
    if (gz && ix && ix->max_text <= chunk) { // (a larger segment: the file goes through zlib in this pass too)
      pl.kind = FilePlan::GZSEG;
      pl.want = GzipSegFeed::want(chunk, *ix);
    }
    pl.build_index = gz && !ix;
  }
  if (pl.kind == FilePlan::TEXT && regular && !gz && !getenv("GRP_ZLIB_READER")) {
    pl.plain = true;
    pl.plain_size = p.size;
  }
  return pl;
}

// GRP_GZIP_WALK=on, once per run, where the plans of the first pass's files are about to be made: every file that
// plan_feed would read as text through GzIndexReader — gzip, not routed to the BGZF form, without an index, on an engine
// that inflates segments — is walked on the device, all of them side by side (gr_gzwalk.hpp).  A file the walk completes
// has its index in PathRun::gzidx and plan_feed chooses GzipSegFeed by itself; every other file is read as without the walk.
// With GRP_GZIP_WALK_MEMBERS=on the members of a file are walked side by side too (GzWalkMembers): the indexes are the same.
void
walk_gzip_files(PathRun& run)
{
  if (run.gzip_walked) {
    return;
  }
  run.gzip_walked = true;
  if (!run.gzip_walk || !run.ext.gzip_walk || !run.ext.gzip_inflate || !gzip_index_enabled()) {
    return;
  }
  const char* e = getenv("GRP_BGZF");
  const bool bgzf_routed = run.ext.bgzf_inflate && !(e && !strcmp(e, "off"));
  std::vector<size_t> which;
  std::vector<std::string> paths;
  std::vector<unsigned char> head(BGZF_MAX_MEMBER);
  for (size_t f = 0; f < run.files.size(); ++f) {
    const FileProbe p = probe_file(run.files[f]);
    if (!p.opened || !p.regular || p.magic != FileProbe::GZIP || run.gzidx[f]) {
      continue;
    }
    if (bgzf_routed) { // (plan_feed's test: is the first member a complete BGZF member?)
      const int fd = ::open(run.files[f].c_str(), O_RDONLY | O_CLOEXEC);
      int err = 0;
      const size_t k = pread_full(fd, head.data(), head.size(), 0, &err);
      if (fd >= 0) {
        ::close(fd);
      }
      grp_bgzf_block b;
      if (k > 0 && bgzf_scan(head.data(), k, &b, 1, nullptr, nullptr) == 1) {
        continue;
      }
    }
    which.push_back(f);
    paths.push_back(run.files[f]);
  }
  GzWalkStats st;
  if (!paths.empty()) {
    const auto launch = [&run](const uint8_t* comp, uint64_t n_comp, const uint8_t* dict, uint64_t n_dict, const grp_gzip_walk_step* steps, uint32_t n, grp_gzip_walk_result* res, uint8_t* hist) {
      return run.ext.gzip_walk(run.ctx, comp, n_comp, dict, n_dict, steps, n, res, hist, nullptr, 0, nullptr) == GRP_OK;
    };
    GzWalkBuffer pin, unpin;
    if (run.vt.fastq_pin && run.vt.fastq_unpin) { // the windows of all files: one page-locked buffer (the source pins its own behind the walk)
      pin = [&run](uint8_t* buf, size_t n) { (void)run.vt.fastq_pin(run.ctx, reinterpret_cast<const char*>(buf), n); };
      unpin = [&run](uint8_t*, size_t) { (void)run.vt.fastq_unpin(run.ctx); };
    }
    std::vector<GzWalkFile> got = gzip_walk(paths, gzip_index_span(), gzip_index_max_bytes(), gzip_walk_sizes(), launch, &st, pin, unpin, run.gzip_walk_members);
    for (size_t i = 0; i < got.size(); ++i) {
      if (got[i].index) {
        run.gzidx[which[i]] = std::move(got[i].index);
      }
    }
  }
  if (getenv("GRP_TRACE_INGEST") && run.rank == 0) {
    std::cerr << "GRP_TRACE_INGEST gzip walk: files=" << st.files << " walked=" << st.walked << " left_to_zlib=" << st.left_to_zlib << " rounds=" << st.rounds << " text=" << st.text_bytes << " seconds=" << st.seconds << std::endl;
    if (run.gzip_walk_members.on) {
      std::cerr << "GRP_TRACE_INGEST gzip walk members: candidates=" << st.candidates << " streams=" << st.streams << " adopted=" << st.adopted << " dropped=" << st.dropped << " max_in_flight=" << st.max_in_flight
                << " wasted_text=" << st.wasted_text << " scan_seconds=" << st.scan_seconds << std::endl;
    }
  }
}

std::unique_ptr<Feed>
open_feed(PathRun& run, size_t file, const FilePlan& pl)
{
  const std::string& path = run.files[file];
  run.bgzf_map[file].reset(); // (the map of the pass before: this pass writes its own, or the file has none)
  if (pl.kind != FilePlan::TEXT) {
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd >= 0) {
      return pl.kind == FilePlan::BGZF ? std::unique_ptr<Feed>(new BgzfFeed(run, file, fd)) : std::unique_ptr<Feed>(new GzipSegFeed(run, file, fd));
    }
    note_input_failure("reading " + path + " failed: it cannot be opened again: " + strerror(errno));
  }
  std::unique_ptr<GzIndexReader> build;
  if (pl.kind == FilePlan::TEXT && pl.build_index) {
    build.reset(new GzIndexReader(path, gzip_index_span(), gzip_index_max_bytes()));
    if (!build->ok()) {
      build.reset();
    }
  }
  return std::unique_ptr<Feed>(new TextFeed(run, file, std::unique_ptr<InputFile>(new InputFile(path)), std::move(build)));
}

// Raw text chunks parsed, filtered and packed on the GPU (grpath_ingest.h).  An unaligned BAM input (gr_bam.hpp) takes the
// same way: the feeds deliver its bytes, the header is skipped in front of the first parse — it may span chunks: the
// carry of partial records holds it until it is complete — and grp_engine_ext::bam_parse stands where fastq_parse does
// (bam_parse_ex with GRP_BAM_ALIGNED=on: reverse-strand records come back with GRP_FQ_REVERSED, secondary and supplementary
// ones are consumed without an entry).
// A reader thread keeps the NEXT chunk of the input coming (Feed::fill) while the caller works on the current one —
// inflate, upload, parse, pack, fill or classify — so a pass costs max(read, GPU) per chunk instead of their sum.  Four
// slots in ONE page-locked buffer; every slot has room in front of the bytes read for the unconsumed tail of
// the chunk before it (a partial record), which is copied there before the parse.
//
// Several files: ONE source, one buffer, one reader thread and one pin for the pass.  At a file's end the
// reader opens the next file's feed and goes on filling slots, so the next file's first chunk is on its way while the
// consumer still works on the last chunks of the file before.  A slot says which file it belongs to, whether it is that
// file's first and whether it is its last; the consumer parses a file's last chunk as a final one, begins every file
// without a carried tail (and, BAM, with its header) and takes the format from the slot.  A feed lives from the reader's
// first fill of its file to the consumer's inflate of that file's last slot.
class GpuSource : public RecordSource
{
public:
  GpuSource(PathRun& run, const std::vector<int>& format)
    : run_(run)
    , format_(format)
  {
    const size_t n_files = run.files.size();
    chunk_ = std::max<size_t>(ingest_chunk_bytes(), 64);
    plan_.resize(n_files);
    feeds_.resize(n_files);
    walk_gzip_files(run_);
    Feed::Sizes sz{ chunk_, 0, 0 };
    uint64_t largest = 0; // plain files, all of known size: the largest of them
    bool sized = true;
    for (size_t f = 0; f < n_files; ++f) {
      plan_[f] = plan_feed(run_, f, chunk_);
      sz.chunk = std::max(sz.chunk, plan_[f].want.chunk);
      sz.comp = std::max(sz.comp, plan_[f].want.comp);
      sz.dict = std::max(sz.dict, plan_[f].want.dict);
      sized = sized && plan_[f].plain;
      largest = std::max(largest, plan_[f].plain_size);
    }
    chunk_ = sz.chunk;
    comp_cap_ = sz.comp;
    dict_cap_ = sz.dict;
    if (sized && largest != 0) { // small files: one slot holds any of them, no 2 x 256 MiB to allocate and page-lock
      chunk_ = std::min<size_t>(chunk_, std::max<size_t>((size_t)largest + 1, size_t(1) << 16));
    }
    layout_ = Feed::Sizes{ chunk_, comp_cap_, dict_cap_ };
    // the first file's feed now: what is no regular file says what it is through it (is_fastq)
    feeds_[0] = open_feed(run_, 0, plan_[0]);
    feeds_[0]->layout(layout_, kSlots);
    opened_ = feeds_[0]->ok();
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
    for (size_t f = 0; f < feeds_.size(); ++f) {
      close_feed(f);
    }
    if (getenv("GRP_TRACE_INGEST")) {
      std::cerr << "GRP_TRACE_INGEST source: " << n_pre_[0] << " chunks, next chunk not ready at " << n_pre_[1] << ", uploads started ahead " << n_pre_[2] << "; seconds waiting for the reader " << t_tr_[0]
                << ", in fastq_parse " << t_tr_[1] << ", in fastq_prefetch " << t_tr_[2] << ", copying tails " << t_tr_[3] << ", BGZF blocks inflated on the device " << counts_.bgzf_blocks
                << ", gzip segments inflated on the device " << counts_.gzip_segs;
      if (run_.files.size() > 1) {
        std::cerr << "; files " << run_.files.size() << ", begun " << n_files_[0] << ", parse calls " << n_files_[1];
      }
      std::cerr << std::endl;
    }
    if (pinned_) {
      run_.vt.fastq_unpin(run_.ctx); // before the buffer goes away: the engine cannot know when the host frees memory
    }
  }
  bool ok() const override { return run_.files.size() > 1 || opened_; }
  bool is_fastq() override // (asked before the first chunk is read; several files: check_inputs has looked at them all)
  {
    return run_.files.size() > 1 || (format_[0] < 0 ? feeds_[0] && feeds_[0]->peek() == '@' : format_[0] != 0);
  }
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
      const size_t file = sl->file;
      const bool eof = sl->eof; // the FILE ends with this chunk
      if (sl->first) {
        // a file begins: nothing of the file before is carried into it — its last chunk was parsed as a final one, and
        // what that left over was its own truncation
        carry_.clear();
        bam_header_done_ = false;
        bam_skipped_ = bam_reversed_ = 0;
        ++n_files_[0];
      }
      if ((long)file == skip_file_) { // behind a line that is no FASTQ header the file has ended for good: what the reader had read of it already
        if (eof) {
          close_feed(file);
        }
        if (sl->last) {
          done_ = true;
        }
        continue;
      }
      const bool inflated = inflate_slot(held_);
      if (eof) {
        close_feed(file); // (its last slot has been inflated: nothing reads through it any more)
      }
      if (!inflated) { // (the failure is noted: the run ends with an error behind this pass)
        done_ = true;
        break;
      }
      const std::string& path = run_.files[file];
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
      uint64_t text_off = sl->file_off - carry_.size(); // offset of text[0] in the file's stream
      if (fill == 0) { // (a file without a byte, or one whose last chunk is empty)
        if (eof && format_[file] == 2) {
          run_.note_bam_aligned(file, bam_skipped_, bam_reversed_);
        }
        if (sl->last) {
          done_ = true;
        }
        continue;
      }
      int format = format_[file];
      if (format < 0) { // no regular file: FASTQ, if anything
        format = text[0] == '@' ? 1 : 0;
      }
      if (format == 0 && run_.files.size() > 1) {
        note_input_failure("reading " + path + " failed: it is neither FASTQ nor BAM");
        done_ = true;
        break;
      }
      uint64_t n_rec = 0, used = 0;
      int stopped = 0;
      const bool bam = format == 2;
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
          note_bam_failure(path, text_off, hrc == 0 ? "the stream ends inside the BAM header (truncated)" : "not a BAM header");
          done_ = true;
          break;
        }
        bam_header_done_ = true;
        text += hb;
        fill -= hb;
        text_off += hb;
        if (fill == 0 && eof) { // a header and no record
          carry_.clear();
          if (sl->last) {
            done_ = true;
          }
          continue;
        }
      }
      const double tp0 = now_s();
      uint64_t bad_off = 0, n_skipped = 0;
      ++n_files_[1];
      const int prc = bam && run_.bam_accept ? run_.ext.bam_parse_ex(run_.ctx, text, fill, eof ? 1 : 0, run_.bam_accept, &fq_, &n_rec, &used, &bad_off, &n_skipped)
                      : bam                  ? run_.ext.bam_parse(run_.ctx, text, fill, eof ? 1 : 0, &fq_, &n_rec, &used, &bad_off)
                                             : run_.vt.fastq_parse(run_.ctx, text, fill, eof ? 1 : 0, &fq_, &n_rec, &used, &stopped);
      t_tr_[1] += now_s() - tp0;
      if (prc == GRP_ERR_INVALID && bam) { // a refused record: the input's failure, not the engine's
        note_bam_failure(path, text_off + bad_off, run_.vt.last_error ? run_.vt.last_error(run_.ctx) : nullptr);
        done_ = true;
        break;
      }
      if (prc != GRP_OK) {
        std::cerr << "goldrush-path: FASTQ ingest: " << (run_.vt.last_error ? run_.vt.last_error(run_.ctx) : "failed") << std::endl;
        failed_ = true;
        done_ = true;
        break;
      }
      if (n_rec == 0 && used == 0 && !eof && !stopped) {
        // not one complete record yet: everything is carried into the next chunk
        release();
        carry_.assign(text, text + fill);
        continue;
      }
      // (an aligned BAM chunk may consume bytes and hand out no record: secondary / supplementary records alone)
      bam_skipped_ += n_skipped;
      carry_.assign(text + used, text + fill);
      if (stopped && !eof) {
        // the file has ended here, like a reader at the end of its input; the reader thread leaves it at its next chunk
        skip_file_ = (long)file;
        abandon_.store((long)file);
      }
      if ((eof || stopped) && file + 1 == run_.files.size()) {
        done_ = true;
      }
      if (n_rec) {
        meta_.resize(n_rec);
        run_.vt.fastq_records(fq_, meta_.data());
        for (size_t i = 0; bam && i < n_rec; ++i) {
          bam_reversed_ += (meta_[i].flags & GRP_FQ_REVERSED) ? 1 : 0;
        }
      }
      if (bam && eof) { // the file has been read to its end
        run_.note_bam_aligned(file, bam_skipped_, bam_reversed_);
      }
      if (n_rec == 0) {
        release();
        continue;
      }
      b.text = text;
      b.file = file;
      b.base_off = text_off;
      b.rec.resize(n_rec);
      for (size_t i = 0; i < n_rec; ++i) {
        const grp_fastq_record& m = meta_[i];
        b.rec[i] = Rec{ (size_t)m.id_off, m.id_len, (size_t)m.seq_off, m.seq_len, (size_t)m.qual_off, m.qual_len, bam && (m.flags & GRP_FQ_REVERSED) != 0 };
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
  // (grpath_ingest.h: grp_fastq_prefetch).  The bodies may be another file's, of another format: the engine is handed bytes.
  // Not handed over ahead: the first chunk of a BAM file, nor anything behind it — its parse begins behind the header, not at
  // the body, so the engine would take it for another text and drop every pending body (they are parsed in the order issued).
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
        if (slot_[j].last && slot_[j].n == 0) {
          return;
        }
        n = slot_[j].n; // (a READY slot is the consumer's until it releases it)
      }
      if (slot_[j].uploaded || n == 0 || (long)slot_[j].file == skip_file_) {
        continue;
      }
      if (slot_[j].first && format_[slot_[j].file] == 2) {
        return;
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
    size_t file = 0;       // which of the run's files they are from (and so their format, and the feed that inflates them)
    uint64_t file_off = 0; // offset of the first of them in that file's stream
    bool first = false;    // the file begins with this chunk
    bool eof = false;      // the file ends with this chunk ...
    bool last = false;     // ... and it is the last file: the data ends with it
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
      sl.bad = !feeds_[sl.file]->inflate(j, slot_buf(j), chunk_);
    }
    return !sl.bad;
  }
  // consumer (or the destructor, behind the reader's end): the file's feed is done with; its counts stay
  void close_feed(size_t f)
  {
    if (feeds_[f]) {
      const Feed::Counts n = feeds_[f]->counts();
      counts_.bgzf_blocks += n.bgzf_blocks;
      counts_.gzip_segs += n.gzip_segs;
      feeds_[f].reset();
    }
  }
  // Slot after slot, file after file.  feeds_[f] is written here before the first slot of file f is published (under the
  // mutex) and reset by the consumer behind its last: the two threads never hold it at the same time.
  void read_loop()
  {
    size_t file = 0;
    uint64_t off = 0;
    bool first = true;
    for (int i = 0;; i = (i + 1) % kSlots) {
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return stop_ || slot_[i].state == Slot::FREE; });
        if (stop_) {
          return;
        }
      }
      if (!feeds_[file]) { // (the first file's is the constructor's)
        feeds_[file] = open_feed(run_, file, plan_[file]);
        feeds_[file]->layout(layout_, kSlots);
      }
      bool eof = false;
      slot_[i].inflated = slot_[i].bad = false; // (a FREE slot is the reader's)
      size_t got = 0;
      if (abandon_.load() == (long)file) {
        eof = true; // the consumer has met the file's end in front of the end of its bytes
      } else {
        got = feeds_[file]->fill(i, slot_buf(i), chunk_, eof);
      }
      const bool last = eof && file + 1 == run_.files.size();
      {
        std::lock_guard<std::mutex> g(mu_);
        slot_[i].n = got;
        slot_[i].file = file;
        slot_[i].file_off = off;
        slot_[i].first = first;
        slot_[i].eof = eof;
        slot_[i].last = last;
        slot_[i].state = Slot::READY;
      }
      cv_.notify_all();
      off += got;
      first = false;
      if (last) {
        return;
      }
      if (eof) {
        ++file;
        off = 0;
        first = true;
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
  const std::vector<int> format_;   // probe_format of every file
  std::vector<FilePlan> plan_;      // how every file is read (decided when the pass began)
  std::vector<std::unique_ptr<Feed>> feeds_; // the feeds of the files between the reader's first fill and the consumer's last inflate
  Feed::Sizes layout_{ 0, 0, 0 };   // the slots, as every feed is told
  Feed::Counts counts_;             // of the feeds that are done with
  bool opened_ = false;             // the first file could be opened
  std::vector<char> buf_;  // kSlots x [front | chunk], then what the feeds asked for beside them
  uint64_t n_pre_[3] = { 0, 0, 0 }; // developer trace: chunks returned, next slot not ready, prefetches the engine took
  double t_tr_[4] = { 0, 0, 0, 0 };  // developer trace: seconds waiting for the reader / in the parse call / in the prefetch calls / copying tails
  uint64_t n_files_[2] = { 0, 0 };  // developer trace: files begun, parse calls
  std::vector<char> carry_; // unconsumed tail of the chunk before (of the same file)
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
  long skip_file_ = -1;            // consumer's: the file that ended at a line that is no FASTQ header
  std::atomic<long> abandon_{ -1 }; // ... said to the reader thread
  bool bam_header_done_ = false;   // BAM: the header of the file being parsed has been skipped
  uint64_t bam_skipped_ = 0, bam_reversed_ = 0; // ... and what the parses of that file have met of an aligned file's records
  void* fq_ = nullptr;
  std::vector<grp_fastq_record> meta_;
};

} // namespace

std::unique_ptr<RecordSource>
open_source(PathRun& run)
{
  if (run.files.empty()) {
    run.files.push_back(run.opt.input);
  }
  run.gzidx.resize(run.files.size());
  run.bgzf_map.resize(run.files.size());
  bool gpu = run.vt.fastq_parse && run.vt.fastq_records && run.vt.fastq_pack && run.vt.fastq_free && !getenv("GRP_HOST_INGEST");
  std::vector<int> format(run.files.size(), 0);
  for (size_t f = 0; gpu && f < run.files.size(); ++f) {
    format[f] = probe_format(run.files[f]);
    // (a BAM file and an engine without bam_parse — GRP_BAM_ALIGNED=on: without bam_parse_ex: the host reader, for all the files)
    gpu = !(format[f] == 2 && !(run.bam_accept ? run.ext.bam_parse_ex != nullptr : run.ext.bam_parse != nullptr));
  }
  if (gpu) {
    return std::unique_ptr<RecordSource>(new GpuSource(run, format));
  }
  return std::unique_ptr<RecordSource>(new HostSource(run));
}

std::string
check_inputs(const PathRun& run)
{
  for (const std::string& path : run.files) {
    const FileProbe p = probe_file(path);
    if (!p.opened) {
      return path + ": cannot be opened: " + strerror(p.err);
    }
    if (p.regular && p.size != 0 && probe_format(path) <= 0) {
      return path + ": neither FASTQ nor BAM";
    }
  }
  return std::string();
}

} // namespace gr
