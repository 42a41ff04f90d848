// Streaming FASTQ reader with the record semantics the reference gets from
// btllib::SeqReader (LONG_MODE, default flags): id = header up to the first
// whitespace, sequence case-folded to upper case, 4-line records, records in
// file order.  Plain or gzip-compressed text (zlib; btllib::SeqReader pipes compressed
// input through an external decompressor).
// An unaligned BAM stream (gr_bam.hpp) is handed out as the records of its FASTQ twin.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace gr {

// the input file: a plain regular file (pread, large requests by several threads) or anything
// zlib reads — gzip data, pipes (GRP_ZLIB_READER=1 sends plain files through zlib too)
// An input that could not be read to its end (EIO, a file that shrank under the run, a damaged gzip stream) must not
// pass for a shorter input: the readers below note it here (first message wins) and the program ends with an
// error behind the pass that met it instead of classifying a prefix of the reads silently.
void note_input_failure(const std::string& what);
bool input_failed(std::string* what = nullptr);
void clear_input_failure();
// ... a BAM input (gr_bam.hpp) whose record at `off` of the decompressed stream is refused
void note_bam_failure(const std::string& path, uint64_t off, const char* why);
// what the first four bytes of the data say: 1 FASTQ ('@'), 2 BAM ("BAM\1"), 0 neither
int input_format(const unsigned char* head, size_t n);
// `want` bytes at `off`; fewer: the file ends there (*err 0) or the read failed (*err: errno; no descriptor: EBADF)
size_t pread_full(int fd, void* dst, size_t want, uint64_t off, int* err);
// One look at an input file: can it be opened (else err: the errno), is it a regular file, its size and what it begins
// with.  Only a regular file is read from — the bytes of a pipe are the input.
struct FileProbe
{
  bool opened = false, regular = false;
  int err = 0;
  uint64_t size = 0;
  enum Magic { NONE, GZIP, BAM, OTHER } magic = NONE; // fewer than two bytes / 1f 8b / "BAM\1" (not compressed) / anything else
};
FileProbe probe_file(const std::string& path);

class InputFile
{
public:
  explicit InputFile(const std::string& path);
  // the rest of `path` from where the descriptor stands, through zlib (the descriptor becomes the object's): what is left
  // of a file whose BGZF members end in front of a plain gzip member
  InputFile(const std::string& path, int gz_fd);
  ~InputFile();
  InputFile(const InputFile&) = delete;
  InputFile& operator=(const InputFile&) = delete;
  bool ok() const { return opened_; } // the file could be opened (it stays true behind the end of the data)
  size_t read(char* dst, size_t n); // 0 at the end of the data (or on a read error)
  int peek();                      // next byte without consuming it, -1 at the end
  uint64_t plain_size() const { return size_; } // bytes of a plain regular file, 0: unknown (gzip data, a pipe)

private:
  void* f_ = nullptr; // gzFile; closed (nullptr) once the data has ended, so that a truncated stream is noticed
  bool opened_ = false;
  int fd_ = -1;       // plain regular file
  uint64_t off_ = 0;  // ... and the read position in it
  uint64_t size_ = 0;
  std::string path_;
};

struct RecordRef
{
  size_t id_off, id_len;
  size_t seq_off, seq_len;
  size_t qual_off, qual_len;
};

// a run of consecutive records; all text lives in one buffer
struct RecordBatch
{
  std::vector<char> text;
  std::vector<RecordRef> rec;
  size_t bases = 0;
  void clear()
  {
    text.clear();
    rec.clear();
    bases = 0;
  }
  const char* id(size_t i) const { return text.data() + rec[i].id_off; }
  const char* seq(size_t i) const { return text.data() + rec[i].seq_off; }
  const char* qual(size_t i) const { return text.data() + rec[i].qual_off; }
  std::string id_str(size_t i) const { return std::string(id(i), rec[i].id_len); }
};

class FastqStream
{
public:
  // bam_accept (gr_bam.hpp: the walk's `accept`): the flags of 0x910 that a BAM input is read with instead of refused —
  // 0x910 hands out the records of the aligned twin (GRP_BAM_ALIGNED=on), 0 reads unaligned BAM only
  explicit FastqStream(const std::string& path, uint32_t bam_accept = 0);
  ~FastqStream();
  // BAM: the secondary / supplementary records passed over and the reverse-strand records handed out so far
  uint64_t bam_skipped() const { return bam_skipped_; }
  uint64_t bam_reversed() const { return bam_reversed_; }
  bool ok() const { return in_.ok(); }
  // SeqReader::get_format() == FASTQ  <=>  first byte of the file is '@'; unaligned BAM (the data begins with "BAM\1")
  // is read as its FASTQ twin (gr_bam.hpp): a format this program reads
  bool is_fastq();
  // appends up to max_records / ~max_bases to `out` (cleared first); false at EOF
  bool next_batch(RecordBatch& out, size_t max_records, size_t max_bases);

private:
  bool fill();
  bool get_line(const char*& p, size_t& n); // without the trailing newline / CR / blanks
  bool next_batch_bam(RecordBatch& out, size_t max_records, size_t max_bases);
  std::string path_;
  int format_ = -1;          // input_format of the data (-1: not looked at yet)
  bool bam_header_done_ = false;
  uint32_t bam_accept_ = 0;
  uint64_t bam_skipped_ = 0, bam_reversed_ = 0;
  uint64_t stream_off_ = 0;  // BAM: offset of buf_[pos_] in the decompressed stream
  InputFile in_;
  std::vector<char> buf_;
  size_t pos_ = 0, end_ = 0;
  bool eof_ = false;
  bool stopped_ = false; // a line that is not a FASTQ header was met: end of input for good (as the GPU ingest)
  std::vector<char> carry_;
};

} // namespace gr
