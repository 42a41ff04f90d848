// The reads kept on the device (gr_resident.hpp): which files may stay, their units, their descriptors.
#include "gr_resident.hpp"
#include "gr_fastq.hpp"

#include <cstring>
#include <fcntl.h>

namespace gr {

void
Resident::decide(const PathRun& run)
{
  const char* e = getenv("GRP_RESIDENT");
  const bool gpu_ingest = run.vt.fastq_parse && run.vt.fastq_records && run.vt.fastq_pack && run.vt.fastq_free && !getenv("GRP_HOST_INGEST");
  all = e && !strcmp(e, "all");
  kind.assign(run.files.size(), PLAIN);
  bam.assign(run.files.size(), 0);
  if ((e && !strcmp(e, "off")) || !gpu_ingest || run.opt.debug) {
    say_dropped(run, run.opt.debug ? "--debug" : getenv("GRP_HOST_INGEST") ? "GRP_HOST_INGEST" : "the engine has no ingest entry points");
    return;
  }
  on = true;
  for (size_t f = 0; f < run.files.size() && on; ++f) {
    const FileProbe p = probe_file(run.files[f]);
    // a plain regular file (no gzip magic; not BAM that is not compressed: its records are not text), whose records can be
    // read back with pread?  One of several files may hold no byte (no record is ever read back from it).
    if (p.regular && ((run.files.size() > 1 && p.size == 0) || p.magic == FileProbe::OTHER)) {
      continue;
    }
    // GRP_RESIDENT=all: or a regular file of gzip members (BGZF among them), whose records could be fetched through
    // inflatable units; whether its units are known is seen behind the fill pass (resolve_units).  Else why not.
    const char* why = !p.opened ? "it cannot be opened" : !p.regular ? "it is no regular file" : p.magic == FileProbe::BAM ? "it is an uncompressed BAM file" : p.magic != FileProbe::GZIP ? "it is neither plain FASTQ nor gzip data" : "";
    if (all && !*why) {
      kind[f] = UNKNOWN;
    } else {
      on = false;
      say_dropped(run, why, run.files[f]);
    }
  }
  const char* cap = getenv("GRP_RESIDENT_MAX_GB");
  max_bytes = (uint64_t)((cap ? atof(cap) : 100.0) * (double)(1ull << 30));
}

bool
Resident::resolve_units(PathRun& run)
{
  gz_text_off.assign(run.files.size(), std::vector<uint64_t>());
  for (size_t f = 0; f < run.files.size(); ++f) {
    if (kind[f] != UNKNOWN) {
      continue;
    }
    std::string why;
    if (run.bgzf_map[f]) {
      kind[f] = BGZF;
      if (!run.ext.records_fetch && !run.ext.bgzf_inflate) {
        why = "the engine cannot inflate BGZF members";
      }
    } else if (run.gzidx[f] && run.gzidx[f]->matches(run.files[f])) {
      kind[f] = GZIP;
      const GzIndex& ix = *run.gzidx[f];
      std::vector<uint64_t>& toff = gz_text_off[f];
      toff.assign(1, 0);
      for (const GzSegment& g : ix.segs) {
        toff.push_back(toff.back() + g.text_len);
      }
      if (!run.ext.records_fetch && !run.ext.gzip_inflate) {
        why = "the engine cannot inflate gzip segments";
      } else if (ix.max_text > kTextCap) {
        why = "a segment of its index holds more text (" + std::to_string(ix.max_text) + " bytes) than a fetch takes";
      }
    } else {
      why = "the fill pass left neither a table of its BGZF members (a member that is not BGZF hands the file to zlib) nor a complete gzip index (GRP_GZIP_INDEX=off, dropped at GRP_GZIP_INDEX_MAX_GB, bytes behind the last member)";
    }
    if (!why.empty()) {
      say_dropped(run, why, run.files[f]);
      drop(run);
      return false;
    }
  }
  return true;
}

int
Resident::fd_of(const PathRun& run, uint32_t file)
{
  fds.resize(run.files.size(), -1);
  if (fds[file] < 0) {
    if (n_open == kMaxOpen) {
      close_files();
    }
    fds[file] = open(run.files[file].c_str(), O_RDONLY | O_CLOEXEC);
    n_open += fds[file] >= 0 ? 1 : 0;
  }
  return fds[file];
}

} // namespace gr
