// goldrush-path as a function: main() of goldrush_path/goldrush_path.cpp:1096-1275
// with the miBF work going through the engine ABI (grpath.h) instead of
// MIBloomFilter / MIBFConstructSupport / multiLensfrHashIterator.
//
// Same flags, same stderr messages, same output files (<prefix>_<n>.fq in
// --silver_path mode, <prefix>.fa otherwise), same exit codes.
// Here: options, ranks, the engine, the banner and the passes in order (gr_passes.hpp, over gr_resident.hpp and gr_writer.hpp);
// and, not the reference's, --golden_path: that flow twice in one process, the golden path behind the silver paths (gr_golden.hpp).
#include "../../../include/grpath_host.h"
#include "gr_fastq.hpp"
#include "gr_golden.hpp"
#include "gr_gzwalk.hpp"
#include "gr_opts.hpp"
#include "gr_params.hpp"
#include "gr_passes.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <iomanip>
#include <sys/stat.h>
#include <unistd.h>
#if defined(_OPENMP)
#include <omp.h>
#endif

namespace gr {
namespace {

uint32_t
env_u32(const char* a, const char* b, uint32_t dflt)
{
  const char* e = getenv(a);
  if (!e || !*e) {
    e = getenv(b);
  }
  return (e && *e) ? (uint32_t)strtoul(e, nullptr, 10) : dflt;
}

struct Quiet // ranks > 0: nothing on stdout / stderr
{
  std::streambuf *cerr_buf = nullptr, *cout_buf = nullptr;
  std::ofstream null;
  ~Quiet()
  {
    if (cerr_buf) {
      std::cerr.rdbuf(cerr_buf);
      std::cout.rdbuf(cout_buf);
    }
  }
};

struct ShmGuard
{
  void* h = nullptr;
  ~ShmGuard() { gr_shm_allgather_close(h); }
};

struct RunGuard // the engine, and what a resident run holds of it and of the files
{
  PathRun& run;
  Resident& res;
  GoldenCarry *collect, *from; // --golden_path: the stage fills one, or is built from one (gr_golden.hpp)
  ~RunGuard()
  {
    res.drop(run);
    res.close_files();
    for (GoldenCarry* g : { collect, from }) {
      if (g && !(g == collect && g->on && g->done)) {
        g->free_parts(run);
      }
    }
    if (run.ctx && collect && collect->on && collect->done) {
      collect->ctx = run.ctx; // the first stage ended well: its engine goes to the second, with the parts
    } else if (run.ctx) {
      run.vt.destroy(run.ctx);
    }
    run.ctx = nullptr;
  }
};

// The engine's tables.  Of the optional one (grpath_host.h) the prefix struct_size covers, cut to whole members: a member
// it ends in front of, or a table that is NULL, leaves the host on the path it took without it.
void
take_engine(PathRun& run, const grp_engine_vt* vt, const grp_engine_ext* ext)
{
  run.vt = *vt;
  constexpr size_t first = offsetof(grp_engine_ext, bgzf_inflate), each = sizeof(ext->bgzf_inflate);
  static_assert((sizeof(grp_engine_ext) - first) % each == 0, "every member behind struct_size is one function pointer");
  if (ext && ext->struct_size >= first) {
    const size_t whole = (std::min<size_t>(ext->struct_size, sizeof(grp_engine_ext)) - first) / each;
    memcpy(reinterpret_cast<char*>(&run.ext) + first, reinterpret_cast<const char*>(ext) + first, whole * each);
  }
}

// Several GPUs of one node: one process per GPU (GRP_WORLD / GRP_RANK, or the launcher's
// WORLD_SIZE / RANK; LOCAL_RANK picks the device).  Every rank runs the whole program on
// its own replica of the miBF — the same input, the same passes, every insert — and the
// ranks share the QUERY work of each classification window (gr_classifier: the window's
// reads are split / striped over the ranks, the 32-byte decisions all-gathered through
// /dev/shm).  Rank 0 writes the files and the log; the others are silent.
// Then the options, the input files and GRP_BAM_ALIGNED.  -1, or the exit code.
int
read_options(PathRun& run, int argc, char** argv, Quiet& quiet)
{
  run.world = std::max<uint32_t>(1, env_u32("GRP_WORLD", "WORLD_SIZE", 1));
  run.rank = env_u32("GRP_RANK", "RANK", 0);
  if (run.rank >= run.world) {
    std::cerr << "goldrush-path: rank " << run.rank << " outside the world of " << run.world << std::endl;
    return 1;
  }
  if (run.rank != 0) {
    quiet.null.open("/dev/null");
    quiet.cerr_buf = std::cerr.rdbuf(quiet.null.rdbuf());
    quiet.cout_buf = std::cout.rdbuf(quiet.null.rdbuf());
  }
  clear_input_failure();
  const int ec = process_options(run.opt, argc, argv);
  if (ec >= 0) {
    return ec;
  }
  if (run.opt.golden_path) {
    // --golden_path: refused here, in front of the first pass, where it cannot run
    const char* why = !run.opt.silver_path            ? "it needs --silver_path: the golden path is built from the silver paths of the same command"
                      : run.opt.golden_prefix.empty() ? "the prefix of the golden path's file is empty"
                      : run.world > 1                 ? "several ranks are out of scope of the option: it runs on one rank (GRP_WORLD=1)"
                                                      : nullptr;
    if (why) {
      std::cerr << "goldrush-path: --golden_path: " << why << std::endl;
      return 1;
    }
  }
  // every -i is an input, a ".fofn" list stands for the files it names (gr_opts.hpp); no -i at all: the reference's empty name
  std::string bad_list;
  if (!expand_inputs(run.opt.inputs, run.files, bad_list)) {
    std::cerr << "goldrush-path: " << bad_list << std::endl;
    return 1;
  }
  if (run.files.empty()) {
    run.files.push_back(run.opt.input);
  }
  run.bam_aligned.resize(run.files.size()); // (gzidx and bgzf_map: open_source)
  // GRP_BAM_ALIGNED=on: a BAM input is read as its aligned twin — what `samtools fastq -n` writes for it with its default
  // filters (gr_bam.hpp).  Read here, once, in front of the first pass; opt-in, because records are dropped
  const char* e = getenv("GRP_BAM_ALIGNED");
  if (e && !strcmp(e, "on")) {
    run.bam_accept = BAM_REFUSED_FLAGS;
  } else if (e && strcmp(e, "off")) {
    std::cerr << "goldrush-path: GRP_BAM_ALIGNED=" << e << ": the switch takes on or off" << std::endl;
    return 1;
  }
  // GRP_GZIP_WALK=on: the restart points of the plain gzip inputs are found on the device in front of the first pass
  // (gr_gzwalk.hpp).  Opt-in: it pays from some tens of files upward and loses on a single one
  const int walk = gzip_walk_switch();
  if (walk < 0) {
    std::cerr << "goldrush-path: GRP_GZIP_WALK=" << getenv("GRP_GZIP_WALK") << ": the switch takes on or off" << std::endl;
    return 1;
  }
  run.gzip_walk = walk == 1;
  // GRP_GZIP_WALK_MEMBERS=on, beside it: the members of one file side by side too (cat *.fastq.gz > reads.fq.gz).  Off by
  // default, and without effect where the walk is off
  if (gzip_walk_members_switch() < 0) {
    std::cerr << "goldrush-path: GRP_GZIP_WALK_MEMBERS=" << getenv("GRP_GZIP_WALK_MEMBERS") << ": the switch takes on or off" << std::endl;
    return 1;
  }
  run.gzip_walk_members = gzip_walk_members();
  return -1;
}

bool
create_engine(PathRun& run, uint64_t filter_size)
{
  std::vector<const char*> sp;
  for (const auto& s : run.seeds) {
    sp.push_back(s.c_str());
  }
  grp_params gp{};
  gp.struct_size = sizeof(gp);
  gp.k = (uint32_t)run.opt.kmer_size;
  gp.h = (uint32_t)run.opt.hash_num;
  gp.tile = (uint32_t)run.opt.tile_length;
  gp.m = filter_size;
  gp.seeds = sp.data();
  gp.device = run.device; // (run_stage)
  if (run.vt.create(&gp, &run.ctx) != GRP_OK) {
    std::cerr << "goldrush-path: cannot set up the MI355X engine: " << (run.vt.last_error ? run.vt.last_error(nullptr) : "") << std::endl;
    return false;
  }
  return true;
}

// behind the Phred pass: the reference's banner, the -f list, the output file and the lines of the allocation
void
say_banner(PathRun& run, uint64_t filter_size)
{
  const Opts& opt = run.opt;
  std::cerr << "Calculating " << (opt.silver_path ? std::to_string(opt.max_paths) + " silver path(s)" : std::string("the golden path")) << "\n"
            << "Using:\n"
            << "\ttile length: " << opt.tile_length << "\n"
            << "\tblock size: " << opt.block_size << "\n"
            << "\tseed patterns: " << opt.hash_num << "\n"
            << "\tthreshold: " << opt.threshold << "\n"
            << "\tbase seed pattern: " << run.seeds[0] << "\n"
            << "\tminimum unassigned tiles: " << opt.unassigned_min << "\n"
            << "\tmaximum assigned tiles: " << opt.assigned_max << "\n"
            << "\texpected hash space: " << opt.hash_universe << "\n"
            << "\tminimum average phred quality score: " << opt.phred_min << "\n"
            << "\tmaximum average phred delta between first and second half of read: " << opt.phred_delta << "\n"
            << "\toccupancy: " << opt.occupancy << "\n"
            << "\tjobs: " << opt.jobs << std::endl;
  if (!opt.filter_file.empty()) {
    std::cerr << "Using only reads not found in: " << opt.filter_file << std::endl;
    std::ifstream in(opt.filter_file);
    std::string name;
    while (in >> name) {
      run.filter_out_reads.insert(name);
    }
  }
  run.out.open(run.rank != 0 ? std::string("/dev/null") : opt.silver_path ? opt.prefix_file + "_1.fq" : opt.prefix_file + ".fa");
  if (run.rank == 0) {
    run.out_files.push_back(opt.silver_path ? opt.prefix_file + "_1.fq" : opt.prefix_file + ".fa");
  }
  const double s_time = now_s();
  std::cerr << "allocating bit vector" << std::endl;
  std::cerr << "m_filterSize: " << filter_size << std::endl;
  std::cerr << "finished allocating bit vector" << std::endl;
  std::cerr << "in " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  for (const std::string& path : run.files) {
    std::cerr << "opening: " << path << std::endl;
  }
}

gr_classifier_params
classifier_params(const PathRun& run)
{
  const Opts& opt = run.opt;
  gr_classifier_params cp{};
  cp.struct_size = sizeof(cp);
  cp.tile_length = (uint32_t)opt.tile_length;
  cp.block_size = (uint32_t)opt.block_size;
  cp.threshold = (uint32_t)opt.threshold;
  cp.unassigned_min = (uint32_t)opt.unassigned_min;
  cp.assigned_max = (uint32_t)opt.assigned_max;
  cp.kmer_size = (uint32_t)opt.kmer_size;
  cp.hash_num = (uint32_t)opt.hash_num;
  cp.target_bases = (uint64_t)(opt.ratio * opt.genome_size); // :1223
  cp.max_paths = opt.max_paths;
  cp.silver_path = opt.silver_path;
  cp.verbose = opt.verbose;
  cp.world = run.world;
  cp.rank = run.rank;
  cp.debug = opt.debug;
  cp.seed0_span = (uint32_t)run.seeds[0].size();
  return cp;
}

// One run of the program behind its options: `run` holds the engine's tables, the ranks, the options and the files to
// read; everything else — the engine, the reads kept on the device, the classifier, the sink — lives and dies in here.
// The exit code: 0 also where the reference does exit(0) inside silver_path_check.
// --golden_path: `collect`, the first stage, remembers what it writes; `from`, the second stage on the device route, is built
// from what the first remembered — its engine rewound, its Phred median and its fill from the kept records.
int
run_stage(PathRun& run, void* shm_h, GoldenCarry* collect = nullptr, GoldenCarry* from = nullptr)
{
  Resident res;
  Opts& opt = run.opt;
  int ec = -1;
#if defined(_OPENMP)
  // the reference uses -j for its OpenMP regions; here it only drives the host
  // side (parsing, Phred, packing, decisions) and is capped at the machine size
  omp_set_num_threads((int)std::max<size_t>(1, std::min<size_t>(opt.jobs, (size_t)effective_cpus())));
#endif
  run.seeds = make_seed_pattern(opt.seed_preset, (unsigned)opt.kmer_size, (unsigned)opt.weight, (unsigned)opt.hash_num, true);
  const bool use_ntcard = opt.hash_universe == 0 && opt.ntcard;
  if (use_ntcard && !(run.vt.ntcard_begin && run.vt.ntcard_add && run.vt.ntcard_finish && run.vt.set_filter_size)) {
    std::cerr << "goldrush-path: --ntcard needs an engine with the ntcard entry points" << std::endl;
    return 1;
  }
  if (opt.hash_universe == 0 && !use_ntcard) {
    opt.hash_universe = hash_universe(opt.weight, opt.genome_size, opt.hash_num);
  }
  // the engine is set up before the first pass over the input (the Phred median
  // pass already uses the GPU ingest); the reference's messages keep their order.
  // With --ntcard the filter size is only known after the ntcard pass.
  uint64_t filter_size = use_ntcard ? 0 : calc_optimal_size(opt.hash_universe, 1, opt.occupancy);
  run.device = run.world > 1 ? (int32_t)env_u32("GRP_LOCAL_RANK", "LOCAL_RANK", run.rank) : -1;
  if (run.world > 1 && shm_h && gr_ranks_share_device(shm_h, run.world, run.device) == 1) {
    // ranks on one device (a test box): their windows' launches must all fit it at once — the in-launch inserts of
    // the ranks' windows wait grid-wide.  In front of the engine: it reads its switches when its context is created
    // (an explicit setting stands; the second stage of --golden_path takes over a context created behind this line)
    setenv("GRP_STREAM_WGS_PER_CU", "1", 0);
  }
  if (from) {
    // the first stage's engine, returned to its fill state: its tables go, this stage's take their place
    run.ctx = from->ctx;
    from->ctx = nullptr;
  } else if (!create_engine(run, filter_size)) {
    return 1;
  }
  RunGuard guard{ run, res, collect, from };
  if (from && (filter_size != from->filter_size || run.ext.rewind(run.ctx) != GRP_OK)) {
    return run.fail_engine("returning the engine to its fill state");
  }
  if (collect) {
    collect->filter_size = filter_size;
  }
  if (run.files.size() > 1) {
    // several inputs: each is looked at before the first pass — a run does not get an hour into the fill before it finds
    // that its last file is missing
    const std::string bad = check_inputs(run);
    if (!bad.empty()) {
      std::cerr << "goldrush-path: " << bad << std::endl;
      std::cerr << "Gold Path requires fastq format" << std::endl;
      return 1;
    }
  }
  if (use_ntcard) {
    uint64_t genome_size = 0;
    ec = after_pass(run, calc_ntcard_genome_size(run, genome_size));
    if (ec >= 0) {
      return ec;
    }
    opt.hash_universe = genome_size;
    filter_size = calc_optimal_size(opt.hash_universe, 1, opt.occupancy);
    if (run.vt.set_filter_size(run.ctx, filter_size) != GRP_OK) {
      return run.fail_engine("allocating the bit vector");
    }
  }
  if (run.vt.occupancy_hint && opt.occupancy > 0.0 && opt.occupancy < 1.0) {
    // the ID / count tables of phase 2 are sized by the occupancy the fill will reach: -o, by construction of the filter
    // size (:1183-1184) — the engine allocates them beside the fill instead of between the passes (a hint: ignored where wrong)
    (void)run.vt.occupancy_hint(run.ctx, opt.occupancy);
  }
  if (run.world > 1 && !getenv("GRP_REPLICATED_FILL")) {
    // A sharded fill needs a way to merge: RCCL inside the engine (one GPU per rank), else the
    // host-staged form (ranks sharing a device, engines without RCCL).  Every decision below is
    // taken by ALL ranks alike (flags all-gathered through /dev/shm).
    run.shm = shm_h;
    const int plan = gr_fill_merge_plan(&run.vt, run.ctx, shm_h, run.world, run.rank, run.device);
    run.merge_rccl = plan == GR_MERGE_RCCL;
    run.shard_fill = plan != GR_MERGE_NONE;
  }
  ec = after_pass(run, from ? golden_phred_threshold(run, *from) : calc_min_phred_threshold(run));
  if (ec >= 0) {
    return ec;
  }
  say_banner(run, filter_size);
  if (!from) {
    res.decide(run);
  }
  ec = after_pass(run, from ? golden_fill(run, res, *from) : fill_bit_vector(run, res));
  if (ec >= 0) {
    return ec;
  }
  if (res.on && res.any_compressed()) {
    (void)res.resolve_units(run); // (false: dropped, with its reason line)
  }
  uint64_t pop = 0;
  if (run.vt.finalize(run.ctx, &pop) != GRP_OK) {
    return run.fail_engine("building the rank structure");
  }
  // every rank classifies on its own replica: they must hold the same filter (a merge that failed on one rank
  // would otherwise only show as diverging decisions much later)
  if (run.world > 1 && run.shm && gr_ranks_same_u64(run.shm, run.world, pop) != 1) {
    std::cerr << "ERROR: the ranks' filters differ after the merge (rank " << run.rank << ": " << pop << " set bits)" << std::endl;
    return 1;
  }

  std::cerr << "assigning tiles" << std::endl;
  const double s_time = now_s();
  if (opt.debug && run.world > 1) {
    std::cerr << "goldrush-path: --debug runs on one rank" << std::endl;
    return 1;
  }
  Classifier cls(classifier_params(run), run.vt, run.ctx);
  SinkState sink;
  sink.run = &run;
  sink.golden = collect;
  cls.set_callbacks(commit_sink, rollover_sink, nullptr, &sink);
  if (run.world > 1) {
    cls.set_allgather(gr_shm_allgather, shm_h);
  }
  if (opt.debug) {
    cls.set_debug(debug_sink);
  }
  ec = res.on ? classify_resident(run, res, cls, sink) : classify_source(run, cls, sink);
  if (ec >= 0) {
    if (collect) {
      collect->done = ec == 0;
    }
    return ec;
  }
  if (input_error()) {
    return 1;
  }
  if (opt.silver_path && opt.max_paths > cls.curr_path()) {
    std::cerr << "WARNING: Expected " << std::to_string(opt.max_paths) << " silver paths, but only " << std::to_string(cls.curr_path()) << " generated.\n"
              << "Possible reasons include:\n"
              << "\t- Input reads sorted by chromosome/position\n"
              << "\t- Genome size set too large\n";
  }
  if (opt.verbose) {
    cls.log_path_stat();
  }
  std::cerr << "assigned" << std::endl;
  std::cerr << "in " << std::setprecision(4) << std::fixed << now_s() - s_time << "\n";
  if (collect) {
    collect->done = true;
  }
  return 0;
}

// --golden_path: the silver files stage A wrote that hold something, in the order `cat PREFIX_*.fq` puts them — their names
// compared byte by byte (_1, _10, _11, _2, ... once there are ten).  An empty file adds nothing to the concatenation and is
// left out; where every file is empty the first one stands for the empty concatenation.
std::vector<std::string>
silver_files(const PathRun& a)
{
  std::vector<std::string> all = a.out_files, files;
  std::sort(all.begin(), all.end());
  for (const std::string& f : all) {
    struct stat st;
    if (stat(f.c_str(), &st) == 0 && st.st_size > 0) {
      files.push_back(f);
    }
  }
  if (files.empty() && !all.empty()) {
    files.push_back(all.front());
  }
  return files;
}

// --golden_path, stage B: the run `goldrush-path <the options of stage A without --silver_path, -M, -r, -f, -i, -p> -m 0
// -p PREFIX -i F1 -i F2 ...` would be, in this process.  Nothing of stage A is left but the engine's function tables, the
// switches read from the environment, the names of its files and — on the device route — what `carry` holds: a new PathRun,
// its own reads, and std::cerr as a new process finds it (the reference leaves `fixed` and a precision of 4 on it behind
// its first timing line).  Its engine is A's, rewound, on the device route and one of its own where the files are read back.
int
golden_stage(const PathRun& a, const Opts& parsed, GoldenCarry& carry)
{
  PathRun b;
  b.vt = a.vt;
  b.ext = a.ext;
  b.bam_accept = a.bam_accept;
  b.opt = parsed;
  const Opts dflt;
  b.opt.golden_path = 0;
  b.opt.golden_prefix.clear();
  b.opt.silver_path = 0;
  b.opt.max_paths = dflt.max_paths;
  b.opt.ratio = dflt.ratio;
  b.opt.filter_file.clear();
  b.opt.min_length = 0;
  b.opt.prefix_file = parsed.golden_prefix;
  b.files = silver_files(a);
  b.opt.inputs = b.files;
  b.opt.input = b.files.empty() ? std::string() : b.files.back();
  if (b.files.empty()) {
    b.files.push_back(b.opt.input);
  }
  b.bam_aligned.resize(b.files.size());
  clear_input_failure();
  std::cerr.unsetf(std::ios::floatfield);
  std::cerr.precision(6);
  if (carry.on && carry.recs.empty()) {
    carry.give_up(a, "the first stage wrote no record");
  }
  if (!carry.on && carry.ctx) {
    a.vt.destroy(carry.ctx);
    carry.ctx = nullptr;
  }
  const bool device = carry.on && carry.ctx;
  uint64_t n_records = carry.n_written, n_parts = carry.parts.size(), bytes_read = 0;
  if (device) {
    golden_order(carry, a.out_files, b.files);
  } else {
    std::cerr << "--golden_path: the silver reads are read back from their files: " << carry.why << std::endl;
    for (const std::string& f : b.files) {
      struct stat st;
      bytes_read += stat(f.c_str(), &st) == 0 ? (uint64_t)st.st_size : 0;
    }
  }
  const int ec = run_stage(b, nullptr, nullptr, device ? &carry : nullptr);
  if (getenv("GRP_TRACE_INGEST")) {
    std::cerr << "GRP_TRACE_INGEST golden: route=" << (device ? "device" : "files") << " records=" << n_records << " parts=" << n_parts << " batches=" << carry.n_batches << " bytes_read=" << bytes_read << std::endl;
  }
  return ec;
}

} // namespace
} // namespace gr

extern "C" int
gr_path_main(int argc, char** argv, const grp_engine_vt* vt)
{
  return gr_path_main_ext(argc, argv, vt, nullptr);
}

extern "C" int
gr_path_main_ext(int argc, char** argv, const grp_engine_vt* vt, const grp_engine_ext* ext)
{
  using namespace gr;
  PathRun run;
  take_engine(run, vt, ext);
  Quiet quiet;
  int ec = read_options(run, argc, argv, quiet);
  if (ec >= 0) {
    return ec;
  }
  ShmGuard shm;
  if (run.world > 1) {
    const char* key = getenv("GRP_SHM_KEY");
    std::string k = key && *key ? key : std::string("path_") + (getenv("MASTER_PORT") ? getenv("MASTER_PORT") : "0") + "_" + std::to_string((unsigned long)getppid());
    shm.h = gr_shm_allgather_open(run.world, run.rank, k.c_str(), 120.0);
    if (!shm.h) {
      std::cerr << "goldrush-path: cannot set up the exchange between the " << run.world << " ranks (/dev/shm/grp_" << k << ")" << std::endl;
      return 1;
    }
  }
  if (!run.opt.golden_path) {
    return run_stage(run, shm.h);
  }
  // --golden_path: stage A is the command as written; behind it — where it ends at the end of its input or where the
  // reference does exit(0), not behind an error — stage B reads the silver files A has written and closed
  const Opts parsed = run.opt; // (a stage completes its own copy: the hash universe, the Phred threshold)
  GoldenCarry carry;
  carry.decide(run);
  ec = run_stage(run, shm.h, &carry);
  if (ec != 0) {
    return ec;
  }
  run.out.close();
  return golden_stage(run, parsed, carry);
}
