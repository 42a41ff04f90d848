// The bit-vector merge of a multi-GPU fill inside the engine (round 3): every rank fills the
// reads of its shard, the plain bit vectors are OR-merged before grp_finalize (SURVEY 8(e): the
// fill is order-free, its merge a bitwise OR).  RCCL has no OR reduction (rccl.h: sum / prod / max /
// min / avg), so the OR "all-reduce" is spelled out as reduce-scatter + all-gather:
// ncclAllToAll sends slice r of every rank's vector to rank r, rank r ORs the N slices
// (k_bv_or), ncclAllGather hands the merged slices round — 2 x (N-1)/N of one vector per rank
// over xGMI (13 GB at C2, N = 8), one collective each, on the context's stream.
// librccl.so is loaded on first use (dlopen): a single-GPU run never touches it.
// Included by grpath_hip.hip (same translation unit).
#include <dlfcn.h>

namespace {

struct RcclId
{
  char internal[128]; // NCCL_UNIQUE_ID_BYTES (rccl.h:40-43)
};

struct RcclApi
{
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId /* ncclUniqueId, by value */, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllToAll)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*CommGetAsyncError)(void*, int*) = nullptr; // optional: the communicator's asynchronous error state
  int (*GetVersion)(int*) = nullptr;               // optional
};

RcclApi g_rccl;
std::mutex g_rccl_mutex;

const char*
rccl_load()
{
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (g_rccl.lib) {
    return nullptr;
  }
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  }
  if (!lib) {
    return "librccl.so not found";
  }
  RcclApi a;
  a.lib = lib;
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  a.AllToAll = reinterpret_cast<decltype(a.AllToAll)>(dlsym(lib, "ncclAllToAll"));
  a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(lib, "ncclAllGather"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  a.CommGetAsyncError = reinterpret_cast<decltype(a.CommGetAsyncError)>(dlsym(lib, "ncclCommGetAsyncError"));
  a.GetVersion = reinterpret_cast<decltype(a.GetVersion)>(dlsym(lib, "ncclGetVersion"));
  if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllToAll || !a.AllGather) {
    dlclose(lib);
    return "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllToAll / ncclAllGather";
  }
  g_rccl = a;
  return nullptr;
}

constexpr int RCCL_UINT8 = 1; // ncclUint8 (rccl.h:459-460)

void
comm_release(grp_ctx* c)
{
  if (c->comm && g_rccl.CommDestroy) {
    (void)g_rccl.CommDestroy(c->comm);
  }
  c->comm = nullptr;
}

} // namespace

extern "C" {

int
grp_comm_unique_id(void* out, size_t cap)
{
  if (!out || cap < sizeof(RcclId)) {
    return GRP_ERR_INVALID;
  }
  if (const char* e = rccl_load()) {
    return set_err(nullptr, GRP_ERR_INVALID, "grp_comm_unique_id: %s", e);
  }
  const int rc = g_rccl.GetUniqueId(out);
  return rc == 0 ? GRP_OK : set_err(nullptr, GRP_ERR_HIP, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "failed");
}

int
grp_comm_init(grp_ctx* c, const void* unique_id, uint32_t world, uint32_t rank)
{
  if (!c || !unique_id || world < 1 || rank >= world) { // (world = 1: a communicator of one — the merge is then two copies; what a 1-GPU box can run of this path)
    return set_err(c, GRP_ERR_INVALID, "grp_comm_init: bad argument");
  }
  if (c->comm) {
    return set_err(c, GRP_ERR_STATE, "grp_comm_init: the context already has a communicator");
  }
  if (const char* e = rccl_load()) {
    return set_err(c, GRP_ERR_INVALID, "grp_comm_init: %s", e);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  RcclId id;
  memcpy(&id, unique_id, sizeof(id));
  void* comm = nullptr;
  const int rc = g_rccl.CommInitRank(&comm, (int)world, id, (int)rank);
  if (rc != 0) {
    return set_err(c, GRP_ERR_HIP, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "failed");
  }
  c->comm = comm;
  c->comm_world = world;
  c->comm_rank = rank;
  return GRP_OK;
}

// bv = OR over the ranks' bit vectors (before grp_finalize; every rank calls it)
int
grp_bv_merge_ranks(grp_ctx* c)
{
  if (!c || !c->comm) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_merge_ranks: no communicator (grp_comm_init)");
  }
  if (c->finalized || c->f.m == 0) {
    return set_err(c, GRP_ERR_STATE, "grp_bv_merge_ranks: only between the fill and grp_finalize");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t world = c->comm_world;
  const uint64_t slice_words = ((c->n_bv_words + world - 1) / world + 3) / 4 * 4; // 16-byte multiples
  const size_t slice_bytes = slice_words * 4, total = slice_bytes * world;
  DevBuf<uint8_t> mine, got;
  HIP_TRY(c, mine.reset(total));
  if (got.reset(total) != hipSuccess) {
    return set_err(c, GRP_ERR_NOMEM, "grp_bv_merge_ranks: no room for two copies of the bit vector");
  }
  // every exit waits for the stream (the buffers are freed); a collective, the OR kernel or the import that failed
  // asynchronously shows there or in the communicator's error state — never GRP_OK on a partly merged vector (ADVICE r03)
  auto done = [&](int rc) {
    const hipError_t se = hipStreamSynchronize(c->stream);
    int async = 0;
    if (g_rccl.CommGetAsyncError && g_rccl.CommGetAsyncError(c->comm, &async) != 0) {
      async = -1;
    }
    clear_all(mine, got);
    if (rc == GRP_OK && se != hipSuccess) {
      return set_err(c, GRP_ERR_HIP, "grp_bv_merge_ranks: the merge failed on the stream: %s", hipGetErrorString(se));
    }
    if (rc == GRP_OK && async != 0) {
      return set_err(c, GRP_ERR_HIP, "grp_bv_merge_ranks: the communicator reports an asynchronous error: %s", async > 0 && g_rccl.GetErrorString ? g_rccl.GetErrorString(async) : "unknown");
    }
    if (rc == GRP_OK) {
      ++c->n_comm_merges;
    }
    return rc;
  };
  if (hipMemsetAsync(mine, 0, total, c->stream) != hipSuccess || hipMemcpyAsync(mine, c->f.bv, c->n_bv_words * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
    return done(set_err(c, GRP_ERR_HIP, "grp_bv_merge_ranks: staging the bit vector failed"));
  }
  int rc = g_rccl.AllToAll(mine, got, slice_bytes, RCCL_UINT8, c->comm, c->stream); // got[p] = slice `rank` of rank p's vector
  if (rc != 0) {
    return done(set_err(c, GRP_ERR_HIP, "ncclAllToAll: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "failed"));
  }
  for (uint32_t p = 1; p < world; ++p) {
    k_bv_or<<<dim3(4096), dim3(THREADS), 0, c->stream>>>(reinterpret_cast<uint4*>(got.p), reinterpret_cast<const uint4*>(got.p + (size_t)p * slice_bytes), slice_words / 4, nullptr, nullptr, 0);
  }
  if (hipGetLastError() != hipSuccess) {
    return done(set_err(c, GRP_ERR_HIP, "grp_bv_merge_ranks: OR kernel failed"));
  }
  rc = g_rccl.AllGather(got, mine, slice_bytes, RCCL_UINT8, c->comm, c->stream);
  if (rc != 0) {
    return done(set_err(c, GRP_ERR_HIP, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "failed"));
  }
  if (hipMemcpyAsync(c->f.bv, mine, c->n_bv_words * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
    return done(set_err(c, GRP_ERR_HIP, "grp_bv_merge_ranks: importing the merged vector failed"));
  }
  return done(GRP_OK);
}

int
grp_comm_info(const grp_ctx* c, uint32_t* world, uint32_t* rank, int* rccl_version, uint32_t* merges)
{
  if (!c) {
    return GRP_ERR_INVALID;
  }
  if (world) {
    *world = c->comm ? c->comm_world : 0u;
  }
  if (rank) {
    *rank = c->comm ? c->comm_rank : 0u;
  }
  if (rccl_version) {
    int v = 0;
    if (c->comm && g_rccl.GetVersion && g_rccl.GetVersion(&v) != 0) {
      v = 0;
    }
    *rccl_version = v;
  }
  if (merges) {
    *merges = c->n_comm_merges;
  }
  return GRP_OK;
}

// The same merge for ranks that cannot form an RCCL communicator (several ranks on ONE device:
// the plumbing tests of a 1-GPU box): words [first, first + n) of the plain bit vector to / from
// host memory; the caller exchanges them (shared memory) and ORs the other ranks' words in.
int
grp_bv_export_words(grp_ctx* c, uint64_t first, uint64_t n, uint32_t* words)
{
  if (!c || !words || c->finalized || first + n > c->n_bv_words) {
    return set_err(c, GRP_ERR_INVALID, "grp_bv_export_words: bad range, or after grp_finalize");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(words, c->f.bv + first, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return GRP_OK;
}

int
grp_bv_or_words(grp_ctx* c, uint64_t first, uint64_t n, const uint32_t* words)
{
  if (!c || !words || c->finalized || first + n > c->n_bv_words || (first & 3u)) {
    return set_err(c, GRP_ERR_INVALID, "grp_bv_or_words: bad range (first must be a multiple of 4 words), or after grp_finalize");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf<uint32_t> tmp;
  const uint64_t n_pad = (n + 3) / 4 * 4;
  HIP_TRY(c, tmp.reset(n_pad));
  hipError_t e = hipMemsetAsync(tmp, 0, n_pad * 4, c->stream);
  if (e == hipSuccess) {
    e = hipMemcpyAsync(tmp, words, n * 4, hipMemcpyHostToDevice, c->stream);
  }
  if (e == hipSuccess) {
    // (the vector is padded with 3 zero words: a padded tail never reaches beyond it)
    k_bv_or<<<dim3(1024), dim3(THREADS), 0, c->stream>>>(reinterpret_cast<uint4*>(c->f.bv + first), reinterpret_cast<const uint4*>(tmp.p), n_pad / 4, nullptr, nullptr, 0);
    e = hipGetLastError();
  }
  const hipError_t se = hipStreamSynchronize(c->stream);
  tmp.clear();
  if (e == hipSuccess) {
    e = se;
  }
  if (e != hipSuccess) {
    return set_err(c, GRP_ERR_HIP, "grp_bv_or_words: %s", hipGetErrorString(e));
  }
  return GRP_OK;
}

} // extern "C"
