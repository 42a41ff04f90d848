// The contract of goldrush_amd/csrc/grp_buffers.h on a machine WITHOUT a GPU (tests/test_buffers_cpu.py builds this with
// the address and undefined-behaviour sanitizers and runs it): there every HIP allocation fails, so this is the side
// of the owners no GPU test reaches — the failing reset / ensure, and what moves and release leave behind.
// Exit status 0: every check held; a check that fails prints its line.
#include "grp_buffers.h"

#include <cstdio>
#include <type_traits>
#include <utility>

static int g_failed = 0;

#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);                                         \
      ++g_failed;                                                                                                      \
    }                                                                                                                  \
  } while (0)

static_assert(!std::is_copy_constructible_v<DevBuf<uint32_t>> && !std::is_copy_assignable_v<DevBuf<uint32_t>>, "DevBuf copies");
static_assert(!std::is_copy_constructible_v<HostBuf<uint32_t>> && !std::is_copy_assignable_v<HostBuf<uint32_t>>, "HostBuf copies");
static_assert(!std::is_copy_constructible_v<Event> && !std::is_copy_assignable_v<Event>, "Event copies");
static_assert(std::is_nothrow_move_constructible_v<DevBuf<uint32_t>> && std::is_nothrow_move_assignable_v<DevBuf<uint32_t>>, "DevBuf moves");
static_assert(std::is_nothrow_move_constructible_v<HostBuf<uint32_t>> && std::is_nothrow_move_assignable_v<HostBuf<uint32_t>>, "HostBuf moves");
static_assert(std::is_nothrow_move_constructible_v<Event> && std::is_nothrow_move_assignable_v<Event>, "Event moves");

// memory that is nobody's to free: what a moved owner holds in these checks, always taken away again
static uint32_t g_fake[64], g_fake2[64];

static void
dev_buf()
{
  {
    DevBuf<uint32_t> b;
    CHECK(b.p == nullptr && b.cap == 0 && static_cast<uint32_t*>(b) == nullptr);
    CHECK(b.reset(100) != hipSuccess); // no device: the allocation fails
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.ensure(100) != hipSuccess); // a second failure, then destruction
    CHECK(b.p == nullptr && b.cap == 0);
    b.clear();
    CHECK(b.release() == nullptr);
  }
  {
    // ensure within the capacity makes no runtime call: it succeeds where every call fails, and changes nothing
    DevBuf<uint32_t> b;
    b.p = g_fake;
    b.cap = 64;
    CHECK(b.ensure(0) == hipSuccess && b.ensure(1) == hipSuccess && b.ensure(64) == hipSuccess);
    CHECK(b.p == g_fake && b.cap == 64 && static_cast<uint32_t*>(b) == g_fake);
    // move construction and move assignment: the source is empty, the target holds what the source held
    DevBuf<uint32_t> c(std::move(b));
    CHECK(b.p == nullptr && b.cap == 0 && c.p == g_fake && c.cap == 64);
    DevBuf<uint32_t> d;
    d = std::move(c);
    CHECK(c.p == nullptr && c.cap == 0 && d.p == g_fake && d.cap == 64);
    d = std::move(d); // (self-assignment keeps it)
    CHECK(d.p == g_fake && d.cap == 64);
    CHECK(d.release() == g_fake && d.p == nullptr && d.cap == 0);
    CHECK(d.ensure(65) != hipSuccess && d.p == nullptr && d.cap == 0);
  }
  {
    DevBuf<uint32_t> a, b, c;
    clear_all(a, b, c);
    CHECK(!a.p && !b.p && !c.p);
  }
}

static void
host_buf()
{
  for (unsigned int flags : { (unsigned int)hipHostMallocDefault, (unsigned int)(hipHostMallocMapped | hipHostMallocCoherent) }) {
    HostBuf<uint32_t> b;
    CHECK(b.p == nullptr && b.dev == nullptr && b.cap == 0);
    CHECK(b.reset(100, flags) != hipSuccess);
    CHECK(b.p == nullptr && b.dev == nullptr && b.cap == 0);
    CHECK(b.reset(7, flags) != hipSuccess);
    CHECK(b.p == nullptr && b.dev == nullptr && b.cap == 0);
  }
  {
    HostBuf<uint32_t> b;
    b.p = g_fake;
    b.dev = g_fake2;
    b.cap = 64;
    CHECK(b.p == g_fake && b.dev == g_fake2 && b.cap == 64 && static_cast<uint32_t*>(b) == g_fake);
    HostBuf<uint32_t> c(std::move(b));
    CHECK(b.p == nullptr && b.dev == nullptr && b.cap == 0 && c.p == g_fake && c.dev == g_fake2 && c.cap == 64);
    HostBuf<uint32_t> d;
    d = std::move(c);
    CHECK(c.p == nullptr && c.dev == nullptr && c.cap == 0 && d.p == g_fake && d.dev == g_fake2 && d.cap == 64);
    CHECK(d.release() == g_fake && d.p == nullptr && d.dev == nullptr && d.cap == 0);
  }
}

static void
event()
{
  {
    Event e;
    CHECK(e.e == nullptr);
    CHECK(e.create(hipEventDisableTiming) != hipSuccess && e.e == nullptr);
    CHECK(e.create(hipEventDefault) != hipSuccess && e.e == nullptr);
  }
  {
    Event a;
    a.e = reinterpret_cast<hipEvent_t>(g_fake);
    Event b(std::move(a));
    CHECK(a.e == nullptr && b.e == reinterpret_cast<hipEvent_t>(g_fake) && static_cast<hipEvent_t>(b) == b.e);
    Event c;
    c = std::move(b);
    CHECK(b.e == nullptr && c.e == reinterpret_cast<hipEvent_t>(g_fake));
    c.e = nullptr; // (taken away again)
  }
}

int
main()
{
  dev_buf();
  host_buf();
  event();
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("grp_buffers.h: contract holds\n");
  return 0;
}
