// The words a query launch and the host thread hand each other: the streaming window's acknowledgement block, command,
// abort line and `executed` counters, the query counters of every k_query / k_verify launch, and the control block of a
// window that applies inserts itself.  grpath_hip.hip includes it in front of the kernels (grp_kernels.inc, grp_verify.inc)
// and the host code (grp_query.inc, grp_stream.inc), which all use it: an index or a code is written here and nowhere else.
// Plain C++, no HIP types.
#pragma once
#include <stdint.h>

// ---- acknowledgement block (QuerySlot::StreamWindow::h_ack, DevStreamCtl::ack_host): mapped host memory, uint32 words,
// written by the launch, read by the host
enum : uint32_t
{
  ACK_APPLIED = 0,       // inserts the launch has applied (= the sequence number of the last command that is through)
  ACK_CODE = 1,          // ACK_CODE_*: why the launch ended without the command posted last
  ACK_PHASE = 4,         // [ACK_PHASES] workgroup 0's times of the last insert, 100 MHz ticks: collect, first wait, apply, second wait
  ACK_IDLE_PARK = 8,     // what a launch that left at its idle limit was waiting on: the park word,
  ACK_IDLE_DECIDED = 9,  //   SCT_DECIDED,
  ACK_IDLE_NEXT_TILE = 10, // the tile dispenser,
  ACK_IDLE_EVENT = 11,   //   SCT_EVENT,
  ACK_IDLE_CMD_SEQ = 12, //   the command sequence number it saw,
  ACK_IDLE_GEN = 13,     //   SCT_GEN
  ACK_GAVE_UP_WHO = 14,  // the first workgroup whose grid-wide wait timed out: wait number [15:0], workgroup [31:16]
  ACK_GAVE_UP_COUNT = 15, // ... members that had arrived [15:0] of how many [31:16]
  ACK_WORDS = 16         // the block's allocation
};
constexpr uint32_t ACK_PHASES = 4;

enum : uint32_t
{
  ACK_CODE_NONE = 0,
  ACK_CODE_NOT_APPLIED = 1,  // the first grid-wide wait timed out: only the scratch table was touched, the host applies the insert
  ACK_CODE_WAIT_TIMEOUT = 2, // the second one did, in the middle of the insert: the ID array may be inconsistent
  ACK_CODE_IDLE_EXIT = 3     // the parked launch was told nothing for its idle limit and left; it had modified nothing
};

// what grp_classify_stream_end returns (beside GRP_OK / an error) for a launch that ended without the insert posted last
// (include/grpath.h), by the launch's code: 2 = its first grid-wide wait timed out (ACK_CODE_NOT_APPLIED), 1 = it had left or an
// abort overtook the command (ACK_CODE_NONE, ACK_CODE_IDLE_EXIT; ACK_CODE_WAIT_TIMEOUT is an error before this is asked)
constexpr int
stream_end_unapplied(uint32_t code)
{
  return code == ACK_CODE_NOT_APPLIED ? 2 : 1;
}

// ---- command (h_cmd, DevStreamCtl::cmd_host): mapped host memory; word CMD_SEQ the sequence number of the newest
// command, its fields from word CMD_FIELDS on.  The relay copies the fields to SCT_CMD: one enum serves both.
enum : uint32_t
{
  CMD_READ = 0,         // the inserting read (batch index)
  CMD_TILE_START = 1,
  CMD_TILE_END = 2,
  CMD_BLOCK_TILES = 3,
  CMD_FIRST_ID = 4,
  CMD_ID_OFFSET = 5,
  CMD_RESUME_READ = 6,  // window index of the first read behind it
  CMD_RESUME_TILE = 7,  // this launch's first tile behind it (where its dispenser starts over)
  CMD_DECIDED_BASE = 8, // this launch's decidable reads up to it
  CMD_GEN = 9,          // generation of the records from here on
  CMD_N_FIELDS = 10
};
constexpr uint32_t CMD_SEQ = 0, CMD_FIELDS = 1;
constexpr uint32_t CMD_WORDS = 16; // the block's allocation

// ---- abort line (d_abort): device memory, what the workgroups test and draw from
enum : uint32_t
{
  ABORT_FLAG = 0,       // raised by the relays (and the deciding wave) when the host's flag is up
  ABORT_NEXT_TILE = 32, // the tile dispenser, on a 128-byte line of its own
  ABORT_PARK = 48,      // first stale read of the window (UINT_MAX: none)
  ABORT_WORDS = 64
};
constexpr uint32_t ABORT_BYTES = ABORT_WORDS * 4u; // cleared in front of every window

constexpr uint32_t STREAM_STOP = 0x40000000u; // the tile dispenser at or beyond this: no more tiles are handed out (windows hold at most 2^30 tiles)

// ---- `executed` (d_executed / h_executed, DevStreamCtl::executed): unsigned long long counters of one window.  Words 1 .. 7
// are what grp_debug_stream_stats returns in this order; goldrush_amd/native.py (Engine.stream_stats) names them by
// position and is the other holder of the order.
enum : uint32_t
{
  EXE_PROBES = 0,          // probes of the tiles that were processed
  EXE_KEPT = 1,            // behind in-launch inserts: finished tiles kept,
  EXE_REDONE_DIRTY = 2,    //   finished tiles queried again (a probe's slot changed),
  EXE_REDONE_LOST = 3,     //   finished tiles queried again (fingerprints gone),
  EXE_INPROGRESS_KEPT = 4, //   tiles in progress that went on,
  EXE_INPROGRESS_REDONE = 5, // that started over,
  EXE_INSERTS_KEPT_NONE = 6, // inserts that kept nothing (everything handed out again),
  EXE_INSERTS_KEPT = 7,    //   inserts that kept
  EXE_WORDS = 8
};

// ---- query counters (d_qctr / h_qctr; the `ctr` of k_query and k_verify): 64-bit words, zero between calls
enum : uint32_t
{
  QCTR_UNUSED = 0,
  QCTR_FLAGGED_DISTINCT = 1, // statistics: tiles with more distinct IDs than the launch's table takes
  QCTR_FLAGGED_LIST = 2,     // statistics: ... with a longer list than the launch takes
  QCTR_LIST_CURSOR = 3,      // list arena cursor
  QCTR_FLAGGED = 4,          // tiles flagged for the worst-case launch (their indices: d_flag_idx)
  QCTR_IMPOSSIBLE = 5,       // k_verify: tiles with an impossible delta
  QCTR_UNCERTIFIED = 6,      // k_verify: tiles redone because their patch was not certified,
  QCTR_UNPATCHED = 7,        //   because they could not be patched
  QCTR_WORDS = 8
};

// ---- control block of a streaming window that applies inserts itself (grp_classify_stream_insert) ----
// uint32 words, every hot word on its own 128-byte line
enum : uint32_t
{
  SCT_GEN = 0 * 32,      // generation of the records being produced (= 1 + inserts applied by this launch); .pad of a record
  SCT_EVENT = 1 * 32,    // master event word: (insert commands seen << 1) | exit bit; advanced by CAS (relay workgroups)
  SCT_CMD = 2 * 32,      // the insert command, copied from host memory by the relay: its CMD_* fields
  SCT_DECIDED = 3 * 32,  // reads decided since the last resume (+ base)
  SCT_UNIT = 4 * 32,     // [parity] collect-unit dispenser
  SCT_APPLY = 5 * 32,    // [parity] apply-chunk dispenser
  SCT_IRCOUNT = 6 * 32,  // [parity] claimed table slots
  SCT_ALIVE = 7 * 32,    // round 6: workgroups of the launch that have begun [11:0], inserts the launch has taken [30:12], bit 31: an insert
                         //   is in progress (a workgroup that begins now is not among its members: stream_register)
  SCT_ERR = 8 * 32,      // != 0: a grid-wide wait timed out
  SCT_BAR = 9 * 32,      // [4 lines: parity x first / second wait] members that have arrived (zeroed with the other parity's insert)
  SCT_MEMBERS = 13 * 32, // workgroups the insert in progress waits for (SCT_ALIVE's count when its event was published)
  SCT_DONE = 14 * 32,    // [0] event word of the last insert that is through, [1] grid-wide waits passed with it: where a workgroup that begins late picks up
  SCT_EV = 41 * 32,      // [16 lines] copy of the event word per group (what idle workgroups poll)
  SCT_SCAN_END = 57 * 32,  // round 6: dispenser position the insert in progress found (tiles in front of it were handed out under the old state: they carry marks); bit 31: nothing of them is kept
  SCT_FRONTIER = 58 * 32,  // the furthest the dispenser has stood at an insert (monotonic): the end of the second walk — tiles in front of it may carry marks
  SCT_WORDS = 59 * 32
};
constexpr uint32_t SCT_GROUPS = 16;

constexpr uint32_t STREAM_REL_WGS = 4096; // workgroups of a streaming launch at most (a release line each)

// ---- what the code assumes of the above
namespace grp_proto_check {
template<typename... T>
constexpr bool
distinct_below(uint32_t limit, T... words)
{
  const uint32_t w[] = { (uint32_t)words... };
  for (unsigned i = 0; i < sizeof...(T); ++i) {
    if (w[i] >= limit) {
      return false;
    }
    for (unsigned j = 0; j < i; ++j) {
      if (w[j] == w[i]) {
        return false;
      }
    }
  }
  return true;
}
} // namespace grp_proto_check
static_assert(grp_proto_check::distinct_below(ACK_WORDS, ACK_APPLIED, ACK_CODE, ACK_PHASE, ACK_PHASE + 1, ACK_PHASE + 2, ACK_PHASE + 3, ACK_IDLE_PARK, ACK_IDLE_DECIDED, ACK_IDLE_NEXT_TILE, ACK_IDLE_EVENT,
                                              ACK_IDLE_CMD_SEQ, ACK_IDLE_GEN, ACK_GAVE_UP_WHO, ACK_GAVE_UP_COUNT) && ACK_PHASES == 4,
              "the acknowledgement block's words are distinct and inside its allocation");
static_assert(grp_proto_check::distinct_below(CMD_N_FIELDS, CMD_READ, CMD_TILE_START, CMD_TILE_END, CMD_BLOCK_TILES, CMD_FIRST_ID, CMD_ID_OFFSET, CMD_RESUME_READ, CMD_RESUME_TILE, CMD_DECIDED_BASE, CMD_GEN),
              "the command's fields are distinct");
static_assert(CMD_SEQ < CMD_FIELDS && CMD_FIELDS + CMD_N_FIELDS <= CMD_WORDS, "the command fits its block in host memory");
static_assert(CMD_N_FIELDS <= 32 && SCT_CMD + CMD_N_FIELDS <= SCT_DECIDED, "the command fits SCT_CMD's 128-byte line");
static_assert(grp_proto_check::distinct_below(ABORT_WORDS, ABORT_FLAG, ABORT_NEXT_TILE, ABORT_PARK) && ABORT_BYTES == ABORT_WORDS * sizeof(uint32_t), "the abort line's clear covers its words");
static_assert(ABORT_NEXT_TILE / 32 != ABORT_FLAG / 32, "the tile dispenser has a 128-byte line of its own");
static_assert(grp_proto_check::distinct_below(EXE_WORDS, EXE_PROBES, EXE_KEPT, EXE_REDONE_DIRTY, EXE_REDONE_LOST, EXE_INPROGRESS_KEPT, EXE_INPROGRESS_REDONE, EXE_INSERTS_KEPT_NONE, EXE_INSERTS_KEPT),
              "the executed counters are distinct and inside their allocation");
static_assert(grp_proto_check::distinct_below(QCTR_WORDS, QCTR_UNUSED, QCTR_FLAGGED_DISTINCT, QCTR_FLAGGED_LIST, QCTR_LIST_CURSOR, QCTR_FLAGGED, QCTR_IMPOSSIBLE, QCTR_UNCERTIFIED, QCTR_UNPATCHED),
              "the query counters are distinct and inside their allocation");
static_assert(SCT_EV + SCT_GROUPS * 32 <= SCT_SCAN_END && SCT_BAR + 4 * 32 <= SCT_MEMBERS && SCT_FRONTIER < SCT_WORDS, "the control block's lines do not overlap");
