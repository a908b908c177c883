// frame_state.h — the per-frame device block of a handle, described once for device and host code:
//   FrameState = FrameCounters | FramePlans { keys, pairs, os } | FrameArgs
// Two of the plans' histogram rows carry words of their own during a frame, named here and nowhere else: the frame's key sort keeps
// its totals in the OsPlan, so keys.ghist is the 32 statistics lines (FrameStatLine); the direct binning runs no pair sort, so the
// first rows of pairs.ghist are its tables (DirectBinTables).
#pragma once
#include <cstddef>
#include <cstdint>

#include "device_types.h"
#include "sort_plan.h"

namespace mgs {

// device-resident counters of one frame
struct FrameCounters
{
  uint32_t pad0;
  uint32_t sortedCount;    // V: elements handed to the radix sort
  uint32_t pairCount;      // D: (tile, splat) records
  uint32_t errorFlags;
  uint32_t pad[27];
};

// One line of the frame's statistics.  Whoever counts picks a line by a number of its own (region, partition, wave) and adds with
// a fire-and-forget atomic; the host sums the lines (foldFrameStats).  32 lines, because a single line's atomic unit was what the
// kernels' tails waited for.
constexpr uint32_t kFrameStatSlots = 32;
struct FrameStatLine
{
  uint32_t staged;       // records the compositors staged and shaded (MgsFrameOut::shaded_count)
  uint32_t scanned;      // list entries their regions looked at (scanned_entries)
  uint32_t survivors;    // splats that passed the dist-stage cull, one add per partition of the project kernels (frustum_count)
  uint32_t escapes;      // sorted splats whose bin rectangle fitted no code: k_dbin_count (escape_count)
  uint32_t listEntries;  // line 0 only: the frame's list entries D, stored by k_dbin_emit for the adaptive bin size (BinPolicy)
  uint32_t pad[27];
};

// The direct binning's tables.  On the record path the same rows are the pair sort's digit totals, and the compositors — which
// read binOrderValid on either path — find zero there because that sort never runs a third pass: a bin coordinate is 8 bits, so
// there are at most 65 536 bins and the sorted key has at most 16 bits (kPairSortMaxBits; issueBinning checks it).
struct DirectBinTables
{
  uint32_t binTotal[256];  // list entries per bin (k_dbin_scan)
  uint32_t binOrder[256];  // binOrder[rank] = bin: the order the compositors take the bins in (k_dbin_emit)
  uint32_t binOrderValid;  // != 0: binOrder was written this frame
};
constexpr int kPairSortMaxBits = 16;

// the per-frame sort state of one context
struct FramePlans
{
  SortPlan keys;   // what the consumers of the sorted ids read (n, finalSel, passesRun, rideInfo); its ghist: the statistics lines
  SortPlan pairs;  // the record path's pair sort; its ghist otherwise: the direct binning's tables
  OsPlan   os;     // the key sort's own plan
};

// One device block per handle: what every frame starts from zero, followed by the frame's constants.  A frame begins with ONE
// upload that carries the zeros along with the constants, so a captured frame graph replays with nothing but the upload.
struct FrameState
{
  FrameCounters ctr;
  FramePlans    plans;
  FrameArgs     args;  // view / proj, instances, knobs: the kernels read them through this pointer
};

// ---- the layout is part of the kernels' machine code (immediate offsets) and of the upload's size: pinned -----------------------
static_assert(sizeof(FrameCounters) == 124 && sizeof(SortPlan) == 4160 && sizeof(OsPlan) == 4672, "frame block: member sizes");
static_assert(offsetof(FramePlans, keys) == 0 && offsetof(FramePlans, pairs) == 4160 && offsetof(FramePlans, os) == 8320, "FramePlans");
static_assert(offsetof(FrameState, ctr) == 0 && offsetof(FrameState, plans) == 124 && offsetof(FrameState, args) == 13120, "FrameState");
static_assert(sizeof(FrameStatLine) == 128, "one statistics line");
static_assert(offsetof(SortPlan, ghist) == 0 && sizeof(FrameStatLine) * kFrameStatSlots == sizeof(SortPlan::ghist),
              "the statistics lines cover the keys plan's histogram rows exactly");
static_assert(offsetof(DirectBinTables, binTotal) == offsetof(SortPlan, ghist[0]) && offsetof(DirectBinTables, binOrder) == offsetof(SortPlan, ghist[1])
                  && offsetof(DirectBinTables, binOrderValid) == offsetof(SortPlan, ghist[2][0]),
              "the direct binning's tables are rows 0, 1 and the first word of row 2 of the pairs plan");
static_assert(kPairSortMaxBits <= 16, "a third pass of the pair sort would write its totals over binOrderValid");

// ---- typed views (host and device; only addresses are formed, so the host may call them on device pointers) ------------------------
// (the kernels hold the keys plan as const — they only read the plan proper — and add to the lines beside it)
__host__ __device__ inline FrameStatLine* frameStatLines(const SortPlan* keys /* &FramePlans::keys */)
{
  return reinterpret_cast<FrameStatLine*>(const_cast<uint32_t(*)[256]>(keys->ghist));
}
__host__ __device__ inline DirectBinTables* directBinTables(SortPlan* pairs /* &FramePlans::pairs */) { return reinterpret_cast<DirectBinTables*>(pairs->ghist); }
__host__ __device__ inline const DirectBinTables* directBinTables(const SortPlan* pairs) { return reinterpret_cast<const DirectBinTables*>(pairs->ghist); }

// A kernel receives one plan, not the block.  From that plan to the block: `held` is offsetof(FramePlans, <the member it addresses>).
__host__ __device__ inline const FramePlans* framePlansOf(const void* plan, size_t held)
{
  return reinterpret_cast<const FramePlans*>(static_cast<const char*>(plan) - held);
}
// ... and to a statistics line, for the three kinds of kernel that count: k_dbin_* hold the keys plan, k_composite* the pairs plan,
// k_project* the key sort's.  (The line's offset is formed in 32-bit words, the way the kernels have always formed it: indexing
// the lines gives the same address by other instructions, and this header's introduction was to leave the machine code alone.)
__host__ __device__ inline FrameStatLine* frameStatLine(const void* plan, size_t held, uint32_t slot)
{
  constexpr uint32_t kLineWords = sizeof(FrameStatLine) / sizeof(uint32_t);
  uint32_t*          words      = &frameStatLines(&framePlansOf(plan, held)->keys)->staged;
  return reinterpret_cast<FrameStatLine*>(words + kLineWords * (slot & (kFrameStatSlots - 1u)));
}
__host__ __device__ inline FrameStatLine* frameStatLineFromKeys(const SortPlan* keys, uint32_t slot) { return frameStatLine(keys, offsetof(FramePlans, keys), slot); }
__host__ __device__ inline FrameStatLine* frameStatLineFromPairs(const SortPlan* pairs, uint32_t slot) { return frameStatLine(pairs, offsetof(FramePlans, pairs), slot); }
__host__ __device__ inline FrameStatLine* frameStatLineFromOs(const OsPlan* os, uint32_t slot) { return frameStatLine(os, offsetof(FramePlans, os), slot); }
// k_dbin_emit receives binTotal and binOrder as two pointers (read-only / written): the flag behind the latter
__host__ __device__ inline uint32_t* binOrderValidOf(uint32_t* binOrder /* DirectBinTables::binOrder */)
{
  return binOrder + (offsetof(DirectBinTables, binOrderValid) - offsetof(DirectBinTables, binOrder)) / sizeof(uint32_t);
}

// the lines' sums, as mgs_frame_stats reports them (32-bit counts wrap like the MgsFrameOut fields they fill)
struct FrameStatTotals
{
  uint32_t staged = 0, survivors = 0, escapes = 0, listEntries = 0;
  uint64_t scanned = 0;
};
inline FrameStatTotals foldFrameStats(const FrameStatLine* lines /* host copy */)
{
  FrameStatTotals t;
  for(uint32_t i = 0; i < kFrameStatSlots; ++i)
    t.staged += lines[i].staged, t.scanned += lines[i].scanned, t.survivors += lines[i].survivors, t.escapes += lines[i].escapes;
  t.listEntries = lines[0].listEntries;
  return t;
}

}  // namespace mgs
