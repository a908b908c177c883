// osort_common.h — what the units of the frame's depth-key sort share: constants, the look-back words' access, the argument
// struct of a pass and the launchers that cross the units.  No kernels.
//
// The sort: stable LSD radix sort of (u32 key, u32 id) pairs, 8-bit digits, element count read on the device (behavioural spec:
// vrdxCmdSortKeyValueIndirect, 3rdparty/vrdx/src/vk_radix_sort.cc:262-416).  Every pass is ONE kernel: each partition publishes
// its digit counts, resolves its digit prefixes from the partitions before it while it ranks its keys, and scatters.  What the
// passes need up front comes from the producer:
//   * pass 0 is virtual.  k_project writes its slot grouped by the key's low byte (slot_emit.h) together with the groups' counts
//     and starts; where a pair stands after a stable pass on bits 0-7 is a function of those counts alone, so that pass is never
//     run: k_os_prepare turns the counts into two small tables and the sort's first kernel (bits 8-15) gathers its dense
//     partitions straight from the slots in digit-0 order (k_os_pass<3>);
//   * k_project also leaves the slot's histogram of bits 8-15 and, per wave, a record of how often each value of key >> 16
//     occurs; k_os_prepare reduces them to the digit totals and a 64 K-entry count table, and when at most 256 values of
//     key >> 16 occur pass 2 sorts on the RANK of key >> 16 among them and pass 3 does not run (foldTop16).
//   => launches per frame sort: prepare + 2 passes (+ 1 that exits at once).
//
//   k_osort_prepare.hip  k_os_hist (stand-alone sort: digit totals), k_os_prepare (frame: totals and the virtual pass 0's tables),
//                        k_os_plan_clear
//   k_osort_pass.hip     foldTop16, k_os_pass: one pass, with the look-back protocol
//   osort_launch.hip     host only: grid and status-word sizing, the pass schedules and their look-back rota, launchOsSort
// What was tried, measured and dropped on the way here: docs/DESIGN_history_keysort.md.
#pragma once
#include "kernels_common.h"
#include "frame_state.h"
#include "sort_plan.h"

namespace mgs {

constexpr int      kThreads = 256;
constexpr int      kKpt     = kOsPart / kThreads;  // 16
constexpr int      kWaves   = kThreads / 64;
// look-back words: flag (bits 30-31) and value in one 32-bit word
constexpr uint32_t kAgg = 1u << 30, kInc = 2u << 30, kValMask = (1u << 30) - 1u;
constexpr int      kGroupWindow = 16;
constexpr uint32_t kSpinMax     = 1u << 21;  // polls before a wait gives up (seconds; a healthy wait is a few polls)
static_assert(kOsGroup == 32, "the member mask is one 32-bit word");
// workgroups beyond the partitions of the frame's first sort kernel: they fold the count table of key >> 16 (foldTop16)
constexpr uint32_t kOsFoldWgs = 8;
// Grid of a pass (and rows of its look-back words): partitions of kOsPart pairs for the largest count, and at least as many
// workgroups as 1024-pair partitions of that count, up to kOsSmallGrid, so that a sort of few keys can spread over the chip
// (osPartOf).  Workgroups beyond the partitions exit after the set-up.
constexpr uint32_t kOsSmallGrid = 1024;

__device__ __forceinline__ uint32_t ldAgent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void     stAgent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive scan of one value per digit over the 256 threads of the block
__device__ __forceinline__ uint32_t scan256(uint32_t v, uint32_t* s_tmp /*4*/)
{
  const int      lane = laneId(), w = threadIdx.x >> 6;
  const uint32_t inc  = waveInclusiveScan(v);
  if(lane == 63)
    s_tmp[w] = inc;
  __syncthreads();
  uint32_t base = 0;
  if(w > 0) base += s_tmp[0];
  if(w > 1) base += s_tmp[1];
  if(w > 2) base += s_tmp[2];
  __syncthreads();
  return base + inc - v;
}

#ifdef MGS_OS_TRACE  // debug build (tools/os_trace.py): per-workgroup wall-clock stamps (100 MHz) of the phases of every pass
#define MGS_OS_STAMP(i) if(threadIdx.x == 0) trc[i] = wall_clock64();
#define MGS_OS_GSTAMP(i) if(threadIdx.x == 0 && gtr[i] == 0) gtr[i] = wall_clock64();  // the virtual pass 0's table (first time only)
#else
#define MGS_OS_STAMP(i)
#define MGS_OS_GSTAMP(i)
#endif

// One pass.  IN: 0 dense pairs (the output of the pass before); 2 split key / value arrays (pass 0 of the stand-alone sort);
// 3 the project kernels' slots, read in the order a stable pass on key bits 0-7 WOULD have left them in ("virtual pass 0": the
// first kernel of a frame's sort sorts on bits 8-15).  Dense partition p = positions [4096 p, 4096 p + count) of that order.
// Position x holds a pair of digit-0 value d = the one with D[d] <= x < D[d + 1] (D = exclusive scan of plan->total[0]); within
// d the slots follow each other, each with its group of d (slot_emit.h), so with c = the chunk of 32 slots and s the slot that
// x - D[d] falls into: x = D[d] + (sum of chunkSum[c'][d], c' < c) + runTab[d][s].low16 + i, and the pair is entry
// runTab[d][s].high16 + i of slot s.  The workgroup expands exactly the runs that overlap its partition into a 4096-entry
// source table in LDS (one prefix scan over the chunks per digit value it touches — usually one or two —, then one coalesced
// read of the runTab segment) and gathers: loads of <= 8-byte runs of ~6 pairs instead of contiguous reads, but everything else
// of a pass 0 — ranking, look-back, re-order, scatter, 67 MB of traffic — is not done at all.
struct OsPassArgs
{
#ifdef MGS_OS_TRACE
  uint64_t* trace;  // [partition][8]
#endif
  const uint2*    srcPairs;
  const uint32_t* chunkSum;  // IN 3: [chunks][256]
  const uint32_t* runTab;    // IN 3: [256][32 chunks]
  uint32_t        chunks;
  uint32_t        srcLimit;  // IN 3: the last valid pair index (a corrupted table must not turn into a wild read)
  uint32_t*       top16Count;  // IN 3: the grid's LAST workgroups fold the count table of key >> 16 for the kernel behind this one
  int             allowRemap;
  // the bin rectangles' codes ride above the ids (kernels_common.h: rideEncode); the final pass of a frame separates them:
  // clean ids for everybody, the codes in sorted order for the binning stage
  uint32_t        rideShift;   // bits of the id proper; 0 = nothing rides
  uint32_t        rideSplit;   // 1: the code's low 8 bits lie in the key's low byte, the rest above the id (slot_emit.h)
  uint32_t        rideInfo;    // what planOut->rideInfo tells k_dbin_count: shapes | code bits << 8
  uint16_t*       dstCode16;
  const uint32_t* srcKeys;
  const uint32_t* srcVals;
  uint2*          dstPairs;
  uint32_t*       dstKeys;  // final pass: may be null (the frame does not need the keys again)
  uint32_t*       dstVals;
  OsPlan*         plan;
  SortPlan*       planOut;  // what the consumers of the sorted ids read: n, finalSel (always 0 here), passesRun
  uint32_t*       status;   // [maxParts][256] this pass: one 1 KB row of digit counts per partition
  uint32_t*       gstatus;  // [ceil(maxParts / 32)][256]
  uint32_t*       zStatus;  // look-back words no pass is using: cleared here for a later pass (osort_launch.hip has the rota)
  uint32_t        zWords;
  const uint32_t* nPtr;
  FrameCounters*  ctr;
  int             pass;
  int             digitMode;  // 0 plain byte `pass`; 1 pass 2: rank of key >> 16 when the plan says remap, else plain; 2 pass 3: exits when remapped
  int             finalMode;  // 0 writes pairs; 1 writes the result; 2 writes the result iff the plan says remap (pass 2)
  // the partition size is chosen ON THE DEVICE from the element count (osPartOf below): ~384 partitions between partMin and kOsPart
  uint32_t        partMin;    // smallest partition size allowed (kOsPart: fixed partitions)
  uint32_t        resSlots;   // workgroups of this kernel the chip holds at once
  uint32_t        flatLookback;  // 1: sorts of at most 32 groups resolve the groups before a partition from COUNTED SUMS instead of the chain of group prefixes (k_osort_pass.hip; MGS_OS_FLAT)
};

// A sort of few keys would run on few workgroups (a strip's 0.32 M keys are 78 partitions of 4096 on 256 CUs).  The rounds of a
// partition adapt to its element count anyway (the ragged last one), so the SAME kernel takes smaller partitions: every workgroup
// derives the size from n (device-side count, identical for all) and the grid the host launched — no host-side guess, nothing in
// the graph key.  The size: ~384 partitions, in steps of 512 pairs, between partMin (1 536) and 4 096 — so every sort above 1.5 M
// keys keeps 4 096 — and only while all partitions are resident at once.  MGS_OS_PART_MIN=4096: fixed partitions (A/B; the variants
// test runs it).  Measurements: docs/DESIGN_history_keysort.md.
__device__ __forceinline__ uint32_t osPartOf(uint32_t n, uint32_t grid, uint32_t partMin, uint32_t resSlots)
{
  if(partMin >= kOsPart)
    return kOsPart;
  // ~384 partitions, in steps of 512 pairs, between partMin and kOsPart
  const uint32_t cap  = min(grid, resSlots);
  const uint32_t want = ((n / 384u + 511u) / 512u) * 512u;
  const uint32_t part = min(max(want, partMin), kOsPart);
  return (n + part - 1u) / part <= cap ? part : kOsPart;
}

// ---- launchers that cross the units (a kernel is launched from the unit that defines it) -------------------------------------
// The kernel instantiations of a pass: what it reads (IN above) and whether it can sort on the rank of key >> 16 (REMAP).
enum class OsVariant
{
  Split,     // k_os_pass<2, false>: split key / value arrays
  Slots,     // k_os_pass<3, false>: the project kernels' slots (virtual pass 0); kOsFoldWgs workgroups more than partitions
  Dense,     // k_os_pass<0, false>
  DenseRank  // k_os_pass<0, true>
};
void launchOsHist(hipStream_t stream, const OsLaunch& L);     // stand-alone sort only
void launchOsPrepare(hipStream_t stream, const OsLaunch& L);  // both: a frame's sort is the one with L.pairs0
void launchOsPass(hipStream_t stream, OsVariant variant, uint32_t grid, const OsPassArgs& a);
#ifdef MGS_OS_TRACE
void osPrepTraceBind(uint64_t* buf);  // [reduce workgroup][8]: where k_os_prepare leaves its stamps
#endif

}  // namespace mgs
