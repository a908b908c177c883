// osort_launch.hip — the key sort as its callers see it (sort_plan.h): sizing of grids and look-back words, the schedules of
// the passes, launchOsSort.  Host only; the kernels are in k_osort_prepare.hip and k_osort_pass.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "osort_common.h"

namespace mgs {

// partMin = the smallest partition size the passes may choose on the device (osPartOf; Tuning::osPartMin): kOsPart = fixed
// partitions, and a grid of kOsPart-pair partitions is enough.
uint32_t osSortMaxParts(uint32_t maxElems, uint32_t partMin)
{
  const uint32_t big = (uint32_t)(((uint64_t)maxElems + kOsPart - 1u) / kOsPart);
  if(partMin >= kOsPart)
    return big;
  const uint32_t small = (uint32_t)std::min<uint64_t>(((uint64_t)maxElems + 1023u) / 1024u, kOsSmallGrid);
  return std::max(big, small);
}
// per set of look-back words: partition rows [partition][digit] (rounded up to whole groups) followed by group rows [group][digit]
static size_t osStatusGroups(uint32_t maxParts) { return (maxParts + kOsGroup - 1u) / kOsGroup + 1u; }
size_t        osSortStatusWords(uint32_t maxParts)
{
  const size_t groups = osStatusGroups(maxParts);
  return groups * 256u * kOsGroup + groups * 256u;
}

// ---------------------------------------------------------------------------------------------------------------------
// The schedules: one row per pass that runs.
//
// Look-back words come in kOsSets sets (L.status holds them back to back).  A pass needs the set it uses ZERO when it starts,
// and nobody sweeps the sets between sorts: every pass clears, beside its own work, sets that no pass is using, for a later pass
// of this sort or the first one of the next (the sets of a sort are zero before its first use: the callers' allocation).  A pass
// never clears the set it uses — its own workgroups are reading it.  A pass that can exit at once (digitMode 2) clears nothing,
// and what it may or may not have used is cleared before anybody uses it again, so the rota does not depend on whether it ran.
//   frame:        pass 1 uses set 0, clears 1 and 2;  pass 2 uses 1, clears 0 (for the next frame);  pass 3 uses 2.
//   stand-alone:  pass 0 uses set 0, clears 1 and 2;  pass 1 uses 1, clears 0 (for the next sort);  pass 2 uses 2, clears 1;
//                 pass 3 uses 1.
// Pairs ping-pong between L.pairA and L.pairB.  A frame's first pass reads the project kernels' slots, L.pairs0, which may alias
// pairB: it writes A, and the second pass is the first to write B.  The stand-alone sort's first pass reads L.keys0 / L.vals0.
// The last pass writes L.outVals (and L.outKeys, L.outCode16).  The checks below hold both tables to all of this.
constexpr int kOsSets = 3;
enum class OsBuf
{
  Slots,  // L.pairs0
  A,      // L.pairA
  B       // L.pairB
};
struct OsPassRow
{
  int       pass;  // the byte of the key: digit, plan->total row, passesRun
  OsVariant variant;
  int       set;                    // look-back words it uses
  int       clearFirst, clearSets;  // sets [clearFirst, clearFirst + clearSets) it clears
  OsBuf     src, dst;               // OsPassArgs::srcPairs (not read by OsVariant::Split), dstPairs (not written when finalMode is 1)
  int       digitMode, finalMode;   // OsPassArgs
  bool      foldWgs;                // kOsFoldWgs workgroups more than partitions
};
struct OsSchedule
{
  const OsPassRow* rows;
  int              count;
};
template <int N>
constexpr OsSchedule osSchedule(const OsPassRow (&rows)[N])
{
  return {rows, N};
}
// clang-format off
constexpr OsPassRow kOsFramePasses[] = {
    // pass variant               set  clears  src           dst       digit final fold
    {1, OsVariant::Slots,     0,   1, 2,   OsBuf::Slots, OsBuf::A, 0,    0,    true},
    {2, OsVariant::DenseRank, 1,   0, 1,   OsBuf::A,     OsBuf::B, 1,    2,    false},
    {3, OsVariant::Dense,     2,   0, 0,   OsBuf::B,     OsBuf::B, 2,    1,    false},
};
constexpr OsPassRow kOsAlonePasses[] = {
    {0, OsVariant::Split,     0,   1, 2,   OsBuf::B,     OsBuf::A, 0,    0,    false},
    {1, OsVariant::Dense,     1,   0, 1,   OsBuf::A,     OsBuf::B, 0,    0,    false},
    {2, OsVariant::Dense,     2,   1, 1,   OsBuf::B,     OsBuf::A, 0,    0,    false},
    {3, OsVariant::Dense,     1,   1, 0,   OsBuf::A,     OsBuf::B, 2,    1,    false},
};
// clang-format on

template <int N>
constexpr bool osScheduleOk(const OsPassRow (&rows)[N])
{
  bool zero[kOsSets] = {true, true, true};  // the callers' allocation
  for(int sort = 0; sort < 3; ++sort)       // a sort leaves the sets for the next one: the third starts as every later one does
    for(int i = 0; i < N; ++i)
    {
      const OsPassRow& r = rows[i];
      if(i > 0 && r.pass <= rows[i - 1].pass)
        return false;
      if(r.set < 0 || r.set >= kOsSets || !zero[r.set])
        return false;  // stale look-back words
      if(r.clearFirst < 0 || r.clearSets < 0 || r.clearFirst + r.clearSets > kOsSets)
        return false;
      if(r.clearSets > 0 && (r.digitMode == 2 || (r.clearFirst <= r.set && r.set < r.clearFirst + r.clearSets)))
        return false;  // clears what it is reading, or relies on a clear that does not happen when the pass exits
      zero[r.set] = false;  // (a pass that can exit at once as well: either is possible)
      for(int s = r.clearFirst; s < r.clearFirst + r.clearSets; ++s)
        zero[s] = true;
      if((r.variant == OsVariant::DenseRank) != (r.digitMode == 1) || (r.variant == OsVariant::Slots) != r.foldWgs)
        return false;
      if((r.src == OsBuf::Slots) != (r.variant == OsVariant::Slots) || r.dst == OsBuf::Slots)
        return false;
      if(r.finalMode != 1 && (r.src == OsBuf::Slots ? OsBuf::B : r.src) == r.dst)
        return false;  // scatters into what it reads (the slots may be B)
      if(r.finalMode == 2 && (r.digitMode != 1 || i + 1 >= N || rows[i + 1].digitMode != 2))
        return false;  // final iff the plan says remap: then every later pass must exit
      if((r.finalMode == 1) != (i == N - 1))
        return false;  // the last pass, and only the last, always writes the result
    }
  return true;
}
static_assert(osScheduleOk(kOsFramePasses), "the frame's pass schedule breaks a rule of the rota above");
static_assert(osScheduleOk(kOsAlonePasses), "the stand-alone pass schedule breaks a rule of the rota above");

// ---------------------------------------------------------------------------------------------------------------------
// Trace build (tools/os_trace.py, MGS_OS_TRACE_FILE): the passes' stamps, [4 passes][maxParts][8], and k_os_prepare's,
// [4096 reduce workgroups][8], are collected on the device and written to the file when the sort has been launched:
// header {maxParts, 0}, the passes' stamps, k_os_prepare's.  Frames only.
#ifdef MGS_OS_TRACE
struct OsTrace
{
  const char* path;  // null: not tracing
  uint64_t*   passBuf;
  uint64_t*   prepBuf;
  uint32_t    maxParts;
  size_t      passWords;  // per pass
};
static OsTrace osTraceBegin(hipStream_t stream, bool frame, uint32_t maxParts)
{
  static uint64_t* passBuf = nullptr;
  static uint64_t* prepBuf = nullptr;
  OsTrace          t{frame ? std::getenv("MGS_OS_TRACE_FILE") : nullptr, nullptr, nullptr, maxParts, (size_t)maxParts * 8};
  if(t.path)
  {
    if(!passBuf)
    {
      (void)hipMalloc(&passBuf, (size_t)4 << 24);
      (void)hipMalloc(&prepBuf, 4096 * 64);
      osPrepTraceBind(prepBuf);
    }
    (void)hipMemsetAsync(passBuf, 0, 4 * t.passWords * 8, stream);
    (void)hipMemsetAsync(prepBuf, 0, 4096 * 64, stream);
    t.passBuf = passBuf;
    t.prepBuf = prepBuf;
  }
  return t;
}
static void osTracePass(const OsTrace& t, int pass, OsPassArgs& a)
{
  a.trace = t.path ? t.passBuf + (size_t)pass * t.passWords : nullptr;
}
static void osTraceEnd(hipStream_t stream, const OsTrace& t)
{
  if(!t.path)
    return;
  (void)hipStreamSynchronize(stream);
  std::vector<uint64_t> h(4 * t.passWords);
  (void)hipMemcpy(h.data(), t.passBuf, 4 * t.passWords * 8, hipMemcpyDeviceToHost);
  if(FILE* fp = std::fopen(t.path, "wb"))
  {
    const uint64_t hdr[2] = {t.maxParts, 0};
    std::fwrite(hdr, 8, 2, fp);
    std::fwrite(h.data(), 8, 4 * t.passWords, fp);
    std::vector<uint64_t> hp(4096 * 8);
    (void)hipMemcpy(hp.data(), t.prepBuf, 4096 * 64, hipMemcpyDeviceToHost);
    std::fwrite(hp.data(), 8, hp.size(), fp);
    std::fclose(fp);
  }
}
#else
struct OsTrace
{
};
static inline OsTrace osTraceBegin(hipStream_t, bool, uint32_t) { return {}; }
static inline void    osTracePass(const OsTrace&, int, OsPassArgs&) {}
static inline void    osTraceEnd(hipStream_t, const OsTrace&) {}
#endif

// ---------------------------------------------------------------------------------------------------------------------
// what every pass of a sort receives alike
static OsPassArgs osCommonArgs(const OsLaunch& L, bool frame)
{
  OsPassArgs a{};
  a.plan         = L.plan;
  a.planOut      = L.planOut;
  a.nPtr         = L.nPtr;
  a.ctr          = L.ctr;
  a.partMin      = L.partMin;
  a.resSlots     = L.resSlots;
  a.flatLookback = L.flatLookback;
  a.dstKeys      = L.outKeys;
  a.dstVals      = L.outVals;
  a.chunkSum     = L.chunkSum;
  a.runTab       = L.runTab;
  a.chunks       = frame ? osSortChunks(L.prjParts) : 0u;
  a.srcLimit     = L.prjParts * kOsSlot - 1u;
  a.top16Count   = L.top16Count;
  // the rank digit and the riding codes are a frame's: the stand-alone sort's keys are anybody's
  a.allowRemap   = (frame && L.allowRemap) ? 1 : 0;
  a.rideShift    = frame ? L.rideShift : 0u;
  a.rideSplit    = frame ? L.rideSplit : 0u;
  a.rideInfo     = L.rideInfo;
  a.dstCode16    = L.outCode16;
  a.srcKeys      = L.keys0;
  a.srcVals      = L.vals0;
  return a;
}

void launchOsSort(hipStream_t stream, const OsLaunch& L)
{
  if(L.maxElems == 0 || (uint64_t)L.maxElems >= kOsMaxPairs)
    return;  // (the callers reject / re-route 2^30 pairs and more: a prefix would wrap inside its status word)
  const bool       frame    = L.pairs0 != nullptr;  // the project kernels' slots of pairs + their histograms / records
  const OsSchedule sched    = frame ? osSchedule(kOsFramePasses) : osSchedule(kOsAlonePasses);
  const uint32_t   maxParts = osSortMaxParts(L.maxElems, L.partMin);  // >= 1: the grid of every pass
  const size_t     sWords   = osSortStatusWords(maxParts);
  const size_t     gOffset  = osStatusGroups(maxParts) * 256u * kOsGroup;  // a set's group rows follow its partition rows
  const OsTrace    trace    = osTraceBegin(stream, frame, maxParts);
  if(!frame)
    launchOsHist(stream, L);
  launchOsPrepare(stream, L);
  const uint2* const srcOf[] = {L.pairs0, L.pairA, L.pairB};  // by OsBuf
  uint2* const       dstOf[] = {nullptr, L.pairA, L.pairB};
  OsPassArgs         a       = osCommonArgs(L, frame);
  for(int i = 0; i < sched.count; ++i)
  {
    const OsPassRow& r = sched.rows[i];
    a.pass      = r.pass;
    a.status    = L.status + (size_t)r.set * sWords;
    a.gstatus   = a.status + gOffset;
    a.zStatus   = L.status + (size_t)r.clearFirst * sWords;
    a.zWords    = (uint32_t)r.clearSets * (uint32_t)sWords;
    a.srcPairs  = srcOf[(int)r.src];
    a.dstPairs  = dstOf[(int)r.dst];
    a.digitMode = r.digitMode;
    a.finalMode = r.finalMode;
    osTracePass(trace, r.pass, a);
    launchOsPass(stream, r.variant, maxParts + (r.foldWgs ? kOsFoldWgs : 0u), a);
  }
  osTraceEnd(stream, trace);
}

}  // namespace mgs
