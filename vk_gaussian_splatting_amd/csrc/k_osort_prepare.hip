// k_osort_prepare.hip — the key sort before its passes: the digit totals every pass needs up front (osort_common.h has the
// sort's outline).  k_os_hist counts them for the stand-alone sort; k_os_prepare takes them, and the tables of the virtual
// pass 0, from what the project kernels left (slot_emit.h); k_os_plan_clear zeroes the plan of a stand-alone sort.
#include <algorithm>

#include "osort_common.h"

namespace mgs {

// ---------------------------------------------------------------------------------------------------------------------
// (a) uniform input only (the stand-alone sort API): digit totals of all four passes in one read of the keys
__global__ __launch_bounds__(256) void k_os_hist(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ nPtr, OsPlan* __restrict__ plan)
{
  __shared__ uint32_t s_h[4][256];
  const int      t = threadIdx.x;
  const uint32_t n = *nPtr;
  for(int q = 0; q < 4; ++q)
    s_h[q][t] = 0u;
  __syncthreads();
  for(uint64_t i0 = (uint64_t)blockIdx.x * 2048u; i0 < n; i0 += (uint64_t)gridDim.x * 2048u)
  {
    uint32_t kk[8];
#pragma unroll
    for(int u = 0; u < 8; ++u)
    {
      const uint64_t i = i0 + (uint64_t)u * 256u + (uint64_t)t;
      kk[u]            = keys[i < n ? i : (uint64_t)n - 1u];  // clamped, not predicated
    }
#pragma unroll
    for(int u = 0; u < 8; ++u)
      if(i0 + (uint64_t)u * 256u + (uint64_t)t < n)
      {
#pragma unroll
        for(int q = 0; q < 4; ++q)
          atomicAdd(&s_h[q][(kk[u] >> (8 * q)) & 255u], 1u);
      }
  }
  __syncthreads();
#pragma unroll
  for(int q = 0; q < 4; ++q)
    if(s_h[q][t])
      atomicAdd(&plan->total[q][t], s_h[q][t]);
}

#ifdef MGS_OS_TRACE
__device__ uint64_t* g_osPrepTrace = nullptr;  // [reduce workgroup][8]
void osPrepTraceBind(uint64_t* buf) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_osPrepTrace), &buf, sizeof(buf)); }
#endif
// ---------------------------------------------------------------------------------------------------------------------
// (b) prepare: the digit totals of all passes and the tables of the virtual pass 0, from what the producer left.
// Grid: reduce workgroups of 1024 threads, one per CHUNK of 32 slots.  A reduce workgroup
//   * turns its slots' digit-0 group counts (slot_emit.h) into the chunk's part of the virtual pass 0: per digit-0 value d the
//     chunk's total (chunkSum[chunk][d]) and, per slot, how many pairs of value d the chunk's earlier slots hold together with
//     where the slot's group of d starts inside the slot (runTab[d][slot], 16 + 16 bits) — and adds the totals to
//     plan->total[0];  the pair that a stable pass on bits 0-7 would put at position x of its output is then found from
//     D[d] (scan of the totals), the prefix of chunkSum[.][d] and one runTab row segment, all of which the sort's first
//     kernel reads for just the part of the order it owns (k_os_pass<3>).  Nothing here waits for another workgroup;
//   * sums its slots' histograms of key bits 8-15 into plan->total[1] (<= 256 atomics, one per non-empty bin);
//   * folds its slots' key >> 16 records (slot_emit.h: one 32-word record per producer wave: counts of the values lo..lo+24)
//     in an LDS table and adds each occurring value ONCE to the 64 K-entry count table.  The producers do not touch that
//     table themselves: thousands of partitions hold the same handful of values, and that many atomics on a few addresses
//     serialise (measured: 0.13 -> 0.55 ms for k_project).  Partitions that span more than 24 values (a cell around the
//     camera) are the exception: their keys are spread over many addresses and were added one by one.
// Turning the count table into what the upper passes sort on (at most 256 values within a span < 4096 -> pass 2 sorts on their
// rank; otherwise plain digits for passes 2 and 3) is not done here: the table is complete when this kernel ends and its fold is
// needed by the second sort kernel only, so workgroups beyond the partitions of the FIRST sort kernel do it (foldTop16,
// k_osort_pass.hip).
// One more workgroup (the last of the grid) sums the slots' counts — the frame's number of sorted pairs — and leaves the project
// kernel's dispatch order for the NEXT frame, fullest slot first.
__global__ __launch_bounds__(1024) void k_os_prepare(const uint32_t* __restrict__ slotHist, const uint32_t* __restrict__ top16Rec, uint32_t prjParts,
                                                     uint32_t* __restrict__ top16Count, OsPlan* __restrict__ plan, const uint32_t* __restrict__ nPtr,
                                                     uint32_t reduceWgs, const uint32_t* __restrict__ slotCount,
                                                     uint32_t* __restrict__ chunkSum, uint32_t* __restrict__ runTab,
                                                     uint32_t* __restrict__ nOut, uint32_t* __restrict__ orderOut)
{
  const int t = threadIdx.x, lane = laneId(), w = t >> 6;
#ifdef MGS_OS_TRACE
  __shared__ uint64_t trc[8];
  if(t < 8) trc[t] = 0;
  MGS_OS_STAMP(0)
#endif
  if(slotHist == nullptr)
  {  // uniform input (stand-alone sort): k_os_hist has the totals
    if(blockIdx.x == 0 && t == 0)
      plan->n = *nPtr;
    return;
  }
  __shared__ uint32_t s_tab[2048];
  if(blockIdx.x == reduceWgs)
  {
    __shared__ uint32_t s_scan[16];
    uint32_t sum = 0;
    for(uint32_t q = t; q < prjParts; q += 1024u)
      sum += slotCount[q];
    const uint32_t inc = waveInclusiveScan(sum);
    if(lane == 63)
      s_scan[w] = inc;
    __syncthreads();
    if(t == 0)
    {
      uint32_t total = 0;
      for(int q = 0; q < 16; ++q)
        total += s_scan[q];
      plan->n = total;
      *nOut   = total;
    }
    if(orderOut != nullptr)
    {  // The NEXT frame's dispatch order of the project kernel's partitions: fullest slot first.  That kernel runs 1.85
       // residency waves of workgroups that take 19 .. 80 us each; in storage order a third of its span is a draining tail
       // (profiles/r4_z_prj_trace.log).  A partition's cost follows its survivor count, which hardly changes from one frame of
       // a sequence to the next.  Scheduling only: slots are per partition, the frame does not depend on the order.  A counting
       // sort on count / 64 (33 classes), the order inside a class is whatever the atomics give.
      __shared__ uint32_t s_cls[40];
      if(t < 40)
        s_cls[t] = 0u;
      __syncthreads();
      for(uint32_t q = t; q < prjParts; q += 1024u)
        atomicAdd(&s_cls[32u - min(slotCount[q] >> 6, 32u)], 1u);
      __syncthreads();
      if(t == 0)
      {
        uint32_t run = 0;
        for(int c = 0; c < 33; ++c)
        {
          const uint32_t v = s_cls[c];
          s_cls[c]         = run;
          run += v;
        }
      }
      __syncthreads();
      for(uint32_t q = t; q < prjParts; q += 1024u)
        orderOut[atomicAdd(&s_cls[32u - min(slotCount[q] >> 6, 32u)], 1u)] = q;
    }
    return;
  }
  if(blockIdx.x >= reduceWgs)
    return;
  __shared__ uint32_t s_part[512];
  __shared__ uint32_t s_lo, s_hi;
  const uint32_t slot0 = blockIdx.x * 32u;
  // the records' loads go out with the histograms' (one round trip instead of three): thread t owns words j0 .. j0 + 3 of
  // record t / 8, and reads that record's header itself
  const uint32_t recR = (uint32_t)t >> 3, recJ0 = ((uint32_t)t & 7u) * 4u, recSlot = slot0 + recR / 4u;
  uint32_t       recHdr = 0xFFFFFFFFu;
  uint4          recC   = make_uint4(0u, 0u, 0u, 0u);
  if(recSlot < prjParts)
  {
    const uint32_t* rp = &top16Rec[((size_t)recSlot * 4u + (recR & 3u)) * 32u];
    recHdr             = rp[31];
    recC               = *reinterpret_cast<const uint4*>(rp + recJ0);
  }
  {  // the slots' rows: thread = (packed column c: digits 2 c and 2 c + 1, group j of four consecutive slots)
    __shared__ uint32_t s_grp[8][256];
    const uint32_t c = (uint32_t)t & 127u, j = (uint32_t)t >> 7;
    uint32_t       w0[4], w1[4], w2[4];
#pragma unroll
    for(int i = 0; i < 4; ++i)
    {
      const uint32_t  sl  = slot0 + 4u * j + (uint32_t)i;
      const uint32_t* row = slotHist + (size_t)min(sl, prjParts - 1u) * kSlotHistWords;
      const bool      ok  = sl < prjParts;
      w0[i]               = row[c];
      w1[i]               = row[128u + c];
      w2[i]               = row[256u + c];
      if(!ok)
        w0[i] = w1[i] = w2[i] = 0u;
    }
    s_tab[t]         = 0u;
    s_tab[t + 1024u] = 0u;
    if(t < 512)
      s_part[t] = 0u;
    if(t == 0)
    {
      s_lo = 0xFFFFu;
      s_hi = 0u;
    }
    uint32_t pLo[4], pHi[4], sLo = 0, sHi = 0, lo1 = 0, hi1 = 0;
#pragma unroll
    for(int i = 0; i < 4; ++i)
    {
      pLo[i] = sLo;
      pHi[i] = sHi;
      sLo += w0[i] & 0xFFFFu;
      sHi += w0[i] >> 16;
      lo1 += w1[i] & 0xFFFFu;
      hi1 += w1[i] >> 16;
    }
    s_grp[j][2u * c]      = sLo;
    s_grp[j][2u * c + 1u] = sHi;
    __syncthreads();
    if(lo1)
      atomicAdd(&s_part[256u + 2u * c], lo1);
    if(hi1)
      atomicAdd(&s_part[256u + 2u * c + 1u], hi1);
    uint32_t bLo = 0, bHi = 0;
#pragma unroll
    for(uint32_t q = 0; q < 7u; ++q)
      if(q < j)
      {
        bLo += s_grp[q][2u * c];
        bHi += s_grp[q][2u * c + 1u];
      }
    if(j == 7u)
    {  // the chunk's totals of digits 2 c and 2 c + 1
      const uint32_t tLo = bLo + sLo, tHi = bHi + sHi;
      *reinterpret_cast<uint2*>(&chunkSum[(size_t)blockIdx.x * 256u + 2u * c]) = make_uint2(tLo, tHi);
      if(tLo)
        atomicAdd(&plan->total[0][2u * c], tLo);
      if(tHi)
        atomicAdd(&plan->total[0][2u * c + 1u], tHi);
    }
    // (pairs of the value in the chunk's earlier slots: <= 31 x 2048, 16 bits) | (start of the value's group in its slot: <= 2048) << 16
    const size_t spad = (size_t)reduceWgs * kOsChunk, col = (size_t)slot0 + 4u * j;
    *reinterpret_cast<uint4*>(&runTab[(size_t)(2u * c) * spad + col]) =
        make_uint4((bLo + pLo[0]) | (w2[0] << 16), (bLo + pLo[1]) | (w2[1] << 16), (bLo + pLo[2]) | (w2[2] << 16), (bLo + pLo[3]) | (w2[3] << 16));
    *reinterpret_cast<uint4*>(&runTab[(size_t)(2u * c + 1u) * spad + col]) =
        make_uint4((bHi + pHi[0]) | (w2[0] & 0xFFFF0000u), (bHi + pHi[1]) | (w2[1] & 0xFFFF0000u), (bHi + pHi[2]) | (w2[2] & 0xFFFF0000u),
                   (bHi + pHi[3]) | (w2[3] & 0xFFFF0000u));
    __syncthreads();
    if(t >= 256 && t < 512 && s_part[t])
      atomicAdd(&plan->total[1][t & 255u], s_part[t]);
  }
  MGS_OS_STAMP(1)
  // key >> 16 records of the 32 slots x 4 producer waves: header word 31 = lo | span << 16 (0xFFFFFFFF: nothing to fold)
  if((t & 7) == 0 && recHdr != 0xFFFFFFFFu)
  {
    atomicMin(&s_lo, recHdr & 0xFFFFu);
    atomicMax(&s_hi, (recHdr & 0xFFFFu) + (recHdr >> 16));
  }
  __syncthreads();
  if(recHdr != 0xFFFFFFFFu && recJ0 <= (recHdr >> 16))
  {
    const uint32_t cv[4] = {recC.x, recC.y, recC.z, recC.w};
#pragma unroll
    for(int j = 0; j < 4; ++j)
      if(recJ0 + j <= (recHdr >> 16) && cv[j])
      {
        const uint32_t v = (recHdr & 0xFFFFu) + recJ0 + j, idx = v - s_lo;
        if(idx < 2048u)
          atomicAdd(&s_tab[idx], cv[j]);
        else
          atomicAdd(&top16Count[v], cv[j]);
      }
  }
  __syncthreads();
  for(uint32_t b = t; b < 2048u; b += 1024u)
    if(s_tab[b])
      atomicAdd(&top16Count[s_lo + b], s_tab[b]);
  if(t == 0 && s_hi >= s_lo)  // (s_lo = 0xFFFF, s_hi = 0 is the empty state: 0xFFFF itself is a legal value of key >> 16)
  {  // occurring range over all workgroups (the plan is zeroed per sort: both as maxima)
    atomicMax(&plan->top16MinInv, 0x10000u - s_lo);
    atomicMax(&plan->top16MaxP1, s_hi + 1u);
  }
#ifdef MGS_OS_TRACE
  MGS_OS_STAMP(2)
  if(t == 0 && g_osPrepTrace)
    for(int i = 0; i < 8; ++i) g_osPrepTrace[(size_t)blockIdx.x * 8 + i] = trc[i];
#endif
}

// small state clear for the stand-alone sort (inside a frame the frame-init kernel zeroes the plan)
__global__ void k_os_plan_clear(OsPlan* plan)
{
  uint32_t* w = reinterpret_cast<uint32_t*>(plan);
  for(uint32_t i = threadIdx.x; i < sizeof(OsPlan) / 4; i += blockDim.x)
    w[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
void launchOsSortClearPlan(hipStream_t stream, OsPlan* plan)
{
  hipLaunchKernelGGL(k_os_plan_clear, dim3(1), dim3(256), 0, stream, plan);
}

void launchOsHist(hipStream_t stream, const OsLaunch& L)
{
  hipLaunchKernelGGL(k_os_hist, dim3(std::min<uint32_t>((L.maxElems + 2047u) / 2048u, 1024u)), dim3(256), 0, stream, L.keys0, L.nPtr, L.plan);
}

// A frame's sort (L.pairs0): one reduce workgroup per chunk of slots and the one that counts.  Stand-alone: that one alone,
// which copies the element count into the plan.
void launchOsPrepare(hipStream_t stream, const OsLaunch& L)
{
  const bool     frame     = L.pairs0 != nullptr;
  const uint32_t reduceWgs = frame ? osSortChunks(L.prjParts) : 0u;
  hipLaunchKernelGGL(k_os_prepare, dim3(reduceWgs + 1u), dim3(1024), 0, stream, frame ? L.slotHist : nullptr, L.top16Rec, L.prjParts,
                     L.top16Count, L.plan, L.nPtr, reduceWgs, L.slotCount, L.chunkSum, L.runTab, L.nOut, L.prjOrderOut);
}

}  // namespace mgs
