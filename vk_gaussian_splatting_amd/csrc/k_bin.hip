// k_bin.hip — the record + pair-sort binning for gfx950: frames with more than 256 bins (k_dbin.hip bins the others directly).
//
// The reference has no counterpart for binning: it emits one quad per splat and lets the
// fixed-function rasterizer + ROP blend in primitive (= sorted) order
// (shaders/threedgs_raster.frag.slang:223-309, src/gaussian_splatting.cpp:2066-2087).
// Contract kept here: every pixel centre inside the splat's ellipse
// (A <= 8) with alpha > 1/255 is blended, in the global depth order produced by the sort (k_composite.hip walks the lists).
#include "kernels_common.h"
#include "launchers.h"

namespace mgs {

constexpr int kBinThreads = 256;
constexpr int kBinItems   = 8;
constexpr int kBinPart    = kBinThreads * kBinItems;  // 2048 sorted splats per workgroup

__device__ __forceinline__ uint32_t rectTiles(uint32_t r)
{
  const uint32_t x0 = r & 255u, y0 = (r >> 8) & 255u, x1 = (r >> 16) & 255u, y1 = r >> 24;
  return (x1 - x0 + 1u) * (y1 - y0 + 1u);
}

// ---- frame init of the record path: empty tile ranges (counters and sort plans arrive zeroed with the frame's upload) ----
__global__ void k_frame_init(uint2* ranges, uint32_t nTiles)
{
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
  for(uint32_t i = gid; i < nTiles; i += gsz)
    ranges[i] = make_uint2(0u, 0u);
}

// ---- binning, record path (frames with more than 256 bins; the default is the direct multi-split below) ----
// Contract: per bin, the splats whose footprint box overlaps it, in global depth order.
// Records (bin id, global id) are emitted in sorted-splat order; a STABLE sort by bin id then keeps
// every bin's list depth-ordered.  The expansion is partitioned by OUTPUT range, not by splat: the
// nearest splats are the largest on screen and sit together at the end of the sorted list, so a
// splat-partitioned expansion leaves a ~1 ms tail on a handful of workgroups (profiles/r1_a).
//   k_bin_count   : tile count of every sorted splat (+ its rect, re-laid out in sorted order) -> block sums
//   k_bin_scan    : exclusive scan of the block sums, total D
//   k_bin_offsets : per-splat exclusive offsets; marks, for every 2048-record output chunk, the sorted
//                   splat that contains the chunk's first record
//   k_bin_expand  : one workgroup per output chunk, balanced and fully coalesced writes
constexpr int kChunk = 2048;  // output records per expand workgroup

__global__ __launch_bounds__(kBinThreads) void k_bin_count(const uint32_t* __restrict__ idsX, const uint32_t* __restrict__ idsY,
                                                           const SortPlan* __restrict__ plan, const uint32_t* __restrict__ rect,
                                                           uint32_t* __restrict__ sortedRect, uint32_t* __restrict__ blockCount,
                                                           int gather)
{
  __shared__ uint32_t s_tmp[4];
  const uint32_t      n     = plan->n;
  const uint32_t      parts = (n + kBinPart - 1) / kBinPart;
  if(blockIdx.x >= parts)
    return;
  const uint32_t* ids = plan->finalSel ? idsY : idsX;
  uint32_t        sum = 0;
#pragma unroll
  for(int i = 0; i < kBinItems; ++i)
  {
    const uint32_t e = blockIdx.x * kBinPart + i * kBinThreads + threadIdx.x;
    if(e < n)
    {
      uint32_t r;
      if(gather)  // CPU-sort mode: nothing has produced sortedRect yet
      {
        r             = rect[ids[e]];
        sortedRect[e] = r;
      }
      else  // GPU sort: the last radix pass wrote the rects in sorted order (fused gather)
        r = sortedRect[e];
      sum += rectTiles(r);
    }
  }
  sum = waveSum(sum);
  if(laneId() == 0)
    s_tmp[threadIdx.x >> 6] = sum;
  __syncthreads();
  if(threadIdx.x == 0)
    blockCount[blockIdx.x] = s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
}

__global__ __launch_bounds__(256) void k_bin_scan(const SortPlan* __restrict__ plan, uint32_t* __restrict__ blockCount,
                                                  FrameCounters* __restrict__ ctr, uint32_t capacity)
{
  __shared__ uint32_t s_tmp[4];
  const uint32_t      n     = plan->n;
  const uint32_t      parts = (n + kBinPart - 1) / kBinPart;
  uint64_t            carry = 0;
  for(uint32_t base = 0; base < parts; base += 256)
  {
    const uint32_t p = base + threadIdx.x;
    const uint32_t v = (p < parts) ? blockCount[p] : 0u;
    uint32_t       chunk;
    const uint32_t ex = blockExclusiveScan256(v, s_tmp, &chunk);
    if(p < parts)
      blockCount[p] = (uint32_t)min(carry + ex, (uint64_t)0xFFFFFFFFull);
    carry += chunk;
  }
  if(threadIdx.x == 0)
  {
    if(carry > capacity)
    {
      atomicOr(&ctr->errorFlags, kErrPairOverflow);
      carry = capacity;
    }
    ctr->pairCount = (uint32_t)carry;
  }
}

__global__ __launch_bounds__(kBinThreads) void k_bin_offsets(const SortPlan* __restrict__ plan, const uint32_t* __restrict__ sortedRect,
                                                             const uint32_t* __restrict__ blockOffset,
                                                             uint32_t* __restrict__ splatOffset, uint32_t* __restrict__ chunkStart,
                                                             uint32_t maxChunks)
{
  __shared__ uint32_t s_tmp[4];
  const uint32_t      n     = plan->n;
  const uint32_t      parts = (n + kBinPart - 1) / kBinPart;
  if(blockIdx.x >= parts)
    return;
  // thread t owns the 8 consecutive sorted entries [base + 8t, base + 8t + 8)
  const uint32_t e0 = blockIdx.x * kBinPart + threadIdx.x * kBinItems;
  uint32_t       cnt[kBinItems], sum = 0;
#pragma unroll
  for(int i = 0; i < kBinItems; ++i)
  {
    cnt[i] = (e0 + i < n) ? rectTiles(sortedRect[e0 + i]) : 0u;
    sum += cnt[i];
  }
  uint32_t total;
  uint32_t run = blockOffset[blockIdx.x] + blockExclusiveScan256(sum, s_tmp, &total);
#pragma unroll
  for(int i = 0; i < kBinItems; ++i)
  {
    if(e0 + i < n)
    {
      splatOffset[e0 + i] = run;
      if(cnt[i])
      {  // every multiple of kChunk inside [run, run+cnt) starts an output chunk inside this splat
        const uint32_t first = (run + kChunk - 1) / kChunk, last = (run + cnt[i] - 1) / kChunk;
        for(uint32_t m = first; m <= last && m < maxChunks; ++m)
          chunkStart[m] = e0 + i;
      }
    }
    run += cnt[i];
  }
}

__global__ __launch_bounds__(kBinThreads) void k_bin_expand(const uint32_t* __restrict__ idsX, const uint32_t* __restrict__ idsY,
                                                            const SortPlan* __restrict__ plan, const FrameCounters* __restrict__ ctr,
                                                            const uint32_t* __restrict__ sortedRect,
                                                            const uint32_t* __restrict__ splatOffset,
                                                            const uint32_t* __restrict__ chunkStart, uint32_t* __restrict__ pairKey,
                                                            uint32_t* __restrict__ pairVal, int binsX)
{
  constexpr int       kWin = 2048;
  __shared__ uint32_t s_off[kWin + 1];
  __shared__ uint32_t s_rect[kWin];
  __shared__ uint32_t s_gid[kWin];
  const uint32_t      D = ctr->pairCount;  // already clamped to the capacity
  const uint32_t      n = plan->n;
  const uint32_t      o0 = blockIdx.x * (uint32_t)kChunk;
  if(o0 >= D)
    return;
  const uint32_t  o1  = min(o0 + (uint32_t)kChunk, D);
  const uint32_t* ids = plan->finalSel ? idsY : idsX;
  const int       t   = threadIdx.x;
  const uint32_t  s0  = chunkStart[blockIdx.x];
  // the splat holding the next chunk's first record may also hold the tail of this chunk
  const uint32_t s1 = (o1 < D) ? chunkStart[blockIdx.x + 1] : (n - 1);
  for(uint32_t w0 = s0; w0 <= s1; w0 += kWin)
  {
    const uint32_t wn = min((uint32_t)kWin, s1 + 1 - w0);
    __syncthreads();
    for(uint32_t i = t; i < wn; i += kBinThreads)
    {
      s_off[i]  = splatOffset[w0 + i];
      s_rect[i] = sortedRect[w0 + i];
      s_gid[i]  = ids[w0 + i];
    }
    if(t == 0)
      s_off[wn] = (w0 + wn < n) ? splatOffset[w0 + wn] : 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t lo = max(o0, s_off[0]), hi = min(o1, s_off[wn]);
    for(uint32_t o = lo + t; o < hi; o += kBinThreads)
    {
      // last window entry whose offset <= o
      uint32_t a = 0, b = wn;
      while(b - a > 1)
      {
        const uint32_t mid = (a + b) >> 1;
        if(s_off[mid] <= o)
          a = mid;
        else
          b = mid;
      }
      const uint32_t r  = s_rect[a];
      const uint32_t x0 = r & 255u, y0 = (r >> 8) & 255u, x1 = (r >> 16) & 255u;
      const uint32_t wd = x1 - x0 + 1u;
      const uint32_t k  = o - s_off[a];
      pairKey[o]        = (y0 + k / wd) * (uint32_t)binsX + (x0 + k % wd);
      pairVal[o]        = s_gid[a];
    }
  }
}

// ---- tile ranges over the tile-sorted pair list ------------------------------------------------
// 4 keys per thread (one 16-byte load) + the two neighbours.
__global__ void k_tile_ranges(const uint32_t* __restrict__ keyX, const uint32_t* __restrict__ keyY,
                              const SortPlan* __restrict__ plan, uint2* __restrict__ ranges)
{
  const uint32_t  n    = plan->n;
  const uint32_t* keys = plan->finalSel ? keyY : keyX;
  const uint32_t  n4   = (n + 3u) >> 2;
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x)
  {
    const uint32_t j = i << 2;
    uint32_t       k[6];
    if(j + 4 <= n)
    {
      const uint4 v = *reinterpret_cast<const uint4*>(keys + j);
      k[1] = v.x; k[2] = v.y; k[3] = v.z; k[4] = v.w;
    }
    else
    {
#pragma unroll
      for(int q = 0; q < 4; ++q)
        k[1 + q] = (j + q < n) ? keys[j + q] : 0xFFFFFFFFu;
    }
    k[0] = (j > 0) ? keys[j - 1] : 0xFFFFFFFFu;
    k[5] = (j + 4 < n) ? keys[j + 4] : 0xFFFFFFFFu;
#pragma unroll
    for(int q = 0; q < 4; ++q)
    {
      if(j + q < n)
      {
        if(k[q] != k[q + 1] || (j + q) == 0)
          ranges[k[q + 1]].x = j + q;
        if(k[q + 2] != k[q + 1] || (j + q) == n - 1)
          ranges[k[q + 1]].y = j + q + 1;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
void launchFrameInit(hipStream_t stream, uint2* ranges, uint32_t nTiles)
{
  const uint32_t blocks = (nTiles + 255u) / 256u < 4u ? 4u : min((nTiles + 255u) / 256u, 256u);
  hipLaunchKernelGGL(k_frame_init, dim3(blocks), dim3(256), 0, stream, ranges, nTiles);
}

static_assert(kBinPart == (int)kPart, "the host sizes the binning's grid by kPart");
void launchBinning(hipStream_t stream, const BinLaunch& L)
{
  if(L.maxBlocks == 0)
    return;
  hipLaunchKernelGGL(k_bin_count, dim3(L.maxBlocks), dim3(kBinThreads), 0, stream, L.idsX, L.idsY, L.planKeys, L.rect, L.sortedRect,
                     L.blockCount, L.gatherRects ? 1 : 0);
  hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(256), 0, stream, L.planKeys, L.blockCount, L.ctr, L.capacity);
  const uint32_t chunks = (L.capacity + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(k_bin_offsets, dim3(L.maxBlocks), dim3(kBinThreads), 0, stream, L.planKeys, L.sortedRect, L.blockCount,
                     L.splatOffset, L.chunkStart, chunks + 1);
  hipLaunchKernelGGL(k_bin_expand, dim3(chunks), dim3(kBinThreads), 0, stream, L.idsX, L.idsY, L.planKeys, L.ctr, L.sortedRect,
                     L.splatOffset, L.chunkStart, L.pairKey, L.pairVal, L.binsX);
}

void launchTileRanges(hipStream_t stream, const uint32_t* keyX, const uint32_t* keyY, const SortPlan* planPairs,
                      uint2* ranges)
{
  hipLaunchKernelGGL(k_tile_ranges, dim3(4096), dim3(256), 0, stream, keyX, keyY, planPairs, ranges);
}

}  // namespace mgs
