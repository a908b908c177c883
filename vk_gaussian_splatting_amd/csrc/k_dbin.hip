// k_dbin.hip — direct binning for gfx950: the depth-sorted splat list split into per-bin lists without (bin, splat) records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels_common.h"
#include "launchers.h"
#include "tuning.h"

namespace mgs {

// ---- direct binning (<= 256 bins, <= 32 bin columns and <= 32 bin rows) ----------------------------
// With coarse bins the (bin, splat) records never need to exist as sortable pairs: splitting the
// depth-sorted splat list into per-bin lists is ONE stable multi-split, done reduce-then-scan like a
// radix pass whose "digit" is a set (every bin of the splat's rect):
//   k_dbin_count : per chunk of 1024 sorted splats, how many of them touch each bin -> binHist[bin][chunk]
//                  (also re-lays the rects out in sorted order: the only random gather of the stage)
//   k_dbin_scan  : one workgroup per bin: exclusive scan of its row, row total
//   k_dbin_emit  : per chunk, append the ids to every bin list at binBase + rowOffset, in sorted order
// Both per-chunk kernels work on bit matrices: per round of 64 splats, column mask c[bx] = lanes whose rect
// spans column bx (one ballot), row mask r[by] likewise; the lanes hitting bin (bx,by) are c[bx] & r[by].
// Counting is a popcount per bin (lane = bin), emission walks the set bits (lane = bin, appending to its own
// list), so the cost per splat does not depend on how many bins it covers — a splat covering the whole
// screen is one more bit in every mask (per-lane loops over the rect were tried: every round of 64
// depth-neighbours contains some large splat, and the wave pays its trip count).  Gone with the records:
// their 8-byte round trips, the output-partitioned expansion and the whole pair sort.
#ifndef MGS_DB_ROUNDS
#define MGS_DB_ROUNDS 4
#endif
#ifndef MGS_DB_STAGE
#define MGS_DB_STAGE 3072
#endif
constexpr int kDbRounds = MGS_DB_ROUNDS;     // rounds of 64 splats per wave
constexpr int kDbChunk  = 256 * kDbRounds;   // sorted splats per workgroup
constexpr int kDbStage  = MGS_DB_STAGE;      // list entries staged in LDS per chunk so that the appends are coalesced
constexpr int kDbMaxDim = 32;
#ifndef MGS_DB_CNT_MUL
#define MGS_DB_CNT_MUL 1
#endif
constexpr int kDbCntMul = MGS_DB_CNT_MUL;  // chunks counted per workgroup of k_dbin_count
constexpr int kDbMaxSum = 40;  // binsX + binsY of a frame the direct binning takes (each <= 32, product <= 256: 32 + 8)

// v_writelane_b32: a wave-uniform value into ONE lane's register
__device__ __forceinline__ void writeLane(uint32_t& dst, uint32_t value, uint32_t lane)
{
  // one SGPR per VALU op on gfx9: the lane select goes through m0.  Round 6: m0 is an INPUT ("{m0}") that the compiler sets up and
  // tracks itself — rounds 3-5 wrote it inside the asm and listed it as a clobber, which hipcc flags as possibly undefined; this
  // clang has no __builtin_amdgcn_writelane.
  asm volatile("v_writelane_b32 %0, %1, m0" : "+v"(dst) : "s"(value), "{m0}"(lane));
}

// column / row hit masks of one round of 64 rects.  Lane b < binsX ends up holding the mask of column b, lane binsX + b the
// mask of row b (the layout of maskBuf): each ballot is kept by ONE lane through a select — no exec juggling, no branch, one
// LDS write at the end instead of one per ballot.  (A third fewer instructions than lane-0 stores per ballot; the kernel's
// time did not move — 38 us is what 4.2 M random 4-byte gathers of `rect` cost, not what its instructions cost.)
__device__ __forceinline__ uint64_t rectMasks(uint32_t r, bool valid, int binsX, int binsY, uint64_t* s_col, uint64_t* s_row)
{
  const int lane = laneId();
  if(!valid)
    r = 1u;  // x0 = 1 > x1 = 0: no bins
  const uint32_t x0 = r & 255u, y0 = (r >> 8) & 255u, dx = ((r >> 16) & 255u) - x0, dy = (r >> 24) - y0;
  const bool     ok = (int)dx >= 0 && (int)dy >= 0;
  const uint32_t ux = ok ? dx : 0u, nx0 = ok ? x0 : 0xFFFFu;  // rejected: b - nx0 wraps far above ux
  // (v_writelane: the ballot is a scalar pair, lane b's registers take it directly — no compare, no select)
  uint32_t mlo = 0u, mhi = 0u;
  for(int b = 0; b < binsX; ++b)
  {
    const uint64_t m = __ballot((uint32_t)b - nx0 <= ux);
    writeLane(mlo, (uint32_t)m, (uint32_t)b);
    writeLane(mhi, (uint32_t)(m >> 32), (uint32_t)b);
  }
  for(int b = 0; b < binsY; ++b)
  {
    const uint64_t m = __ballot((uint32_t)b - y0 <= dy);
    writeLane(mlo, (uint32_t)m, (uint32_t)(binsX + b));
    writeLane(mhi, (uint32_t)(m >> 32), (uint32_t)(binsX + b));
  }
  const uint64_t mine = ((uint64_t)mhi << 32) | mlo;
  if(lane < binsX)
    s_col[lane] = mine;
  else if(lane < binsX + binsY)
    s_row[lane - binsX] = mine;
  return mine;
}

// the (up to 4) bins lane `lane` is responsible for: b = lane + 64 j
struct LaneBins
{
  int  bx[4], by[4];
  bool on[4];
};
__device__ __forceinline__ LaneBins laneBins(int binsX, int nb)
{
  LaneBins       L;
  const uint32_t inv = (65536u + (uint32_t)binsX - 1u) / (uint32_t)binsX;  // wave-uniform; (b*inv)>>16 == b/binsX for b < 256, binsX <= 32
#pragma unroll
  for(int j = 0; j < 4; ++j)
  {
    const int b = laneId() + 64 * j;
    L.on[j]     = b < nb;
    const int q = (int)(((uint32_t)b * inv) >> 16);
    L.by[j]     = L.on[j] ? q : 0;
    L.bx[j]     = L.on[j] ? b - q * binsX : 0;
  }
  return L;
}

// The same masks by a bit-matrix transpose (round 5, third session): a lane's rectangle IS a row of the (splat x bin-column / bin-row)
// bit matrix — columns x0..x1 in bits [0, binsX), rows y0..y1 in bits [binsX, binsX + binsY) — and the masks are its columns.
// Five butterfly stages (partner's word by DPP for lane distances 1, 2, 8, by ds_swizzle for 4 and 16; v_alignbit + v_bfi)
// transpose the 32 x 32 blocks of both wave halves at once, one ds_bpermute brings the upper half's word to lane b: ~25 vector
// instructions per round of 64 splats, whatever binsX + binsY is, where the ballots cost (binsX + binsY) x 7 (compare, ballot
// into an SGPR pair, two v_writelane through m0) — 119 at 1080p, 224 at 4K — in one dependent chain.  Needs binsX + binsY <= 32.
struct TransposeConst
{
  uint32_t keep[5];  // the bits a lane keeps at stage k (distance 1 << k): those whose index has bit k like the lane's own
  uint32_t rot[5];   // v_alignbit shift that brings the partner's other bits under the complement of keep
};
__device__ __forceinline__ TransposeConst transposeConst()
{
  TransposeConst C;
  const uint32_t lowMask[5] = {0x55555555u, 0x33333333u, 0x0F0F0F0Fu, 0x00FF00FFu, 0x0000FFFFu};
  const uint32_t lane = (uint32_t)laneId();
#pragma unroll
  for(int k = 0; k < 5; ++k)
  {
    const bool up = (lane >> k) & 1u;
    C.keep[k]     = up ? ~lowMask[k] : lowMask[k];
    C.rot[k]      = up ? (1u << k) : 32u - (1u << k);  // rotate right by d (upper lane) / left by d (lower lane)
  }
  return C;
}
template <int N>
__device__ __forceinline__ void transposeWords(uint32_t (&x)[N], const TransposeConst& C)
{
#define MGS_TR_STAGE(K, PARTNER)                                                                        \
  _Pragma("unroll") for(int i = 0; i < N; ++i)                                                          \
  {                                                                                                     \
    const uint32_t p = (uint32_t)(PARTNER);                                                             \
    const uint32_t r = __builtin_amdgcn_alignbit(p, p, C.rot[K]);                                       \
    x[i]             = (C.keep[K] & x[i]) | (~C.keep[K] & r);                                           \
  }
  MGS_TR_STAGE(0, __builtin_amdgcn_update_dpp(0, (int)x[i], 0xB1, 0xF, 0xF, true))   // quad_perm [1,0,3,2]: lane ^ 1
  MGS_TR_STAGE(1, __builtin_amdgcn_update_dpp(0, (int)x[i], 0x4E, 0xF, 0xF, true))   // quad_perm [2,3,0,1]: lane ^ 2
  MGS_TR_STAGE(2, __builtin_amdgcn_ds_swizzle((int)x[i], (4 << 10) | 0x1F))          // BITMASK_PERM xor 4
  MGS_TR_STAGE(3, __builtin_amdgcn_update_dpp(0, (int)x[i], 0x128, 0xF, 0xF, true))  // row_ror:8 = lane ^ 8 within a row of 16
  MGS_TR_STAGE(4, __builtin_amdgcn_ds_swizzle((int)x[i], (16 << 10) | 0x1F))         // BITMASK_PERM xor 16
#undef MGS_TR_STAGE
}
// a lane's row of the bit matrix: bins columns x0..x1 | bin rows y0..y1 << binsX (empty for an invalid / inverted rectangle)
__device__ __forceinline__ uint32_t rectWord(uint32_t r, bool valid, int binsX, uint32_t colAll, uint32_t rowAll)
{
  const uint32_t x0 = r & 255u, y0 = (r >> 8) & 255u, dx = ((r >> 16) & 255u) - x0, dy = (r >> 24) - y0;
  const bool     ok = valid && (int)dx >= 0 && (int)dy >= 0;
  const uint32_t cb = (((2u << (dx & 31u)) - 1u) << (x0 & 31u)) & colAll;
  const uint32_t rb = (((2u << (dy & 31u)) - 1u) << (y0 & 31u)) & rowAll;
  return ok ? (cb | (rb << binsX)) : 0u;
}

__global__ __launch_bounds__(256) void k_dbin_count(const uint32_t* __restrict__ idsX, const uint32_t* __restrict__ idsY,
                                                    const SortPlan* __restrict__ plan, const uint32_t* __restrict__ rect,
                                                    const uint16_t* __restrict__ sortedCode16, uint64_t* __restrict__ maskBuf,
                                                    uint32_t* __restrict__ binHist, uint32_t pStride, int binsX, int binsY, int transpose)
{
  __shared__ uint64_t s_col[4][kDbMaxDim], s_row[4][kDbMaxDim];
  __shared__ uint64_t s_msk[4][kDbRounds][32];  // transpose path: the rounds' masks, columns then rows (binsX + binsY <= 32)
  __shared__ uint32_t s_cnt[4][256];
  const uint32_t n      = plan->n;
  const uint32_t chunks = (n + kDbChunk - 1) / kDbChunk;
  // a workgroup counts kDbCntMul consecutive chunks (k_dbin_emit's unit stays one chunk): the kernel is a chain of dependent round
  // trips per workgroup (plan -> codes + ids -> the escapes' rectangles -> masks), so with every chunk's loads in flight at once
  // the grid passes through the chip in one residency wave instead of two
  const uint32_t chunk0 = blockIdx.x * (uint32_t)kDbCntMul;
  if(chunk0 >= chunks)
    return;
  const int       t = threadIdx.x, lane = laneId(), w = t >> 6;
  const uint32_t* ids = plan->finalSel ? idsY : idsX;
  uint32_t        r[kDbCntMul][kDbRounds];
  const uint32_t  ride = plan->rideInfo;
  const uint32_t  eW   = (uint32_t)w * (kDbRounds * 64) + (uint32_t)lane;
  if(ride != 0u)
  {  // the rectangles rode through the key sort as codes above the ids and lie in sorted order (kernels_common.h: rideEncode);
    // only the escapes — splats over more than 2 x 2 bins — are looked up by id.  The ids are requested beside the codes
    // (coalesced, 4 B per splat): an escape's rectangle is two dependent trips away, not three
    const uint32_t escape = (1u << (ride >> 8)) - 1u;
    RideDecoder    dec    = rideDecoder(binsX, binsY);
    asm volatile("" : "+s"(dec.i0), "+s"(dec.i1));  // made once: left alone the compiler repeats the uniform divisions per decode
    uint32_t       v[kDbCntMul][kDbRounds], id[kDbCntMul][kDbRounds];
#pragma unroll
    for(int c = 0; c < kDbCntMul; ++c)
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
      {
        const uint32_t e = min((chunk0 + c) * (uint32_t)kDbChunk + eW + i * 64u, n - 1u);
        v[c][i]          = sortedCode16[e];
        id[c][i]         = ids[e];
      }
#pragma unroll
    for(int c = 0; c < kDbCntMul; ++c)
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
        r[c][i] = (v[c][i] == escape) ? rect[id[c][i]] : rideDecode(v[c][i], dec);
    // how many rectangles did NOT fit a code (MgsFrameOut::escape_count: the only rect[id] stores / gathers of the frame): one
    // fire-and-forget atomic per wave on the frame's statistics lines
    uint32_t esc = 0u;
#pragma unroll
    for(int c = 0; c < kDbCntMul; ++c)
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
        esc += (uint32_t)__popcll(__ballot(v[c][i] == escape && (chunk0 + c) * (uint32_t)kDbChunk + eW + i * 64u < n));
    if(lane == 0 && esc != 0u)
      atomicAdd(&frameStatLineFromKeys(plan, blockIdx.x * 4u + (uint32_t)w)->escapes, esc);
  }
  else
  {
    uint32_t id[kDbCntMul][kDbRounds];
#pragma unroll
    for(int c = 0; c < kDbCntMul; ++c)
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
        id[c][i] = ids[min((chunk0 + c) * (uint32_t)kDbChunk + eW + i * 64u, n - 1u)];  // clamped, not predicated: all loads in flight
#pragma unroll
    for(int c = 0; c < kDbCntMul; ++c)
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
        r[c][i] = rect[id[c][i]];  // one random gather per splat: 4.2 M of them run at ~120 G/s (L2-miss sectors), 35 us, wherever
                                   // they are issued (moving them into the sort's final pass was measured twice: +36 us there for -16 us here)
  }
  const int            nb = binsX * binsY, S = binsX + binsY;
  const LaneBins       L  = laneBins(binsX, nb);
  const bool           viaTranspose = S <= 32 && transpose != 0;
  const TransposeConst C  = transposeConst();
#pragma unroll
  for(int c = 0; c < kDbCntMul; ++c)
  {
    const uint32_t chunk = chunk0 + (uint32_t)c;
    if(chunk >= chunks)
      break;
    const uint32_t e0     = chunk * (uint32_t)kDbChunk + eW;
    uint32_t       cnt[4] = {0u, 0u, 0u, 0u};
    // the masks of every round are kept for k_dbin_emit (binsX + binsY words of 8 B per round instead of re-reading 64 rects and
    // redoing the masks): maskBuf[((chunk*4 + wave)*rounds + round)*S + {column masks, row masks}]
    uint64_t* mOut = maskBuf + ((size_t)chunk * 4 + w) * kDbRounds * S;
    if(viaTranspose)
    {  // masks by transpose (above): the four rounds' butterflies are independent and interleave
      const uint32_t colAll = (1u << binsX) - 1u, rowAll = (1u << binsY) - 1u;  // (binsX, binsY <= 31 here)
      uint32_t       x[kDbRounds];
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
        x[i] = rectWord(r[c][i], e0 + i * 64u < n, binsX, colAll, rowAll);
      transposeWords(x, C);
      const int up = ((lane + 32) & 63) << 2;
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
      {
        const uint32_t hi   = (uint32_t)__builtin_amdgcn_ds_bpermute(up, (int)x[i]);  // lane b: the word of lane 32 + b
        const uint64_t mine = ((uint64_t)hi << 32) | x[i];
        if(lane < S)
        {
          s_msk[w][i][lane] = mine;
          mOut[i * S + lane] = mine;
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for(int i = 0; i < kDbRounds; ++i)
#pragma unroll
        for(int j = 0; j < 4; ++j)
          if(j * 64 < nb)
          {
            const uint64_t m = L.on[j] ? (s_msk[w][i][L.bx[j]] & s_msk[w][i][binsX + L.by[j]]) : 0ull;
            cnt[j] += (uint32_t)__popcll(m);
          }
    }
    else
#pragma unroll
    for(int i = 0; i < kDbRounds; ++i)
    {
      const uint64_t mine = rectMasks(r[c][i], e0 + i * 64u < n, binsX, binsY, s_col[w], s_row[w]);
      __builtin_amdgcn_wave_barrier();
      if(lane < S)
        mOut[i * S + lane] = mine;
#pragma unroll
      for(int j = 0; j < 4; ++j)
        if(j * 64 < nb)
        {
          const uint64_t m = L.on[j] ? (s_col[w][L.bx[j]] & s_row[w][L.by[j]]) : 0ull;
          cnt[j] += (uint32_t)__popcll(m);
        }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for(int j = 0; j < 4; ++j)
      s_cnt[w][lane + 64 * j] = cnt[j];
    __syncthreads();
    if(t < nb)
      binHist[(size_t)t * pStride + chunk] = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
    if(c + 1 < kDbCntMul)
      __syncthreads();  // s_cnt (and a wave's s_msk rows) are written again for the next chunk
  }
}

__global__ __launch_bounds__(256) void k_dbin_scan(const SortPlan* __restrict__ plan, uint32_t* __restrict__ binHist,
                                                   uint32_t pStride, uint32_t* __restrict__ binTotal)
{
  __shared__ uint32_t s_tmp[4];
  const int      t      = threadIdx.x;
  const uint32_t n      = plan->n;
  const uint32_t chunks = (n + kDbChunk - 1) / kDbChunk;
  uint32_t*      row    = binHist + (size_t)blockIdx.x * pStride;
  uint32_t       carry  = 0;
  // 16 values per thread: a garden-sized frame's ~4 080 chunks are ONE trip of loads, one block scan, one trip of stores (8 per
  // thread were two dependent rounds of that: the kernel is its latency)
  constexpr int kPer = 16;
  for(uint32_t base = 0; base < chunks; base += 256 * kPer)
  {
    const uint32_t p0 = base + t * kPer;
    uint32_t       v[kPer], sum = 0;
#pragma unroll
    for(int i = 0; i < kPer; ++i)
    {
      v[i] = (p0 + i < chunks) ? row[p0 + i] : 0u;
      sum += v[i];
    }
    uint32_t chunk;
    uint32_t run = carry + blockExclusiveScan256(sum, s_tmp, &chunk);
#pragma unroll
    for(int i = 0; i < kPer; ++i)
    {
      if(p0 + i < chunks)
        row[p0 + i] = run;
      run += v[i];
    }
    carry += chunk;
  }
  if(t == 0)
    binTotal[blockIdx.x] = carry;
}

#ifdef MGS_DB_TRACE  // debug build (tools/db_trace.py): per-workgroup wall-clock stamps (100 MHz) of k_dbin_emit's phases
__device__ uint64_t* g_dbTrace = nullptr;
#define MGS_DB_STAMP(i) if(threadIdx.x == 0) dbt[i] = wall_clock64();
#else
#define MGS_DB_STAMP(i)
#endif
__global__ __launch_bounds__(256) void k_dbin_emit(const uint32_t* __restrict__ idsX, const uint32_t* __restrict__ idsY,
                                                   const SortPlan* __restrict__ plan, const uint64_t* __restrict__ maskBuf,
                                                   const uint32_t* __restrict__ binHist, uint32_t pStride,
                                                   const uint32_t* __restrict__ binTotal, uint32_t* __restrict__ binList,
                                                   uint2* __restrict__ ranges, FrameCounters* __restrict__ ctr,
                                                   uint32_t capacity, int binsX, int binsY, uint32_t* __restrict__ binOrder,
                                                   const uint16_t* __restrict__ sortedCode16, uint32_t* __restrict__ binCost)
{
  // LDS diet (round 5): this kernel's residency is set by its LDS — 32 KB were 5 workgroups per CU, and 3 KB more cost a fifth of
  // them and 9 us (seen by accident) — so: column and row masks share one row of binsX + binsY <= 40 words per (wave, round)
  // (8 -> 5 KB), a staged entry is a 16-bit position + an 8-bit bin in two arrays (12 -> 9 KB), the bin ranking borrows the stage.
  __shared__ uint64_t s_msk[4][kDbRounds][kDbMaxSum];  // masks of every round: columns [0, binsX), rows [binsX, binsX + binsY)
  __shared__ uint32_t s_cnt[4][256];  // per-wave counts, then per-wave write cursors
  __shared__ uint32_t s_ids[kDbChunk];
  __shared__ __attribute__((aligned(16))) uint16_t s_spos[kDbStage];  // staged entry: position inside the chunk ...
  __shared__ uint8_t  s_sbin[kDbStage];                              // ... and its bin
  __shared__ uint32_t s_gdst[256], s_loc[256];
  __shared__ uint32_t s_tmp[4], s_tmp64[2];
  const uint32_t n      = plan->n;
  const uint32_t chunks = (n + kDbChunk - 1) / kDbChunk;
  if(chunks == 0u && blockIdx.x == 0u && (int)threadIdx.x < binsX * binsY)
    ranges[threadIdx.x] = make_uint2(0u, 0u);  // nothing sorted: every list is empty (nobody else writes the ranges)
  if(blockIdx.x >= chunks)
    return;
#ifdef MGS_DB_TRACE
  __shared__ uint64_t dbt[8];
  MGS_DB_STAMP(0)
#endif
  // nearest splats (the end of the list) are the largest: start their chunks first
  const uint32_t  chunk = chunks - 1u - blockIdx.x;
  const int       t = threadIdx.x, lane = laneId(), w = t >> 6;
  const uint32_t* ids = plan->finalSel ? idsY : idsX;
  const uint32_t  wbase = (uint32_t)w * (kDbRounds * 64);
  const uint32_t  e0    = chunk * (uint32_t)kDbChunk + wbase + (uint32_t)lane;
  const int       nb    = binsX * binsY;
  const LaneBins  L     = laneBins(binsX, nb);
  uint32_t        cnt[4] = {0u, 0u, 0u, 0u};
  // where every bin's list starts = exclusive prefix of the bins' totals: the same for every chunk, so one wave does it on the
  // side (four bins per lane, wave scans, no barrier of its own) instead of three block-wide scans per workgroup
  uint32_t bt[4] = {0u, 0u, 0u, 0u};
  if(w == 3)
  {
#pragma unroll
    for(int i = 0; i < 4; ++i)
      bt[i] = (4 * lane + i < nb) ? binTotal[4 * lane + i] : 0u;
  }
  // the splats' own rectangles, where they rode through the key sort as codes (k_dbin_count has the story): lane == splat for the
  // walk below
  const uint32_t ride = plan->rideInfo;
  uint32_t       code[kDbRounds];
#pragma unroll
  for(int i = 0; i < kDbRounds; ++i)
    code[i] = ride != 0u ? (uint32_t)sortedCode16[min(e0 + i * 64u, n - 1u)] : 0u;
  {
    const int       S   = binsX + binsY;
    const uint64_t* mIn = maskBuf + ((size_t)chunk * 4 + w) * kDbRounds * S;
    uint64_t        mk[kDbRounds];
#pragma unroll
    for(int i = 0; i < kDbRounds; ++i)
    {
      s_ids[wbase + i * 64 + lane] = ids[min(e0 + i * 64u, n - 1u)];
      mk[i]                        = (lane < S) ? mIn[i * S + lane] : 0ull;
    }
#pragma unroll
    for(int i = 0; i < kDbRounds; ++i)
      if(lane < S)
      {
        s_msk[w][i][lane] = mk[i];  // (the masks arrive in this order: maskBuf holds columns, then rows)
      }
  }
  __builtin_amdgcn_wave_barrier();
  // pop[j]: the populations of bin lane + 64 j's mask in the wave's rounds, 8 bits each (<= 64) — the cursors advance by them below
  uint32_t pop[4] = {0u, 0u, 0u, 0u};
  static_assert(kDbRounds <= 4, "pop[] packs one byte per round");
#pragma unroll
  for(int i = 0; i < kDbRounds; ++i)
#pragma unroll
    for(int j = 0; j < 4; ++j)
      if(j * 64 < nb)
      {
        const uint64_t m = L.on[j] ? (s_msk[w][i][L.bx[j]] & s_msk[w][i][binsX + L.by[j]]) : 0ull;
        const uint32_t c = (uint32_t)__popcll(m);
        cnt[j] += c;
        pop[j] |= c << (8 * i);
      }
#pragma unroll
  for(int j = 0; j < 4; ++j)
    s_cnt[w][lane + 64 * j] = cnt[j];
  __syncthreads();
  MGS_DB_STAMP(1)

  // thread t == bin t: where this chunk's run starts in the bin's list, and in the LDS stage
  const uint32_t c0 = s_cnt[0][t], c1 = s_cnt[1][t], c2 = s_cnt[2][t], c3 = s_cnt[3][t];
  const uint32_t tot   = (t < nb) ? c0 + c1 + c2 + c3 : 0u;
  uint32_t       P;
  if(w == 3)
  {
    const uint32_t sum4 = bt[0] + bt[1] + bt[2] + bt[3];
    uint32_t       run  = waveInclusiveScan(sum4) - sum4;
#pragma unroll
    for(int i = 0; i < 4; ++i)
    {
      s_gdst[4 * lane + i] = run;  // bin base (consumed below, behind the block scan's barriers)
      run += bt[i];
    }
    // the 64-bit total without 64-bit shuffles: the halves summed separately
    const uint32_t dLo = waveSum((bt[0] & 0xFFFFu) + (bt[1] & 0xFFFFu) + (bt[2] & 0xFFFFu) + (bt[3] & 0xFFFFu));
    const uint32_t dHi = waveSum((bt[0] >> 16) + (bt[1] >> 16) + (bt[2] >> 16) + (bt[3] >> 16));
    if(lane == 0)
    {
      s_tmp64[0] = dLo;
      s_tmp64[1] = dHi;
    }
  }
  const uint32_t local   = blockExclusiveScan256(tot, s_tmp, &P);  // (two barriers: the bases above are visible behind them)
  const uint32_t binBase = s_gdst[t];
  const uint64_t D64     = ((uint64_t)s_tmp64[1] << 16) + s_tmp64[0];
  const bool     wrapped = D64 > 0xFFFFFFFFull;  // bin bases are meaningless: emit nothing, report the overflow
  const bool     staged  = P <= (uint32_t)kDbStage;
  const uint32_t gdst    = binBase + ((t < nb) ? binHist[(size_t)t * pStride + chunk] : 0u);  // (requested here, not at the kernel's head: 256 strided loads beside the ids and masks cost 1.5 us — measured)
  __syncthreads();  // everybody has read its base: s_gdst is overwritten
  s_gdst[t] = gdst;
  s_loc[t]  = local;
  {
    const uint32_t start = staged ? local : gdst;
    s_cnt[0][t] = start;
    s_cnt[1][t] = start + c0;
    s_cnt[2][t] = start + c0 + c1;
    s_cnt[3][t] = start + c0 + c1 + c2;
  }
  if(chunk == 0)
  {
    // longest list first: the compositor hands its workgroups out in this bin order, so the regions with the most
    // to blend start early instead of forming the kernel's tail (binOrder[rank] = bin; ties by bin index)
    // The order: by how long the bin's slowest region took in the PREVIOUS frame of this context (k_composite leaves it in
    // binCost; consumed and cleared here) — the regions that never saturate are the long ones, and they are the same from one
    // frame of a sequence to the next; scheduling only, the frame does not depend on it.  Without a history (first frame, the
    // frame before was not composited by k_composite): longest list first.
    uint32_t*      s_tot = reinterpret_cast<uint32_t*>(s_spos);  // [256] (the stage is filled only after this block)
    const uint32_t btot = (t < nb) ? binTotal[t] : 0u;
    uint32_t       cost = 0u;
    if(t < nb)
    {
      cost       = binCost[t];
      binCost[t] = 0u;
    }
    const bool     history = __syncthreads_or(cost != 0u) != 0;
    const uint32_t sortKey = history ? cost : btot;
    s_tot[t] = sortKey;
    __syncthreads();
    if(t < nb)
    {
      uint32_t rank = 0;
      for(int u = 0; u < nb; ++u)
        rank += (s_tot[u] > sortKey || (s_tot[u] == sortKey && u < t)) ? 1u : 0u;
      binOrder[rank] = (uint32_t)t;
    }
    if(t == 0)
      *binOrderValidOf(binOrder) = 1u;
    if(t < nb)
      ranges[t] = wrapped ? make_uint2(0u, 0u)
                          : make_uint2(min(binBase, capacity), (uint32_t)min((uint64_t)binBase + btot, (uint64_t)capacity));
    if(t == 0)
    {
      ctr->pairCount = (uint32_t)min(D64, (uint64_t)capacity);
      // ... and beside the compositor's statistics (line 0 of the statistics lines), so that ONE small copy
      // tells the host how much of their lists the regions scan: the adaptive bin size's input (api_frame.hip: BinPolicy)
      frameStatLineFromKeys(plan, 0u)->listEntries = (uint32_t)min(D64, (uint64_t)capacity);
      if(D64 > capacity)
        atomicOr(&ctr->errorFlags, kErrPairOverflow);
    }
  }
  __syncthreads();
  MGS_DB_STAMP(2)
  if(wrapped)
    return;

  if(staged && ride != 0u)
  {
    // The rectangles are known per splat: most splats cover 1-4 bins (the coded shapes), so LANE == SPLAT places its few entries
    // directly — position = the bin's cursor + the splats before it in this round's mask of the bin —, and only the splats with
    // larger rectangles (escape code) are found by LANE == BIN walking the bits of its mask.  (Walking every bit that way, below,
    // keeps 2-3 % of the lanes busy: the trip count of a round is the population of its densest bin.)  Cursors live in LDS,
    // advanced by the bin lanes once per round, between two wave barriers.  (Cursor-free — every entry summing the bin's
    // population over the wave's earlier rounds itself — was measured: no faster, the bin lanes run anyway because nearly every
    // wave holds an escape.)
    const uint32_t escape = (1u << (ride >> 8)) - 1u;
    // (round 5, third session: the kernel is bound by VALU issue — 14 M instructions, 26 of its 37 us — so the placement was put on
    //  a diet: a coded splat's two column and two row masks are read once instead of per bin, its rank in a bin's mask is
    //  v_mbcnt_lo / hi instead of and + popcount on both halves, the bin lanes keep their cursors in registers and advance them by
    //  the populations the counting above already found, and a round without escapes does not touch its bin masks again)
    uint32_t run[4];
#pragma unroll
    for(int j = 0; j < 4; ++j)
      run[j] = s_cnt[w][lane + 64 * j];
    RideDecoder dec = rideDecoder(binsX, binsY);
    asm volatile("" : "+s"(dec.i0), "+s"(dec.i1));  // (made once, see k_dbin_count)
    const uint32_t xLast = (uint32_t)binsX - 1u, yLast = (uint32_t)(binsX + binsY) - 1u;
#pragma unroll
    for(int i = 0; i < kDbRounds; ++i)
    {
      const bool     valid = e0 + (uint32_t)i * 64u < n;
      const bool     coded = valid && code[i] != escape;
      const uint32_t idx   = wbase + (uint32_t)i * 64u + (uint32_t)lane;
      if(coded)
      {
        const uint32_t r  = rideDecode(code[i], dec);
        const uint32_t x0 = r & 255u, y0 = (r >> 8) & 255u, dx = ((r >> 16) & 255u) - x0, dy = (r >> 24) - y0;
        const uint64_t cm[2] = {s_msk[w][i][x0], s_msk[w][i][min(x0 + 1u, xLast)]};
        const uint64_t rm[2] = {s_msk[w][i][(uint32_t)binsX + y0], s_msk[w][i][min((uint32_t)binsX + y0 + 1u, yLast)]};
        const uint32_t b0    = y0 * (uint32_t)binsX + x0;
#pragma unroll
        for(uint32_t ky = 0; ky < 2u; ++ky)
#pragma unroll
          for(uint32_t kx = 0; kx < 2u; ++kx)
            if(kx <= dx && ky <= dy)
            {
              const uint32_t b  = b0 + ky * (uint32_t)binsX + kx;
              const uint64_t m  = cm[kx] & rm[ky];
              const uint32_t at = s_cnt[w][b] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
              s_spos[at]        = (uint16_t)idx;
              s_sbin[at]        = (uint8_t)b;
            }
      }
      const uint64_t escM = __ballot(valid && !coded);
      __builtin_amdgcn_wave_barrier();
      // (The escapes one after the other in a SCALAR loop — bin lane b takes escape e iff bit e of its mask is set, one-hot and
      //  below-mask as scalar pairs, no per-lane ctz / 64-bit shifts — was measured: bin 64.6 -> 67.4 us, 4K 91.8 -> 94.5: a round
      //  holds more escapes than its fullest bin takes trips.)
#pragma unroll
      for(int j = 0; j < 4; ++j)
        if(j * 64 < nb)
        {
          if(escM != 0ull)  // wave-uniform
          {
            const uint64_t m    = L.on[j] ? (s_msk[w][i][L.bx[j]] & s_msk[w][i][binsX + L.by[j]]) : 0ull;
            uint64_t       me   = m & escM;
            const uint8_t  btag = (uint8_t)(lane + 64 * j);
            while(__ballot(me != 0ull) != 0ull)
              if(me != 0ull)
              {
                const uint32_t bit = (uint32_t)__builtin_ctzll(me);
                const uint32_t at  = run[j] + (uint32_t)__popcll(m & ((1ull << bit) - 1ull));
                s_spos[at]         = (uint16_t)(wbase + (uint32_t)i * 64u + bit);
                s_sbin[at]         = btag;
                me &= me - 1ull;
              }
          }
          run[j] += (pop[j] >> (8 * i)) & 255u;
          if(L.on[j] && i + 1 < kDbRounds)
            s_cnt[w][lane + 64 * j] = run[j];
        }
      __builtin_amdgcn_wave_barrier();
    }
  }
  else
  // lane == bin: walk the set bits of its mask (low word, then high word), appending to its own list
#pragma unroll
  for(int j = 0; j < 4; ++j)
    if(j * 64 < nb)
    {
      uint32_t       run  = s_cnt[w][lane + 64 * j];
      const uint8_t  btag = (uint8_t)(lane + 64 * j);
      for(int i = 0; i < kDbRounds; ++i)
      {
        const uint64_t m = L.on[j] ? (s_msk[w][i][L.bx[j]] & s_msk[w][i][binsX + L.by[j]]) : 0ull;
#pragma unroll
        for(int h = 0; h < 2; ++h)
        {
          uint32_t       mh  = h ? (uint32_t)(m >> 32) : (uint32_t)m;
          const uint32_t pos0 = wbase + (uint32_t)i * 64u + (uint32_t)h * 32u;
          if(staged)
          {  // no memory read in the loop: the entry is (bin, position), the id is looked up at copy-out
            while(__ballot(mh != 0u) != 0ull)
              if(mh != 0u)
              {
                s_spos[run]   = (uint16_t)(pos0 + (uint32_t)__builtin_ctz(mh));
                s_sbin[run++] = btag;
                mh &= mh - 1u;
              }
          }
          else
          {
            while(__ballot(mh != 0u) != 0ull)
              if(mh != 0u)
              {
                const uint32_t id = s_ids[pos0 + (uint32_t)__builtin_ctz(mh)];
                mh &= mh - 1u;
                if(run < capacity)
                  binList[run] = id;
                ++run;
              }
          }
        }
      }
    }
  if(!staged)
    return;
  __syncthreads();
  MGS_DB_STAMP(3)
  for(uint32_t i = t; i < P; i += 256)
  {
    const uint32_t b   = s_sbin[i];
    const uint32_t dst = s_gdst[b] + (i - s_loc[b]);
    if(dst < capacity)
      binList[dst] = s_ids[s_spos[i]];
  }
#ifdef MGS_DB_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  MGS_DB_STAMP(4)
  if(t == 0 && g_dbTrace)
  {
    uint64_t* o = g_dbTrace + (size_t)blockIdx.x * 8;
    for(int i = 0; i < 5; ++i) o[i] = dbt[i];
    o[5] = P;
  }
#endif
}

// ---------------------------------------------------------------------------------------------
bool directBinningSupported(int binsX, int binsY)
{
  return binsX <= kDbMaxDim && binsY <= kDbMaxDim && binsX * binsY <= 256 && binsX + binsY <= kDbMaxSum;
}

void launchDirectBinning(hipStream_t stream, const DirectBinLaunch& L)
{
  const uint32_t maxChunks = (L.maxSplats + kDbChunk - 1) / kDbChunk;
  if(maxChunks == 0)
    return;
  // MGS_DB_TRANSPOSE=0: the rounds' masks by ballots everywhere (the masks are the same; the transpose path is the default)
  hipLaunchKernelGGL(k_dbin_count, dim3((maxChunks + kDbCntMul - 1) / kDbCntMul), dim3(256), 0, stream, L.idsX, L.idsY, L.planKeys, L.rect, L.sortedCode16,
                     L.maskBuf, L.binHist, L.pStride, L.binsX, L.binsY, tuning().dbTranspose);
  hipLaunchKernelGGL(k_dbin_scan, dim3(L.binsX * L.binsY), dim3(256), 0, stream, L.planKeys, L.binHist, L.pStride, L.tables->binTotal);
#ifdef MGS_DB_TRACE
  static uint64_t* traceBuf = nullptr;
  const char*      tracePath = std::getenv("MGS_DB_TRACE_FILE");
  if(tracePath)
  {
    if(!traceBuf)
    {
      (void)hipMalloc(&traceBuf, (size_t)maxChunks * 64);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbTrace), &traceBuf, sizeof(traceBuf));
    }
    (void)hipMemsetAsync(traceBuf, 0, (size_t)maxChunks * 64, stream);
  }
#endif
  hipLaunchKernelGGL(k_dbin_emit, dim3(maxChunks), dim3(256), 0, stream, L.idsX, L.idsY, L.planKeys, L.maskBuf, L.binHist, L.pStride,
                     L.tables->binTotal, L.binList, L.ranges, L.ctr, L.capacity, L.binsX, L.binsY, L.tables->binOrder, L.sortedCode16, L.binCost);
#ifdef MGS_DB_TRACE
  if(tracePath)
  {
    (void)hipStreamSynchronize(stream);
    std::vector<uint64_t> h((size_t)maxChunks * 8);
    (void)hipMemcpy(h.data(), traceBuf, h.size() * 8, hipMemcpyDeviceToHost);
    if(FILE* fp = std::fopen(tracePath, "wb"))
    {
      std::fwrite(h.data(), 8, h.size(), fp);
      std::fclose(fp);
    }
  }
#endif
}

}  // namespace mgs
