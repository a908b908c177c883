// k_composite.hip — per-pixel compositing of the 3DGS pipeline for gfx950.
//
// The reference has no counterpart for binning: it emits one quad per splat and lets the
// fixed-function rasterizer + ROP blend in primitive (= sorted) order
// (shaders/threedgs_raster.frag.slang:223-309, src/gaussian_splatting.cpp:2066-2087).
// Contract kept here: every pixel centre inside the splat's ellipse
// (A <= 8) with alpha > 1/255 is blended, in the global depth order produced by the sort.
// The reference blends back-to-front ("over"); we walk the same order from the other end and
// accumulate front-to-back with transmittance, which is the same sum in exact arithmetic:
//   C = sum_i c_i a_i prod_{j nearer than i} (1 - a_j).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "composite_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "sh_eval.h"
#include "surface_normal.h"

namespace mgs {

// ---- compositing ------------------------------------------------------------------------------
// One workgroup per 32x16-pixel region (two 16x16 tiles side by side), one wave per 16x8 quarter, TWO
// pixels per lane (x and x+8): the per-fragment arithmetic then runs on gfx950's packed-fp32 pipe
// (v_pk_fma_f32 & co, two pixels per instruction) with the splat's parameters broadcast through op_sel.
// Lists exist per BIN (a block of tiles, e.g. 256x128 px), not per tile: duplicating every splat into every
// 16x16 tile it touches costs ~13 records per splat and made the (tile,id) sort the most expensive stage
// (profiles/r1_a/b).  Instead each workgroup walks its bin's depth-ordered list nearest-first and does
// the fine culling on chip:
//   stage A  every thread fetches 2 list entries (id -> the 32-byte record: centre, p1, p2, opacity, fp16 extents),
//            tests the footprint against the workgroup's region, and the survivors are compacted
//            IN ORDER (ballot + mbcnt) into an LDS batch, their records as they are;
//   finish   one thread per STAGED record (dense lanes, at the head of the shading loop) turns it into the blend walk's operands:
//            axes scaled by sqrt(log2 e) (the exponential is then a bare v_exp_f32), centre terms around the region centre,
//            log2 of the opacity, the fragment rule's cutoff term, the mask of the quarters its ellipse can reach;
//   shading  colour + SH of the staged records (deferred from the projection: a sixth of the sorted splats are ever staged);
//   stage B  each wave walks the batch, skips records that miss its quarter, and blends front-to-back:
//            q=(d.p1)^2+(d.p2)^2 (== A/2, frag.slang:236), alpha = 2^(log2 a - q), discard q>4 and alpha<=1/255 (one cutoff per
//            record, applied as a packed fma with the clamp modifier).
// A wave retires when all 128 pixels have T < 1e-4; the workgroup stops fetching when all 4 have.  In MGS_ALPHA_SUM mode, where the
// reference's additive alpha must see every fragment, a saturated wave goes on SUMMING alpha (a walk of its own: two LDS quads,
// seven packed fmas, two v_exp per record), and the batches staged after all four are saturated are staged and walked as a
// quadratic in the pixel offset.
#ifndef MGS_CMP_ENTRIES
#define MGS_CMP_ENTRIES 2
#endif
constexpr int kCmpEntries = MGS_CMP_ENTRIES;                  // list entries per thread per stage-A round (sweep with shading in the kernel: 1/2/3/4/6 -> 0.137/0.134/0.140/0.142/0.157 ms; 4K 0.374/0.379/-/0.42/-)
// (a stage-A round scans 256 * kCmpEntries list entries)
#ifndef MGS_CMP_CAP
#define MGS_CMP_CAP 288
#endif
#ifndef MGS_CMP_GO
#define MGS_CMP_GO 32
#endif
constexpr int kCmpCap     = MGS_CMP_CAP;                // LDS batch capacity (records): 18 KB -> 8 workgroups per CU (sweep: 384/512/768 -> 0.220/0.230/0.275 ms)
constexpr int kCmpGo      = MGS_CMP_GO;                // blend as soon as this many records are staged (<= kCmpCap-256)
typedef float v2f __attribute__((ext_vector_type(2)));

// MODE: the compositor mode bits of composite_common.h (with the predicates surf_lds / occ_lds / sum_walk); SHF: SH storage format
#ifndef MGS_SUM_ENTRIES
#define MGS_SUM_ENTRIES MGS_CMP_ENTRIES
#endif
#ifndef MGS_SUM_CAP
#define MGS_SUM_CAP 448  // (sweep, garden-sized frame: 288/32 2.89 ms, 352/96 2.82, 416/160 2.80, 448/192 2.79 — 25.6 KB, still 6 workgroups
#endif                   //  per CU —, 544/288 2.77, 672/416 and beyond lose more to the residency than the longer batches gain)
#ifndef MGS_SUM_GO
#define MGS_SUM_GO 192
#endif
// MGS_CMP_FOLD: the blend walk's fragment alpha as 2^(log2 a - q) with the fragment rule as one packed fma + clamp (17 instead of
// 23 vector instructions per record and wave)
#ifndef MGS_CMP_FOLD
#define MGS_CMP_FOLD 1
#endif
#ifdef MGS_CMP_EXACT_PRED
#undef MGS_CMP_FOLD
#define MGS_CMP_FOLD 0
#endif
#ifndef MGS_SUM_POLY  // 0: A/B — batches of an all-saturated region are walked in the (s, u) form as well
#define MGS_SUM_POLY 1
#endif
#ifndef MGS_SUM_UNROLL
#define MGS_SUM_UNROLL 2
#endif
#ifndef MGS_CMP_WAVES
#define MGS_CMP_WAVES 6
#endif
template <int MODE, int SHF>
__global__ __launch_bounds__(256, MGS_CMP_WAVES) void k_composite(const std::conditional_t<occ_lds(MODE), CompositeArgsOcc, CompositeArgs> F, const uint2* __restrict__ ranges,
                                                   const uint32_t* __restrict__ valX, const uint32_t* __restrict__ valY,
                                                   const SortPlan* __restrict__ plan, const SplatRec* __restrict__ rec,
                                                   void* __restrict__ outImage, int fmt, FrameCounters* __restrict__ ctr,
                                                   float* __restrict__ outDepth, uint32_t* __restrict__ outSplatId,
                                                   const FrameArgs* __restrict__ Ap, float4* __restrict__ outNormal)
{
  // batch geometry: the additive-alpha mode (every fragment of a region's whole list is composited) has its own
  constexpr int cEnt = sum_walk(MODE) ? MGS_SUM_ENTRIES : kCmpEntries, cRound = 256 * cEnt;
  constexpr int cCap = sum_walk(MODE) ? MGS_SUM_CAP : kCmpCap, cGo = sum_walk(MODE) ? MGS_SUM_GO : kCmpGo;
  static_assert(cGo <= cCap - 256, "sub-group 0 of a stage-A round must always fit");
  uint32_t statStaged = 0, statScanned = 0;
  const uint64_t costT0 = wall_clock64();  // this region's duration feeds the next frame's bin order (F.binCost)
#ifdef MGS_CMP_TRACE  // debug build (tools/cmp_trace.py): per-workgroup wall-clock stamps, 100 MHz
  const uint64_t traceT0 = wall_clock64();
  uint64_t       traceA = 0, traceS = 0, traceB = 0, traceLast;  // time spent in stage A / shading / blending
  uint32_t       traceIters = 0, traceRounds = 0, traceNeed = 0, traceNeeded = 0;
  __shared__ uint32_t s_traceNeed;
  traceLast = traceT0;
#define MGS_TRACE_PHASE(acc) { const uint64_t now_ = wall_clock64(); acc += now_ - traceLast; traceLast = now_; }
#else
#define MGS_TRACE_PHASE(acc)
#endif
  __shared__ float4   s_a[cCap];  // k1, k2 (centre terms of d.p1, d.p2), fragment cutoff, -
  __shared__ float4   s_b[cCap];  // p1, p2 (scaled by sqrt(log2 e))
  __shared__ float4   s_c[cCap];  // r, g, b, a
  __shared__ uint32_t s_g[cCap];  // global id: what the deferred shading needs
  __shared__ float    s_z[surf_lds(MODE) ? cCap : 1];  // fragCoord.z of the record (surface outputs only)
  __shared__ float4   s_n[surf_lds(MODE) ? cCap : 1];  // world normal of the record (surface outputs only)
  __shared__ float    s_zo[occ_lds(MODE) ? cCap : 1];  // the record's tested depth: ndc z as the depth key has it (occluder only)
  __shared__ float    s_dmax[occ_lds(MODE) ? 4 : 1];   // per wave: the largest bound depth of its pixels (occluder only)
  __shared__ uint32_t s_wc[2][cEnt][4];
  __shared__ uint8_t  s_m[cCap];  // which of the 4 quarters (waves) the record's footprint touches
  // MGS_ALPHA_SUM without surface outputs: s_a = (k1, k2, log2 opacity, cutoff term) feeds the saturated waves' two-quad walk
  // (below); the unsaturated walk's fragment cutoff lives here instead
  __shared__ float    s_t[(sum_walk(MODE) && MGS_CMP_FOLD == 0) ? cCap : 1];

  const int t = threadIdx.x, lane = laneId(), w = t >> 6;
  // regions are 32-px columns x 16-px rows ("tile pairs"); binShiftX >= 1, so a pair never straddles two bins.
  // XCD-aware mapping: workgroup b lands on XCD b%8 (observed dispatch rule).  All regions of a bin — which
  // read the same list — go to one XCD (shared L2), and consecutive bins go to different XCDs so that the dense
  // part of the image is spread over all eight (contiguous screen bands per XCD left most of them idle).
  const int colsX    = (F.tilesX + 1) >> 1;
  const int bw       = 1 << (F.binShiftX - 1), bh = 1 << F.binShiftY;  // bin size in regions
  const int binRow0  = F.stripRow0 >> F.binShiftY;
  const int binRows  = ((F.stripRow1 - 1) >> F.binShiftY) - binRow0 + 1;
  const int perBin   = bw * bh;
  const int seq      = (int)(blockIdx.x >> 3);
  int       ord      = (seq / perBin) * 8 + (int)(blockIdx.x & 7);  // bin ordinal
  const int inBin    = seq % perBin;
  // (compositeRegionGrid of composite_common.h is the grid of this mapping; k_composite_gut2 maps its workgroups the same way)
  const bool ordered = directBinTables(plan)->binOrderValid != 0u;  // the binning stage ranked the bins by list length (all bins of the frame)
  int cx2, ty;
  if(ordered)
  {
    if(ord >= F.binsX * F.binsY)
      return;
    const int b = (int)directBinTables(plan)->binOrder[ord];
    cx2         = (b % F.binsX) * bw + inBin % bw;
    ty          = (b / F.binsX) * bh + inBin / bw;
  }
  else
  {
    if(ord >= binRows * F.binsX)
      return;
    cx2 = (ord % F.binsX) * bw + inBin % bw;
    ty  = (binRow0 + ord / F.binsX) * bh + inBin / bw;
  }
  if(cx2 >= colsX || ty < F.stripRow0 || ty >= F.stripRow1)
    return;
  const int      tx  = cx2 * 2;  // left 16-px tile of the region
  const int      qx0 = tx * kTilePx + (w & 1) * 16, qy0 = ty * kTilePx + (w >> 1) * 8;
  const int      px = qx0 + (lane & 7), py = qy0 + (lane >> 3);  // second pixel: px + 8
  const v2f      pcx = {(float)px + 0.5f, (float)px + 8.5f};
  const float    pcy = (float)py + 0.5f;
  const float    bcx = (float)(tx * kTilePx) + 16.0f, bcy = (float)(ty * kTilePx) + 8.0f;  // region centre
  const v2f      lx  = {pcx.x - bcx, pcx.y - bcx};  // pixel centre relative to the region centre (exact: half-integers)
  const float    ly  = pcy - bcy;
  const bool     in0 = px < F.width && py < F.height, in1 = px + 8 < F.width && py < F.height;
  constexpr bool early   = (MODE & kCmpAlphaSum) == 0;
  constexpr bool noGauss = (MODE & kCmpNoGauss) != 0;
  constexpr bool surf    = surf_lds(MODE);  // FTB side outputs: picked depth + the splat that set it (frag.slang:320-349)
  constexpr bool stoch   = (MODE & kCmpStochastic) != 0;
  constexpr bool occ     = occ_lds(MODE);
  constexpr bool sumWalk = sum_walk(MODE);
  constexpr bool fold    = MGS_CMP_FOLD != 0;  // s_a = (k1, k2, log2 a, cutoff term), s_b = (p1x, p2x, p1y, p2y)  // saturated waves only sum alpha (s_a layout: see s_t)
  constexpr float kSumBig = 1073741824.0f;   // 2^30: (log2 alpha - cutoff) * 2^30, clamped to [0, 1], is the fragment's 0 / 1 weight
  // frag.slang:271: seed = xxhash32(uint3(fragCoord.xy, frameSampleId)); the sample id changes every frame: read through
  // the per-frame constants, not the by-value arguments a captured graph freezes
  uint32_t seedPx0 = 0u, seedPx1 = 0u;
  if constexpr(stoch)
  {
    const uint32_t sid = (uint32_t)Ap->f.frameSampleId;
    seedPx0            = rngXxhash32((uint32_t)px, (uint32_t)py, sid);
    seedPx1            = rngXxhash32((uint32_t)px + 8u, (uint32_t)py, sid);
  }
  v2f            pickZ   = {0.0f, 0.0f};
  uint32_t       pickId0 = 0xFFFFFFFFu, pickId1 = 0xFFFFFFFFu;
  v2f            nx = {0.f, 0.f}, ny = {0.f, 0.f}, nz = {0.f, 0.f};  // integrated normal (surface outputs)
  // a saturated pixel (T < 1e-4) takes no further fragments: the result must not depend on WHEN its wave
  // notices (batch boundaries differ between a strip and the full frame, the frames must not)
  const float    tMin    = early ? 1.0e-4f : -1.0f;
  const uint32_t* vals   = plan->finalSel ? valY : valX;
  const int      bin     = (ty >> F.binShiftY) * F.binsX + (tx >> F.binShiftX);
  const uint2    range   = ranges[bin];
  constexpr float kSqrtLog2e = 1.2011224087864498f;   // sqrt(log2 e): exp(-q) == exp2(-(q * log2 e))
  constexpr float kQMax      = 4.0f * 1.4426950408889634f;

  // pixels outside the image start saturated (they are never stored), so "any T >= tMin" is the wave's liveness
  v2f  T = {in0 ? 1.0f : 0.0f, in1 ? 1.0f : 0.0f}, cr = {0.f, 0.f}, cg = {0.f, 0.f}, cb = {0.f, 0.f}, asum = {0.f, 0.f};
  bool waveDone = (__ballot(in0 || in1) == 0ull);
  // MGS_ALPHA_SUM (no early-out: the additive alpha sees every fragment): once every pixel of the wave is saturated (T < 1e-4)
  // the fragments that follow cannot change the colour any more (each weighs < 1e-4, as in the default mode, where the wave
  // retires at this point) — they are only SUMMED: no colour, no transmittance, and once all four waves are there the batch is
  // not shaded either (the SH sum is most of a staged record's cost).  The switch is checked per record, like the retirement.
  bool waveSat = waveDone, allSat = false;  // (a wave without pixels inside the image has nothing to saturate)
  // Occluder: D = the bound depth of this lane's two pixels (-inf outside the image; a NaN stays a NaN and passes nothing).  A fragment
  // of a record exists iff z <= D, z = the record's key depth (kernels_common.h: keyDepthNdcZ).  With a GPU-sorted list (F.occStop)
  // the records arrive in ascending z, so a record with z > max D of a wave ends that wave exactly as saturation does, and a
  // record with z > max D of the region is not even shaded.
  v2f   occD = {0.f, 0.f};
  float waveMaxD = 0.0f, regMaxD = 0.0f;
  if constexpr(occ)
  {
    constexpr float kNegInf = -__builtin_huge_valf();
    occD.x  = in0 ? F.occDepth[(size_t)py * (size_t)F.width + (size_t)px] : kNegInf;
    occD.y  = in1 ? F.occDepth[(size_t)py * (size_t)F.width + (size_t)(px + 8)] : kNegInf;
    float m = fmaxf(fmaxf(occD.x, kNegInf), fmaxf(occD.y, kNegInf));  // (fmaxf drops a NaN)
#pragma unroll
    for(int o = 32; o > 0; o >>= 1)
      m = fmaxf(m, __shfl_xor(m, o, 64));
    waveMaxD = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
    if(lane == 0)
      s_dmax[w] = waveMaxD;
    __syncthreads();
    regMaxD = fmaxf(fmaxf(s_dmax[0], s_dmax[1]), fmaxf(s_dmax[2], s_dmax[3]));
  }

  uint32_t hi   = range.y;
  uint32_t fill = 0;  // records currently in the LDS batch
  int      rnd  = 0;
  uint32_t gNext[cEnt];
  bool     prefValid = false;
#pragma unroll
  for(int k = 0; k < cEnt; ++k)
    gNext[k] = 0u;
  for(;;)
  {
    // ---- stage A: scan list entries (nearest first) until enough records are staged or the list ends ----
    // A round looks at up to 1024 entries as 4 sub-groups of 256 (k-th sub-group = entries k*256+t).  The
    // sub-groups are accepted in order while they fit into the batch; since fill < cGo <= cap-256 on
    // entry, sub-group 0 always fits, so every round makes progress and the batch can never overflow.
    // The ids of the NEXT round are fetched before this round's barrier (one dependent trip instead of two).
    while(hi > range.x && fill < (uint32_t)cGo)
    {
#ifdef MGS_CMP_TRACE
      ++traceRounds;
#endif
      const uint32_t avail = hi - range.x;
      uint32_t       g[cEnt];
      float4         a[cEnt], pb[cEnt];  // (cx, cy, ex, ey), (p1, p2)
      float          al[cEnt];                  // opacity
      bool           ok[cEnt];
      uint64_t       bal[cEnt];
#pragma unroll
      for(int k = 0; k < cEnt; ++k)
      {
        const uint32_t e = k * 256u + (uint32_t)t;  // e-th nearest remaining entry
        ok[k]            = e < avail;
        g[k]             = prefValid ? gNext[k] : (ok[k] ? vals[hi - 1u - e] : 0u);
      }
#pragma unroll
      for(int k = 0; k < cEnt; ++k)
      {  // the whole 32-byte record (half a sector): centre + p1 | p2 + opacity + fp16 extents
        const float4* r  = reinterpret_cast<const float4*>(rec + g[k]);
        const float4  r0 = ok[k] ? r[0] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4  r1 = ok[k] ? r[1] : make_float4(0.f, 0.f, 0.f, __uint_as_float(0xBC00BC00u));  // extents -1: fails the test
        const uint32_t eb = __float_as_uint(r1.w);
        const float2   e  = __half22float2(*reinterpret_cast<const __half2*>(&eb));
        a[k]  = make_float4(r0.x, r0.y, e.x, e.y);
        pb[k] = make_float4(r0.z, r0.w, r1.x, r1.y);
        al[k] = r1.z;
      }
      // speculative prefetch of the next round's ids (valid if this round is consumed completely)
      {
        const uint32_t hiN = hi - min(avail, (uint32_t)cRound);
        const uint32_t avN = hiN - range.x;
#pragma unroll
        for(int k = 0; k < cEnt; ++k)
        {
          const uint32_t e = k * 256u + (uint32_t)t;
          gNext[k]         = (e < avN) ? vals[hiN - 1u - e] : 0u;
        }
      }
#pragma unroll
      for(int k = 0; k < cEnt; ++k)
      {
        // pixel centres of the region span bcx +- 15.5, bcy +- 7.5
        ok[k]  = ok[k] && fabsf(a[k].x - bcx) <= a[k].z + 15.5f && fabsf(a[k].y - bcy) <= a[k].w + 7.5f;
        bal[k] = __ballot(ok[k]);
        if(lane == 0)
          s_wc[rnd & 1][k][w] = (uint32_t)__popcll(bal[k]);
      }
      __syncthreads();
      const uint32_t(*cnt)[4] = s_wc[rnd & 1];
      ++rnd;
      uint32_t base = fill;
      int      used = 0;  // sub-groups consumed
#pragma unroll
      for(int k = 0; k < cEnt; ++k)
      {
        const uint32_t m = cnt[k][0] + cnt[k][1] + cnt[k][2] + cnt[k][3];
        if(used == k && base + m <= (uint32_t)cCap)
        {
          uint32_t wb = 0;
          if(w > 0) wb += cnt[k][0];
          if(w > 1) wb += cnt[k][1];
          if(w > 2) wb += cnt[k][2];
          if(ok[k])
          {
            // the survivor's record goes to its place in the batch as it is (centre + extents | p1, p2 | opacity | id); what the
            // blend walk reads is computed from it by finishRecord below, once per STAGED record and on dense lanes — here,
            // under the survivors' predicate, the arithmetic ran for every round of 64 entries (a quarter of which survive)
            const uint32_t pos = base + wb + lanesBelow(bal[k]);
            s_a[pos]           = a[k];
            s_b[pos]           = pb[k];
            // (the opacity alone, a 4-byte LDS store: a 16-byte one costs the wave 13 cycles of the LDS path however few of its lanes
            //  are survivors — composite -3 us; rgb is the shading phase's)
            reinterpret_cast<float*>(&s_c[pos])[3] = al[k];
            s_g[pos]           = g[k];
          }
          base += m;
          used = k + 1;
        }
      }
      statStaged += base - fill;
      fill                    = base;
      const uint32_t consumed = min(avail, (uint32_t)used * 256u);
      statScanned += consumed;
      prefValid               = (used == cEnt);
      hi -= consumed;
      if(used < cEnt)
        break;  // batch full: blend, then rescan the unconsumed sub-groups
    }
    __syncthreads();
    MGS_TRACE_PHASE(traceA)
    // ---- shading: the SH sum of the staged splats (mesh.slang:243), one thread per record ---------------------
    // Deferred from the projection: only splats that reach an unsaturated region are ever shaded (a quarter of
    // the frustum survivors on the garden-sized bench), and their 192-byte SH records are the bulk of a splat.
    // ---- finish the staged records (dense lanes, one thread per record): the blend walk's operands and the quarter masks ----
    auto finishRecord = [&](uint32_t pos) {
      const float4 ak = s_a[pos], pbk = s_b[pos];  // (cx, cy, ex, ey), (p1, p2)
      const float  alk = s_c[pos].w;
        const float4   sb  = make_float4(pbk.x * kSqrtLog2e, pbk.y * kSqrtLog2e, pbk.z * kSqrtLog2e, pbk.w * kSqrtLog2e);
        // (s, u) = (d.p1, d.p2) with d = pixel - centre, rewritten around the region centre: s = lx*p1x + (ly*p1y + k1),
        // k1 = -((cx - bcx)*p1x + (cy - bcy)*p1y), lx/ly = the pixel relative to the region centre (|.| <= 15.5):
        // two instructions per pixel pair instead of three, and small operands (no 1000-px coordinates in the products)
        const float rx = ak.x - bcx, ry = ak.y - bcy;
        s_a[pos]       = make_float4(-(rx * sb.x + ry * sb.y), -(rx * sb.z + ry * sb.w), 0.0f, 0.0f);  // .z: the fragment cutoff, below
        // (saturated Σα walk: the y terms of (s, u) are ONE packed fma when p1y, p2y are neighbours — as k1, k2 are)
        s_b[pos]           = (sumWalk || fold) ? make_float4(sb.x, sb.z, sb.y, sb.w) : sb;
        // quarter (qx,qy): pixel centres x in [bcx-15.5,bcx-0.5] / [bcx+0.5,bcx+15.5], y in [bcy-7.5,bcy-0.5] / [bcy+0.5,bcy+7.5].
        // Footprint box first, then a bound in the ellipse's own frame: over the quarter (centre m, half
        // extents 7.5 x 3.5) s = d.p1 stays within |s_m| -+ (7.5|p1x| + 3.5|p1y|), likewise u = d.p2, so
        // q >= max(0,|s_m|-rs)^2 + max(0,|u_m|-ru)^2; a quarter whose bound exceeds what the alpha
        // threshold lets through (a 2^-q > 1/255) cannot receive a fragment.  43 % of the wave-level
        // evaluations were empty before this test (corner overlaps of slanted ellipses).
        const bool  xl = ak.x - ak.z <= bcx - 0.5f, xr = ak.x + ak.z >= bcx + 0.5f;
        const bool  yt = ak.y - ak.w <= bcy - 0.5f, yb = ak.y + ak.w >= bcy + 0.5f;
        const float rc = alk;
        // Fragment rule of frag.slang:242-262 — discard A > 8 (q > kQMax here), discard alpha <= 1/255 — as ONE compare per
        // pixel: alpha = a 2^-q > 1/255  <=>  q < log2(255 a).  (Two compares + the saturation test per pixel were a
        // quarter of the blend loop's instructions.)  A fragment whose alpha is within rounding of 1/255 may fall on
        // the other side than with the exp-then-compare order: a contribution of <= 0.4 % of one splat's colour.
        const float qCut = noGauss ? kQMax : fminf(kQMax, __log2f(fmaxf(rc * 255.0f, 1.0f)));
        if constexpr(sumWalk || fold)
        {  // saturated waves: alpha = 2^(l2a - q), kept iff q <= qCut  <=>  l2a - q >= l2a - qCut =: c, evaluated as
           // clamp((l2a - q) * 2^30 - c * 2^30) in {0, 1}
          const float l2a = noGauss ? 0.0f : __log2f(fmaxf(rc, 1.0e-30f));
          const float tb  = (qCut - l2a) * kSumBig;
          if(sumWalk && MGS_SUM_POLY && allSat)
          {  // every wave of the region is saturated: this batch is only ever summed, by the polynomial walk (stage B) —
             // nq = l2a - q as a quadratic in the pixel's offset (lx, ly) from the region centre,
             // q = (lx p1x + ly p1y + k1)^2 + (lx p2x + ly p2y + k2)^2:
             // nq = (nA lx + (nB ly + nD)) lx + ((nC ly + nE) ly + F'), coefficients per record, computed here once
            const float k1 = -(rx * sb.x + ry * sb.y), k2 = -(rx * sb.z + ry * sb.w);
            s_a[pos] = make_float4(-2.0f * (sb.x * sb.y + sb.z * sb.w), -(sb.y * sb.y + sb.w * sb.w),
                                   -2.0f * (k1 * sb.x + k2 * sb.z), -2.0f * (k1 * sb.y + k2 * sb.w));
            s_b[pos] = make_float4(-(sb.x * sb.x + sb.z * sb.z), l2a - (k1 * k1 + k2 * k2), tb, 0.0f);
          }
          else
          {
            s_a[pos].z = l2a;
            s_a[pos].w = tb;
            if constexpr(!fold)
              s_t[pos] = qCut;
          }
        }
        else
        {
          s_a[pos].z = qCut;
          s_a[pos].w = rc;
        }
        const float qLim = qCut * 1.001f + 1e-3f;
        const float rs = 7.5f * fabsf(sb.x) + 3.5f * fabsf(sb.y), ru = 7.5f * fabsf(sb.z) + 3.5f * fabsf(sb.w);
        uint32_t    qm = 0;
#pragma unroll
        for(int qd = 0; qd < 4; ++qd)
        {
          const float mx = bcx + ((qd & 1) ? 8.0f : -8.0f) - ak.x, my = bcy + ((qd & 2) ? 4.0f : -4.0f) - ak.y;
          const float ds = fmaxf(fabsf(mx * sb.x + my * sb.y) - rs, 0.0f), du = fmaxf(fabsf(mx * sb.z + my * sb.w) - ru, 0.0f);
          const bool  box = ((qd & 1) ? xr : xl) && ((qd & 2) ? yb : yt);
          qm |= (box && ds * ds + du * du <= qLim) ? (1u << qd) : 0u;
        }
        //  a record with a non-finite axis or centre takes no part: the folded fragment rule is clamp(fma) * exp2(nq), and a
        // NaN nq would pass the clamp as 0 and then poison colour and T through 0 * NaN — the select it replaced mapped NaN to 0.
        // k1 + k2 is non-finite whenever any of sb, rx, ry is (0 * Inf = NaN included); two instructions per STAGED record.
        if(!(fabsf((rx * sb.x + ry * sb.y) + (rx * sb.z + ry * sb.w)) < 3.0e38f))
          qm = 0u;
        s_m[pos] = (uint8_t)qm;
    };
    for(uint32_t j = t; j < fill; j += 256)
    {
      finishRecord(j);
      if(allSat)
        continue;  // (a region whose four waves are saturated sums alpha only: nothing to shade)
      const uint32_t gid = s_g[j];
      CompositeArgs::Inst I = F.inst[0];
      int                 instIdx = 0;
      if(F.nInstances <= kMaxInlineInstances)
      {
        for(int i = 1; i < F.nInstances; ++i)
          if(gid >= F.inst[i].globalOffset)
          {
            I       = F.inst[i];
            instIdx = i;
          }
      }
      else
      {  // many instances: binary search in the device table (ascending global offsets)
        int lo = 0, hi2 = F.nInstances;
        while(hi2 - lo > 1)
        {
          const int mid = (lo + hi2) >> 1;
          if(gid >= F.instTable[mid].globalOffset)
            lo = mid;
          else
            hi2 = mid;
        }
        I       = F.instTable[lo];
        instIdx = lo;
      }
      const uint32_t li = gid - I.globalOffset;
      // base colour (mesh.slang:162,205-207) and the view direction in model space (mesh.slang:240-241); the
      // camera position of the instance is per-frame data, read through the frame-argument pointer.
      // (Fetching the first part of the SH record together with these loads — it does not depend on the direction —
      // was measured: the extra live registers spill, 0.140 -> 0.179 ms.)
      const float4 col = I.rgba[li];  // fetchColor, dequantised at commit
      const float  cpx = I.centers[3 * (size_t)li], cpy = I.centers[3 * (size_t)li + 1], cpz = I.centers[3 * (size_t)li + 2];
      if constexpr(occ)
      {
        const float zo = keyDepthNdcZ(Ap->inst[instIdx].model, Ap->f.view, Ap->f.proj, cpx, cpy, cpz);
        s_zo[j]        = zo;
        if(F.occStop && zo > regMaxD)
        {  // behind the occluder at every pixel of the region: no wave walks it, nothing to shade
          s_m[j] = 0;
          continue;
        }
      }
      const float* cam = Ap->inst[instIdx].camModel;
      float        dx = cpx - cam[0], dy = cpy - cam[1], dz = cpz - cam[2];
      const float  dl = rsqrtf(dx * dx + dy * dy + dz * dz);
      dx *= dl;
      dy *= dl;
      dz *= dl;
      float4 c = s_c[j];
      c.x = F.shOnly ? 0.5f : col.x;
      c.y = F.shOnly ? 0.5f : col.y;
      c.z = F.shOnly ? 0.5f : col.z;
      const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
      if(deg > 0)
        addShRadiance<SHF>(I.sh, li, deg, dx, dy, dz, c.x, c.y, c.z);
      s_c[j] = c;
      if constexpr(surf)
      {
        const InstanceConst& IC = Ap->inst[instIdx];
        s_n[j] = splatWorldNormal(Ap->f, IC, li, Ap->f.quantizeNormals != 0);
        // fragCoord.z of the splat's quad: clip.z / clip.w of the centre (mesh.slang:175-178,276-289)
        const float* MV = IC.modelView;
        const float* P  = Ap->f.proj;
        const float  tx = MV[0] * cpx + MV[4] * cpy + MV[8] * cpz + MV[12];
        const float  ty = MV[1] * cpx + MV[5] * cpy + MV[9] * cpz + MV[13];
        const float  tz = MV[2] * cpx + MV[6] * cpy + MV[10] * cpz + MV[14];
        const float  tw = MV[3] * cpx + MV[7] * cpy + MV[11] * cpz + MV[15];
        const float  cz = P[2] * tx + P[6] * ty + P[10] * tz + P[14] * tw;
        const float  cw = P[3] * tx + P[7] * ty + P[11] * tz + P[15] * tw;
        s_z[j]          = cz * (1.0f / cw);
      }
    }
    __syncthreads();
    MGS_TRACE_PHASE(traceS)
    // ---- stage B: blend the batch ------------------------------------------------------------------------
    // 64 records at a time: a ballot over the quarter masks gives this wave's hit set; the hits are walked
    // with scalar bit tricks (no per-record branch) and the per-pixel discards are predicated.
    if(!waveDone)
    {
      // (the wave's quarter bit as a scalar: derived from the thread index it was a vector register the compiler spilled and
      //  re-loaded from scratch at the head of every 64-record chunk)
      const uint32_t wbit = 1u << (uint32_t)__builtin_amdgcn_readfirstlane(w);
      const v2f      sumBig2 = {kSumBig, kSumBig};
      for(uint32_t j0 = 0; j0 < fill; j0 += 64)
      {
        const uint32_t jl   = j0 + (uint32_t)lane;
        const bool     mine = jl < fill && (s_m[jl] & wbit) != 0u;
        uint64_t       hits = __ballot(mine);
        if constexpr(sumWalk)
        {
          if(MGS_SUM_POLY && allSat)
          {  // the batch was staged for the polynomial walk (stage A): 5 packed fmas, one plain one, two v_exp per record
            uint64_t hs = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(hits >> 32)) << 32)
                          | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hits);
            auto polyTerm = [&](const float4 a1, const float4 b1, v2f& m, v2f& e) {  // (nB, nC, nD, nE), (nA, F', cutoff term, -)
              const v2f    bc = {a1.x, a1.y}, de = {a1.z, a1.w}, tz = {b1.z, b1.w};
              const v2f    hg = ly * bc + de;          // (nB ly + nD, nC ly + nE)
              const float  g  = hg.y * ly + b1.y;
              const v2f    nq = (lx * b1.x + hg.x) * lx + g;
              asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,1,0] clamp" : "=v"(m) : "v"(nq), "s"(sumBig2), "v"(tz));
              if(noGauss)
                e = (v2f){1.0f, 1.0f};
              else
                e = (v2f){__builtin_amdgcn_exp2f(nq.x), __builtin_amdgcn_exp2f(nq.y)};
            };
#if MGS_SUM_UNROLL >= 2
            // several records per trip, their LDS quads requested together: the walk of ONE wave is a latency chain per record
            // (LDS round trip, four dependent packed fmas, v_exp), and the region with the longest list is the kernel's span
            while(__builtin_popcountll(hs) >= MGS_SUM_UNROLL)
            {
              float4 qa[MGS_SUM_UNROLL], qb[MGS_SUM_UNROLL];
#pragma unroll
              for(int u = 0; u < MGS_SUM_UNROLL; ++u)
              {
                const uint32_t j = j0 + (uint32_t)__builtin_ctzll(hs);
                hs &= hs - 1ull;
                qa[u] = s_a[j];
                qb[u] = s_b[j];
              }
              v2f mm[MGS_SUM_UNROLL], ee[MGS_SUM_UNROLL];
#pragma unroll
              for(int u = 0; u < MGS_SUM_UNROLL; ++u)
                polyTerm(qa[u], qb[u], mm[u], ee[u]);
#pragma unroll
              for(int u = 0; u < MGS_SUM_UNROLL; ++u)
                asum = ee[u] * mm[u] + asum;  // in list order
            }
#endif
            while(hs != 0ull)
            {
              const uint32_t j = j0 + (uint32_t)__builtin_ctzll(hs);
              hs &= hs - 1ull;
              v2f m, e;
              polyTerm(s_a[j], s_b[j], m, e);
              asum = e * m + asum;
            }
            continue;
          }
        }
        // MGS_ALPHA_SUM: a saturated wave walks its hits in a loop of its own (below); the switch happens per record
        while(hits != 0ull && !(sumWalk && waveSat))
        {
          const uint32_t j = j0 + (uint32_t)__builtin_ctzll(hits);
          hits &= hits - 1ull;
          float zo = 0.0f;
          if constexpr(occ)
          {
            zo = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_zo[j])));
            if(F.occStop && zo > waveMaxD)
            {  // this record and every later one of the list lie behind the occluder at every pixel of the wave
              waveDone = true;
              break;
            }
          }
#if MGS_CMP_FOLD
          // alpha = a 2^-q as 2^(log2 a - q); the fragment rule of frag.slang:242-262 (discard A > 8, discard alpha <= 1/255: one
          // cutoff per record, stage A) as clamp((log2 a - q) * 2^30 + cutoff term) in {0, 1} — a packed fma instead of two
          // compares and two selects; the y terms of (s, u) packed.  No test of T: a saturated pixel of a live wave keeps taking
          // fragments (each weighs < 1e-4) until the WAVE retires, which is checked per record and depends only on the
          // sequence of records — the same in a strip and in the full frame
          const float4 a1 = s_a[j], b1 = s_b[j];  // (k1, k2, log2 a, cutoff term), (p1x, p2x, p1y, p2y)
          const v2f    k12 = {a1.x, a1.y}, py12 = {b1.z, b1.w}, zw = {a1.z, a1.w};
          const v2f    yt  = ly * py12 + k12;
          const v2f    s1 = lx * b1.x + yt.x, u1 = lx * b1.y + yt.y;
          const v2f    nq = -(u1 * u1) + (-(s1 * s1) + a1.z);  // log2 alpha;  q == (A/2) * log2 e of frag.slang:236
          float4       c1 = s_c[j];
          {  // keep (b, a) a register pair: the whole quad in one ds_read_b128 (4 LDS cycles; the b96 the compiler picks when
             // .w is unused takes 8) and blue broadcast through op_sel instead of a move
            v2f czw = {c1.z, c1.w};
            asm("" : "+v"(czw));
            c1.z = czw.x;
            c1.w = czw.y;
          }
          v2f          ah;
          asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,1,1] clamp" : "=v"(ah) : "v"(nq), "s"(sumBig2), "v"(zw));
          if(!noGauss)  // frag.slang:248-254
          {
            const v2f e = {__builtin_amdgcn_exp2f(nq.x), __builtin_amdgcn_exp2f(nq.y)};
            ah          = e * ah;
          }
#else
          const float4 a1 = s_a[j], b0 = s_b[j];
          const float4 b1 = sumWalk ? make_float4(b0.x, b0.z, b0.y, b0.w) : b0;  // (p1x, p1y, p2x, p2y)
          const v2f    s1 = lx * b1.x + (ly * b1.y + a1.x), u1 = lx * b1.z + (ly * b1.w + a1.y);
          const v2f    q  = s1 * s1 + u1 * u1;  // == (A/2) * log2 e of frag.slang:236
          const float  qc = sumWalk ? s_t[j] : a1.z;
          const float4 c1 = s_c[j];
          v2f          al = {1.0f, 1.0f};
          if(!noGauss)  // frag.slang:248-254
          {
            const v2f e = {__builtin_amdgcn_exp2f(-q.x), __builtin_amdgcn_exp2f(-q.y)};
            al          = e * c1.w;
          }
          v2f ah;  // frag.slang:242-245,258-262, predicated (cutoff per record, see stage A)
#ifdef MGS_CMP_EXACT_PRED
          ah.x = (q.x <= kQMax && al.x > (1.0f / 255.0f) && T.x >= tMin) ? al.x : 0.0f;
          ah.y = (q.y <= kQMax && al.y > (1.0f / 255.0f) && T.y >= tMin) ? al.y : 0.0f;
#else
          // no test of T: a saturated pixel of a live wave keeps taking fragments (each weighs < 1e-4) until the WAVE retires,
          // which is checked per record and depends only on the sequence of records — the same in a strip and in the full frame
          ah.x = (q.x <= qc) ? al.x : 0.0f;
          ah.y = (q.y <= qc) ? al.y : 0.0f;
#endif
#endif
          if constexpr(occ)
          {  // the depth test: LESS_OR_EQUAL against the pixel's bound depth, one z per record
            ah.x = (zo <= occD.x) ? ah.x : 0.0f;
            ah.y = (zo <= occD.y) ? ah.y : 0.0f;
          }
          if constexpr(stoch)
          {  // frag.slang:272-276: seed = xxhash32(uint3(seed, splatId, primitiveID)); accept iff rand(seed) < opacity.
            // primitiveID = 2 * (index of the splat in its mesh workgroup of 32) + triangle; the quad (-1,-1),(1,-1),(1,1),(-1,1)
            // is split along (-1,-1)-(1,1): triangle 0 = (0,2,1) holds u > v (mesh.slang:158-159,193).  The reference's index
            // comes from an unsorted, atomically compacted list (not reproducible); ours is the global id modulo 32.
            const uint32_t gid = s_g[j], prim = 2u * (gid & 31u);
            uint32_t       h0 = rngXxhash32(seedPx0, gid, prim + (s1.x > u1.x ? 0u : 1u));
            uint32_t       h1 = rngXxhash32(seedPx1, gid, prim + (s1.y > u1.y ? 0u : 1u));
            ah.x = (ah.x > 0.0f && rngRand(h0) < ah.x) ? 1.0f : 0.0f;
            ah.y = (ah.y > 0.0f && rngRand(h1) < ah.y) ? 1.0f : 0.0f;
          }
          const v2f wgt = ah * T;
          cr += wgt * c1.x;
          cg += wgt * c1.y;
          cb += wgt * c1.z;
          if(!early)
            asum += ah;
          T -= wgt;
          if constexpr(surf)
          {  // normal attachment: "under" blend of (normal * opacity, opacity) (gaussian_splatting.cpp:2095-2107)
            const float4 n1 = s_n[j];
            nx += wgt * n1.x;
            ny += wgt * n1.y;
            nz += wgt * n1.z;
            // transmittance *= (1 - opacity); if(depth == 0 && transmittance < threshold) depth = fragCoord.z
            const float    zr  = s_z[j];
            const uint32_t gid = s_g[j];
            if(ah.x > 0.0f && pickZ.x == 0.0f && T.x < F.depthIsoThreshold)
            {
              pickZ.x = zr;
              pickId0 = gid;
            }
            if(ah.y > 0.0f && pickZ.y == 0.0f && T.y < F.depthIsoThreshold)
            {
              pickZ.y = zr;
              pickId1 = gid;
            }
          }
          // checked per record (the compares are the predicate's): a 64-record chunk used to run to its end
          // after the last pixel had saturated
          if(early && __ballot(T.x >= tMin || T.y >= tMin) == 0ull)
          {
            waveDone = true;
#ifdef MGS_CMP_TRACE
            traceNeed = j + 1u;  // this wave needed the batch's records up to here
#endif
            break;
          }
          if(!early && __ballot(T.x >= 1.0e-4f || T.y >= 1.0e-4f) == 0ull)
            waveSat = true;
        }
        if constexpr(sumWalk)
        {
          // Saturated wave in MGS_ALPHA_SUM mode: the fragment only adds its alpha.  (Not with surface outputs: the depth / id
          // pick fires when T crosses depth_iso_threshold, which may lie below 1e-4 — T has to keep falling there, as in the
          // reference, the oracle and the default mode's full path.)  Two LDS quads per record; the opacity is folded into the
          // exponent (nq = log2 a - q, alpha = 2^nq) and the fragment rule (q <= qCut) is one packed fma with the clamp
          // modifier instead of two compares + two selects: seven packed fmas and two v_exp per record and 128 pixels — this
          // walk IS bound by VALU issue.
          // (the hit mask is wave-uniform; said explicitly, or the walk's bit tricks land on the vector unit)
          uint64_t hs = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(hits >> 32)) << 32)
                        | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hits);
          // one record's fragments for this lane's two pixels: weight m in {0, 1} (the fragment rule) and alpha e
          auto sumTerm = [&](uint32_t j, v2f& m, v2f& e) {
            const float4 a1 = s_a[j], b1 = s_b[j];  // (k1, k2, log2 a, cutoff term), (p1x, p2x, p1y, p2y)
            const v2f    k12 = {a1.x, a1.y}, py12 = {b1.z, b1.w}, zw = {a1.z, a1.w};
            const v2f    yt  = ly * py12 + k12;
            const v2f    s1 = lx * b1.x + yt.x, u1 = lx * b1.y + yt.y;
            const v2f    nq = -(u1 * u1) + (-(s1 * s1) + a1.z);
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,1,1] clamp" : "=v"(m) : "v"(nq), "s"(sumBig2), "v"(zw));
            if(noGauss)
              e = (v2f){1.0f, 1.0f};
            else
              e = (v2f){__builtin_amdgcn_exp2f(nq.x), __builtin_amdgcn_exp2f(nq.y)};
          };
#if MGS_SUM_UNROLL == 2
          // two records per trip: two independent chains (LDS round trip, six dependent packed fmas, v_exp) in flight per wave;
          // the sums are added in list order, as in the one-record form
          while((hs & (hs - 1ull)) != 0ull)
          {
            const uint32_t ja = j0 + (uint32_t)__builtin_ctzll(hs);
            hs &= hs - 1ull;
            const uint32_t jb = j0 + (uint32_t)__builtin_ctzll(hs);
            hs &= hs - 1ull;
            v2f ma, ea, mb, eb;
            sumTerm(ja, ma, ea);
            sumTerm(jb, mb, eb);
            asum = ea * ma + asum;
            asum = eb * mb + asum;
          }
#endif
          while(hs != 0ull)
          {
            const uint32_t j = j0 + (uint32_t)__builtin_ctzll(hs);
            hs &= hs - 1ull;
            v2f m, e;
            sumTerm(j, m, e);
            asum = e * m + asum;
          }
        }
        if(waveDone)
          break;
      }
    }
#ifdef MGS_CMP_TRACE
    {  // how many of the batch's (shaded) records did the region need?  max over the waves that blended this batch
      if(!waveDone)
        traceNeed = fill;
      if(t == 0) s_traceNeed = 0u;
      __syncthreads();
      if(lane == 0 && traceNeed) atomicMax(&s_traceNeed, traceNeed);
      __syncthreads();
      traceNeeded += s_traceNeed;
      traceNeed = 0u;
    }
    ++traceIters;
#endif
    if constexpr(occ)
    {  // records the wave's quarter mask skipped count too: the batch's last record has the batch's largest z
      if(F.occStop && fill > 0u && s_zo[fill - 1u] > waveMaxD)
        waveDone = true;
    }
    fill = 0;
    const int allFlag = __syncthreads_and(((early || occ) ? waveDone : waveSat) ? 1 : 0);
    MGS_TRACE_PHASE(traceB)
    const bool allDone = (early || occ) && allFlag != 0;
    allSat             = !early && !surf && !occ && allFlag != 0;  // (surface outputs: the records' depth and normal stay needed)
    if(allDone || hi <= range.x)
      break;
  }

#ifdef MGS_CMP_TRACE
  if(t == 0 && F.trace)
  {
    uint64_t* o = F.trace + (size_t)blockIdx.x * 10;
    o[0] = traceT0; o[1] = wall_clock64(); o[2] = statScanned; o[3] = statStaged; o[4] = traceIters | ((uint64_t)traceNeeded << 32); o[5] = traceRounds;
    o[6] = traceA; o[7] = traceS; o[8] = traceB; o[9] = ((uint64_t)range.y - range.x) | ((uint64_t)(ty * colsX + cx2) << 32);
  }
#endif
  if(t == 0)
  {  // frame statistics (mgs_frame_stats): two fire-and-forget adds per workgroup
    FrameStatLine* stat = frameStatLineFromPairs(plan, blockIdx.x >> 3);
    atomicAdd(&stat->staged, statStaged);
    atomicAdd(&stat->scanned, statScanned);
    // the bin's longest region, for the next frame of this context: regions that never saturate take twice as long as the
    // others, and starting them late is the kernel's tail; which ones they are is the same from one frame to the next
    atomicMax(&F.binCost[bin], (uint32_t)(wall_clock64() - costT0) + 1u);
  }
  const v2f aout = early ? (v2f){1.0f - T.x, 1.0f - T.y} : asum;
#pragma unroll
  for(int h = 0; h < 2; ++h)
  {
    if(h ? in1 : in0)
    {
      float        r = h ? cr.y : cr.x, g = h ? cg.y : cg.x, b = h ? cb.y : cb.x, ao = h ? aout.y : aout.x;
      const size_t o = (size_t)py * (size_t)F.width + (size_t)(px + 8 * h);
      if constexpr(occ)
      {  // the caller's geometry behind the splats: final = splats + T * geometry (gaussian_splatting.cpp:2343-2356); MGS_ALPHA_SUM
         // adds the geometry's alpha (the blend equations started from a destination that holds it)
        if(F.occColor)
        {
          const float4 bg = F.occColor[o];
          const float  Th = h ? T.y : T.x;
          r += Th * bg.x;
          g += Th * bg.y;
          b += Th * bg.z;
          if(!early)
            ao += bg.w;
        }
      }
      storePixel(outImage, fmt, o, r, g, b, ao);
      if constexpr(surf)
      {
        outDepth[o]   = h ? pickZ.y : pickZ.x;
        outSplatId[o] = h ? pickId1 : pickId0;
        outNormal[o]  = h ? make_float4(nx.y, ny.y, nz.y, 1.0f - T.y) : make_float4(nx.x, ny.x, nz.x, 1.0f - T.x);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the kernel's by-value arguments from the frame's constants (the instantiations without an occluder take the CompositeArgs part)
static CompositeArgsOcc compositeArgs(const CompositeLaunch& L)
{
  const FrameArgs&  A = *L.A;
  const FrameConst& F = A.f;
  CompositeArgsOcc  C;
  std::memset(&C, 0, sizeof(C));
  C.width = F.width; C.height = F.height; C.tilesX = F.tilesX;
  C.binShiftX = F.binShiftX; C.binShiftY = F.binShiftY; C.binsX = F.binsX; C.binsY = F.binsY;
  C.stripRow0 = F.stripRow0; C.stripRow1 = F.stripRow1;
  C.nInstances = F.nInstances; C.shDegree = F.shDegree;
  C.depthIsoThreshold = F.depthIsoThreshold;
  C.shOnly     = (F.debugFlags & 2) ? 1 : 0;
  C.binCost    = L.binCost;
  for(int i = 0; i < F.nInstances && i < kMaxInlineInstances; ++i)
  {
    C.inst[i].sh           = A.inst[i].sh;
    C.inst[i].rgba         = reinterpret_cast<const float4*>(A.inst[i].rgbaF32);
    C.inst[i].centers      = A.inst[i].centers;
    C.inst[i].globalOffset = A.inst[i].globalOffset;
    C.inst[i].shDegree     = A.inst[i].shDegree;
  }
  C.instTable = static_cast<const CompositeArgs::Inst*>(L.instTable);
  C.occDepth  = L.occ.depth;
  C.occColor  = reinterpret_cast<const float4*>(L.occ.color);
  C.occStop   = L.occ.sortedByKey ? 1 : 0;
  return C;
}

// one mode in the three SH storage formats
template <int MODE>
static void launchCompositeMode(hipStream_t stream, const CompositeLaunch& L, const CompositeArgsOcc& C, int grid)
{
#define MGS_CMP_SHF(SHF)                                                                                                      \
  hipLaunchKernelGGL((k_composite<MODE, SHF>), dim3(grid), dim3(256), 0, stream, C, L.ranges, L.valX, L.valY, L.planPairs, L.rec, \
                     L.image, L.fmt, L.ctr, L.outDepth, L.outSplatId, L.dArgs, L.outNormal)
  switch(L.shFormat)
  {
    case 0: MGS_CMP_SHF(0); break;
    case 1: MGS_CMP_SHF(1); break;
    default: MGS_CMP_SHF(2); break;
  }
#undef MGS_CMP_SHF
}

void launchComposite(hipStream_t stream, const CompositeLaunch& L)
{
  const FrameConst& F = L.A->f;
  if(F.stripRow1 <= F.stripRow0)
    return;
  const bool noGauss = (F.debugFlags & 4) != 0;
  int mode = (F.alphaMode != 0 ? kCmpAlphaSum : 0) | (noGauss ? kCmpNoGauss : 0) | (F.surfaceOutputs ? kCmpSurface : 0)
             | (L.occ.depth ? kCmpOccluder : 0);
  // stochastic splats: opaque writes, so the alpha mode is irrelevant; with the opacity gaussian disabled every fragment is
  // accepted (alpha 1) and the plain path already yields the nearest fragment.  (No occluder bit: mgs_render refuses that frame.)
  if(F.stochastic && !noGauss)
    mode = kCmpStochastic | (F.surfaceOutputs ? kCmpSurface : 0);
  CompositeArgsOcc C    = compositeArgs(L);
  const int        grid = compositeRegionGrid(F);
#ifdef MGS_CMP_TRACE
  static uint64_t* traceBuf = nullptr;
  const char*      tracePath = std::getenv("MGS_CMP_TRACE_FILE");
  const size_t     traceN = (size_t)grid * 10;
  if(tracePath)
  {
    if(!traceBuf)
      (void)hipMalloc(&traceBuf, (size_t)1 << 24);
    (void)hipMemsetAsync(traceBuf, 0, traceN * 8, stream);
    C.trace = traceBuf;
  }
#endif
  // the instantiated modes, each in three SH formats: alpha sum x opacity gaussian x surface outputs, plain and with an occluder;
  // stochastic splats with and without surface outputs
#define MGS_CMP(M) case(M): launchCompositeMode<(M)>(stream, L, C, grid); break;
#define MGS_CMP_AGS(X)                                                                                                  \
  MGS_CMP(X) MGS_CMP(X | kCmpAlphaSum) MGS_CMP(X | kCmpNoGauss) MGS_CMP(X | kCmpNoGauss | kCmpAlphaSum)                 \
  MGS_CMP(X | kCmpSurface) MGS_CMP(X | kCmpSurface | kCmpAlphaSum) MGS_CMP(X | kCmpSurface | kCmpNoGauss)               \
  MGS_CMP(X | kCmpSurface | kCmpNoGauss | kCmpAlphaSum)
  switch(mode)
  {
    MGS_CMP_AGS(0)
    MGS_CMP_AGS(kCmpOccluder)
    MGS_CMP(kCmpStochastic)
    MGS_CMP(kCmpStochastic | kCmpSurface)
    default:
      std::fprintf(stderr, "launchComposite: no k_composite instantiation for mode %d\n", mode);
      std::abort();
  }
#undef MGS_CMP_AGS
#undef MGS_CMP
#ifdef MGS_CMP_TRACE
  if(tracePath)
  {
    (void)hipStreamSynchronize(stream);
    std::vector<uint64_t> h(traceN);
    (void)hipMemcpy(h.data(), traceBuf, traceN * 8, hipMemcpyDeviceToHost);
    if(FILE* fp = std::fopen(tracePath, "wb"))
    {
      std::fwrite(h.data(), 8, traceN, fp);
      std::fclose(fp);
    }
  }
#endif
}

}  // namespace mgs
