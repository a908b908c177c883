// k_composite_gut.hip — the compositors of the 3DGUT raster pipeline (PIPELINE_MESH_3DGUT) for gfx950: SURVEY.md §8f rank 3.
//
// Replaces
//   shaders/threedgut_raster.frag.slang:87-183    per-fragment: ray generation (cameras.h.slang:27-82), model-space ray,
//                                                  particleProcessHitGut (threedgrt.h.slang:57-135,238-278), blend source
// Structure: k_composite_gut walks the bin lists of the 96-byte GutRecs that k_project_gut.hip wrote
// nearest-first like k_composite (one workgroup per 16x16 tile, one pixel per thread, records staged through
// LDS in list order) and evaluates the particle response per fragment.  This pipeline is a "next" row: correct and
// reasonably fast, not tuned like the 3DGS compositor.
// Depth of field and stochastic splats are the XT variant of the compositor (random numbers: kernels_common.h).
// Kernel degrees other than 2 and the surface side outputs run in the XT variant too.  Not built (stated in DESIGN.md):
// rolling shutter (untested in the reference).
#include <cstdio>
#include <cstdlib>

#include "composite_common.h"
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "sh_eval.h"
#include "surface_normal.h"

namespace mgs {

// ---- compositor: one workgroup per 16x16 tile, one pixel per thread -------------------------------------------------------
constexpr int kGutBatch = 256;  // list entries scanned per round == staging capacity

// XT 1 (2: + the non-quadratic particle kernels, the surface side outputs and their LDS; 3: + NORMAL_METHOD_ISO_SURFACE): the variant with depth of field (frag.slang:104-109, cameras.h.slang:85-108), stochastic splats (:150-172) and/or
// a particle kernel other than the quadratic one, and/or the surface side outputs (picked depth, splat id, integrated normal)
// OCC: occluder (mgs_frame_set_occluder): fragments depth-tested against occDepth with the record's key depth (kernels_common.h:
// keyDepthNdcZ, staged in the free lane of the record's second quad), the caller's colour added behind them; occStop (lists sorted by
// the depth key): a pixel whose last record failed the test is finished, every later record fails too
struct GutOccArgs
{
  const float*  depth;  // [height][width] window depth of the caller's geometry
  const float4* color;  // [height][width] linear RGBA of that geometry, nullptr = transparent black
  int32_t       stop;   // 1: the lists are sorted by the depth key
};
template <class T>
__device__ __forceinline__ const T& firstArg(const T& a) { return a; }
// (OCC's extra argument is a parameter pack so that the instantiations without an occluder keep their argument block as it was)
template <int SHF, int XT, bool OCC = false, class... OccArg>
__global__ __launch_bounds__(256) void k_composite_gut(const FrameArgs* __restrict__ Ap, const uint2* __restrict__ ranges,
                                                       const uint32_t* __restrict__ valX, const uint32_t* __restrict__ valY,
                                                       const SortPlan* __restrict__ plan, const GutRec* __restrict__ rec,
                                                       void* __restrict__ outImage, int fmt, FrameCounters* __restrict__ ctr,
                                                       float* __restrict__ outDepth, uint32_t* __restrict__ outSplatId,
                                                       float4* __restrict__ outNormal, const OccArg... occArg)
{
  static_assert(sizeof...(OccArg) == (OCC ? 1 : 0), "the occluder variant takes one GutOccArgs");
  const float*  occDepth = nullptr;
  const float4* occColor = nullptr;
  int           occStop  = 0;
  if constexpr(OCC)
  {
    const GutOccArgs& O = firstArg(occArg...);
    occDepth = O.depth;
    occColor = O.color;
    occStop  = O.stop;
  }
  __shared__ float4   s_r[kGutBatch][6];
  __shared__ uint32_t s_gid[XT ? kGutBatch : 1];
  __shared__ float4   s_n[XT >= 2 ? kGutBatch : 1];  // surface outputs (XT 2): world normal of the record (.w = 1: minus the pixel's ray)
  __shared__ float    s_z[XT >= 2 ? kGutBatch : 1];  //                         fragCoord.z of the record's quad
  __shared__ float4   s_iso[XT == 3 ? kGutBatch : 1][3];  // NORMAL_METHOD_ISO_SURFACE: canonical -> world normal matrix (surface_normal.h)
  __shared__ uint32_t s_wc[4];
  __shared__ uint32_t s_live;
  const FrameConst& F = Ap->f;
  const int t = threadIdx.x, lane = laneId(), w = t >> 6;
  const int tilesInStrip = F.tilesX * (F.stripRow1 - F.stripRow0);
  if((int)blockIdx.x >= tilesInStrip)
    return;
  const int tx = (int)blockIdx.x % F.tilesX, ty = F.stripRow0 + (int)blockIdx.x / F.tilesX;
  const int px = tx * kTilePx + (t & 15), py = ty * kTilePx + (t >> 4);
  const bool inside = px < F.width && py < F.height;
  const float pcx = (float)px + 0.5f, pcy = (float)py + 0.5f;
  const float bcx = (float)(tx * kTilePx) + 8.0f, bcy = (float)(ty * kTilePx) + 8.0f;
  // ray of this pixel in world space (frag.slang:101-111)
  float dxw, dyw, dzw;
  const bool rayOk = gutPixelRay(F, pcx, pcy, dxw, dyw, dzw);
  // depth of field: the ray leaves a random point of the lens and still passes through the focal point of the pinhole ray
  float    lensX = 0.0f, lensY = 0.0f, lensZ = 0.0f;
  uint32_t seedPx = 0u;
  const bool stoch = XT && F.stochastic != 0 && !((F.debugFlags & 4) != 0);
  if constexpr(XT != 0)
  {
    seedPx = rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId);  // int(position.x), int(position.y), frameSampleId
    if(F.dofMode != 0)
      gutLensSample<false>(F, seedPx, lensX, lensY, lensZ, dxw, dyw, dzw);
  }
  const bool  early   = F.alphaMode == 0;
  const bool  noGauss = (F.debugFlags & 4) != 0;
  const float tMin    = early ? 1.0e-4f : -1.0f;
  const uint32_t* vals = plan->finalSel ? valY : valX;
  const int      bin   = (ty >> F.binShiftY) * F.binsX + (tx >> F.binShiftX);
  const uint2    range = ranges[bin];
  // a pixel without a ray (outside the image, outside the fisheye's field of view: frag.slang:96-100 discards) starts below every
  // tMin, the additive-alpha mode's -1 included, so that no record hits it: its count is 0 as its coverage is
  float T = (inside && rayOk) ? 1.0f : -2.0f, cr = 0.f, cg = 0.f, cb = 0.f, asum = 0.f;
  float occD = 0.0f;          // this pixel's bound depth (-inf outside the image; NaN passes nothing)
  bool  occBehind = !inside;  // the last record seen lies behind it
  if constexpr(OCC)
    occD = inside ? occDepth[(size_t)py * F.width + px] : -__builtin_huge_valf();
  const bool surf = XT >= 2 && F.surfaceOutputs != 0;
  float      nx = 0.f, ny = 0.f, nz = 0.f, pickZ = 0.f;
  uint32_t   pickId = 0xFFFFFFFFu;
  uint32_t hi = range.y;
  uint32_t statScanned = 0, statStaged = 0;
  while(hi > range.x)
  {
    // ---- stage: the next 256 nearest entries, culled against the tile, compacted in list order ----
    const uint32_t avail = hi - range.x;
    const bool     have  = (uint32_t)t < avail;
    uint32_t       g     = have ? vals[hi - 1u - (uint32_t)t] : 0u;
    float4         r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, -1.f, -1.f);
    if(have)
    {
      const float4* rp = reinterpret_cast<const float4*>(rec + g);
      r0 = rp[0];
      r1 = rp[1];
    }
    const bool     ok  = have && fabsf(r0.x - bcx) <= r1.z + 7.5f && fabsf(r0.y - bcy) <= r1.w + 7.5f;
    uint32_t       fill;
    const uint32_t pos = gutCompactSlot(ok, s_wc, lane, w, fill);
    if(ok)
    {
      const float4*  rp  = reinterpret_cast<const float4*>(rec + g);
      const float4   r2 = rp[2], r3 = rp[3], r4 = rp[4];
      float4         c5 = rp[5];
      // deferred shading (mesh.slang:142-148): base colour + SH in the splat's model coordinates, once per staged record.  The same
      // text as in k_composite_gut2, written out in both: as a shared function it changes the VGPR count of this kernel's
      // XT >= 2 instantiations, which use I and li below
      int k = 0;
      for(int i = 1; i < F.nInstances; ++i)
        if(g >= Ap->inst[i].globalOffset)
          k = i;
      const InstanceConst& I  = Ap->inst[k];
      const uint32_t       li = g - I.globalOffset;
      const float4         col = reinterpret_cast<const float4*>(I.rgbaF32)[li];
      float dx = I.centers[3 * (size_t)li] - I.camModel[0], dy = I.centers[3 * (size_t)li + 1] - I.camModel[1],
            dz = I.centers[3 * (size_t)li + 2] - I.camModel[2];
      const float dl = rsqrtf(dx * dx + dy * dy + dz * dz);
      dx *= dl; dy *= dl; dz *= dl;
      const bool shOnly = (F.debugFlags & 2) != 0;
      c5.x = shOnly ? 0.5f : col.x;
      c5.y = shOnly ? 0.5f : col.y;
      c5.z = shOnly ? 0.5f : col.z;
      const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
      if(deg > 0)
        addShRadiance<SHF>(I.sh, li, deg, dx, dy, dz, c5.x, c5.y, c5.z);
      // acceptance (threedgrt.h.slang:259-267) with two compares less per fragment: density > alphaCull, alpha = min(clamp,
      // response * density) > 1/255 and response > kMin  <=>  response > max(kMin, 1 / (255 density)) — a per-record cutoff
      // that takes the slot of the box extents (needed above only)
      const float rcut = (c5.w > F.alphaCull) ? fmaxf(F.kernelMinResponse, 1.0f / (255.0f * fmaxf(c5.w, 1e-30f))) : 3.0e38f;
      float zo = 0.0f;
      if constexpr(OCC)
        zo = keyDepthNdcZ(I.model, F.view, F.proj, I.centers[3 * (size_t)li], I.centers[3 * (size_t)li + 1], I.centers[3 * (size_t)li + 2]);
      s_r[pos][0] = r0;
      s_r[pos][1] = make_float4(r1.x, r1.y, rcut, zo);
      s_r[pos][2] = r2;
      s_r[pos][3] = r3;
      s_r[pos][4] = r4;
      s_r[pos][5] = c5;
      if constexpr(XT != 0)
      {
        s_gid[pos] = g;
        if constexpr(XT >= 2)
        {  // frag.slang:127-131 -> particleProcessHitGutWithNormal (threedgrt.h.slang:281-345): the max-density-plane normal is a
          // per-splat quantity (ray ORIGIN only) except for particles with two degenerate axes; no octahedral round trip here
          // (the normal is computed in the fragment shader, not carried through an interstage variable).  fragCoord.z: the
          // quad sits at the pinhole depth of the centre (mesh.slang:221-226)
          if constexpr(XT == 3)
          {  // the fragment's own normal: where its ray enters the kernel ellipsoid (threedgrt.h.slang:330-335, 423-497)
            float4 isoRec[3];
            splatIsoNormalRec(F, I, li, isoRec);
            s_iso[pos][0] = isoRec[0];
            s_iso[pos][1] = isoRec[1];
            s_iso[pos][2] = isoRec[2];
            s_n[pos]      = make_float4(isoRec[0].x, isoRec[0].y, isoRec[0].z, isoRec[0].w == 2.0f ? 1.0f : 0.0f);
          }
          else
          {
            s_n[pos] = splatWorldNormal(F, I, li, false);
          }
          const float  cpx = I.centers[3 * (size_t)li], cpy = I.centers[3 * (size_t)li + 1], cpz = I.centers[3 * (size_t)li + 2];
          const float* MV = I.modelView;
          const float* P  = F.proj;
          const float  tx = MV[0] * cpx + MV[4] * cpy + MV[8] * cpz + MV[12];
          const float  ty = MV[1] * cpx + MV[5] * cpy + MV[9] * cpz + MV[13];
          const float  tz = MV[2] * cpx + MV[6] * cpy + MV[10] * cpz + MV[14];
          const float  tw = MV[3] * cpx + MV[7] * cpy + MV[11] * cpz + MV[15];
          const float  cz = P[2] * tx + P[6] * ty + P[10] * tz + P[14] * tw;
          const float  cw = P[3] * tx + P[7] * ty + P[11] * tz + P[15] * tw;
          s_z[pos]        = cz * gRcp(cw);
        }
      }
    }
    if(t == 0)
      s_live = 0u;
    __syncthreads();
    statScanned += min(avail, (uint32_t)kGutBatch);
    statStaged += fill;
    hi -= min(avail, (uint32_t)kGutBatch);
    // ---- blend front to back ----
    for(uint32_t j = 0; j < fill; ++j)
    {
      const float4 a0 = s_r[j][0], a1 = s_r[j][1];
      const float  ddx = pcx - a0.x, ddy = pcy - a0.y;
      const bool   inQuad = fabsf(ddx * a0.z + ddy * a0.w) <= 1.0f && fabsf(ddx * a1.x + ddy * a1.y) <= 1.0f;
      const float4 b0 = s_r[j][2], b1 = s_r[j][3], b2 = s_r[j][4], c4 = s_r[j][5];
      // canonical ray direction ~ B d, origin ro; dist^2 = |g x ro|^2 / |g|^2  (threedgrt.h.slang:57-81)
      const float gx = b0.x * dxw + b0.y * dyw + b0.z * dzw;
      const float gy = b0.w * dxw + b1.x * dyw + b1.y * dzw;
      const float gz = b1.z * dxw + b1.w * dyw + b2.x * dzw;
      float rox = b2.y, roy = b2.z, roz = b2.w;
      if constexpr(XT != 0)
      {  // rayOrigin += randomAperturePos: canonical origin + B * offset
        rox += b0.x * lensX + b0.y * lensY + b0.z * lensZ;
        roy += b0.w * lensX + b1.x * lensY + b1.y * lensZ;
        roz += b1.z * lensX + b1.w * lensY + b2.x * lensZ;
      }
      const float kx = gy * roz - gz * roy, ky = gz * rox - gx * roz, kz = gx * roy - gy * rox;
      const float dist2 = (kx * kx + ky * ky + kz * kz) * gRcp(gx * gx + gy * gy + gz * gz);
      float resp = __expf(-0.5f * dist2);                            // quadratic kernel, :127-131
      if constexpr(XT >= 2)
        if(F.kernelDegree != 2)  // degree 2 is the line above (kernelResponse's default); calling without the test changes the VGPR count
          resp = kernelResponse(F.kernelDegree, dist2);
      const float al    = fminf(F.alphaClamp, resp * c4.w);          // :263
      bool        hit   = inQuad && resp > a1.z && T >= tMin;
      if constexpr(OCC)
        hit = hit && a1.w <= occD;  // the depth test: LESS_OR_EQUAL, one z per record
      float       op    = hit ? (noGauss ? 1.0f : al) : 0.0f;
      if constexpr(XT != 0)
      {
        if(stoch)
        {  // frag.slang:153-158; primitive id as in the 3DGS compositor (k_composite.hip): 2 * (id mod 32) + triangle
          const uint32_t gid = s_gid[j];
          const float    qu = ddx * a0.z + ddy * a0.w, qv = ddx * a1.x + ddy * a1.y;
          uint32_t       h  = rngXxhash32(seedPx, gid, 2u * (gid & 31u) + (qu > qv ? 0u : 1u));
          op                = (hit && rngRand(h) < op) ? 1.0f : 0.0f;
        }
      }
      const float wgt   = op * T;
      cr += wgt * c4.x;
      cg += wgt * c4.y;
      cb += wgt * c4.z;
      asum += op;
      T -= wgt;
      if constexpr(XT >= 2)
      {
        if(surf)
        {  // frag.slang:195-228: normal attachment "under"-blended with (normal * opacity, opacity); picked depth = the
          // fragment after which the transmittance is below the threshold, and the splat that set it
          float4 n1  = s_n[j];
          bool   ray = n1.w != 0.0f;  // degenerate particle: -rayDirection (model -> world: minus the pixel's world ray)
          if constexpr(XT == 3)
          if(wgt != 0.0f && !ray && s_iso[j][0].w == 0.0f)
          {  // raySphereIntersection(canonical origin, canonical direction, 3, 0, inf), threedgrt.h.slang:502-540.  The same two
            // roots, written around the point of closest approach (t_mid = -(o.g)/(g.g), half chord = sqrt((9 - dist^2)/(g.g)))
            // instead of b^2 - 4ac: the canonical origin lies hundreds of radii from a small particle and the discriminant of
            // the textbook form cancels in fp32 (the oracle follows the shader; tests/test_oracle_cpu.py has the numbers)
            const float qa = gx * gx + gy * gy + gz * gz;
            const float tm = -(rox * gx + roy * gy + roz * gz) * gRcp(qa);
            const float dd = 9.0f - dist2;
            ray = true;  // no intersection in front of the origin: -rayDirection (:468-472)
            if(dd >= 0.0f)
            {
              const float half = sqrtf(dd * gRcp(qa));
              const float th   = (tm - half >= 0.0f) ? tm - half : tm + half;
              if(th >= 0.0f)
              {
                const float  hx = rox + th * gx, hy = roy + th * gy, hz = roz + th * gz;
                const float4 i0 = s_iso[j][0], i1 = s_iso[j][1], i2 = s_iso[j][2];
                const float  wx = i0.x * hx + i0.y * hy + i0.z * hz;
                const float  wy = i1.x * hx + i1.y * hy + i1.z * hz;
                const float  wz = i2.x * hx + i2.y * hy + i2.z * hz;
                const float  rl = rsqrtf(wx * wx + wy * wy + wz * wz);
                n1  = make_float4(wx * rl, wy * rl, wz * rl, 0.0f);
                ray = false;
              }
            }
          }
          nx += wgt * (ray ? -dxw : n1.x);
          ny += wgt * (ray ? -dyw : n1.y);
          nz += wgt * (ray ? -dzw : n1.z);
          if(op > 0.0f && pickZ == 0.0f && T < F.depthIsoThreshold)
          {
            pickZ  = s_z[j];
            pickId = s_gid[j];
          }
        }
      }
    }
    if constexpr(OCC)
    {
      if(fill > 0u)
        occBehind = !inside || s_r[fill - 1u][1].w > occD;  // (the batch's last record has its largest z)
    }
    if(early || (OCC && occStop != 0))
    {
      if((T >= tMin) && !(OCC && occStop != 0 && occBehind))
        s_live = 1u;  // benign race: every writer stores 1
      __syncthreads();
      if(s_live == 0u)
        break;
    }
    else
      __syncthreads();
  }
  if(t == 0)
  {
    FrameStatLine* stat = frameStatLineFromPairs(plan, blockIdx.x >> 3);
    atomicAdd(&stat->scanned, statScanned);
    atomicAdd(&stat->staged, statStaged);
  }
  if(!inside)
    return;
  float alphaOut = F.alphaMode == 1 ? asum : 1.0f - ((inside && rayOk) ? T : 1.0f);
  const size_t pix = (size_t)py * F.width + px;
  if constexpr(OCC)
  {  // the caller's geometry behind the splats (k_composite.hip has the rule); a pixel without a valid ray has T = 1 here
    if(occColor)
    {
      const float4 bg = occColor[pix];
      const float  Tb = rayOk ? T : 1.0f;
      cr += Tb * bg.x;
      cg += Tb * bg.y;
      cb += Tb * bg.z;
      if(F.alphaMode == 1)
        alphaOut += bg.w;
    }
  }
  if constexpr(XT >= 2)
  {
    if(surf)
    {
      outDepth[pix]   = pickZ;
      outSplatId[pix] = pickId;
      outNormal[pix]  = make_float4(nx, ny, nz, 1.0f - ((inside && rayOk) ? T : 1.0f));
    }
  }
  storePixel(outImage, fmt, pix, cr, cg, cb, alphaOut);
}


// ---- packed compositor (plain mode: quadratic kernel, coverage alpha, no depth of field / stochastic / surface outputs) -------------
// The geometry of the 3DGS compositor (k_composite.hip): one workgroup per 32x16-pixel region, one wave per 16x8 quarter, TWO pixels
// per lane (x and x + 8) so that the per-fragment arithmetic runs on gfx950's packed-fp32 instructions with the particle's
// parameters broadcast — the one-pixel-per-lane kernel above spends ~45 instructions per (record, pixel), this one ~50 per
// (record, pixel PAIR) — and a region twice as large halves the list entries scanned per pixel.  Records are culled against the
// region, compacted in list order into an LDS batch together with a 4-bit mask of the quarters their quad's box touches, shaded
// there (deferred SH), and each wave walks only the records of its quarter.  Saturation is a per-fragment predicate (T >= 1e-4),
// so the frame does not depend on batch boundaries (strips == full frame).
typedef float gv2f __attribute__((ext_vector_type(2)));
constexpr int kGut2Cap = 256;  // LDS batch capacity == entries scanned per round

// XT 1: + depth of field (a lens offset per pixel) and stochastic splats (quadratic kernel only)
template <int SHF, int XT>
__global__ __launch_bounds__(256) void k_composite_gut2(const FrameArgs* __restrict__ Ap, const uint2* __restrict__ ranges,
                                                        const uint32_t* __restrict__ valX, const uint32_t* __restrict__ valY,
                                                        const SortPlan* __restrict__ plan, const GutRec* __restrict__ rec,
                                                        void* __restrict__ outImage, int fmt, FrameCounters* __restrict__ ctr)
{
  __shared__ float4   s_r[kGut2Cap][6];
  __shared__ uint8_t  s_m[kGut2Cap];
  __shared__ uint32_t s_gid[XT ? kGut2Cap : 1];
  __shared__ uint32_t s_wc[4];
  const FrameConst& F = Ap->f;
  const int t = threadIdx.x, lane = laneId(), w = t >> 6;
  // region order as in k_composite (k_composite.hip; the grid: compositeRegionGrid): all regions of a bin on one XCD (workgroup b runs on XCD b % 8; they read
  // the same list), consecutive bins on different XCDs, bins taken longest list first (ranked by the binning stage)
  const int colsX    = (F.tilesX + 1) >> 1;
  const int bw       = 1 << (F.binShiftX - 1), bh = 1 << F.binShiftY;  // bin size in regions
  const int binRow0  = F.stripRow0 >> F.binShiftY;
  const int binRows  = ((F.stripRow1 - 1) >> F.binShiftY) - binRow0 + 1;
  const int perBin   = bw * bh;
  const int seq      = (int)(blockIdx.x >> 3);
  const int ord      = (seq / perBin) * 8 + (int)(blockIdx.x & 7);  // bin ordinal
  const int inBin    = seq % perBin;
  const bool ordered = directBinTables(plan)->binOrderValid != 0u;
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
  const int tx  = cx2 * 2;
  const int qx0 = tx * kTilePx + (w & 1) * 16, qy0 = ty * kTilePx + (w >> 1) * 8;
  const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);  // second pixel: px + 8
  const bool in0 = px < F.width && py < F.height, in1 = px + 8 < F.width && py < F.height;
  const gv2f  pcx = {(float)px + 0.5f, (float)px + 8.5f};
  const float pcy = (float)py + 0.5f;
  const float bcx = (float)(tx * kTilePx) + 16.0f, bcy = (float)(ty * kTilePx) + 8.0f;  // region centre
  gv2f dxw, dyw, dzw;
  bool ok0, ok1;
  {
    float a, b, c;
    ok0 = gutPixelRay(F, pcx.x, pcy, a, b, c);
    dxw.x = a; dyw.x = b; dzw.x = c;
    ok1 = gutPixelRay(F, pcx.y, pcy, a, b, c);
    dxw.y = a; dyw.y = b; dzw.y = c;
  }
  // depth of field (frag.slang:104-109, cameras.h.slang:85-108): one lens sample per pixel and frame
  gv2f     lensX = {0.f, 0.f}, lensY = {0.f, 0.f}, lensZ = {0.f, 0.f};
  uint32_t seed0 = 0u, seed1 = 0u;
  if constexpr(XT != 0)
  {
    seed0 = rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId);
    seed1 = rngXxhash32((uint32_t)px + 8u, (uint32_t)py, (uint32_t)F.frameSampleId);
    if(F.dofMode != 0)
    {
#pragma unroll
      for(int h = 0; h < 2; ++h)
      {
        float lx, ly, lz, dx = h ? dxw.y : dxw.x, dy = h ? dyw.y : dyw.x, dz = h ? dzw.y : dzw.x;
        gutLensSample<true>(F, h ? seed1 : seed0, lx, ly, lz, dx, dy, dz);
        if(h) { lensX.y = lx; lensY.y = ly; lensZ.y = lz; dxw.y = dx; dyw.y = dy; dzw.y = dz; }
        else  { lensX.x = lx; lensY.x = ly; lensZ.x = lz; dxw.x = dx; dyw.x = dy; dzw.x = dz; }
      }
    }
  }
  const bool  stoch   = XT && F.stochastic != 0 && !((F.debugFlags & 4) != 0);
  const bool  noGauss = (F.debugFlags & 4) != 0;
  constexpr float tMin = 1.0e-4f;
  const uint32_t* vals = plan->finalSel ? valY : valX;
  const int      bin   = (ty >> F.binShiftY) * F.binsX + (tx >> F.binShiftX);
  const uint2    range = ranges[bin];
  gv2f T = {(in0 && ok0) ? 1.0f : 0.0f, (in1 && ok1) ? 1.0f : 0.0f}, cr = {0.f, 0.f}, cg = {0.f, 0.f}, cb = {0.f, 0.f};
  uint32_t hi = range.y;
  uint32_t statScanned = 0, statStaged = 0;
  while(hi > range.x)
  {
    // ---- stage: the next 256 nearest entries, culled against the region, compacted in list order ----
    const uint32_t avail = hi - range.x;
    const bool     have  = (uint32_t)t < avail;
    const uint32_t g     = have ? vals[hi - 1u - (uint32_t)t] : 0u;
    float4         r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, -1.f, -1.f);
    if(have)
    {
      const float4* rp = reinterpret_cast<const float4*>(rec + g);
      r0 = rp[0];
      r1 = rp[1];
    }
    // pixel centres of the region span bcx +- 15.5, bcy +- 7.5
    const bool     ok  = have && fabsf(r0.x - bcx) <= r1.z + 15.5f && fabsf(r0.y - bcy) <= r1.w + 7.5f;
    uint32_t       fill;
    const uint32_t pos = gutCompactSlot(ok, s_wc, lane, w, fill);
    if(ok)
    {
      const float4*  rp  = reinterpret_cast<const float4*>(rec + g);
      const float4   r2 = rp[2], r3 = rp[3], r4 = rp[4];
      float4         c5 = rp[5];
      // deferred shading, as in k_composite_gut (which says why it is no function of gut_common.h)
      int k = 0;
      for(int i = 1; i < F.nInstances; ++i)
        if(g >= Ap->inst[i].globalOffset)
          k = i;
      const InstanceConst& I  = Ap->inst[k];
      const uint32_t       li = g - I.globalOffset;
      const float4         col = reinterpret_cast<const float4*>(I.rgbaF32)[li];
      float dx = I.centers[3 * (size_t)li] - I.camModel[0], dy = I.centers[3 * (size_t)li + 1] - I.camModel[1],
            dz = I.centers[3 * (size_t)li + 2] - I.camModel[2];
      const float dl = rsqrtf(dx * dx + dy * dy + dz * dz);
      dx *= dl; dy *= dl; dz *= dl;
      const bool shOnly = (F.debugFlags & 2) != 0;
      c5.x = shOnly ? 0.5f : col.x;
      c5.y = shOnly ? 0.5f : col.y;
      c5.z = shOnly ? 0.5f : col.z;
      const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
      if(deg > 0)
        addShRadiance<SHF>(I.sh, li, deg, dx, dy, dz, c5.x, c5.y, c5.z);
      if(!(c5.w > F.alphaCull))
        c5.w = 0.0f;  // particleProcessHitGut rejects the whole particle (density <= alphaCullThreshold): no fragment can pass
      // acceptance of particleProcessHitGut (threedgrt.h.slang:259-267) as ONE compare per pixel: alpha = min(clamp, response *
      // density) > 1/255 and response > kernelMinResponse  <=>  response > max(kMin, 1 / (255 density))  <=>  (quadratic
      // kernel) dist^2 < -2 ln(that): a per-record cutoff, staged in the slot of the box extents (used above only)
      const float rcut  = fmaxf(F.kernelMinResponse, 1.0f / (255.0f * fmaxf(c5.w, 1e-30f)));
      const float d2cut = (c5.w > 0.0f && rcut < 1.0f) ? -2.0f * __logf(rcut) : -1.0f;
      s_r[pos][0] = r0;
      s_r[pos][1] = make_float4(r1.x, r1.y, d2cut, 0.0f);
      s_r[pos][2] = r2;
      s_r[pos][3] = r3;
      s_r[pos][4] = r4;
      s_r[pos][5] = c5;
      if constexpr(XT != 0)
        s_gid[pos] = g;
      // quarters (16 x 8 pixels; centres x in [bcx-15.5,bcx-0.5] / [bcx+0.5,bcx+15.5], y in [bcy-7.5,bcy-0.5] / [bcy+0.5,bcy+7.5])
      // the box of the quad touches
      const bool xl = r0.x - r1.z <= bcx - 0.5f, xr = r0.x + r1.z >= bcx + 0.5f;
      const bool yt = r0.y - r1.w <= bcy - 0.5f, yb = r0.y + r1.w >= bcy + 0.5f;
      s_m[pos] = (uint8_t)(((xl && yt) ? 1u : 0u) | ((xr && yt) ? 2u : 0u) | ((xl && yb) ? 4u : 0u) | ((xr && yb) ? 8u : 0u));
    }
    __syncthreads();
    statScanned += min(avail, (uint32_t)kGut2Cap);
    statStaged += fill;
    hi -= min(avail, (uint32_t)kGut2Cap);
    // ---- blend front to back: 64 records at a time, this wave's hit set from the quarter masks ----
    for(uint32_t j0 = 0; j0 < fill; j0 += 64)
    {
      const uint32_t jl   = j0 + (uint32_t)lane;
      const bool     mine = jl < fill && ((s_m[jl] >> w) & 1u);
      uint64_t       hits = __ballot(mine);
      while(hits != 0ull)
      {
        const uint32_t j = j0 + (uint32_t)__builtin_ctzll(hits);
        hits &= hits - 1ull;
        const float4 a0 = s_r[j][0], a1 = s_r[j][1], b0 = s_r[j][2], b1 = s_r[j][3], b2 = s_r[j][4], c4 = s_r[j][5];
        const gv2f   ddx = pcx - a0.x;
        const float  ddy = pcy - a0.y;
        const gv2f   qu = ddx * a0.z + ddy * a0.w, qv = ddx * a1.x + ddy * a1.y;
        // canonical ray direction ~ B d, origin ro; dist^2 = |g x ro|^2 / |g|^2  (threedgrt.h.slang:57-81)
        const gv2f gx = dxw * b0.x + (dyw * b0.y + dzw * b0.z);
        const gv2f gy = dxw * b0.w + (dyw * b1.x + dzw * b1.y);
        const gv2f gz = dxw * b1.z + (dyw * b1.w + dzw * b2.x);
        gv2f rox = {b2.y, b2.y}, roy = {b2.z, b2.z}, roz = {b2.w, b2.w};
        if constexpr(XT != 0)
        {  // rayOrigin += randomAperturePos: canonical origin + B * offset
          rox += lensX * b0.x + (lensY * b0.y + lensZ * b0.z);
          roy += lensX * b0.w + (lensY * b1.x + lensZ * b1.y);
          roz += lensX * b1.z + (lensY * b1.w + lensZ * b2.x);
        }
        const gv2f kx = gy * roz - gz * roy, ky = gz * rox - gx * roz, kz = gx * roy - gy * rox;
        const gv2f kk = kx * kx + (ky * ky + kz * kz), gg = gx * gx + (gy * gy + gz * gz);
        const gv2f dist2 = {kk.x * gRcp(gg.x), kk.y * gRcp(gg.y)};
        const gv2f resp  = {__expf(-0.5f * dist2.x), __expf(-0.5f * dist2.y)};  // quadratic kernel, :127-131
        const gv2f raw   = resp * c4.w;
        const gv2f al    = {fminf(F.alphaClamp, raw.x), fminf(F.alphaClamp, raw.y)};  // :263
        const bool h0 = fmaxf(fabsf(qu.x), fabsf(qv.x)) <= 1.0f && dist2.x < a1.z && T.x >= tMin;
        const bool h1 = fmaxf(fabsf(qu.y), fabsf(qv.y)) <= 1.0f && dist2.y < a1.z && T.y >= tMin;
        gv2f op  = {h0 ? (noGauss ? 1.0f : al.x) : 0.0f, h1 ? (noGauss ? 1.0f : al.y) : 0.0f};
        if constexpr(XT != 0)
        {
          if(stoch)
          {  // frag.slang:153-158; primitive id as in the other compositors: 2 * (id mod 32) + triangle (0: u > v)
            const uint32_t gid = s_gid[j], prim = 2u * (gid & 31u);
            uint32_t       q0 = rngXxhash32(seed0, gid, prim + (qu.x > qv.x ? 0u : 1u));
            uint32_t       q1 = rngXxhash32(seed1, gid, prim + (qu.y > qv.y ? 0u : 1u));
            op.x = (h0 && rngRand(q0) < op.x) ? 1.0f : 0.0f;
            op.y = (h1 && rngRand(q1) < op.y) ? 1.0f : 0.0f;
          }
        }
        const gv2f wgt = op * T;
        cr += wgt * c4.x;
        cg += wgt * c4.y;
        cb += wgt * c4.z;
        T -= wgt;
      }
    }
    // all four waves saturated: stop fetching (the predicate above already keeps saturated pixels unchanged)
    if(__syncthreads_and((T.x >= tMin || T.y >= tMin) ? 0 : 1))
      break;
  }
  if(t == 0)
  {
    FrameStatLine* stat = frameStatLineFromPairs(plan, blockIdx.x >> 3);
    atomicAdd(&stat->scanned, statScanned);
    atomicAdd(&stat->staged, statStaged);
  }
#pragma unroll
  for(int h = 0; h < 2; ++h)
  {
    if(!(h ? in1 : in0))
      continue;
    const bool  rok = h ? ok1 : ok0;
    const float r = h ? cr.y : cr.x, g = h ? cg.y : cg.x, b = h ? cb.y : cb.x;
    const float alphaOut = 1.0f - (rok ? (h ? T.y : T.x) : 1.0f);
    const size_t pix = (size_t)py * F.width + (size_t)(px + 8 * h);
    storePixel(outImage, fmt, pix, r, g, b, alphaOut);
  }
}

// ---------------------------------------------------------------------------------------------
[[noreturn]] static void unlisted(int v)
{
  std::fprintf(stderr, "launchCompositeGut: no compositor instantiation for variant %d\n", v);
  std::abort();
}

template <int SHF, int XT, bool OCC>
static void launchGutVariant(hipStream_t stream, const CompositeLaunch& L, int tiles)
{
  if constexpr(OCC)
  {
    const GutOccArgs occArgs{L.occ.depth, reinterpret_cast<const float4*>(L.occ.color), L.occ.sortedByKey ? 1 : 0};
    hipLaunchKernelGGL((k_composite_gut<SHF, XT, true, GutOccArgs>), dim3(tiles), dim3(256), 0, stream, L.dArgs, L.ranges, L.valX, L.valY,
                       L.planPairs, L.recGut, L.image, L.fmt, L.ctr, L.outDepth, L.outSplatId, L.outNormal, occArgs);
  }
  else
    hipLaunchKernelGGL((k_composite_gut<SHF, XT>), dim3(tiles), dim3(256), 0, stream, L.dArgs, L.ranges, L.valX, L.valY, L.planPairs,
                       L.recGut, L.image, L.fmt, L.ctr, L.outDepth, L.outSplatId, L.outNormal);
}

void launchCompositeGut(hipStream_t stream, const CompositeLaunch& L)
{
  const FrameConst& F     = L.A->f;
  const int         tiles = F.tilesX * (F.stripRow1 - F.stripRow0);
  if(tiles <= 0)
    return;
  const int  shf  = L.shFormat == 0 ? 0 : L.shFormat == 1 ? 1 : 2;
  const bool lens = F.dofMode != 0 || F.stochastic != 0;  // depth of field and / or stochastic splats
  const int  occ  = L.occ.depth ? 1 : 0;
  // the quadratic-kernel modes without side outputs and without an occluder run on the packed two-pixels-per-lane compositor
  if(F.kernelDegree == 2 && F.surfaceOutputs == 0 && (F.alphaMode == 0 || F.stochastic != 0) && !occ)
  {
#define MGS_GUT2(SHF, XT) case(SHF) * 2 + (XT):                                                                                       \
    hipLaunchKernelGGL((k_composite_gut2<SHF, XT>), dim3(compositeRegionGrid(F)), dim3(256), 0, stream, L.dArgs, L.ranges, L.valX, L.valY, \
                       L.planPairs, L.recGut, L.image, L.fmt, L.ctr);                                                                 \
    return;
    switch(shf * 2 + (lens ? 1 : 0))
    {
      MGS_GUT2(0, 0) MGS_GUT2(0, 1) MGS_GUT2(1, 0) MGS_GUT2(1, 1) MGS_GUT2(2, 0) MGS_GUT2(2, 1)
      default: unlisted(shf * 2 + (lens ? 1 : 0));
    }
#undef MGS_GUT2
  }
  // the one-pixel-per-lane compositor's XT (see the kernel); a frame with an occluder runs on XT >= 1, whatever its mode
  const bool surf = F.surfaceOutputs != 0;
  const int  xt   = (surf && F.normalMethod == 1) ? 3 : (surf || F.kernelDegree != 2) ? 2 : (lens || occ) ? 1 : 0;
  // the instantiated variants, each in three SH formats: XT 0-3 without an occluder, XT 1-3 with one
#define MGS_GUT(SHF, XT, OCC) case(SHF) * 8 + (XT) * 2 + (OCC): launchGutVariant<SHF, XT, (OCC) != 0>(stream, L, tiles); break;
#define MGS_GUT_SHF(SHF) \
  MGS_GUT(SHF, 0, 0) MGS_GUT(SHF, 1, 0) MGS_GUT(SHF, 2, 0) MGS_GUT(SHF, 3, 0) MGS_GUT(SHF, 1, 1) MGS_GUT(SHF, 2, 1) MGS_GUT(SHF, 3, 1)
  switch(shf * 8 + xt * 2 + occ)
  {
    MGS_GUT_SHF(0) MGS_GUT_SHF(1) MGS_GUT_SHF(2)
    default: unlisted(shf * 8 + xt * 2 + occ);
  }
#undef MGS_GUT_SHF
#undef MGS_GUT
}

}  // namespace mgs
