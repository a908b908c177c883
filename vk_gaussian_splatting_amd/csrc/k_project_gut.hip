// k_project_gut.hip — the per-splat front end of the 3DGUT raster pipeline (PIPELINE_MESH_3DGUT) for gfx950: SURVEY.md §8f rank 3.
//
// Replaces
//   shaders/threedgut_raster.mesh.slang:111-254   per-splat front end: colour + SH, alpha cull, unscented projection,
//                                                  quad extent (conic / eigen), quad placement
//   shaders/threedgut.h.slang:26-163              threedgutParticleProjection (7 sigma points, GUT_* of
//                                                  threedgut_definitions.h.slang), threedgutProjectedExtentConicOpacity
//   shaders/threedgut_camera_projections.h.slang:84-201  perfect pinhole / fisheye projection, global shutter
// Shared with the 3DGS path and unchanged: depth keys + frustum cull (dist.comp.slang), the key sort, the per-bin lists.
// Structure: k_project_gut is k_project's phase 1 (key, cull, ordered compaction: same code, same bits) followed by the
// 3DGUT front end for the survivors; it writes one 96-byte GutRec per sorted splat (composited by k_composite_gut.hip).
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "partition_cull.h"
#include "slot_emit.h"

namespace mgs {

constexpr int kGutThreads = 256;
constexpr int kGutItems   = 8;
constexpr int kGutPart    = kGutThreads * kGutItems;  // == the project kernel's partition: same slots, same sort input

// projectPointWithShutter (global shutter) + projectPoint for the perfect pinhole / fisheye models.  `cam` is the
// view-space point with z negated (RUB -> RUF: the flips of :188-196 amount to F (R p + t), F = diag(1,1,-1)).
__device__ __forceinline__ bool gutProjectCam(const FrameConst& F, float cx, float cy, float cz, float& ox, float& oy)
{
  const float resx = (float)F.width, resy = (float)F.height;
  bool        ok;
  if(F.cameraModel == 1)
  {  // projectPointFisheye, radial coefficients 0: :151-176
    const float rho       = fmaxf(gutStableNorm2(cx, cy), 1e-7f);
    const float thetaFull = atan2f(rho, cz);
    const float theta     = fminf(thetaFull, F.gutMaxAngle);
    const float delta     = theta * gRcp(rho);
    ox                    = F.gutFocal[0] * cx * delta + resx * 0.5f;
    oy                    = F.gutFocal[1] * cy * delta + resy * 0.5f;
    ok                    = theta < F.gutMaxAngle;
  }
  else
  {  // projectPointPinhole, distortion coefficients 0 (icD = 1, delta = 0): :85-137
    if(cz <= 0.0f)
    {
      ox = oy = 0.0f;
      return false;
    }
    const float rcz = gRcp(cz);
    ox = (cx * rcz) * F.gutFocal[0] + resx * 0.5f;
    oy = (cy * rcz) * F.gutFocal[1] + resy * 0.5f;
    ok = true;
  }
  const float mx = resx * 0.1f, my = resy * 0.1f;  // withinResolution, GUT_IN_IMAGE_MARGIN_FACTOR
  return ok && (ox > -mx) && (oy > -my) && (ox < resx + mx) && (oy < resy + my);
}

// a sigma point through the frame's camera: the perfect models above, or the handle's sensor model (gut_common.h: gutProjectSensor)
template <bool SENSOR>
__device__ __forceinline__ bool gutProjectPoint(const FrameConst& F, float cx, float cy, float cz, float& ox, float& oy)
{
  if constexpr(SENSOR)
    return gutProjectSensor(F, cx, cy, cz, ox, oy);
  else
    return gutProjectCam(F, cx, cy, cz, ox, oy);
}

// the per-splat 3DGUT front end; returns false when the splat emits no quad
template <bool SENSOR>
__device__ __forceinline__ bool projectSplatGut(const FrameConst& F, const InstanceConst& I, uint32_t li, GutRec& out, uint32_t& rectOut)
{
  // mesh.slang:116-122.  The colour (base + SH, :142-148) does not influence any decision of the front end: it is
  // evaluated by the compositor for the records it stages (deferred shading, as in the 3DGS path: 0.96 M staged
  // (tile, splat) pairs against 4.1 M sorted splats on the garden-sized frame; the SH records were half of this kernel's time)
  const float  px = I.centers[3 * (size_t)li], py = I.centers[3 * (size_t)li + 1], pz = I.centers[3 * (size_t)li + 2];
  const float  s0 = __expf(I.scales[3 * (size_t)li]), s1 = __expf(I.scales[3 * (size_t)li + 1]), s2 = __expf(I.scales[3 * (size_t)li + 2]);
  const float4 rq = *reinterpret_cast<const float4*>(I.rotations + 4 * (size_t)li);  // (w,x,y,z)
  const float  ql = rsqrtf(rq.x * rq.x + rq.y * rq.y + rq.z * rq.z + rq.w * rq.w);
  const float  w = rq.x * ql, x = rq.y * ql, y = rq.z * ql, z = rq.w * ql;
  const float  xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  // quatToMat3 (quaternions.h.slang:39-58): row a = a-th principal axis
  const float R[3][3] = {{1.0f - 2.0f * (yy + zz), 2.0f * (xy + wz), 2.0f * (xz - wy)},
                         {2.0f * (xy - wz), 1.0f - 2.0f * (xx + zz), 2.0f * (yz + wx)},
                         {2.0f * (xz + wy), 2.0f * (yz - wx), 1.0f - 2.0f * (xx + yy)}};
  const float sc[3] = {s0, s1, s2};
  float alpha = I.alpha[li];  // the opacity as fetchColor returns it
  if(alpha < F.alphaCull)     // :150-155
    return false;
  // threedgutParticleProjection, threedgut.h.slang:26-110 (GUT_D 3, alpha 1, beta 2, kappa 0 -> lambda 0, delta sqrt 3)
  // the sigma points p +- delta_a through V*M: the map is affine, so the mean goes through the model-view matrix once and each
  // axis offset through its 3x3 (7 x 18 FMAs -> 9 + 3 x 9 + adds); only the camera model is evaluated per point
  const float* MV = I.modelView;
  const float  vcx = MV[0] * px + MV[4] * py + MV[8] * pz + MV[12];
  const float  vcy = MV[1] * px + MV[5] * py + MV[9] * pz + MV[13];
  const float  vcz = MV[2] * px + MV[6] * py + MV[10] * pz + MV[14];
  float spx[7], spy[7];
  int   nValid = gutProjectPoint<SENSOR>(F, vcx, vcy, -vcz, spx[0], spy[0]) ? 1 : 0;
  constexpr float kDelta = 1.73205080757f, kWI = 1.0f / 6.0f;
  float ccx = 0.0f, ccy = 0.0f;  // weight of the mean: lambda / (D + lambda) = 0
#pragma unroll
  for(int a = 0; a < 3; ++a)
  {
    const float ex = kDelta * sc[a] * R[a][0], ey = kDelta * sc[a] * R[a][1], ez = kDelta * sc[a] * R[a][2];
    const float dvx = MV[0] * ex + MV[4] * ey + MV[8] * ez;
    const float dvy = MV[1] * ex + MV[5] * ey + MV[9] * ez;
    const float dvz = MV[2] * ex + MV[6] * ey + MV[10] * ez;
    nValid += gutProjectPoint<SENSOR>(F, vcx + dvx, vcy + dvy, -(vcz + dvz), spx[a + 1], spy[a + 1]) ? 1 : 0;
    ccx += kWI * spx[a + 1];
    ccy += kWI * spy[a + 1];
    nValid += gutProjectPoint<SENSOR>(F, vcx - dvx, vcy - dvy, -(vcz - dvz), spx[a + 4], spy[a + 4]) ? 1 : 0;
    ccx += kWI * spx[a + 4];
    ccy += kWI * spy[a + 4];
  }
  if(nValid == 0)
    return false;
  float c0, c1, c2;
  {
    const float ex = spx[0] - ccx, ey = spy[0] - ccy;  // weight0 = 0 + (1 - alpha^2 + beta) = 2
    c0 = 2.0f * (ex * ex);
    c1 = 2.0f * (ex * ey);
    c2 = 2.0f * (ey * ey);
  }
#pragma unroll
  for(int a = 1; a < 7; ++a)
  {
    const float ex = spx[a] - ccx, ey = spy[a] - ccy;
    c0 += kWI * (ex * ex);
    c1 += kWI * (ex * ey);
    c2 += kWI * (ey * ey);
  }
  float h1x, h1y, h2x, h2y;
  if(F.extentMethod == 1)
  {  // threedgutProjectedExtentConicOpacity, threedgut.h.slang:113-160
    const float ddx = c0 + 0.3f, ddy = c1, ddz = c2 + 0.3f;
    const float det = ddx * ddz - ddy * ddy;
    if(det == 0.0f)
      return false;
    float wop = alpha;
    if(F.msAA)
      wop = alpha * gSqrt(fmaxf(0.000025f, (c0 * c2 - c1 * c1) * gRcp(det)));
    if(wop < 0.01f)
      return false;
    const float maxPower = __logf(wop * 100.0f);
    const float factor   = fminf(3.33f, gSqrt(2.0f * maxPower));
    const float mid      = 0.5f * (ddx + ddz);
    const float lambda   = mid + gSqrt(fmaxf(0.01f, mid * mid - det));
    const float radius   = factor * gSqrt(lambda);
    if(!(radius > 0.0f))
      return false;
    if(F.msAA)
      alpha = wop;
    h1x = fminf(factor * gSqrt(ddx), radius);
    h1y = 0.0f;
    h2x = 0.0f;
    h2y = fminf(factor * gSqrt(ddz), radius);
  }
  else
  {  // threedgsProjectedExtentBasis(cov, 3.33, splatScale, ...), threedgs.h.slang:60-121
    float a = c0, b = c1, d = c2, detOrig = 0.0f;
    if(F.msAA)
      detOrig = a * d - b * b;
    a += 0.3f;
    d += 0.3f;
    if(F.msAA)
      alpha *= gSqrt(fmaxf(detOrig * gRcp(a * d - b * b), 0.0f));
    const float D = a * d - b * b, half = 0.5f * (a + d);
    const float term2 = gSqrt(fmaxf(0.1f, half * half - D));
    float ev1 = half + term2, ev2 = half - term2;
    if(ev2 <= 0.0f)
      return false;
    if(F.debugFlags & 1)
      ev1 = ev2 = 0.2f;
    float       e1x = (fabsf(b) < 0.001f) ? 1.0f : b, e1y = ev1 - a;
    const float el  = rsqrtf(e1x * e1x + e1y * e1y);
    e1x *= el;
    e1y *= el;
    const float l1 = F.splatScale * fminf(3.33f * gSqrt(ev1), 2048.0f), l2 = F.splatScale * fminf(3.33f * gSqrt(ev2), 2048.0f);
    h1x = e1x * l1;
    h1y = e1y * l1;
    h2x = e1y * l2;
    h2y = -e1x * l2;
  }
  // depth of the quad from the pinhole projection matrix (":205-214": a coarse approximation for fisheye) and the
  // fixed-function clip of a quad emitted at z = ndc.z, w = 1
  const float* P  = F.proj;
  const float  tx = vcx, ty = vcy, tz = vcz;  // the mean in view space, computed above
  const float  tw = MV[3] * px + MV[7] * py + MV[11] * pz + MV[15];
  const float  cz = P[2] * tx + P[6] * ty + P[10] * tz + P[14] * tw;
  const float  cw = P[3] * tx + P[7] * ty + P[11] * tz + P[15] * tw;
  const float  ndcz = cz * gRcp(cw);
  if(!(ndcz >= 0.0f && ndcz <= 1.0f))
    return false;
  const float n1 = h1x * h1x + h1y * h1y, n2 = h2x * h2x + h2y * h2y;
  if(!(n1 > 0.0f && n2 > 0.0f))
    return false;
  // bounding box of the quad -> pixel centres covered -> bin rectangle (as the 3DGS path)
  const float bex = fabsf(h1x) + fabsf(h2x), bey = fabsf(h1y) + fabsf(h2y);
  const float fx0 = ceilf(ccx - bex - 0.5f), fx1 = floorf(ccx + bex - 0.5f);
  const float fy0 = ceilf(ccy - bey - 0.5f), fy1 = floorf(ccy + bey - 0.5f);
  const float ymin = (float)(F.stripRow0 * kTilePx), ymax = (float)(min(F.stripRow1 * kTilePx, F.height) - 1);
  if(!(fx1 >= fx0 && fy1 >= fy0 && fx1 >= 0.f && fx0 <= (float)(F.width - 1) && fy1 >= ymin && fy0 <= ymax))
    return false;
  const int x0 = (int)fmaxf(fx0, 0.f), x1 = (int)fminf(fx1, (float)(F.width - 1));
  const int y0 = (int)fmaxf(fy0, ymin), y1 = (int)fminf(fy1, ymax);
  const int sx = 4 + F.binShiftX, sy = 4 + F.binShiftY;
  rectOut = (uint32_t)(x0 >> sx) | ((uint32_t)(y0 >> sy) << 8) | ((uint32_t)(x1 >> sx) << 16) | ((uint32_t)(y1 >> sy) << 24);

  out.cx  = ccx;
  out.cy  = ccy;
  const float rn1 = gRcp(n1), rn2 = gRcp(n2);
  out.q1x = h1x * rn1;
  out.q1y = h1y * rn1;
  out.q2x = h2x * rn2;
  out.q2y = h2y * rn2;
  out.bex = bex + 0.01f;
  out.bey = bey + 0.01f;
  // canonical frame: A = S^-1 R^T, i.e. A[k][r] = R[k][r] / s_k with R's rows the axes;  B = A N, ro = A (M^-1 o - p)
  const float* Mi = I.modelInv;
  float        A[3][3];
  const float  rsc[3] = {gRcp(sc[0]), gRcp(sc[1]), gRcp(sc[2])};
#pragma unroll
  for(int k = 0; k < 3; ++k)
#pragma unroll
    for(int r = 0; r < 3; ++r)
      A[k][r] = R[k][r] * rsc[k];
#pragma unroll
  for(int k = 0; k < 3; ++k)
#pragma unroll
    for(int c = 0; c < 3; ++c)  // N(r,c) = Mi[c*4 + r]
      out.B[3 * k + c] = A[k][0] * Mi[c * 4 + 0] + A[k][1] * Mi[c * 4 + 1] + A[k][2] * Mi[c * 4 + 2];
  // camera origin in model space: M^-1 * (V^-1 * (0,0,0,1))
  const float ox = F.viewInv[12], oy = F.viewInv[13], oz = F.viewInv[14];
  const float mox = Mi[0] * ox + Mi[4] * oy + Mi[8] * oz + Mi[12];
  const float moy = Mi[1] * ox + Mi[5] * oy + Mi[9] * oz + Mi[13];
  const float moz = Mi[2] * ox + Mi[6] * oy + Mi[10] * oz + Mi[14];
  const float gx = mox - px, gy = moy - py, gz = moz - pz;
#pragma unroll
  for(int k = 0; k < 3; ++k)
    out.ro[k] = A[k][0] * gx + A[k][1] * gy + A[k][2] * gz;
  out.r = out.g = out.b = 0.0f;  // shaded by the compositor
  out.a = alpha;
  return true;
}

// Phase 1 (key + frustum cull + ordered compaction) is k_project's, statement for statement: the sorted (key, id)
// stream of a 3DGUT frame is bit-identical to the 3DGS frame's before the front-end rejections.  SENSOR: the sigma points go
// through the handle's sensor model (mgs_frame_set_sensor) instead of the frame's perfect camera; nothing else differs, and the
// host switches the partition pre-cull off for such a frame (partition_cull.h bounds the two perfect models only).
template <bool SENSOR>
__global__ __launch_bounds__(kGutThreads) void k_project_gut(const FrameArgs* __restrict__ Ap, FrameCounters* __restrict__ ctr,
                                                             uint2* __restrict__ slotPairs, uint32_t* __restrict__ slotCount,
                                                             GutRec* __restrict__ rec, uint32_t* __restrict__ rect,
                                                             uint32_t* __restrict__ slotHist2,
                                                             uint32_t* __restrict__ top16Rec, uint32_t* __restrict__ top16Count,
                                                             OsPlan* __restrict__ osPlan, const uint32_t* __restrict__ order)
{
  const FrameArgs& A = *Ap;
  __shared__ uint32_t s_hist2[256];  // 2 x 256 sixteen-bit counters (slot_emit.h)
  __shared__ uint16_t s_li[kGutPart];
  __shared__ uint32_t s_key[kGutPart];
  __shared__ uint32_t s_cnt[32];
  __shared__ uint32_t s_base[33];
  const int      t = threadIdx.x, lane = laneId(), w = t >> 6;
  const uint32_t part = order[blockIdx.x];  // fullest slot of the previous frame first (k_project.hip)
  int            k    = 0;
  for(int i = 1; i < A.f.nInstances; ++i)
    if(part >= A.inst[i].blockBegin)
      k = i;
  const InstanceConst& I      = A.inst[k];
  const uint32_t       local0 = (part - I.blockBegin) * kGutPart;
  const PartitionBox pbox = partitionLoad(I, part - I.blockBegin);  // ahead of the centres (partition_cull.h)
  float px[kGutItems], py[kGutItems], pz[kGutItems];
#pragma unroll
  for(int it = 0; it < kGutItems; ++it)
  {
    const uint32_t li = min(local0 + it * kGutThreads + t, I.count - 1u);
    px[it] = I.centers[3 * (size_t)li];
    py[it] = I.centers[3 * (size_t)li + 1];
    pz[it] = I.centers[3 * (size_t)li + 2];
  }
  {  // the partition as a whole (partition_cull.h): no splat of it can survive the cull / reach the strip
    float partRadius;
    if(A.f.partitionCull && (partitionTest(A, I, pbox, partRadius) & 1u) != 0u)
    {
      emitEmptySlot<kGutThreads>(slotCount, slotHist2, top16Rec, part);
      return;
    }
  }
  // (s_hist2: the hand-over's small tables, slot_emit.h)
  uint32_t key[kGutItems];
  uint64_t bal[kGutItems];
  bool     vis[kGutItems];
#pragma unroll
  for(int it = 0; it < kGutItems; ++it)
  {
    const uint32_t li = local0 + it * kGutThreads + t;
    float          wp[4], vp[4], cp[4];
    mulMat4Exact(I.model, px[it], py[it], pz[it], 1.0f, wp);  // dist.comp.slang:58
    mulMat4Exact(A.f.view, wp[0], wp[1], wp[2], wp[3], vp);
    mulMat4Exact(A.f.proj, vp[0], vp[1], vp[2], vp[3], cp);   // :60
    const float nx = divExact(cp[0], cp[3]), ny = divExact(cp[1], cp[3]), nz = divExact(cp[2], cp[3]);  // :61
    bool        v  = li < I.count;
    if(A.f.cullMode == 1 && distStageCulled(A.f, nx, ny, nz, vp[0], vp[1], vp[2]))  // dist.comp.slang:64-91
      v = false;
    if(A.f.sizeCulling && v)
      v = !sizeCulled(I.maxScale[min(li, I.count - 1u)], A.f.splatScale, I.modelAxisMax, vp[2], A.f.maxFocal, A.f.sizeCullingMinPixels);
    vis[it] = v;
    key[it] = A.f.frontToBack ? encodeKey(nz) : encodeKey(-nz);
    bal[it] = __ballot(v);
    if(lane == 0)
      s_cnt[it * 4 + w] = (uint32_t)__popcll(bal[it]);
  }
  const uint32_t Mv = scanRoundWaveCounts(s_cnt, s_base);
#pragma unroll
  for(int it = 0; it < kGutItems; ++it)
    if(vis[it])
    {
      const uint32_t pos = s_base[it * 4 + w] + lanesBelow(bal[it]);
      s_li[pos]          = (uint16_t)(it * kGutThreads + t);
      s_key[pos]         = key[it];
    }
  __syncthreads();
  if(t == 0 && Mv)
    atomicAdd(&frameStatLineFromOs(osPlan, part)->survivors, Mv);  // (32 lines, not the counters' one)
  // ---- 3DGUT front end over the survivors ----
  // The 96-byte records leave through LDS (as k_project's do): every lane builds one record, then the wave stores its 64 records
  // six lanes per record, so that a store instruction covers whole sectors wherever neighbouring ids both survive (a wave's
  // survivors are mostly consecutive ids: 6 KB contiguous).  Written lane-per-record, each of the six instructions put 16 bytes
  // into 64 different sectors.  Pitch 7 quads: conflict-free 16-byte LDS accesses.
  __shared__ float4   s_grec[4][64 * 7];
  __shared__ uint32_t s_ggid[4][64];
  // the bin rectangles' codes for the hand-over (kernels_common.h: rideEncode): in LDS here — this kernel runs at 169 VGPRs
  // and three workgroups per CU either way, and k_project's register chain cost it 60 us
  __shared__ uint16_t s_code[kGutPart];
  const uint32_t      rideShift = (uint32_t)A.f.rideShift;
  for(uint32_t j0 = 0; j0 < Mv; j0 += kGutThreads)
  {
    const uint32_t j = j0 + t;
    uint32_t       gidOk = 0xFFFFFFFFu;
    if(j < Mv)
    {
      const uint32_t li = local0 + s_li[j];
      GutRec         r;
      uint32_t       rc;
      if(projectSplatGut<SENSOR>(A.f, I, li, r, rc))
      {
        gidOk       = I.globalOffset + li;
        float4* dst = &s_grec[w][lane * 7];
        dst[0]      = make_float4(r.cx, r.cy, r.q1x, r.q1y);
        dst[1]      = make_float4(r.q2x, r.q2y, r.bex, r.bey);
        dst[2]      = make_float4(r.B[0], r.B[1], r.B[2], r.B[3]);
        dst[3]      = make_float4(r.B[4], r.B[5], r.B[6], r.B[7]);
        dst[4]      = make_float4(r.B[8], r.ro[0], r.ro[1], r.ro[2]);
        dst[5]      = make_float4(r.r, r.g, r.b, r.a);
        uint32_t code = A.f.rideEscape;
        if(rideShift != 0u)
          s_code[j] = (uint16_t)(code = rideEncode(rc, A.f.binsX, A.f.binsY, A.f.rideShapes, A.f.rideEscape));  // own entry only
        if(rideShift == 0u || code == A.f.rideEscape)  // read back by id only where the code cannot say it (k_project.hip)
          rect[gidOk] = rc;
        s_li[j] |= 0x8000u;
      }
    }
    s_ggid[w][lane] = gidOk;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for(int i = 0; i < 6; ++i)
    {
      const uint32_t idx = (uint32_t)(i * 64 + lane), rr = idx / 6u, pt = idx - rr * 6u;
      const uint32_t g   = s_ggid[w][rr];
      if(g != 0xFFFFFFFFu)
        reinterpret_cast<float4*>(rec + g)[pt] = s_grec[w][rr * 7 + pt];
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // second ordered compaction into the partition's slot + what the key sort needs up front (slot_emit.h)
  // (the record staging area is free now: 16 KB of it hold the grouped slot, 2 KB behind them the per-wave digit counts)
  EmitLds E;
  E.li    = s_li;
  E.key   = s_key;
  E.code  = rideShift != 0u ? s_code : nullptr;
  E.stage = reinterpret_cast<uint2*>(&s_grec[0][0]);
  E.whist = reinterpret_cast<uint16_t*>(reinterpret_cast<unsigned char*>(&s_grec[0][0]) + 16384);
  E.hist1 = s_hist2;
  E.start = reinterpret_cast<uint16_t*>(s_hist2 + 128);
  E.cnt   = s_cnt;
  static_assert(sizeof(s_grec) >= 16384 + 2048, "the hand-over's stage and counters live in the record staging area");
  emitSlot<kGutThreads, kGutItems>(Mv, false, E, slotPairs, slotCount, slotHist2, top16Rec, top16Count, osPlan, ctr, part,
                                   I.globalOffset + local0, rideShift | (A.f.rideSplit ? 0x100u : 0u));
}

// ---------------------------------------------------------------------------------------------
void launchProjectGut(hipStream_t stream, const ProjectLaunch& L)
{
  if(L.totalPartitions == 0)
    return;
  if(L.sensor)
    hipLaunchKernelGGL(k_project_gut<true>, dim3(L.totalPartitions), dim3(kGutThreads), 0, stream, L.dArgs, L.ctr, L.slotPairs, L.slotCount, L.recGut,
                       L.rect, L.slotHist2, L.top16Rec, L.top16Count, L.osPlan, L.order);
  else
    hipLaunchKernelGGL(k_project_gut<false>, dim3(L.totalPartitions), dim3(kGutThreads), 0, stream, L.dArgs, L.ctr, L.slotPairs, L.slotCount, L.recGut,
                       L.rect, L.slotHist2, L.top16Rec, L.top16Count, L.osPlan, L.order);
}

}  // namespace mgs
