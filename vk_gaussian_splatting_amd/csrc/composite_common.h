// composite_common.h — what the compositors share: k_composite's mode bits and the grid size of the packed compositors (k_composite.hip,
// k_composite_gut.hip).  A finished pixel goes into the frame through target_pixel.h.
#pragma once
#include <hip/hip_runtime.h>

#include "target_pixel.h"

namespace mgs {

// ---- k_composite's MODE -------------------------------------------------------------------------------------------------------
constexpr int kCmpAlphaSum   = 1;   // additive alpha (MGS_ALPHA_SUM): no early-out, every fragment of the list is summed
constexpr int kCmpNoGauss    = 2;   // DISABLE_OPACITY_GAUSSIAN
constexpr int kCmpSurface    = 4;   // surface side outputs: picked depth, the splat that set it, integrated normal
constexpr int kCmpStochastic = 8;   // stochastic splats (frag.slang:265-290: a fragment is accepted with probability alpha and written
                                    // opaque; the depth test keeps the nearest accepted one == the first accepted one of the list)
constexpr int kCmpOccluder   = 16;  // mgs_frame_set_occluder: fragments depth-tested against the caller's depth image, the caller's
                                    // colour behind them
constexpr bool surf_lds(int mode) { return (mode & kCmpSurface) != 0; }
constexpr bool occ_lds(int mode) { return (mode & kCmpOccluder) != 0; }
// MGS_ALPHA_SUM without surface outputs and without an occluder (the saturated-tail walks sum fragments without looking at them one
// by one; with an occluder every fragment is tested, so that mode takes the general walk, as the surface outputs do)
constexpr bool sum_walk(int mode) { return (mode & kCmpAlphaSum) != 0 && !surf_lds(mode) && !occ_lds(mode); }

// ---- grid of the packed compositors (k_composite, k_composite_gut2) -----------------------------------------------------------
// Their workgroups map to regions bin by bin, eight bins at a time (one per XCD), every bin of the frame enumerated; the mapping
// itself is written out in both kernels, because their machine code changes when it is a function (four forms tried).
template <class Args>  // CompositeArgs or FrameConst
inline int compositeRegionGrid(const Args& F)
{
  const int nBins = F.binsX * F.binsY;
  return ((nBins + 7) / 8) * (1 << (F.binShiftX - 1 + F.binShiftY)) * 8;  // a multiple of 8: the same count on every XCD
}

}  // namespace mgs
