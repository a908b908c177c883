// trace_dispatch.h — what the launchers of the traced pipeline (k_trace.hip, k_trace_stochastic.hip, k_trace_rays.hip,
// k_trace_light.hip, k_hybrid.hip) and its host side (api_trace.hip) decide alike: the SH-format index, the K-buffer size of a
// samples_per_pass, the strip's tile count, and the walk from those two runtime values to a kernel's <SHF, KB> instantiation.
// Host code only.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "device_types.h"

namespace mgs {

// the SH storage format as the kernels' SHF: 0 and 1 as they are, everything else 2
inline int shFormatIndex(int shFormat) { return shFormat == 0 ? 0 : shFormat == 1 ? 1 : 2; }

// 16 x 16 tiles of the frame's strip: the workgroups of every kernel in k_trace's tiling
inline int stripTiles(const FrameConst& F) { return F.tilesX * (F.stripRow1 - F.stripRow0); }

// fn(std::integral_constant<int, SHF>) for the scene's SH format
template <class Fn>
void withShFormat(int shFormat, Fn&& fn)
{
  switch(shFormatIndex(shFormat))
  {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case 1: fn(std::integral_constant<int, 1>{}); break;
    default: fn(std::integral_constant<int, 2>{}); break;
  }
}

// fn(std::integral_constant<int, KB>) for the smallest K-buffer in registers that holds samples_per_pass: 4, 18 or 32 slots.  The
// API admits [1, 32] (validateTrace); a launcher handed more has no instantiation and says so
template <class Fn>
void withKBuffer(const char* launcher, int samplesPerPass, Fn&& fn)
{
  if(samplesPerPass <= 4)
    fn(std::integral_constant<int, 4>{});
  else if(samplesPerPass <= 18)
    fn(std::integral_constant<int, 18>{});
  else if(samplesPerPass <= 32)
    fn(std::integral_constant<int, 32>{});
  else
  {
    std::fprintf(stderr, "%s: no instantiation for samples_per_pass %d\n", launcher, samplesPerPass);
    std::abort();
  }
}

// fn(shf, kb) with both as integral constants: the nine <SHF, KB> instantiations of a traversal kernel
template <class Fn>
void withShFormatAndKBuffer(const char* launcher, int shFormat, int samplesPerPass, Fn&& fn)
{
  withShFormat(shFormat, [&](auto shf) { withKBuffer(launcher, samplesPerPass, [&](auto kb) { fn(shf, kb); }); });
}

}  // namespace mgs
