// pack_roundtrip.cpp — stand-alone check of the host-side pack of a splat set (csrc/host_model.cpp: packSplatSet, unpackPlane,
// quantise, dequantise).  Built with g++ together with host_model.cpp and run as a program (tests/test_host_cpu.py), plainly and
// under ASan + UBSan.  It asserts the layout properties below for a generated set in all nine format pairs, and prints one digest
// per plane: the test compares those with tests/golden/pack_digests.txt, recorded from the commit path before the pack moved here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_model.h"

using namespace mgs;

#define CHECK(cond, ...)                                                                                                \
  do                                                                                                                    \
  {                                                                                                                     \
    if(!(cond))                                                                                                         \
    {                                                                                                                   \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);                                                     \
      std::printf(__VA_ARGS__);                                                                                         \
      std::printf("\n");                                                                                                \
      std::exit(1);                                                                                                     \
    }                                                                                                                   \
  } while(0)

// 4100 splats: two full 2048-splat partitions and a partial one.  Every value is an integer times one constant, so the set is
// the same whichever compiler builds this file.  Log scales span [-12, 2.2] (20 octaves of the footprint radius, more than the 16
// size classes of mortonOrder); the last splat is the largest, has a NaN x and lies far out in y and z, which puts it at the end
// of the storage order, in the last partition.
static uint64_t g_rng;
static int      rnd(int lo, int hi)  // inclusive
{
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (int)((g_rng >> 33) % (uint64_t)(hi - lo + 1));
}
static void makeSet(size_t n, uint32_t fRest, HostSplatSet& h)
{
  g_rng = 0x9E3779B97F4A7C15ull + fRest;
  h.positions.resize(3 * n), h.f_dc.resize(3 * n), h.f_rest.resize((size_t)fRest * n), h.opacity.resize(n), h.scale.resize(3 * n);
  h.rotation.resize(4 * n);
  for(size_t i = 0; i < n; ++i)
  {
    const int base = rnd(-12000, 2000);
    for(int a = 0; a < 3; ++a)
    {
      h.positions[3 * i + a] = (float)rnd(-10000, 10000) * 0.001f;
      h.f_dc[3 * i + a]      = (float)rnd(-2500, 2500) * 0.001f;  // some colours clamp at 0 and at 1
      h.scale[3 * i + a]     = (float)(base + rnd(0, 200)) * 0.001f;
    }
    for(int a = 0; a < 4; ++a)
      h.rotation[4 * i + a] = (float)rnd(-1000, 1000) * 0.001f;
    h.opacity[i] = (float)rnd(-6000, 6000) * 0.001f;
    for(uint32_t k = 0; k < fRest; ++k)
      h.f_rest[i * fRest + k] = (float)rnd(-1300, 1300) * 0.001f;  // some beyond the u8 range [-1, 1]
  }
  h.scale[3 * n - 3] = h.scale[3 * n - 2] = h.scale[3 * n - 1] = 3.0f;
  h.positions[3 * n - 3]                                        = std::nanf("");
  h.positions[3 * n - 2] = h.positions[3 * n - 1] = 1000.0f;  // the highest Morton code of its size class
}

static uint64_t digest(const void* p, size_t bytes)
{  // FNV-1a, 64 bit
  uint64_t h = 0xcbf29ce484222325ull;
  for(size_t i = 0; i < bytes; ++i)
    h = (h ^ ((const uint8_t*)p)[i]) * 0x100000001b3ull;
  return h;
}
template <typename T>
static void printDigest(const char* run, const char* plane, const std::vector<T>& v)
{
  std::printf("%s %s %zu %016llx\n", run, plane, v.size() * sizeof(T), (unsigned long long)digest(v.data(), v.size() * sizeof(T)));
}
static bool sameBits(const std::vector<float>& a, const std::vector<float>& b)
{
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}
// what a plane holds after it went through a storage format and back
static std::vector<float> throughFormat(const std::vector<float>& v, int format, bool isSh)
{
  std::vector<uint8_t> q(v.size() * formatBytes(format));
  std::vector<float>   back(v.size());
  quantise(v.data(), v.size(), format, isSh, q.data());
  dequantise(q.data(), v.size(), format, isSh, back.data());
  return back;
}

static void checkSet(uint32_t fRest)
{
  const size_t n = 4100, np = 3;
  HostSplatSet h;
  makeSet(n, fRest, h);
  std::vector<float> cov, rgba, sh;
  buildCov6(h, cov);
  buildRgba(h, rgba);
  buildShInterleaved(h, sh);
  const int stride = shStride(fRest);

  for(int shFormat = 0; shFormat < 3; ++shFormat)
    for(int rgbaFormat = 0; rgbaFormat < 3; ++rgbaFormat)
    {
      PackedSplatSet P;
      packSplatSet(h, shFormat, rgbaFormat, P);
      CHECK(P.count == n && P.shStride == stride && P.shPitch == (stride ? 48 : 0), "count %u stride %d pitch %d", P.count, P.shStride, P.shPitch);

      // the two permutations are each other's inverse
      CHECK(P.newToOld.size() == n && P.oldToNew.size() == n, "permutation sizes");
      for(size_t i = 0; i < n; ++i)
        CHECK(P.newToOld[i] < n && P.oldToNew[P.newToOld[i]] == i, "storage index %zu", i);
      for(size_t o = 0; o < n; ++o)
        CHECK(P.newToOld[P.oldToNew[o]] == o, "caller's index %zu", o);
      CHECK(P.oldToNew[n - 1] >= 2 * kPackPart, "the non-finite splat sits at storage index %u", P.oldToNew[n - 1]);

      // unpacking returns the caller's arrays: exactly for fp32, exactly their quantise-dequantise otherwise
      std::vector<float> got;
      auto unpack = [&](int which, const void* raw, size_t rawBytes, int format, size_t elems) {
        CHECK(rawBytes == packedPlaneBytes(which, n, P.shPitch, format), "plane %d holds %zu bytes", which, rawBytes);
        got.assign(elems, -77.f);
        unpackPlane(which, (const uint8_t*)raw, format, P.newToOld, P.shStride, P.shPitch, got.data());
      };
      unpack(0, P.centers.data(), P.centers.size() * 4, 0, 3 * n);
      CHECK(sameBits(got, h.positions), "centres");
      unpack(1, P.cov6.data(), P.cov6.size() * 4, 0, 6 * n);
      CHECK(sameBits(got, cov), "cov6");
      unpack(2, P.rgba.data(), P.rgba.size(), rgbaFormat, 4 * n);
      CHECK(sameBits(got, rgbaFormat == 0 ? rgba : throughFormat(rgba, rgbaFormat, false)), "rgba in format %d", rgbaFormat);
      // the fp32 colour plane is the unpacked formatted plane (in storage order), alpha its fourth component
      // (a plane of its own exactly when the formatted plane is not fp32)
      CHECK(P.rgbaRead.size() == (rgbaFormat == 0 ? 0 : 4 * n) && P.alpha.size() == n, "colour read-back sizes");
      const std::vector<float> rgbaF32(P.rgbaF32(), P.rgbaF32() + 4 * n);
      for(size_t i = 0; i < n; ++i)
      {
        CHECK(std::memcmp(&rgbaF32[4 * i], &got[4 * (size_t)P.newToOld[i]], 16) == 0, "rgbaF32 of storage index %zu", i);
        CHECK(std::memcmp(&P.alpha[i], &rgbaF32[4 * i + 3], 4) == 0, "alpha of storage index %zu", i);
      }
      if(stride)
      {
        unpack(3, P.sh.data(), P.sh.size(), shFormat, (size_t)stride * n);
        CHECK(sameBits(got, shFormat == 0 ? sh : throughFormat(sh, shFormat, true)), "sh in format %d", shFormat);
        // records are padded to 48 elements with the quantised zero
        const size_t         esz = formatBytes(shFormat), pad = 48 - (size_t)stride;
        std::vector<float>   zeros(pad, 0.f);
        std::vector<uint8_t> qz(pad * esz);
        quantise(zeros.data(), pad, shFormat, true, qz.data());
        for(size_t i = 0; i < n; ++i)
          CHECK(std::memcmp(&P.sh[(i * 48 + (size_t)stride) * esz], qz.data(), qz.size()) == 0, "sh padding of storage index %zu", i);
      }
      else
        CHECK(P.sh.empty(), "a set without SH has an SH plane of %zu bytes", P.sh.size());

      // the planes download_set does not reach
      CHECK(P.maxScale.size() == n && P.scales.size() == 3 * n && P.rotations.size() == 4 * n, "plane sizes");
      for(size_t i = 0; i < n; ++i)
      {
        const size_t o  = P.newToOld[i];
        const float* sc = &h.scale[3 * o];
        CHECK(std::memcmp(&P.scales[3 * i], sc, 12) == 0 && std::memcmp(&P.rotations[4 * i], &h.rotation[4 * o], 16) == 0, "scales / rotations of %zu", i);
        CHECK(P.maxScale[i] == std::max(std::exp(sc[0]), std::max(std::exp(sc[1]), std::exp(sc[2]))), "maxScale of %zu", i);
      }
      // partition boxes: a finite partition's box holds its centres and its radius bound every footprint; only the last is flagged
      CHECK(P.partBox.size() == np * 8, "partBox holds %zu floats", P.partBox.size());
      for(size_t p = 0; p < np; ++p)
      {
        const float* b = &P.partBox[8 * p];
        CHECK(b[7] == (p == np - 1 ? 1.0f : 0.0f), "partition %zu: non-finite flag %g", p, b[7]);
        if(b[7] != 0.0f)
          continue;
        for(size_t i = p * kPackPart; i < std::min(n, (p + 1) * (size_t)kPackPart); ++i)
        {
          const float* c = &cov[6 * (size_t)P.newToOld[i]];
          for(int a = 0; a < 3; ++a)
            CHECK(b[a] <= P.centers[3 * i + a] && P.centers[3 * i + a] <= b[3 + a], "partition %zu: centre %zu outside the box", p, i);
          // rmax^2 >= 8 * trace, compared on the square roots: squaring the rounded root again would lose the half ulp that
          // sqrt rounded away for the very splat that sets the bound; sqrt is monotone, so this comparison needs no tolerance
          CHECK(b[6] >= std::sqrt(8.0f * (c[0] + c[3] + c[5])), "partition %zu: rmax %g below splat %zu", p, b[6], i);
        }
      }

      char run[64];
      std::snprintf(run, sizeof(run), "f_rest=%u sh=%d rgba=%d", fRest, shFormat, rgbaFormat);
      printDigest(run, "newToOld", P.newToOld), printDigest(run, "oldToNew", P.oldToNew), printDigest(run, "centers", P.centers);
      printDigest(run, "cov6", P.cov6), printDigest(run, "partBox", P.partBox), printDigest(run, "maxScale", P.maxScale);
      printDigest(run, "scales", P.scales), printDigest(run, "rotations", P.rotations), printDigest(run, "rgba", P.rgba);
      printDigest(run, "rgbaF32", rgbaF32), printDigest(run, "alpha", P.alpha), printDigest(run, "sh", P.sh);
    }
}

int main()
{
  for(uint32_t fRest : {0u, 9u, 24u, 45u})
    checkSet(fRest);
  std::printf("pack_roundtrip ok\n");
  return 0;
}
