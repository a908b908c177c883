// host_model.h — RAM-side splat model and helpers shared by the C ABI implementation.
// Mirrors struct SplatSet of the reference (src/splat_set.h:33-48): INRIA SoA arrays in RUB.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mgs {

struct HostSplatSet
{
  std::vector<float> positions;  // 3n
  std::vector<float> f_dc;       // 3n
  std::vector<float> f_rest;     // (3*coeffsPerChannel) n, channel-major per splat
  std::vector<float> opacity;    // n (logit)
  std::vector<float> scale;      // 3n (log)
  std::vector<float> rotation;   // 4n (w,x,y,z)
  std::string        path;

  size_t   size() const { return positions.size() / 3; }
  uint32_t fRestPerSplat() const { return size() ? uint32_t(f_rest.size() / size()) : 0u; }
  int      maxShDegree() const;                 // src/splat_set.h:52-74
  void     convertRdfToRub();                   // src/splat_set.h:78-114 with (RDF -> RUB)
};

// RAM-side triangle mesh (ObjLoader's m_vertices / m_indices / m_matIndices / m_materials, src/obj_loader.h), RUB frame
struct HostMeshMaterial
{
  float ambient[3], diffuse[3], specular[3], emission[3];
  float shininess;
};
// what a material library says about bounces (mgs_mesh_bounce_materials): tinyobj's initial values are Tf 0, Ni 1, illum 0
struct HostMtlBounce
{
  float tf[3] = {0.0f, 0.0f, 0.0f};
  float ni    = 1.0f;
  int   illum = 0;
};
struct HostMesh
{
  std::vector<float>            positions, normals;  // 3 per vertex
  std::vector<uint32_t>         indices;             // 3 per triangle
  std::vector<uint32_t>         materialIds;         // 1 per triangle, < materials.size()
  std::vector<HostMeshMaterial> materials;           // never empty
  std::vector<HostMtlBounce>    mtlBounce;           // per material the MTL's Tf / Kt, Ni and illum statements; empty for a mesh from arrays
  std::string                   path;
};
HostMeshMaterial defaultMeshMaterial();  // the loader's default, src/obj_loader.cpp:72-81
// per-vertex normals the way src/obj_loader.cpp:98-151 generates them: faces in index order, the first face that touches a vertex sets
// its normal, every later one replaces it by mix(old, face normal, 0.5).  normals / visited persist across the shapes of a file.
void accumulateFaceNormals(const float* positions, const uint32_t* indices, size_t indexCount, std::vector<float>& normals, std::vector<uint8_t>& visited);
int  loadObj(const std::string& path, HostMesh& out);  // the OBJ subset documented in include/mgs.h (mgs_mesh_load_obj)

// thread-local error message used by the C ABI
void        setError(const std::string& msg);
const char* lastError();

// loaders: return 0 or a negative MgsStatus
int loadPly(const std::string& path, HostSplatSet& out);    // src/ply_loader_async.cpp:357-441
int loadSpz(const std::string& path, HostSplatSet& out);    // src/ply_loader_async.cpp:304-353 + 3rdparty/spz
int loadSplat(const std::string& path, HostSplatSet& out);  // src/ply_loader_async.cpp:43-183

// 4x4 helpers, glm column-major memory (m[col*4+row]); plain unfused fp32 like glm on the host
void mat4Mul(const float a[16], const float b[16], float out[16]);
void mat4Inverse(const float m[16], float out[16]);
void mat4MulVec4(const float m[16], const float v[4], float out[4]);

// upload transform of SplatSetVk::initDataBuffers (src/splat_set_vk.cpp:263-435), host side, threaded
void buildCov6(const HostSplatSet& s, std::vector<float>& cov6);
void buildRgba(const HostSplatSet& s, std::vector<float>& rgba);
int  shStride(uint32_t fRestPerSplat);
void buildShInterleaved(const HostSplatSet& s, std::vector<float>& sh);
uint16_t floatToHalf(float f);
float    halfToFloat(uint16_t h);
uint8_t  toUint8(float v, float lo, float hi);  // src/splat_set_vk.cpp:85-89

// spatially coherent storage order: permutation newToOld sorted by the 63-bit Morton code of the centre
// `radius` (optional, one per splat): splats are first split into 16 size classes (octaves of the radius
// around the median), then Morton-sorted inside each class, so that a partition's footprint bound is not
// set by a few outliers.
void mortonOrder(const HostSplatSet& s, const std::vector<float>* radius, std::vector<uint32_t>& newToOld);

// ---- the planes of a committed splat set, as they lie in device memory (mgs_scene_commit uploads them as they are) ----
// Storage formats are include/mgs.h's MGS_FORMAT_FLOAT32 / FLOAT16 / UINT8 (0 / 1 / 2).  UINT8 maps [0,1] (colours) or [-1,1] (SH).
constexpr uint32_t kPackPart = 2048;  // splats per partition (= kPart of the kernels)
inline size_t formatBytes(int format) { return format == 0 ? 4 : format == 1 ? 2 : 1; }
void quantise(const float* src, size_t n, int format, bool isSh, uint8_t* dst);    // the ONE float -> storage format ...
void dequantise(const uint8_t* src, size_t n, int format, bool isSh, float* dst);  // ... and the ONE way back (fetchColor's read)

struct PackedSplatSet
{
  // storage order (size classes, then Morton order of the centres) <-> caller's order.  Ids inside the pipeline are STORAGE ids; ties
  // between equal depth keys resolve in storage order (the reference's tie order is nondeterministic, dist.comp.slang:137-139)
  std::vector<uint32_t> newToOld, oldToNew;
  // everything below in storage order
  std::vector<float>   centers;    // [count*3]
  std::vector<float>   cov6;       // planar: float4 covA[count] = (S00,S01,S02,S11) then float2 covB[count] = (S12,S22)
  std::vector<float>   partBox;    // [ceil(count/2048)][8]: min xyz, max xyz of the centres, rmax = sqrt(8 * max trace(Sigma)), and
                                   // 1.0 where the partition holds non-finite data (never culled)
  std::vector<float>   maxScale;   // [count] max(exp(scale)): size culling (dist.comp.slang:93-134), exp() on the host like the oracle
  std::vector<float>   scales;     // [count*3] log scales   } as stored (splat_set_vk.cpp:221-251), read by the surface normal only
  std::vector<float>   rotations;  // [count*4] (w,x,y,z)    }
  std::vector<uint8_t> rgba;       // [count*4] in the colour format
  std::vector<float>   rgbaRead;   // [count*4] `rgba` as fetchColor reads it back (threedgs_particle_buffers.h.slang:72-90); empty
                                   // when `rgba` is stored as fp32 and is that plane itself
  std::vector<float>   alpha;      // [count] the fourth component of rgbaF32(): all the projection needs
  std::vector<uint8_t> sh;         // [count] records of shPitch elements in the SH format, [coef][rgb] like the reference then
                                   // zeros: the compositor fetches whole records (192 B fp32 = three 64-byte sectors)
  uint32_t count = 0;
  int      shDegree = 0, shStride = 0;  // logical SH elements per splat (0/9/24/45)
  int      shPitch = 0;                 // stored ones (48, or 0 without SH)
  // [count*4] the colours as the shaders read them back
  const float* rgbaF32() const { return rgbaRead.empty() ? reinterpret_cast<const float*>(rgba.data()) : rgbaRead.data(); }
};
// a4: SplatSetVk::initDataBuffers (src/splat_set_vk.cpp:188-480), host loops like the reference
void packSplatSet(const HostSplatSet& h, int shFormat, int rgbaFormat, PackedSplatSet& out);
// the inverse for the planes mgs_scene_download_set names (0 centres, 1 cov6 as 6 floats per splat, 2 rgba, 3 SH as
// [splat][coef][rgb]): `raw` is the plane as stored, `dst` fp32 in the caller's order
size_t packedPlaneBytes(int which, size_t count, int shPitch, int format);
void   unpackPlane(int which, const uint8_t* raw, int format, const std::vector<uint32_t>& newToOld, int shStride, int shPitch, float* dst);

// parallel-for over [0,n) in batches of 8192 (START_PAR_LOOP, src/utilities.h:52-59)
template <typename F>
void parallelBatches(size_t n, F&& fn);

}  // namespace mgs

#include <algorithm>
#include <thread>
namespace mgs {
template <typename F>
void parallelBatches(size_t n, F&& fn)
{
  const size_t batch   = 8192;
  const size_t nBatch  = (n + batch - 1) / batch;
  unsigned     threads = std::max(1u, std::thread::hardware_concurrency());
  threads              = (unsigned)std::min<size_t>(threads, std::max<size_t>(1, nBatch));
  if(threads > 32)
    threads = 32;
  auto worker = [&](unsigned tid) {
    for(size_t b = tid; b < nBatch; b += threads)
    {
      const size_t lo = b * batch, hi = std::min(n, lo + batch);
      for(size_t i = lo; i < hi; ++i)
        fn(i);
    }
  };
  std::vector<std::thread> pool;
  for(unsigned t = 1; t < threads; ++t)
    pool.emplace_back(worker, t);
  worker(0);
  for(auto& th : pool)
    th.join();
}
}  // namespace mgs
