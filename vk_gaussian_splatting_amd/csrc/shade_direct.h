// shade_direct.h — the direct shading the deferred lighting pass (k_light.hip), the mesh pass (k_mesh.hip) and the light pass of a
// traced frame (k_trace_light.hip) evaluate: wavefrontComputeShadingDirectOnly with wavefrontComputeSpecular
// (shaders/wavefront.h.slang:233-280,388-403) in their own order of operations, the material and light types it reads with the
// materials' unpacking and createHeadlight (:104-119), each once for the raster and the traced passes, the small vector helpers, and
// for the traced pass computeLightToSurfaceVector (:33-70) with the shadow's factor on the light's colour.
// Device code only; every kernel file that includes it gets its own inlined copy.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mgs.h"
#include "device_types.h"
#include "kernels_common.h"

namespace mgs {

namespace {

struct V3
{
  float x, y, z;
};
__device__ __forceinline__ V3    operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3    operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3    operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3    operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3    operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3    normalize3(V3 a) { return a * (1.0f / sqrtf(dot3(a, a))); }
__device__ __forceinline__ V3    load3(const float* p) { return {p[0], p[1], p[2]}; }

struct Mat
{
  V3    ambient, diffuse, specular, emission;
  float shininess;
  int   needShading;
};

// a material record as the shading reads it: four 16-byte loads
__device__ __forceinline__ Mat material(const MaterialDev& m)
{
  const float4* mp = reinterpret_cast<const float4*>(&m);
  const float4  m0 = mp[0], m1 = mp[1], m2 = mp[2], m3 = mp[3];
  Mat           mat;
  mat.ambient     = {m0.x, m0.y, m0.z};
  mat.diffuse     = {m0.w, m1.x, m1.y};
  mat.specular    = {m1.z, m1.w, m2.x};
  mat.emission    = {m2.y, m2.z, m2.w};
  mat.shininess   = m3.x;
  mat.needShading = __float_as_int(m3.y);
  return mat;
}
// the splat surface's material: an instance's record times the base radiance (splatSetDesc.material, rgen.slang:1084-1105)
__device__ __forceinline__ Mat splatMaterial(const MaterialDev& m, V3 baseRadiance)
{
  Mat mat      = material(m);
  mat.ambient  = baseRadiance * mat.ambient;
  mat.diffuse  = baseRadiance * mat.diffuse;
  mat.specular = baseRadiance * mat.specular;
  mat.emission = baseRadiance * mat.emission;
  return mat;
}
// a mesh's material with the transmittance in front of it: wavefrontComputeShading{,DirectOnly} weight the ambient and the
// (diffuse + specular) terms (wavefront.h.slang:249, :279, :303, :332); the emission is added unweighted, as written (rgen.slang:1159)
__device__ __forceinline__ Mat weightedMaterial(Mat mat, V3 weight)
{
  mat.ambient  = mat.ambient * weight;
  mat.diffuse  = mat.diffuse * weight;
  mat.specular = mat.specular * weight;
  return mat;
}

// createHeadlight (wavefront.h.slang:104-119): a point light at the camera, no attenuation; what shades a scene without lights
__device__ __forceinline__ LightDev headlight(const float cameraPos[3])
{
  LightDev h;
  h.type      = MGS_LIGHT_POINT;
  h.attMode   = 0;
  h.color[0] = h.color[1] = h.color[2] = 1.0f;
  h.intensity = 1.0f;
  h.pos[0]    = cameraPos[0];
  h.pos[1]    = cameraPos[1];
  h.pos[2]    = cameraPos[2];
  h.range     = 1e10f;
  h.dirN[0] = h.dirN[1] = 0.0f;
  h.dirN[2]  = -1.0f;
  h.innerCos = h.outerCos = 1.0f;
  return h;
}

// distance attenuation of computePointLight / computeSpotLight (wavefront.h.slang:160-174, 193-206)
__device__ __forceinline__ float attenuate(int mode, float distance, float range)
{
  float attenuation = 1.0f;
  if(mode == 1)
    attenuation = 1.0f - (distance / range);
  else if(mode == 2)
    attenuation = 1.0f / (1.0f + distance * distance);
  else if(mode == 3)
    attenuation = 1.0f / (distance * distance + 0.01f);
  return attenuation;
}

// computeLightToSurfaceVector (wavefront.h.slang:33-70), hard shadows: the direction to the light and its distance; false when a
// point or spot light is farther away than its range.  The traced pass SKIPS such a light entirely (rgen.slang:1120-1121), ambient
// term included; the deferred raster pass calls shadeDirect for every light, which adds the ambient term and no more.  A point that
// coincides with the light divides 0 by 0 as normalize(toLight) does in the reference: the pixel is NaN there and here.
__device__ __forceinline__ bool lightToSurface(const LightDev& light, V3 worldPos, V3& lightDir, float& lightDist)
{
  if(light.type == MGS_LIGHT_DIRECTIONAL)
  {
    lightDir  = -load3(light.dirN);
    lightDist = 1e10f;
    return true;
  }
  const V3 toLight = load3(light.pos) - worldPos;
  lightDist        = sqrtf(dot3(toLight, toLight));
  if(lightDist > light.range)
    return false;
  lightDir = toLight * (1.0f / lightDist);
  return true;
}

// computeLightToSurfaceVector under SHADOWS_MODE == SHADOWS_SOFT (wavefront.h.slang:33-102): a point or spot light with a radius is
// sampled on a disk of half that radius around its position, perpendicular to the direction from the surface to the light
// (buildOrthonormalBasis: Frisvad's basis with its n.z < -0.9999999 branch; sampleDisk: the radius is drawn first, then the angle).
// The two numbers come from the pixel's state `seed` (rgen.slang:228) and are drawn BEFORE the range test, which is decided by the
// sample's distance: a culled light has consumed them.  A directional light, or a radius <= 0, draws nothing and is lightToSurface
// operation for operation.  sqrtf, sinf and cosf are the accurate ones: the float64 restatement's margin rests on their bounds.
__device__ __forceinline__ bool lightToSurfaceSoft(const LightDev& light, V3 worldPos, uint32_t& seed, V3& lightDir, float& lightDist)
{
  if(light.type == MGS_LIGHT_DIRECTIONAL)
  {
    lightDir  = -load3(light.dirN);
    lightDist = 1e10f;
    return true;
  }
  V3 samplePos = load3(light.pos);
  if(light.radius > 0.0f)
  {
    const V3 n = normalize3(load3(light.pos) - worldPos);
    V3       tangent, bitangent;
    if(n.z < -0.9999999f)
    {
      tangent   = {0.0f, -1.0f, 0.0f};
      bitangent = {-1.0f, 0.0f, 0.0f};
    }
    else
    {
      const float a = 1.0f / (1.0f + n.z);
      const float b = -n.x * n.y * a;
      tangent       = {1.0f - n.x * n.x * a, b, -n.x};
      bitangent     = {b, 1.0f - n.y * n.y * a, -n.y};
    }
    const float r     = (light.radius * 0.5f) * sqrtf(rngRand(seed));
    const float theta = 2.0f * 3.14159265f * rngRand(seed);
    samplePos         = samplePos + (tangent * cosf(theta) + bitangent * sinf(theta)) * r;
  }
  const V3 toLight = samplePos - worldPos;
  lightDist        = sqrtf(dot3(toLight, toLight));
  if(lightDist > light.range)
    return false;
  lightDir = toLight * (1.0f / lightDist);
  return true;
}

// wavefrontComputeShadingDirectOnly (wavefront.h.slang:233-280) with transmittance = 1.  SHADOWED: light.color was multiplied by
// the shadow ray's transmittance `shadowT` before the call (rgen.slang:1126), and inShadow returns after the ambient term (:252).
template <bool SHADOWED>
__device__ __forceinline__ void shadeDirectT(const LightDev& light, V3 worldPos, V3 n, const Mat& mat, V3 viewDir, V3 shadowT,
                                             bool inShadow, V3& radiance)
{
  radiance = radiance + mat.ambient;  // ambient once per light, as written
  if(SHADOWED && inShadow)
    return;
  const V3 lightColor = SHADOWED ? load3(light.color) * shadowT : load3(light.color);
  V3       L;
  V3       lightDiffuse = {0.0f, 0.0f, 0.0f};
  if(light.type == MGS_LIGHT_DIRECTIONAL)
  {
    L                 = -load3(light.dirN);
    const float NdotL = fmaxf(dot3(n, L), 0.0f);
    lightDiffuse      = lightColor * light.intensity * NdotL;
  }
  else
  {
    const V3    toLight  = load3(light.pos) - worldPos;
    const float distance = sqrtf(dot3(toLight, toLight));
    L                    = toLight * (1.0f / distance);
    if(!(distance > light.range))
    {
      const float attenuation = attenuate(light.attMode, distance, light.range);
      const float NdotL       = fmaxf(dot3(n, L), 0.0f);
      if(light.type == MGS_LIGHT_POINT)
        lightDiffuse = lightColor * light.intensity * attenuation * NdotL;
      else if(light.type == MGS_LIGHT_SPOT)
      {
        const float theta = dot3(L, -load3(light.dirN));
        if(!(theta < light.outerCos))
        {  // smoothstep(outerCos, innerCos, theta)
          const float t          = fminf(fmaxf((theta - light.outerCos) / (light.innerCos - light.outerCos), 0.0f), 1.0f);
          const float spotEffect = t * t * (3.0f - 2.0f * t);
          lightDiffuse           = lightColor * light.intensity * attenuation * spotEffect * NdotL;
        }
      }
    }
  }
  const V3 fragDiffuse = mat.diffuse * lightDiffuse;
  // wavefrontComputeSpecular (:388-403)
  const float kPi                 = 3.14159265f;
  const float kShininess          = fmaxf(mat.shininess, 4.0f);
  const float kEnergyConservation = (2.0f + kShininess) / (2.0f * kPi);
  const V3    V                   = normalize3(-viewDir);
  const V3    I                   = -L;
  const V3    R                   = I - n * (2.0f * dot3(n, I));  // reflect(-L, n)
  // powf, not the fast intrinsic: with shininess up to 2000 the exponent multiplies the base's relative error, and __powf's own
  // exp2(y * log2(x)) would add ~2000 x 2^-22 on top of it
  const float specular             = kEnergyConservation * powf(fmaxf(dot3(V, R), 0.0f), kShininess);
  const V3    specularContribution = mat.specular * specular * lightColor * light.intensity;
  radiance                         = radiance + (fragDiffuse + specularContribution);
}
// ... with inShadow = false and an unshadowed light: the raster passes
__device__ __forceinline__ void shadeDirect(const LightDev& light, V3 worldPos, V3 n, const Mat& mat, V3 viewDir, V3& radiance)
{
  shadeDirectT<false>(light, worldPos, n, mat, viewDir, V3{1.0f, 1.0f, 1.0f}, false, radiance);
}

}  // namespace

}  // namespace mgs
