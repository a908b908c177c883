// api_math.hip — the entry points of include/mgs.h that touch no device: version, last error, camera and transform helpers.  Built like
// the other units (same compiler, same floating-point contraction), so the matrices come out bit for bit as they always have.
#include <cmath>
#include <cstring>

#include "../../include/mgs.h"
#include "host_model.h"

using namespace mgs;

const char* mgs_last_error(void) { return lastError(); }
const char* mgs_version(void) { return "mgs 0.4 (gfx950, ABI 5.1)"; }

// ------------------------------------------------------------------------------------------------
// build-defined camera helper (nvutils::CameraManipulator is absent)
void mgs_camera_lookat_perspective(const float eye[3], const float center[3], const float up[3], float fovDeg, float zn,
                                   float zf, int width, int height, int flipY, float view[16], float proj[16])
{
  auto norm3 = [](float v[3]) {
    const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
  };
  float f[3] = {center[0] - eye[0], center[1] - eye[1], center[2] - eye[2]};
  norm3(f);
  float sx[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
  norm3(sx);
  const float u[3] = {sx[1] * f[2] - sx[2] * f[1], sx[2] * f[0] - sx[0] * f[2], sx[0] * f[1] - sx[1] * f[0]};
  // right-handed lookAt, column-major
  view[0] = sx[0]; view[4] = sx[1]; view[8]  = sx[2]; view[12] = -(sx[0] * eye[0] + sx[1] * eye[1] + sx[2] * eye[2]);
  view[1] = u[0];  view[5] = u[1];  view[9]  = u[2];  view[13] = -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]);
  view[2] = -f[0]; view[6] = -f[1]; view[10] = -f[2]; view[14] = (f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]);
  view[3] = 0; view[7] = 0; view[11] = 0; view[15] = 1;
  // right-handed perspective, clip z in [0,1]
  const float aspect = (float)width / (float)height;
  const float t      = std::tan(fovDeg * 0.017453292519943295f * 0.5f);
  std::memset(proj, 0, sizeof(float) * 16);
  proj[0]  = 1.0f / (aspect * t);
  proj[5]  = (flipY ? -1.0f : 1.0f) / t;
  proj[10] = zf / (zn - zf);
  proj[11] = -1.0f;
  proj[14] = -(zf * zn) / (zf - zn);
}

// T*R*S with R from Euler angles (degrees) through a quaternion, computeTransform (src/utilities.h:170-199)
void mgs_compute_transform(const float scale[3], const float rotDeg[3], const float tr[3], float M[16], float Minv[16])
{
  const float d2r = 0.017453292519943295f;
  const float hx = rotDeg[0] * d2r * 0.5f, hy = rotDeg[1] * d2r * 0.5f, hz = rotDeg[2] * d2r * 0.5f;
  const float cx = std::cos(hx), sx = std::sin(hx), cy = std::cos(hy), sy = std::sin(hy), cz = std::cos(hz),
              sz = std::sin(hz);
  // [glm] quat(eulerAngles): w = cx*cy*cz + sx*sy*sz, x = sx*cy*cz - cx*sy*sz, y = cx*sy*cz + sx*cy*sz, z = cx*cy*sz - sx*sy*cz
  const float w = cx * cy * cz + sx * sy * sz, x = sx * cy * cz - cx * sy * sz, y = cx * sy * cz + sx * cy * sz,
              z = cx * cy * sz - sx * sy * cz;
  const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y + w * z),     2 * (x * z - w * y),
                      2 * (x * y - w * z),     1 - 2 * (x * x + z * z), 2 * (y * z + w * x),
                      2 * (x * z + w * y),     2 * (y * z - w * x),     1 - 2 * (x * x + y * y)};  // columns
  for(int c = 0; c < 3; ++c)
  {
    for(int r = 0; r < 3; ++r)
      M[c * 4 + r] = R[c * 3 + r] * scale[c];
    M[c * 4 + 3] = 0.f;
  }
  M[12] = tr[0]; M[13] = tr[1]; M[14] = tr[2]; M[15] = 1.f;
  if(Minv)
    mat4Inverse(M, Minv);
}
