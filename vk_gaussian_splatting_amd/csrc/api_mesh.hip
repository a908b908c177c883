// api_mesh.hip — triangle meshes: the RAM model, the scene's mesh instances and the mesh pass (mgs_mesh_*, mgs_meshes_*).
//
// Replaces ObjLoader (src/obj_loader.cpp), MeshManagerVk's instances (src/mesh_manager_vk.cpp) and
// GaussianSplatting::drawMeshPrimitives (src/gaussian_splatting.cpp:1467-1525).  The pass writes the handle's owned occluder images
// and binds them, so the following frames composite the splats with the meshes through the occluder path as it is.
#include <cmath>

#include "scene_state.h"

static MaterialDev meshMaterialToDevice(const HostMeshMaterial& m)
{
  MaterialDev d{};
  std::memcpy(d.ambient, m.ambient, 12);
  std::memcpy(d.diffuse, m.diffuse, 12);
  std::memcpy(d.specular, m.specular, 12);
  std::memcpy(d.emission, m.emission, 12);
  d.shininess = m.shininess;
  auto len = [](const float* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
  d.needShading = (len(m.diffuse) > 0.001f || len(m.ambient) > 0.001f || len(m.specular) > 0.001f) ? 1 : 0;  // wavefront.h:55-59
  return d;
}

// ---- the RAM model ------------------------------------------------------------------------------------------------------------
static int mgs_mesh_from_arrays_impl(const MgsMeshView* v, MgsMesh* out)
{
  if(!v || !out || !v->positions || !v->indices || v->vertex_count == 0 || v->index_count == 0 || v->index_count % 3 != 0
     || (v->material_count != 0 && !v->materials))
  {
    setError("mgs_mesh_from_arrays: null argument, no vertices, or an index count that is no multiple of three");
    return MGS_ERR_INVALID_ARG;
  }
  if(v->vertex_count > 0xFFFFFFFFull || v->index_count / 3 >= kMeshMaxPrims)
  {
    setError("mgs_mesh_from_arrays: more than 2^32 - 1 vertices or 2^29 - 1 triangles");
    return MGS_ERR_UNSUPPORTED;
  }
  for(uint64_t i = 0; i < v->index_count; ++i)
    if(v->indices[i] >= v->vertex_count)
    {
      setError("mgs_mesh_from_arrays: index " + std::to_string(i) + " is " + std::to_string(v->indices[i]) + ", the mesh has " + std::to_string(v->vertex_count) + " vertices");
      return MGS_ERR_INVALID_ARG;
    }
  auto m = std::make_shared<HostMesh>();
  m->positions.assign(v->positions, v->positions + 3 * v->vertex_count);
  m->indices.assign(v->indices, v->indices + v->index_count);
  if(v->normals)
    m->normals.assign(v->normals, v->normals + 3 * v->vertex_count);
  else
  {
    std::vector<uint8_t> visited(v->vertex_count, 0);
    m->normals.assign(3 * v->vertex_count, 0.0f);
    accumulateFaceNormals(m->positions.data(), m->indices.data(), m->indices.size(), m->normals, visited);
  }
  if(v->material_count == 0)
    m->materials.push_back(defaultMeshMaterial());
  else
    for(uint32_t k = 0; k < v->material_count; ++k)
    {
      HostMeshMaterial h{};
      std::memcpy(&h, &v->materials[k], sizeof(h));
      m->materials.push_back(h);
    }
  m->materialIds.assign(v->index_count / 3, 0u);
  if(v->material_ids)
    for(size_t t = 0; t < m->materialIds.size(); ++t)
      m->materialIds[t] = v->material_ids[t] >= m->materials.size() ? 0u : v->material_ids[t];  // obj_loader.cpp:190-196
  *out = new MgsMesh_t{m};
  return MGS_OK;
}
static_assert(sizeof(HostMeshMaterial) == sizeof(MgsMaterial), "the RAM model keeps MgsMaterial's fields");
int mgs_mesh_from_arrays(const MgsMeshView* v, MgsMesh* out)
{
  return guarded("mgs_mesh_from_arrays", [&] { return mgs_mesh_from_arrays_impl(v, out); });
}

int mgs_mesh_load_obj(const char* path, MgsMesh* out)
{
  return guarded("mgs_mesh_load_obj", [&]() -> int {
    if(!path || !out)
    {
      setError("mgs_mesh_load_obj: null argument");
      return (int)MGS_ERR_INVALID_ARG;
    }
    auto m = std::make_shared<HostMesh>();
    if(int rc = loadObj(path, *m))
      return rc;
    if(m->indices.size() / 3 >= kMeshMaxPrims)
    {
      setError("mgs_mesh_load_obj: 2^29 or more triangles");
      return (int)MGS_ERR_UNSUPPORTED;
    }
    *out = new MgsMesh_t{m};
    return (int)MGS_OK;
  });
}

int mgs_mesh_view(MgsMesh mesh, MgsMeshView* out)
{
  if(!mesh || !out)
  {
    setError("mgs_mesh_view: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  const HostMesh& m   = *mesh->data;
  out->positions      = m.positions.data();
  out->normals        = m.normals.data();
  out->indices        = m.indices.data();
  out->material_ids   = m.materialIds.data();
  out->materials      = reinterpret_cast<const MgsMaterial*>(m.materials.data());
  out->vertex_count   = m.positions.size() / 3;
  out->index_count    = m.indices.size();
  out->material_count = (uint32_t)m.materials.size();
  return MGS_OK;
}

void mgs_mesh_destroy(MgsMesh mesh) { delete mesh; }

// ---- the scene's mesh instances -----------------------------------------------------------------------------------------------
// inverse(mat3(transform)) in double, rounded once (glm::inverse is not part of the reference tree: PARITY UNPINNED)
void rotScaleInverse(const float M[16], float out[9])
{
  double a[3][3];
  for(int r = 0; r < 3; ++r)
    for(int c = 0; c < 3; ++c)
      a[r][c] = (double)M[c * 4 + r];
  const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
  const double inv[3][3] = {{c00 / det, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det},
                            {c01 / det, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det},
                            {c02 / det, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det}};
  for(int r = 0; r < 3; ++r)
    for(int c = 0; c < 3; ++c)
      out[c * 3 + r] = (float)inv[r][c];
}

template <class T>
static int uploadVector(DevBuf<T>& dst, const T* src, size_t count)
{
  if(int rc = dst.ensure(count))
    return rc;
  HIPCHK(hipMemcpy(dst.p, src, count * sizeof(T), hipMemcpyHostToDevice));
  return MGS_OK;
}

// rebuilds the host table from the instance list and rewrites the device copy, after the frames in flight on every handle of the
// scene are done (the rule of mgs_scene_set_lights)
static int rewriteMeshTable(SceneData& d)
{
  HIPCHK(hipSetDevice(d.device));
  if(!d.meshHost)
    d.meshHost.reset(new MeshTable());
  MeshTable& T = *d.meshHost;
  std::memset(&T, 0, sizeof(T));
  uint32_t tri = 0;
  for(size_t k = 0; k < d.meshInstances.size(); ++k)
  {
    const MeshInstance& I = d.meshInstances[k];
    const DeviceMesh&   m = d.meshes[I.mesh];
    MeshInstDev&        D = T.inst[k];
    D.pos   = m.pos.p;
    D.nrm   = m.nrm.p;
    D.idx   = m.idx.p;
    D.matId = m.matId.p;
    D.mats  = m.mats.p;
    std::memcpy(D.M, I.M, sizeof(D.M));
    rotScaleInverse(I.M, D.rsInv);
    D.triBegin = tri;
    D.triCount = (uint32_t)(m.host->indices.size() / 3);
    D.visible  = I.visible ? 1u : 0u;
    tri += D.triCount;
  }
  T.count     = (uint32_t)d.meshInstances.size();
  T.totalTris = tri;
  {
    std::lock_guard<std::mutex> lk(d.mtx);
    for(MgsScene_t* h : d.handles)
      HIPCHK(hipStreamSynchronize(h->stream));
  }
  if(int rc = d.meshTab.ensure(1))
    return rc;
  const size_t bytes = offsetof(MeshTable, inst) + std::max<size_t>(T.count, 1) * sizeof(MeshInstDev);
  HIPCHK(hipMemcpy(d.meshTab.p, &T, bytes, hipMemcpyHostToDevice));
  return MGS_OK;
}

static int editable(MgsScene s, const char* who)
{
  if(!s)
  {
    setError(std::string(who) + ": null handle");
    return MGS_ERR_INVALID_ARG;
  }
  if(s->isContext)
  {
    setError(std::string(who) + ": a frame context is read-only; the mesh instances belong to the scene it was created from");
    return MGS_ERR_STATE;
  }
  return MGS_OK;
}

static int mgs_mesh_instance_add_impl(MgsScene s, MgsMesh mesh, const float M[16], int* id)
{
  if(int rc = editable(s, "mgs_mesh_instance_add"))
    return rc;
  if(!mesh || !M)
  {
    setError("mgs_mesh_instance_add: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  SceneData& d = *s->d;
  uint64_t   tris = mesh->data->indices.size() / 3;
  for(const auto& I : d.meshInstances)
    tris += d.meshes[I.mesh].host->indices.size() / 3;
  if((int)d.meshInstances.size() >= kMaxMeshInstances || tris >= kMeshMaxPrims)
  {
    setError("mgs_mesh_instance_add: at most " + std::to_string(kMaxMeshInstances) + " mesh instances and 2^29 - 1 triangles per scene in this build");
    return MGS_ERR_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(d.device));
  int idx = -1;
  for(size_t i = 0; i < d.meshes.size(); ++i)
    if(d.meshes[i].host == mesh->data)
      idx = (int)i;
  if(idx < 0)
  {
    DeviceMesh      m;
    const HostMesh& h = *mesh->data;
    m.host            = mesh->data;
    std::vector<MaterialDev> mats;
    for(const auto& hm : h.materials)
      mats.push_back(meshMaterialToDevice(hm));
    int rc = uploadVector(m.pos, h.positions.data(), h.positions.size());
    rc     = rc ? rc : uploadVector(m.nrm, h.normals.data(), h.normals.size());
    rc     = rc ? rc : uploadVector(m.idx, h.indices.data(), h.indices.size());
    rc     = rc ? rc : uploadVector(m.matId, h.materialIds.data(), h.materialIds.size());
    rc     = rc ? rc : uploadVector(m.mats, mats.data(), mats.size());
    if(rc)
    {
      m.release();
      return rc;
    }
    d.meshes.push_back(m);
    idx = (int)d.meshes.size() - 1;
  }
  MeshInstance I;
  I.mesh = idx;
  std::memcpy(I.M, M, sizeof(I.M));
  d.meshInstances.push_back(I);
  if(int rc = rewriteMeshTable(d))
  {
    d.meshInstances.pop_back();
    return rc;
  }
  if(id)
    *id = (int)d.meshInstances.size() - 1;
  return MGS_OK;
}
int mgs_mesh_instance_add(MgsScene s, MgsMesh mesh, const float M[16], int* id)
{
  return guarded("mgs_mesh_instance_add", [&] { return mgs_mesh_instance_add_impl(s, mesh, M, id); });
}

int mgs_mesh_instance_set_transform(MgsScene s, int id, const float M[16])
{
  return guarded("mgs_mesh_instance_set_transform", [&]() -> int {
    if(int rc = editable(s, "mgs_mesh_instance_set_transform"))
      return rc;
    if(!M || id < 0 || id >= (int)s->d->meshInstances.size())
    {
      setError("mgs_mesh_instance_set_transform: bad argument");
      return (int)MGS_ERR_INVALID_ARG;
    }
    std::memcpy(s->d->meshInstances[id].M, M, sizeof(float) * 16);
    return rewriteMeshTable(*s->d);
  });
}

int mgs_mesh_instance_set_visible(MgsScene s, int id, int visible)
{
  return guarded("mgs_mesh_instance_set_visible", [&]() -> int {
    if(int rc = editable(s, "mgs_mesh_instance_set_visible"))
      return rc;
    if(id < 0 || id >= (int)s->d->meshInstances.size())
    {
      setError("mgs_mesh_instance_set_visible: bad argument");
      return (int)MGS_ERR_INVALID_ARG;
    }
    s->d->meshInstances[id].visible = visible != 0;
    return rewriteMeshTable(*s->d);
  });
}

// ---- bounce materials (mgs_render_traced_indirect) -------------------------------------------------------------------------------
static_assert(sizeof(BounceMatDev) == sizeof(MgsBounceMaterial) && sizeof(MgsBounceMaterial) == 32, "the kernels read MgsBounceMaterial as it is");
static_assert(sizeof(MgsTraceBounceParams) == 16 && sizeof(MgsTraceBounceOut) == 272, "documented sizes");

void mgs_bounce_material_default(MgsBounceMaterial* m)
{
  if(!m)
    return;
  std::memset(m, 0, sizeof(*m));
  m->ior = 1.0f;
}

// src/obj_loader.cpp:50-59 as written: transmittance.x is tested twice and .z never
void mgs_bounce_material_from_mtl(const float tf[3], float ni, int mtl_illum, MgsBounceMaterial* out)
{
  if(!out)
    return;
  mgs_bounce_material_default(out);
  if(tf)
    std::memcpy(out->transmittance, tf, 12);
  out->ior = ni;
  if(out->transmittance[0] != 0.0f || out->transmittance[1] != 0.0f || out->transmittance[0] != 0.0f)
    out->illum = 2;  // refractive
  else if(mtl_illum > 1)
    out->illum = 1;  // reflective
  else
    out->illum = 0;
}

// what the mesh's material library says, through the loader's rule; a mesh from arrays has no library: defaults
int mgs_mesh_bounce_materials(MgsMesh mesh, MgsBounceMaterial* out, uint32_t capacity, uint32_t* count)
{
  if(!mesh || !count || (capacity > 0 && !out))
  {
    setError("mgs_mesh_bounce_materials: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  const HostMesh& m = *mesh->data;
  const uint32_t  n = (uint32_t)m.materials.size();
  *count = n;
  if(capacity < n)
  {
    if(capacity == 0)
      return MGS_OK;  // the size query
    setError("mgs_mesh_bounce_materials: the mesh has " + std::to_string(n) + " materials, the destination holds " + std::to_string(capacity));
    return MGS_ERR_INVALID_ARG;
  }
  for(uint32_t k = 0; k < n; ++k)
  {
    if(k < m.mtlBounce.size())
      mgs_bounce_material_from_mtl(m.mtlBounce[k].tf, m.mtlBounce[k].ni, m.mtlBounce[k].illum, &out[k]);
    else
      mgs_bounce_material_default(&out[k]);
  }
  return MGS_OK;
}

// rebuilds the flat array and the per-instance slices and rewrites the device copies, after the frames in flight on every handle of
// the scene are done (the rule of mgs_scene_set_lights).  The triangle hierarchy does not depend on them.
static int rewriteBounceTable(SceneData& d)
{
  HIPCHK(hipSetDevice(d.device));
  auto                      T = std::make_unique<BounceTable>();
  std::vector<BounceMatDev> flat;
  std::memset(T.get(), 0, sizeof(BounceTable));
  for(size_t k = 0; k < d.bounceMats.size() && k < (size_t)kMaxMeshInstances; ++k)
  {
    T->offset[k] = (uint32_t)flat.size();
    T->count[k]  = (uint32_t)d.bounceMats[k].size();
    flat.insert(flat.end(), d.bounceMats[k].begin(), d.bounceMats[k].end());
  }
  {
    std::lock_guard<std::mutex> lk(d.mtx);
    for(MgsScene_t* h : d.handles)
      HIPCHK(hipStreamSynchronize(h->stream));
  }
  if(int rc = d.bounceTab.ensure(1))
    return rc;
  if(int rc = d.bounceMatsDev.ensure(std::max<size_t>(flat.size(), 1)))
    return rc;
  if(!flat.empty())
    HIPCHK(hipMemcpy(d.bounceMatsDev.p, flat.data(), flat.size() * sizeof(BounceMatDev), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.bounceTab.p, T.get(), sizeof(BounceTable), hipMemcpyHostToDevice));
  return MGS_OK;
}

// The caller holds d.meshBvh.mtx (an indirect frame's set-up does, from traceMeshSetUp to its last launch): two contexts' first
// indirect frames, or a frame and mgs_mesh_instance_set_bounce_materials, never create or rewrite the copies at the same time.
int ensureBounceTable(SceneData& d)
{
  return d.bounceTab.p ? (int)MGS_OK : rewriteBounceTable(d);
}

int mgs_mesh_instance_set_bounce_materials(MgsScene s, int id, const MgsBounceMaterial* m, uint32_t count)
{
  return guarded("mgs_mesh_instance_set_bounce_materials", [&]() -> int {
    // (before the handle is looked at: the values can be checked without a device)
    if(count > 0 && !m)
    {
      setError("mgs_mesh_instance_set_bounce_materials: null materials with a count");
      return (int)MGS_ERR_INVALID_ARG;
    }
    for(uint32_t k = 0; k < count; ++k)
    {
      const MgsBounceMaterial& b = m[k];
      const bool finite = std::isfinite(b.transmittance[0]) && std::isfinite(b.transmittance[1]) && std::isfinite(b.transmittance[2]) && std::isfinite(b.ior);
      if(!finite || (b.illum >= 2 && !(b.ior > 0.0f)) || b.reserved[0] != 0 || b.reserved[1] != 0 || b.reserved[2] != 0)
      {
        setError("mgs_mesh_instance_set_bounce_materials: material " + std::to_string(k)
                 + ": the fields must be finite, ior > 0 for illum >= 2, and the reserved words 0");
        return (int)MGS_ERR_INVALID_ARG;
      }
    }
    if(int rc = editable(s, "mgs_mesh_instance_set_bounce_materials"))
      return rc;
    SceneData& d = *s->d;
    if(id < 0 || id >= (int)d.meshInstances.size())
    {
      setError("mgs_mesh_instance_set_bounce_materials: no such mesh instance");
      return (int)MGS_ERR_INVALID_ARG;
    }
    if(d.bounceMats.size() < d.meshInstances.size())
      d.bounceMats.resize(d.meshInstances.size());
    std::vector<BounceMatDev> v(count);
    if(count)
      std::memcpy(v.data(), m, (size_t)count * sizeof(BounceMatDev));
    std::lock_guard<std::mutex> tables(d.meshBvh.mtx);  // (an indirect frame's set-up on any context holds it while it looks at the copies)
    d.bounceMats[id] = std::move(v);
    return rewriteBounceTable(d);
  });
}

// ---- the pass -------------------------------------------------------------------------------------------------------------------
// translation of inverse(view), in double, rounded once: for a view matrix [R t; 0 1] the general inverse is taken, as the lighting
// pass does for viewInverse
static void viewOrigin(const float V[16], float out[3])
{
  double a[4][5];
  for(int r = 0; r < 4; ++r)
  {
    for(int c = 0; c < 4; ++c)
      a[r][c] = (double)V[c * 4 + r];
    a[r][4] = r == 3 ? 1.0 : 0.0;  // solve V x = (0, 0, 0, 1)
  }
  for(int k = 0; k < 4; ++k)
  {
    int piv = k;
    for(int r = k + 1; r < 4; ++r)
      if(std::fabs(a[r][k]) > std::fabs(a[piv][k]))
        piv = r;
    for(int c = 0; c < 5; ++c)
      std::swap(a[k][c], a[piv][c]);
    const double dd = 1.0 / a[k][k];
    for(int c = 0; c < 5; ++c)
      a[k][c] *= dd;
    for(int r = 0; r < 4; ++r)
      if(r != k)
      {
        const double f = a[r][k];
        for(int c = 0; c < 5; ++c)
          a[r][c] -= f * a[k][c];
      }
  }
  for(int c = 0; c < 3; ++c)
    out[c] = (float)a[c][4];
}

static int mgs_meshes_render_impl(MgsScene s, const MgsFrameParams* p, MgsMeshOut* out)
{
  if(!s || !p)
  {
    setError("mgs_meshes_render: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(p->width <= 0 || p->height <= 0 || p->width > 8192 || p->height > 8192)
  {
    setError("mgs_meshes_render: width and height must be in 1..8192");
    return MGS_ERR_INVALID_ARG;
  }
  if(p->lighting_mode < MGS_LIGHTING_DISABLED || p->lighting_mode > MGS_LIGHTING_INDIRECT)
  {
    setError("mgs_meshes_render: lighting_mode must be one of MGS_LIGHTING_*");
    return MGS_ERR_INVALID_ARG;
  }
  const int tileRows = (p->height + kTilePx - 1) / kTilePx;
  int       t0 = 0, t1 = tileRows;
  if(!(p->strip_row_begin == 0 && p->strip_row_end == 0))
  {
    t0 = p->strip_row_begin;
    t1 = std::min(p->strip_row_end, tileRows);
    if(t0 < 0 || t0 > t1)
    {
      setError("mgs_meshes_render: bad strip rows");
      return MGS_ERR_INVALID_ARG;
    }
  }
  if(int rc = refuseBoundSensor(s, "mgs_meshes_render", "the mesh pass rasterises through view / proj, which has no distortion"))
    return rc;
  SceneData& d = *s->d;
  HIPCHK(hipSetDevice(s->device));
  const size_t n = (size_t)p->width * (size_t)p->height;
  if(p->lighting_mode != MGS_LIGHTING_DISABLED)
    if(int rc = ensureLightTable(d))
      return rc;
  if(!d.meshTab.p)
    if(int rc = rewriteMeshTable(d))  // no instance yet: an empty table
      return rc;
  const uint32_t totalTris = d.meshHost->totalTris;
  uint64_t       trisIn    = 0;
  for(uint32_t k = 0; k < d.meshHost->count; ++k)
    trisIn += d.meshHost->inst[k].visible ? d.meshHost->inst[k].triCount : 0u;

  MeshPassState& m = s->mesh;
  // buffers that have to grow may still be read by work in flight on this handle (and captured frames point at the occluder images)
  const size_t clipCap = 2 * (size_t)totalTris + 64;
  if(n > m.vis.n || n > m.prim.n || totalTris > m.recs.n || clipCap > m.clips.n || n > s->occ.ownDepth.n || 4 * n > s->occ.ownColor.n)
  {
    HIPCHK(hipStreamSynchronize(s->stream));
    if(n > s->occ.ownDepth.n && s->surf.lastOccDepth == s->occ.ownDepth.p && s->surf.lastOccDepth)
      s->surf.lastOccGone = true;
  }
  int rc = m.vis.ensure(n);
  rc     = rc ? rc : m.prim.ensure(n);
  rc     = rc ? rc : m.recs.ensure(totalTris);
  rc     = rc ? rc : m.clips.ensure(clipCap);
  rc     = rc ? rc : m.work.ensure(tuning().meshWorkItems);
  rc     = rc ? rc : m.ctr.ensure(1);
  rc     = rc ? rc : s->occ.ownDepth.ensure(n);
  rc     = rc ? rc : s->occ.ownColor.ensure(4 * n);
  if(rc)
    return rc;

  MeshPassArgs a{};
  std::memcpy(a.view, p->view, sizeof(a.view));
  std::memcpy(a.proj, p->proj, sizeof(a.proj));
  viewOrigin(p->view, a.origin);
  std::memcpy(a.cameraPos, p->camera_pos, sizeof(a.cameraPos));
  a.width        = p->width;
  a.height       = p->height;
  a.row0         = std::min(t0 * kTilePx, p->height);
  a.row1         = std::min(t1 * kTilePx, p->height);
  a.lightingMode = p->lighting_mode;
  a.table        = d.meshTab.p;
  a.lights       = d.lightTab.p;
  a.vis          = m.vis.p;
  a.recs         = m.recs.p;
  a.clips        = m.clips.p;
  a.clipCapacity = (uint32_t)std::min<size_t>(m.clips.n, 0xFFFFFFFFu);
  a.work         = m.work.p;
  a.workCapacity = tuning().meshWorkItems;
  a.ctr          = m.ctr.p;
  a.outDepth     = s->occ.ownDepth.p;
  a.outColor     = reinterpret_cast<float4*>(s->occ.ownColor.p);
  a.outPrim      = m.prim.p;

  if(out && !m.ev[0])
    for(auto& e : m.ev)
      HIPCHK(hipEventCreate(&e));
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
  if(out)
    HIPCHK(hipEventRecord(m.ev[0], s->stream));
  launchMeshPass(s->stream, a, trisIn ? totalTris : 0u, (uint32_t)std::max(cus, 1) * 4u);
  HIPCHK(hipGetLastError());
  if(out)
    HIPCHK(hipEventRecord(m.ev[1], s->stream));
  m.w    = p->width;
  m.h    = p->height;
  m.have = true;
  if(int rc2 = mgs_frame_set_occluder(s, s->occ.ownDepth.p, s->occ.ownColor.p, p->width, p->height))
    return rc2;
  if(out)
  {
    MeshCounters c{};
    HIPCHK(hipMemcpyAsync(&c, m.ctr.p, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    std::memset(out, 0, sizeof(*out));
    out->triangles_in         = trisIn;
    out->triangles_rasterised = c.trisRasterised;
    out->fragments            = c.fragments;
    out->flags                = (c.flags & 2u) ? MGS_MESH_WORK_LIST_FULL : 0u;
    HIPCHK(hipEventElapsedTime(&out->elapsed_ms, m.ev[0], m.ev[1]));
    if(c.flags & 1u)
    {
      setError("mgs_meshes_render: more clipped triangles than the clip records hold (2 per triangle); some geometry was dropped");
      return MGS_ERR_OVERFLOW;
    }
  }
  return MGS_OK;
}
int mgs_meshes_render(MgsScene s, const MgsFrameParams* p, MgsMeshOut* out)
{
  return guarded("mgs_meshes_render", [&] { return mgs_meshes_render_impl(s, p, out); });
}

int mgs_meshes_download(MgsScene s, int which, void* dst, size_t bytes)
{
  return guarded("mgs_meshes_download", [&]() -> int {
    if(!s || !dst || which < 0 || which > 2)
    {
      setError("mgs_meshes_download: bad argument");
      return (int)MGS_ERR_INVALID_ARG;
    }
    if(!s->mesh.have)
    {
      setError("mgs_meshes_download: no mesh pass has run on this handle");
      return (int)MGS_ERR_STATE;
    }
    const size_t n    = (size_t)s->mesh.w * (size_t)s->mesh.h;
    const size_t need = n * (which == 1 ? 16 : 4);
    if(bytes < need)
    {
      setError("mgs_meshes_download: the destination holds " + std::to_string(bytes) + " bytes, the image " + std::to_string(need));
      return (int)MGS_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(s->device));
    const void* src = which == 0 ? (const void*)s->occ.ownDepth.p : which == 1 ? (const void*)s->occ.ownColor.p : (const void*)s->mesh.prim.p;
    HIPCHK(hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return (int)MGS_OK;
  });
}
