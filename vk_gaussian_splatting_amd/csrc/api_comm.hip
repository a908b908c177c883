// api_comm.hip — multi-GPU strips: the RCCL shim, the communicator, strip tables, the gathered frame and the row costs.
#include <dlfcn.h>

#include "scene_state.h"

// ---- RCCL, resolved at first use ------------------------------------------------------------------------------------
namespace {
struct Rccl
{
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*)                                                             = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int)                                      = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t)                                                                = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t)                                                                  = nullptr;
  ncclResult_t (*GroupStart)()                                                                           = nullptr;
  ncclResult_t (*GroupEnd)()                                                                             = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)    = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)         = nullptr;
  const char* (*GetErrorString)(ncclResult_t)                                                            = nullptr;
  bool ok = false;
};
Rccl& rccl()
{
  static Rccl R = [] {
    Rccl r;
    // MGS_RCCL_LIB=path: load THIS library instead (and nothing else if it fails) — the seam of the test double that lets several
    // ranks share one GPU (tests/helpers/fake_rccl.cpp); never set in production, never a fallback
    if(tuning().rcclLib)
      r.lib = dlopen(tuning().rcclLib->c_str(), RTLD_NOW | RTLD_LOCAL);
    else
      for(const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if((r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL)))
          break;
    if(!r.lib)
      return r;
    auto sym = [&](const char* n) { return dlsym(r.lib, n); };
    r.GetUniqueId    = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank   = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy    = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.CommAbort      = (decltype(r.CommAbort))sym("ncclCommAbort");
    r.GroupStart     = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd       = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.Broadcast      = (decltype(r.Broadcast))sym("ncclBroadcast");
    r.AllGather      = (decltype(r.AllGather))sym("ncclAllGather");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Broadcast && r.AllGather;
    return r;
  }();
  return R;
}
int rcclFail(const char* what, ncclResult_t e)
{
  setError(std::string(what) + ": RCCL error " + std::to_string((int)e) + (rccl().GetErrorString ? std::string(" (") + rccl().GetErrorString(e) + ")" : ""));
  return MGS_ERR_DEVICE;
}
}  // namespace

int mgs_comm_unique_id(void* idOut)
{
  static_assert(sizeof(ncclUniqueId) == MGS_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  if(!idOut)
  {
    setError("mgs_comm_unique_id: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!rccl().ok)
  {
    setError("mgs_comm_unique_id: librccl could not be loaded");
    return MGS_ERR_UNSUPPORTED;
  }
  ncclUniqueId id;
  const ncclResult_t e = rccl().GetUniqueId(&id);
  if(e != ncclSuccess)
    return rcclFail("ncclGetUniqueId", e);
  std::memcpy(idOut, &id, sizeof(id));
  return MGS_OK;
}

int mgs_scene_comm_destroy(MgsScene s)
{
  if(!s)
  {
    setError("mgs_scene_comm_destroy: null scene");
    return MGS_ERR_INVALID_ARG;
  }
  if(s->comm.handle)
  {
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    (void)rccl().CommDestroy(s->comm.handle);
    s->comm.handle = nullptr;
  }
  s->comm.rank  = 0;
  s->comm.world = 1;
  return MGS_OK;
}

int mgs_scene_comm_init(MgsScene s, int rank, int world, const void* id)
{
  if(!s || !id || world < 1 || rank < 0 || rank >= world)
  {
    setError("mgs_scene_comm_init: bad argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!rccl().ok)
  {
    setError("mgs_scene_comm_init: librccl could not be loaded");
    return MGS_ERR_UNSUPPORTED;
  }
  (void)mgs_scene_comm_destroy(s);
  HIPCHK(hipSetDevice(s->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  const ncclResult_t e = rccl().CommInitRank(&s->comm.handle, world, uid, rank);
  if(e != ncclSuccess)
  {
    s->comm.handle = nullptr;
    return rcclFail("ncclCommInitRank", e);
  }
  s->comm.rank  = rank;
  s->comm.world = world;
  s->comm.stripBounds.clear();
  return MGS_OK;
}

int mgs_scene_set_strip_rows(MgsScene s, const int32_t* bounds, int count)
{
  if(!s)
  {
    setError("mgs_scene_set_strip_rows: null scene");
    return MGS_ERR_INVALID_ARG;
  }
  if(!bounds)
  {
    s->comm.stripBounds.clear();
    return MGS_OK;
  }
  if(count != s->comm.world + 1 || bounds[0] != 0)
  {
    setError("mgs_scene_set_strip_rows: need world_size + 1 ascending tile-row bounds starting at 0");
    return MGS_ERR_INVALID_ARG;
  }
  for(int i = 0; i < count - 1; ++i)
    if(bounds[i + 1] < bounds[i])
    {
      setError("mgs_scene_set_strip_rows: bounds must be ascending");
      return MGS_ERR_INVALID_ARG;
    }
  s->comm.stripBounds.assign(bounds, bounds + count);
  return MGS_OK;
}

static void stripOfRank(MgsScene s, int tilesY, int r, int& b, int& e)
{
  if(!s->comm.stripBounds.empty())
  {
    b = std::min(s->comm.stripBounds[r], tilesY);
    e = std::min(s->comm.stripBounds[r + 1], tilesY);
    if(r == s->comm.world - 1)
      e = tilesY;  // the last strip takes whatever the table left over
    return;
  }
  const int per = (tilesY + s->comm.world - 1) / s->comm.world;
  b             = std::min(r * per, tilesY);
  e             = std::min(b + per, tilesY);
}

// the frame buffer of a rank that does not render this frame (empty strip) or whose render failed: the exchange still
// receives everybody else's rows into it
static int ensureFrameBufferFor(MgsScene s, const MgsFrameParams* p)
{
  if(p->width <= 0 || p->height <= 0 || p->target_format < MGS_TARGET_RGBA16F || p->target_format > MGS_TARGET_RGBA8)
  {
    setError("frame: bad size / target_format");
    return MGS_ERR_INVALID_ARG;
  }
  s->fb.imageRowBytes  = (size_t)p->width * targetLayout(p->target_format).pixelBytes;
  s->fb.imageBytes     = s->fb.imageRowBytes * (size_t)p->height;
  if(s->fb.image.n < s->fb.imageBytes)
  {
    HIPCHK(hipStreamSynchronize(s->stream));
    s->graphs.drop();  // captured frames hold the old image pointer
    int rc = s->fb.image.ensure(s->fb.imageBytes);
    if(rc != MGS_OK)
      return rc;
    HIPCHK(hipMemsetAsync(s->fb.image.p, 0, s->fb.imageBytes, s->stream));
  }
  return MGS_OK;
}

static int mgs_render_gathered_impl(MgsScene s, const MgsFrameParams* p, MgsFrameOut* out)
{
  if(!s || !p)
  {
    setError("mgs_render_gathered: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->comm.handle)
  {
    setError("mgs_render_gathered: call mgs_scene_comm_init first");
    return MGS_ERR_STATE;
  }
  const int tilesY = (p->height + kTilePx - 1) / kTilePx;
  MgsFrameParams q = *p;
  int b, e;
  stripOfRank(s, tilesY, s->comm.rank, b, e);
  // A rank must reach the exchange whatever happens to its own strip: the peers block in the collective otherwise.  A failed
  // (or absent) local render still joins with a frame buffer of the right size — its rows are stale, the error is returned
  // after the exchange.  Only if no buffer can be had at all is the communicator aborted, which fails the peers' collective
  // instead of hanging it.
  int         localRc = MGS_OK;
  std::string localErr;
  if(e > b)
  {
    q.strip_row_begin = b;
    q.strip_row_end   = e;
    localRc           = mgs_render(s, &q, out);
  }
  else if(out)
    std::memset(out, 0, sizeof(*out));  // more ranks than tile rows (or an empty strip in the table): nothing to render
  if(localRc != MGS_OK)
    localErr = lastError();
  HIPCHK(hipSetDevice(s->device));
  const int bufRc = ensureFrameBufferFor(s, p);
  if(bufRc != MGS_OK)
  {
    if(rccl().CommAbort)
      (void)rccl().CommAbort(s->comm.handle);
    else
      (void)rccl().CommDestroy(s->comm.handle);
    s->comm.handle      = nullptr;
    s->comm.world = 1;
    s->comm.rank  = 0;
    return localRc != MGS_OK ? localRc : bufRc;
  }
  // exchange in place: rank r's rows are broadcast from r into the same rows of everybody's frame buffer.  One group
  // = one fused launch on the render stream; it overlaps with the next frame's key/sort when frames are in flight.
  ncclResult_t ne = rccl().GroupStart();
  if(ne != ncclSuccess)
    return rcclFail("ncclGroupStart", ne);
  for(int r = 0; r < s->comm.world; ++r)
  {
    int rb, re;
    stripOfRank(s, tilesY, r, rb, re);
    const int    y0 = rb * kTilePx, y1 = std::min(re * kTilePx, p->height);
    if(y1 <= y0)
      continue;
    uint8_t*     ptr = s->fb.image.p + (size_t)y0 * s->fb.imageRowBytes;
    const size_t n   = (size_t)(y1 - y0) * s->fb.imageRowBytes;
    ne               = rccl().Broadcast(ptr, ptr, n, ncclUint8, r, s->comm.handle, s->stream);
    if(ne != ncclSuccess)
    {
      (void)rccl().GroupEnd();
      return rcclFail("ncclBroadcast", ne);
    }
  }
  ne = rccl().GroupEnd();
  if(ne != ncclSuccess)
    return rcclFail("ncclGroupEnd", ne);
  if(localRc != MGS_OK)
  {
    setError("mgs_render_gathered: this rank's strip failed (" + localErr + "); the exchange was still joined");
    return localRc;
  }
  // the frame is whole again: downloads address all rows.  The bin lists of the last frame cover this rank's rows only.
  s->last.params                 = q;
  s->last.params.strip_row_begin = 0;
  s->last.params.strip_row_end   = tilesY;
  s->last.have                  = true;
  s->last.wasSortOnly            = false;
  s->last.listsPartial           = s->comm.world > 1;
  return MGS_OK;
}
int mgs_render_gathered(MgsScene s, const MgsFrameParams* p, MgsFrameOut* out)
{
  return guarded("mgs_render_gathered", [&] { return mgs_render_gathered_impl(s, p, out); });
}

int mgs_frame_row_costs(MgsScene s, uint32_t* cost, size_t rows)
{
  if(!s || !cost)
  {
    setError("mgs_frame_row_costs: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have || s->last.wasSortOnly)
  {
    setError("mgs_frame_row_costs: no frame rendered yet");
    return MGS_ERR_STATE;
  }
  if(s->last.listsPartial)
  {  // every rank would see its own rows only and derive a different table: the exchange sizes would no longer agree
    setError("mgs_frame_row_costs: the last frame came from mgs_render_gathered (bin lists of this rank's strip only); "
             "calibrate on a full-frame mgs_render");
    return MGS_ERR_STATE;
  }
  return guarded("mgs_frame_row_costs", [&]() -> int {
    FrameArgs A;
    int       rc = buildFrameArgs(s, &s->last.params, A);
    if(rc != MGS_OK)
      return rc;
    FrameConst& F = A.f;
    // the lists are those of the LAST frame: its bin grid, not the one the adaptive policy would pick for the next frame
    F.binShiftX = s->last.binShift[0];
    F.binShiftY = s->last.binShift[1];
    F.binsX     = (F.tilesX + (1 << F.binShiftX) - 1) >> F.binShiftX;
    F.binsY     = (F.tilesY + (1 << F.binShiftY) - 1) >> F.binShiftY;
    if(rows < (size_t)F.tilesY)
    {
      setError("mgs_frame_row_costs: need one entry per 16-pixel tile row");
      return MGS_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    const int          bins = F.binsX * F.binsY;
    std::vector<uint2> rg((size_t)bins);
    HIPCHK(hipMemcpy(rg.data(), s->fb.ranges.p, (size_t)bins * sizeof(uint2), hipMemcpyDeviceToHost));
    std::vector<double> acc((size_t)F.tilesY, 0.0);
    const int           rowsPerBin = 1 << F.binShiftY;
    for(int by = 0; by < F.binsY; ++by)
    {
      double len = 0;
      for(int bx = 0; bx < F.binsX; ++bx)
        len += (double)(rg[(size_t)by * F.binsX + bx].y - rg[(size_t)by * F.binsX + bx].x);
      const int r0 = by * rowsPerBin, r1 = std::min(r0 + rowsPerBin, F.tilesY);
      for(int r = r0; r < r1; ++r)
        acc[(size_t)r] += len / (double)(r1 - r0);
    }
    for(int r = 0; r < F.tilesY; ++r)
      cost[r] = (uint32_t)std::min(acc[(size_t)r], 4.0e9);
    for(size_t r = (size_t)F.tilesY; r < rows; ++r)
      cost[r] = 0u;
    return MGS_OK;
  });
}
