// api_sets.hip — splat sets (load, build from arrays, view) and the asynchronous loader of include/mgs.h.
#include <deque>

#include "scene_state.h"

static int mgs_splatset_load_impl(const char* path, MgsSplatSet* out)
{
  if(!path || !out)
  {
    setError("mgs_splatset_load: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  std::string p(path), ext;
  const auto  dot = p.find_last_of('.');
  if(dot != std::string::npos)
    ext = p.substr(dot);
  for(auto& c : ext)
    c = (char)std::tolower((unsigned char)c);  // hasExtension lower-cases, src/utilities.h:65-70
  auto set = std::make_shared<HostSplatSet>();
  int  rc;
  if(ext == ".splat")
    rc = loadSplat(p, *set);
  else if(ext == ".spz")
    rc = loadSpz(p, *set);
  else
    rc = loadPly(p, *set);  // the reference hands every other extension to miniply
  if(rc != MGS_OK)
    return rc;
  *out = new MgsSplatSet_t{set};
  return MGS_OK;
}
int mgs_splatset_load(const char* path, MgsSplatSet* out)
{
  return guarded("mgs_splatset_load", [&] { return mgs_splatset_load_impl(path, out); });
}

static int mgs_splatset_from_arrays_impl(const MgsSplatSetView* v, MgsSplatSet* out)
{
  if(!v || !out || !v->positions || !v->f_dc || !v->opacity || !v->scale || !v->rotation)
  {
    setError("mgs_splatset_from_arrays: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(v->splat_count == 0 || v->splat_count > 0xFFFFFFFFull)
  {
    setError("mgs_splatset_from_arrays: splat_count must be in [1, 2^32)");
    return MGS_ERR_INVALID_ARG;
  }
  if(v->f_rest_per_splat != 0 && v->f_rest == nullptr)
  {
    setError("mgs_splatset_from_arrays: f_rest is null but f_rest_per_splat != 0");
    return MGS_ERR_INVALID_ARG;
  }
  if(v->f_rest_per_splat % 3 != 0 || v->f_rest_per_splat > 45)
  {
    setError("mgs_splatset_from_arrays: f_rest_per_splat must be a multiple of 3, at most 45");
    return MGS_ERR_INVALID_ARG;
  }
  const size_t n   = (size_t)v->splat_count;
  auto         set = std::make_shared<HostSplatSet>();
  set->positions.assign(v->positions, v->positions + 3 * n);
  set->f_dc.assign(v->f_dc, v->f_dc + 3 * n);
  if(v->f_rest_per_splat)
    set->f_rest.assign(v->f_rest, v->f_rest + (size_t)v->f_rest_per_splat * n);
  set->opacity.assign(v->opacity, v->opacity + n);
  set->scale.assign(v->scale, v->scale + 3 * n);
  set->rotation.assign(v->rotation, v->rotation + 4 * n);
  *out = new MgsSplatSet_t{set};
  return MGS_OK;
}
int mgs_splatset_from_arrays(const MgsSplatSetView* v, MgsSplatSet* out)
{
  return guarded("mgs_splatset_from_arrays", [&] { return mgs_splatset_from_arrays_impl(v, out); });
}

int mgs_splatset_view(MgsSplatSet set, MgsSplatSetView* out)
{
  if(!set || !out)
  {
    setError("mgs_splatset_view: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  const HostSplatSet& s = *set->data;
  out->positions        = s.positions.data();
  out->f_dc             = s.f_dc.data();
  out->f_rest           = s.f_rest.empty() ? nullptr : s.f_rest.data();
  out->opacity          = s.opacity.data();
  out->scale            = s.scale.data();
  out->rotation         = s.rotation.data();
  out->splat_count      = s.size();
  out->f_rest_per_splat = s.fRestPerSplat();
  out->sh_degree        = s.maxShDegree();
  return MGS_OK;
}

void mgs_splatset_destroy(MgsSplatSet set) { delete set; }

// ---- asynchronous loader + request queue (PlyLoaderAsync + sceneLoadQueue) -----------------------------------------
struct MgsLoader_t
{
  std::thread             worker;
  std::mutex              mtx;
  std::condition_variable cv;
  std::deque<std::string> queue;     // waiting requests; front() is the head while LOADING / LOADED / FAILURE
  int                     state = MGS_LOADER_READY;
  bool                    shutdown = false;
  MgsSplatSet             result = nullptr;
  int                     resultCode = MGS_OK;
  std::string             resultError;

  void run()
  {
    std::unique_lock<std::mutex> lk(mtx);
    for(;;)
    {
      cv.wait(lk, [&] { return shutdown || (state == MGS_LOADER_READY && !queue.empty()); });
      if(shutdown)
        return;
      state                  = MGS_LOADER_LOADING;
      const std::string path = queue.front();
      lk.unlock();
      MgsSplatSet set = nullptr;
      const int   rc  = mgs_splatset_load(path.c_str(), &set);  // the synchronous loader (thread-local error string)
      const std::string err = rc == MGS_OK ? std::string() : std::string(mgs_last_error());
      lk.lock();
      result      = set;
      resultCode  = rc;
      resultError = err;
      state       = rc == MGS_OK ? MGS_LOADER_LOADED : MGS_LOADER_FAILURE;
      cv.notify_all();
    }
  }
};

int mgs_loader_create(MgsLoader* out)
{
  if(!out)
  {
    setError("mgs_loader_create: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  return guarded("mgs_loader_create", [&] {
    auto* L   = new MgsLoader_t();
    L->worker = std::thread([L] { L->run(); });
    *out      = L;
    return (int)MGS_OK;
  });
}

void mgs_loader_destroy(MgsLoader L)
{
  if(!L)
    return;
  {
    std::lock_guard<std::mutex> lk(L->mtx);
    L->shutdown = true;
  }
  L->cv.notify_all();
  L->worker.join();
  if(L->result)
    mgs_splatset_destroy(L->result);
  delete L;
}

int mgs_loader_push(MgsLoader L, const char* path)
{
  if(!L || !path)
  {
    setError("mgs_loader_push: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  return guarded("mgs_loader_push", [&] {
    {
      std::lock_guard<std::mutex> lk(L->mtx);
      L->queue.emplace_back(path);
    }
    L->cv.notify_all();
    return (int)MGS_OK;
  });
}

int mgs_loader_status(MgsLoader L, int* state, uint32_t* queued, char* pathOut, size_t cap)
{
  if(!L || !state)
  {
    setError("mgs_loader_status: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lk(L->mtx);
  // a request that has been queued but not picked up yet already counts as LOADING for the poller
  const bool busy = !L->queue.empty();
  *state          = (L->state == MGS_LOADER_READY && busy) ? MGS_LOADER_LOADING : L->state;
  if(queued)
    *queued = busy ? (uint32_t)L->queue.size() - 1u : 0u;
  if(pathOut && cap)
  {
    const std::string& p = busy ? L->queue.front() : std::string();
    std::snprintf(pathOut, cap, "%s", busy ? p.c_str() : "");
  }
  return MGS_OK;
}

int mgs_loader_take(MgsLoader L, MgsSplatSet* out)
{
  if(!L || !out)
  {
    setError("mgs_loader_take: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  int rc;
  {
    std::lock_guard<std::mutex> lk(L->mtx);
    if(L->state != MGS_LOADER_LOADED && L->state != MGS_LOADER_FAILURE)
    {
      setError("mgs_loader_take: nothing loaded (poll mgs_loader_status)");
      return MGS_ERR_STATE;
    }
    rc = L->resultCode;
    if(L->state == MGS_LOADER_LOADED)
      *out = L->result;
    else
      setError(L->resultError);
    L->result = nullptr;
    L->queue.pop_front();
    L->state = MGS_LOADER_READY;  // reset(): the next queued file may start
  }
  L->cv.notify_all();
  return rc;
}
