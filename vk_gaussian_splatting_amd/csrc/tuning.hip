// tuning.hip — reads the environment switches of tuning.h, once per process (host code only).
#include "tuning.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sort_plan.h"

namespace mgs {

static Tuning readTuning()
{
  Tuning t;
  auto flag = [](const char* name, bool dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) != 0 : dflt;
  };
  t.directBin      = flag("MGS_DIRECT_BIN", true);
  t.rectRide       = flag("MGS_RECT_RIDE", true);
  t.exactShortcuts = flag("MGS_EXACT_SHORTCUTS", true);
  t.sortRemap      = flag("MGS_SORT_REMAP", true);
  t.useGraph       = flag("MGS_GRAPH", true);
  t.softShadows    = flag("MGS_SOFT_SHADOWS", false);
  if(const char* e = std::getenv("MGS_RIDE_SPLIT"))
    t.rideSplitAlways = std::atoi(e) == 2;
  if(const char* e = std::getenv("MGS_DB_TRANSPOSE"))
    t.dbTranspose = std::atoi(e);
  if(const char* e = std::getenv("MGS_BIN_SHIFT"))
  {
    int       x = 0, y = 0;
    const int got = std::sscanf(e, "%d,%d", &x, &y);
    t.binShiftSet = true;
    if(got >= 1)
      t.binShiftX = x;
    if(got >= 2)
      t.binShiftY = y;
  }
  t.binAdapt = flag("MGS_BIN_ADAPT", true) && !t.binShiftSet;
  if(const char* e = std::getenv("MGS_PAIR_CAPACITY"))
    t.pairCapacity = std::strtoull(e, nullptr, 10);
  if(const char* e = std::getenv("MGS_RAW_SORT"))
    t.rawSortGeneric = std::strcmp(e, "generic") == 0;
  if(const char* e = std::getenv("MGS_OS_FLAT"))
    t.osFlat = (uint32_t)std::atoi(e);
  if(const char* e = std::getenv("MGS_OS_PART_MIN"))
  {
    const int x = std::atoi(e);
    if(x >= 1024 && x <= (int)kOsPart && x % 256 == 0)
      t.osPartMin = (uint32_t)x;
  }
  if(const char* e = std::getenv("MGS_MESH_WORK_ITEMS"))
  {
    const long long x = std::atoll(e);
    if(x >= 1 && x <= (1ll << 26))
      t.meshWorkItems = (uint32_t)x;
  }
  if(const char* e = std::getenv("MGS_RCCL_LIB"))
    t.rcclLib = e;
  return t;
}

const Tuning& tuning()
{
  static const Tuning t = readTuning();
  return t;
}

}  // namespace mgs
