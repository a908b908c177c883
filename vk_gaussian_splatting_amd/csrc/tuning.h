// tuning.h — the library's environment switches (README: "Environment knobs"), read once per process by tuning().
// Every getenv of libmgs.so is in tuning.hip, except the trace-file paths of the instrumentation builds (-DMGS_*_TRACE).
#pragma once
#include <cstdint>
#include <optional>
#include <string>

namespace mgs {

struct Tuning
{
  // binning
  bool directBin       = true;   // MGS_DIRECT_BIN=0: the record + pair-sort path even for frames of <= 256 bins
  bool rectRide        = true;   // MGS_RECT_RIDE=0: k_dbin_count gathers every bin rectangle by id instead of reading the ridden codes
  bool rideSplitAlways = false;  // MGS_RIDE_SPLIT=2: the codes are always split between the key's low byte and the id's spare bits
  int  dbTranspose     = 1;      // MGS_DB_TRANSPOSE=0: the binning's column / row masks by ballots instead of the transpose
  bool binAdapt        = true;   // MGS_BIN_ADAPT=0 (or any MGS_BIN_SHIFT): no adaptive bin size (BinPolicy)
  bool binShiftSet     = false;  // MGS_BIN_SHIFT="x,y": the bin shifts of every frame (buildFrameArgs clamps them) ...
  std::optional<int> binShiftX, binShiftY;  // ... as far as sscanf("%d,%d") read them; an axis it did not read keeps its default
  std::optional<uint64_t> pairCapacity;     // MGS_PAIR_CAPACITY=n: entries of the per-bin lists / record buffers (strtoull)
  // project kernels
  bool exactShortcuts  = true;   // MGS_EXACT_SHORTCUTS=0: always the full unfused products of P*V*M
  // sorts
  bool     sortRemap       = true;   // MGS_SORT_REMAP=0: the key sort keeps its four plain passes (no pass elision)
  bool     rawSortGeneric  = false;  // MGS_RAW_SORT=generic: mgs_radix_sort_u32 on the generic sort for every bit range
  uint32_t osFlat          = 1;      // MGS_OS_FLAT: the key sort's flat level-2 look-back where it applies (raw atoi; != 0 = on)
  uint32_t osPartMin       = 1536;   // MGS_OS_PART_MIN: smallest partition size the key sort may choose on the device
                                     // (a multiple of 256 in [1024, kOsPart]; kOsPart = fixed partitions)
  // mesh pass
  uint32_t meshWorkItems = 1u << 20;  // MGS_MESH_WORK_ITEMS=n: capacity of the large-triangle work list, 1 .. 2^26 chunks of 16 tiles
  // traced light pass
  bool softShadows = false;  // MGS_SOFT_SHADOWS=1: mgs_render_traced_lit and mgs_render_hybrid accept MGS_SHADOWS_SOFT; unset, they
                             // answer it with MGS_ERR_UNSUPPORTED as every build before did (ABI 5.1: same behaviour by default).
                             // TEMPORARY: goes with the next ABI minor, which accepts the mode unconditionally
  // frame submission
  bool useGraph = true;  // MGS_GRAPH=0: plain kernel launches instead of replaying the captured frame graph
  // multi-GPU
  std::optional<std::string> rcclLib;  // MGS_RCCL_LIB=path: resolve the RCCL entry points from this library only (tests)
};

const Tuning& tuning();

}  // namespace mgs
