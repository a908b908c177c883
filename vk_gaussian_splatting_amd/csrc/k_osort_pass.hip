// k_osort_pass.hip — one pass of the key sort in one kernel (osort_common.h has the sort's outline and OsPassArgs).
//
// Look-back: the classic chain resolves partition p from p-1, one dependent cross-CU load per hop; with all ~1 000 partitions
// of a frame's sort resident at once that serialises (measured 1.27 us per hop, tools/micro/lookback_rate.hip).  Here the prefix
// is resolved in TWO LEVELS of fan-in 32, every level one batch of independent loads:
//   1. member m of a group sums the published counts of the m members before it (<= 31 loads in flight per thread);
//   2. the group's last member publishes the group total, resolves the group's base with a windowed look-back over the
//      GROUP totals (16 per batch, stopping at the first inclusive prefix) and publishes the inclusive group prefix;
//   3. every member reads ONE word: the inclusive prefix of the previous group.
// Three round trips whatever the partition count, overlapped with the ranking.  Sorts of at most 32 groups replace 2 and 3 by
// the flat level 2 (in the kernel, below).  Status words carry flag and value in one 32-bit word written by one relaxed
// agent-scope store (sc1: the data is the flag, no fence to order), polled with relaxed agent-scope loads.  The level-1 loads
// are issued right after a partition has published its own counts and consumed behind its ranking, the group level behind its
// LDS re-order: the round trips overlap the pass's own work.
// Partition = blockIdx.x.  A workgroup waits only for lower-numbered ones, and the dispatcher starts the workgroups of a 1-D
// grid in index order on every XCD, so whatever is waited for is running or done.  (A ticket per workgroup would not have to
// lean on that, and costs ~10 us per pass: docs/DESIGN_history_keysort.md.)  Every spin is bounded: if the order were ever
// violated, the wait gives up and raises kErrSpinTimeout (the frame is wrong, the GPU does not hang).
//
// Pairs travel interleaved (uint2): one 8-byte access per element, digit runs of 16 elements are 128 contiguous bytes; the
// last pass writes the ids alone (the keys are dead; the sort-only hook asks for them explicitly).
#include "osort_common.h"

namespace mgs {

// The count table of key >> 16 -> what the upper passes sort on.  At most 256 occurring values within a span < 4096: the second
// kernel sorts on their RANK (plan->remapVals, totals per rank) and is final; otherwise plain digits for passes 2 and 3 (totals of
// bits 16-23 and 24-31).  Clears what it read: the table is clean for the next sort of this context.  The table is complete (the
// kernel that filled it has ended).
// kOsFoldWgs workgroups take part: the narrow case (the rule) is workgroup 0's alone; a wide range — up to 64 K values — is split
// between all of them (one 256-thread workgroup walking it alone holds the first sort kernel up for 50 us).
template <int THREADS>
__device__ __forceinline__ void foldTop16(OsPlan* __restrict__ plan, uint32_t* __restrict__ top16Count, int allowRemap, uint32_t wg,
                                          uint32_t* s_part /*512*/, uint32_t* s_sum /*THREADS / 64*/)
{
  constexpr uint32_t kPer = kRemapSpan / THREADS;  // consecutive values per thread (ordered compaction)
  const int          t = threadIdx.x, lane = laneId(), w = t >> 6;
  const uint32_t     minInv = plan->top16MinInv, maxP1 = plan->top16MaxP1;
  if(minInv == 0u || maxP1 == 0u)
  {  // no real keys at all
    if(t == 0 && wg == 0u)
      plan->remapOn = plan->remapCount = plan->remapBase = 0u;
    return;
  }
  const uint32_t vlo = 0x10000u - minInv, span = maxP1 - vlo;  // values vlo .. vlo + span - 1
  for(int i = t; i < 512; i += THREADS)
    s_part[i] = 0u;
  if(span <= kRemapSpan - 1u)
  {
    if(wg != 0u)
      return;
    uint32_t c[kPer], nz = 0;
#pragma unroll
    for(uint32_t i = 0; i < kPer; ++i)
    {
      const uint32_t k = (uint32_t)t * kPer + i;
      c[i]             = k < span ? top16Count[vlo + k] : 0u;
      nz += c[i] ? 1u : 0u;
    }
#pragma unroll
    for(uint32_t i = 0; i < kPer; ++i)
      if(c[i])
        top16Count[vlo + (uint32_t)t * kPer + i] = 0u;  // consumed
    const uint32_t inc = waveInclusiveScan(nz);
    if(lane == 63)
      s_sum[w] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for(int q = 0; q < THREADS / 64; ++q)
    {
      if(q < w) base += s_sum[q];
      total += s_sum[q];
    }
    const bool on = allowRemap != 0 && total >= 1u && total <= 256u;
    uint32_t   run = base + inc - nz;
#pragma unroll
    for(uint32_t i = 0; i < kPer; ++i)
      if(c[i])
      {
        const uint32_t v = vlo + (uint32_t)t * kPer + i;
        if(on)
        {
          plan->remapVals[run] = (uint16_t)v;
          plan->total[2][run]  = c[i];  // pass 2 sorts on the rank
          ++run;
        }
        else
        {
          atomicAdd(&s_part[v & 255u], c[i]);
          atomicAdd(&s_part[256u + (v >> 8)], c[i]);
        }
      }
    __syncthreads();
    if(!on)
      for(int i = t; i < 256; i += THREADS)
      {
        plan->total[2][i] = s_part[i];
        plan->total[3][i] = s_part[256 + i];
      }
    if(t == 0)
    {
      plan->remapOn      = on ? 1u : 0u;
      plan->remapCount   = on ? total : 0u;
      plan->remapBase    = on ? vlo : 0u;
      plan->remapPadRank = on ? total - 1u : 0u;  // keys outside the table (padding) take the largest rank
    }
    return;
  }
  // wide range (camera inside the cloud): plain digits of bits 16-23 and 24-31; this workgroup's share of the range, eight loads
  // in flight per thread, the totals added to the plan's (zero when the frame starts)
  __syncthreads();
  const uint32_t share = (span + kOsFoldWgs - 1u) / kOsFoldWgs, k0 = wg * share, k1 = min(span, k0 + share);
  for(uint32_t kb = k0; kb < k1; kb += 8u * THREADS)
  {
    uint32_t c[8];
#pragma unroll
    for(int i = 0; i < 8; ++i)
    {
      const uint32_t k = kb + (uint32_t)i * THREADS + (uint32_t)t;
      c[i]             = k < k1 ? top16Count[vlo + k] : 0u;
    }
#pragma unroll
    for(int i = 0; i < 8; ++i)
      if(c[i])
      {
        const uint32_t v = vlo + kb + (uint32_t)i * THREADS + (uint32_t)t;
        top16Count[v]    = 0u;
        atomicAdd(&s_part[v & 255u], c[i]);
        atomicAdd(&s_part[256u + (v >> 8)], c[i]);
      }
  }
  __syncthreads();
  for(int i = t; i < 256; i += THREADS)
  {
    if(s_part[i])
      atomicAdd(&plan->total[2][i], s_part[i]);
    if(s_part[256 + i])
      atomicAdd(&plan->total[3][i], s_part[256 + i]);
  }
  if(t == 0 && wg == 0u)
    plan->remapOn = plan->remapCount = plan->remapBase = 0u;
}

// ---------------------------------------------------------------------------------------------------------------------
template <int IN, bool REMAP>
__global__ __launch_bounds__(kThreads, MGS_OS_WAVES) void k_os_pass(const OsPassArgs a)
{
  __shared__ uint2    s_pair[kOsPart];       // 32 KB: the partition's pairs ordered by digit
  __shared__ uint16_t s_whist[kWaves][256];  //  2 KB: per wave digit counts -> offsets
  __shared__ uint16_t s_loff[256];           //  partition-local exclusive digit offsets
  __shared__ uint32_t s_cnt[256];            //  digit counts of the partition, later the global base of every digit
  __shared__ uint8_t  s_rv[REMAP ? kRemapSpan : 4];  // 4 KB: rank table of key >> 16 (remapped pass)
  __shared__ uint32_t s_tmp[8];

  const int t = threadIdx.x, lane = laneId(), w = t >> 6;
  OsPlan*   plan = a.plan;
  const bool remapped = plan->remapOn != 0u;
  if(a.digitMode == 2 && remapped)
    return;  // pass 2 sorted on the rank of the top 16 bits and wrote the result
#ifdef MGS_OS_TRACE
  __shared__ uint64_t trc[8];
  __shared__ uint64_t gtr[8];
  if(threadIdx.x < 8) gtr[threadIdx.x] = 0;
  MGS_OS_STAMP(0)
#endif
  const uint32_t p = blockIdx.x;  // partitions in dispatch order (header: why no ticket)
  const uint32_t n = *a.nPtr;
  [[maybe_unused]] uint4 tot0q = make_uint4(0u, 0u, 0u, 0u);
  if constexpr(IN == 3)  // the virtual pass 0 starts from the digit-0 totals (lane l: values 4 l .. 4 l + 3): their round trip passes behind the set-up
    tot0q = *reinterpret_cast<const uint4*>(&plan->total[0][4 * lane]);
  // clear look-back words for a later pass (stream order: nobody reads them any more)
  for(uint32_t i = blockIdx.x * kThreads + t; i < a.zWords; i += gridDim.x * kThreads)
    a.zStatus[i] = 0u;
  if constexpr(IN == 3)
    if(blockIdx.x >= gridDim.x - kOsFoldWgs)
    {  // workgroups beyond the partitions: what the SECOND kernel sorts on (foldTop16), beside this kernel's own work
      foldTop16<kThreads>(plan, a.top16Count, a.allowRemap, blockIdx.x - (gridDim.x - kOsFoldWgs), reinterpret_cast<uint32_t*>(s_pair), s_tmp);
      return;
    }
  const uint32_t part  = osPartOf(n, gridDim.x - (IN == 3 ? kOsFoldWgs : 0u), a.partMin, a.resSlots);  // wave-uniform, the same in every workgroup
  const uint32_t parts = (uint32_t)(((uint64_t)n + part - 1u) / part);
  if(p >= parts)
    return;
  const bool finalOut = a.finalMode == 1 || (a.finalMode == 2 && remapped);
  if(p == 0 && t == 0 && a.planOut != nullptr && (finalOut || a.digitMode == 2))
  {
    a.planOut->n         = plan->n;
    a.planOut->finalSel  = 0u;
    a.planOut->passesRun = (uint32_t)a.pass + 1u;
    if(finalOut)
      a.planOut->rideInfo = a.rideShift != 0u ? a.rideInfo : 0u;  // the binning stage finds the rectangles in sorted order
  }

  // ---- load: wave w owns a contiguous quarter of the partition, lane-interleaved, so (wave, round, lane) is memory order.
  // The rounds adapt to the element count (the last partition is ragged).
  const uint32_t count = (uint32_t)min((uint64_t)part, (uint64_t)n - (uint64_t)p * part);
  const uint32_t rounds = (count + kThreads - 1u) / kThreads;  // per wave: `rounds` rounds of 64 keys
  const uint32_t wofs   = w * 64u * rounds;
  uint32_t       key[kKpt], val[kKpt];
  MGS_OS_STAMP(1)
  [[maybe_unused]] uint32_t srcAt[IN == 3 ? kKpt : 1];
  auto loadPairs = [&]() {
    // clamped, not predicated: a predicated load becomes a branch + wait and serialises the fetches
#pragma unroll
    for(int i = 0; i < kKpt; ++i)
    {
      key[i] = 0xFFFFFFFFu;
      val[i] = 0u;
      if((uint32_t)i < rounds)  // wave-uniform
      {
        const uint32_t idx = min(wofs + (uint32_t)i * 64u + lane, count - 1u);
        if(IN == 2)
        {
          key[i] = a.srcKeys[(size_t)p * part + idx];
          val[i] = a.srcVals[(size_t)p * part + idx];
        }
        else
        {
          const uint2 kv = IN == 3 ? a.srcPairs[srcAt[IN == 3 ? i : 0]] : a.srcPairs[(size_t)p * part + idx];
          key[i] = kv.x;
          val[i] = kv.y;
        }
      }
    }
#pragma unroll
    for(int i = 0; i < kKpt; ++i)
      if(wofs + (uint32_t)i * 64u + lane >= count)
      {
        key[i] = 0xFFFFFFFFu;
        val[i] = 0u;
      }
  };
  // a pass over contiguous input requests its pairs BEFORE it sets up its LDS (the zeroed wave histograms, the rank table and
  // their two barriers: 1.9 us of the workgroup's life that the loads' round trip passes behind); the first pass of a frame
  // cannot — its source table is built in LDS first
  if constexpr(IN != 3)
    loadPairs();
  for(int i = t; i < kWaves * 256; i += kThreads)
    (&s_whist[0][0])[i] = 0;
  const bool useRemap = REMAP && remapped;
  if constexpr(REMAP)
    if(useRemap)
    {  // every entry holds the largest rank first: a value outside the table (padding keys) sorts behind every real key
      const uint32_t count = plan->remapCount, base = plan->remapBase;
      const uint32_t fill  = plan->remapPadRank * 0x01010101u;
      for(int i = t; i < (int)kRemapSpan / 4; i += kThreads)
        reinterpret_cast<uint32_t*>(s_rv)[i] = fill;
      __syncthreads();
      for(uint32_t i = t; i < count; i += kThreads)
        s_rv[(uint32_t)plan->remapVals[i] - base] = (uint8_t)i;
    }
  __syncthreads();
  // IN 3: the source table of the virtual pass 0 (header of OsPassArgs).  s_pair is not in use before the re-order: its first
  // half holds the table.  Everything that locates the runs — the digit bases D, the prefix over the chunks — is computed by
  // EVERY WAVE FOR ITSELF (identical results, a few dozen loads each): the construction has no workgroup barrier except the
  // one before the table is read (with block-wide scans it had nine, 8 us per digit value; profiles/r4_c_os_trace.log).
  if constexpr(IN == 3)
  {
    uint32_t* s_src = reinterpret_cast<uint32_t*>(s_pair);       // [4096] pair index (slot * 2048 + entry) of every position of the partition
    uint32_t* s_cpw = s_src + kOsPart + (uint32_t)w * 264u;      // [257] this wave's prefix of chunkSum[.][d] over a tile of chunks
    constexpr uint32_t kCpTile = 256;                            // chunks per tile: four per lane
    const uint32_t a0 = p * part, e0 = a0 + count;
    // D: lane l holds digit-0 values 4 l .. 4 l + 3
    const uint32_t tk[4] = {tot0q.x, tot0q.y, tot0q.z, tot0q.w};
    uint32_t       d     = 256u;
    {
      const uint32_t s4 = tk[0] + tk[1] + tk[2] + tk[3];
      uint32_t       dq = waveInclusiveScan(s4) - s4;
#pragma unroll
      for(int k = 0; k < 4; ++k)
      {
        s_cnt[4 * lane + k] = dq;  // (s_cnt is free until the scatter; the four waves write the same values)
        const uint64_t bk   = __ballot(tk[k] != 0u && dq <= a0 && a0 < dq + tk[k]);
        if(bk != 0ull)
          d = 4u * (uint32_t)__builtin_ctzll(bk) + (uint32_t)k;  // the value the partition starts in
        dq += tk[k];
      }
    }
    __builtin_amdgcn_wave_barrier();
    MGS_OS_GSTAMP(0)
    auto loadCs = [&](uint32_t dd, uint32_t c0, uint32_t cs[4]) {
#pragma unroll
      for(int k = 0; k < 4; ++k)
      {
        const uint32_t c = c0 + 4u * (uint32_t)lane + (uint32_t)k;
        cs[k]            = (dd < 256u && c < a.chunks) ? a.chunkSum[(size_t)c * 256u + dd] : 0u;
      }
    };
    const uint32_t spad = a.chunks * kOsChunk;
    uint32_t       csN[4];
    loadCs(d, 0u, csN);
    while(d < 256u)
    {  // uniform (every wave computes the same): the digit-0 values whose range [Dd, De) overlaps [a0, e0)
      const uint32_t Dd = s_cnt[d], De = d < 255u ? s_cnt[d + 1u] : n;
      if(Dd >= e0)
        break;
      uint32_t cs[4] = {csN[0], csN[1], csN[2], csN[3]};
      loadCs(De < e0 ? d + 1u : 256u, 0u, csN);  // the next value's first tile travels behind this one's expansion
      if(De > a0 && De != Dd)
      {
        uint32_t carry = Dd;  // position of the first pair of value d in the tile's first chunk
        for(uint32_t c0 = 0;;)
        {
          const uint32_t sum = cs[0] + cs[1] + cs[2] + cs[3];
          const uint32_t inc = waveInclusiveScan(sum);
          MGS_OS_GSTAMP(1)  // chunk sums arrived
          const uint32_t tileTotal = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
          uint32_t       run = inc - sum, cA = kCpTile, cB = 0u;  // chunks [cA, cB) of the tile hold pairs inside [a0, e0)
#pragma unroll
          for(int k = 0; k < 4; ++k)
          {
            s_cpw[4 * lane + k] = run;
            const uint32_t lo   = carry + run, hi = lo + cs[k];
            const uint64_t bk   = __ballot(cs[k] != 0u && lo < e0 && hi > a0);
            if(bk != 0ull)
            {
              cA = min(cA, 4u * (uint32_t)__builtin_ctzll(bk) + (uint32_t)k);
              cB = max(cB, 4u * (63u - (uint32_t)__builtin_clzll(bk)) + (uint32_t)k + 1u);
            }
            run += cs[k];
          }
          if(lane == 63)
            s_cpw[kCpTile] = run;
          __builtin_amdgcn_wave_barrier();
          MGS_OS_GSTAMP(2)  // chunk range known
          if(cB != 0u)
          {
            const uint32_t  entries = (cB - cA) * kOsChunk;
            const uint32_t* row     = a.runTab + (size_t)d * spad + (size_t)(c0 + cA) * kOsChunk;
            // lane == run: 32 consecutive lanes hold a chunk's 32 slots; the workgroup's 256 threads share the runs.  Four loads in
            // flight per thread (the usual partition overlaps ~700 runs: one batch).
            auto expand = [&](uint32_t i, uint32_t ic, uint32_t v) {
              const uint32_t cl  = cA + ic / kOsChunk;  // chunk within the tile
              const uint32_t inC = v & 0xFFFFu;
              const uint32_t nxt = (uint32_t)__shfl_down((int)inC, 1, 64);
              const uint32_t len = ((ic & (kOsChunk - 1u)) == kOsChunk - 1u ? s_cpw[cl + 1u] - s_cpw[cl] : nxt) - inC;
              const uint32_t R   = carry + s_cpw[cl] + inC;  // position of the run's first pair
              uint32_t       lo  = max(R, a0), hi = min(R + len, e0);
              if(i >= entries || hi <= lo)
                lo = hi = 0u;
              const uint32_t src = ((c0 + cl) * kOsChunk + (ic & (kOsChunk - 1u))) * kOsSlot + (v >> 16);  // the run's first pair
              // short runs (the rule: ~6 pairs) are written by their lane; long ones by the wave together
              const bool     big = hi - lo > 16u;
              if(!big)
                for(uint32_t x = lo; x < hi; ++x)
                  s_src[x - a0] = src + (x - R);
              uint64_t bm = __ballot(big);
              while(bm != 0ull)
              {
                const int      l   = (int)__builtin_ctzll(bm);
                bm &= bm - 1ull;
                const uint32_t loL = (uint32_t)__builtin_amdgcn_readlane((int)lo, l), hiL = (uint32_t)__builtin_amdgcn_readlane((int)hi, l);
                const uint32_t dl  = (uint32_t)__builtin_amdgcn_readlane((int)(src - R), l);
                for(uint32_t x = loL + (uint32_t)lane; x < hiL; x += 64u)
                  s_src[x - a0] = dl + x;
              }
            };
            for(uint32_t i0 = 0; i0 < entries; i0 += 4u * kThreads)
            {
              uint32_t vv[4];
#pragma unroll
              for(int k = 0; k < 4; ++k)
                vv[k] = row[min(i0 + (uint32_t)k * kThreads + (uint32_t)t, entries - 1u)];
#ifdef MGS_OS_TRACE
              if(vv[0] + vv[1] + vv[2] + vv[3] == 0x12345678u) gtr[7] = 1;  // consume the loads: the stamp follows their arrival
              MGS_OS_GSTAMP(3)
#endif
#pragma unroll
              for(int k = 0; k < 4; ++k)
              {
                const uint32_t i = i0 + (uint32_t)k * kThreads + (uint32_t)t;
                if(i0 + (uint32_t)k * kThreads + (uint32_t)(t & ~63) < entries)  // wave-uniform
                  expand(i, min(i, entries - 1u), vv[k]);
              }
            }
          }
          carry += tileTotal;
          c0 += kCpTile;
          if(c0 >= a.chunks || carry >= e0)
            break;
          __builtin_amdgcn_wave_barrier();  // the wave's prefix table is rewritten
          loadCs(d, c0, cs);
        }
        MGS_OS_GSTAMP(4)  // first digit value expanded
      }
      ++d;
    }
    __syncthreads();
    MGS_OS_STAMP(1)  // (trace build: the table's construction counts as "table + zeroing", the gather itself as "loads")
#pragma unroll
    for(int i = 0; i < kKpt; ++i)
      srcAt[i] = min(s_src[min(wofs + (uint32_t)i * 64u + lane, count - 1u)], a.srcLimit);
  }
  if constexpr(IN == 3)
    loadPairs();
  const int      shift = 8 * a.pass;
  const uint32_t rbase = plan->remapBase;
  uint32_t       rd[kKpt];  // digit << 16 | rank inside the wave (one register per key)
#pragma unroll
  for(int i = 0; i < kKpt; ++i)
  {
    uint32_t d;
    if(REMAP && useRemap)
      d = s_rv[min((key[i] >> 16) - rbase, kRemapSpan - 1u)];
    else
      d = (key[i] >> shift) & 255u;
    rd[i] = d << 16;
  }
  const uint32_t g = p / kOsGroup, m = p % kOsGroup;
  // bits that tell the digits of this pass apart: 8, or — sorting on the rank of key >> 16 — as many as the largest rank has
  [[maybe_unused]] const int rankBits = (REMAP && useRemap) ? 32 - __builtin_clz(plan->remapPadRank | 1u) : 8;
  MGS_OS_STAMP(2)
  // Flat level 2 (sorts of at most 32 groups = 1 024 partitions: a frame's).  The chain — a group's last member folds its rows,
  // publishes the group total, looks back over the group totals, publishes the inclusive prefix; every other member polls that
  // word — is three dependent round trips that START when the last member has ranked its keys, the moment everybody else starts
  // waiting: the partitions of a pass run in step.  Instead every partition ADDS its counts to its group's row — one
  // fire-and-forget atomic per digit; the word carries the sum (< 2^20: 32 x 4096) and, above it, how many partitions have added
  // — and reads the rows of ALL groups before its own (<= 31 words per digit thread, requested behind the level-1 fold, consumed
  // behind the LDS re-order); a row counts once 32 partitions have arrived.  No last member, no dependent trips.
  const uint32_t groupsAll = (parts + kOsGroup - 1u) / kOsGroup;
  const bool     flat      = a.flatLookback != 0u && groupsAll <= 32u;

  // ---- (the look-back is software-pipelined with the rest of the pass: level 1 is issued right after the partition's own
  // counts are published, behind the ranking, and consumed behind the scans; level 2 travels behind the LDS re-order) ----

  // ---- per-wave multi-split: rank of each key among the keys of its wave with the same digit (stable) ----
#pragma unroll
  for(int i = 0; i < kKpt; ++i)
  {
    if((uint32_t)i < rounds)  // wave-uniform: skipped rounds hold nothing
    {
      // padding lanes (idx >= count) carry key 0xFFFFFFFF: the largest digit, behind every real key of the partition
      // lanes holding the same digit: per bit, x = 0 / ~0 from the bit (one bfe), the ballot of the bit, and
      // mask &= ~(ballot ^ x) on both halves — 6 vector instructions per bit
      const uint32_t d = rd[i] >> 16;
      uint32_t       mlo = ~0u, mhi = ~0u;
#pragma unroll
      for(int b = 0; b < 8; ++b)
      {
        if(REMAP && b >= rankBits)  // wave-uniform: the ranks of a remapped pass need ceil(log2(values)) bits — 3 for the usual 5-8
          break;
        uint32_t x = (uint32_t)((int32_t)(d << (31 - b)) >> 31);
        asm volatile("" : "+v"(x));  // the ballot compares x itself: left alone the compiler re-derives it from d (a shift per bit)
        const uint64_t bal = __ballot(x != 0u);
        // m & ~(bal ^ x) in one v_bitop3 per half (truth table 0x90: a & !(b ^ c))
        mlo = __builtin_amdgcn_bitop3_b32(mlo, (uint32_t)bal, x, 0x90);
        mhi = __builtin_amdgcn_bitop3_b32(mhi, (uint32_t)(bal >> 32), x, 0x90);
      }
      const uint32_t lower = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
      const uint32_t cnt   = (uint32_t)__popc(mlo) + (uint32_t)__popc(mhi);
      const uint32_t pre   = s_whist[w][d];
      rd[i] |= pre + lower;
      __builtin_amdgcn_wave_barrier();  // every lane of the group has read `pre` before the leader bumps it
      if(lower == 0)
        s_whist[w][d] = (uint16_t)(pre + cnt);
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  MGS_OS_STAMP(3)
  // thread t == digit t: the partition's count of digit t (the ranking counted the padding lanes too: they sit in the
  // largest digit) -> published; per wave offsets
  uint32_t tot = 0;
#pragma unroll
  for(int q = 0; q < kWaves; ++q)
  {
    const uint32_t c = s_whist[q][t];
    s_whist[q][t]    = (uint16_t)tot;
    tot += c;
  }
  const uint32_t padDigit = (REMAP && useRemap) ? plan->remapPadRank : 255u;
  const uint32_t myCount  = tot - (((uint32_t)t == padDigit) ? rounds * kThreads - count : 0u);
  stAgent(&a.status[(size_t)p * 256u + t], kAgg | myCount);
  if(flat)
    __hip_atomic_fetch_add(&a.gstatus[(size_t)g * 256u + t], myCount | (1u << 20), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // Level 1 by rows: the counts a member published are one 1 KB row (256 digits).  Wave w folds the rows w, w + 4, ... of the
  // members before me for four digits per lane (lane l: digits 4 l .. 4 l + 3);
  // the four waves' partial sums meet in LDS.  Issued now, consumed behind the scans.
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  const uint32_t wu = (uint32_t)__builtin_amdgcn_readfirstlane(w);  // the compiler does not know that the wave index is uniform
  // four dword sc1 loads per lane and row (a wave instruction covers 256 contiguous bytes).  One 16-byte
  // buffer_load_dwordx4 ... sc1 per lane was tried and does NOT work: re-polls kept returning the zeros of the first read
  // (every wait ran into its bound), while dword / dwordx2 sc1 loads of the same words see the update.
  auto loadRow = [&](uint32_t row) -> v4u {
    const uint32_t* q = a.status + ((size_t)g * kOsGroup + row) * 256u + (uint32_t)lane * 4u;
    return v4u{ldAgent(q), ldAgent(q + 1), ldAgent(q + 2), ldAgent(q + 3)};
  };
  v4u rv[8];
#pragma unroll
  for(int k = 0; k < 8; ++k)
  {
    const uint32_t row = wu + 4u * k;
    rv[k]              = v4u{kAgg, kAgg, kAgg, kAgg};
    if(row < m)
      rv[k] = loadRow(row);
  }
  uint32_t spins = 0, intra = 0, base = 0;
  bool     bad   = false;
  // level 1, consume: fold the rows (a member that had not published all four words when they were read is re-polled);
  // the four waves' partial sums meet in the first 4 KB of s_pair, which is not in use before the re-order
  auto foldRows = [&]() {
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for(int k = 0; k < 8; ++k)
    {
      const uint32_t row = wu + 4u * k;
      if(row < m)
      {
        while(((rv[k].x >> 30) == 0u || (rv[k].y >> 30) == 0u || (rv[k].z >> 30) == 0u || (rv[k].w >> 30) == 0u) && !bad)
        {
          rv[k] = loadRow(row);
          if(++spins > kSpinMax)
            bad = true;
        }
        acc[0] += rv[k].x & kValMask;
        acc[1] += rv[k].y & kValMask;
        acc[2] += rv[k].z & kValMask;
        acc[3] += rv[k].w & kValMask;
      }
    }
    reinterpret_cast<uint4*>(s_pair)[wu * 64 + lane] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    const uint32_t* s_l1 = reinterpret_cast<const uint32_t*>(s_pair);
    intra                = s_l1[t] + s_l1[256 + t] + s_l1[512 + t] + s_l1[768 + t];
  };
  // level 2.  The group's LAST member does the group's work at once, before its own scans: it folds its rows (the other
  // members published at the same moment), publishes the group total, looks back over the groups (16 per batch, down to the
  // first inclusive prefix) and publishes the inclusive prefix — so that the 31 other members, which fold behind their scans
  // and need that one word behind their LDS re-order, find it there.  It finishes ~3 us behind them instead of all of them
  // waiting ~5 us for it.
  const bool lastMember = !flat && m == kOsGroup - 1u;
  if(lastMember)
  {
    foldRows();
    const uint32_t gtotal = intra + myCount;
    stAgent(&a.gstatus[(size_t)g * 256u + t], kAgg | gtotal);
    int gq = (int)g - 1;
    while(gq >= 0 && !bad)
    {
      uint32_t gw[kGroupWindow];
#pragma unroll
      for(int j = 0; j < kGroupWindow; ++j)
        gw[j] = (gq - j >= 0) ? ldAgent(&a.gstatus[(size_t)(gq - j) * 256u + t]) : kInc;
      bool done = false;
#pragma unroll
      for(int j = 0; j < kGroupWindow; ++j)
      {
        if(done)
          continue;
        if((gw[j] >> 30) == 0u)
        {  // not published yet: resume the window at this group
          done = true;
          gq -= j;
          if(++spins > kSpinMax)
            bad = true;
          continue;
        }
        base += gw[j] & kValMask;
        if((gw[j] >> 30) == 2u)
        {
          done = true;
          gq   = -1;
        }
        else if(j == kGroupWindow - 1)
        {
          done = true;
          gq -= kGroupWindow;
        }
      }
    }
    stAgent(&a.gstatus[(size_t)g * 256u + t], kInc | ((base + gtotal) & kValMask));
  }
  // local exclusive scan over the digits (padding included)
  const uint32_t loff = scan256(tot, s_tmp);
  s_loff[t]           = (uint16_t)loff;
  // digit bases of the whole array: exclusive scan of the totals (known before the pass started)
  const uint32_t below = scan256(plan->total[a.pass][t], s_tmp);
  if(!lastMember)
    foldRows();
  // flat level 2: the counted sums of the groups before mine, thread t == digit t, all requested now (the registers of the
  // level-1 rows are free), consumed behind the re-order
  uint32_t gl[31];
  if(flat)
  {
#pragma unroll
    for(uint32_t k = 0; k < 31u; ++k)
    {
      gl[k] = 32u << 20;
      if(k < g)
        gl[k] = ldAgent(&a.gstatus[(size_t)k * 256u + t]);
    }
  }
  __syncthreads();  // everybody has read the partial sums: s_pair may be overwritten
  MGS_OS_STAMP(4)
  // ---- re-order through LDS so that equal digits are contiguous ----
#pragma unroll
  for(int i = 0; i < kKpt; ++i)
    if((uint32_t)i < rounds)
    {
      const uint32_t d   = rd[i] >> 16;
      const uint32_t pos = (uint32_t)s_loff[d] + (uint32_t)s_whist[w][d] + (rd[i] & 0xFFFFu);
      s_pair[pos]        = make_uint2(key[i], val[i]);
    }
  if(flat)
  {
#pragma unroll
    for(uint32_t k = 0; k < 31u; ++k)
      if(k < g)
      {
        while((gl[k] >> 20) != kOsGroup && !bad)
        {
          gl[k] = ldAgent(&a.gstatus[(size_t)k * 256u + t]);
          if(++spins > kSpinMax)
            bad = true;
        }
        base += gl[k] & 0xFFFFFu;
      }
  }
  else if(!lastMember && g > 0u)
  {  // the inclusive prefix of the previous group is one word
    uint32_t v;
    while(((v = ldAgent(&a.gstatus[(size_t)(g - 1u) * 256u + t])) >> 30) != 2u)
      if(++spins > kSpinMax)
      {
        bad = true;
        break;
      }
    base = v & kValMask;
  }
  if(bad)
    atomicOr(&a.ctr->errorFlags, kErrSpinTimeout);
  s_cnt[t] = below + (base + intra) - loff;  // wraps are fine: only base + idx is used
  __syncthreads();
  MGS_OS_STAMP(5)

  // ---- coalesced scatter: consecutive threads write consecutive addresses inside each digit run ----
#pragma unroll
  for(int i = 0; i < kKpt; ++i)
    if((uint32_t)i < rounds)
    {
      const uint32_t idx = (uint32_t)i * kThreads + t;
      if(idx < count)
      {
        const uint2 kv = s_pair[idx];
        uint32_t    d;
        if(REMAP && useRemap)
          d = s_rv[min((kv.x >> 16) - rbase, kRemapSpan - 1u)];
        else
          d = (kv.x >> shift) & 255u;
        const uint32_t dst = s_cnt[d] + idx;
        if(finalOut && a.rideShift != 0u)
        {
          a.dstVals[dst]   = kv.y & ((1u << a.rideShift) - 1u);
          a.dstCode16[dst] = a.rideSplit ? (uint16_t)((kv.x & 255u) | ((kv.y >> a.rideShift) << 8)) : (uint16_t)(kv.y >> a.rideShift);
        }
        else if(finalOut)
        {
          a.dstVals[dst] = kv.y;
          if(a.dstKeys != nullptr)
            a.dstKeys[dst] = kv.x;
        }
        else
          a.dstPairs[dst] = kv;
      }
    }
#ifdef MGS_OS_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  MGS_OS_STAMP(6)
  if(t == 0 && a.trace)
  {
    uint64_t* o = a.trace + (size_t)p * 8;
    for(int i = 0; i < 7; ++i) o[i] = trc[i];
    o[7] = ((uint64_t)count << 32) | spins;
    if(IN == 3)
    {  // the table's sub-stamps go where the (virtual) pass 0 would have put its own
      uint64_t* g = a.trace - (size_t)(gridDim.x - kOsFoldWgs) * 8 + (size_t)p * 8;  // (this kernel's grid has workgroups beyond the partitions)
      g[0] = trc[0];
      for(int i = 0; i < 5; ++i) g[1 + i] = gtr[i];
      g[6] = trc[1];
      g[7] = 0;
    }
  }
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
void launchOsPass(hipStream_t stream, OsVariant variant, uint32_t grid, const OsPassArgs& a)
{
  switch(variant)
  {
    case OsVariant::Split: hipLaunchKernelGGL((k_os_pass<2, false>), dim3(grid), dim3(kThreads), 0, stream, a); break;
    case OsVariant::Slots: hipLaunchKernelGGL((k_os_pass<3, false>), dim3(grid), dim3(kThreads), 0, stream, a); break;
    case OsVariant::Dense: hipLaunchKernelGGL((k_os_pass<0, false>), dim3(grid), dim3(kThreads), 0, stream, a); break;
    case OsVariant::DenseRank: hipLaunchKernelGGL((k_os_pass<0, true>), dim3(grid), dim3(kThreads), 0, stream, a); break;
  }
}

}  // namespace mgs
