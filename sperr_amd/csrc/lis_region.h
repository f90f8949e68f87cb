// lis_region.h -- what the two region kernels of the decoder's sorting pass (k_lis_hi: speck_dec.hip, regular trees;
// k_lis_mx: speck_mx.hip, every other chunk extent and every slice) agree on with each other and with the kernels and
// the host code around them.  The walks themselves -- tables, rows, queues, the state words a region publishes -- are
// the kernels' own.
//
// A phase's stream is cut into regions that a ticket counter (DecState::hiTicket) hands out in order to the workgroups
// of a chunk, at most kRegionGroups of them; a region takes the walker's state from the tagged words of the region
// before it (DecBuffers::hiFlags, tag = plane + 1 at kRegionTagShift) and publishes its own.  Who does what:
//
//   carve_dec (decode.hip)   sizes the chunk's birth and leaf-event arrays: SegArray::pitch() slots each, the segment
//                            size by region_seg_slots
//   dec_scan_chunk           before a plane: ticket, shared counters and the groups' counts back to zero
//   k_lis_hi / k_lis_mx      take tickets (region_ticket); wait for the predecessor (LookBackWait); claim slots of
//                            their group (SegGroup: region_claim_births, region_claim_leaf), record births (region_write_birth: the slot's two words and the bit of
//                            the level's position mask) and leaf events (leaf_event_pack, lis_token.h); at their end
//                            publish how much of their segment they filled (region_publish_counts)
//   k_lis_compact            its last workgroup clamps the shared counters (SegArray::shared_count)
//   k_place_scatter          enumerates the births, k_leaf_apply the leaf events: SegRanks, SegArray::slot_of_rank
//   launchers                never start more than kRegionGroups workgroups a chunk
//
// THE SEGMENTED ARRAY.  Births and leaf events of a plane are each one array per chunk: a shared part of `cap` slots
// claimed on a global counter (the block-parallel list kernels k_lis_l0 / _l1 / _l2 claim there too), then one segment
// of `seg` slots per workgroup of the chunk, claimed on a counter in LDS -- no returning global atomic on the hot
// path.  A claim that does not fit what is left of the segment goes to the shared part, whole, and the segment is full
// from that claim on: its counter stands past the segment's end, so no later claim is granted there either, and the
// group publishes the counter's value before the first refusal.  The shared part holds the worst case of a valid
// stream; only a damaged one runs it over, and loses those births.
//
// THE WAIT.  A region is handed out only after all earlier ones, so a waiting workgroup always waits for one that is
// running; the wait is still bounded, by the phase's end marker and by wall time (spin_expired, common.h), because on
// a shared device this is the loop that must not spin for ever.  LookBackWait is that rule; the block-chain kernels
// (lis_chain.h: lookback_wait, k_lis_l0's wave-wide look-back) use it as well.
//
// The arithmetic is plain integer code for host and device (tests/test_lis_region_host.py runs it under the address
// and undefined sanitizers); what needs atomics is device code below it.
#ifndef SPERR_AMD_LIS_REGION_H
#define SPERR_AMD_LIS_REGION_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LR_HD __host__ __device__ __forceinline__
#else
#define LR_HD inline
#endif

namespace sperrhip {

constexpr uint32_t kRegionGroups = 8;      // workgroups of a chunk that have segments of their own
constexpr uint32_t kRegionTagShift = 57;   // a region's state words: (plane + 1) << 57 | payload
constexpr uint32_t kSegNoSlot = 0xffffffffu;
constexpr uint32_t kSegOwn = 0x80000000u;   // marks a birth slot that a group's own segment granted (arrays stay below 2^31 slots)

// segment slots for a tree of nsets sets: a sixteenth of the shared part's worst case (a set is born once, so a plane's
// births are a fraction of the sets, and the three smallest set sizes, whose kernels claim shared slots, hold most)
LR_HD uint32_t region_seg_slots(size_t nsets)
{
  return (uint32_t)((nsets + 8) / 16 + 64);
}

// end[0] = filled slots of the shared part, end[g + 1] = end[g] + filled slots of group g's segment
struct SegRanks {
  uint32_t end[kRegionGroups + 1];
  LR_HD uint32_t total() const { return end[kRegionGroups]; }
};

struct SegArray {
  uint32_t cap;      // slots of the shared part
  uint32_t seg;      // slots of a group's segment
  uint32_t groups;   // groups that have one (<= kRegionGroups)

  LR_HD size_t pitch() const { return (size_t)cap + (size_t)seg * groups; }
  LR_HD uint32_t base(uint32_t g) const { return cap + g * seg; }
  // what a group publishes: its counter, cut at the first claim that was refused and at the segment's size
  LR_HD uint32_t published(uint32_t counter, uint32_t firstRefused) const
  {
    const uint32_t m = counter < firstRefused ? counter : firstRefused;
    return m < seg ? m : seg;
  }
  LR_HD uint32_t shared_count(uint32_t counter) const { return counter < cap ? counter : cap; }
  LR_HD SegRanks ranks(uint32_t sharedCount, const uint32_t* groupCount) const
  {
    SegRanks r;
    r.end[0] = sharedCount;
    for (uint32_t g = 0; g < kRegionGroups; g++)
      r.end[g + 1] = r.end[g] + (g < groups ? groupCount[g] : 0u);
    return r;
  }
  // the slot of the kk-th filled one overall, kk < r.total(): the shared part first, then the groups in order
  LR_HD uint32_t slot_of_rank(const SegRanks& r, uint32_t kk) const
  {
    if (kk < r.end[0])
      return kk;
    uint32_t g = 0, first = r.end[0];   // (a loop of known length: the ranks stay in registers)
    for (uint32_t j = 1; j < kRegionGroups; j++)
      if (kk >= r.end[j]) {
        g = j;
        first = r.end[j];
      }
    return base(g) + (kk - first);
  }
};

// one group's view of the array, worked out once by its workgroup; `base` carries kSegOwn
struct SegGroup {
  uint32_t cap, seg, base;
  // a claim of n slots for which the group's counter returned k: does it lie in the segment (then its first slot is
  // base + k), or is it the shared counter's to grant
  LR_HD bool in_segment(uint32_t k, uint32_t n) const { return k + n <= seg; }
  // may the group write this slot of a birth claim.  What its segment granted carries kSegOwn (slot & ~kSegOwn is
  // the index) and lies in the segment whole; anything else came from the shared counter, which grants slots that are
  // not there once it has run past `cap`.  (A test by range -- below cap, or inside the own segment -- would also
  // pass what a shared counter past `cap` hands out.)
  LR_HD bool may_write(uint32_t slot) const { return (slot & kSegOwn) != 0 || slot < cap; }
};
LR_HD SegGroup seg_group(const SegArray& a, uint32_t g)
{
  return SegGroup{a.cap, a.seg, a.base(g) | kSegOwn};
}

// is a birth at bit `rel` of the phase recorded at all: its level has a position mask and the mask reaches that far
// (past the usable stream decoding stops after this plane anyway)
LR_HD bool region_birth_counts(uint32_t levelSlot, uint64_t rel, uint64_t maskBits)
{
  return levelSlot != 0xffu && rel < maskBits;
}

}  // namespace sperrhip

#if defined(__HIPCC__)
#include "common.h"

namespace sperrhip {

// Lanes of ONE wavefront that talk through LDS: the hardware keeps a wavefront's LDS traffic in
// order, but the compiler reasons per thread (it may forward a lane's own earlier store to its
// later load and never look at memory), so every hand-over between lanes needs a fence.
#define WAVE_LDS_SYNC()                                       \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");    \
    __builtin_amdgcn_wave_barrier();                          \
  } while (0)

// one thread: the next region of the pass, or kRegionNoTicket once the pass's end marker is set
constexpr uint32_t kRegionNoTicket = 0xffffffffu;
__device__ __forceinline__ uint32_t region_ticket(const int32_t* planeP1, uint32_t* ticket, int p)
{
  const bool over = __hip_atomic_load(planeP1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p + 1;
  return over ? kRegionNoTicket : atomicAdd(ticket, 1u);
}

// ---- the segmented arrays: the atomics.  segCount / segRefused are the workgroup's LDS counters (0 and 0xffffffff
//      at the kernel's start), shared the chunk's global counter.

// n >= 1 slots in a row for births of the group: the first one, for region_write_birth alone to read (it carries kSegOwn
// when the segment granted it; the shared counter's come back as they are).  No test for n == 0: k_lis_hi always asks
// for one, k_lis_mx for one or for the popcount of a ballot it has tested to be non-zero.
__device__ __forceinline__ uint32_t region_claim_births(const SegGroup& a, uint32_t* segCount, uint32_t* segRefused,
                                                        uint32_t* shared, uint32_t n)
{
  const uint32_t k = atomicAdd(segCount, n);
  if (a.in_segment(k, n))
    return a.base + k;
  atomicMin(segRefused, k);   // the segment is full from here on
  return atomicAdd(shared, n);
}

// the index of one slot for a leaf event, or kSegNoSlot (claims of one never straddle the segment's end: no segRefused)
__device__ __forceinline__ uint32_t region_claim_leaf(const SegGroup& a, uint32_t* segCount, uint32_t* shared)
{
  const uint32_t k = atomicAdd(segCount, 1u);
  if (a.in_segment(k, 1u))
    return (a.base + k) & ~kSegOwn;
  const uint32_t sl = atomicAdd(shared, 1u);
  return sl < a.cap ? sl : kSegNoSlot;
}

// a set of list level `lev` born insignificant at bit `rel` of the phase, into a slot of a claim (the first one, or one
// of the n - 1 behind it); levelMask: the position mask of that level
__device__ __forceinline__ void region_write_birth(const SegGroup& a, uint32_t slot, uint64_t* bornPacked,
                                                   uint64_t* bornPosLev, uint64_t* levelMask, uint32_t lev, uint64_t rel,
                                                   uint64_t packed)
{
  if (!a.may_write(slot))
    return;   // (only a damaged stream asks for more slots than there are sets)
  slot &= ~kSegOwn;
  bornPacked[slot] = packed;
  bornPosLev[slot] = ((uint64_t)lev << 48) | rel;
  atomic_or64(levelMask + (rel >> 6), 1ull << (rel & 63));
}

// one thread of a group g < kRegionGroups, after the workgroup's last region
__device__ __forceinline__ void region_publish_counts(const SegArray& born, const SegArray& leaf, uint32_t g, uint32_t bornCount,
                                                      uint32_t bornRefused, uint32_t leafCount, uint32_t* hiBornCnt,
                                                      uint32_t* hiLeafCnt)
{
  hiBornCnt[g] = born.published(bornCount, bornRefused);
  hiLeafCnt[g] = leaf.published(leafCount, kSegNoSlot);
}

// ---- the bounded wait for a tagged word.  After every poll that did not find its word:
//        switch (w.step(marker, p, sleep)) { kWaitOn: poll again; kWaitPhaseOver: the pass has ended, the word will
//        not come; kWaitExpired: a minute of wall time has passed, the device has stopped making progress -- the caller
//        gives up, as a rule with lookback_give_up }
//      `sleep`: s_sleep 1 before the next poll -- each call site says which and why.
enum WaitStep { kWaitOn, kWaitPhaseOver, kWaitExpired };

struct LookBackWait {
  uint32_t spins = 0;
  uint64_t t0 = 0;
  __device__ __forceinline__ WaitStep step(const int32_t* planeP1, int p, bool sleep)
  {
    // (the end-of-pass marker is looked at now and then: the poll stays one load long)
    if ((++spins & 15u) == 0 && __hip_atomic_load(planeP1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p + 1)
      return kWaitPhaseOver;
    if (spin_expired(spins, t0))
      return kWaitExpired;
    if (sleep)
      __builtin_amdgcn_s_sleep(1);
    return kWaitOn;
  }
};

// the wait has expired: the host reports kErrLookBackTimeout apart from a damaged stream, and the marker ends every
// other wait of the pass
__device__ __forceinline__ void lookback_give_up(uint32_t* error, int32_t* planeP1, int p)
{
  *error = kErrLookBackTimeout;
  __hip_atomic_store(planeP1, p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace sperrhip
#endif

#endif
