// boxes.hip -- the one kernel of the boxes call's staged form (boxes.h: the plan, the pair record, the constants).
//
//   k_boxes_copy<T, kVec>   every pair's window, from the staging array into its entry's box of the output
//
// The samples of all pairs' windows, pair after pair and x fastest inside a window, are one run of `total` samples --
// as many as the output has, for the windows tile every box.  The work is split by OUTPUT BYTES, as k_trunc_container
// splits its own: workgroup b moves the samples of kBoxesSliceBytes of that run and finds the pairs under them by
// binary search over `first`, so one pair of 256^3 and five hundred of 8^3 load the device alike and the grid has one
// dimension.  Consecutive lanes take consecutive samples of a window's row: loads and stores coalesce on both sides.
//
// kVec moves 16-byte packs; the host chooses it once per call (boxes_vec_ok: both arrays, every window's first
// sample and width and all pitches are whole packs).  The other form moves element by element and needs the
// alignment of T only.  T is an unsigned integer of the output's width: the kernel moves bits.
#include "common.h"
#include "boxes.h"

namespace sperrhip {

namespace {

template <typename T>
struct BoxesPack;
template <>
struct BoxesPack<uint32_t> {
  typedef uint32_t type __attribute__((ext_vector_type(4)));
};
template <>
struct BoxesPack<uint64_t> {
  typedef uint64_t type __attribute__((ext_vector_type(2)));
};

template <typename T, bool kVec>
__global__ __launch_bounds__(kBoxesThreads) void k_boxes_copy(const T* __restrict__ stage, T* __restrict__ out,
                                                              const BoxesCopyPair* __restrict__ pairs,
                                                              const uint64_t* __restrict__ first, BoxesCopyGeom g)
{
  using Pack = typename BoxesPack<T>::type;
  constexpr uint32_t P = kVec ? kBoxesPackBytes / sizeof(T) : 1u;   // samples a lane moves at a time
  constexpr uint32_t kSlice = kBoxesSliceBytes / sizeof(T);         // samples of a workgroup
  const uint64_t lo = (uint64_t)blockIdx.x * kSlice;
  if (lo >= g.total)
    return;
  const uint64_t hi = min(lo + kSlice, g.total);
  // (uniform) the pairs a .. e - 1 have samples in the slice: first[a] <= lo, first[e] >= hi
  uint32_t a = 0, e = g.npairs;
  while (e - a > 1) {
    const uint32_t m = a + (e - a) / 2;
    if (first[m] <= lo)
      a = m;
    else
      e = m;
  }
  uint32_t f = a;
  e = g.npairs;
  while (e - f > 1) {
    const uint32_t m = f + (e - f) / 2;
    if (first[m] < hi)
      f = m;
    else
      e = m;
  }
  for (uint64_t i = lo + (uint64_t)threadIdx.x * P; i < hi; i += (uint64_t)kBoxesThreads * P) {
    uint32_t p = a, q = e;   // first[p] <= i < first[q]
    while (q - p > 1) {
      const uint32_t m = p + (q - p) / 2;
      if (first[m] <= i)
        p = m;
      else
        q = m;
    }
    const BoxesCopyPair c = pairs[p];
    const uint64_t r = i - first[p];
    const uint32_t x = (uint32_t)(r % c.w[0]);
    const uint64_t row = r / c.w[0];
    const uint32_t y = (uint32_t)(row % c.w[1]), z = (uint32_t)(row / c.w[1]);
    const T* s = stage + (c.src + (uint64_t)z * g.srcSlice + (uint64_t)y * g.srcRow + x);
    T* d = out + (c.dst + (uint64_t)z * g.dstSlice + (uint64_t)y * g.dstRow + x);
    if (kVec)
      *reinterpret_cast<Pack*>(d) = *reinterpret_cast<const Pack*>(s);
    else
      *d = *s;
  }
}

template <typename T>
int copy_launch(const void* d_stage, void* d_out, const BoxesCopyPair* d_pairs, const uint64_t* d_first,
                const BoxesCopyGeom& g, bool vec, hipStream_t st)
{
  const uint64_t slice = kBoxesSliceBytes / sizeof(T), nblocks = (g.total + slice - 1) / slice;
  if (nblocks == 0 || nblocks > 0x7fffffffull)
    return -1;
  const T* s = static_cast<const T*>(d_stage);
  T* d = static_cast<T*>(d_out);
  if (vec)
    LAUNCH_K((k_boxes_copy<T, true>), dim3((uint32_t)nblocks), dim3(kBoxesThreads), 0, st, s, d, d_pairs, d_first, g);
  else
    LAUNCH_K((k_boxes_copy<T, false>), dim3((uint32_t)nblocks), dim3(kBoxesThreads), 0, st, s, d, d_pairs, d_first, g);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int boxes_copy_run(const void* d_stage, void* d_out, size_t elem_size, const BoxesCopyPair* d_pairs,
                   const uint64_t* d_first, const BoxesCopyGeom& g, bool vec, void* hip_stream)
{
  if (!d_stage || !d_out || !d_pairs || !d_first || g.npairs == 0 || (elem_size != 4 && elem_size != 8))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  return elem_size == 4 ? copy_launch<uint32_t>(d_stage, d_out, d_pairs, d_first, g, vec, st)
                        : copy_launch<uint64_t>(d_stage, d_out, d_pairs, d_first, g, vec, st);
}

}  // namespace sperrhip
