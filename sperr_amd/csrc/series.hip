// series.hip -- the kernels of the time-series calls (series.h: the rule).
//
//   k_series_fwd<T, l>    the 2^l steps of a group, through a table of device pointers, into its 2^l dense fp64 bands: all
//                         l levels in registers, the steps once in and the bands once out
//   k_series_inv<OT, l>   the bands of a group (a NULL entry: a band that is not needed, zero) into those of its steps
//                         whose entry of the output table is not NULL
//
// One launch takes every consecutive group of one l.  A lane takes a pack of 16 bytes of the narrower side -- four floats,
// two doubles; two floats in k_series_fwd<float, 4> -- of every step at one position: items are (group, pack) pairs in
// a grid-stride loop.  Time steps rarely lie back to back and every pointer needs only the alignment of its type, so
// there is no common head to peel: each pointer is tested where it is used (the same answer for every pack of a
// volume), one vector access where pointer and pack are aligned, element by element otherwise and in the last, short
// pack.  No LDS, no scratch.
#include "series_run.h"

#include <algorithm>

namespace sperrhip {

namespace {

typedef float SFloat4 __attribute__((ext_vector_type(4)));
typedef float SFloat2 __attribute__((ext_vector_type(2)));
typedef double SDouble2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kSeriesThreads = 256;
constexpr uint32_t kSeriesGroupsPerCU = 4;

// samples of a lane's pack in k_series_fwd: 16 bytes of the steps, but 8 for sixteen fp32 steps, whose 64 doubles in
// flight would leave one wavefront per SIMD (264 registers; 2 x 16 doubles need 140)
template <typename T, int l>
constexpr uint32_t series_fwd_pack()
{
  return sizeof(T) == 4 && l == 4 ? 2 : 16 / sizeof(T);
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// P consecutive samples at s[i ..], widened; `full`: all of them are inside the volume
template <uint32_t P>
__device__ __forceinline__ void load_pack(const float* s, uint64_t i, uint64_t n, bool full, double* out)
{
  if (P == 4 && full && aligned16(s + i)) {
    const SFloat4 pk = *reinterpret_cast<const SFloat4*>(s + i);
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      out[j] = (double)pk[j];
  }
  else if (P == 2 && full && (reinterpret_cast<uintptr_t>(s + i) & 7) == 0) {
    const SFloat2 pk = *reinterpret_cast<const SFloat2*>(s + i);
    out[0] = (double)pk[0];
    out[1] = (double)pk[1];
  }
  else {
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      out[j] = i + j < n ? (double)s[i + j] : 0.0;
  }
}
template <uint32_t P>
__device__ __forceinline__ void load_pack(const double* s, uint64_t i, uint64_t n, bool full, double* out)
{
  if (full && aligned16(s + i)) {
#pragma unroll
    for (uint32_t j = 0; j < P; j += 2) {
      const SDouble2 pk = *reinterpret_cast<const SDouble2*>(s + i + j);
      out[j] = pk[0];
      out[j + 1] = pk[1];
    }
  }
  else {
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      out[j] = i + j < n ? s[i + j] : 0.0;
  }
}

template <uint32_t P>
__device__ __forceinline__ void store_pack(double* d, uint64_t i, uint64_t n, bool full, const double* v)
{
  if (full && aligned16(d + i)) {
#pragma unroll
    for (uint32_t j = 0; j < P; j += 2)
      *reinterpret_cast<SDouble2*>(d + i + j) = SDouble2{v[j], v[j + 1]};
  }
  else {
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      if (i + j < n)
        d[i + j] = v[j];
  }
}
template <uint32_t P>
__device__ __forceinline__ void store_pack(float* d, uint64_t i, uint64_t n, bool full, const double* v)
{
  if (P == 4 && full && aligned16(d + i))
    *reinterpret_cast<SFloat4*>(d + i) = SFloat4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  else {
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      if (i + j < n)
        d[i + j] = (float)v[j];
  }
}

// A lane's walk over the (group, pack) items of a launch, item = q * npacks + p, in a grid-stride loop: one division
// where it starts and one where it crosses into another group; in between the stride is added to p
struct SeriesWalk {
  uint64_t q, p;
  __device__ __forceinline__ explicit SeriesWalk(uint64_t npacks)
  {
    const uint64_t item = (uint64_t)blockIdx.x * kSeriesThreads + threadIdx.x;
    q = item / npacks;
    p = item - q * npacks;
  }
  __device__ __forceinline__ void next(uint64_t npacks)
  {
    p += (uint64_t)gridDim.x * kSeriesThreads;
    if (p >= npacks) {   // (rare: a lane leaves a group npacks / stride passes after it entered it)
      const uint64_t c = p / npacks;
      q += c;
      p -= c * npacks;
    }
  }
};

// steps, bands: the series' tables, entry `first` the first step (band) of the launch's first group
template <typename T, int l>
__global__ __launch_bounds__(kSeriesThreads) void k_series_fwd(const T* const* __restrict__ steps,
                                                               double* const* __restrict__ bands, uint64_t first,
                                                               uint64_t ngroups, uint64_t n)
{
  constexpr int g = 1 << l;
  constexpr uint32_t P = series_fwd_pack<T, l>();
  const uint64_t npacks = (n + P - 1) / P;
  SeriesWalk w(npacks);
  for (; w.q < ngroups; w.next(npacks)) {
    const uint64_t q = w.q, i = w.p * P;
    const bool full = i + P <= n;
    const T* const* sp = steps + first + q * g;
    double* const* bp = bands + first + q * g;
    double v[P][g];
#pragma unroll
    for (int t = 0; t < g; t++) {
      double in[P];
      load_pack<P>(sp[t], i, n, full, in);
#pragma unroll
      for (uint32_t j = 0; j < P; j++)
        v[j][t] = in[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      series_forward<l>(v[j]);
#pragma unroll
    for (int t = 0; t < g; t++) {
      double out[P];
#pragma unroll
      for (uint32_t j = 0; j < P; j++)
        out[j] = v[j][t];
      store_pack<P>(bp[t], i, n, full, out);
    }
  }
}

// (the outputs never alias the bands: the calls decode into the library's buffer, and the stage call refuses it)
template <typename OT, int l>
__global__ __launch_bounds__(kSeriesThreads) void k_series_inv(const double* const* __restrict__ bands,
                                                               OT* const* __restrict__ outs, uint64_t first,
                                                               uint64_t ngroups, uint64_t n)
{
  constexpr int g = 1 << l;
  constexpr uint32_t P = 16 / sizeof(OT);
  const uint64_t npacks = (n + P - 1) / P;
  SeriesWalk w(npacks);
  for (; w.q < ngroups; w.next(npacks)) {
    const uint64_t q = w.q, i = w.p * P;
    const bool full = i + P <= n;
    const double* const* bp = bands + first + q * g;
    OT* const* op = outs + first + q * g;
    double v[P][g];
#pragma unroll
    for (int t = 0; t < g; t++) {
      double in[P];
      const double* b = bp[t];
      if (b)
        load_pack<P>(b, i, n, full, in);
      else {
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          in[j] = 0.0;
      }
#pragma unroll
      for (uint32_t j = 0; j < P; j++)
        v[j][t] = in[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < P; j++)
      series_inverse<l>(v[j]);
#pragma unroll
    for (int t = 0; t < g; t++) {
      OT* o = op[t];
      if (!o)
        continue;
      double out[P];
#pragma unroll
      for (uint32_t j = 0; j < P; j++)
        out[j] = v[j][t];
      store_pack<P>(o, i, n, full, out);
    }
  }
}

int series_grid(uint64_t items, uint32_t* groups)
{
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const uint64_t cap = (uint64_t)std::max(cus, 1) * kSeriesGroupsPerCU;
  const uint64_t want = (items + kSeriesThreads - 1) / kSeriesThreads;
  *groups = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
  return 0;
}

template <typename T, int l>
int fwd_launch(const void* const* steps, double* const* bands, uint64_t first, uint64_t ngroups, uint64_t n,
               hipStream_t st)
{
  constexpr uint64_t P = series_fwd_pack<T, l>();
  uint32_t grid = 0;
  if (series_grid(ngroups * ((n + P - 1) / P), &grid))
    return -1;
  LAUNCH_K((k_series_fwd<T, l>), dim3(grid), dim3(kSeriesThreads), 0, st, reinterpret_cast<const T* const*>(steps),
           bands, first, ngroups, n);
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename OT, int l>
int inv_launch(const double* const* bands, void* const* outs, uint64_t first, uint64_t ngroups, uint64_t n,
               hipStream_t st)
{
  constexpr uint64_t P = 16 / sizeof(OT);
  uint32_t grid = 0;
  if (series_grid(ngroups * ((n + P - 1) / P), &grid))
    return -1;
  LAUNCH_K((k_series_inv<OT, l>), dim3(grid), dim3(kSeriesThreads), 0, st, bands,
           reinterpret_cast<OT* const*>(outs), first, ngroups, n);
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int fwd_level(int l, const void* const* steps, double* const* bands, uint64_t first, uint64_t ngroups, uint64_t n,
              hipStream_t st)
{
  switch (l) {
    case 0: return fwd_launch<T, 0>(steps, bands, first, ngroups, n, st);
    case 1: return fwd_launch<T, 1>(steps, bands, first, ngroups, n, st);
    case 2: return fwd_launch<T, 2>(steps, bands, first, ngroups, n, st);
    case 3: return fwd_launch<T, 3>(steps, bands, first, ngroups, n, st);
    case 4: return fwd_launch<T, 4>(steps, bands, first, ngroups, n, st);
    default: return -1;
  }
}

template <typename OT>
int inv_level(int l, const double* const* bands, void* const* outs, uint64_t first, uint64_t ngroups, uint64_t n,
              hipStream_t st)
{
  switch (l) {
    case 0: return inv_launch<OT, 0>(bands, outs, first, ngroups, n, st);
    case 1: return inv_launch<OT, 1>(bands, outs, first, ngroups, n, st);
    case 2: return inv_launch<OT, 2>(bands, outs, first, ngroups, n, st);
    case 3: return inv_launch<OT, 3>(bands, outs, first, ngroups, n, st);
    case 4: return inv_launch<OT, 4>(bands, outs, first, ngroups, n, st);
    default: return -1;
  }
}

// the runs of consecutive groups of one l among the groups [g0, g1) of the plan: f(l, first step, groups)
template <typename F>
int for_runs(size_t nsteps, int levels, size_t g0, size_t g1, F&& f)
{
  size_t i = g0;
  while (i < g1) {
    size_t start, s2;
    int l, l2;
    series_group(nsteps, levels, i, &start, &l);
    size_t k = i + 1;
    for (; k < g1; k++) {
      series_group(nsteps, levels, k, &s2, &l2);
      if (l2 != l)
        break;
    }
    if (f(l, start, k - i))
      return -1;
    i = k;
  }
  return 0;
}

}  // namespace

int series_forward_run(const void* const* d_steps, int is_float, double* const* d_bands, size_t nsteps, int levels,
                       size_t g0, size_t g1, size_t n, hipStream_t st)
{
  if (!d_steps || !d_bands || n == 0 || levels < 0 || levels > kSeriesMaxLevels || g0 > g1 ||
      g1 > series_group_count(nsteps, levels))
    return -1;
  return for_runs(nsteps, levels, g0, g1, [&](int l, size_t first, size_t ngroups) {
    return is_float ? fwd_level<float>(l, d_steps, d_bands, first, ngroups, n, st)
                    : fwd_level<double>(l, d_steps, d_bands, first, ngroups, n, st);
  });
}

int series_inverse_run(const double* const* d_bands, void* const* d_outs, int output_float, size_t nsteps, int levels,
                       size_t g0, size_t g1, size_t n, hipStream_t st)
{
  if (!d_bands || !d_outs || n == 0 || levels < 0 || levels > kSeriesMaxLevels || g0 > g1 ||
      g1 > series_group_count(nsteps, levels))
    return -1;
  return for_runs(nsteps, levels, g0, g1, [&](int l, size_t first, size_t ngroups) {
    return output_float ? inv_level<float>(l, d_bands, d_outs, first, ngroups, n, st)
                        : inv_level<double>(l, d_bands, d_outs, first, ngroups, n, st);
  });
}

}  // namespace sperrhip
