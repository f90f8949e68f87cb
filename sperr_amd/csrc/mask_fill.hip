// mask_fill.hip -- the kernels of the smooth in-fill of missing values (mask_fill.h: the rule, the levels, the constants).
//
//   k_mask_pull0<T>          level 1 from the samples and the bit array k_mask_survey stored: a cell per lane
//   k_mask_pull              level l + 1 from level l, both in global memory
//   k_mask_top               one workgroup: reads level G, builds the levels G + 1 .. L in LDS, sets an unknown top to
//                            0.0, pushes back down and stores level G complete; sets MaskResult::finite from the flag
//   k_mask_push              completes level l from the complete level l + 1
//   k_mask_fill_smooth<T>    dst[i] = missing ? (T)interp(level 1) : src[i]; dst may be src
//
// As in mask.hip no kernel waits on another workgroup and there are no float atomics: a lane owns its cell, every level
// is a launch of its own, and a sum that is not finite sets the flag word at the head of the pyramid with an integer
// atomic OR.  Every load and store is an element of its type: the samples need the alignment of T only.  The unit
// is built with -ffp-contract=off as all of them are: the rule's products and sums are rounded one by one.
#include "common.h"
#include "mask.h"
#include "mask_fill.h"

namespace sperrhip {

namespace {

constexpr uint32_t kFillThreads = kMaskThreads;
constexpr uint32_t kFillMaxGroups = 8192;

struct LevelDims {
  uint64_t x, y, z;
};

int fill_grid(uint64_t lanes, uint32_t* groups)
{
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const uint64_t cap = std::min<uint64_t>((uint64_t)std::max(cus, 1) * kMaskGroupsPerCU, kFillMaxGroups);
  const uint64_t want = (lanes + kFillThreads - 1) / kFillThreads;
  *groups = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
  return 0;
}

__device__ __forceinline__ bool word_bit(const uint64_t* __restrict__ words, uint64_t i)
{
  return (words[i >> 6] >> (i & 63)) & 1;
}

template <typename T>
__global__ __launch_bounds__(kFillThreads) void k_mask_pull0(const T* __restrict__ src,
                                                             const uint64_t* __restrict__ words, LevelDims d,
                                                             LevelDims c, double* __restrict__ out,
                                                             uint32_t* __restrict__ flag)
{
  const uint64_t cells = c.x * c.y * c.z;
  bool finite = true;
  for (uint64_t cell = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; cell < cells;
       cell += (uint64_t)gridDim.x * kFillThreads) {
    const uint64_t row = cell / c.x, X = cell - row * c.x, Z = row / c.y, Y = row - Z * c.y;
    out[cell] = mask_fill_pull_cell<uint64_t>(
        X, Y, Z, d.x, d.y, d.z,
        [&](uint64_t x, uint64_t y, uint64_t z) {
          const uint64_t i = (z * d.y + y) * d.x + x;
          return word_bit(words, i) ? mask_fill_unknown() : (double)src[i];
        },
        &finite);
  }
  if (!finite)
    atomicOr(flag, 1u);
}

__global__ __launch_bounds__(kFillThreads) void k_mask_pull(const double* __restrict__ fine, LevelDims d, LevelDims c,
                                                            double* __restrict__ out, uint32_t* __restrict__ flag)
{
  const uint64_t cells = c.x * c.y * c.z;
  bool finite = true;
  for (uint64_t cell = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; cell < cells;
       cell += (uint64_t)gridDim.x * kFillThreads) {
    const uint64_t row = cell / c.x, X = cell - row * c.x, Z = row / c.y, Y = row - Z * c.y;
    out[cell] = mask_fill_pull_cell<uint64_t>(
        X, Y, Z, d.x, d.y, d.z, [&](uint64_t x, uint64_t y, uint64_t z) { return fine[(z * d.y + y) * d.x + x]; },
        &finite);
  }
  if (!finite)
    atomicOr(flag, 1u);
}

// the dims of the level j levels above one of dims g (j = 0: g itself), and the cells of the levels 1 .. j - 1 above
// it: where level j begins in LDS
struct TopLevel {
  uint32_t x, y, z, off;
};
__device__ __forceinline__ TopLevel top_level(uint32_t gx, uint32_t gy, uint32_t gz, uint32_t j)
{
  TopLevel t{gx, gy, gz, 0};
  for (uint32_t k = 0; k < j; k++) {
    if (k > 0)
      t.off += t.x * t.y * t.z;
    t.x = (t.x + 1) >> 1;
    t.y = (t.y + 1) >> 1;
    t.z = (t.z + 1) >> 1;
  }
  return t;
}

// `above` = L - G levels in LDS (the host has checked that they fit); level G, of dims (gx, gy, gz), is lvG
__global__ __launch_bounds__(kMaskTopThreads) void k_mask_top(double* __restrict__ lvG, uint32_t gx, uint32_t gy,
                                                              uint32_t gz, uint32_t above,
                                                              const uint32_t* __restrict__ flag,
                                                              uint64_t* __restrict__ res_finite)
{
  __shared__ double s_lv[kMaskTopLdsCells];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0)
    s_bad = 0;
  __syncthreads();
  bool finite = true;
  // the pull: level j from level j - 1, which for j = 1 is the one in global memory
  for (uint32_t j = 1; j <= above; j++) {
    const TopLevel f = top_level(gx, gy, gz, j - 1), c = top_level(gx, gy, gz, j);
    const uint32_t cells = c.x * c.y * c.z;
    for (uint32_t cell = threadIdx.x; cell < cells; cell += kMaskTopThreads) {
      const uint32_t row = cell / c.x, X = cell - row * c.x, Z = row / c.y, Y = row - Z * c.y;
      double v;
      if (j == 1)
        v = mask_fill_pull_cell<uint32_t>(
            X, Y, Z, f.x, f.y, f.z, [&](uint32_t x, uint32_t y, uint32_t z) { return lvG[(z * f.y + y) * f.x + x]; },
            &finite);
      else
        v = mask_fill_pull_cell<uint32_t>(
            X, Y, Z, f.x, f.y, f.z,
            [&](uint32_t x, uint32_t y, uint32_t z) { return s_lv[f.off + (z * f.y + y) * f.x + x]; }, &finite);
      s_lv[c.off + cell] = v;
    }
    __syncthreads();
  }
  if (!finite)
    atomicOr(&s_bad, 1u);
  // the top: one cell, in LDS or -- a volume of at most two samples an axis -- level G itself
  if (threadIdx.x == 0) {
    double* top = above ? &s_lv[top_level(gx, gy, gz, above).off] : lvG;
    if (!mask_fill_known(*top))
      *top = 0.0;
  }
  __syncthreads();
  // the push: level j from level j + 1; level 0 of these is level G, completed where it lies
  for (uint32_t j = above; j-- > 0;) {
    const TopLevel f = top_level(gx, gy, gz, j), c = top_level(gx, gy, gz, j + 1);
    const uint32_t cells = f.x * f.y * f.z;
    for (uint32_t cell = threadIdx.x; cell < cells; cell += kMaskTopThreads) {
      double* at = j == 0 ? &lvG[cell] : &s_lv[f.off + cell];
      if (mask_fill_known(*at))
        continue;
      const uint32_t row = cell / f.x, x = cell - row * f.x, z = row / f.y, y = row - z * f.y;
      *at = mask_fill_interp<uint32_t>(
          x, y, z, c.x, c.y, c.z, [&](uint32_t X, uint32_t Y, uint32_t Z) { return s_lv[c.off + (Z * c.y + Y) * c.x + X]; });
    }
    __syncthreads();
  }
  // (the flag word has what the launches before this one found; s_bad what this one did)
  if (threadIdx.x == 0)
    *res_finite = (*flag | s_bad) ? 0ull : 1ull;
}

__global__ __launch_bounds__(kFillThreads) void k_mask_push(double* __restrict__ lev, LevelDims d,
                                                            const double* __restrict__ coarse, LevelDims c)
{
  const uint64_t cells = d.x * d.y * d.z;
  for (uint64_t cell = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; cell < cells;
       cell += (uint64_t)gridDim.x * kFillThreads) {
    if (mask_fill_known(lev[cell]))
      continue;
    const uint64_t row = cell / d.x, x = cell - row * d.x, z = row / d.y, y = row - z * d.y;
    lev[cell] = mask_fill_interp<uint64_t>(
        x, y, z, c.x, c.y, c.z, [&](uint64_t X, uint64_t Y, uint64_t Z) { return coarse[(Z * c.y + Y) * c.x + X]; });
  }
}

// I: uint32_t where the volume has fewer than 2^32 samples -- the divisions of a missing sample's index are the cost
template <typename T, typename I>
__global__ __launch_bounds__(kFillThreads) void k_mask_fill_smooth(const T* src, T* dst, LevelDims d,
                                                                   const uint64_t* __restrict__ words,
                                                                   const double* __restrict__ lv1, LevelDims c)
{
  const uint64_t n = d.x * d.y * d.z;
  for (uint64_t i = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFillThreads) {
    T v = src[i];
    if (word_bit(words, i)) {
      const I row = (I)i / (I)d.x, x = (I)i - row * (I)d.x, z = row / (I)d.y, y = row - z * (I)d.y;
      v = (T)mask_fill_interp<I>(x, y, z, (I)c.x, (I)c.y, (I)c.z, [&](I X, I Y, I Z) {
        return lv1[((uint64_t)Z * c.y + Y) * c.x + X];
      });
    }
    dst[i] = v;
  }
}

LevelDims dims_of(const MaskFillPlan& p, uint32_t l) { return LevelDims{p.dim[l][0], p.dim[l][1], p.dim[l][2]}; }

uint32_t* flag_of(void* pyr) { return static_cast<uint32_t*>(pyr); }
double* level_of(const MaskFillPlan& p, void* pyr, uint32_t l)
{
  return reinterpret_cast<double*>(static_cast<char*>(pyr) + kMaskFillHeadBytes) + p.off[l];
}

template <typename T>
int pull0_launch(const T* src, const uint64_t* words, const MaskFillPlan& p, void* pyr, hipStream_t st)
{
  uint32_t groups = 0;
  if (fill_grid(p.cells[1], &groups))
    return -1;
  LAUNCH_K((k_mask_pull0<T>), dim3(groups), dim3(kFillThreads), 0, st, src, words, dims_of(p, 0), dims_of(p, 1),
           level_of(p, pyr, 1), flag_of(pyr));
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int fill_smooth_launch(const T* src, T* dst, const uint64_t* words, const MaskFillPlan& p, void* pyr, hipStream_t st)
{
  uint32_t groups = 0;
  if (fill_grid(p.cells[0], &groups))
    return -1;
  if (p.cells[0] < (uint64_t(1) << 32))
    LAUNCH_K((k_mask_fill_smooth<T, uint32_t>), dim3(groups), dim3(kFillThreads), 0, st, src, dst, dims_of(p, 0), words,
             level_of(p, pyr, 1), dims_of(p, 1));
  else
    LAUNCH_K((k_mask_fill_smooth<T, uint64_t>), dim3(groups), dim3(kFillThreads), 0, st, src, dst, dims_of(p, 0), words,
             level_of(p, pyr, 1), dims_of(p, 1));
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

size_t mask_fill_workspace_bytes(size_t dimx, size_t dimy, size_t dimz)
{
  MaskFillPlan p;
  return mask_fill_plan(dimx, dimy, dimz, &p) ? p.bytes : 0;
}

int mask_fill_pull_run(const void* d_src, int is_float, const MaskFillPlan& p, void* ws, void* pyr, void* hip_stream)
{
  if (p.L == 0)
    return 0;
  if (!d_src || !ws || !pyr || (uintptr_t)pyr % 256 != 0 || p.ldsCells > kMaskTopLdsCells ||
      p.cells[p.G] > 8ull * kMaskTopCells)
    return -1;
  uint64_t* finite = mask_result_finite(ws, (size_t)p.cells[0]);
  const uint64_t* words = mask_bit_words(ws, (size_t)p.cells[0]);
  if (!finite || !words)
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  HIP_CHECK(hipMemsetAsync(flag_of(pyr), 0, sizeof(uint32_t), st));
  if (is_float ? pull0_launch(static_cast<const float*>(d_src), words, p, pyr, st)
               : pull0_launch(static_cast<const double*>(d_src), words, p, pyr, st))
    return -1;
  for (uint32_t l = 1; l < p.G; l++) {
    uint32_t groups = 0;
    if (fill_grid(p.cells[l + 1], &groups))
      return -1;
    LAUNCH_K(k_mask_pull, dim3(groups), dim3(kFillThreads), 0, st, level_of(p, pyr, l), dims_of(p, l), dims_of(p, l + 1),
             level_of(p, pyr, l + 1), flag_of(pyr));
    HIP_CHECK(hipGetLastError());
  }
  LAUNCH_K(k_mask_top, dim3(1), dim3(kMaskTopThreads), 0, st, level_of(p, pyr, p.G), (uint32_t)p.dim[p.G][0],
           (uint32_t)p.dim[p.G][1], (uint32_t)p.dim[p.G][2], p.L - p.G, flag_of(pyr), finite);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int mask_fill_push_run(const void* d_src, int is_float, const MaskFillPlan& p, const void* ws, void* pyr,
                       void* d_filled, void* hip_stream)
{
  if (!d_src || !ws || !d_filled || p.L == 0 || !pyr)
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t* words = mask_bit_words(const_cast<void*>(ws), (size_t)p.cells[0]);
  if (!words)
    return -1;
  for (uint32_t l = p.G; l-- > 1;) {
    uint32_t groups = 0;
    if (fill_grid(p.cells[l], &groups))
      return -1;
    LAUNCH_K(k_mask_push, dim3(groups), dim3(kFillThreads), 0, st, level_of(p, pyr, l), dims_of(p, l),
             level_of(p, pyr, l + 1), dims_of(p, l + 1));
    HIP_CHECK(hipGetLastError());
  }
  return is_float ? fill_smooth_launch(static_cast<const float*>(d_src), static_cast<float*>(d_filled), words, p, pyr, st)
                  : fill_smooth_launch(static_cast<const double*>(d_src), static_cast<double*>(d_filled), words, p, pyr,
                                       st);
}

}  // namespace sperrhip
