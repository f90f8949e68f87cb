// quality.h -- the quality figures of a reconstruction (sperr::calc_stats<T> then sperr::calc_mean_var<T> of the
// reference, src/sperr_helper.cpp:429-518,594-641) from block partials: the block plan and the host finish.
// Plain C++: no HIP here, so a host program (tests/cpp/quality_check.cpp) uses it without a GPU.  quality.hip forms
// the partials on the device; quality_run is its entry point.
//
// The figures are blocked, strictly sequential sums in T: squared differences in blocks of 8192, mean and variance
// in blocks of 16384, every block summed left to right, then the block sums left to right with the tail block last.
// That order is part of the result.
#ifndef SPERR_AMD_QUALITY_H
#define SPERR_AMD_QUALITY_H

#include <array>
#include <cmath>
#include <cstddef>
#include <limits>

#include "view.h"

namespace sperrhip {

constexpr size_t kQualSqBlock = 8192;     // calc_stats: stride_size
constexpr size_t kQualMvBlock = 16384;    // calc_mean_var: stride_size (two squared-difference blocks)

struct QualityPlan {
  size_t n;
  size_t sq_blocks, sq_tail;   // whole blocks of 8192 and the length of the tail block (0: an empty one, sum 0)
  size_t mv_blocks, mv_tail;   // the same in blocks of 16384
  // partials a finish reads: the whole blocks, then the tail block's
  size_t sq_partials() const { return sq_blocks + 1; }
  size_t mv_partials() const { return mv_blocks + 1; }
};

inline QualityPlan quality_plan(size_t n)
{
  return {n, n / kQualSqBlock, n % kQualSqBlock, n / kQualMvBlock, n % kQualMvBlock};
}

// block sums left to right, the tail block's last (std::accumulate from T{0} over sum_vec / tmp_buf)
template <typename T>
inline T quality_sum_partials(const T* part, size_t count)
{
  T total = 0;
  for (size_t i = 0; i < count; i++)
    total += part[i];
  return total;
}

// what is left of a pair of arrays once the blocks are summed
template <typename T>
struct QualityPartials {
  const T* sq;       // plan.sq_partials() sums of d * d, d = |a[i] - b[i]|
  const T* var;      // plan.mv_partials() sums of (a[i] - mean) * (a[i] - mean)
  T mean;            // quality_sum_partials of the mv_partials() sums of a[i], divided by T(n)
  T linfty;          // max d
  T min, max;        // of a
  bool differ;       // any a[i] != b[i]
};

// {rmse, linfty, psnr, min, max, mean, var, mse}.  Identical arrays: {0, 0, +inf, min, max, mean, var, 0} whatever
// the range (the reference's early return).  libm runs here, on the host.
template <typename T>
inline std::array<T, 8> quality_finish(const QualityPlan& plan, const QualityPartials<T>& p)
{
  const T var = quality_sum_partials(p.var, plan.mv_partials()) / T(plan.n);
  if (!p.differ)
    return {T(0), T(0), std::numeric_limits<T>::infinity(), p.min, p.max, p.mean, var, T(0)};
  const T mse = quality_sum_partials(p.sq, plan.sq_partials()) / T(plan.n);
  const T rmse = std::sqrt(mse);
  const T range_sq = (p.max - p.min) * (p.max - p.min);
  const T psnr = std::log10(range_sq / mse) * T(10);
  return {rmse, p.linfty, psnr, p.min, p.max, p.mean, var, mse};
}

// ---- the device side (quality.hip) ----------------------------------------------------------------------------
// Bytes of workspace quality_run needs for nvol arrays of n values; 0: the sizes overflow or are empty.
size_t quality_workspace_bytes(size_t nvol, size_t n, int is_float);
// out[nvol * 8] from nvol arrays of n values back to back in d_orig / d_recon.  `ws`: quality_workspace_bytes() of
// device memory, 256-byte aligned.  Three kernels and one copy on `hip_stream` (a hipStream_t), one host wait at
// the end.  0 ok, -1 a HIP error (out untouched).
int quality_run(const void* d_orig, const void* d_recon, int is_float, size_t nvol, size_t n, void* ws,
                double* out, void* hip_stream);

// The same for one pair of arrays read through strided views (view.h) of dims (dimx, dimy, dimz), each from its
// first element: the figures are bit for bit those of quality_run on packed copies.  dimx and dimy stay below
// kViewCursorMaxDim.  The workspace's size is 0 for dims that are refused; -1 also for a view that is not valid.
size_t quality_view_workspace_bytes(size_t dimx, size_t dimy, size_t dimz, int is_float);
int quality_view_run(const void* d_orig, ViewPitch p_orig, const void* d_recon, ViewPitch p_recon, int is_float,
                     size_t dimx, size_t dimy, size_t dimz, void* ws, double* out, void* hip_stream);

}  // namespace sperrhip

#endif
