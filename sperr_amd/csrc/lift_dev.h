// lift_dev.h -- device-side pieces that several units of the float stages share: the crop writers' rule (xform.hip's
// scatter and every lifting unit), the lifting kernels' dynamic LDS, the halo of a tile and the mirror rule at a
// signal's ends (lift_axis.hip, lift_xyz_fwd.hip, lift_xyz_inv.hip, lift_xyz_inv_crop.hip)
#ifndef SPERR_AMD_LIFT_DEV_H
#define SPERR_AMD_LIFT_DEV_H

#include "common.h"

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// crop variant of the writers (kCrop, CropGeom): a chunk writes only the samples of its window, at box
// addresses.  kCrop false is the whole-volume decode: those instantiations compile to what they were.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool crop_has(const CropGeom& g, uint32_t x, uint32_t y, uint32_t z)
{
  return x - g.lo[0] < g.hi[0] - g.lo[0] && y - g.lo[1] < g.hi[1] - g.lo[1] && z - g.lo[2] < g.hi[2] - g.lo[2];
}
// box address of chunk sample (x, y, z) of the window
__device__ __forceinline__ size_t crop_addr(const CropGeom& g, const VolDesc& vd, uint32_t x, uint32_t y, uint32_t z)
{
  const size_t bx = (size_t)((int64_t)x + g.rel[0]), by = (size_t)((int64_t)y + g.rel[1]),
               bz = (size_t)((int64_t)z + g.rel[2]);
  return (bz * vd.dims[1] + by) * vd.dims[0] + bx;
}

// the one declaration of the lifting kernels' dynamic LDS
extern __shared__ __attribute__((aligned(16))) char dyn_smem[];

// rows (samples) of halo on each side of a tile: the four lifting steps reach one further each
constexpr int kXYHalo = 4;

// position q of the whole-sample symmetric extension of a signal of n >= 2 samples
__device__ __forceinline__ uint32_t reflect_index(int q, int n)
{
  const int period = 2 * (n - 1);
  q = q < 0 ? -q : q;
  if (q >= period)
    q %= period;
  return (uint32_t)(q < n ? q : period - q);
}

}  // namespace sperrhip

#endif
