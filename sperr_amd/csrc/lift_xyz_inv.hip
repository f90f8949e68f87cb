// lift_xyz_inv.hip -- the inverse CDF 9/7 lifting DWT with the three passes of a level in one kernel, as HIP kernels
// for gfx950: the finest level through the chunk map into the volume, k_lift_xyz_inv<IO, SG> (lift_xyz_inv.h: four of
// its instantiations), and the second level into a compact box, k_lift2_inv<SG>.  The finest level's crop variants:
// lift_xyz_inv_crop.hip.  Compile with -ffp-contract=off.
#include "lift_xyz_inv.h"

namespace sperrhip {

// The second level, inverse: the region (cx, cy, cz) of every chunk from the box the coarser levels worked in (F.bufx /
// F.bufy, the samples inside F.inner) and the coefficients (at the chunk's strides qrow / qslice) into `out`, a box of
// its own with rows of cx samples, chunk c's outStride samples in; no mean added.  See k_lift2_fwd.
template <bool SG>
__global__ void __launch_bounds__(kXYZThreadsI) __attribute__((amdgpu_waves_per_eu(kXYZThreadsI / 256, kXYZThreadsI / 256)))
k_lift2_inv(const double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz, LiftConsts K, const CoderState* st,
            double* out, size_t outStride, LiftFuse F, uint32_t nseg, uint32_t qrow, size_t qslice)
{
  if (st[blockIdx.y].is_const != 0)
    return;
  const VolDesc vd{{cx, cy, cz}};
  xyz_inv_body<2, SG, false, kL2PosI, true>(vals, valsStride, cx, cy, cz, K, st, out + blockIdx.y * outStride, vd, nullptr, F, nseg,
                                            qrow, qslice);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------

int launch_xyz_inv(hipStream_t stream, dim3 grid, const double* vals, size_t valsStride, const uint32_t cdims[3],
                   const CoderState* st, int io, void* volume, VolDesc vd, const ChunkGeom* geom, const LiftFuse& F,
                   uint32_t nseg)
{
  const size_t smem = xyz_inv_smem(cdims[0], kXYZPosI);
  {
    const void* fns[4] = {reinterpret_cast<const void*>(&k_lift_xyz_inv<1, false>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, false>),
                          reinterpret_cast<const void*>(&k_lift_xyz_inv<1, true>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const LiftConsts K = lift_consts();
  const bool sg = F.mode == 2 && F.src.coefSigned != 0;
#define XYZ_INV_LAUNCH(io_, sg_)                                                                                    \
  LAUNCH_K((k_lift_xyz_inv<io_, sg_>), grid, dim3(kXYZThreadsI), smem, stream, vals, valsStride, cdims[0], cdims[1], \
           cdims[2], K, st, volume, vd, geom, F, nseg)
  if (io == 1) {
    if (sg)
      XYZ_INV_LAUNCH(1, true);
    else
      XYZ_INV_LAUNCH(1, false);
  }
  else {
    if (sg)
      XYZ_INV_LAUNCH(2, true);
    else
      XYZ_INV_LAUNCH(2, false);
  }
#undef XYZ_INV_LAUNCH
  HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_lift2_inv(hipStream_t stream, const double* box, size_t boxStride, double* out, size_t outStride,
                     uint32_t nchunks, const uint32_t cdims[3], const uint32_t region[3], const CoderState* st,
                     const LiftFuse* fuse)
{
  // (every sample outside fuse->inner comes from the coefficients: there is no fp64 copy of the region to read them from)
  if (!lift2_applicable(region) || !box || !out || !fuse || fuse->mode != 2 || region[0] > cdims[0] ||
      region[1] > cdims[1] || region[2] > cdims[2] || outStride < (size_t)region[0] * region[1] * region[2])
    return -1;
  LiftFuse F = *fuse;
  F.noMean = 1;
  const size_t smem = xyz_inv_smem(region[0], kL2PosI);
  if (set_max_dyn_lds(reinterpret_cast<const void*>(&k_lift2_inv<false>), 160 * 1024) ||
      set_max_dyn_lds(reinterpret_cast<const void*>(&k_lift2_inv<true>), 160 * 1024))
    return -1;
  const uint32_t ntile = (region[1] + kXYZRows - 1) / kXYZRows;
  const uint32_t nseg = lift2_segments(ntile, nchunks, region[2]);
  const dim3 grid(ntile * nseg, nchunks);
  const LiftConsts K = lift_consts();
  if (F.src.coefSigned != 0)
    LAUNCH_K((k_lift2_inv<true>), grid, dim3(kXYZThreadsI), smem, stream, box, boxStride, region[0], region[1], region[2], K,
             st, out, outStride, F, nseg, cdims[0], (size_t)cdims[0] * cdims[1]);
  else
    LAUNCH_K((k_lift2_inv<false>), grid, dim3(kXYZThreadsI), smem, stream, box, boxStride, region[0], region[1], region[2], K,
             st, out, outStride, F, nseg, cdims[0], (size_t)cdims[0] * cdims[1]);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace sperrhip
