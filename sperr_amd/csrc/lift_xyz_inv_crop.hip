// lift_xyz_inv_crop.hip -- the crop variants of the finest level's inverse three-pass lifting kernel,
// k_lift_xyz_inv<IO, SG, true> (lift_xyz_inv.h): a chunk's window of a decoded box.  The instantiations through the chunk
// map and the second level: lift_xyz_inv.hip.  Compile with -ffp-contract=off.
#include "lift_xyz_inv.h"

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------

int launch_xyz_inv_crop(hipStream_t stream, dim3 grid, const double* vals, size_t valsStride, const uint32_t cdims[3],
                        const CoderState* st, int io, void* volume, VolDesc vd, const CropGeom* crop, const LiftFuse& F,
                        uint32_t nseg)
{
  const size_t smem = xyz_inv_smem(cdims[0], kXYZPosI);
  {
    const void* fns[4] = {reinterpret_cast<const void*>(&k_lift_xyz_inv<1, false, true>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, false, true>),
                          reinterpret_cast<const void*>(&k_lift_xyz_inv<1, true, true>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, true, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const LiftConsts K = lift_consts();
  const bool sg = F.mode == 2 && F.src.coefSigned != 0;
#define XYZ_CROP_LAUNCH(io_, sg_)                                                                                   \
  LAUNCH_K((k_lift_xyz_inv<io_, sg_, true>), grid, dim3(kXYZThreadsI), smem, stream, vals, valsStride, cdims[0],      \
           cdims[1], cdims[2], K, st, volume, vd, crop, F, nseg)
  if (io == 1 && sg)
    XYZ_CROP_LAUNCH(1, true);
  else if (io == 1)
    XYZ_CROP_LAUNCH(1, false);
  else if (sg)
    XYZ_CROP_LAUNCH(2, true);
  else
    XYZ_CROP_LAUNCH(2, false);
#undef XYZ_CROP_LAUNCH
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace sperrhip
