// abi_stages.hip -- stage access for the parity tests: the entry points of include/sperr_hip.h that run ONE stage of
// the pipeline on the caller's data -- the transform, the integer coder each way, the outlier coder -- so that a test
// can compare it with the reference's stage alone.  Each leases an engine, takes the plan of the chunk shape and calls
// the stage's front (engine_core.h); the kernels that feed and drain a stage sit with it in encode.hip and decode.hip.
#include "engine_core.h"

using namespace sperrhip;

extern "C" {

int sperrhip_dwt3d_dev(double* d_vals, size_t dimx, size_t dimy, size_t dimz, int inverse,
                       void* hip_stream)
{
  return guarded("sperrhip_dwt3d_dev", [&]() -> int {
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    ShapePlan* P = E.plan(dimx, dimy, dimz);
    if (!P || E.misc.ensure(4096))
      return -1;
    CoderState* cst = static_cast<CoderState*>(E.misc.p);
    HIP_CHECK(hipMemsetAsync(cst, 0, sizeof(CoderState), st));
    const uint32_t cd[3] = {P->dims[0], P->dims[1], P->dims[2]};
    if (!inverse) {
      for (const LiftPass& ps : P->fwd)
        if (launch_lift(st, true, d_vals, P->N, 1, cd, ps.axis, ps.region, cst))
          return -1;
    }
    else {
      for (size_t k = P->fwd.size(); k-- > 0;)
        if (launch_lift(st, false, d_vals, P->N, 1, cd, P->fwd[k].axis, P->fwd[k].region, cst))
          return -1;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    E.prof.collect();
    return 0;
  });
}

int sperrhip_speck3d_encode_dev(const void* d_coef, int width, const uint64_t* d_sign, size_t dimx,
                                size_t dimy, size_t dimz, size_t budget_bits, void* d_dst,
                                size_t dst_cap, size_t* dst_len, void* hip_stream)
{
  return guarded("sperrhip_speck3d_encode_dev", [&]() -> int {
    if (width != 4 && width != 8)
      return 2;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    ShapePlan* P = E.plan(dimx, dimy, dimz);
    if (!P)
      return -1;
    return speck3d_encode_stage(E, st, *P, d_coef, width == 8, d_sign, budget_bits, static_cast<uint8_t*>(d_dst),
                                dst_cap, dst_len);
  });
}

int sperrhip_speck3d_plane_bits_dev(const void* d_coef, int width, const uint64_t* d_sign, size_t dimx, size_t dimy,
                                    size_t dimz, uint64_t* end, int* nbp, void* hip_stream)
{
  return guarded("sperrhip_speck3d_plane_bits_dev", [&]() -> int {
    // (refused: the 64-bit coefficient pass, and 2D slices -- the type-I set's bits are not in the table)
    if (width != 4 || !d_coef || !d_sign || !end || !nbp || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    ShapePlan* P = E.plan(dimx, dimy, dimz);
    if (!P)
      return -1;
    return speck3d_plane_bits_stage(E, st, *P, d_coef, d_sign, end, nbp);
  });
}

int sperrhip_outlier_encode_dev(const void* d_orig, int is_float, const double* d_recon, size_t dimx, size_t dimy,
                                size_t dimz, size_t nchunks, double tol, void* d_dst, size_t dst_cap, size_t* lens,
                                void* hip_stream)
{
  return guarded("sperrhip_outlier_encode_dev", [&]() -> int {
    if (!d_orig || !d_recon || !lens || !(tol > 0.0) || nchunks == 0 || dimx == 0 || dimy == 0 || dimz == 0)
      return 2;
    if (nchunks > 0xffffffffull / dimz)   // (a chunk's origin along z is a uint32)
      return 2;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    ShapePlan* P = E.plan(dimx, dimy, dimz);
    if (!P)
      return -1;
    return outlier_encode_stage(E, st, *P, d_orig, is_float, d_recon, (uint32_t)nchunks, tol,
                                static_cast<uint8_t*>(d_dst), dst_cap, lens);
  });
}

int sperrhip_speck3d_decode_dev(const void* d_stream, size_t stream_len, size_t dimx, size_t dimy,
                                size_t dimz, void* d_coef, uint64_t* d_sign, int* width_out,
                                void* hip_stream)
{
  return guarded("sperrhip_speck3d_decode_dev", [&]() -> int {
    if (stream_len < 9)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    ShapePlan* P = E.plan(dimx, dimy, dimz);
    if (!P)
      return -1;
    return speck3d_decode_stage(E, st, *P, d_stream, stream_len, d_coef, d_sign, width_out);
  });
}

}  // extern "C"
