// xform.h -- launchers of the floating-point stage kernels (conditioner and quantiser: xform.hip; lifting:
// lift_axis.hip, lift_xyz_fwd.hip, lift_xyz_inv.hip, lift_xyz_inv_crop.hip)
#ifndef SPERR_AMD_XFORM_H
#define SPERR_AMD_XFORM_H

#include <string.h>

#include "common.h"
#include "psnr_vol.h"

namespace sperrhip {

struct LiftConsts {
  double alpha, beta, gamma, delta, eps, inv_eps;
};
LiftConsts lift_consts();

template <typename T>
int launch_condition(hipStream_t stream, const T* vol, VolDesc vd, const ChunkGeom* geom,
                     uint32_t nchunks, const uint32_t cdims[3], uint32_t nstrides,
                     double* strideMean, size_t strideMeanStride, double* vals,
                     size_t valsStride, CoderState* st, bool gather, bool want_range = false,
                     bool org_x_aligned = false);   // every chunk's x origin is a multiple of 16 bytes

// crop (all the writers below): not null, the volume is a box of `vd`'s dims and every chunk writes
// its window of it (CropGeom, one per chunk); `geom` is not read then
template <typename T>
int launch_scatter(hipStream_t stream, T* vol, VolDesc vd, const ChunkGeom* geom,
                   uint32_t nchunks, const uint32_t cdims[3], const double* vals,
                   size_t valsStride, const CoderState* st, const CropGeom* crop = nullptr);

// What a lifting pass can do on the way for the samples of its region that no LATER pass (in
// forward order) touches, i.e. those outside `inner`, the region of the next pass:
//   forward (mode 1)  they have their final value: the largest magnitude goes to
//                     CoderState::maxabs (src/SPECK_FLT.cpp:282-301), no pass of its own;
//   inverse (mode 2)  they come straight from the decoder: the pass dequantises them from the
//                     integer coefficients while it loads (src/SPECK_FLT.cpp:373-399, with the
//                     decoder's masks completing the ones never refined), so no fp64 copy of the
//                     whole chunk is written and read again.  Chunks with 64-bit coefficients keep
//                     theirs in the fp64 buffer (converted in place beforehand) and are read as ever.
struct DecState;

// Where the integer coefficients of a batch's chunks are, for every kernel that makes samples of them (dequant.h):
// chunk c's arrays start c strides in
struct DequantSrc {
  // uint32_t magnitudes -- or, the 64-bit pass, uint64_t ones in the fp64 buffer that is converted in place: the
  // caller knows which (coefs<CT>)
  const void* coef = nullptr;
  size_t coefStride = 0;
  const uint64_t* sign = nullptr;     // a set bit: positive
  size_t signStride = 0;
  // the decoder's significance masks and state, to complete the coefficients that were never refined (the decoder
  // is told to skip its own finishing pass, DecPlanHost::skipFinish); all null: nothing to complete (the encoder's
  // reconstruction of its own coefficients)
  const uint64_t* sigNew = nullptr;
  const uint64_t* sigOld = nullptr;
  size_t maskStride = 0;
  const DecState* dst = nullptr;
  // 1: k_ref_assemble has written the coefficients complete (never-refined ones included) and, chunk by chunk where
  // coef_scheme(dst[c]) allows it, with the sign in bit 31 (dequant.h): the sign and mask words are not read at all then
  int coefSigned = 0;

  __host__ __device__ bool has_masks() const { return sigNew != nullptr && dst != nullptr; }
  template <typename CT>
  __host__ __device__ const CT* coefs(uint32_t c) const { return static_cast<const CT*>(coef) + c * coefStride; }
};

struct LiftFuse {
  int mode = 0;
  uint32_t inner[3] = {0, 0, 0};
  // mode 2.  (no_unique_address: noMean lies in the padding at src's end, as it did when src's fields were LiftFuse's own
  // -- k_lift_xyz_inv spills three to seven more scalar registers when the kernel's argument block is laid out otherwise)
  [[no_unique_address]] DequantSrc src;
  // k_lift_xyz_inv: do not add the chunk's mean to what it writes (the encoder's point-wise error stage compares in the
  // conditioned domain, src/SPECK_FLT.cpp:461-486)
  int noMean = 0;
  // inverse, compact chunk buffer (round 3): `vals` holds only the box the coarser levels work in,
  // rows of bufx samples and bufy rows per slice (0: the chunk's own dims); the coefficient and mask
  // arrays keep the chunk's dims
  uint32_t bufx = 0, bufy = 0;
};
static_assert(sizeof(LiftFuse) == 96 && __builtin_offsetof(LiftFuse, noMean) == 84, "the argument block of the lifting kernels");

// io: 0 in place; 1 / 2: the pass also reads (forward) or writes (inverse) the float / double
// volume through the chunk map -- only valid for a pass whose region is the whole chunk
int launch_lift(hipStream_t stream, bool forward, double* vals, size_t valsStride,
                uint32_t nchunks, const uint32_t cdims[3], int axis, const uint32_t region[3],
                CoderState* st, int io = 0, void* volume = nullptr, VolDesc vd = VolDesc{},
                const ChunkGeom* geom = nullptr, const LiftFuse* fuse = nullptr,
                const CropGeom* crop = nullptr);

// The x and y passes of the finest level fused with the volume access (forward: volume -> vals,
// inverse: vals -> volume); only for chunks whose first two passes are the full-size x and y ones.
bool lift_xy_applicable(const uint32_t cdims[3]);
int launch_lift_xy(hipStream_t stream, bool forward, double* vals, size_t valsStride,
                   uint32_t nchunks, const uint32_t cdims[3], const CoderState* st, int io,
                   void* volume, VolDesc vd, const ChunkGeom* geom, const CropGeom* crop = nullptr);

// The x, y AND z pass of the finest level in one kernel (k_lift_xyz_fwd / _inv): the z direction is
// a sliding window of per-position lifting pipelines in registers.  Forward: volume -> vals, with
// the largest magnitude collected when fuse->mode == 1; inverse: (coefficients dequantised on the
// way when fuse->mode == 2, never-refined ones completed from the decoder's masks: dequant.h) -> volume.  Only
// for chunks whose first three passes are the full-size x, y and z ones and whose rows fit.
bool lift_xyz_applicable(const uint32_t cdims[3]);
int launch_lift_xyz(hipStream_t stream, bool forward, double* vals, size_t valsStride, uint32_t nchunks,
                    const uint32_t cdims[3], CoderState* st, int io, void* volume, VolDesc vd,
                    const ChunkGeom* geom, const LiftFuse* fuse, const CropGeom* crop = nullptr,
                    double* box = nullptr, size_t boxStride = 0);

// The SECOND level's x, y and z pass in one launch of the same sliding-window code (k_lift2_fwd / k_lift2_inv), between
// compact boxes: a box holds `region` -- the finest level's low-low-low octant -- as rows of region[0] samples,
// region[1] rows a slice, chunk c's `boxStride` samples in.  Neither launch can work in place (a tile's outputs land in
// rows other tiles still read).
//   forward: launch_lift_xyz(..., box, boxStride) has written the octant into `box` instead of `vals`; this launch reads
//            it, nothing subtracted, and writes the corner of `vals` at the chunk's strides, collecting the largest
//            magnitude outside fuse->inner when fuse->mode == 1.
//   inverse: the samples inside fuse->inner come from `box` (rows of fuse->bufx samples), every other one from the
//            coefficients, addressed at the chunk's strides (fuse->mode == 2: dequant.h); the region goes to `out`, no
//            mean added, where launch_lift_xyz(inverse) takes it as its `vals` with fuse->bufx / bufy = region.
// Only for regions that pass lift_xyz_applicable and whose rows are at most 128 samples.
bool lift2_applicable(const uint32_t region[3]);
int launch_lift2_fwd(hipStream_t stream, const double* box, size_t boxStride, double* vals, size_t valsStride,
                     uint32_t nchunks, const uint32_t cdims[3], const uint32_t region[3], CoderState* st,
                     const LiftFuse* fuse);
int launch_lift2_inv(hipStream_t stream, const double* box, size_t boxStride, double* out, size_t outStride,
                     uint32_t nchunks, const uint32_t cdims[3], const uint32_t region[3], const CoderState* st,
                     const LiftFuse* fuse);

// have_max: CoderState::maxabs is already there (the lifting passes collected it)
int launch_maxabs_q(hipStream_t stream, const double* vals, size_t valsStride, uint32_t nchunks,
                    uint32_t n, CoderState* st, bool have_max = false);
int launch_make_q_wide(hipStream_t stream, uint32_t nchunks, CoderState* st);
int launch_mark_wide(hipStream_t stream, uint32_t nchunks, CoderState* st);

// PSNR mode: st[c].mse = quantisation error estimate of st[c].q for the chunks with mse_active set
// (partial: n / 4096 + 1 doubles per chunk)
int launch_mse(hipStream_t stream, const double* vals, size_t valsStride, uint32_t nchunks,
               uint32_t n, double* partial, size_t partialStride, CoderState* st);

// PSNR of the whole volume (psnr_vol.h): every chunk's q, mse, need_retry and refusal mark (CoderState::mse_active) from
// the common ladder L, on the device -- k_mse_ladder, then k_mse_ladder_pick.  partial: kPsnrRungs * rungStride doubles per
// chunk, rungStride at least n / 4096 + 1
int launch_mse_ladder(hipStream_t stream, const double* vals, size_t valsStride, uint32_t nchunks, uint32_t n,
                      double* partial, size_t rungStride, CoderState* st, const PsnrLadder& L);

// doubles as unsigned keys of the same order (the keys of a zeroed state are below every value)
__host__ __device__ inline unsigned long long order_key(double v)
{
  unsigned long long b;
  memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double order_key_value(unsigned long long k)
{
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &b, 8);
  return v;
}

int launch_quantize(hipStream_t stream, bool wide, const double* vals, size_t valsStride,
                    uint32_t nchunks, uint32_t n, void* coef, size_t coefStride, uint64_t* sign,
                    size_t signStride, int8_t* msb, size_t msbStride, const CoderState* st);

// every chunk with 32-bit (wide: 64-bit) coefficients, whole: src.coef holds magnitudes of that width, never packed
// words (src.coefSigned is not looked at)
int launch_inv_quantize(hipStream_t stream, bool wide, const DequantSrc& src, uint32_t nchunks, uint32_t n,
                        double* vals, size_t valsStride, const CoderState* st);

}  // namespace sperrhip

#endif
