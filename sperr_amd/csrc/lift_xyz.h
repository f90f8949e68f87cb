// lift_xyz.h -- what the fused three-pass lifting kernels share, forward (lift_xyz_fwd.hip: k_lift_xyz_fwd, k_lift2_fwd)
// and inverse (lift_xyz_inv.hip, lift_xyz_inv_crop.hip: k_lift_xyz_inv, k_lift2_inv): the compile-time switches, the
// tile's constants and LDS layout, the x and y passes of a staged slice, and the functions one of these units calls in
// another.
#ifndef SPERR_AMD_LIFT_XYZ_H
#define SPERR_AMD_LIFT_XYZ_H

#include "xform.h"
#include "lift_dev.h"
#include "lift_window.h"

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// The THREE passes of the finest level fused with the volume access (round 3): the z pass joins
// k_lift_xy's x and y passes, so the fp64 chunk buffer is written once (forward) / the integer
// coefficients are read once (inverse) instead of a 16-byte-per-sample round trip through HBM for
// the z pass alone.  A brick that is whole along all three axes is the chunk, so the z direction
// is a SLIDING WINDOW: a workgroup owns kXYZRows rows (all of x) and marches through the slices;
// every slice is staged with a halo of four rows, x- and y-lifted in LDS exactly as in k_lift_xy,
// and its samples then enter per-position lifting PIPELINES along z held in registers.
//
// The four lifting steps along z as a pipeline (forward; x = input, d = odd, e = even samples):
//     d1[2m-1] = x[2m-1] + a (x[2m-2] + x[2m])         known when slice 2m arrives
//     e1[2m-2] = x[2m-2] + b (d1[2m-3] + d1[2m-1])
//     d2[2m-3] = d1[2m-3] + g (e1[2m-4] + e1[2m-2])    -> high[m-2] = -1/eps d2[2m-3]
//     e2[2m-4] = eps (e1[2m-4] + d (d2[2m-5] + d2[2m-3]))   -> low[m-2]
// so five values per position (x[2m], x[2m+1], d1[2m-1], e1[2m-2], d2[2m-3]) carry everything;
// the ends follow the reference's clamped indices (src/CDF97.cpp:598-666: a = max(i,1)-1,
// b = min(i, odd_len-1), r = min(i+1, even_len-1)), written out below.  Every sample goes through
// the very same operations, in the same order, as in k_lift_axis: bit-identical.
// The inverse runs the mirror image: pairs (low[m], high[m]) enter, four values per position stay
// (o1[m], e1[m], o2[m-1], e2[m-1]), slices 2m-3 and 2m-2 leave and go through the y and x passes.
// ------------------------------------------------------------------------------------------
// (the pipelines live in registers: the forward kernel fits 16 wavefronts of 128 VGPRs, the inverse one,
//  which inverts the halo rows along z too, as well -- with a few spills outside its main loop)
#ifndef XYZ_INV_THREADS
#define XYZ_INV_THREADS 1024
#endif
#ifndef XYZ_INV_PREFETCH
#define XYZ_INV_PREFETCH 2   // 0: the loads of rounds 1-3 (kept for A/B builds, tools/build_variant.sh)
#endif
#ifndef XYZ_FWD_THREADS
#define XYZ_FWD_THREADS 1024
#endif
constexpr int kXYZThreadsF = XYZ_FWD_THREADS, kXYZThreadsI = XYZ_INV_THREADS;
constexpr int kXYZRows = 16;
constexpr int kXYZStaged = kXYZRows + 2 * kXYHalo;   // LDS rows of a slice
constexpr int kXYZPosF = (4096 + kXYZThreadsF - 1) / kXYZThreadsF;    // z pipelines per thread, forward: kXYZRows * cx <= 4096
constexpr int kXYZStageF = (6144 + kXYZThreadsF - 1) / kXYZThreadsF;  // staged samples per thread, forward: kXYZStaged * cx <= 6144
constexpr int kXYZPosI = 6144 / kXYZThreadsI;   // inverse: kXYZStaged * cx <= 6144
#ifndef XYZ_INV_GROUP
#define XYZ_INV_GROUP 3
#endif
constexpr int kXYZGroupI = XYZ_INV_GROUP;       // positions whose loads are in flight together
// samples a task of the y / x pass produces (window: that + 8), forward and inverse; A/B builds: tools/build_variant.sh
#ifndef XYZ_FWD_YOUT
#define XYZ_FWD_YOUT 4
#endif
#ifndef XYZ_FWD_XOUT
#define XYZ_FWD_XOUT 8
#endif
#ifndef XYZ_INV_YOUT
#define XYZ_INV_YOUT 4
#endif
#ifndef XYZ_INV_XOUT
#define XYZ_INV_XOUT 4
#endif
#ifndef XYZ_INV_XSTORE
#define XYZ_INV_XSTORE 1   // the inverse kernel's x pass writes the volume itself (0: back into LDS, rows stored from there)
#endif
// Timing only (tools/build_variant.sh; the results of such a build are wrong): parts of the two kernels switched off,
// a sum of 1: global loads, 2: y and x passes, 4: global stores, 8: z pipelines -- 15 leaves staging and barriers.
#ifndef XYZ_FWD_OFF
#define XYZ_FWD_OFF 0
#endif
#ifndef XYZ_INV_OFF
#define XYZ_INV_OFF 0
#endif
// part `bit` of a kernel is switched off.  A timing build asks a value of the launch as well, one that never has the
// value asked for: what feeds the part stays needed and the rest of the kernel stays what it was.  Folds to false
// in the product's build.
template <int MASK>
__device__ __forceinline__ bool xyz_off(int bit, uint32_t nseg)
{
  return (MASK & bit) != 0 && nseg != ~0u;
}
constexpr int kXYZOutFY = XYZ_FWD_YOUT, kXYZOutFX = XYZ_FWD_XOUT, kXYZOutIY = XYZ_INV_YOUT, kXYZOutIX = XYZ_INV_XOUT;
constexpr bool xyz_out_ok(int n) { return n == 2 || n == 4 || n == 8; }   // (a row's and a tile's last window stays inside the aprons)
static_assert(xyz_out_ok(kXYZOutFY) && xyz_out_ok(kXYZOutFX) && xyz_out_ok(kXYZOutIY) && xyz_out_ok(kXYZOutIX), "2, 4 or 8 outputs a task");
constexpr int kXYZBoxSlots = 48;                // inverse, sign-in-word kernel: 256-byte rows of box samples on their way in (12 rows x 4)

// LDS layout of a slice: kXYZStaged rows; row r holds row reflect_index(y0 - 4 + r, cy) of the slice
// (the four rows above and below the tile -- mirrored at the ends of the slice, so the first and the
// last tile need nothing special), each row as [4 mirrored samples | cx samples | 4 mirrored samples]:
// lift16 then never has to reflect an index along x or y.
__host__ __device__ inline uint32_t xyz_row_stride(uint32_t cx)
{
  return ((cx + 7u) & ~7u) + 9u;   // (odd: rows start in different banks)
}

// A workgroup barrier that waits for the LDS traffic only.  __syncthreads() also waits for every global
// load and store in flight (s_waitcnt vmcnt(0)): here those are the NEXT slice's samples on their way
// in and the last slice's results on their way out, which no other thread of the workgroup looks at.
#define XYZ_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// sample x of LDS row `row`, with its mirror images in the row's apron
__device__ __forceinline__ void xyz_put(double* row, uint32_t x, uint32_t cx, double v)
{
  row[4 + x] = v;
  if (x - 1u < 4u)
    row[4 - x] = v;
  if (cx - 2u - x < 4u)
    row[2 * cx + 2 - x] = v;   // 4 + (cx - 1) + ((cx - 1) - x)
}

// x pass: rows [jlo, jhi) of `src` (aprons filled) -> the same rows of `dst` (another buffer: no barrier
// inside); a task produces NOUT samples of a row
template <bool FORWARD, int NT, int NOUT>
__device__ __forceinline__ void xyz_lift_x(const double* src, double* dst, uint32_t RS, uint32_t cx, uint32_t jlo,
                                           uint32_t jhi, uint32_t tid, const LiftConsts& K)
{
  const uint32_t nseg = (cx + NOUT - 1) / NOUT;
  const uint32_t ntask = (jhi - jlo) * nseg;
#pragma unroll 1
  for (uint32_t t = tid; t < ntask; t += NT) {
    // lanes of a wavefront take different rows: their addresses differ by the (odd) row stride
    const uint32_t rows = jhi - jlo, sg = t / rows, rb = jlo + (t - sg * rows);
    const double* row = src + (size_t)rb * RS + sg * NOUT;
    double r[NOUT + 8];
#pragma unroll
    for (int k = 0; k < NOUT + 8; k++)
      r[k] = row[k];
    lift_window<FORWARD, NOUT + 8>(r, K);
    double* out = dst + (size_t)rb * RS + 4 + sg * NOUT;
#pragma unroll
    for (int k = 0; k < NOUT; k++)
      if (sg * NOUT + k < cx)
        out[k] = r[4 + k];
  }
}

// the inverse kernel's x pass with the volume as its destination: row rb of `src` is row rb - jlo of `vrows` (rows `vsy`
// samples apart); what a task produces goes out as it is -- mean added, narrowed -- without another trip through LDS
template <int NT, int NOUT, typename VT>
__device__ __forceinline__ void xyz_lift_x_store(const double* src, VT* vrows, size_t vsy, uint32_t RS, uint32_t cx, uint32_t jlo,
                                                 uint32_t jhi, uint32_t tid, const LiftConsts& K, double mean, bool noMean,
                                                 bool doStore)
{
  const uint32_t nseg = (cx + NOUT - 1) / NOUT;
  const uint32_t ntask = (jhi - jlo) * nseg;
#pragma unroll 1
  for (uint32_t t = tid; t < ntask; t += NT) {
    const uint32_t rows = jhi - jlo, sg = t / rows, rb = t - sg * rows;   // (lanes take different rows, see xyz_lift_x)
    const double* row = src + (size_t)(jlo + rb) * RS + sg * NOUT;
    double r[NOUT + 8];
#pragma unroll
    for (int k = 0; k < NOUT + 8; k++)
      r[k] = row[k];
    lift_window<false, NOUT + 8>(r, K);
    VT* out = vrows + (size_t)rb * vsy + sg * NOUT;
    VT v[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; k++)
      v[k] = (VT)(noMean ? r[4 + k] : r[4 + k] + mean);
    if (!doStore)
      continue;
    if (sg * NOUT + NOUT <= cx) {   // (a whole segment: one store, aligned as a single sample is)
      typedef VT Seg __attribute__((ext_vector_type(NOUT), aligned(sizeof(VT))));
      Seg s;
#pragma unroll
      for (int k = 0; k < NOUT; k++)
        s[k] = v[k];
      *reinterpret_cast<Seg*>(out) = s;
    }
    else {
#pragma unroll
      for (int k = 0; k < NOUT; k++)
        if (sg * NOUT + k < cx)
          out[k] = v[k];
    }
  }
}

// y pass: tile rows (LDS rows 4 .. 4 + nt) of `src` -> the same rows of `dst`; a task produces NOUT samples of a column
template <bool FORWARD, bool APRON, int NT, int NOUT>
__device__ __forceinline__ void xyz_lift_y(const double* src, double* dst, uint32_t RS, uint32_t cx, uint32_t nt,
                                           uint32_t tid, const LiftConsts& K)
{
  const uint32_t nq = (nt + NOUT - 1) / NOUT;
  const uint32_t ntask = nq * cx;
#pragma unroll 1
  for (uint32_t t = tid; t < ntask; t += NT) {
    const uint32_t q = t / cx, x = t - q * cx;   // lanes take consecutive columns
    const double* top = src + (size_t)(q * NOUT) * RS + 4 + x;
    double r[NOUT + 8];
#pragma unroll
    for (int k = 0; k < NOUT + 8; k++)
      r[k] = top[(size_t)k * RS];
    lift_window<FORWARD, NOUT + 8>(r, K);
#pragma unroll
    for (int k = 0; k < NOUT; k++) {
      if (q * NOUT + k < nt) {
        double* row = dst + (size_t)(4 + q * NOUT + k) * RS;
        if (APRON)
          xyz_put(row, x, cx, r[4 + k]);
        else
          row[4 + x] = r[4 + k];
      }
    }
  }
}

// the second level's kernels (k_lift2_fwd, k_lift2_inv): rows of at most kL2MaxRow samples, so half the z pipelines
// per thread
constexpr int kL2MaxRow = 128;
constexpr int kL2PosF = (kXYZRows * kL2MaxRow + kXYZThreadsF - 1) / kXYZThreadsF;
constexpr int kL2StageF = (kXYZStaged * kL2MaxRow + kXYZThreadsF - 1) / kXYZThreadsF;
constexpr int kL2PosI = (kXYZStaged * kL2MaxRow + kXYZThreadsI - 1) / kXYZThreadsI;

// ------------------------------------------------------------------------------------------
// host side: what one of the units' launchers calls in another (a kernel is launched only from the unit that
// defines it)
// ------------------------------------------------------------------------------------------

// segments per tile of a launch (lift_xyz_fwd.hip)
uint32_t xyz_segments(uint32_t ntile, uint32_t nchunks, uint32_t cz);
uint32_t lift2_segments(uint32_t ntile, uint32_t nchunks, uint32_t cz);

// dynamic LDS of an inverse kernel with rows of cx samples and NPOS = npos positions per thread
inline size_t xyz_inv_smem(uint32_t cx, int npos)
{
  size_t smem = 2 * (size_t)kXYZStaged * xyz_row_stride(cx) * sizeof(double);   // two staging buffers
#if XYZ_INV_PREFETCH == 2
  smem += (size_t)kXYZThreadsI * npos * 2 * sizeof(uint32_t) +   // + the coefficients on their way in
          (size_t)kXYZBoxSlots * 64 * sizeof(uint32_t);          //   and the box samples (k_lift_xyz_inv<.., true>)
#endif
  return smem;
}

// The inverse half of launch_lift_xyz (lift_xyz_fwd.hip), which has checked the arguments and made the grid:
// k_lift_xyz_inv<io, sg> through the chunk map (lift_xyz_inv.hip), k_lift_xyz_inv<io, sg, true> into the chunks'
// windows of a box (lift_xyz_inv_crop.hip)
int launch_xyz_inv(hipStream_t stream, dim3 grid, const double* vals, size_t valsStride, const uint32_t cdims[3],
                   const CoderState* st, int io, void* volume, VolDesc vd, const ChunkGeom* geom, const LiftFuse& F,
                   uint32_t nseg);
int launch_xyz_inv_crop(hipStream_t stream, dim3 grid, const double* vals, size_t valsStride, const uint32_t cdims[3],
                        const CoderState* st, int io, void* volume, VolDesc vd, const CropGeom* crop, const LiftFuse& F,
                        uint32_t nseg);

}  // namespace sperrhip

#endif
