// lift_xyz_fwd.hip -- the forward CDF 9/7 lifting DWT with the three passes of a level in one kernel, as HIP kernels
// for gfx950: the finest level straight from the volume (k_lift_xyz_fwd) and the second level between compact boxes
// (k_lift2_fwd); the rules for which shapes they serve, and launch_lift_xyz, whose inverse half calls into
// lift_xyz_inv.hip and lift_xyz_inv_crop.hip.  The sliding window and what both directions share: lift_xyz.h.
// Everything is fp64 with the reference's exact operation order; compile with -ffp-contract=off (SURVEY.md
// Appendix B).
//
// Reference behaviour restated (file:line of the reference):
//   src/CDF97.cpp:132-148,284-302,345-474,598-666   dyadic / wavelet-packet 3D transform (forward lifting: 598-631)
#include <type_traits>

#include "lift_xyz.h"

namespace sperrhip {

// The body of the forward kernels: one chunk's tile (and segment) of a workgroup.  `volc`: the chunk's samples, rows vsy
// and slices vsz apart, `mean` subtracted on the way in; `buf`: where the transformed chunk goes, rows `orow` and slices
// `sliceN` samples apart.  NPOS / NSTG: z pipelines / staged samples per thread (kXYZRows * cx <= NPOS * threads,
// kXYZStaged * cx <= NSTG * threads).
// `box` (not null: the finest level with the second level fused, k_lift2_fwd): the samples of the next level's box --
// low along x, y and z -- go there instead, rows of in0 samples and in1 rows a slice; L2: the second level itself, which has
// no box of its own.
template <typename VT, int NPOS, int NSTG, bool L2>
__device__ __forceinline__ void xyz_fwd_body(double* buf, const uint32_t orow, const size_t sliceN, uint32_t cx, uint32_t cy,
                                             uint32_t cz, const LiftConsts& K, CoderState* stc, const VT* volc, const size_t vsy,
                                             const size_t vsz, const double mean, int wantMax, uint32_t in0, uint32_t in1,
                                             uint32_t in2, uint32_t nseg, double* box)
{
  const uint32_t tid = threadIdx.x;
  // A small batch has too few tiles for the device: the slices are then dealt to `nseg` workgroups
  // per tile.  Segment g emits what the even slices 2m, m in [mA, mB), complete (the last one also
  // the end of the lines); a pipeline's output depends on the ten slices before it, so the segment
  // starts that much earlier and throws away what comes out before its own part.
  const uint32_t seg = blockIdx.x % nseg, npairsAll = (cz + 1) / 2;   // even slices 0, 2, ...: m < npairsAll
  const uint32_t mA = seg == 0 ? 0u : (uint32_t)((uint64_t)npairsAll * seg / nseg);
  const uint32_t mB = seg + 1 == nseg ? npairsAll : (uint32_t)((uint64_t)npairsAll * (seg + 1) / nseg);
  const uint32_t zFirst = mA >= 6 ? 2 * (mA - 6) : 0u;          // first slice this workgroup lifts
  const uint32_t zEnd = seg + 1 == nseg ? cz : 2 * mB - 1;       // one past its last slice
  const uint32_t y0 = (blockIdx.x / nseg) * kXYZRows;
  const uint32_t nt = min((uint32_t)kXYZRows, cy - y0);   // rows of this tile
  const uint32_t RS = xyz_row_stride(cx);
  // two staging buffers that swap roles from pass to pass (three barriers per slice instead of six);
  // (offsets, not an array of pointers: the compiler must see that these are LDS addresses)
  double* sm = reinterpret_cast<double*>(dyn_smem);
  const uint32_t bufN = (uint32_t)kXYZStaged * RS;
  const uint32_t xe = cx - cx / 2, ye = cy - cy / 2, ze = cz - cz / 2;
  const size_t boxSlice = (size_t)in0 * in1;

  // staging map: value k of this thread is sample x of LDS row j = row ysrc of the slice:
  // j << 27 | ysrc << 12 | x
  const uint32_t nstage = (uint32_t)kXYZStaged * cx;
  uint32_t pk[NSTG];
#pragma unroll
  for (int k = 0; k < NSTG; k++) {
    const uint32_t q = tid + (uint32_t)k * kXYZThreadsF;
    const uint32_t j = q / cx, x = q - j * cx;
    pk[k] = (j << 27) | (reflect_index((int)y0 - kXYHalo + (int)j, (int)cy) << 12) | x;
  }
  // z pipelines: position k of this thread is (row y0 + row, column col) of the tile
  const uint32_t npos = nt * cx;
  uint32_t srow[NPOS], ooff[NPOS];   // (LDS row << 16 | column), offset in a slice of the chunk buffer
  uint32_t boff[L2 ? 1 : NPOS];          // ... and in a slice of the box
  uint32_t outerMask = 0;   // bit k: position k lies outside the next level's box along x or y
#pragma unroll
  for (int k = 0; k < NPOS; k++) {
    const uint32_t q = tid + (uint32_t)k * kXYZThreadsF;
    const uint32_t row = q / cx, col = q - row * cx, y = y0 + row;
    srow[k] = ((row + kXYHalo) << 16) | col;
    const uint32_t drow = (y & 1) ? ye + (y >> 1) : (y >> 1), dcol = (col & 1) ? xe + (col >> 1) : (col >> 1);
    ooff[k] = drow * orow + dcol;
    if constexpr (!L2)
      boff[k] = drow * in0 + dcol;
    if (!(dcol < in0 && drow < in1))
      outerMask |= 1u << k;
  }
  double sxe[NPOS], sxo[NPOS], d1p[NPOS], e1p[NPOS], d2p[NPOS];
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    sxe[k] = sxo[k] = d1p[k] = e1p[k] = d2p[k] = 0.0;
  double vmax = 0.0;
  auto emit = [&](int k, uint32_t zp, double v) {   // sample (ooff, zp) of the transformed chunk
    bool toBox = false;
    if constexpr (!L2)
      toBox = box != nullptr && zp < in2 && !((outerMask >> k) & 1u);
    if (!xyz_off<XYZ_FWD_OFF>(4, nseg))   // (one store, its address chosen)
      *(toBox ? box + ((size_t)zp * boxSlice + boff[L2 ? 0 : k]) : buf + ((size_t)zp * sliceN + ooff[k])) = v;
    if (wantMax && (((outerMask >> k) & 1u) || zp >= in2))
      vmax = fmax(vmax, fabs(v));
  };

  VT pre[NSTG];
  auto issue = [&](uint32_t z) {
    const VT* src = volc + (size_t)z * vsz;
#pragma unroll
    for (int k = 0; k < NSTG; k++) {
      if (xyz_off<XYZ_FWD_OFF>(1, nseg)) {   // (noise instead of the volume: the coder gets something to code)
        pre[k] = (VT)(((pk[k] + z * 40503u) * 2654435761u) >> 20);
      }
      else {
        pre[k] = (tid + (uint32_t)k * kXYZThreadsF) < nstage
                     ? src[(size_t)((pk[k] >> 12) & 0x7fffu) * vsy + (pk[k] & 0xfffu)] : (VT)0;
      }
    }
  };
  issue(zFirst);
  for (uint32_t z = zFirst; z < zEnd; z++) {
    // (what the addresses below are made of goes through an empty asm once per slice: otherwise the
    //  compiler computes every one of them before the loop and keeps -- spills -- some 200 values)
    uint32_t RSv = RS, tidv = tid;
    asm volatile("" : "+s"(RSv), "+v"(tidv));
#pragma unroll
    for (int k = 0; k < NSTG; k++)
      asm volatile("" : "+v"(pk[k]));
#pragma unroll
    for (int k = 0; k < NPOS; k++)
      asm volatile("" : "+v"(srow[k]), "+v"(ooff[k]));
    if constexpr (!L2) {
#pragma unroll
      for (int k = 0; k < NPOS; k++)
        asm volatile("" : "+v"(boff[k]));
    }
    double* A = sm + ((z & 1) ? bufN : 0u);
    double* B = sm + ((z & 1) ? 0u : bufN);
#pragma unroll
    for (int k = 0; k < NSTG; k++)
      if ((tid + (uint32_t)k * kXYZThreadsF) < nstage)
        xyz_put(A + (pk[k] >> 27) * RSv, pk[k] & 0xfffu, cx, (double)pre[k] - mean);
    if (z + 1 < zEnd)
      issue(z + 1);   // (in flight while this slice is lifted)
    XYZ_LDS_BARRIER();
    if (!xyz_off<XYZ_FWD_OFF>(2, nseg))
      xyz_lift_x<true, kXYZThreadsF, kXYZOutFX>(A, B, RSv, cx, 0, kXYZStaged, tidv, K);
    XYZ_LDS_BARRIER();
    if (!xyz_off<XYZ_FWD_OFF>(2, nseg))
      xyz_lift_y<true, false, kXYZThreadsF, kXYZOutFY>(B, A, RSv, cx, nt, tidv, K);
    XYZ_LDS_BARRIER();   // (A's tile rows: this slice after x and y; the next slice is staged into B)
    const uint32_t m = z >> 1;
    if (xyz_off<XYZ_FWD_OFF>(8, nseg))
      continue;
    if (z & 1) {
#pragma unroll
      for (int k = 0; k < NPOS; k++)
        if ((tid + (uint32_t)k * kXYZThreadsF) < npos)
          sxo[k] = A[(srow[k] >> 16) * RSv + 4 + (srow[k] & 0xffffu)];
    }
    else {
#pragma unroll
      for (int k = 0; k < NPOS; k++) {
        if ((tid + (uint32_t)k * kXYZThreadsF) >= npos)
          continue;
        const double v = A[(srow[k] >> 16) * RSv + 4 + (srow[k] & 0xffffu)];
        if (m >= 1) {
          const double d1n = fma(K.alpha, sxe[k] + v, sxo[k]);                          // d1[2m-1]
          const double e1n = fma(K.beta, (m == 1 ? d1n : d1p[k]) + d1n, sxe[k]);        // e1[2m-2]
          if (m >= 2) {
            const double d2n = fma(K.gamma, e1p[k] + e1n, d1p[k]);                      // d2[2m-3]
            const double e2 = K.eps * fma(K.delta, (m == 2 ? d2n : d2p[k]) + d2n, e1p[k]);   // e2[2m-4]
            if (m >= mA) {   // (before that: the segment's run-up)
              emit(k, m - 2, e2);
              emit(k, ze + m - 2, (-K.inv_eps) * d2n);
            }
            d2p[k] = d2n;
          }
          d1p[k] = d1n;
          e1p[k] = e1n;
        }
        sxe[k] = v;
      }
    }
  }
  // ---- the end of the lines: the samples still in the pipelines (the last segment's to emit)
#pragma unroll
  for (int k = 0; k < NPOS; k++) {
    if ((tid + (uint32_t)k * kXYZThreadsF) >= npos || seg + 1 != nseg)
      continue;
    if ((cz & 1) == 0) {   // the last sample is odd: x[2M+1], M = cz / 2 - 1
      const uint32_t M = cz / 2 - 1;
      const double d1L = fma(K.alpha, sxe[k] + sxe[k], sxo[k]);          // d1[2M+1]
      const double e1M = fma(K.beta, d1p[k] + d1L, sxe[k]);              // e1[2M]
      const double d2a = fma(K.gamma, e1p[k] + e1M, d1p[k]);             // d2[2M-1]
      const double e2a = K.eps * fma(K.delta, d2p[k] + d2a, e1p[k]);     // e2[2M-2]
      const double d2L = fma(K.gamma, e1M + e1M, d1L);                   // d2[2M+1]
      const double e2L = K.eps * fma(K.delta, d2a + d2L, e1M);           // e2[2M]
      emit(k, M - 1, e2a);
      emit(k, ze + M - 1, (-K.inv_eps) * d2a);
      emit(k, M, e2L);
      emit(k, ze + M, (-K.inv_eps) * d2L);
    }
    else {                 // the last sample is even: x[2M], M = cz / 2 (its slice went through the loop)
      const uint32_t M = cz / 2;
      const double e1M = fma(K.beta, d1p[k] + d1p[k], sxe[k]);           // e1[2M]
      const double d2a = fma(K.gamma, e1p[k] + e1M, d1p[k]);             // d2[2M-1]
      const double e2a = K.eps * fma(K.delta, d2p[k] + d2a, e1p[k]);     // e2[2M-2]
      const double e2L = K.eps * fma(K.delta, d2a + d2a, e1M);           // e2[2M]
      emit(k, M - 1, e2a);
      emit(k, ze + M - 1, (-K.inv_eps) * d2a);
      emit(k, M, e2L);
    }
  }
  if (wantMax) {
    for (int d = 32; d > 0; d >>= 1)
      vmax = fmax(vmax, __shfl_xor(vmax, d, 64));
    if ((tid & 63) == 0 && vmax > 0.0)
      atomicMax(reinterpret_cast<unsigned long long*>(&stc->maxabs),
                (unsigned long long)__double_as_longlong(vmax));
  }
}

// box (not null): the next level's box goes there, chunk c's boxStride samples in, and not to `vals` (xyz_fwd_body)
template <int IO>
__global__ void __launch_bounds__(kXYZThreadsF) __attribute__((amdgpu_waves_per_eu(kXYZThreadsF / 256, kXYZThreadsF / 256)))
k_lift_xyz_fwd(double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz, LiftConsts K,
               CoderState* st, const void* volume, VolDesc vd, const ChunkGeom* geom, int wantMax,
               uint32_t in0, uint32_t in1, uint32_t in2, uint32_t nseg, double* box, size_t boxStride)
{
  static_assert(IO == 1 || IO == 2, "float or double volume");
  using VT = typename std::conditional<IO == 1, float, double>::type;
  const uint32_t c = blockIdx.y;
  if (st[c].is_const != 0)
    return;
  const VT* vol = reinterpret_cast<const VT*>(volume);
  const size_t vsy = vd.dims[0], vsz = (size_t)vd.dims[0] * vd.dims[1];
  const VT* volc = vol + ((size_t)geom[c].org[2] * vsz + (size_t)geom[c].org[1] * vsy + geom[c].org[0]);
  xyz_fwd_body<VT, kXYZPosF, kXYZStageF, false>(vals + c * valsStride, cx, (size_t)cx * cy, cx, cy, cz, K, st + c, volc, vsy, vsz,
                                                 st[c].mean, wantMax, in0, in1, in2, nseg, box ? box + c * boxStride : nullptr);
}

// The SECOND level's three passes in one launch of the same sliding-window code: the box the finest-level kernel
// has written (rows of cx samples, cy rows a slice: read like a volume of doubles, nothing subtracted) -> the corner of
// the chunk buffer, at the chunk's strides `orow` / `oslice`.  Rows of at most 128 samples: half the z pipelines per
// thread, and no scratch.
__global__ void __launch_bounds__(kXYZThreadsF) __attribute__((amdgpu_waves_per_eu(kXYZThreadsF / 256, kXYZThreadsF / 256)))
k_lift2_fwd(const double* box, size_t boxStride, double* vals, size_t valsStride, uint32_t orow, size_t oslice, uint32_t cx,
            uint32_t cy, uint32_t cz, LiftConsts K, CoderState* st, int wantMax, uint32_t in0, uint32_t in1, uint32_t in2,
            uint32_t nseg)
{
  const uint32_t c = blockIdx.y;
  if (st[c].is_const != 0)
    return;
  xyz_fwd_body<double, kL2PosF, kL2StageF, true>(vals + c * valsStride, orow, oslice, cx, cy, cz, K, st + c, box + c * boxStride,
                                                  (size_t)cx, (size_t)cx * cy, 0.0, wantMax, in0, in1, in2, nseg, nullptr);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------

bool lift_xyz_applicable(const uint32_t cdims[3])
{
  if (cdims[0] < 9 || cdims[1] < 9 || cdims[2] < 9)
    return false;
  // a thread's z pipelines are registers: (rows + halo) * cx positions over the workgroup's threads
  // (and the packed staging map holds 12 bits of x, 15 bits of y)
  return (size_t)kXYZStaged * cdims[0] <= (size_t)kXYZPosI * kXYZThreadsI &&
         (size_t)kXYZStaged * cdims[0] <= (size_t)kXYZStageF * kXYZThreadsF &&
         (size_t)kXYZRows * cdims[0] <= (size_t)kXYZPosF * kXYZThreadsF && cdims[0] < 4096 && cdims[1] < 32768;
}

// a batch with fewer tiles than two per CU: the slices of a tile are dealt to several workgroups
uint32_t xyz_segments(uint32_t ntile, uint32_t nchunks, uint32_t cz)
{
  uint32_t nseg = 1;
  while (nseg < 4 && (size_t)ntile * nchunks * nseg < 512 && cz / (2 * nseg) >= 24)
    nseg *= 2;
  return nseg;
}

int launch_lift_xyz(hipStream_t stream, bool forward, double* vals, size_t valsStride, uint32_t nchunks,
                    const uint32_t cdims[3], CoderState* st, int io, void* volume, VolDesc vd,
                    const ChunkGeom* geom, const LiftFuse* fuse, const CropGeom* crop, double* box, size_t boxStride)
{
  if (!lift_xyz_applicable(cdims) || (io != 1 && io != 2) || (crop && forward))
    return -1;
  if (box && !forward)
    return -1;
  const LiftFuse F = fuse ? *fuse : LiftFuse{};
  const uint32_t ntile = (cdims[1] + kXYZRows - 1) / kXYZRows;
  const uint32_t nseg = xyz_segments(ntile, nchunks, cdims[2]);
  const dim3 grid(ntile * nseg, nchunks);
  if (!forward)   // (the inverse kernels are other units': lift_xyz.h)
    return crop ? launch_xyz_inv_crop(stream, grid, vals, valsStride, cdims, st, io, volume, vd, crop, F, nseg)
                : launch_xyz_inv(stream, grid, vals, valsStride, cdims, st, io, volume, vd, geom, F, nseg);
  const size_t smem = 2 * (size_t)kXYZStaged * xyz_row_stride(cdims[0]) * sizeof(double);   // two staging buffers
  {
    const void* fns[2] = {reinterpret_cast<const void*>(&k_lift_xyz_fwd<1>), reinterpret_cast<const void*>(&k_lift_xyz_fwd<2>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const LiftConsts K = lift_consts();
  const int wantMax = F.mode == 1 ? 1 : 0;
  if (io == 1)
    LAUNCH_K((k_lift_xyz_fwd<1>), grid, dim3(kXYZThreadsF), smem, stream, vals, valsStride, cdims[0], cdims[1],
             cdims[2], K, st, volume, vd, geom, wantMax, F.inner[0], F.inner[1], F.inner[2], nseg, box, boxStride);
  else
    LAUNCH_K((k_lift_xyz_fwd<2>), grid, dim3(kXYZThreadsF), smem, stream, vals, valsStride, cdims[0], cdims[1],
             cdims[2], K, st, volume, vd, geom, wantMax, F.inner[0], F.inner[1], F.inner[2], nseg, box, boxStride);
  HIP_CHECK(hipGetLastError());
  return 0;
}

bool lift2_applicable(const uint32_t region[3])
{
  return lift_xyz_applicable(region) && region[0] <= (uint32_t)kL2MaxRow;
}

// segments per tile of a level-2 launch (SPERR_HIP_L2_NSEG, diagnostics build: 1, 2 or 4 whatever the rule says)
uint32_t lift2_segments(uint32_t ntile, uint32_t nchunks, uint32_t cz)
{
  static const int forced = tune_getenv("SPERR_HIP_L2_NSEG") ? atoi(tune_getenv("SPERR_HIP_L2_NSEG")) : 0;
  if ((forced == 1 || forced == 2 || forced == 4) && cz / (2 * (uint32_t)forced) >= 8)
    return (uint32_t)forced;
  return xyz_segments(ntile, nchunks, cz);
}

int launch_lift2_fwd(hipStream_t stream, const double* box, size_t boxStride, double* vals, size_t valsStride,
                     uint32_t nchunks, const uint32_t cdims[3], const uint32_t region[3], CoderState* st,
                     const LiftFuse* fuse)
{
  if (!lift2_applicable(region) || !box || region[0] > cdims[0] || region[1] > cdims[1] || region[2] > cdims[2])
    return -1;
  const LiftFuse F = fuse ? *fuse : LiftFuse{};
  const size_t smem = 2 * (size_t)kXYZStaged * xyz_row_stride(region[0]) * sizeof(double);   // two staging buffers
  if (set_max_dyn_lds(reinterpret_cast<const void*>(&k_lift2_fwd), 160 * 1024))
    return -1;
  const uint32_t ntile = (region[1] + kXYZRows - 1) / kXYZRows;
  const uint32_t nseg = lift2_segments(ntile, nchunks, region[2]);
  LAUNCH_K(k_lift2_fwd, dim3(ntile * nseg, nchunks), dim3(kXYZThreadsF), smem, stream, box, boxStride, vals, valsStride,
           cdims[0], (size_t)cdims[0] * cdims[1], region[0], region[1], region[2], lift_consts(), st, F.mode == 1 ? 1 : 0,
           F.inner[0], F.inner[1], F.inner[2], nseg);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace sperrhip

