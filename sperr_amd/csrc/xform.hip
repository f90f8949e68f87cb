// xform.hip -- floating-point stages of the chunk pipeline as HIP kernels for gfx950:
// conditioner (mean / constant test), max-reduce, mid-tread quantiser and its inverse, chunk
// gather/scatter.  (The CDF 9/7 lifting DWT and IDWT: lift_axis.hip, lift_xyz_fwd.hip,
// lift_xyz_inv.hip, lift_xyz_inv_crop.hip.)  Everything is fp64 with the reference's exact
// operation order; compile with -ffp-contract=off (every fused multiply-add of the canonical
// reference build is an explicit fma()).
//
// Reference behaviour restated (file:line under /root/reference):
//   src/Conditioner.cpp:10-64,119-163   strided sequential mean, constant test
//   src/SPECK_FLT.cpp:282-301,311-399   q, quantise, inverse quantise
//   src/SPERR3D_OMP_C.cpp:236-261, src/SPERR3D_OMP_D.cpp:167-184   gather / scatter
#include "xform.h"
#include "lift_dev.h"
#include "dequant.h"
#include "psnr_vol.h"

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// conditioner
// ------------------------------------------------------------------------------------------

// Strided mean (src/Conditioner.cpp:119-135): every stride is summed strictly sequentially in fp64
// (the order is part of the result), so one thread owns one stride -- but reading a stride per
// thread straight from HBM touches a different cache line per lane.  A workgroup therefore takes
// kSumStrides strides and stages them segment by segment through LDS: all threads load
// kSumStrides x kSumSeg samples with coalesced row reads through the chunk's gather map, then
// kSumStrides threads add their row of the tile in order.  Also tests "all samples equal".
constexpr int kSumStrides = 64, kSumSeg = 64;


template <typename T>
__global__ void __launch_bounds__(kThreads)
k_stride_sums(const T* __restrict__ vol, VolDesc vd, const ChunkGeom* geom, uint32_t cx,
              uint32_t cy, uint32_t cz, uint32_t nstrides, uint32_t ssz, double* strideMean,
              size_t strideMeanStride, CoderState* st, int want_range)
{
  __shared__ double tile[kSumStrides][kSumSeg + 1];
  __shared__ uint32_t sh_differs;
  double vmax = -INFINITY, vnegmax = -INFINITY;   // (PSNR mode) range of the chunk's samples
  const uint32_t c = blockIdx.y;
  const uint32_t s0 = blockIdx.x * kSumStrides;
  const ChunkGeom g = geom[c];
  const size_t vx = vd.dims[0], vy = vd.dims[1];
  const T first = vol[((size_t)g.org[2] * vy + g.org[1]) * vx + g.org[0]];
  if (threadIdx.x == 0)
    sh_differs = 0;
  double acc = 0.0;
  bool differs = false;
  (void)cz;
  for (uint32_t seg = 0; seg < ssz; seg += kSumSeg) {
    const uint32_t len = min((uint32_t)kSumSeg, ssz - seg);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)(kSumStrides * kSumSeg); k += kThreads) {
      const uint32_t r = k / kSumSeg, j = k % kSumSeg;
      const uint32_t sidx = s0 + r;
      if (sidx < nstrides && j < len) {
        const uint32_t e = sidx * ssz + seg + j;      // sample index inside the chunk
        const uint32_t x = e % cx, q = e / cx;
        const uint32_t y = q % cy, z = q / cy;
        const T v = vol[((size_t)(g.org[2] + z) * vy + (g.org[1] + y)) * vx + g.org[0] + x];
        differs |= (v != first);
        tile[r][j] = (double)v;
        vmax = fmax(vmax, (double)v);
        vnegmax = fmax(vnegmax, -(double)v);
      }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kSumStrides && s0 + threadIdx.x < nstrides)
      for (uint32_t j = 0; j < len; j++)
        acc += tile[threadIdx.x][j];
  }
  if (differs)
    sh_differs = 1;
  __syncthreads();
  if (threadIdx.x < (uint32_t)kSumStrides && s0 + threadIdx.x < nstrides)
    strideMean[c * strideMeanStride + s0 + threadIdx.x] = acc / (double)ssz;
  if (threadIdx.x == 0 && sh_differs)
    st[c].not_const_flag = 1;
  if (want_range) {
    for (int d = 32; d > 0; d >>= 1) {
      vmax = fmax(vmax, __shfl_xor(vmax, d, 64));
      vnegmax = fmax(vnegmax, __shfl_xor(vnegmax, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].vmaxKey), order_key(vmax));
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].vnegmaxKey), order_key(vnegmax));
    }
  }
}

// The same sums when a stride is a whole number of chunk rows (every power-of-two chunk): one
// thread per stride streams its rows with 16-byte loads, several in flight, and adds them in
// order.  Eight wavefronts per CU keep enough bytes in flight to follow HBM.
template <typename T>
__global__ void __launch_bounds__(64)
k_stride_sums_rows(const T* __restrict__ vol, VolDesc vd, const ChunkGeom* geom, uint32_t cx,
                   uint32_t cy, uint32_t nstrides, uint32_t ssz, double* strideMean,
                   size_t strideMeanStride, CoderState* st, int want_range)
{
  constexpr int V = 16 / sizeof(T);                 // samples per 16-byte load
  struct alignas(16) Pack { T v[V]; };
  const uint32_t c = blockIdx.y;
  const uint32_t sidx = blockIdx.x * 64 + threadIdx.x;
  const ChunkGeom g = geom[c];
  const size_t vx = vd.dims[0], vy = vd.dims[1];
  const T first = vol[((size_t)g.org[2] * vy + g.org[1]) * vx + g.org[0]];
  double acc = 0.0, vmax = -INFINITY, vnegmax = -INFINITY;
  bool differs = false;
  if (sidx < nstrides) {
    const uint32_t rows = ssz / cx, row0 = sidx * rows;   // chunk rows of this stride
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t y = (row0 + r) % cy, z = (row0 + r) / cy;
      const T* src = vol + ((size_t)(g.org[2] + z) * vy + (g.org[1] + y)) * vx + g.org[0];
      for (uint32_t x = 0; x < cx; x += 8 * V) {
        Pack pk[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
          pk[k] = *reinterpret_cast<const Pack*>(src + x + k * V);
#pragma unroll
        for (int k = 0; k < 8; k++)
#pragma unroll
          for (int e = 0; e < V; e++) {
            const T v = pk[k].v[e];
            differs |= (v != first);
            acc += (double)v;
            vmax = fmax(vmax, (double)v);
            vnegmax = fmax(vnegmax, -(double)v);
          }
      }
    }
    strideMean[c * strideMeanStride + sidx] = acc / (double)ssz;
  }
  if (__any(differs) && threadIdx.x == 0)
    st[c].not_const_flag = 1;
  if (want_range) {
    for (int d = 32; d > 0; d >>= 1) {
      vmax = fmax(vmax, __shfl_xor(vmax, d, 64));
      vnegmax = fmax(vnegmax, __shfl_xor(vnegmax, d, 64));
    }
    if (threadIdx.x == 0) {
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].vmaxKey), order_key(vmax));
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].vnegmaxKey), order_key(vnegmax));
    }
  }
}

// The stride means added up in the reference's order (src/Conditioner.cpp:137-163): one thread does the
// additions, but out of LDS, where the workgroup has put the means with coalesced loads (round 3: one
// thread reading them from global memory one dependent load at a time took 0.44 ms for 2048 strides,
// on the critical path of every compression call)
constexpr int kMeanStage = 2048;
template <typename T>
__global__ void __launch_bounds__(kThreads)
k_mean_finalize(const T* __restrict__ vol, VolDesc vd, const ChunkGeom* geom, uint32_t nstrides,
                const double* strideMean, size_t strideMeanStride, CoderState* st)
{
  __shared__ double stage[kMeanStage];
  const uint32_t c = blockIdx.x;
  const double* sm = strideMean + c * strideMeanStride;
  double total = 0.0;
  for (uint32_t base = 0; base < nstrides; base += kMeanStage) {
    const uint32_t n = min((uint32_t)kMeanStage, nstrides - base);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += kThreads)
      stage[k] = sm[base + k];
    __syncthreads();
    if (threadIdx.x == 0)
      for (uint32_t k = 0; k < n; k++)
        total += stage[k];
  }
  if (threadIdx.x != 0)
    return;
  const ChunkGeom g = geom[c];
  const bool is_const = st[c].not_const_flag == 0;
  st[c].is_const = is_const ? 1u : 0u;
  if (is_const)  // the header stores the value itself (Conditioner.cpp:28-44)
    st[c].mean = (double)vol[((size_t)g.org[2] * vd.dims[1] + g.org[1]) * vd.dims[0] + g.org[0]];
  else
    st[c].mean = total / (double)nstrides;
}

// vals[i] = (double)vol[gather(i)] - mean
template <typename T>
__global__ void k_gather_condition(const T* __restrict__ vol, VolDesc vd, const ChunkGeom* geom,
                                   uint32_t cx, uint32_t cy, uint32_t n, double* vals,
                                   size_t valsStride, const CoderState* st)
{
  const uint32_t c = blockIdx.y;
  const ChunkGeom g = geom[c];
  const double mean = st[c].mean;
  const size_t vx = vd.dims[0], vy = vd.dims[1];
  double* out = vals + c * valsStride;
  for (uint32_t i = blockIdx.x * blockDim.x * 4 + threadIdx.x, k = 0; k < 4 && i < n;
       k++, i += blockDim.x) {
    const uint32_t x = i % cx, r = i / cx;
    const uint32_t y = r % cy, z = r / cy;
    const T v = vol[((size_t)(g.org[2] + z) * vy + (g.org[1] + y)) * vx + g.org[0] + x];
    out[i] = (double)v - mean;
  }
}

// out[scatter(i)] = (T)(vals[i] + mean), or the constant value (Conditioner.cpp:66-96)
template <typename T, bool kCrop = false>
__global__ void k_scatter_uncondition(T* __restrict__ vol, VolDesc vd, const GeomOf<kCrop>* geom,
                                      uint32_t cx, uint32_t cy, uint32_t n, const double* vals,
                                      size_t valsStride, const CoderState* st)
{
  const uint32_t c = blockIdx.y;
  const GeomOf<kCrop> g = geom[c];
  const double mean = st[c].mean;
  const bool is_const = st[c].is_const != 0;
  const size_t vx = vd.dims[0], vy = vd.dims[1];
  const double* in = vals + c * valsStride;
  for (uint32_t i = blockIdx.x * blockDim.x * 4 + threadIdx.x, k = 0; k < 4 && i < n;
       k++, i += blockDim.x) {
    const uint32_t x = i % cx, r = i / cx;
    const uint32_t y = r % cy, z = r / cy;
    if constexpr (kCrop) {
      if (crop_has(g, x, y, z))
        vol[crop_addr(g, vd, x, y, z)] = (T)(is_const ? mean : in[i] + mean);
    }
    else {
      const double v = is_const ? mean : in[i] + mean;
      vol[((size_t)(g.org[2] + z) * vy + (g.org[1] + y)) * vx + g.org[0] + x] = (T)v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// quantiser
// ------------------------------------------------------------------------------------------

constexpr int kMaxPer = 16;   // samples per thread, as 16-byte loads
__global__ void __launch_bounds__(kThreads)
k_maxabs(const double* vals, size_t valsStride, uint32_t n, CoderState* st)
{
  const uint32_t c = blockIdx.y;
  if (st[c].is_const)
    return;
  __shared__ double wmax[kThreads / 64];
  const double* in = vals + c * valsStride;
  const uint32_t base = blockIdx.x * (kThreads * kMaxPer);
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxPer / 2; k++) {
    const uint32_t i = base + (k * kThreads + threadIdx.x) * 2;
    if (i + 1 < n) {
      const double2 v = *reinterpret_cast<const double2*>(in + i);
      m = fmax(m, fmax(fabs(v.x), fabs(v.y)));
    }
    else if (i < n)
      m = fmax(m, fabs(in[i]));
  }
  for (int d = 32; d > 0; d >>= 1)
    m = fmax(m, __shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0)
    wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; w++)
      m = fmax(m, wmax[w]);
    if (m > 0.0)  // non-negative doubles order like their bit patterns
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].maxabs),
                (unsigned long long)__double_as_longlong(m));
  }
}

// ------------------------------------------------------------------------------------------
// PSNR mode: error of the mid-tread quantiser with step q (src/SPECK_FLT.cpp:237-266).  Strides
// of 4096 coefficients are summed one after the other, each sequentially, with the fused
// multiply-adds of the canonical build: diff = fma(-q, rint(v / q'), v), acc = fma(diff, diff, acc)
// where q' = 1/q is formed first.  Same LDS staging as k_stride_sums.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kMseStride = 4096;

__global__ void __launch_bounds__(kThreads)
k_mse_strides(const double* vals, size_t valsStride, uint32_t n, double* partial,
              size_t partialStride, const CoderState* st)
{
  __shared__ double tile[kSumStrides][kSumSeg + 1];
  const uint32_t c = blockIdx.y;
  if (st[c].is_const || !st[c].mse_active)
    return;
  const double q = st[c].q, rcp_q = 1.0 / q;
  const double* in = vals + c * valsStride;
  const uint32_t npart = n / kMseStride + 1;            // the last one may be short or empty
  const uint32_t s0 = blockIdx.x * kSumStrides;
  double acc = 0.0;
  for (uint32_t seg = 0; seg < kMseStride; seg += kSumSeg) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)(kSumStrides * kSumSeg); k += kThreads) {
      const uint32_t r = k / kSumSeg, j = k % kSumSeg;
      const uint64_t e = (uint64_t)(s0 + r) * kMseStride + seg + j;
      tile[r][j] = (s0 + r < npart && e < n) ? in[e] : 0.0;   // (a zero adds exactly nothing)
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kSumStrides && s0 + threadIdx.x < npart) {
      const uint64_t e0 = (uint64_t)(s0 + threadIdx.x) * kMseStride + seg;
      const uint32_t len = e0 >= n ? 0u : (uint32_t)min((uint64_t)kSumSeg, n - e0);
      for (uint32_t j = 0; j < len; j++) {
        const double v = tile[threadIdx.x][j];
        const double diff = fma(-q, rint(v * rcp_q), v);
        acc = fma(diff, diff, acc);
      }
    }
  }
  if (threadIdx.x < (uint32_t)kSumStrides && s0 + threadIdx.x < npart)
    partial[c * partialStride + s0 + threadIdx.x] = acc;
}

__global__ void k_mse_final(uint32_t n, const double* partial, size_t partialStride,
                            CoderState* st, uint32_t nchunks)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks || st[c].is_const || !st[c].mse_active)
    return;
  const uint32_t npart = n / kMseStride + 1;
  const double* pp = partial + c * partialStride;
  double total = 0.0;
  for (uint32_t s = 0; s < npart; s++)
    total += pp[s];
  st[c].mse = total / (double)n;
}

// PSNR of the whole volume (psnr_vol.h): every chunk walks the same ladder of five q, so one pass over the coefficients
// takes all five estimates -- k_mse_strides' staging, five accumulators a lane, each rung's chain of 4096 dependent
// fused multiply-adds independent of the others'.  partial[chunk][rung][stride]; every entry k_mse_ladder_pick reads
// is written here, the short or empty last stride included.
__global__ void __launch_bounds__(kThreads)
k_mse_ladder(const double* vals, size_t valsStride, uint32_t n, double* partial, size_t rungStride,
             const CoderState* st, PsnrLadder L)
{
  __shared__ double tile[kSumStrides][kSumSeg + 1];
  const uint32_t c = blockIdx.y;
  if (st[c].is_const)
    return;
  double q[kPsnrRungs], rcp_q[kPsnrRungs], acc[kPsnrRungs];
#pragma unroll
  for (int k = 0; k < kPsnrRungs; k++) {
    q[k] = L.q[k];
    rcp_q[k] = 1.0 / q[k];
    acc[k] = 0.0;
  }
  const double* in = vals + c * valsStride;
  const uint32_t npart = psnr_vol_strides(n);
  const uint32_t s0 = blockIdx.x * kSumStrides;
  for (uint32_t seg = 0; seg < kPsnrStride; seg += kSumSeg) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)(kSumStrides * kSumSeg); k += kThreads) {
      const uint32_t r = k / kSumSeg, j = k % kSumSeg;
      const uint64_t e = (uint64_t)(s0 + r) * kPsnrStride + seg + j;
      tile[r][j] = (s0 + r < npart && e < n) ? in[e] : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kSumStrides && s0 + threadIdx.x < npart) {
      const uint64_t e0 = (uint64_t)(s0 + threadIdx.x) * kPsnrStride + seg;
      const uint32_t len = e0 >= n ? 0u : (uint32_t)min((uint64_t)kSumSeg, n - e0);
      for (uint32_t j = 0; j < len; j++) {
        const double v = tile[threadIdx.x][j];
#pragma unroll
        for (int k = 0; k < kPsnrRungs; k++)
          acc[k] = psnr_vol_term(acc[k], v, q[k], rcp_q[k]);
      }
    }
  }
  if (threadIdx.x < (uint32_t)kSumStrides && s0 + threadIdx.x < npart) {
    double* out = partial + (size_t)c * kPsnrRungs * rungStride + s0 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kPsnrRungs; k++)
      out[k * rungStride] = acc[k];
  }
}

// One lane per chunk: each rung's stride sums in order, the first rung at or under t, the width rule.  A chunk that is
// refused keeps a q the coder can run on (the call is refused once the batch's states are read back)
__global__ void k_mse_ladder_pick(uint32_t n, const double* partial, size_t rungStride, CoderState* st,
                                  uint32_t nchunks, PsnrLadder L)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks)
    return;
  CoderState& s = st[c];
  s.mse_active = 0;
  s.wide = 0;
  s.need_retry = 0;
  if (s.is_const)
    return;
  const uint32_t npart = psnr_vol_strides(n);
  const double* pp = partial + (size_t)c * kPsnrRungs * rungStride;
  int rung = -1;
  double mse = 0.0;
  for (int k = 0; k < kPsnrRungs && rung < 0; k++) {
    mse = psnr_vol_total(pp + k * rungStride, npart, n);
    if (mse <= L.t)
      rung = k;
  }
  const int width = rung < 0 ? -1 : psnr_vol_width(s.maxabs, L.q[rung]);
  s.mse = mse;
  if (width < 0) {
    const double q = s.maxabs / 4294967295.0;
    s.q = q > 0.0 && q < INFINITY ? q : 1.0;
    s.mse_active = rung < 0 ? kPsnrRefusedNoRung : kPsnrRefusedWidth;
    return;
  }
  s.q = L.q[rung];
  s.need_retry = (uint32_t)width;
}

// SPECK_FLT.cpp:282-301 (fixed-rate q) ; `wide` selects the high-precision retry
__global__ void k_make_q_rate(CoderState* st, uint32_t nchunks, int wide_pass)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks)
    return;
  if (wide_pass) {
    if (!st[c].need_retry)
      return;
    st[c].q = st[c].maxabs / 0x1.fffffffffffffp52;
    st[c].wide = 1;
  }
  else {
    st[c].q = st[c].maxabs / 4294967295.0;
    st[c].wide = 0;
  }
}

// SPECK_FLT.cpp:345-368 : ll = llrint(v * (1/q)) ; sign bit = (ll >= 0) ; magnitude ; plus the
// msb position that the coder's significance pyramid starts from.  One wave = one sign word.
template <typename CT>
__global__ void k_quantize(const double* vals, size_t valsStride, uint32_t n, CT* coef,
                           size_t coefStride, uint64_t* sign, size_t signStride, int8_t* msb,
                           size_t msbStride, const CoderState* st, int wide_pass)
{
  const uint32_t c = blockIdx.y;
  const CoderState& s = st[c];
  if (s.is_const || (wide_pass && !s.need_retry))
    return;
  const double inv = 1.0 / s.q;
  const double* in = vals + c * valsStride;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  long long ll = 0;
  bool nonneg = false;
  if (i < n) {
    ll = __double2ll_rn(in[i] * inv);
    nonneg = ll >= 0;
    const unsigned long long mag = (unsigned long long)(ll < 0 ? -ll : ll);
    coef[c * coefStride + i] = (CT)mag;
    msb[c * msbStride + i] = mag ? (int8_t)(63 - __clzll((long long)mag)) : (int8_t)-1;
  }
  const unsigned long long word = __ballot(nonneg);
  if ((threadIdx.x & 63) == 0 && i < n)
    sign[c * signStride + (i >> 6)] = word;
}

// The same for 32-bit magnitudes, four consecutive samples per thread: 32-byte loads, 16-byte stores of
// the magnitudes, one 4-byte store of the four msb positions; the sign word of 64 samples is put
// together by the 16 lanes that hold them (all strides and n are multiples of 4 -- launch_quantize).
__global__ void __launch_bounds__(kThreads)
k_quantize4(const double* vals, size_t valsStride, uint32_t n, uint32_t* coef, size_t coefStride,
            uint64_t* sign, size_t signStride, int8_t* msb, size_t msbStride, const CoderState* st)
{
  const uint32_t c = blockIdx.y;
  const CoderState& s = st[c];
  if (s.is_const)
    return;
  const double inv = 1.0 / s.q;
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  uint32_t nn = 0;   // bit e: sample i + e is non-negative
  if (i < n) {
    const double2* in = reinterpret_cast<const double2*>(vals + c * valsStride + i);
    const double2 a = in[0], b2 = in[1];
    const double v[4] = {a.x, a.y, b2.x, b2.y};
    uint32_t mag[4], mb = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const long long ll = __double2ll_rn(v[e] * inv);
      nn |= (ll >= 0 ? 1u : 0u) << e;
      const unsigned long long m = (unsigned long long)(ll < 0 ? -ll : ll);
      mag[e] = (uint32_t)m;
      mb |= (uint32_t)(uint8_t)(m ? (int8_t)(63 - __clzll((long long)m)) : (int8_t)-1) << (8 * e);
    }
    *reinterpret_cast<uint4*>(coef + c * coefStride + i) = make_uint4(mag[0], mag[1], mag[2], mag[3]);
    *reinterpret_cast<uint32_t*>(msb + c * msbStride + i) = mb;
  }
  // 16 lanes x 4 bits = one sign word
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t word = (uint64_t)nn << (4 * (lane & 15u));
#pragma unroll
  for (int d = 1; d < 16; d <<= 1)
    word |= __shfl_xor(word, d, 64);
  if ((lane & 15u) == 0 && i < n)
    sign[c * signStride + (i >> 6)] = word;
}

// Every sample of a chunk from its coefficient (dequant.h), four per lane.  When the decoder's masks are given, the
// coefficients that became significant but were never refined are completed here instead of in a pass of their own
// (k_dec_finish, speck_dec.hip).
template <typename CT>
__global__ void __launch_bounds__(kThreads)
k_inv_quantize(DequantSrc Q, uint32_t n, double* vals, size_t valsStride, const CoderState* st, int wide_pass)
{
  const uint32_t c = blockIdx.y;
  const CoderState& s = st[c];
  if (s.is_const || (int)s.wide != wide_pass)
    return;
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;   // four samples of one mask word
  if (i0 >= n)
    return;
  const CT* in = Q.coefs<CT>(c) + i0;
  double* out = vals + c * valsStride + i0;
  CT v[4];
  const uint32_t cnt = min(4u, n - i0);
  if (cnt == 4) {
    if (sizeof(CT) == 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(in);
      v[0] = (CT)q.x, v[1] = (CT)q.y, v[2] = (CT)q.z, v[3] = (CT)q.w;
    }
    else {
      const ulonglong2 q0 = *reinterpret_cast<const ulonglong2*>(in);
      const ulonglong2 q1 = *reinterpret_cast<const ulonglong2*>(in + 2);
      v[0] = (CT)q0.x, v[1] = (CT)q0.y, v[2] = (CT)q1.x, v[3] = (CT)q1.y;
    }
  }
  else
    for (uint32_t k = 0; k < 4; k++)
      v[k] = k < cnt ? in[k] : (CT)1;
  const uint32_t w = i0 >> 6, sh = i0 & 63;
  // (the mask words and the decoder's state are read only where a coefficient is 0: few are)
  if (Q.has_masks() && (v[0] == 0 || v[1] == 0 || v[2] == 0 || v[3] == 0)) {
    const uint32_t mn = (uint32_t)(Q.sigNew[c * Q.maskStride + w] >> sh) & 15u;
    const uint32_t mo = (uint32_t)(Q.sigOld[c * Q.maskStride + w] >> sh) & 15u;
    if (mn | mo) {
      const int pl = Q.dst[c].lastPlane;   // (few lanes get here: the threshold per element, not a DequantRule)
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (v[k] == 0 && ((mn | mo) >> k) & 1u)
          v[k] = never_refined<CT>(pl + (((mn >> k) & 1u) ? 0 : 1));
    }
  }
  const uint32_t sg = (uint32_t)(Q.sign[c * Q.signStride + w] >> sh);
  double r[4];
#pragma unroll
  for (int k = 0; k < 4; k++)
    r[k] = dequant_value(s.q, v[k], ((sg >> k) & 1u) != 0);
  if (cnt == 4) {
    *reinterpret_cast<double2*>(out) = make_double2(r[0], r[1]);
    *reinterpret_cast<double2*>(out + 2) = make_double2(r[2], r[3]);
  }
  else
    for (uint32_t k = 0; k < cnt; k++)
      out[k] = r[k];
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------

template <typename T>
int launch_condition(hipStream_t stream, const T* vol, VolDesc vd, const ChunkGeom* geom,
                     uint32_t nchunks, const uint32_t cdims[3], uint32_t nstrides,
                     double* strideMean, size_t strideMeanStride, double* vals,
                     size_t valsStride, CoderState* st, bool gather, bool want_range,
                     bool org_x_aligned)
{
  const uint32_t n = cdims[0] * cdims[1] * cdims[2];
  const uint32_t ssz = n / nstrides;
  // rows of whole 128-byte pieces, 16-byte aligned in the volume, a stride = whole rows
  const uint32_t perLoad = 8 * (16 / (uint32_t)sizeof(T));
  const bool rowsPath = cdims[0] % perLoad == 0 && ssz % cdims[0] == 0 &&
                        vd.dims[0] % (16 / sizeof(T)) == 0 &&
                        reinterpret_cast<uintptr_t>(vol) % 16 == 0 && org_x_aligned;
  if (rowsPath)
    LAUNCH_K(k_stride_sums_rows<T>, dim3((nstrides + 63) / 64, nchunks), dim3(64), 0, stream, vol,
             vd, geom, cdims[0], cdims[1], nstrides, ssz, strideMean, strideMeanStride, st,
             want_range ? 1 : 0);
  else
    LAUNCH_K(k_stride_sums<T>, dim3((nstrides + kSumStrides - 1) / kSumStrides, nchunks),
             dim3(kThreads), 0, stream, vol, vd, geom, cdims[0], cdims[1], cdims[2], nstrides, ssz,
             strideMean, strideMeanStride, st, want_range ? 1 : 0);
  LAUNCH_K(k_mean_finalize<T>, dim3(nchunks), dim3(kThreads), 0, stream, vol, vd, geom,
                     nstrides, strideMean, strideMeanStride, st);
  if (gather)   // otherwise the first lifting pass reads the volume itself
    LAUNCH_K(k_gather_condition<T>, dim3((n + kThreads * 4 - 1) / (kThreads * 4), nchunks),
             dim3(kThreads), 0, stream, vol, vd, geom, cdims[0], cdims[1], n, vals, valsStride, st);
  HIP_CHECK(hipGetLastError());
  return 0;
}
template int launch_condition<float>(hipStream_t, const float*, VolDesc, const ChunkGeom*,
                                     uint32_t, const uint32_t[3], uint32_t, double*, size_t,
                                     double*, size_t, CoderState*, bool, bool, bool);
template int launch_condition<double>(hipStream_t, const double*, VolDesc, const ChunkGeom*,
                                      uint32_t, const uint32_t[3], uint32_t, double*, size_t,
                                      double*, size_t, CoderState*, bool, bool, bool);

template <typename T>
int launch_scatter(hipStream_t stream, T* vol, VolDesc vd, const ChunkGeom* geom,
                   uint32_t nchunks, const uint32_t cdims[3], const double* vals,
                   size_t valsStride, const CoderState* st, const CropGeom* crop)
{
  const uint32_t n = cdims[0] * cdims[1] * cdims[2];
  if (crop)
    LAUNCH_K((k_scatter_uncondition<T, true>), dim3((n + kThreads * 4 - 1) / (kThreads * 4), nchunks), dim3(kThreads), 0,
             stream, vol, vd, crop, cdims[0], cdims[1], n, vals, valsStride, st);
  else
  LAUNCH_K(k_scatter_uncondition<T>,
                     dim3((n + kThreads * 4 - 1) / (kThreads * 4), nchunks), dim3(kThreads), 0,
                     stream, vol, vd, geom, cdims[0], cdims[1], n, vals, valsStride, st);
  HIP_CHECK(hipGetLastError());
  return 0;
}
template int launch_scatter<float>(hipStream_t, float*, VolDesc, const ChunkGeom*, uint32_t,
                                   const uint32_t[3], const double*, size_t, const CoderState*,
                                   const CropGeom*);
template int launch_scatter<double>(hipStream_t, double*, VolDesc, const ChunkGeom*, uint32_t,
                                    const uint32_t[3], const double*, size_t, const CoderState*,
                                    const CropGeom*);

int launch_maxabs_q(hipStream_t stream, const double* vals, size_t valsStride, uint32_t nchunks,
                    uint32_t n, CoderState* st, bool have_max)
{
  if (!have_max)
    LAUNCH_K(k_maxabs, dim3((n + kThreads * kMaxPer - 1) / (kThreads * kMaxPer), nchunks),
                       dim3(kThreads), 0, stream, vals, valsStride, n, st);
  LAUNCH_K(k_make_q_rate, dim3((nchunks + 63) / 64), dim3(64), 0, stream, st, nchunks,
                     0);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_mse(hipStream_t stream, const double* vals, size_t valsStride, uint32_t nchunks,
               uint32_t n, double* partial, size_t partialStride, CoderState* st)
{
  const uint32_t npart = n / kMseStride + 1;
  LAUNCH_K(k_mse_strides, dim3((npart + kSumStrides - 1) / kSumStrides, nchunks), dim3(kThreads), 0,
           stream, vals, valsStride, n, partial, partialStride, st);
  LAUNCH_K(k_mse_final, dim3((nchunks + 63) / 64), dim3(64), 0, stream, n, partial, partialStride,
           st, nchunks);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_mse_ladder(hipStream_t stream, const double* vals, size_t valsStride, uint32_t nchunks, uint32_t n,
                      double* partial, size_t rungStride, CoderState* st, const PsnrLadder& L)
{
  const uint32_t npart = psnr_vol_strides(n);
  if (rungStride < npart)
    return -1;
  LAUNCH_K(k_mse_ladder, dim3((npart + kSumStrides - 1) / kSumStrides, nchunks), dim3(kThreads), 0, stream, vals,
           valsStride, n, partial, rungStride, st, L);
  LAUNCH_K(k_mse_ladder_pick, dim3((nchunks + 63) / 64), dim3(64), 0, stream, n, partial, rungStride, st, nchunks, L);
  HIP_CHECK(hipGetLastError());
  return 0;
}

// PSNR mode: the chunks flagged for 64-bit coefficients keep their q
__global__ void k_mark_wide(CoderState* st, uint32_t nchunks)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nchunks && st[c].need_retry)
    st[c].wide = 1;
}

int launch_mark_wide(hipStream_t stream, uint32_t nchunks, CoderState* st)
{
  LAUNCH_K(k_mark_wide, dim3((nchunks + 63) / 64), dim3(64), 0, stream, st, nchunks);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_make_q_wide(hipStream_t stream, uint32_t nchunks, CoderState* st)
{
  LAUNCH_K(k_make_q_rate, dim3((nchunks + 63) / 64), dim3(64), 0, stream, st, nchunks,
                     1);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_quantize(hipStream_t stream, bool wide, const double* vals, size_t valsStride,
                    uint32_t nchunks, uint32_t n, void* coef, size_t coefStride, uint64_t* sign,
                    size_t signStride, int8_t* msb, size_t msbStride, const CoderState* st)
{
  dim3 grid((n + kThreads - 1) / kThreads, nchunks);
  if (wide)
    LAUNCH_K(k_quantize<uint64_t>, grid, dim3(kThreads), 0, stream, vals, valsStride, n,
                       (uint64_t*)coef, coefStride, sign, signStride, msb, msbStride, st, 1);
  else if (n % 64 == 0 && valsStride % 4 == 0 && coefStride % 4 == 0 && msbStride % 4 == 0)
    LAUNCH_K(k_quantize4, dim3((n / 4 + kThreads - 1) / kThreads, nchunks), dim3(kThreads), 0, stream, vals,
             valsStride, n, (uint32_t*)coef, coefStride, sign, signStride, msb, msbStride, st);
  else
    LAUNCH_K(k_quantize<uint32_t>, grid, dim3(kThreads), 0, stream, vals, valsStride, n,
                       (uint32_t*)coef, coefStride, sign, signStride, msb, msbStride, st, 0);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_inv_quantize(hipStream_t stream, bool wide, const DequantSrc& src, uint32_t nchunks, uint32_t n,
                        double* vals, size_t valsStride, const CoderState* st)
{
  dim3 grid((n + kThreads * 4 - 1) / (kThreads * 4), nchunks);
  if (wide)
    LAUNCH_K(k_inv_quantize<uint64_t>, grid, dim3(kThreads), 0, stream, src, n, vals, valsStride, st, 1);
  else
    LAUNCH_K(k_inv_quantize<uint32_t>, grid, dim3(kThreads), 0, stream, src, n, vals, valsStride, st, 0);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace sperrhip
