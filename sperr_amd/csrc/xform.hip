// xform.hip -- floating-point stages of the chunk pipeline as HIP kernels for gfx950:
// conditioner (mean / constant test), CDF 9/7 lifting DWT and IDWT, max-reduce, mid-tread
// quantiser and its inverse, chunk gather/scatter.  Everything is fp64 with the reference's exact
// operation order; compile with -ffp-contract=off (every fused multiply-add of the canonical
// reference build is an explicit fma()).
//
// Reference behaviour restated (file:line under /root/reference):
//   src/Conditioner.cpp:10-64,119-163   strided sequential mean, constant test
//   src/CDF97.cpp:132-148,284-302,345-474,598-666   dyadic / wavelet-packet 3D transform
//   src/SPECK_FLT.cpp:282-301,311-399   q, quantise, inverse quantise
//   src/SPERR3D_OMP_C.cpp:236-261, src/SPERR3D_OMP_D.cpp:167-184   gather / scatter
#include <type_traits>

#include "xform.h"
#include "lift_window.h"
#include "dequant.h"

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
// CDF 9/7 lifting along one axis, LDS-staged line tiles
// ------------------------------------------------------------------------------------------
//
// A workgroup stages NL adjacent lines of length `len` in LDS as sm[pos * (NL+1) + line] with the
// samples already de-interleaved ([even | odd], src/CDF97.cpp:476-519), runs the four lifting
// steps + scaling with a barrier between dependent steps, and writes the lines back.  For the Y
// and Z axes the NL lines are NL consecutive x positions, so every global access is a coalesced
// NL*8-byte segment; for the X axis the lines are NL consecutive rows and lanes run along x.

extern __shared__ __attribute__((aligned(16))) char dyn_smem[];

// IO: 0 = in place on the fp64 chunk buffer; 1 / 2 = the pass also moves the chunk between the
// float / double VOLUME and the chunk buffer: the first forward pass reads the volume through the
// gather map and subtracts the mean (src/SPERR3D_OMP_C.cpp:236-261, Conditioner.cpp:48-50), the
// last inverse pass adds the mean, narrows and scatters (Conditioner.cpp:66-96,
// SPERR3D_OMP_D.cpp:167-184, SPERR_C_API.cpp:246-250).  Both passes cover the whole chunk.
constexpr int kLoadBatch = 8;

// kCrop (inverse, IO != 0 only): the pass writes the chunk's window into the box; a tile with no line
// in the window has nothing to do
template <bool FORWARD, int IO, bool kCrop = false>
__global__ void __launch_bounds__(kThreads)
k_lift_axis(double* vals, size_t valsStride, uint32_t cx, uint32_t cy, int axis, uint32_t rx,
            uint32_t ry, uint32_t rz, int NL, LiftConsts K, CoderState* st, void* volume,
            VolDesc vd, const GeomOf<kCrop>* geom, LiftFuse F)
{
  static_assert(!kCrop || (!FORWARD && IO != 0), "the crop variant is a last inverse pass");
  const uint32_t c = blockIdx.y;
  const bool is_const = st[c].is_const != 0;
  if (is_const && !(IO != 0 && !FORWARD))
    return;
  double* sm = reinterpret_cast<double*>(dyn_smem);
  double* buf = vals + c * valsStride;
  const uint32_t region[3] = {rx, ry, rz};
  const uint32_t bx = (!FORWARD && F.bufx) ? F.bufx : cx, by = (!FORWARD && F.bufy) ? F.bufy : cy;   // (compact buffer)
  const size_t stride[3] = {1, bx, (size_t)bx * by};
  const int ua = (axis == 0) ? 1 : 0;            // axis along which the NL lines are adjacent
  const int wa = (axis == 2) ? 1 : 2;            // remaining axis
  const uint32_t len = region[axis];
  const uint32_t ntu = (region[ua] + NL - 1) / NL;
  const uint32_t tu = blockIdx.x % ntu, tw = blockIdx.x / ntu;
  const uint32_t u0 = tu * NL;
  const uint32_t nl = min((uint32_t)NL, region[ua] - u0);  // valid lines in this tile
  double* tile = buf + (size_t)u0 * stride[ua] + (size_t)tw * stride[wa];
  const size_t sl = stride[axis], su = stride[ua];
  const int NLP = NL + 1;
  const uint32_t even_len = len - len / 2, odd_len = len / 2;
  const int tid = threadIdx.x;

  // volume address of chunk sample (line l, position p) of this tile
  using VT = typename std::conditional<IO == 1, float, double>::type;
  VT* vol = reinterpret_cast<VT*>(volume);
  size_t vbase = 0, vsl = 0, vsu = 0;
  double mean = 0.0;
  CropGeom cg{};
  if constexpr (kCrop) {   // (uniform)
    cg = geom[c];
    if (tw - cg.lo[wa] >= cg.hi[wa] - cg.lo[wa] || u0 >= cg.hi[ua] || u0 + nl <= cg.lo[ua])
      return;
    mean = st[c].mean;
  }
  else if (IO != 0) {
    const ChunkGeom g = geom[c];
    const size_t vstride[3] = {1, (size_t)vd.dims[0], (size_t)vd.dims[0] * vd.dims[1]};
    vbase = (size_t)g.org[0] * vstride[0] + (size_t)g.org[1] * vstride[1] +
            (size_t)g.org[2] * vstride[2] + (size_t)u0 * vstride[ua] + (size_t)tw * vstride[wa];
    vsl = vstride[axis];
    vsu = vstride[ua];
    mean = st[c].mean;
  }

  // ---- load: a thread issues kLoadBatch loads before it uses the first value (one at a time
  // leaves the pass waiting on HBM latency) ----
  using LT = typename std::conditional<(IO != 0 && FORWARD), VT, double>::type;
  // (l, p) of this tile as chunk coordinates, and whether a later pass of the forward order
  // touches the sample (LiftFuse)
  auto outside_inner = [&](uint32_t l, uint32_t p, size_t& idx) -> bool {
    uint32_t xyz[3];
    xyz[axis] = p;
    xyz[ua] = u0 + l;
    xyz[wa] = tw;
    idx = ((size_t)xyz[2] * cy + xyz[1]) * cx + xyz[0];
    return !(xyz[0] < F.inner[0] && xyz[1] < F.inner[1] && xyz[2] < F.inner[2]);
  };
  const bool dequant = !FORWARD && F.mode == 2 && !st[c].wide;
  const DequantSrc& Q = F.src;
  const bool haveMasks = dequant && Q.has_masks();
  const DequantRule<uint32_t> rule =
      dequant_rule<uint32_t>(dequant ? st[c].q : 0.0, haveMasks, haveMasks ? Q.dst + c : nullptr, Q.coefSigned != 0);
  auto fetch = [&](uint32_t l, uint32_t p) -> LT {
    if (IO != 0 && FORWARD)
      return (LT)vol[vbase + l * vsu + p * vsl];
    if (!FORWARD && dequant) {
      size_t idx;
      if (outside_inner(l, p, idx)) {   // this one sample from its coefficient (dequant.h); the loads are independent
        const uint32_t v = Q.coefs<uint32_t>(c)[idx];
        if (rule.scheme)   // (the sign in bit 31, the value complete: DequantSrc::coefSigned)
          return (LT)dequant_signed(rule, v);
        const uint32_t w = (uint32_t)(idx >> 6), sh = (uint32_t)(idx & 63);
        const uint64_t sgw = Q.sign[c * Q.signStride + w];
        const uint64_t mnw = haveMasks ? Q.sigNew[c * Q.maskStride + w] : 0ull;
        const uint64_t mow = haveMasks ? Q.sigOld[c * Q.maskStride + w] : 0ull;
        return (LT)dequant_masks(rule, v, mnw, mow, sgw, sh);
      }
    }
    return (LT)tile[l * su + p * sl];
  };
  auto deposit = [&](uint32_t l, uint32_t p, LT v) {
    const uint32_t dst = FORWARD ? ((p & 1) ? even_len + (p >> 1) : (p >> 1)) : p;
    sm[dst * NLP + l] = (IO != 0 && FORWARD) ? (double)v - mean : (double)v;
  };
  if (!(is_const && !(IO != 0 && FORWARD))) {
    if (axis == 0) {  // lanes along the line: a wavefront moves 64 consecutive samples of a line
      const uint32_t nseg = (len + 63) / 64, nsg = nl * nseg, step = kThreads / 64;
      for (uint32_t sg0 = tid / 64; sg0 < nsg; sg0 += step * kLoadBatch) {
        LT v[kLoadBatch];
#pragma unroll
        for (int u = 0; u < kLoadBatch; u++) {
          const uint32_t sg = sg0 + u * step, l = sg / nseg, p = (sg % nseg) * 64 + tid % 64;
          v[u] = (sg < nsg && p < len) ? fetch(l, p) : (LT)0;
        }
#pragma unroll
        for (int u = 0; u < kLoadBatch; u++) {
          const uint32_t sg = sg0 + u * step, l = sg / nseg, p = (sg % nseg) * 64 + tid % 64;
          if (sg < nsg && p < len)
            deposit(l, p, v[u]);
        }
      }
    }
    else {            // lanes across the lines
      const uint32_t l = tid % NL, k0 = tid / NL, kg = kThreads / NL;
      if (l < nl)
        for (uint32_t p0 = k0; p0 < len; p0 += kg * kLoadBatch) {
          LT v[kLoadBatch];
#pragma unroll
          for (int u = 0; u < kLoadBatch; u++)
            v[u] = p0 + u * kg < len ? fetch(l, p0 + u * kg) : (LT)0;
#pragma unroll
          for (int u = 0; u < kLoadBatch; u++)
            if (p0 + u * kg < len)
              deposit(l, p0 + u * kg, v[u]);
        }
    }
  }
  __syncthreads();

  // ---- lift ----
  if (!is_const) {
    const uint32_t l = tid % NL, k0 = tid / NL, kg = kThreads / NL;
    double* E = sm + l;
    double* O = sm + (size_t)even_len * NLP + l;
#define EV(i) E[(size_t)(i) * NLP]
#define OD(i) O[(size_t)(i) * NLP]
    auto odd_step = [&](double k) {
      if (l < nl)
        for (uint32_t i = k0; i < odd_len; i += kg) {
          const uint32_t r = min(i + 1, even_len - 1);
          OD(i) = fma(k, EV(i) + EV(r), OD(i));
        }
      __syncthreads();
    };
    auto even_step = [&](double k) {
      if (l < nl)
        for (uint32_t i = k0; i < even_len; i += kg) {
          const uint32_t a = max(i, 1u) - 1, b = min(i, odd_len - 1);
          EV(i) = fma(k, OD(a) + OD(b), EV(i));
        }
      __syncthreads();
    };
    if (FORWARD) {  // src/CDF97.cpp:598-631
      odd_step(K.alpha);
      even_step(K.beta);
      odd_step(K.gamma);
      if (l < nl) {
        for (uint32_t i = k0; i < even_len; i += kg) {
          const uint32_t a = max(i, 1u) - 1, b = min(i, odd_len - 1);
          EV(i) = K.eps * fma(K.delta, OD(a) + OD(b), EV(i));
        }
      }
      __syncthreads();
      if (l < nl)
        for (uint32_t i = k0; i < odd_len; i += kg)
          OD(i) = (-K.inv_eps) * OD(i);
      __syncthreads();
    }
    else {          // src/CDF97.cpp:633-666
      if (l < nl)
        for (uint32_t i = k0; i < odd_len; i += kg)
          OD(i) = (-K.eps) * OD(i);
      __syncthreads();
      if (l < nl)
        for (uint32_t i = k0; i < even_len; i += kg) {
          const uint32_t a = max(i, 1u) - 1, b = min(i, odd_len - 1);
          const double t = K.delta * (OD(a) + OD(b));
          EV(i) = fma(EV(i), K.inv_eps, -t);
        }
      __syncthreads();
      odd_step(-K.gamma);
      even_step(-K.beta);
      odd_step(-K.alpha);
    }
#undef EV
#undef OD
  }

  // ---- store ----
  // (crop variant: sample (line l, position p) goes to the box when it lies in the chunk's window)
  auto crop_store = [&](uint32_t l, uint32_t p, VT v) {
    uint32_t xyz[3];
    xyz[axis] = p;
    xyz[ua] = u0 + l;
    xyz[wa] = tw;
    if (crop_has(cg, xyz[0], xyz[1], xyz[2]))
      vol[crop_addr(cg, vd, xyz[0], xyz[1], xyz[2])] = v;
  };
  (void)crop_store;
  const bool wantMax = FORWARD && F.mode == 1 && !is_const;
  double vmax = 0.0;
  if (axis == 0) {
    const uint32_t nseg = (len + 63) / 64;
    for (uint32_t sg = tid / 64; sg < nl * nseg; sg += kThreads / 64) {
      const uint32_t l = sg / nseg, p = (sg % nseg) * 64 + tid % 64;
      if (p >= len)
        continue;
      const uint32_t src = FORWARD ? p : ((p & 1) ? even_len + (p >> 1) : (p >> 1));
      if constexpr (kCrop)
        crop_store(l, p, (VT)(is_const ? mean : sm[src * NLP + l] + mean));
      else if (IO != 0 && !FORWARD)
        vol[vbase + l * vsu + p * vsl] = (VT)(is_const ? mean : sm[src * NLP + l] + mean);
      else {
        const double v = sm[src * NLP + l];
        tile[l * su + p] = v;
        size_t idx;
        if (wantMax && outside_inner(l, p, idx))
          vmax = fmax(vmax, fabs(v));
      }
    }
  }
  else {
    const uint32_t l = tid % NL, k0 = tid / NL, kg = kThreads / NL;
    if (l < nl)
      for (uint32_t p = k0; p < len; p += kg) {
        const uint32_t src = FORWARD ? p : ((p & 1) ? even_len + (p >> 1) : (p >> 1));
        if constexpr (kCrop)
          crop_store(l, p, (VT)(is_const ? mean : sm[src * NLP + l] + mean));
        else if (IO != 0 && !FORWARD)
          vol[vbase + l * vsu + p * vsl] = (VT)(is_const ? mean : sm[src * NLP + l] + mean);
        else {
          const double v = sm[src * NLP + l];
          tile[l * su + p * sl] = v;
          size_t idx;
          if (wantMax && outside_inner(l, p, idx))
            vmax = fmax(vmax, fabs(v));
        }
      }
  }
  if (FORWARD && F.mode == 1) {   // (uniform: every wavefront reduces, one atomic each)
    for (int d = 32; d > 0; d >>= 1)
      vmax = fmax(vmax, __shfl_xor(vmax, d, 64));
    if ((tid & 63) == 0 && vmax > 0.0)  // non-negative doubles order like their bit patterns
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].maxabs),
                (unsigned long long)__double_as_longlong(vmax));
  }
}

// ------------------------------------------------------------------------------------------
// The two passes of the finest level that touch the volume, fused: forward x-lift then y-lift
// (volume -> fp64 buffer), inverse y-lift then x-lift (fp64 buffer -> volume).  A workgroup owns
// R rows of one z-slice and stages them in LDS together with a halo of 4 rows on each side: the
// four lifting steps reach one row further each, so rows y0-4 .. y0+R+3 determine the R rows
// exactly (the symmetric boundary rule only ever refers to rows of the slice itself).  Every
// sample goes through the very same operations as in k_lift_axis; halo rows are recomputed by the
// neighbouring tiles.  Saves one full read + write of the fp64 buffer per direction.
// The lifting itself runs in registers (lift16): the first version kept every intermediate in LDS
// and was bound by LDS bandwidth (about 40 eight-byte LDS accesses per sample against 12 bytes of
// HBM traffic); now a sample costs about 6.
// ------------------------------------------------------------------------------------------
constexpr int kXYHalo = 4;
constexpr int kXYThreads = 512;    // two workgroups per CU (LDS) = 4 waves per SIMD: 128 VGPRs each
constexpr int kStage = 16;         // global loads a lane has in flight while staging
constexpr int kSeg = 8;            // samples a thread produces per pass (plus 4 + 4 halo = 16 registers)

// position q of the whole-sample symmetric extension of a signal of n >= 2 samples
__device__ __forceinline__ uint32_t reflect_index(int q, int n)
{
  const int period = 2 * (n - 1);
  q = q < 0 ? -q : q;
  if (q >= period)
    q %= period;
  return (uint32_t)(q < n ? q : period - q);
}

// (lift16, lift_window: lift_window.h)

// kCrop (inverse only): the tile's rows of the chunk's window go to the box; a tile without one returns
template <bool FORWARD, int IO, bool kCrop = false>
__global__ void __launch_bounds__(kXYThreads)
k_lift_xy(double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz, int R,
          LiftConsts K, const CoderState* st, void* volume, VolDesc vd, const GeomOf<kCrop>* geom)
{
  static_assert(IO == 1 || IO == 2, "float or double volume");
  static_assert(!kCrop || !FORWARD, "the crop variant is a last inverse pass");
  using VT = typename std::conditional<IO == 1, float, double>::type;
  const uint32_t c = blockIdx.y;
  const bool is_const = st[c].is_const != 0;
  if (is_const && FORWARD)
    return;
  double* sm = reinterpret_cast<double*>(dyn_smem);
  const uint32_t ntile = (cy + R - 1) / R;
  const uint32_t z = blockIdx.x / ntile, y0 = (blockIdx.x % ntile) * R;
  const uint32_t ylo = y0 >= (uint32_t)kXYHalo ? y0 - kXYHalo : 0u;
  const uint32_t yhi = min(cy, y0 + R + kXYHalo);       // rows [ylo, yhi) are staged
  const uint32_t yend = min(cy, y0 + R);                // rows [y0, yend) are this tile's output
  const uint32_t nrow = yhi - ylo;
  const uint32_t RS = cx + 1;                           // row stride in LDS
  const uint32_t xe = cx - cx / 2, ye = cy - cy / 2;    // even samples of a row / of a column
  const GeomOf<kCrop> g = geom[c];
  VT* vol = reinterpret_cast<VT*>(volume);
  const size_t vsy = vd.dims[0], vsz = (size_t)vd.dims[0] * vd.dims[1];
  size_t vbase = 0;
  // rows [wy0, wy1) and columns [wx0, wx1) of the tile are written (all of them but in the crop variant)
  uint32_t wy0 = y0, wy1 = yend, wx0 = 0, wx1 = cx;
  if constexpr (kCrop) {   // (uniform)
    wy0 = max(y0, g.lo[1]);
    wy1 = min(yend, g.hi[1]);
    wx0 = g.lo[0];
    wx1 = g.hi[0];
    if (z - g.lo[2] >= g.hi[2] - g.lo[2] || wy0 >= wy1)
      return;
  }
  else
    vbase = (size_t)(g.org[2] + z) * vsz + (size_t)g.org[1] * vsy + g.org[0];
  // address of sample (x, y) of the tile's slice
  auto out_at = [&](uint32_t x, uint32_t y) -> size_t {
    if constexpr (kCrop)
      return crop_addr(g, vd, x, y, z);
    else
      return vbase + (size_t)y * vsy + x;
  };
  double* buf = vals + c * valsStride + (size_t)z * cx * cy;
  const double mean = st[c].mean;
  const uint32_t tid = threadIdx.x;

  if (is_const) {   // inverse only: the chunk is its constant
    if constexpr (kCrop) {
      const uint32_t w = wx1 - wx0;
      for (uint32_t k = tid; k < (wy1 - wy0) * w; k += kXYThreads)
        vol[out_at(wx0 + k % w, wy0 + k / w)] = (VT)mean;
    }
    else
      for (uint32_t k = tid; k < (yend - y0) * cx; k += kXYThreads)
        vol[vbase + (size_t)(y0 + k / cx) * vsy + k % cx] = (VT)mean;
    return;
  }

  // ---- stage the rows.  In LDS everything is interleaved (sample x of row y at [y - ylo][x]).
  // One wavefront per row, 64 samples per load; a lane issues kStage loads before it touches the
  // first value, so a workgroup keeps its whole tile in flight (one load at a time per wavefront
  // left the kernel waiting on HBM latency).
  const uint32_t lane = tid & 63u, wave = tid >> 6, nwaves = kXYThreads / 64;
  {
    using ST = typename std::conditional<FORWARD, VT, double>::type;
    const uint32_t nxb = (cx + 63) / 64;
    const uint32_t rowsW = nrow > wave ? (nrow - wave + nwaves - 1) / nwaves : 0;
    const uint32_t items = rowsW * nxb;        // (row, 64-sample block) pairs of this wavefront
    uint32_t ri = 0, bi = 0;                   // pair m = (row wave + nwaves * ri, block bi)
    for (uint32_t m0 = 0; m0 < items; m0 += kStage) {
      ST v[kStage];
      uint32_t ri2 = ri, bi2 = bi;
#pragma unroll
      for (int u = 0; u < kStage; u++) {
        const uint32_t j = wave + nwaves * ri2, x = lane + 64 * bi2;
        v[u] = 0;
        if (m0 + u < items && x < cx) {
          const uint32_t y = ylo + j;
          if (FORWARD)
            v[u] = (ST)vol[vbase + (size_t)y * vsy + x];
          else   // the buffer holds low | high halves along x and along y
            v[u] = (ST)buf[(size_t)((y & 1) ? ye + (y >> 1) : (y >> 1)) * cx + ((x & 1) ? xe + (x >> 1) : (x >> 1))];
        }
        if (++bi2 == nxb) {
          bi2 = 0;
          ri2++;
        }
      }
#pragma unroll
      for (int u = 0; u < kStage; u++) {
        const uint32_t j = wave + nwaves * ri, x = lane + 64 * bi;
        if (m0 + u < items && x < cx)
          sm[j * RS + x] = FORWARD ? (double)v[u] - mean : (double)v[u];
        if (++bi == nxb) {
          bi = 0;
          ri++;
        }
      }
    }
  }
  __syncthreads();

  // ---- the passes.  A thread takes 8 consecutive samples of a row (or of a column) together
  // with a halo of 4 on each side into registers (lift16) and writes only its 8 results back.
  // Rows are independent in the x pass and columns in the y pass, so one round handles whole rows
  // (columns): all loads of a round precede its stores.
  const uint32_t nseg = (cx + kSeg - 1) / kSeg;
  auto lift_x = [&](uint32_t jlo, uint32_t jhi) {          // staged rows [jlo, jhi), in place
    // lanes of a wavefront take different rows: addresses differ by the (odd) row stride
    const uint32_t rpr = min(32u, (uint32_t)kXYThreads / nseg);
    const uint32_t l = tid % rpr, sg = tid / rpr;
    for (uint32_t rb = jlo; rb < jhi; rb += rpr) {
      const bool on = sg < nseg && rb + l < jhi;
      double* row = sm + (size_t)(rb + l) * RS;
      const int s = (int)(sg * kSeg);
      double r[16];
      if (on) {
        if (s >= 4 && s + 12 <= (int)cx) {
#pragma unroll
          for (int k = 0; k < 16; k++)
            r[k] = row[s - 4 + k];
        }
        else {
#pragma unroll
          for (int k = 0; k < 16; k++)
            r[k] = row[reflect_index(s - 4 + k, (int)cx)];
        }
        lift16<FORWARD>(r, K);
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int k = 0; k < kSeg; k++)
          if ((uint32_t)(s + k) < cx)
            row[s + k] = r[4 + k];
      }
      __syncthreads();
    }
  };

  // y direction: thread = (column, 8 rows of the tile); lanes take consecutive columns
  const uint32_t nq = (yend - y0 + kSeg - 1) / kSeg;
  const uint32_t cpr = (uint32_t)kXYThreads / nq;          // columns per round
  auto load_column = [&](uint32_t x, uint32_t q, double (&r)[16]) {
    const int s = (int)(y0 + q * kSeg);
    const double* col = sm + x;
    if (s - 4 >= (int)ylo && s + 12 <= (int)yhi) {   // all 16 rows are staged rows of the slice
      const double* top = col + (size_t)(s - 4 - (int)ylo) * RS;
#pragma unroll
      for (int k = 0; k < 16; k++)
        r[k] = top[(size_t)k * RS];
    }
    else {
#pragma unroll
      for (int k = 0; k < 16; k++) {
        // rows outside the slice mirror into it; what lies outside the staged rows is clamped
        // into them: it cannot reach the tile's own rows (see above)
        const uint32_t yy = min(max(reflect_index(s - 4 + k, (int)cy), ylo), yhi - 1);
        r[k] = col[(size_t)(yy - ylo) * RS];
      }
    }
  };

  if (FORWARD) {
    lift_x(0, nrow);
    // y pass straight from LDS into the buffer: low | high halves along both axes
    for (uint32_t xb = 0; xb < cx; xb += cpr) {
      const uint32_t x = xb + tid % cpr, q = tid / cpr;
      if (x < cx && q < nq) {
        double r[16];
        load_column(x, q, r);
        lift16<true>(r, K);
        const uint32_t dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
#pragma unroll
        for (int k = 0; k < kSeg; k++) {
          const uint32_t y = y0 + q * kSeg + k;
          if (y < yend)
            buf[(size_t)((y & 1) ? ye + (y >> 1) : (y >> 1)) * cx + dcol] = r[4 + k];
        }
      }
    }
  }
  else {
    for (uint32_t xb = 0; xb < cx; xb += cpr) {
      const uint32_t x = xb + tid % cpr, q = tid / cpr;
      const bool on = x < cx && q < nq;
      double r[16];
      if (on) {
        load_column(x, q, r);
        lift16<false>(r, K);
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int k = 0; k < kSeg; k++) {
          const uint32_t y = y0 + q * kSeg + k;
          if (y < yend)
            sm[(size_t)(y - ylo) * RS + x] = r[4 + k];
        }
      }
    }
    __syncthreads();
    lift_x(y0 - ylo, yend - ylo);   // (only the tile's own rows go on)
    if constexpr (kCrop) {
      for (uint32_t y = wy0 + wave; y < wy1; y += nwaves) {
        VT* dstrow = vol + out_at(wx0, y);   // (any x origin: one sample per lane)
        const double* srow = sm + (size_t)(y - ylo) * RS;
        for (uint32_t x = wx0 + lane; x < wx1; x += 64)
          dstrow[x - wx0] = (VT)(srow[x] + mean);
      }
    }
    else
    for (uint32_t y = y0 + wave; y < yend; y += nwaves) {
      VT* dstrow = vol + vbase + (size_t)y * vsy;
      const double* srow = sm + (size_t)(y - ylo) * RS;
      for (uint32_t x = lane; x < cx; x += 64)
        dstrow[x] = (VT)(srow[x] + mean);
    }
  }
}

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
constexpr int kL2MaxRow = 128;
constexpr int kL2PosF = (kXYZRows * kL2MaxRow + kXYZThreadsF - 1) / kXYZThreadsF;
constexpr int kL2StageF = (kXYZStaged * kL2MaxRow + kXYZThreadsF - 1) / kXYZThreadsF;
constexpr int kL2PosI = (kXYZStaged * kL2MaxRow + kXYZThreadsI - 1) / kXYZThreadsI;
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

// SG: the coefficients carry their sign where the chunk allows it (DequantSrc::coefSigned, coef_scheme), a kernel of its own -- with both fast paths in
// one function the register allocator spilled inside the slice loop (88 registers against 38) and the kernel took 5.4 ms
// instead of 3.7
// kCrop: the rows of the chunk's window go to the box; a tile with no row in the window returns at once
// The body of the inverse kernels.  NPOS: positions per thread (kXYZStaged * cx <= NPOS * threads).
// L2: the second level (k_lift2_inv) -- `volume` is the chunk's own output box (rows and slices as `vd` says, no chunk
// map, nothing written for a constant chunk), and the coefficient, sign and mask arrays, which keep the CHUNK's dims, have
// rows of `qrowL2` samples and slices of `qsliceL2`; otherwise they are the region's, cx and cx * cy.
template <int IO, bool SG, bool kCrop, int NPOS, bool L2>
__device__ __forceinline__ void xyz_inv_body(const double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz,
                                             const LiftConsts& K, const CoderState* st, void* volume, const VolDesc& vd,
                                             const GeomOf<kCrop>* geom, const LiftFuse& F, uint32_t nseg, uint32_t qrowL2,
                                             size_t qsliceL2)
{
  static_assert(IO == 1 || IO == 2, "float or double volume");
  static_assert(!L2 || (IO == 2 && !kCrop), "the second level writes doubles into a box");
  constexpr int NGRP = NPOS < kXYZGroupI ? NPOS : kXYZGroupI;   // positions whose loads are in flight together
  using VT = typename std::conditional<IO == 1, float, double>::type;
  const uint32_t c = blockIdx.y;
  const uint32_t tid = threadIdx.x;
  // (small batches: `nseg` workgroups per tile share the slices, see k_lift_xyz_fwd; segment g finishes
  //  the slices that the pairs [mA, mB) complete, the last one also the end of the lines, and runs
  //  its pipelines six pairs ahead of that)
  const uint32_t seg = blockIdx.x % nseg, npairsAll = cz / 2;
  const uint32_t mA = seg == 0 ? 0u : (uint32_t)((uint64_t)npairsAll * seg / nseg);
  const uint32_t mB = seg + 1 == nseg ? npairsAll : (uint32_t)((uint64_t)npairsAll * (seg + 1) / nseg);
  const uint32_t mFirst = mA >= 6 ? mA - 6 : 0u;
  const uint32_t y0 = (blockIdx.x / nseg) * kXYZRows;
  const uint32_t nt = min((uint32_t)kXYZRows, cy - y0);
  const uint32_t RS = xyz_row_stride(cx);
  double* sm = reinterpret_cast<double*>(dyn_smem);
  const uint32_t bufN = (uint32_t)kXYZStaged * RS;
  const uint32_t xe = cx - cx / 2, ye = cy - cy / 2, ze = cz - cz / 2;
  VT* vol = reinterpret_cast<VT*>(volume);
  const size_t vsy = vd.dims[0], vsz = (size_t)vd.dims[0] * vd.dims[1];
  VT* volc = vol;
  CropGeom cg{};
  uint32_t wy0 = 0, wy1 = 0;   // crop variant: the tile's rows [y0 + wy0, y0 + wy1) lie in the window
  if constexpr (kCrop) {   // (uniform)
    cg = geom[c];
    wy0 = max(y0, cg.lo[1]) - y0;
    wy1 = min(y0 + nt, cg.hi[1]);
    if (y0 + wy0 >= wy1)
      return;
    wy1 -= y0;
  }
  else if constexpr (!L2)
    volc = vol + ((size_t)geom[c].org[2] * vsz + (size_t)geom[c].org[1] * vsy + geom[c].org[0]);
  // crop variant: row y0 + r of slice z -> the box row that holds its window, x = wx0 at its start
  auto crop_row = [&](uint32_t z, uint32_t r) -> VT* { return vol + crop_addr(cg, vd, cg.lo[0], y0 + r, z); };
  (void)crop_row;
  const double* buf = vals + c * valsStride;
  const uint32_t qrow = L2 ? qrowL2 : cx;                    // the coefficient arrays' rows and slices
  const size_t sliceN = L2 ? qsliceL2 : (size_t)cx * cy;
  const uint32_t bufx = F.bufx ? F.bufx : cx;                       // the chunk buffer may be compact:
  const size_t bufSlice = (size_t)bufx * (F.bufy ? F.bufy : cy);   // only the next level's box
  const double mean = st[c].mean;
  const uint32_t lane = tid & 63u, nwaves = kXYZThreadsI / 64;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (a scalar, and what is made of it)

  if constexpr (!L2) {   // (k_lift2_inv has returned for a constant chunk)
  if (st[c].is_const != 0) {   // the chunk is its constant
    if constexpr (kCrop) {
      const uint32_t w = cg.hi[0] - cg.lo[0], nr = wy1 - wy0;
      for (uint32_t z = cg.lo[2] + seg; z < cg.hi[2]; z += nseg)
        for (uint32_t k = tid; k < nr * w; k += kXYZThreadsI)
          crop_row(z, wy0 + k / w)[k % w] = (VT)mean;
    }
    else
    for (uint32_t z = seg; z < cz; z += nseg)
      for (uint32_t k = tid; k < nt * cx; k += kXYZThreadsI)
        volc[(size_t)z * vsz + (size_t)(y0 + k / cx) * vsy + k % cx] = (VT)mean;
    return;
  }
  }

  // position k of this thread: sample x of LDS row j = row ysrc of a slice (j << 27 | ysrc << 12 | x);
  // in the transformed chunk that is sample (dcol, drow): low | high halves along x and y
  const uint32_t npos = (uint32_t)kXYZStaged * cx;
  uint32_t pk[NPOS];
  uint32_t innerMask = 0;   // bit k: inside the next level's box along x and y
#pragma unroll
  for (int k = 0; k < NPOS; k++) {
    const uint32_t q = tid + (uint32_t)k * kXYZThreadsI;
    const uint32_t j = q / cx, x = q - j * cx, y = reflect_index((int)y0 - kXYHalo + (int)j, (int)cy);
    const uint32_t drow = (y & 1) ? ye + (y >> 1) : (y >> 1), dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
    pk[k] = (j << 27) | (y << 12) | x;
    if (dcol < F.inner[0] && drow < F.inner[1])
      innerMask |= 1u << k;
  }
  const bool dequant = F.mode == 2 && !st[c].wide;
  const double fq = dequant ? st[c].q : 0.0;
  const DequantSrc& Q = F.src;
  const uint32_t* coef = Q.coefs<uint32_t>(c);
  const uint64_t* sign = Q.sign + c * Q.signStride;
  // a coefficient that became significant on the last decoded plane / the one before and was never refined still
  // holds 0: its value comes from the decoder's masks.  (Without masks the rule completes nothing: the mask words
  // read are the sign's then, whatever they hold.)
  const bool haveMasks = dequant && Q.has_masks();
  const uint64_t* mNew = haveMasks ? Q.sigNew + c * Q.maskStride : sign;
  const uint64_t* mOld = haveMasks ? Q.sigOld + c * Q.maskStride : sign;
  // SG: the sign in bit 31, the value complete (k_ref_assemble, DequantSrc::coefSigned): neither the sign nor the mask
  // words are read (scheme 0: this chunk keeps magnitudes and masks)
  const DequantRule<uint32_t> rule = dequant_rule<uint32_t>(fq, haveMasks, haveMasks ? Q.dst + c : nullptr, SG);
  const int scheme = rule.scheme;
  auto sg_value = [&](uint32_t sv) -> double { return dequant_signed(rule, sv); };
  // sample (dcol, drow, zp): straight from the decoder (dequant.h) unless a coarser level's passes have produced it
  auto fetch = [&](int k, uint32_t zp) -> double {
    const uint32_t y = (pk[k] >> 12) & 0x7fffu, x = pk[k] & 0xfffu;
    const uint32_t drow = (y & 1) ? ye + (y >> 1) : (y >> 1), dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
    const size_t idx = (size_t)zp * sliceN + drow * qrow + dcol;
    const bool inBox = ((innerMask >> k) & 1u) && zp < F.inner[2];
    if (!dequant && !inBox && F.bufx)
      return 0.0;   // (a compact buffer holds the box only; the host asks for one only when every chunk dequantises here)
    if (dequant && !inBox) {
      if (SG && scheme)
        return sg_value(coef[idx]);
      const uint32_t v = coef[idx];
      const uint32_t sh = (uint32_t)(idx & 63);
      const uint64_t sgw = sign[idx >> 6], mnw = mNew[idx >> 6], mow = mOld[idx >> 6];   // (independent loads)
      return dequant_masks(rule, v, mnw, mow, sgw, sh);
    }
    return buf[(size_t)zp * bufSlice + drow * bufx + dcol];
  };
  // The slice of z-inverted samples staged in X (all staged rows) -> y pass into Y, x pass into the volume (kDirect,
  // see finish_slice) or, the box variant, back into X and from there into the box: X and Y then swap from slice
  // to slice, three barriers per slice.
  uint32_t flip = 0;
  // sample k of the slice that is finished next (its staging buffer is free: see finish_slice)
  auto stage = [&](int k, double v) {
    uint32_t p = pk[k];
    asm volatile("" : "+v"(p));   // (keeps the LDS address from being computed ahead and spilled)
    (sm + (flip ? bufN : 0u))[(p >> 27) * RS + 4 + (p & 0xfffu)] = v;
  };
  auto stage_all = [&](const double (&v)[NPOS]) {
#pragma unroll
    for (int k = 0; k < NPOS; k++)
      if ((tid + (uint32_t)k * kXYZThreadsI) < npos)
        stage(k, v[k]);
  };
  // rows of a finished slice (in staging buffer `which`) -> volume, mean added, narrowed
  auto store_rows = [&](uint32_t z, uint32_t which) {
    const double* X = sm + (which ? bufN : 0u);
    // (the lane's addresses are made anew for every slice: computed once, ahead of the loop, they are spilled, and a
    //  reload here waits for every load and store in flight)
    uint32_t lanev = lane;
    asm volatile("" : "+v"(lanev));
    if constexpr (kCrop) {   // (any x origin: one sample per lane)
      if (z - cg.lo[2] >= cg.hi[2] - cg.lo[2])
        return;
      for (uint32_t r = wy0 + wave; r < wy1; r += nwaves) {
        VT* dstrow = crop_row(z, r);
        const double* srow = X + (size_t)(kXYHalo + r) * RS + 4;
        for (uint32_t x = cg.lo[0] + lanev; x < cg.hi[0]; x += 64)
          dstrow[x - cg.lo[0]] = (VT)(F.noMean ? srow[x] : srow[x] + mean);
      }
      return;
    }
    if (xyz_off<XYZ_INV_OFF>(4, nseg))
      return;
    for (uint32_t r = wave; r < nt; r += nwaves) {
      VT* dstrow = volc + (size_t)z * vsz + (size_t)(y0 + r) * vsy;
      const double* srow = X + (size_t)(kXYHalo + r) * RS + 4;
      if (F.noMean) {   // (uniform)
        for (uint32_t x = lanev; x < cx; x += 64)
          dstrow[x] = (VT)srow[x];
      }
      else
        for (uint32_t x = lanev; x < cx; x += 64)
          dstrow[x] = (VT)(srow[x] + mean);
    }
  };
  // kDirect: the x pass writes the volume itself.  The slices are then all staged in the first buffer: its y pass has
  // read it when the barrier in front of the x pass is behind a wavefront, and the second buffer, which the x pass
  // reads, is written again only behind the next slice's first barrier.  Two barriers per slice.
  constexpr bool kDirect = !kCrop && XYZ_INV_XSTORE != 0;
  auto finish_slice = [&](uint32_t z) {
    uint32_t RSv = RS, tidv = tid;   // (see k_lift_xyz_fwd)
    asm volatile("" : "+s"(RSv), "+v"(tidv));
    const uint32_t which = flip;
    double* X = sm + (flip ? bufN : 0u);
    double* Y = sm + (flip ? 0u : bufN);
    if constexpr (!kDirect)
      flip ^= 1u;
    XYZ_LDS_BARRIER();
    if (!xyz_off<XYZ_INV_OFF>(2, nseg))
      xyz_lift_y<false, true, kXYZThreadsI, kXYZOutIY>(X, Y, RSv, cx, nt, tidv, K);
    XYZ_LDS_BARRIER();
    if constexpr (kDirect) {
      if (!xyz_off<XYZ_INV_OFF>(2, nseg))
        xyz_lift_x_store<kXYZThreadsI, kXYZOutIX>(Y, volc + (size_t)z * vsz + (size_t)y0 * vsy, vsy, RSv, cx, kXYHalo, kXYHalo + nt,
                                                   tidv, K, mean, F.noMean != 0, !xyz_off<XYZ_INV_OFF>(4, nseg));
      else   // (timing builds: the rows as they are)
        store_rows(z, which ^ 1u);
    }
    else {
      if (!xyz_off<XYZ_INV_OFF>(2, nseg))
        xyz_lift_x<false, kXYZThreadsI, kXYZOutIX>(Y, X, RSv, cx, kXYHalo, kXYHalo + nt, tidv, K);
      XYZ_LDS_BARRIER();
      store_rows(z, which);
      // (the next slice is staged into Y, which nobody reads any more; its y pass writes X only after
      //  the barrier behind that staging, when every row above has been stored)
    }
  };

  double o1p[NPOS], e1p[NPOS], o2p[NPOS], e2p[NPOS];
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    o1p[k] = e1p[k] = o2p[k] = e2p[k] = 0.0;
  const uint32_t npairs = cz / 2;
  // one pair (low[m], high[m]) of position k enters its pipeline; slice 2m-3's sample is staged
  auto zstep = [&](int k, uint32_t m, bool mine, bool active, double E, double O) {
    const double o1 = (-K.eps) * O;                                        // o1[m]
    const double t = K.delta * ((m == 0 ? o1 : o1p[k]) + o1);
    const double e1 = fma(E, K.inv_eps, -t);                               // e1[m]
    if (m >= 1) {
      const double o2 = fma(-K.gamma, e1p[k] + e1, o1p[k]);                // o2[m-1]
      const double e2 = fma(-K.beta, (m == 1 ? o2 : o2p[k]) + o2, e1p[k]); // e2[m-1]
      if (m >= 2 && mine && active)
        stage(k, fma(-K.alpha, e2p[k] + e2, o2p[k]));                      // o3[m-2]: slice 2m-3
      o2p[k] = o2;
      e2p[k] = e2;
    }
    o1p[k] = o1;
    e1p[k] = e1;
  };
#if XYZ_INV_PREFETCH == 2
  // Round 4.  The kernel spent half its time waiting for loads, one after the other: every sample's sign and
  // mask words sat behind a branch of their own (box or not), so a pair was some thirty-six dependent round
  // trips.  Now (chunks that dequantise here):
  //  * pair m + 1's coefficients travel from HBM straight into LDS (global_load_lds: no register holds them)
  //    while pair m's two slices go through the y and x passes; every wavefront has its own 64-dword row
  //    per (position, low / high half) behind the two staging buffers.  They are issued AFTER the pair's
  //    own loads: the memory counter retires in order, a wait for those would wait for these too;
  //  * the sign / mask dwords and the fp64 samples of the coarser levels' box (an eighth of all) are loaded
  //    without any branch -- a lane that does not need one reads a harmless address --, three positions'
  //    worth at a time: two round trips per pair.
  // The arithmetic per sample is what it was.
  uint32_t* myPre = reinterpret_cast<uint32_t*>(sm + 2 * (size_t)bufN) + (size_t)wave * (NPOS * 2 * 64);
  const uint32_t* sign32 = reinterpret_cast<const uint32_t*>(sign);
  const uint32_t* mNew32 = reinterpret_cast<const uint32_t*>(mNew);
  const uint32_t* mOld32 = reinterpret_cast<const uint32_t*>(mOld);
  uint32_t activeMask = 0;
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    if ((tid + (uint32_t)k * kXYZThreadsI) < npos)
      activeMask |= 1u << k;
    else
      pk[k] = pk[0];   // (a valid position: its loads are harmless, nothing of it is staged)
  uint32_t boxAny = 0;   // bit k: some lane of this wavefront has position k inside the coarser levels' box (along x and y)
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    boxAny |= __ballot((innerMask >> k) & 1u) != 0ull ? 1u << k : 0u;
  boxAny = (uint32_t)__builtin_amdgcn_readfirstlane((int)boxAny);
  auto pos_off = [&](int k, uint32_t& drow, uint32_t& dcol) {
    const uint32_t y = (pk[k] >> 12) & 0x7fffu, x = pk[k] & 0xfffu;
    drow = (y & 1) ? ye + (y >> 1) : (y >> 1);
    dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
  };
  // (a high-half sample never lies in the next level's box when that box ends at or before the low half)
  const bool fastLoads = dequant && F.inner[2] <= ze && (!SG || scheme != 0);
  // The fp64 samples of the coarser levels' box THROUGH LDS as well (sign-in-word kernel, round 5): where the lanes of
  // a wavefront that are in the box are exactly its even ones -- rows of a multiple of 64 samples: 32 doubles in a row
  // of the chunk buffer --, the 256 bytes travel like a row of coefficients, a pair ahead (lane i fetches dword i),
  // and lane 2 i reads double i.  Two load round trips per pair in half the wavefronts, with the other half waiting
  // for them at the barrier, before.  A slot per (wavefront, position) that has a box row: 12 rows x cx / 64 <= 48.
  uint32_t boxLds = 0, boxSlot0 = 0;   // (wave-uniform) bit k: position k's box samples come through LDS; the wavefront's first slot
  uint32_t* boxRows = reinterpret_cast<uint32_t*>(sm + 2 * (size_t)bufN) + (size_t)nwaves * (NPOS * 2 * 64);
  if (SG && fastLoads) {
    uint32_t reg = 0;
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      const uint64_t inb = __ballot((innerMask >> k) & 1u), act = __ballot((activeMask >> k) & 1u);
      if (inb == 0x5555555555555555ull && act == ~0ull && (cx & 63u) == 0)
        reg |= 1u << k;
    }
    reg = (uint32_t)__builtin_amdgcn_readfirstlane((int)reg);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(sm);   // (the staging buffers are not in use yet)
    if (lane == 0)
      cnt[wave] = (uint32_t)__popc(reg);
    XYZ_LDS_BARRIER();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < nwaves; w++) {
      const uint32_t v = cnt[w];
      before += w < wave ? v : 0u;
      total += v;
    }
    XYZ_LDS_BARRIER();
    if (total <= (uint32_t)kXYZBoxSlots && reg == (1u << NPOS) - 1u) {   // (all of the wavefront's positions or none)
      boxLds = reg;
      boxSlot0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
    }
  }
  uint32_t* myBox = boxRows + (size_t)boxSlot0 * 64;   // position k's row: myBox + k * 64
  auto pre_issue = [&](uint32_t m) {
    if (xyz_off<XYZ_INV_OFF>(1, nseg))
      return;
    // (the box rows first: what their addresses are made of may have to come back from scratch, and behind the
    //  coefficients' loads that reload would wait for every one of them -- the memory counter retires in order)
    if (SG && boxLds != 0 && m < F.inner[2]) {   // (uniform)
#pragma unroll
      for (int k = 0; k < NPOS; k++) {
        uint32_t drow, dcol;
        pos_off(k, drow, dcol);
        const uint32_t x0h = ((pk[k] & 0xfffu) - lane) >> 1;   // the box column of the wavefront's first lane
        const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + ((size_t)m * bufSlice + (size_t)drow * bufx + x0h)) + lane;
        __builtin_amdgcn_global_load_lds(src, myBox + k * 64, 4, 0, 0);
      }
    }
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      uint32_t drow, dcol;
      pos_off(k, drow, dcol);
      const uint32_t off = drow * qrow + dcol;
      __builtin_amdgcn_global_load_lds(coef + ((size_t)m * sliceN + off), myPre + (k * 2) * 64, 4, 0, 0);
      __builtin_amdgcn_global_load_lds(coef + ((size_t)(ze + m) * sliceN + off), myPre + (k * 2 + 1) * 64, 4, 0, 0);
    }
  };
  if (fastLoads && mFirst < mB)
    pre_issue(mFirst);
#endif
  for (uint32_t m = mFirst; m < mB; m++) {
    const bool mine = m >= mA;   // (else: the segment's run-up)
#pragma unroll
    for (int k = 0; k < NPOS; k++)
      asm volatile("" : "+v"(pk[k]));
#if XYZ_INV_PREFETCH == 2
    if (SG && fastLoads) {
      // (round 5) the coefficients carry their sign and are complete: a pair's global loads are the fp64 samples of
      // the coarser levels' box alone -- and only in the wavefronts that have a lane in the box (with 256 samples a
      // row: those whose rows are the even ones)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this pair's coefficients have landed in LDS (and its box rows)
      const bool boxWave = boxAny != 0 && m < F.inner[2];   // (uniform)
      const bool zOn = !xyz_off<XYZ_INV_OFF>(8, nseg);
      if (zOn && boxWave && boxLds != 0) {   // the box samples were prefetched with the coefficients
#pragma unroll
        for (int k = 0; k < NPOS; k++) {
          const double lo = sg_value(myPre[(k * 2) * 64 + lane]);
          const double hi = sg_value(myPre[(k * 2 + 1) * 64 + lane]);
          const double bxv = reinterpret_cast<const double*>(myBox + k * 64)[lane >> 1];
          zstep(k, m, mine, true, (lane & 1u) ? lo : bxv, hi);   // (the even lanes are the ones in the box)
        }
      }
      else if (zOn) {
#pragma unroll
      for (int g = 0; g < NPOS; g += NGRP) {
        __builtin_amdgcn_sched_barrier(0);   // (NGRP positions' loads in flight at a time)
        double bx[NGRP];
        uint32_t boxm = 0;
        if (boxWave) {
#pragma unroll
          for (int kk = 0; kk < NGRP; kk++) {
            const int k = g + kk;
            if (k >= NPOS)
              continue;
            uint32_t drow, dcol;
            pos_off(k, drow, dcol);
            const bool inBox = ((innerMask >> k) & 1u) != 0;
            boxm |= inBox ? 1u << kk : 0u;
            bx[kk] = buf[inBox ? (size_t)m * bufSlice + drow * bufx + dcol : (size_t)0];
          }
        }
#pragma unroll
        for (int kk = 0; kk < NGRP; kk++) {
          const int k = g + kk;
          if (k >= NPOS)
            continue;
          const double lo = sg_value(myPre[(k * 2) * 64 + lane]);
          const double hi = sg_value(myPre[(k * 2 + 1) * 64 + lane]);
          zstep(k, m, mine, ((activeMask >> k) & 1u) != 0, ((boxm >> kk) & 1u) ? bx[kk] : lo, hi);
        }
      }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (m + 1 < mB)
        pre_issue(m + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    else if (!SG && fastLoads) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this pair's coefficients have landed in LDS
#pragma unroll
      for (int g = 0; g < NPOS; g += NGRP) {
        __builtin_amdgcn_sched_barrier(0);   // (NGRP positions' loads in flight at a time)
        constexpr int NV = 2 * NGRP;
        uint32_t sgw[NV], mnw[NV], mow[NV], cv[NV], shv[NV], boxm = 0;
        double bx[NGRP];   // (only a low-half sample can lie in the box: fastLoads)
#pragma unroll
        for (int j = 0; j < NV; j++) {
          const int k = g + j / 2;
          if (k >= NPOS)
            continue;
          const uint32_t zp = (j & 1) ? ze + m : m;
          uint32_t drow, dcol;
          pos_off(k, drow, dcol);
          const size_t idx = (size_t)zp * sliceN + drow * qrow + dcol;
          sgw[j] = sign32[idx >> 5];
          mnw[j] = mNew32[idx >> 5];
          mow[j] = mOld32[idx >> 5];
          if ((j & 1) == 0) {
            const bool inBox = ((innerMask >> k) & 1u) && zp < F.inner[2];
            boxm |= inBox ? 1u << j : 0u;
            bx[j / 2] = buf[inBox ? (size_t)zp * bufSlice + drow * bufx + dcol : (size_t)0];
          }
          cv[j] = myPre[(k * 2 + (j & 1)) * 64 + lane];
          shv[j] = (uint32_t)idx & 31u;
        }
        double val[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) {
          if (g + j / 2 >= NPOS)
            continue;
          const double dq = dequant_masks(rule, cv[j], mnw[j], mow[j], sgw[j], shv[j]);
          val[j] = ((j & 1) == 0 && ((boxm >> j) & 1u)) ? bx[j / 2] : dq;
        }
#pragma unroll
        for (int kk = 0; kk < NGRP; kk++)
          if (g + kk < NPOS)
            zstep(g + kk, m, mine, ((activeMask >> (g + kk)) & 1u) != 0, val[2 * kk], val[2 * kk + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (m + 1 < mB)
        pre_issue(m + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    else
#endif
    {
#pragma unroll
      for (int k = 0; k < NPOS; k++) {
        if ((k % 3) == 0)
          __builtin_amdgcn_sched_barrier(0);   // (four positions' loads in flight at a time, not all twelve)
        if ((tid + (uint32_t)k * kXYZThreadsI) >= npos)
          continue;
        const double E = fetch(k, m), O = fetch(k, ze + m);
        zstep(k, m, mine, true, E, O);
      }
    }
    if (m >= 2 && mine)
      finish_slice(2 * m - 3);
    if (m >= 1 && mine) {
      stage_all(e2p);
      finish_slice(2 * m - 2);
    }
  }
  // ---- the end of the lines (the last segment's)
  if (seg + 1 != nseg)
    return;
  if ((cz & 1) == 0) {   // pairs 0 .. M, M = cz / 2 - 1
    const uint32_t M = npairs - 1;
    double outC[NPOS];
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      outC[k] = 0.0;
      if ((tid + (uint32_t)k * kXYZThreadsI) >= npos)
        continue;
      const double o2 = fma(-K.gamma, e1p[k] + e1p[k], o1p[k]);              // o2[M]
      const double e2 = fma(-K.beta, o2p[k] + o2, e1p[k]);                   // e2[M]
      stage(k, fma(-K.alpha, e2p[k] + e2, o2p[k]));                          // o3[M-1]: slice 2M-1
      e2p[k] = e2;                                                           // slice 2M
      outC[k] = fma(-K.alpha, e2 + e2, o2);                                  // o3[M]: slice 2M+1
    }
    finish_slice(2 * M - 1);
    stage_all(e2p);
    finish_slice(2 * M);
    stage_all(outC);
    finish_slice(2 * M + 1);
  }
  else {                 // pairs 0 .. M-1 and the lone even sample low[M], M = cz / 2
    const uint32_t M = npairs;
    double outC[NPOS], outD[NPOS];
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      outC[k] = outD[k] = 0.0;
      if ((tid + (uint32_t)k * kXYZThreadsI) >= npos)
        continue;
      const double E = fetch(k, M);
      const double t = K.delta * (o1p[k] + o1p[k]);
      const double e1 = fma(E, K.inv_eps, -t);                               // e1[M]
      const double o2 = fma(-K.gamma, e1p[k] + e1, o1p[k]);                  // o2[M-1]
      const double e2 = fma(-K.beta, o2p[k] + o2, e1p[k]);                   // e2[M-1]
      stage(k, fma(-K.alpha, e2p[k] + e2, o2p[k]));                          // o3[M-2]: slice 2M-3
      e2p[k] = e2;                                                           // slice 2M-2
      const double e2L = fma(-K.beta, o2 + o2, e1);                          // e2[M]: slice 2M
      outC[k] = fma(-K.alpha, e2 + e2L, o2);                                 // o3[M-1]: slice 2M-1
      outD[k] = e2L;
    }
    finish_slice(2 * M - 3);
    stage_all(e2p);
    finish_slice(2 * M - 2);
    stage_all(outC);
    finish_slice(2 * M - 1);
    stage_all(outD);
    finish_slice(2 * M);
  }
}

template <int IO, bool SG, bool kCrop = false>
__global__ void __launch_bounds__(kXYZThreadsI) __attribute__((amdgpu_waves_per_eu(kXYZThreadsI / 256, kXYZThreadsI / 256)))
k_lift_xyz_inv(const double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz, LiftConsts K,
               const CoderState* st, void* volume, VolDesc vd, const GeomOf<kCrop>* geom, LiftFuse F, uint32_t nseg)
{
  xyz_inv_body<IO, SG, kCrop, kXYZPosI, false>(vals, valsStride, cx, cy, cz, K, st, volume, vd, geom, F, nseg, 0u, 0);
}

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

LiftConsts lift_consts()
{
  // include/CDF97.h:136-147 evaluated in IEEE fp64 (bit patterns: SURVEY.md Appendix B)
  auto bits = [](uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
  };
  LiftConsts k;
  k.alpha = bits(0xbff960ce676352c0ull);
  k.beta = bits(0xbfab2035c938c1f9ull);
  k.gamma = bits(0x3fec40ceba5579b7ull);
  k.delta = bits(0x3fdc626a9045727dull);
  k.eps = bits(0x3ff264c795071559ull);
  k.inv_eps = bits(0x3febd5edf975cca4ull);
  return k;
}

// Lines per tile.  The kernel is HBM-bound and synchronises between lifting steps, so it wants
// several workgroups per CU: measured on MI355X (256-sample lines) 8 lines per tile are best along
// x, where a wavefront reads along the line, and 16 across (128-byte rows); larger tiles halve the
// throughput.
static int pick_nl(uint32_t len, int axis, size_t* smem)
{
  // (measured again with the dequantising inverse passes, SPERR_HIP_LIFT_LDS_KB: 20 / 36 / 72 KB
  //  along y and z give 9.1 / 8.3 / 11.5 ms for the 13 inverse passes of the bench volume)
  static const int capYZ = tune_getenv("SPERR_HIP_LIFT_LDS_KB") ? atoi(tune_getenv("SPERR_HIP_LIFT_LDS_KB")) : 36;
  const size_t cap = (size_t)(axis == 0 ? 20 : capYZ) * 1024;
  for (int nl = 32; nl >= 1; nl >>= 1) {
    const size_t bytes = (size_t)len * (nl + 1) * sizeof(double);
    if (bytes <= cap || nl == 1) {
      *smem = bytes;
      return nl;
    }
  }
  return 1;
}

int launch_lift(hipStream_t stream, bool forward, double* vals, size_t valsStride,
                uint32_t nchunks, const uint32_t cdims[3], int axis, const uint32_t region[3],
                CoderState* st, int io, void* volume, VolDesc vd, const ChunkGeom* geom,
                const LiftFuse* fuse, const CropGeom* crop)
{
  const LiftFuse F = fuse ? *fuse : LiftFuse{};
  if (crop && (forward || io == 0))
    return -1;
  {
    const void* fns[8] = {reinterpret_cast<const void*>(&k_lift_axis<true, 0>),
                          reinterpret_cast<const void*>(&k_lift_axis<true, 1>),
                          reinterpret_cast<const void*>(&k_lift_axis<true, 2>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 0>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 1>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 2>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 1, true>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 2, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const uint32_t len = region[axis];
  if (len < 2)
    return io ? -1 : 0;
  size_t smem = 0;
  const int NL = pick_nl(len, axis, &smem);
  if (smem > 160 * 1024) {
    fprintf(stderr, "[sperr_hip] line of %u samples does not fit in LDS\n", len);
    return -1;
  }
  const int ua = (axis == 0) ? 1 : 0, wa = (axis == 2) ? 1 : 2;
  const uint32_t ntu = (region[ua] + NL - 1) / NL;
  dim3 grid(ntu * region[wa], nchunks);
  const LiftConsts K = lift_consts();
#define LIFT_ARGS vals, valsStride, cdims[0], cdims[1], axis, region[0], region[1], region[2], NL, K, st, volume, vd, geom, F
  if (forward) {
    if (io == 1)
      LAUNCH_K((k_lift_axis<true, 1>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else if (io == 2)
      LAUNCH_K((k_lift_axis<true, 2>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else
      LAUNCH_K((k_lift_axis<true, 0>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
  }
  else if (crop) {
#define CROP_ARGS vals, valsStride, cdims[0], cdims[1], axis, region[0], region[1], region[2], NL, K, st, volume, vd, crop, F
    if (io == 1)
      LAUNCH_K((k_lift_axis<false, 1, true>), grid, dim3(kThreads), smem, stream, CROP_ARGS);
    else
      LAUNCH_K((k_lift_axis<false, 2, true>), grid, dim3(kThreads), smem, stream, CROP_ARGS);
#undef CROP_ARGS
  }
  else {
    if (io == 1)
      LAUNCH_K((k_lift_axis<false, 1>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else if (io == 2)
      LAUNCH_K((k_lift_axis<false, 2>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else
      LAUNCH_K((k_lift_axis<false, 0>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
  }
#undef LIFT_ARGS
  HIP_CHECK(hipGetLastError());
  return 0;
}

// rows per tile of k_lift_xy for rows of cx samples, 0 when the fused kernel does not apply
static int xy_rows(uint32_t cx, uint32_t cy)
{
  if (cx < 2 || cy < 2)
    return 0;
  const size_t rowBytes = (size_t)(cx + 1) * sizeof(double);
  static const int ldsKB = tune_getenv("SPERR_HIP_XY_LDS_KB") ? atoi(tune_getenv("SPERR_HIP_XY_LDS_KB")) : 68;
  static const int maxRows = tune_getenv("SPERR_HIP_XY_ROWS") ? atoi(tune_getenv("SPERR_HIP_XY_ROWS")) : 32;
  int rows = (int)(((size_t)ldsKB * 1024) / rowBytes);
  if (rows > maxRows)
    rows = maxRows;
  int R = (rows - 2 * kXYHalo) & ~1;
  if (R <= 0)   // (rows of 1088 samples and more leave no tile: a negative R must not pass for a large one below)
    return 0;
  if ((uint32_t)R > cy)
    R = (int)((cy + 1) & ~1u);
  return R >= 8 ? R : 0;
}

bool lift_xy_applicable(const uint32_t cdims[3])
{
  return xy_rows(cdims[0], cdims[1]) > 0;
}

int launch_lift_xy(hipStream_t stream, bool forward, double* vals, size_t valsStride,
                   uint32_t nchunks, const uint32_t cdims[3], const CoderState* st, int io,
                   void* volume, VolDesc vd, const ChunkGeom* geom, const CropGeom* crop)
{
  if (crop && forward)
    return -1;
  {
    const void* fns[6] = {reinterpret_cast<const void*>(&k_lift_xy<true, 1>),
                          reinterpret_cast<const void*>(&k_lift_xy<true, 2>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 1>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 2>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 1, true>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 2, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const int R = xy_rows(cdims[0], cdims[1]);
  if (R <= 0 || (io != 1 && io != 2))
    return -1;
  const size_t smem = (size_t)(R + 2 * kXYHalo) * (cdims[0] + 1) * sizeof(double);
  const uint32_t ntile = (cdims[1] + R - 1) / R;
  const dim3 grid(ntile * cdims[2], nchunks);
  const LiftConsts K = lift_consts();
#define XY_ARGS vals, valsStride, cdims[0], cdims[1], cdims[2], R, K, st, volume, vd, geom
  if (forward) {
    if (io == 1)
      LAUNCH_K((k_lift_xy<true, 1>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
    else
      LAUNCH_K((k_lift_xy<true, 2>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
  }
  else if (crop) {
#define CROP_ARGS vals, valsStride, cdims[0], cdims[1], cdims[2], R, K, st, volume, vd, crop
    if (io == 1)
      LAUNCH_K((k_lift_xy<false, 1, true>), grid, dim3(kXYThreads), smem, stream, CROP_ARGS);
    else
      LAUNCH_K((k_lift_xy<false, 2, true>), grid, dim3(kXYThreads), smem, stream, CROP_ARGS);
#undef CROP_ARGS
  }
  else {
    if (io == 1)
      LAUNCH_K((k_lift_xy<false, 1>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
    else
      LAUNCH_K((k_lift_xy<false, 2>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
  }
#undef XY_ARGS
  HIP_CHECK(hipGetLastError());
  return 0;
}

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
static uint32_t xyz_segments(uint32_t ntile, uint32_t nchunks, uint32_t cz)
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
  size_t smem = 2 * (size_t)kXYZStaged * xyz_row_stride(cdims[0]) * sizeof(double);   // two staging buffers
#if XYZ_INV_PREFETCH == 2
  if (!forward)
    smem += (size_t)kXYZThreadsI * kXYZPosI * 2 * sizeof(uint32_t) +   // + the coefficients on their way in
            (size_t)kXYZBoxSlots * 64 * sizeof(uint32_t);              //   and the box samples (k_lift_xyz_inv<.., true>)
#endif
  {
    const void* fns[10] = {reinterpret_cast<const void*>(&k_lift_xyz_fwd<1>), reinterpret_cast<const void*>(&k_lift_xyz_fwd<2>),
                           reinterpret_cast<const void*>(&k_lift_xyz_inv<1, false>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, false>),
                           reinterpret_cast<const void*>(&k_lift_xyz_inv<1, true>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, true>),
                           reinterpret_cast<const void*>(&k_lift_xyz_inv<1, false, true>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, false, true>),
                           reinterpret_cast<const void*>(&k_lift_xyz_inv<1, true, true>), reinterpret_cast<const void*>(&k_lift_xyz_inv<2, true, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const uint32_t ntile = (cdims[1] + kXYZRows - 1) / kXYZRows;
  const uint32_t nseg = xyz_segments(ntile, nchunks, cdims[2]);
  const dim3 grid(ntile * nseg, nchunks);
  const LiftConsts K = lift_consts();
  if (forward) {
    const int wantMax = F.mode == 1 ? 1 : 0;
    if (io == 1)
      LAUNCH_K((k_lift_xyz_fwd<1>), grid, dim3(kXYZThreadsF), smem, stream, vals, valsStride, cdims[0], cdims[1],
               cdims[2], K, st, volume, vd, geom, wantMax, F.inner[0], F.inner[1], F.inner[2], nseg, box, boxStride);
    else
      LAUNCH_K((k_lift_xyz_fwd<2>), grid, dim3(kXYZThreadsF), smem, stream, vals, valsStride, cdims[0], cdims[1],
               cdims[2], K, st, volume, vd, geom, wantMax, F.inner[0], F.inner[1], F.inner[2], nseg, box, boxStride);
  }
  else {
    const bool sg = F.mode == 2 && F.src.coefSigned != 0;
#define XYZ_INV_LAUNCH(io_, sg_)                                                                                    \
  LAUNCH_K((k_lift_xyz_inv<io_, sg_>), grid, dim3(kXYZThreadsI), smem, stream, vals, valsStride, cdims[0], cdims[1], \
           cdims[2], K, st, volume, vd, geom, F, nseg)
#define XYZ_CROP_LAUNCH(io_, sg_)                                                                                   \
  LAUNCH_K((k_lift_xyz_inv<io_, sg_, true>), grid, dim3(kXYZThreadsI), smem, stream, vals, valsStride, cdims[0],      \
           cdims[1], cdims[2], K, st, volume, vd, crop, F, nseg)
    if (crop) {
      if (io == 1 && sg)
        XYZ_CROP_LAUNCH(1, true);
      else if (io == 1)
        XYZ_CROP_LAUNCH(1, false);
      else if (sg)
        XYZ_CROP_LAUNCH(2, true);
      else
        XYZ_CROP_LAUNCH(2, false);
    }
    else if (io == 1) {
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
#undef XYZ_CROP_LAUNCH
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

bool lift2_applicable(const uint32_t region[3])
{
  return lift_xyz_applicable(region) && region[0] <= (uint32_t)kL2MaxRow;
}

// segments per tile of a level-2 launch (SPERR_HIP_L2_NSEG, diagnostics build: 1, 2 or 4 whatever the rule says)
static uint32_t lift2_segments(uint32_t ntile, uint32_t nchunks, uint32_t cz)
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
  size_t smem = 2 * (size_t)kXYZStaged * xyz_row_stride(region[0]) * sizeof(double);   // two staging buffers
#if XYZ_INV_PREFETCH == 2
  smem += (size_t)kXYZThreadsI * kL2PosI * 2 * sizeof(uint32_t) + (size_t)kXYZBoxSlots * 64 * sizeof(uint32_t);   // (see launch_lift_xyz)
#endif
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

