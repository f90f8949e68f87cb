// psnr_vol.hip -- the range of a volume's samples on the device (sperrhip_range_dev): what the common target of
// sperrhip_compress_psnr_dev is made from (psnr_vol.h).  A streaming read, the volume once.
#include "engine_core.h"
#include "xform.h"

namespace sperrhip {

namespace {

// Smallest and largest sample of a volume, dense or a strided view (view.h), and the count of NaNs: a NaN loses every
// comparison, so it would vanish from the extremes -- it is counted (v != v) and the caller refuses.
// A row is cut into segments of segLen samples; a workgroup takes (row, segment) items in a grid-stride loop.  kVec:
// the samples in front of a segment's first 16-byte boundary and behind its last one go one per lane, what lies between
// with 16-byte loads, four in flight per lane.  Otherwise (rows shorter than a few loads) one sample per lane.
// The extremes are reduced per wavefront, then per workgroup, then with one pair of atomicMax on the order keys of
// max(v) and max(-v) (xform.h: the keys of a zeroed word are below every value); out = {key of max, key of max(-v), NaNs}
template <typename T, bool kVec>
__global__ void __launch_bounds__(kThreads)
k_vol_range(const T* __restrict__ src, uint64_t dimx, uint64_t dimy, uint64_t nrows, uint64_t pitchY, uint64_t pitchZ,
            uint64_t segLen, uint64_t segsPerRow, unsigned long long* out)
{
  constexpr uint32_t V = 16 / sizeof(T);
  struct alignas(16) Pack { T v[V]; };
  __shared__ double wmax[kThreads / 64], wneg[kThreads / 64];
  __shared__ uint32_t wnan[kThreads / 64];
  double vmax = -INFINITY, vnegmax = -INFINITY;
  uint32_t nans = 0;
  auto take = [&](T v) {
    const double d = (double)v;
    vmax = fmax(vmax, d);
    vnegmax = fmax(vnegmax, -d);
    nans += (v != v) ? 1u : 0u;
  };
  const uint64_t items = nrows * segsPerRow;
  for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const uint64_t r = it / segsPerRow, sg = it - r * segsPerRow;
    const uint64_t z = r / dimy, y = r - z * dimy;
    const uint64_t x0 = sg * segLen;
    const uint64_t len = min(dimx - x0, segLen);
    const T* p = src + z * pitchZ + y * pitchY + x0;
    if constexpr (kVec) {
      const uint64_t mis = (reinterpret_cast<uintptr_t>(p) / sizeof(T)) % V;
      const uint64_t head = min(len, (uint64_t)((V - mis) % V));
      if (threadIdx.x < head)
        take(p[threadIdx.x]);
      const Pack* pv = reinterpret_cast<const Pack*>(p + head);
      const uint64_t nv = (len - head) / V;
      uint64_t i = threadIdx.x;
      for (; i + 3 * kThreads < nv; i += 4 * kThreads) {
        Pack pk[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
          pk[k] = pv[i + k * kThreads];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
          for (uint32_t e = 0; e < V; e++)
            take(pk[k].v[e]);
      }
      for (; i < nv; i += kThreads) {
        const Pack pk = pv[i];
#pragma unroll
        for (uint32_t e = 0; e < V; e++)
          take(pk.v[e]);
      }
      const uint64_t done = head + nv * V;   // (fewer than V samples are left)
      if (done + threadIdx.x < len)
        take(p[done + threadIdx.x]);
    }
    else {
      for (uint64_t i = threadIdx.x; i < len; i += kThreads)
        take(p[i]);
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    vmax = fmax(vmax, __shfl_xor(vmax, d, 64));
    vnegmax = fmax(vnegmax, __shfl_xor(vnegmax, d, 64));
    nans += __shfl_xor(nans, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wmax[threadIdx.x >> 6] = vmax;
    wneg[threadIdx.x >> 6] = vnegmax;
    wnan[threadIdx.x >> 6] = nans;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; w++) {
      vmax = fmax(vmax, wmax[w]);
      vnegmax = fmax(vnegmax, wneg[w]);
      nans += wnan[w];
    }
    atomicMax(out, order_key(vmax));
    atomicMax(out + 1, order_key(vnegmax));
    if (nans)
      atomicAdd(out + 2, (unsigned long long)nans);
  }
}

template <typename T>
int launch_vol_range(hipStream_t st, const T* d_src, const Dims& vol, const ViewPitch& pitch, unsigned long long* d_out)
{
  if (reinterpret_cast<uintptr_t>(d_src) % sizeof(T) != 0)
    return -1;
  constexpr uint64_t V = 16 / sizeof(T);
  uint64_t dimx = vol[0], dimy = vol[1], nrows = (uint64_t)vol[1] * vol[2];
  if (pitch.y == vol[0] && pitch.z == vol[0] * vol[1]) {   // dense: one row
    dimx *= nrows;
    dimy = nrows = 1;
  }
  const uint64_t segLen = (uint64_t)kThreads * V * 8;
  const uint64_t segsPerRow = (dimx + segLen - 1) / segLen;
  const uint64_t items = nrows * segsPerRow;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(items, 256 * 8);
  HIP_CHECK(hipMemsetAsync(d_out, 0, 3 * sizeof(unsigned long long), st));
  if (dimx >= 4 * V)
    LAUNCH_K((k_vol_range<T, true>), dim3(grid), dim3(kThreads), 0, st, d_src, dimx, dimy, nrows, (uint64_t)pitch.y,
             (uint64_t)pitch.z, segLen, segsPerRow, d_out);
  else
    LAUNCH_K((k_vol_range<T, false>), dim3(grid), dim3(kThreads), 0, st, d_src, dimx, dimy, nrows, (uint64_t)pitch.y,
             (uint64_t)pitch.z, segLen, segsPerRow, d_out);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int range_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const ViewPitch* srcView, double* vmin,
             double* vmax, hipStream_t st)
{
  if (E.misc.ensure(4096))
    return -1;
  unsigned long long* d_out = static_cast<unsigned long long*>(E.misc.p);
  const ViewPitch pitch = srcView ? *srcView : view_dense(vol[0], vol[1]);
  if (is_float ? launch_vol_range(st, static_cast<const float*>(d_src), vol, pitch, d_out)
               : launch_vol_range(st, static_cast<const double*>(d_src), vol, pitch, d_out))
    return -1;
  unsigned long long h[3] = {0, 0, 1};
  HIP_CHECK(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  E.prof.collect();
  if (h[2] != 0) {
    fprintf(stderr, "[sperr_hip] the volume holds %llu NaN%s: it has no range\n", h[2], h[2] == 1 ? "" : "s");
    return -1;
  }
  *vmax = order_key_value(h[0]);
  *vmin = -order_key_value(h[1]);
  return 0;
}

}  // namespace sperrhip
