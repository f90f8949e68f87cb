// rel.hip -- the kernels of point-wise relative error (rel.h: the rule, the side stream).
//
//   k_rel_forward<T, kVec>   one read of the volume: y, the sign bits with every tile's toggle count (what k_mask_survey
//                            leaves of a mask, so that k_mask_finish and k_mask_pack make the sign stream), and whether
//                            a sample is not finite.  The zero class is y's NaNs: the masked encoder finds it
//   k_rel_header             the 48 bytes of the side stream's header and the padding between its two streams
//   k_rel_inverse<OT>        a dense box of y' with the zero and sign bits at the box's volume positions into x'
//   k_rel_check<T, kVec>     the four figures of sperrhip_rel_check_dev
// k_rel_forward and k_rel_inverse are the LINEAR map kind's; the log kind's two are rel_log.hip's, launched from here.
//
// The walks are mask.hip's: a wavefront takes a tile of kMaskTile samples at a time and walks the tiles beyond a grid
// capped at kMaskGroupsPerCU workgroups per CU; no kernel waits on another workgroup.  kVec moves 16 bytes per lane and
// is chosen when the pointers allow; the other form moves element by element.  LDS holds a workgroup's partials only.
#include "rel_walk.h"

namespace sperrhip {

namespace {

// what the forward kernel leaves beside the sign bits' workspace, and the check's four words
struct RelRecord {
  uint32_t nonfinite, pad;
  uint64_t check[4];   // the bits of the largest ratio, violations, class mismatches, samples outside the zero class
};

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

template <typename T, bool kVec>
__global__ __launch_bounds__(kMaskThreads) void k_rel_forward(const T* __restrict__ src, uint64_t n,
                                                              double* __restrict__ y, uint64_t* __restrict__ words,
                                                              uint32_t* __restrict__ tileTog,
                                                              uint64_t* __restrict__ partials,
                                                              uint32_t* __restrict__ nonfinite)
{
  constexpr uint32_t P = kVec ? kMaskPackBytes / sizeof(T) : 1;
  constexpr uint32_t kIter = kMaskTile / (64 * P);   // loads of a lane per tile
  using Pack = typename RelPack<T>::type;
  __shared__ uint64_t s_neg[kWavesPerGroup];
  __shared__ uint32_t s_bad[kWavesPerGroup];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ntiles = (n + kMaskTile - 1) / kMaskTile;
  uint64_t nneg = 0;   // (the same in every lane)
  bool bad = false;
  for (uint64_t tile = (uint64_t)blockIdx.x * kWavesPerGroup + wave; tile < ntiles;
       tile += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t s0 = tile * kMaskTile;
    // the sample before the tile, not the word before it: tiles stay independent
    uint64_t carry = s0 > 0 && rel_class((double)src[s0 - 1]).neg ? 1 : 0;
    T v[kIter][P];
#pragma unroll
    for (uint32_t it = 0; it < kIter; it++) {
      const uint64_t i = s0 + (uint64_t)(it * 64 + lane) * P;
      if (kVec && i + P <= n) {
        const Pack pk = *reinterpret_cast<const Pack*>(src + i);
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          v[it][j] = pk[j];
      }
      else {
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          v[it][j] = i + j < n ? src[i + j] : T(0);
      }
    }
    uint32_t tog = 0;
#pragma unroll
    for (uint32_t it = 0; it < kIter; it++) {
      const uint64_t i = s0 + (uint64_t)(it * 64 + lane) * P;
      uint64_t ballot[P];
      double out[P];
#pragma unroll
      for (uint32_t j = 0; j < P; j++) {
        RelClass c;
        out[j] = rel_forward(v[it][j], &c);
        const bool in = i + j < n;
        ballot[j] = __ballot(in && c.neg);
        bad |= in && !c.finite;
      }
      if (kVec && i + P <= n) {
#pragma unroll
        for (uint32_t j = 0; j < P; j += 2)
          *reinterpret_cast<Double2*>(y + i + j) = Double2{out[j], out[j + 1 < P ? j + 1 : j]};
      }
      else {
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          if (i + j < n)
            y[i + j] = out[j];
      }
#pragma unroll
      for (uint32_t w = 0; w < P; w++) {
        const uint64_t sw = s0 + (uint64_t)(it * P + w) * 64;
        if (sw < n) {
          const uint64_t word = mask_word_of_ballots<P>(ballot, w);
          const uint32_t nbits = (uint32_t)min((uint64_t)64, n - sw);
          tog += __popcll(mask_toggle_bits(word, carry, nbits));
          nneg += __popcll(word);
          carry = word >> 63;
          if (lane == w)
            words[sw >> 6] = word;
        }
      }
    }
    if (lane == 0)
      tileTog[tile] = tog;
  }
  const bool waveBad = __any(bad);
  if (lane == 0) {
    s_neg[wave] = nneg;
    s_bad[wave] = waveBad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t anyBad = 0;
    for (uint32_t w = 1; w < kWavesPerGroup; w++)
      nneg += s_neg[w];
    for (uint32_t w = 0; w < kWavesPerGroup; w++)
      anyBad |= s_bad[w];
    // (the signs have no order of their own: k_mask_finish sees a valid range of one finite value)
    partials[(uint64_t)blockIdx.x * 3 + 0] = mask_key(0.0);
    partials[(uint64_t)blockIdx.x * 3 + 1] = mask_key(0.0);
    partials[(uint64_t)blockIdx.x * 3 + 2] = nneg;
    if (anyBad)
      atomicOr(nonfinite, 1u);
  }
}

struct RelHeadBytes {
  uint8_t b[kRelHeaderBytes];
};

// the header, and the `npad` (< 8) zero bytes at pad_at between the zero stream and the sign stream
__global__ __launch_bounds__(64) void k_rel_header(RelHeadBytes h, uint8_t* __restrict__ d_side, uint64_t pad_at,
                                                   uint32_t npad)
{
  if (threadIdx.x < kRelHeaderBytes)
    d_side[threadIdx.x] = h.b[threadIdx.x];
  if (threadIdx.x < npad)
    d_side[pad_at + threadIdx.x] = 0;
}

// (dst may be yp when OT is double: a lane loads its samples of a piece before it stores any, and nobody else's.  All
//  the loads of a piece go out before the first store: the two pointers may alias, so the compiler cannot move them)
template <typename OT>
__global__ __launch_bounds__(kMaskThreads) void k_rel_inverse(const double* yp, OT* dst, RelBox g, BitSrc zero,
                                                              BitSrc sign, bool srcFloat)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t items = g.rows * g.pieces;
  for (uint64_t item = (uint64_t)blockIdx.x * kWavesPerGroup + wave; item < items;
       item += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t row = item / g.pieces, piece = item - row * g.pieces;
    const uint64_t z = row / g.by, yy = row - z * g.by;
    // the row is the bit range [base, base + bx) of the volume
    const uint64_t base = ((g.lz + z) * g.vy + g.ly + yy) * g.vx + g.lx;
    const uint64_t x0 = piece * kMaskTile, x1 = min(g.bx, x0 + kMaskTile);
    const double* s = yp + row * g.bx;
    OT* d = dst + row * g.bx;
    double v[kMaskTileWords];
#pragma unroll
    for (uint32_t k = 0; k < kMaskTileWords; k++) {
      const uint64_t x = x0 + k * 64 + lane;
      v[k] = x < x1 ? s[x] : 0.0;
    }
    BitCursor cz = bit_cursor(zero, base + x0), cs = bit_cursor(sign, base + x0);
#pragma unroll
    for (uint32_t k = 0; k < kMaskTileWords; k++) {
      const uint64_t x = x0 + k * 64;
      if (x < x1) {   // (the same in every lane)
        const uint64_t wz = bit_next64(zero, cz, base + x), ws = bit_next64(sign, cs, base + x);
        if (x + lane < x1)
          d[x + lane] = rel_inverse<OT>(v[k], (wz >> lane) & 1, (ws >> lane) & 1, srcFloat);
      }
    }
  }
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    v = max(v, (uint64_t)__shfl_xor((unsigned long long)v, d, 64));
  return v;
}

// (a ratio is no NaN and not negative: the doubles' bit patterns order as they do)
template <typename T, bool kVec>
__global__ __launch_bounds__(kMaskThreads) void k_rel_check(const T* __restrict__ a, const T* __restrict__ b, uint64_t n,
                                                            double eps, uint64_t* __restrict__ out)
{
  constexpr uint32_t P = kVec ? kMaskPackBytes / sizeof(T) : 1;
  using Pack = typename RelPack<T>::type;
  __shared__ uint64_t s_part[kWavesPerGroup][4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t worst = 0, viol = 0, mis = 0, cnt = 0;
  auto take = [&](T x, T xr) {
    const RelCheck r = rel_check_pair((double)x, (double)xr, eps);
    worst = max(worst, rel_bits(r.ratio));
    viol += r.violates;
    mis += r.mismatch;
    cnt += r.counted;
  };
  const uint64_t npacks = (n + P - 1) / P;
  for (uint64_t p = (uint64_t)blockIdx.x * kMaskThreads + threadIdx.x; p < npacks; p += (uint64_t)gridDim.x * kMaskThreads) {
    const uint64_t i = p * P;
    if (kVec && i + P <= n) {
      const Pack pa = *reinterpret_cast<const Pack*>(a + i), pb = *reinterpret_cast<const Pack*>(b + i);
#pragma unroll
      for (uint32_t j = 0; j < P; j++)
        take(pa[j], pb[j]);
    }
    else {
      for (uint32_t j = 0; j < P && i + j < n; j++)
        take(a[i + j], b[i + j]);
    }
  }
  worst = wave_max64(worst);
  viol = wave_sum64(viol);
  mis = wave_sum64(mis);
  cnt = wave_sum64(cnt);
  if (lane == 0) {
    s_part[wave][0] = worst;
    s_part[wave][1] = viol;
    s_part[wave][2] = mis;
    s_part[wave][3] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kWavesPerGroup; w++) {
      worst = max(worst, s_part[w][0]);
      viol += s_part[w][1];
      mis += s_part[w][2];
      cnt += s_part[w][3];
    }
    // one atomic of each kind per workgroup, into words the call has zeroed
    atomicMax(reinterpret_cast<unsigned long long*>(out + 0), (unsigned long long)worst);
    atomicAdd(reinterpret_cast<unsigned long long*>(out + 1), (unsigned long long)viol);
    atomicAdd(reinterpret_cast<unsigned long long*>(out + 2), (unsigned long long)mis);
    atomicAdd(reinterpret_cast<unsigned long long*>(out + 3), (unsigned long long)cnt);
  }
}

RelRecord* rel_record(void* ws, size_t n)
{
  return reinterpret_cast<RelRecord*>(static_cast<char*>(ws) + up256(mask_workspace_bytes(n)));
}

template <typename T>
int forward_launch(const T* src, size_t n, double* y, const MaskBitsParts& w, uint32_t* flag, uint32_t groups,
                   hipStream_t st)
{
  if ((uintptr_t)src % kMaskPackBytes == 0 && (uintptr_t)y % kMaskPackBytes == 0)
    LAUNCH_K((k_rel_forward<T, true>), dim3(groups), dim3(kMaskThreads), 0, st, src, (uint64_t)n, y, w.words, w.tileTog,
             w.partials, flag);
  else
    LAUNCH_K((k_rel_forward<T, false>), dim3(groups), dim3(kMaskThreads), 0, st, src, (uint64_t)n, y, w.words, w.tileTog,
             w.partials, flag);
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int check_launch(const T* a, const T* b, size_t n, double eps, uint64_t* out, hipStream_t st)
{
  const bool vec = (uintptr_t)a % kMaskPackBytes == 0 && (uintptr_t)b % kMaskPackBytes == 0;
  const uint64_t packs = vec ? (n + kMaskPackBytes / sizeof(T) - 1) / (kMaskPackBytes / sizeof(T)) : n;
  uint32_t groups = 0;
  if (rel_grid((packs + 63) / 64, &groups))
    return -1;
  if (vec)
    LAUNCH_K((k_rel_check<T, true>), dim3(groups), dim3(kMaskThreads), 0, st, a, b, (uint64_t)n, eps, out);
  else
    LAUNCH_K((k_rel_check<T, false>), dim3(groups), dim3(kMaskThreads), 0, st, a, b, (uint64_t)n, eps, out);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

size_t rel_workspace_bytes(size_t n)
{
  const size_t ws = mask_workspace_bytes(n);
  return ws ? up256(ws) + up256(sizeof(RelRecord)) : 0;
}

int rel_forward_run(const void* d_src, int is_float, size_t n, double* d_y, void* ws, RelForward* res, void* hip_stream,
                    int kind)
{
  MaskBitsParts w;
  if (!d_src || !d_y || !res || !ws || !rel_kind_ok(kind) || rel_workspace_bytes(n) == 0 || !mask_bits_parts(ws, n, &w))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  RelRecord* rec = rel_record(ws, n);
  uint32_t groups = 0;
  if (rel_grid((n + kMaskTile - 1) / kMaskTile, &groups))
    return -1;
  HIP_CHECK(hipMemsetAsync(&rec->nonfinite, 0, sizeof(uint32_t), st));
  if (kind == kRelLog ? rel_log_forward_launch(d_src, is_float, n, d_y, w, &rec->nonfinite, groups, hip_stream)
      : is_float      ? forward_launch(static_cast<const float*>(d_src), n, d_y, w, &rec->nonfinite, groups, st)
                      : forward_launch(static_cast<const double*>(d_src), n, d_y, w, &rec->nonfinite, groups, st))
    return -1;
  if (mask_bits_finish_run(ws, n, groups, hip_stream))
    return -1;
  HIP_CHECK(hipMemcpyAsync(&res->sign, w.res, sizeof(MaskResult), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&res->nonfinite, &rec->nonfinite, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  return 0;
}

int rel_side_run(const RelHeader& h, const void* ws, const MaskResult& sign, void* d_side, void* hip_stream)
{
  if (!ws || !d_side || (uintptr_t)d_side % 8 != 0 || sign.mask_len != h.sign_len)
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  uint8_t* side = static_cast<uint8_t*>(d_side);
  // (k_mask_pack reads the workspace alone: the samples' pointer is not looked at without a fill)
  if (mask_pack_fill_run(ws, 0, (size_t)h.n, ws, sign, side + rel_sign_offset(h), nullptr, hip_stream))
    return -1;
  RelHeadBytes hb;
  rel_write_header(h, hb.b);
  const uint64_t padAt = kRelHeaderBytes + h.zero_len;
  LAUNCH_K(k_rel_header, dim3(1), dim3(64), 0, st, hb, side, padAt, (uint32_t)(rel_pad8(h.zero_len) - h.zero_len));
  HIP_CHECK(hipGetLastError());
  return 0;
}

int rel_inverse_run(const double* d_y, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                    const MaskStream& zero, const MaskStream& sign, int src_float, int output_float, void* d_dst,
                    void* hip_stream, int kind)
{
  if (kind == kRelLog)
    return rel_log_inverse_run(d_y, vol, lo, dims, zero, sign, src_float, output_float, d_dst, hip_stream);
  if (!d_y || !d_dst || !zero.d_payload || !sign.d_payload || kind != kRelLinear)
    return -1;
  const RelBox g = rel_box_of(vol, lo, dims, zero.h.n);
  uint32_t groups = 0;
  if (rel_grid(g.rows * g.pieces, &groups))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (output_float)
    LAUNCH_K((k_rel_inverse<float>), dim3(groups), dim3(kMaskThreads), 0, st, d_y, static_cast<float*>(d_dst), g,
             bit_src(zero), bit_src(sign), src_float != 0);
  else
    LAUNCH_K((k_rel_inverse<double>), dim3(groups), dim3(kMaskThreads), 0, st, d_y, static_cast<double*>(d_dst), g,
             bit_src(zero), bit_src(sign), src_float != 0);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int rel_check_run(const void* d_orig, const void* d_recon, int is_float, size_t n, double eps, void* ws,
                  uint64_t out[4], void* hip_stream)
{
  if (!d_orig || !d_recon || !ws || !out || rel_workspace_bytes(n) == 0)
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  RelRecord* rec = rel_record(ws, n);
  HIP_CHECK(hipMemsetAsync(rec->check, 0, sizeof(rec->check), st));
  if (is_float ? check_launch(static_cast<const float*>(d_orig), static_cast<const float*>(d_recon), n, eps, rec->check, st)
               : check_launch(static_cast<const double*>(d_orig), static_cast<const double*>(d_recon), n, eps,
                              rec->check, st))
    return -1;
  HIP_CHECK(hipMemcpyAsync(out, rec->check, sizeof(rec->check), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

}  // namespace sperrhip
