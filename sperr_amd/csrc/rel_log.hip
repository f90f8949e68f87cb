// rel_log.hip -- the two kernels of the LOG map kind of point-wise relative error (rel.h: the rule and both maps).
//
//   k_rel_log_forward<T, kVec>   k_rel_forward's walk with y = rel_log2(|x|): one read of the volume, y, the sign bits
//                                with every tile's toggle count, and whether a sample is not finite
//   k_rel_log_inverse<OT>        k_rel_inverse's walk with |x'| = rel_exp2(y')
//
// A unit of its own so that rel.hip's code object stays what it was: the walks are written out a second time, and what
// they share beyond the rule -- the packs, the grid, the SPMK readers, the box -- is rel_walk.h's.  The maps add about
// forty fp64 operations and, forward, one division per sample to kernels that moved bytes only; the samples of a
// 16-byte pack go through their Horner chains side by side, one pack at a time, which keeps the registers of
// k_rel_forward's shape (profiles/rel_log_codeobj.txt: no scratch).
#include "rel_walk.h"

namespace sperrhip {

namespace {

template <typename T, bool kVec>
__global__ __launch_bounds__(kMaskThreads) void k_rel_log_forward(const T* __restrict__ src, uint64_t n,
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
        out[j] = rel_forward<kRelLog>(v[it][j], &c);
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

// (dst may be yp when OT is double, as in k_rel_inverse: all the loads of a piece go out before its first store)
template <typename OT>
__global__ __launch_bounds__(kMaskThreads) void k_rel_log_inverse(const double* yp, OT* dst, RelBox g, BitSrc zero,
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
          d[x + lane] = rel_inverse<OT, kRelLog>(v[k], (wz >> lane) & 1, (ws >> lane) & 1, srcFloat);
      }
    }
  }
}

template <typename T>
int forward_launch(const T* src, size_t n, double* y, const MaskBitsParts& w, uint32_t* flag, uint32_t groups,
                   hipStream_t st)
{
  if ((uintptr_t)src % kMaskPackBytes == 0 && (uintptr_t)y % kMaskPackBytes == 0)
    LAUNCH_K((k_rel_log_forward<T, true>), dim3(groups), dim3(kMaskThreads), 0, st, src, (uint64_t)n, y, w.words,
             w.tileTog, w.partials, flag);
  else
    LAUNCH_K((k_rel_log_forward<T, false>), dim3(groups), dim3(kMaskThreads), 0, st, src, (uint64_t)n, y, w.words,
             w.tileTog, w.partials, flag);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int rel_log_forward_launch(const void* d_src, int is_float, size_t n, double* d_y, const MaskBitsParts& w,
                           uint32_t* d_nonfinite, uint32_t groups, void* hip_stream)
{
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  return is_float ? forward_launch(static_cast<const float*>(d_src), n, d_y, w, d_nonfinite, groups, st)
                  : forward_launch(static_cast<const double*>(d_src), n, d_y, w, d_nonfinite, groups, st);
}

int rel_log_inverse_run(const double* d_y, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                        const MaskStream& zero, const MaskStream& sign, int src_float, int output_float, void* d_dst,
                        void* hip_stream)
{
  if (!d_y || !d_dst || !zero.d_payload || !sign.d_payload)
    return -1;
  const RelBox g = rel_box_of(vol, lo, dims, zero.h.n);
  uint32_t groups = 0;
  if (rel_grid(g.rows * g.pieces, &groups))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (output_float)
    LAUNCH_K((k_rel_log_inverse<float>), dim3(groups), dim3(kMaskThreads), 0, st, d_y, static_cast<float*>(d_dst), g,
             bit_src(zero), bit_src(sign), src_float != 0);
  else
    LAUNCH_K((k_rel_log_inverse<double>), dim3(groups), dim3(kMaskThreads), 0, st, d_y, static_cast<double*>(d_dst), g,
             bit_src(zero), bit_src(sign), src_float != 0);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace sperrhip
