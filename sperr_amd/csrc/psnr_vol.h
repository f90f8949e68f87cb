// psnr_vol.h -- PSNR of the WHOLE volume: one target error for every chunk, and the five q a chunk can end on.  The ONLY
// statement of the rule: the kernels k_mse_ladder / k_mse_ladder_pick (xform.hip), the engine (encode.hip), the host check
// tests/cpp/psnr_vol_check.cpp and, in numpy, tests/psnr_vol_model.py (which states it again; every bit is compared).
// Plain C++: no HIP here.
//
// PSNR mode (mode 2) is the reference's rule chunk by chunk: each chunk takes the range of its own samples
// (src/SPECK_FLT.cpp:268-279,426-435).  Here the range is the volume's, or one the caller gives:
//
//   range     double(vmax) - double(vmin) of the raw samples, one subtraction; or a positive finite number of the caller's
//   t         (range * range) * pow(10.0, -psnr / 10.0)          the target mean squared error, the reference's order
//   ladder    q_0 = 2.0 * sqrt(t * 3.0),  q_{k+1} = q_k / exp2(0.25)          host libm, the reference's order; k < 5
//   estimate  mse(q) of a chunk's n coefficients v: strides of 4096 in order, each summed in order,
//               diff = fma(-q, rint(v * (1 / q)), v),  acc = fma(diff, diff, acc)
//             the stride sums added in order -- the last stride is short or empty --, divided by n
//   pick      the first rung k with mse(q_k) <= t: what the reference's search `while (mse(q) > t) q /= 2^(1/4)` ends on
//             when started from the common range
//   width     m = maxabs / q; refused unless m < 2^63 (llrint would be undefined from there on, and for a NaN);
//             64-bit coefficients when llrint(m) > 0xffffffff (src/SPECK_FLT.cpp:323-337)
//
// Why five rungs are all there are.  The quantiser is mid-tread: rint(v / q) is the nearest integer, so the error of a
// coefficient is |diff| <= q / 2 and mse(q) <= q^2 / 4 whatever the data.  q_0^2 = 12 t, and four steps halve q:
// q_4 = q_0 / 2 up to the rounding of four divisions, so mse(q_4) <= q_4^2 / 4 = 12 t / 16 = 0.75 t <= t.  Every chunk
// stops at a rung 0 .. 4.  The margin of 25 % is what the rounding has to stay under: of the ladder (four divisions,
// 2^-51 relative) and of the quantiser's product v * (1 / q), which is off by |v / q| 2^-52 before rint and moves the
// half by |v / q| 2^-51 at most.  That is nothing for coefficients that fit 32 bits (|v / q| < 2^32: 2^-19 of a step)
// and negligible below |v| = 2^40 q; it reaches a quarter of a step near |v / q| = 2^49, where the bound stops holding.
// Such a chunk is far beyond the 64-bit pass's useful range; if no rung resolves it the call is refused (no loop
// behind the ladder that nothing could test).
#ifndef SPERR_AMD_PSNR_VOL_H
#define SPERR_AMD_PSNR_VOL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PSNR_VOL_HD __host__ __device__ inline
#else
#define PSNR_VOL_HD inline
#endif

namespace sperrhip {

constexpr int kPsnrRungs = 5;
constexpr uint32_t kPsnrStride = 4096;   // coefficients per stride of the estimate (src/SPECK_FLT.cpp:237-266)

// the common target and the table, as the kernels take them
struct PsnrLadder {
  double t;
  double q[kPsnrRungs];
};

// what k_mse_ladder_pick leaves in CoderState::mse_active (0: the chunk has its q)
constexpr uint32_t kPsnrRefusedWidth = 2;    // maxabs / q is 2^63 or more, or a NaN
constexpr uint32_t kPsnrRefusedNoRung = 3;   // no rung's estimate is at most t

// The table from a range and a target, host libm in the reference's order of operations (host only: the device gets
// the table as a kernel argument).  False when a rung is not a positive finite number -- a range of 0, a target that
// underflows: no chunk can be quantised with it
inline bool psnr_vol_ladder(double range, double psnr, PsnrLadder* L)
{
  L->t = (range * range) * pow(10.0, -psnr / 10.0);
  double q = 2.0 * sqrt(L->t * 3.0);
  for (int k = 0; k < kPsnrRungs; k++) {
    L->q[k] = q;
    q /= exp2(0.25);
  }
  return isfinite(L->q[0]) && L->q[kPsnrRungs - 1] > 0.0;
}

// one coefficient's term of a stride sum
PSNR_VOL_HD double psnr_vol_term(double acc, double v, double q, double rcp_q)
{
  const double diff = fma(-q, rint(v * rcp_q), v);
  return fma(diff, diff, acc);
}

// the stride sums of a rung added in order, divided by n
PSNR_VOL_HD double psnr_vol_total(const double* strideSum, uint32_t nstrides, uint64_t n)
{
  double total = 0.0;
  for (uint32_t s = 0; s < nstrides; s++)
    total += strideSum[s];
  return total / (double)n;
}

// strides of a chunk of n coefficients: the last one is short or empty
PSNR_VOL_HD uint32_t psnr_vol_strides(uint64_t n) { return (uint32_t)(n / kPsnrStride) + 1; }

// the estimate of one q on a chunk, start to end on one thread (the host check and the model's yardstick)
PSNR_VOL_HD double psnr_vol_estimate(const double* v, uint64_t n, double q)
{
  const double rcp_q = 1.0 / q;
  double total = 0.0;
  for (uint64_t beg = 0; beg <= n / kPsnrStride * kPsnrStride; beg += kPsnrStride) {
    const uint64_t end = beg + kPsnrStride < n ? beg + kPsnrStride : n;
    double acc = 0.0;
    for (uint64_t i = beg; i < end; i++)
      acc = psnr_vol_term(acc, v[i], q, rcp_q);
    total += acc;
  }
  return total / (double)n;
}

// the first rung whose estimate is at most t; -1: none
PSNR_VOL_HD int psnr_vol_pick(const double mse[kPsnrRungs], double t)
{
  for (int k = 0; k < kPsnrRungs; k++)
    if (mse[k] <= t)
      return k;
  return -1;
}

// 0: 32-bit coefficients; 1: 64-bit; -1: refused
PSNR_VOL_HD int psnr_vol_width(double maxabs, double q)
{
  const double m = maxabs / q;
  if (!(m < 0x1p63))
    return -1;
  return llrint(m) > (long long)0xffffffffll ? 1 : 0;
}

}  // namespace sperrhip

#endif
