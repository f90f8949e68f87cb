// lift_window.h -- the CDF 9/7 lifting steps on a window of a row in registers (k_lift_xy of lift_axis.hip, the x and y passes of lift_xyz.h;
// compiled for the host as well, where tests/test_lift_window_host.py compares the window widths bit for bit)
#ifndef SPERR_AMD_LIFT_WINDOW_H
#define SPERR_AMD_LIFT_WINDOW_H

#include "xform.h"

namespace sperrhip {

// The lifting steps of QccWAVCDF97AnalysisSymmetric / SynthesisSymmetric (src/CDF97.cpp:598-666) on
// 16 consecutive samples r[0..16) of the symmetrically extended signal, r[0] at an even position:
// r[4..12) come out exactly as the whole-signal loops compute them -- a step reaches one sample to
// each side, the extension is symmetric about the first and the last sample and a + b == b + a, so
// the mirrored copies stay equal to the samples the reference's clamped indices refer to.
template <bool FORWARD>
__host__ __device__ __forceinline__ void lift16(double (&r)[16], const LiftConsts& K)
{
  if (FORWARD) {
#pragma unroll
    for (int k = 1; k <= 13; k += 2)
      r[k] = fma(K.alpha, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 2; k <= 12; k += 2)
      r[k] = fma(K.beta, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 3; k <= 11; k += 2)
      r[k] = fma(K.gamma, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 4; k <= 10; k += 2)
      r[k] = K.eps * fma(K.delta, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 5; k <= 11; k += 2)
      r[k] = (-K.inv_eps) * r[k];
  }
  else {
#pragma unroll
    for (int k = 1; k <= 15; k += 2)
      r[k] = (-K.eps) * r[k];
#pragma unroll
    for (int k = 2; k <= 14; k += 2) {
      const double t = K.delta * (r[k - 1] + r[k + 1]);
      r[k] = fma(r[k], K.inv_eps, -t);
    }
#pragma unroll
    for (int k = 3; k <= 13; k += 2)
      r[k] = fma(-K.gamma, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 4; k <= 12; k += 2)
      r[k] = fma(-K.beta, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 5; k <= 11; k += 2)
      r[k] = fma(-K.alpha, r[k - 1] + r[k + 1], r[k]);
  }
}

// lift16 on a window of W = NOUT + 8 samples, r[0] at an even position: r[4 .. W - 4) come out as lift16's r[4..12)
// do (W = 16 is lift16).  A narrower window gives a pass more tasks -- 1024 with NOUT = 4 where cx = 256, one per
// thread, against 512 -- and a task fewer registers, for three LDS reads per output instead of two.
template <bool FORWARD, int W>
__host__ __device__ __forceinline__ void lift_window(double (&r)[W], const LiftConsts& K)
{
  static_assert(W >= 10 && W <= 16 && (W & 1) == 0, "an even number of outputs");
  if (FORWARD) {
#pragma unroll
    for (int k = 1; k <= W - 3; k += 2)
      r[k] = fma(K.alpha, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 2; k <= W - 4; k += 2)
      r[k] = fma(K.beta, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 3; k <= W - 5; k += 2)
      r[k] = fma(K.gamma, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 4; k <= W - 6; k += 2)
      r[k] = K.eps * fma(K.delta, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 5; k <= W - 5; k += 2)
      r[k] = (-K.inv_eps) * r[k];
  }
  else {
#pragma unroll
    for (int k = 1; k <= W - 1; k += 2)
      r[k] = (-K.eps) * r[k];
#pragma unroll
    for (int k = 2; k <= W - 2; k += 2) {
      const double t = K.delta * (r[k - 1] + r[k + 1]);
      r[k] = fma(r[k], K.inv_eps, -t);
    }
#pragma unroll
    for (int k = 3; k <= W - 3; k += 2)
      r[k] = fma(-K.gamma, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 4; k <= W - 4; k += 2)
      r[k] = fma(-K.beta, r[k - 1] + r[k + 1], r[k]);
#pragma unroll
    for (int k = 5; k <= W - 5; k += 2)
      r[k] = fma(-K.alpha, r[k - 1] + r[k + 1], r[k]);
  }
}

} // namespace sperrhip

#endif
