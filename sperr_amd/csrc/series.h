// series.h -- a time series of one field: an orthonormal Haar transform across the steps, every band an ordinary
// container of a double volume.  The ONLY statement of the rule: the kernels k_series_fwd / k_series_inv (series.hip),
// the calls (abi_series.hip), the host check tests/cpp/series_check.cpp and, in numpy, tests/series_model.py (which
// states it again; every bit is compared).  Plain C++: no HIP here.
//
//   plan       levels L in 0 .. 4.  Steps 0 .. N-1 are cut into consecutive groups of 2^L; a remainder r < 2^L is cut by
//              the binary digits of r, largest first (N = 11, L = 3: 8, 2, 1).  A group of 2^l steps gets l levels; a
//              group of one step is the step itself as a double
//   bands      inside a group of g = 2^l: slot 0 is the approximation a_l, slot 1 is d_l, slots 2 .. 3 are d_{l-1}, ...,
//              slots g/2 .. g-1 are d_1: (level k, index j) is slot g / 2^k + j.  Band b of the series is group start +
//              slot: N steps are N band volumes
//   forward    fp64, no fused multiply-add, s = 0x1.6a09e667f3bcdp-1 (1/sqrt 2 rounded); fp32 samples are widened first
//                a = (e + o) * s,  d = (e - o) * s        e, o the even and odd entries of the level below
//   inverse      e = (a + d) * s,  o = (a - d) * s        narrowed with one (float) when fp32 is asked for
//   needs      slot (level k, index j) covers the steps [j 2^k, (j+1) 2^k) of its group, slot 0 the whole group.  A decode
//              of the steps [t0, t0 + nt) needs exactly the bands whose cover meets it
//
// The point-wise tolerance.  A step is x = 2^(-l/2) a_l +- sum_k 2^(-k/2) d_k along its path.  If every band of a group
// is within tau of its value, the step is within A_l tau, with A_0 = 1 and A_{l+1} = s (A_l + 1): one level of the
// inverse takes an a within A and a d within 1 (in units of tau) to (A + 1) / sqrt 2.  That is 1.414, 1.707, 1.914,
// 2.061 for l = 1 .. 4, and it is tight: the signs can be chosen so that every term adds (the model test enumerates
// them).  The bands of a group of 2^l are coded in point-wise error mode at
//   tau_l = (tol - rho) / A_l,
// rho a bound of what the two butterflies round.  With u = 2^-53, one butterfly output is the exact one times
// (1 + d1)(1 + d2)(1 + d3), |d| <= u: the sum or difference, the rounded constant, the product.  Values of level k are
// at most 2^(k/2) M in magnitude, M the largest |sample| of the series.
//   forward    E_k, the error of a level-k value against the exact transform: E_0 = 0,
//              E_{k+1} <= sqrt 2 E_k + 3u 2^((k+1)/2) M, so E_k <= 3k u 2^(k/2) M.  The exact inverse of these errors moves
//              a step by at most 2^(-l/2) E_l + sum_k 2^(-k/2) E_k = 3u M (l + l (l+1) / 2)
//   inverse    on the decoded bands, whose exact inverse x'' is within tol of x, so level-k values stay within
//              2^(k/2) (M + tol): F_l = 0, F_{k-1} <= F_k / sqrt 2 + 3u 2^((k-1)/2) (M + tol), so F_0 <= 3 l u (M + tol)
//   together   3u (M (l + l (l+1) / 2) + l (M + tol)) <= 3u (3 l + l (l+1) / 2) max(M, tol): 12, 27, 45, 66 u max(M, tol)
//              for l = 1 .. 4; one more u max(M, tol) covers the terms of second order (66 u < 2^-46).
//   rho      = K_L 2^-53 max(M, tol),  K = 0, 13, 28, 46, 67 for L = 0 .. 4: one rho for the series, that of its largest
//              groups.  For every tolerance up to M -- any that keeps something of the data -- that is K_L 2^-53 M.
// A call is refused when rho >= tol / 2 (a tolerance at the rounding of the data's own doubles).  levels = 0 has
// rho = 0 and tau = tol: the plain batch.  The narrowing of an fp32 output is not part of the bound, as in mode 3.
//
// PSNR.  The transform is orthonormal up to that rounding, so the series' squared error is the sum of the bands'.  Every
// band is coded by the rule of psnr_vol.h with `range` the series' range, hence the same target error t.
#ifndef SPERR_AMD_SERIES_H
#define SPERR_AMD_SERIES_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SERIES_HD __host__ __device__ inline
#define SERIES_UNROLL _Pragma("unroll")
#else
#define SERIES_HD inline
#define SERIES_UNROLL
#endif

namespace sperrhip {

constexpr int kSeriesMaxLevels = 4;
constexpr int kSeriesMaxGroup = 1 << kSeriesMaxLevels;
constexpr double kSeriesS = 0x1.6a09e667f3bcdp-1;
constexpr size_t kSeriesInfoBytes = 64;
constexpr int kSeriesKindTol = 0, kSeriesKindPsnr = 1;

// ---- the plan --------------------------------------------------------------------------------------------------------
// groups a series of n steps has at `levels`: n / 2^L whole ones and one per binary digit of the remainder
SERIES_HD size_t series_group_count(size_t n, int levels)
{
  size_t r = n & (((size_t)1 << levels) - 1), c = n >> levels;
  for (; r; r &= r - 1)
    c++;
  return c;
}

// group i of the plan: its first step (= first band) and its level count
SERIES_HD void series_group(size_t n, int levels, size_t i, size_t* start, int* l)
{
  const size_t whole = n >> levels;
  if (i < whole) {
    *start = i << levels;
    *l = levels;
    return;
  }
  size_t at = whole << levels, k = whole;
  for (int b = levels - 1; b >= 0; b--)
    if ((n >> b) & 1) {
      if (k == i) {
        *start = at;
        *l = b;
        return;
      }
      at += (size_t)1 << b;
      k++;
    }
  *start = n;
  *l = 0;
}

// the group a step (or band) lies in
SERIES_HD void series_group_of(size_t n, int levels, size_t t, size_t* start, int* l)
{
  const size_t whole = n >> levels;
  if (t < whole << levels) {
    *start = t >> levels << levels;
    *l = levels;
    return;
  }
  size_t at = whole << levels;
  for (int b = levels - 1; b >= 0; b--)
    if ((n >> b) & 1) {
      if (t < at + ((size_t)1 << b)) {
        *start = at;
        *l = b;
        return;
      }
      at += (size_t)1 << b;
    }
  *start = n;
  *l = 0;
}

// the steps of its group, relative to the group's start, that slot `slot` of a group of 2^l covers: [*lo, *hi)
SERIES_HD void series_slot_cover(int l, size_t slot, size_t* lo, size_t* hi)
{
  if (slot == 0) {
    *lo = 0;
    *hi = (size_t)1 << l;
    return;
  }
  int k = l;   // slot is in [2^(l-k), 2^(l-k+1))
  while (slot >> (l - k + 1))
    k--;
  const size_t j = slot - ((size_t)1 << (l - k));
  *lo = j << k;
  *hi = (j + 1) << k;
}

// need[b] = 1 for the bands a decode of the steps [t0, t0 + nt) needs, 0 for the others; false: the range leaves the series
inline bool series_needs(size_t n, int levels, size_t t0, size_t nt, uint8_t* need)
{
  if (n == 0 || levels < 0 || levels > kSeriesMaxLevels || nt == 0 || t0 >= n || nt > n - t0)
    return false;
  const size_t ng = series_group_count(n, levels);
  for (size_t i = 0; i < ng; i++) {
    size_t start;
    int l;
    series_group(n, levels, i, &start, &l);
    for (size_t slot = 0; slot < (size_t)1 << l; slot++) {
      size_t lo, hi;
      series_slot_cover(l, slot, &lo, &hi);
      need[start + slot] = start + lo < t0 + nt && t0 < start + hi ? 1 : 0;
    }
  }
  return true;
}

// ---- the butterflies: v holds 2^l values, steps going in and bands in slot order coming out, and back ----------------
template <int l>
SERIES_HD void series_forward(double* v)
{
  constexpr int g = 1 << l;
  double w[g > 1 ? g : 1];
  SERIES_UNROLL
  for (int len = g; len > 1; len >>= 1) {
    SERIES_UNROLL
    for (int j = 0; j < len / 2; j++) {
      const double e = v[2 * j], o = v[2 * j + 1];
      w[j] = (e + o) * kSeriesS;
      w[len / 2 + j] = (e - o) * kSeriesS;
    }
    SERIES_UNROLL
    for (int j = 0; j < len; j++)
      v[j] = w[j];
  }
}

template <int l>
SERIES_HD void series_inverse(double* v)
{
  constexpr int g = 1 << l;
  double w[g > 1 ? g : 1];
  SERIES_UNROLL
  for (int len = 2; len <= g; len <<= 1) {
    SERIES_UNROLL
    for (int j = 0; j < len / 2; j++) {
      const double a = v[j], d = v[len / 2 + j];
      w[2 * j] = (a + d) * kSeriesS;
      w[2 * j + 1] = (a - d) * kSeriesS;
    }
    SERIES_UNROLL
    for (int j = 0; j < len; j++)
      v[j] = w[j];
  }
}

// (the same with l at run time: the host check and callers that have no use for the templates)
inline void series_forward_l(int l, double* v)
{
  switch (l) {
    case 1: series_forward<1>(v); break;
    case 2: series_forward<2>(v); break;
    case 3: series_forward<3>(v); break;
    case 4: series_forward<4>(v); break;
    default: break;
  }
}
inline void series_inverse_l(int l, double* v)
{
  switch (l) {
    case 1: series_inverse<1>(v); break;
    case 2: series_inverse<2>(v); break;
    case 3: series_inverse<3>(v); break;
    case 4: series_inverse<4>(v); break;
    default: break;
  }
}

// ---- the tolerance -----------------------------------------------------------------------------------------------------
// A_l by its recurrence, in double
inline double series_gain(int l)
{
  double a = 1.0;
  for (int k = 0; k < l; k++)
    a = kSeriesS * (a + 1.0);
  return a;
}

constexpr double kSeriesRoundK[kSeriesMaxLevels + 1] = {0.0, 13.0, 28.0, 46.0, 67.0};

// rho of a series with largest |sample| M at `levels`, and tau[l] for l = 0 .. levels.  False: tol or M is not a finite
// number, tol is not positive, or rho >= tol / 2
inline bool series_tolerance(double tol, double M, int levels, double* rho, double* tau)
{
  if (levels < 0 || levels > kSeriesMaxLevels || !(tol > 0.0) || !isfinite(tol) || !(M >= 0.0) || !isfinite(M))
    return false;
  const double r = kSeriesRoundK[levels] * 0x1p-53 * (M > tol ? M : tol);
  if (!(r < tol / 2.0))
    return false;
  *rho = r;
  for (int l = 0; l <= levels; l++)
    tau[l] = (tol - r) / series_gain(l);
  return true;
}

// ---- the info record: 64 bytes, little-endian ----------------------------------------------------------------------------
//   0-3 "SPTS" | 4 version 1 | 5 levels | 6 is_float of the steps | 7 kind (0 tol, 1 psnr) | 8-11 N | 12-23 dimx, dimy,
//   dimz (u32 each) | 24-31 tol or psnr | 32-39 range (max - min of the series, or the caller's) | 40-47 M | 48-55 rho
//   (0 in psnr mode) | 56-63 0
struct SeriesInfo {
  int levels, is_float, kind;
  uint64_t n, dims[3];
  double quality, range, M, rho;
};

inline void series_put(uint8_t* p, uint64_t v, int bytes)
{
  for (int i = 0; i < bytes; i++)
    p[i] = (uint8_t)(v >> (8 * i));
}
inline uint64_t series_get(const uint8_t* p, int bytes)
{
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++)
    v |= (uint64_t)p[i] << (8 * i);
  return v;
}
inline uint64_t series_bits(double d)
{
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}
inline double series_double(uint64_t b)
{
  double d;
  memcpy(&d, &b, 8);
  return d;
}

inline bool series_info_ok(const SeriesInfo& h)
{
  return h.levels >= 0 && h.levels <= kSeriesMaxLevels && (h.kind == kSeriesKindTol || h.kind == kSeriesKindPsnr) &&
         h.n > 0 && h.n <= 0xffffffffull && h.dims[0] > 0 && h.dims[1] > 0 && h.dims[2] > 0 &&
         h.dims[0] <= 0xffffffffull && h.dims[1] <= 0xffffffffull && h.dims[2] <= 0xffffffffull;
}

inline void series_write_info(const SeriesInfo& h, uint8_t out[kSeriesInfoBytes])
{
  memset(out, 0, kSeriesInfoBytes);
  memcpy(out, "SPTS", 4);
  out[4] = 1;
  out[5] = (uint8_t)h.levels;
  out[6] = h.is_float ? 1 : 0;
  out[7] = (uint8_t)h.kind;
  series_put(out + 8, h.n, 4);
  for (int a = 0; a < 3; a++)
    series_put(out + 12 + 4 * a, h.dims[a], 4);
  series_put(out + 24, series_bits(h.quality), 8);
  series_put(out + 32, series_bits(h.range), 8);
  series_put(out + 40, series_bits(h.M), 8);
  series_put(out + 48, series_bits(h.rho), 8);
}

inline bool series_parse_info(const uint8_t in[kSeriesInfoBytes], SeriesInfo* h)
{
  if (memcmp(in, "SPTS", 4) != 0 || in[4] != 1 || in[6] > 1)
    return false;
  for (int i = 56; i < 64; i++)
    if (in[i] != 0)
      return false;
  h->levels = in[5];
  h->is_float = in[6];
  h->kind = in[7];
  h->n = series_get(in + 8, 4);
  for (int a = 0; a < 3; a++)
    h->dims[a] = series_get(in + 12 + 4 * a, 4);
  h->quality = series_double(series_get(in + 24, 8));
  h->range = series_double(series_get(in + 32, 8));
  h->M = series_double(series_get(in + 40, 8));
  h->rho = series_double(series_get(in + 48, 8));
  return series_info_ok(*h);
}

}  // namespace sperrhip

#endif
