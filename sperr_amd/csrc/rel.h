// rel.h -- point-wise RELATIVE error, |x' - x| <= eps |x|: the ONLY statement of the rule (the entry points of
// abi_rel.hip, the kernels of rel.hip and rel_log.hip and the host checks tests/cpp/rel_check.cpp and rel_log_check.cpp
// all use these).  Plain C++: no HIP here.
//
// A relative bound is a point-wise bound in a logarithmic domain.  A volume x becomes an ordinary container of a double
// volume y in point-wise error mode at a tolerance t, and a SIDE STREAM that holds what y cannot: which samples are
// zeros, and every sample's sign.  The logarithm is not log2 but its piecewise linear interpolant between the powers of
// two, read off the IEEE bit pattern: integer operations and one add, the same bits on every machine.
//
//   forward   d = (double)x, exact.  d not finite: the call is refused
//             zero class  fabs(d) < 0x1p-1022: +0.0, -0.0 and double subnormals.  Every nonzero float, subnormal floats
//                         included, is a normal double and is NOT in this class
//             sign        the sign bit of d, also of -0.0
//             y           outside the zero class, E the biased exponent field of d and M its 52 mantissa bits:
//                           y = (double)((int)E - 1023) + (double)M * 0x1p-52          (one IEEE add)
//                         exact for fp32 data (24 + 8 bits); for fp64 data rounded once, by at most 2^-44 (|y| < 2^10)
//                         fp32 data only, y < -126 (a subnormal float): y = -126 + 2 * (y + 126), exact -- see below
//                         in the zero class the quiet NaN 0x7ff8000000000000, which the encoder in-fills
//   tolerance t = eps / (1.0 + eps) - s in double as written, s = 0x1p-22 (fp32 data) or 0x1p-40 (fp64 data).  Refused
//             unless eps is finite, eps <= 0.5 and t >= s
//   inverse   zero bit set: a zero carrying its sign bit (what y' holds there is never read as a value)
//             otherwise, the source fp32 data and y' < -126: y' = -126 + 0.5 * (y' + 126); then
//             y' clamped into [-1080, nextafter(1024, 0)] (only a portion decode can need it),
//               e = floor(y'), m = y' - e (exact), a = ldexp(1.0 + m, (int)e),
//             narrowed once for float output -- a narrowing that overflows gives FLT_MAX --, then the sign bit
//
// Why |y' - y| <= t is enough.  g(y) = 2^floor(y) * (1 + y - floor(y)) is the inverse: continuous, increasing, linear
// on every [e, e + 1) with slope 2^e, and 2^e <= g(y) there; g(y(x)) = |x|.  For 0 <= d <= t < 1:
//   upward    g(y + d) - g(y) <= d * (largest slope on [y, y + d]) <= d * g(y + d), so g(y + d) / g(y) <= 1 / (1 - d)
//             and the relative error is at most d / (1 - d) <= t / (1 - t)
//   downward  g(y) - g(y - d) <= d * (largest slope on [y - d, y]) <= d * g(y): at most t
// With t' = eps / (1 + eps), t' / (1 - t') = eps exactly; t = t' - s leaves room for what is rounded on the way, each far
// below s in the y domain: y (2^-44, fp64 data only), 1 + m (2^-53), the narrowing to a normal float (2^-24 of the value).
//
// The subnormal floats.  A float below 2^-126 lies on a grid of ABSOLUTE spacing u = 2^-149, and narrowing x' onto that
// grid adds up to u / 2, which no relative slack covers: with y as above, x = 64 u and eps = 1e-2, y' = y + t gives
// 64.63 u, which narrows to 65 u, an error of 1.56 %.  No inverse can mend that (two floats one unit apart can share a
// y'), so the forward map gives these samples twice the resolution: below -126 the y axis is stretched by 2 about -126,
// which is exact, continuous and monotone, and reaches -172.  There |y' - y| <= t is a relative error below eps / 2
// before the narrowing; the narrowing either gives x back (the error was below u / 2) or at most doubles the error.
// A sample on one side of 2^-126 whose y' lies on the other is closer to it in the unstretched axis than t.  fp64 data
// has no such range: a double that small is in the zero class.  (A double in the lowest binade, 2^-1022 <= |x| <
// 2^-1021, can come back as a subnormal double: within the bound, but in the zero class of sperrhip_rel_check_dev.)
// tests/test_rel_model.py walks eps from the floor to 0.5, d = +-t, the powers of two with their neighbours and the
// float subnormals, and rechecks in exact rational arithmetic every sample that comes near the bound.
//
// The second MAP KIND: the true logarithm.  kind = kRelLinear (0) is everything above and the default everywhere;
// kind = kRelLog (1) codes y = log2|x| itself.  The interpolant has a kink at every power of two, which the wavelet pays
// for at every level, and its tolerance eps / (1 + eps) is 1 / 1.45 of log2(1 + eps): on fields that are smooth in the
// exponent the log kind's container is a growing fraction smaller.  Zero class, sign, the refusal of
// samples that are not finite, the NaN in the zero class, the stretch by 2 below -126 for fp32 data (now rounded once,
// by at most 2^-46), the un-stretch, the clamp and the narrowing are the linear kind's.  What differs:
//
//   forward   y = rel_log2(|d|):  E, M as above, m = 1.M in [1, 2); m >= sqrt(2) (0x1.6a09e667f3bcdp+0): m = m / 2 and
//             e = E - 1022, else e = E - 1023, so m is in [sqrt(1/2), sqrt(2));  s = (m - 1) / (m + 1) (m - 1 is exact),
//             z = s * s, p = c10; p = p * z + ck for k = 9 .. 0 with ck = 2 / (ln 2 (2k + 1)) rounded to double: the
//             series of 2 atanh(s) / ln 2, whose remainder is below 2^-60 of its value for |s| <= 0.1716;
//             y = (double)e + s * p.  A power of two gives its exponent exactly
//   tolerance t = rel_log2(1.0 + eps) - s, the SAME s.  Refused unless eps is finite, 0 < eps <= 0.5 and t >= s
//   inverse   |x'| = rel_exp2(y'), y' un-stretched and clamped as above:  e = floor(y'), f = y' - e (exact); f > 1/2:
//             f = f - 1, e = e + 1, so f is in (-1/2, 1/2];  w = f * ln 2 (0x1.62e42fefa39efp-1), p = 1 / 13!;
//             p = p * w + 1 / k! for k = 12 .. 0 (remainder below 2^-57); ldexp(p, (int)e).  An integer y' gives its
//             power of two exactly.  At the clamp's ends: y' = -1080 gives +0.0 (ldexp rounds 2^-1080 once, to zero, as
//             the linear kind's does); y' = nextafter(1024, 0) has e = 1024 and p just below 1 and gives a value
//             below 2^1024; should p round to 1 or more with e = 1024 the result is DBL_MAX, never an infinity
//
// Every operation is IEEE double, rounded once, in the order written: + - * /, floor, ldexp and bit casts, no libm or
// ocml transcendental, no table, no fused multiply-add (the functions switch contraction off for the compilers that
// would fuse; the host check is built with -ffp-contract=off).  The device's fp64 division is its correctly rounded
// one.  tests/rel_log_model.py states the same sequence in numpy and every bit is compared.
//
// Why |y' - y| <= t is enough here.  Let L = log2|x|, y = L + a with |a| <= dL (the forward map's error), the computed
// t = log2(1 + eps) - s + b with |b| <= dT, and |x'| = 2^y' (1 + c) with |c| <= dX before a narrowing to a normal
// float, which multiplies by at most 1 + 2^-24.  Then
//   upward    |x'| / |x| <= 2^(t + dL) (1 + dX) (1 + 2^-24) <= 1 + eps   is   s >= dL + dT + log2(1 + dX) + log2(1 + 2^-24)
//   downward  |x'| / |x| >= 2^-(t + dL) (1 - dX) (1 - 2^-24) >= 1 - eps  follows from the same s, since
//             2^-t = 2^s / (1 + eps) and 1 / (1 + eps) >= 1 - eps
// Measured against mpmath at 256 bits (tests/test_rel_log_model.py, 30 000 magnitudes, 24 800 y', 3 000 eps):
//   dL = 2^-46.0 over the floats' range and 2^-44.0 over all doubles: the one rounding of e + s p, half an ulp of |y|
//   dX = 2^-51.9 as log2(1 + dX);  dT = 2^-52.1
//   fp32 data: 4 (dL + dX + dT) + log2(1 + 2^-24) = 2^-23.47 <= s = 2^-22;  fp64 data: 4 (dL + dX + dT) = 2^-41.99 <=
//   s = 2^-40.  Both slacks stay what the linear kind's are.
// The subnormal floats keep the stretch and its argument: in the stretched axis |y' - y| <= t is a relative error below
// eps / 2 before the narrowing; the stretch and the un-stretch now round once each (2^-46), far inside that half.
//
// Side stream "SPRL" (linear kind) or "SPLG" (log kind: the same layout under another magic, so that a library from
// before this kind refuses a stream it would decode wrongly), little-endian, 8-byte aligned:
//   0-3 the magic | 4 version 1 | 5 is_float of the source | 6-7 0 | 8-15 the bits of eps (+0.0: none stated) | 16-23 n |
//   24-31 length of the zero stream | 32-39 length of the sign stream | 40-47 0 |
//   48- the zero stream, padding to 8 bytes, the sign stream
// Both are SPMK streams exactly as mask.h defines them: bit 1 = zero class / negative, the same kind rule.
// rel_max_size(n) = 48 + 2 * mask_max_size(n).  A stream that is handed in has its three headers checked (rel_parse,
// mask_parse twice); its payload is trusted, as a mask's is.
#ifndef SPERR_AMD_REL_H
#define SPERR_AMD_REL_H

#include <float.h>

#include "mask.h"

namespace sperrhip {

constexpr size_t kRelHeaderBytes = 48;
constexpr uint8_t kRelVersion = 1;
constexpr uint64_t kRelNanBits = 0x7ff8000000000000ull;
constexpr double kRelEpsMax = 0.5;
constexpr double kRelYMin = -1080.0, kRelYMax = 0x1.fffffffffffffp+9;   // nextafter(1024, 0)
constexpr double kRelYSubFloat = -126.0;   // y of the smallest normal float: fp32 data is stretched by 2 below it

// the map kinds
constexpr int kRelLinear = 0, kRelLog = 1;
SPERR_VIEW_FN bool rel_kind_ok(int kind) { return kind == kRelLinear || kind == kRelLog; }

SPERR_VIEW_FN uint64_t rel_bits(double d)
{
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}
SPERR_VIEW_FN double rel_from_bits(uint64_t u)
{
  double d;
  memcpy(&d, &u, 8);
  return d;
}

// ---- the maps of the log kind ---------------------------------------------------------------------------------------
// (a compiler that contracts a * b + c by default is told not to, function by function)
#if defined(__clang__)
#define SPERR_REL_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SPERR_REL_NO_CONTRACT
#endif

// log2 of a normal positive double
SPERR_VIEW_FN double rel_log2(double mag)
{
  SPERR_REL_NO_CONTRACT
  const uint64_t u = rel_bits(mag);
  int e = (int)((u >> 52) & 0x7ffu) - 1023;
  double m = rel_from_bits((u & ((uint64_t(1) << 52) - 1)) | (uint64_t(0x3ff) << 52));
  if (m >= 0x1.6a09e667f3bcdp+0) {
    m = m * 0.5;
    e = e + 1;
  }
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double p = 0x1.1964ec6fc9491p-3;
  p = p * z + 0x1.3703c1f4d0ffep-3;
  p = p * z + 0x1.5b9ac9b743f0dp-3;
  p = p * z + 0x1.89f3b1694cffep-3;
  p = p * z + 0x1.c68f568d31760p-3;
  p = p * z + 0x1.0c9a84994022dp-2;
  p = p * z + 0x1.484b13d7c02a9p-2;
  p = p * z + 0x1.a61762a7aded9p-2;
  p = p * z + 0x1.2776c50ef9bfep-1;
  p = p * z + 0x1.ec709dc3a03fdp-1;
  p = p * z + 0x1.71547652b82fep+1;
  return (double)e + s * p;
}

// 2^y for y in [kRelYMin, kRelYMax]: finite
SPERR_VIEW_FN double rel_exp2(double y)
{
  SPERR_REL_NO_CONTRACT
  double e = floor(y);
  double f = y - e;
  if (f > 0.5) {
    f = f - 1.0;
    e = e + 1.0;
  }
  const double w = f * 0x1.62e42fefa39efp-1;
  double p = 0x1.6124613a86d09p-33;
  p = p * w + 0x1.1eed8eff8d898p-29;
  p = p * w + 0x1.ae64567f544e4p-26;
  p = p * w + 0x1.27e4fb7789f5cp-22;
  p = p * w + 0x1.71de3a556c734p-19;
  p = p * w + 0x1.a01a01a01a01ap-16;
  p = p * w + 0x1.a01a01a01a01ap-13;
  p = p * w + 0x1.6c16c16c16c17p-10;
  p = p * w + 0x1.1111111111111p-7;
  p = p * w + 0x1.5555555555555p-5;
  p = p * w + 0x1.5555555555555p-3;
  p = p * w + 0x1p-1;
  p = p * w + 1.0;
  p = p * w + 1.0;
  if (e == 1024.0 && !(p < 1.0))
    return DBL_MAX;
  return ldexp(p, (int)e);
}

// ---- the tolerance --------------------------------------------------------------------------------------------------
SPERR_VIEW_FN double rel_slack(bool is_float) { return is_float ? 0x1p-22 : 0x1p-40; }

// t of eps; false: eps is refused
SPERR_VIEW_FN bool rel_tolerance(double eps, bool is_float, double* t, int kind = kRelLinear)
{
  if (!(fabs(eps) <= DBL_MAX) || !(eps <= kRelEpsMax) || !rel_kind_ok(kind))
    return false;
  if (kind == kRelLog && !(eps > 0.0))   // (rel_log2 takes a normal positive double)
    return false;
  const double s = rel_slack(is_float);
  const double q = kind == kRelLog ? rel_log2(1.0 + eps) : eps / (1.0 + eps);
  const double r = q - s;
  if (!(r >= s))
    return false;
  *t = r;
  return true;
}

// ---- forward --------------------------------------------------------------------------------------------------------

struct RelClass {
  bool zero, neg, finite;
};

// the class of a sample, widened to double
SPERR_VIEW_FN RelClass rel_class(double d)
{
  const uint64_t u = rel_bits(d);
  const uint32_t E = (uint32_t)(u >> 52) & 0x7ffu;
  return RelClass{E == 0, (u >> 63) != 0, E != 0x7ffu};
}

// y of a sample and its class; a sample that is not finite has the zero class's y (the call is refused)
template <int kKind = kRelLinear, typename T>
SPERR_VIEW_FN double rel_forward(T x, RelClass* c)
{
  const double d = (double)x;
  const uint64_t u = rel_bits(d);
  *c = rel_class(d);
  if (c->zero || !c->finite)
    return rel_from_bits(kRelNanBits);
  const int E = (int)((u >> 52) & 0x7ffu);
  const uint64_t M = u & ((uint64_t(1) << 52) - 1);
  const double y = kKind == kRelLog ? rel_log2(fabs(d)) : (double)(E - 1023) + (double)M * 0x1p-52;
  if (sizeof(T) == sizeof(float) && y < kRelYSubFloat)
    return kRelYSubFloat + 2.0 * (y - kRelYSubFloat);
  return y;
}

// ---- inverse --------------------------------------------------------------------------------------------------------
SPERR_VIEW_FN double rel_with_sign(double a, bool neg)
{
  return rel_from_bits((rel_bits(a) & ~(uint64_t(1) << 63)) | ((uint64_t)neg << 63));
}
SPERR_VIEW_FN float rel_with_sign(float a, bool neg)
{
  uint32_t u;
  memcpy(&u, &a, 4);
  u = (u & 0x7fffffffu) | ((uint32_t)neg << 31);
  memcpy(&a, &u, 4);
  return a;
}

// |x'| of y' outside the zero class (a y' that is a NaN clamps to the lower end); src_float: the source was fp32 data
template <int kKind = kRelLinear>
SPERR_VIEW_FN double rel_magnitude(double yp, bool src_float)
{
  if (src_float && yp < kRelYSubFloat)
    yp = kRelYSubFloat + 0.5 * (yp - kRelYSubFloat);
  if (!(yp >= kRelYMin))
    yp = kRelYMin;
  if (yp > kRelYMax)
    yp = kRelYMax;
  if (kKind == kRelLog)
    return rel_exp2(yp);
  const double e = floor(yp);
  const double m = yp - e;
  return ldexp(1.0 + m, (int)e);
}

template <typename OT>
SPERR_VIEW_FN OT rel_narrow(double a);
template <>
SPERR_VIEW_FN double rel_narrow<double>(double a)
{
  return a;
}
template <>
SPERR_VIEW_FN float rel_narrow<float>(double a)
{
  return a > (double)FLT_MAX ? FLT_MAX : (float)a;   // (what rounds down to FLT_MAX anyway, and what would overflow)
}

template <typename OT, int kKind = kRelLinear>
SPERR_VIEW_FN OT rel_inverse(double yp, bool zero, bool neg, bool src_float)
{
  const OT a = zero ? OT(0) : rel_narrow<OT>(rel_magnitude<kKind>(yp, src_float));
  return rel_with_sign(a, neg);
}

// ---- the side stream ------------------------------------------------------------------------------------------------
struct RelHeader {
  int is_float;
  double eps;
  uint64_t n, zero_len, sign_len;
  int kind = kRelLinear;
};

SPERR_VIEW_FN uint64_t rel_pad8(uint64_t v) { return (v + 7) / 8 * 8; }
SPERR_VIEW_FN size_t rel_max_size(size_t n) { return kRelHeaderBytes + 2 * mask_max_size(n); }
// where the sign stream starts, and the stream's length
SPERR_VIEW_FN uint64_t rel_sign_offset(const RelHeader& h) { return kRelHeaderBytes + rel_pad8(h.zero_len); }
SPERR_VIEW_FN uint64_t rel_stream_bytes(const RelHeader& h) { return rel_sign_offset(h) + h.sign_len; }

SPERR_VIEW_FN void rel_write_header(const RelHeader& h, uint8_t out[kRelHeaderBytes])
{
  out[0] = 'S';
  out[1] = 'P';
  out[2] = h.kind == kRelLog ? 'L' : 'R';
  out[3] = h.kind == kRelLog ? 'G' : 'L';
  out[4] = kRelVersion;
  out[5] = (uint8_t)(h.is_float != 0);
  out[6] = out[7] = 0;
  mask_put_u64(out + 8, rel_bits(h.eps));
  mask_put_u64(out + 16, h.n);
  mask_put_u64(out + 24, h.zero_len);
  mask_put_u64(out + 32, h.sign_len);
  mask_put_u64(out + 40, 0);
}

// The header of a stream of side_len bytes whose first min(side_len, 48) bytes are at `head`: magic (either, it names
// the kind), version, is_float, the reserved bytes, eps against the tolerance rule OF THAT KIND (or +0.0: the stream of
// a forward call, which states no bound), n,
// and the two lengths against side_len exactly.  The two SPMK
// headers are mask_parse's to check, each against its length and n.  false: the stream is refused
SPERR_VIEW_FN bool rel_parse(const uint8_t* head, size_t side_len, RelHeader* h)
{
  if (!head || side_len < kRelHeaderBytes + 2 * kMaskHeaderBytes)
    return false;
  const bool linear = head[2] == 'R' && head[3] == 'L', log = head[2] == 'L' && head[3] == 'G';
  if (head[0] != 'S' || head[1] != 'P' || !(linear || log) || head[4] != kRelVersion)
    return false;
  if (head[5] > 1 || head[6] != 0 || head[7] != 0 || mask_get_u64(head + 40) != 0)
    return false;
  const RelHeader r{head[5], rel_from_bits(mask_get_u64(head + 8)), mask_get_u64(head + 16), mask_get_u64(head + 24),
                    mask_get_u64(head + 32), log ? kRelLog : kRelLinear};
  double t;
  if ((rel_bits(r.eps) != 0 && !rel_tolerance(r.eps, r.is_float != 0, &t, r.kind)) || r.n == 0)
    return false;
  const uint64_t room = side_len - kRelHeaderBytes;
  if (r.zero_len < kMaskHeaderBytes || r.sign_len < kMaskHeaderBytes || r.zero_len > room ||
      rel_pad8(r.zero_len) > room || room - rel_pad8(r.zero_len) != r.sign_len)
    return false;
  *h = r;
  return true;
}

// ---- the check (sperrhip_rel_check_dev) -----------------------------------------------------------------------------
// what one pair of samples adds to the four figures: over the samples whose ORIGINAL is outside the zero class the
// largest |x' - x| / |x| in double and the count of |x' - x| > eps * |x|; over all samples the count of pairs that
// differ in zero class or in sign
struct RelCheck {
  double ratio;   // (0 in the zero class)
  bool counted, violates, mismatch;
};
SPERR_VIEW_FN RelCheck rel_check_pair(double x, double xr, double eps)
{
  const RelClass a = rel_class(x), b = rel_class(xr);
  RelCheck r{0.0, !a.zero, false, a.zero != b.zero || a.neg != b.neg};
  if (!a.zero) {
    const double err = fabs(xr - x), mag = fabs(x);
    r.ratio = err / mag;
    r.violates = !(err <= eps * mag);
  }
  return r;
}

// ---- the device side (rel.hip; the log kind's two kernels are rel_log.hip's) -----------------------------------------
// bytes of workspace the calls below need for n samples (0: n is refused): the sign bits' mask workspace and a record
size_t rel_workspace_bytes(size_t n);

// what rel_forward_run leaves for the host: valid after the NEXT host wait for the stream
struct RelForward {
  MaskResult sign;      // the sign stream's length and kind, the negative samples
  uint32_t nonfinite;   // not 0: a sample is not finite
};
// k_rel_forward (or, kind = kRelLog, k_rel_log_forward) and k_mask_finish on `hip_stream`: y of the n samples at d_src
// into d_y, the sign bits into `ws` (rel_workspace_bytes(n) of device memory, 256-byte aligned).  No host wait.  0 ok,
// -1 a HIP error or an unknown kind
int rel_forward_run(const void* d_src, int is_float, size_t n, double* d_y, void* ws, RelForward* res,
                    void* hip_stream, int kind = kRelLinear);
// The side stream around a zero stream that stands at d_side + 48 already: the header `h`, the padding and the sign
// stream from `ws`.  No host wait
int rel_side_run(const RelHeader& h, const void* ws, const MaskResult& sign, void* d_side, void* hip_stream);
// x' of the box [lo, lo + dims) of a volume of dims vol, which d_y holds densely as y', into d_dst (floats or doubles;
// d_y itself when doubles); src_float and kind: the side stream's.  The streams' headers are parsed and name the
// volume's n.  No host wait
int rel_inverse_run(const double* d_y, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                    const MaskStream& zero, const MaskStream& sign, int src_float, int output_float, void* d_dst,
                    void* hip_stream, int kind = kRelLinear);
// The four words of the check into out (the first the bits of a double), with ONE host wait; `ws` as above
int rel_check_run(const void* d_orig, const void* d_recon, int is_float, size_t n, double eps, void* ws,
                  uint64_t out[4], void* hip_stream);

}  // namespace sperrhip

#endif
