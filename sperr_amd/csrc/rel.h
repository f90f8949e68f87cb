// rel.h -- point-wise RELATIVE error, |x' - x| <= eps |x|: the ONLY statement of the rule (the entry points of
// abi_rel.hip, the kernels of rel.hip and the host check tests/cpp/rel_check.cpp all use these).  Plain C++: no HIP here.
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
// Side stream "SPRL", little-endian, 8-byte aligned:
//   0-3 "SPRL" | 4 version 1 | 5 is_float of the source | 6-7 0 | 8-15 the bits of eps (+0.0: none stated) | 16-23 n |
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

// ---- the tolerance --------------------------------------------------------------------------------------------------
SPERR_VIEW_FN double rel_slack(bool is_float) { return is_float ? 0x1p-22 : 0x1p-40; }

// t of eps; false: eps is refused
SPERR_VIEW_FN bool rel_tolerance(double eps, bool is_float, double* t)
{
  if (!(fabs(eps) <= DBL_MAX) || !(eps <= kRelEpsMax))
    return false;
  const double s = rel_slack(is_float);
  const double q = eps / (1.0 + eps);
  const double r = q - s;
  if (!(r >= s))
    return false;
  *t = r;
  return true;
}

// ---- forward --------------------------------------------------------------------------------------------------------
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
template <typename T>
SPERR_VIEW_FN double rel_forward(T x, RelClass* c)
{
  const double d = (double)x;
  const uint64_t u = rel_bits(d);
  *c = rel_class(d);
  if (c->zero || !c->finite)
    return rel_from_bits(kRelNanBits);
  const int E = (int)((u >> 52) & 0x7ffu);
  const uint64_t M = u & ((uint64_t(1) << 52) - 1);
  const double y = (double)(E - 1023) + (double)M * 0x1p-52;
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
SPERR_VIEW_FN double rel_magnitude(double yp, bool src_float)
{
  if (src_float && yp < kRelYSubFloat)
    yp = kRelYSubFloat + 0.5 * (yp - kRelYSubFloat);
  if (!(yp >= kRelYMin))
    yp = kRelYMin;
  if (yp > kRelYMax)
    yp = kRelYMax;
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

template <typename OT>
SPERR_VIEW_FN OT rel_inverse(double yp, bool zero, bool neg, bool src_float)
{
  const OT a = zero ? OT(0) : rel_narrow<OT>(rel_magnitude(yp, src_float));
  return rel_with_sign(a, neg);
}

// ---- the side stream ------------------------------------------------------------------------------------------------
struct RelHeader {
  int is_float;
  double eps;
  uint64_t n, zero_len, sign_len;
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
  out[2] = 'R';
  out[3] = 'L';
  out[4] = kRelVersion;
  out[5] = (uint8_t)(h.is_float != 0);
  out[6] = out[7] = 0;
  mask_put_u64(out + 8, rel_bits(h.eps));
  mask_put_u64(out + 16, h.n);
  mask_put_u64(out + 24, h.zero_len);
  mask_put_u64(out + 32, h.sign_len);
  mask_put_u64(out + 40, 0);
}

// The header of a stream of side_len bytes whose first min(side_len, 48) bytes are at `head`: magic, version, is_float,
// the reserved bytes, eps against the tolerance rule (or +0.0: the stream of a forward call, which states no bound), n,
// and the two lengths against side_len exactly.  The two SPMK
// headers are mask_parse's to check, each against its length and n.  false: the stream is refused
SPERR_VIEW_FN bool rel_parse(const uint8_t* head, size_t side_len, RelHeader* h)
{
  if (!head || side_len < kRelHeaderBytes + 2 * kMaskHeaderBytes)
    return false;
  if (head[0] != 'S' || head[1] != 'P' || head[2] != 'R' || head[3] != 'L' || head[4] != kRelVersion)
    return false;
  if (head[5] > 1 || head[6] != 0 || head[7] != 0 || mask_get_u64(head + 40) != 0)
    return false;
  const RelHeader r{head[5], rel_from_bits(mask_get_u64(head + 8)), mask_get_u64(head + 16), mask_get_u64(head + 24),
                    mask_get_u64(head + 32)};
  double t;
  if ((rel_bits(r.eps) != 0 && !rel_tolerance(r.eps, r.is_float != 0, &t)) || r.n == 0)
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

// ---- the device side (rel.hip) --------------------------------------------------------------------------------------
// bytes of workspace the calls below need for n samples (0: n is refused): the sign bits' mask workspace and a record
size_t rel_workspace_bytes(size_t n);

// what rel_forward_run leaves for the host: valid after the NEXT host wait for the stream
struct RelForward {
  MaskResult sign;      // the sign stream's length and kind, the negative samples
  uint32_t nonfinite;   // not 0: a sample is not finite
};
// k_rel_forward and k_mask_finish on `hip_stream`: y of the n samples at d_src into d_y, the sign bits into `ws`
// (rel_workspace_bytes(n) of device memory, 256-byte aligned).  No host wait.  0 ok, -1 a HIP error
int rel_forward_run(const void* d_src, int is_float, size_t n, double* d_y, void* ws, RelForward* res,
                    void* hip_stream);
// The side stream around a zero stream that stands at d_side + 48 already: the header `h`, the padding and the sign
// stream from `ws`.  No host wait
int rel_side_run(const RelHeader& h, const void* ws, const MaskResult& sign, void* d_side, void* hip_stream);
// x' of the box [lo, lo + dims) of a volume of dims vol, which d_y holds densely as y', into d_dst (floats or doubles;
// d_y itself when doubles); src_float: the side stream's is_float.  The streams' headers are parsed and name the
// volume's n.  No host wait
int rel_inverse_run(const double* d_y, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                    const MaskStream& zero, const MaskStream& sign, int src_float, int output_float, void* d_dst,
                    void* hip_stream);
// The four words of the check into out (the first the bits of a double), with ONE host wait; `ws` as above
int rel_check_run(const void* d_orig, const void* d_recon, int is_float, size_t n, double eps, void* ws,
                  uint64_t out[4], void* hip_stream);

}  // namespace sperrhip

#endif
