// dequant.h -- how a decoded integer coefficient becomes a wavelet sample: the ONLY statement of it (the kernels of
// speck_dec.hip, xform.hip (k_inv_quantize), lift_axis.hip, lift_xyz_inv.h and decode.hip that do it on their way all
// call these; compiled for the host as well,
// where tests/test_dequant_host.py compares every function bit for bit with the reference's two statements)
//
//   1. A coefficient that became significant but was never refined still holds 0 and is completed: 1.5 * 2^p - 1, p the
//      last decoded plane (found during it: the decoder's mask sigNew) or the plane above it (found on the plane
//      before, untouched by a complete refinement pass: sigOld) -- src/SPECK_INT.cpp:216-220,462-468.
//   2. The sample is q * double(c) * (+-1.0), evaluated left to right -- src/SPECK_FLT.cpp:373-399.
//   3. Where k_ref_assemble has left the coefficient complete with its sign in the word (coef_scheme 1 or 2), the
//      word is unpacked first and neither the sign array nor the masks are read.
//
// Two sign conventions, and where each holds:
//   the sign ARRAY (DecBuffers::sign, EncBuffers::sign, DequantSrc::sign)   a set bit is POSITIVE
//                                                                            (src/SPECK_INT.cpp:174-175);
//   BIT 31 of a packed word (coef_scheme_pack)                               a set bit is NEGATIVE, the sign bit of
//                                                                            the double it becomes.
// Every function below that takes a sign takes `positive`; only coef_scheme_pack / dequant_signed know of bit 31.
#ifndef SPERR_AMD_DEQUANT_H
#define SPERR_AMD_DEQUANT_H

#include <string.h>

#include "speck_dec.h"

namespace sperrhip {

// rule 1: thr + thr - thr / 2 - 1 with thr = 2^plane, as the reference writes it
template <typename CT>
__host__ __device__ __forceinline__ CT never_refined(int plane)
{
  const CT thr = (CT)1 << plane;
  return thr + thr - thr / 2 - 1;
}

// rule 2
template <typename CT>
__host__ __device__ __forceinline__ double dequant_value(double q, CT mag, bool positive)
{
  return q * (double)mag * (positive ? 1.0 : -1.0);
}

// How k_ref_assemble hands a chunk's finished 32-bit coefficients to the dequantising inverse passes when the host
// asks for it (DecBuffers::coefSigned, DequantSrc::coefSigned): with the SIGN IN BIT 31, so that those passes read
// neither the sign nor the mask words.  Fixed-rate mode quantises to the full range of uint32_t
// (src/SPECK_FLT.cpp:282-290), so a magnitude may need all 32 bits; but a decoded magnitude is
// m + 2^(q-1) - 1 with q the lowest plane the sample was refined on (src/SPECK_INT.cpp:440-468): odd whenever q >= 2.
//   1: at most 31 planes -- the magnitude, sign in bit 31
//   2: 32 planes, every q of the chunk >= 2 (the stream ran out at plane 2 or above) -- half the magnitude rounded
//      down, sign in bit 31 (a non-zero magnitude is 2 t + 1)
//   0: neither: magnitudes as they are, sign and masks read as ever
__host__ __device__ __forceinline__ int coef_scheme(const DecState& s)
{
  if (s.nbp <= 31)
    return 1;
  const int refPlane = s.refPlaneP1 - 1;
  const int qmin = (refPlane >= 0 && refPlane < s.lastPlane) ? refPlane : s.lastPlane;
  return qmin >= 2 ? 2 : 0;
}
// the word of a complete magnitude and its sign (scheme 0: the magnitude)
__host__ __device__ __forceinline__ uint32_t coef_scheme_pack(uint32_t mag, bool positive, int scheme)
{
  if (scheme == 0)
    return mag;
  return (scheme == 2 ? mag >> 1 : mag) | (positive ? 0u : 0x80000000u);
}
// the magnitude of such a word (scheme 1 or 2)
__host__ __device__ __forceinline__ uint32_t coef_scheme_mag(uint32_t stored, bool two)
{
  const uint32_t t = stored & 0x7fffffffu;
  return (two && t) ? 2u * t + 1u : t;
}

// What a chunk's coefficients need beside themselves, made once per chunk: q, the two values of rule 1 (0 where the
// call has no masks: nothing is completed then) and the chunk's scheme (0 unless the caller's words are packed)
template <typename CT>
struct DequantRule {
  double q;
  CT fillNew, fillOld;
  int scheme;
  bool two;   // scheme == 2
};
// masks: the call has the decoder's masks and s, the chunk's decoder state, which is not read otherwise (the encoder's
// reconstruction of its own coefficients has neither)
template <typename CT>
__host__ __device__ __forceinline__ DequantRule<CT> dequant_rule(double q, bool masks, const DecState* s, bool packed = false)
{
  const int p = masks ? s->lastPlane : 0;
  DequantRule<CT> r;
  r.q = q;
  r.fillNew = masks ? never_refined<CT>(p) : (CT)0;
  // (a sample found on the plane above the last one: there is none when that plane does not exist)
  r.fillOld = (masks && (unsigned)p < 8 * sizeof(CT) - 1) ? never_refined<CT>(p + 1) : (CT)0;
  r.scheme = (masks && packed) ? coef_scheme(*s) : 0;
  r.two = r.scheme == 2;
  return r;
}

// rules 1 and 2: the sample of the magnitude `mag` as the decoder left it, completed by its bit of the two masks.  Bit
// `sh` of the three words is the sample's: of the decoder's masks and of the sign array (the callers hold 64-bit words
// or 32-bit halves of them)
template <typename CT, typename W>
__host__ __device__ __forceinline__ double dequant_masks(const DequantRule<CT>& r, CT mag, W newWord, W oldWord,
                                                         W signWord, uint32_t sh)
{
  const CT fill = ((newWord >> sh) & 1u) ? r.fillNew : (((oldWord >> sh) & 1u) ? r.fillOld : (CT)0);
  return dequant_value<CT>(r.q, mag ? mag : fill, ((signWord >> sh) & 1u) != 0);
}

// rules 3 and 2: the sample of a packed word (r.scheme 1 or 2).  The sign goes from bit 31 of the word to bit 63 of
// the product: q * double(mag) * -1.0 exactly, a zero included
__host__ __device__ __forceinline__ double dequant_signed(const DequantRule<uint32_t>& r, uint32_t word)
{
  const double d = r.q * (double)coef_scheme_mag(word, r.two);
#ifdef __HIP_DEVICE_COMPILE__
  // (the high word through the intrinsics: one v_bitop3_b32 per value; taken apart and put together by shifts, the
  // portable way below, it costs two instructions more.  The host test does not see this line: the kernels' output
  // against the reference's, tests/test_gpu_dequant_sites.py, does)
  return __hiloint2double(__double2hiint(d) ^ (int)(word & 0x80000000u), __double2loint(d));
#else
  uint64_t b;
  memcpy(&b, &d, 8);
  b ^= (uint64_t)(word & 0x80000000u) << 32;
  double out;
  memcpy(&out, &b, 8);
  return out;
#endif
}

}  // namespace sperrhip

#endif
