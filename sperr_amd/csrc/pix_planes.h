// pix_planes.h -- what one thread of k_emit_pixels (speck_enc.hip) holds and computes of its 16 samples: the magnitudes
// as PLANE MASKS (bit k of plane pl = bit pl of sample k), the "msb above / equal to the plane" masks that follow from
// them, and the LIP tokens with their sign bits.  Plain integer code for host and device: tests/test_pix_planes_host.py
// builds a program around it that checks every piece against the per-sample definitions it replaced.
#ifndef SPERR_AMD_PIX_PLANES_H
#define SPERR_AMD_PIX_PLANES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

namespace sperrhip {

// 16 magnitudes of 32 bits -> 32 plane masks of 16 bits, in place and two to a register: in, r[k] = magnitude of sample
// k; out, the low half of r[j] is plane j and the high half plane j + 16.  The two 16 x 16 bit matrices a register's
// halves make up are transposed at once: four stages of masked swaps (Hacker's Delight 7-3), 32 swaps of six operations.
PP_HD void pix_transpose16(uint32_t (&r)[16])
{
#define PP_SWAP_STAGE(S, MASK)                                   \
  _Pragma("unroll") for (int i = 0; i < 16; i++) if (!(i & S)) { \
    const uint32_t t = ((r[i] >> S) ^ r[i + S]) & MASK;          \
    r[i + S] ^= t;                                               \
    r[i] ^= t << S;                                              \
  }
  PP_SWAP_STAGE(8, 0x00ff00ffu)
  PP_SWAP_STAGE(4, 0x0f0f0f0fu)
  PP_SWAP_STAGE(2, 0x33333333u)
  PP_SWAP_STAGE(1, 0x55555555u)
#undef PP_SWAP_STAGE
}

// plane pl (0 .. 31) of the transposed samples: bit k = bit pl of sample k
PP_HD uint32_t pix_plane(const uint32_t (&P)[16], int pl)
{
  return (P[pl & 15] >> (pl & 16)) & 0xffffu;
}

// One plane down.  In: gt = the samples whose msb is above plane p, cp = plane p.  Out: eq = those whose msb IS p,
// gt = those whose msb is above p - 1.  (Nothing is set above a sample's msb, so "bit p set and none above" is all
// there is to it; a zero sample, msb -1, never shows up in either.)
PP_HD void pix_msb_step(uint32_t cp, uint32_t& gt, uint32_t& eq)
{
  eq = cp & ~gt;
  gt |= cp;
}

// --- 16-bit pext, a nibble at a time ---------------------------------------------------------------------------
// entry [mask nibble * 16 + value nibble]: the value's bits at the mask's set positions, packed
PP_HD uint8_t pix_pext_entry(uint32_t mk, uint32_t vl)
{
  uint32_t r = 0, o = 0;
  for (int i = 0; i < 4; i++)
    if ((mk >> i) & 1u) {
      r |= ((vl >> i) & 1u) << o;
      o++;
    }
  return (uint8_t)r;
}

// bits of `val` at the set positions of the 16-bit `mask`, packed
template <typename LUT>
PP_HD uint32_t pix_pext16(const LUT& lut, uint32_t val, uint32_t mask)
{
  uint32_t r = 0, sh = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t mn = (mask >> (4 * i)) & 15u;
    r |= (uint32_t)lut[mn * 16 + ((val >> (4 * i)) & 15u)] << sh;
    sh += (uint32_t)__builtin_popcount(mn);
  }
  return r;
}

// --- LIP tokens with their signs -------------------------------------------------------------------------------
// The scan writes one token per sample -- '1': found significant -- and behind every '1' that sample's sign.
// entry [token nibble * 16 + sign nibble]: the four tokens expanded, 4 + popcount(tokens) bits
PP_HD uint8_t pix_sign_entry(uint32_t tn, uint32_t sn)
{
  uint32_t r = 0, o = 0;
  for (int i = 0; i < 4; i++) {
    r |= ((tn >> i) & 1u) << o;
    o++;
    if ((tn >> i) & 1u) {
      r |= ((sn >> i) & 1u) << o;
      o++;
    }
  }
  return (uint8_t)r;
}

// `tok` / `sgn`: the tokens and signs of the thread's nl <= 16 LIP samples (bit i: the i-th of them; nothing set at or
// above nl).  Returns the bits the scan writes for them, nl + popcount(tok) of them.
template <typename LUT>
PP_HD uint32_t pix_sign_expand(const LUT& lut, uint32_t tok, uint32_t sgn)
{
  uint32_t r = 0, sh = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t tn = (tok >> (4 * i)) & 15u;
    r |= (uint32_t)lut[tn * 16 + ((sgn >> (4 * i)) & 15u)] << sh;
    sh += 4u + (uint32_t)__builtin_popcount(tn);
  }
  return r;
}

}  // namespace sperrhip

#endif
