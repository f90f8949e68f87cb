// lis_token.h -- the grammar of a list entry of the sorting pass as the decoder's list kernels read it (k_lis_l0 /
// k_lis_l1 / k_lis_l2 / k_lis_hi of speck_dec.hip, k_lis_mx of speck_mx.hip); compiled for the host as well, where
// tests/test_lis_token_host.py checks every function against a bit-by-bit parse.
//
// A set that is found significant is split into its eight children, coded one after the other
// (src/SPECK3D_INT.cpp:140-212): a child is a test bit, and when that bit is '1' the child's own code -- for a pixel
// its sign bit, for a set its split.  The last child of a set none of whose siblings was significant carries no test
// bit: it is significant.
#ifndef SPERR_AMD_LIS_TOKEN_H
#define SPERR_AMD_LIS_TOKEN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sperrhip {

// Bits the split of a set of N pixels takes, from the 32 stream bits v at its start (at most 2 N of them are looked at).
template <int N>
__host__ __device__ __forceinline__ uint32_t pixel_split_len(uint32_t v)
{
  uint32_t y = 0, found = 0;
#pragma unroll
  for (int k = 0; k + 1 < N; k++) {
    const uint32_t bit = (v >> y) & 1u;
    found |= bit;
    y += 1u + bit;
  }
  const uint32_t bit = found ? (v >> y) & 1u : 1u;
  return y + found + bit;
}

// ... of a 2x2x2 set
__host__ __device__ __forceinline__ uint32_t split8_len(uint32_t v)
{
  return pixel_split_len<8>(v);
}

// The same split decoded: bit k of sigm says that pixel k became significant, bit k of negm that it is negative
// (a sign bit of '0': src/SPECK_INT.cpp's m_sign_array holds true for positive values).
__host__ __device__ __forceinline__ void split8_pixels(uint32_t v, uint32_t& sigm, uint32_t& negm)
{
  uint32_t y = 0, found = 0;
  sigm = 0;
  negm = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const uint32_t bit = (v >> y) & 1u, sgn = (v >> (y + 1)) & 1u;
    sigm |= bit << k;
    negm |= (bit & (sgn ^ 1u)) << k;
    found |= bit;
    y += 1u + bit;
  }
  const uint32_t bit = found ? (v >> y) & 1u : 1u;
  const uint32_t sgn = (v >> (y + found)) & 1u;
  sigm |= bit << 7;
  negm |= (bit & (sgn ^ 1u)) << 7;
}

// A leaf parent whose number of pixels n (1 .. 8) is known only at run time (k_lis_hi's class 0 of a tree that is not
// an octree, every leaf parent of k_lis_mx): the bits its split takes ...
__host__ __device__ __forceinline__ uint32_t pixel_split_len_n(uint32_t v, uint32_t n)
{
  uint32_t y = 0, found = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t coded = found | (uint32_t)(k + 1 != n);
    const uint32_t bit = coded ? (v >> y) & 1u : 1u;
    y += coded;
    found |= bit;
    y += bit;
  }
  return y;
}

// ... and the split decoded, masks by child ordinal as split8_pixels gives them
__host__ __device__ __forceinline__ void split_pixels_n(uint32_t v, uint32_t n, uint32_t& sigm, uint32_t& negm)
{
  uint32_t y = 0, found = 0;
  sigm = 0;
  negm = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t coded = found | (uint32_t)(k + 1 != n);
    const uint32_t bit = coded ? (v >> y) & 1u : 1u;
    y += coded;
    const uint32_t sgn = (v >> y) & 1u;
    sigm |= bit << k;
    negm |= (bit & (sgn ^ 1u)) << k;
    found |= bit;
    y += bit;
  }
}

// The leaf-event word a significant leaf parent leaves for k_leaf_apply: its flat node id, and the two masks.
__host__ __device__ __forceinline__ uint64_t leaf_event_pack(uint32_t flatId, uint32_t sigm, uint32_t negm)
{
  return (uint64_t)flatId | ((uint64_t)sigm << 32) | ((uint64_t)negm << 40);
}
__host__ __device__ __forceinline__ void leaf_event_unpack(uint64_t ev, uint32_t& flatId, uint32_t& sigm, uint32_t& negm)
{
  flatId = (uint32_t)ev;
  sigm = (uint32_t)(ev >> 32) & 0xffu;
  negm = (uint32_t)(ev >> 40) & 0xffu;
}

// Bits the split of a set of eight child sets takes when it starts at position y, from the tables of the children's
// class: U[x] = bits of a coded child at x (1: its test bit is '0'; else 1 + its split), T[x] = bits of a child's
// split that starts at x (the last child's when it has no test bit).
template <typename TU, typename TT>
__host__ __device__ __forceinline__ uint32_t parent_split_len(const TU* U, const TT* T, uint32_t y)
{
  const uint32_t y0 = y;
  uint32_t found = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const uint32_t u = U[y];
    found |= u - 1u;
    y += u;
  }
  y += found ? U[y] : T[y];
  return y - y0;
}

// The stream words of a block or region in LDS, read as bits: position r is bit r + q0 of the words at w32.
struct LdsBits {
  const uint32_t* w32;
  uint32_t q0;
  __host__ __device__ __forceinline__ uint32_t bit_at(uint32_t r) const
  {
    const uint32_t q = r + q0;
    return (w32[q >> 5] >> (q & 31)) & 1u;
  }
  __host__ __device__ __forceinline__ uint32_t bits32(uint32_t r) const   // the 32 stream bits that start at r
  {
    const uint32_t q = r + q0, sh = q & 31;
    const uint32_t lo = w32[q >> 5], hi = w32[(q >> 5) + 1];
    return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
  }
};

}  // namespace sperrhip

#endif
