// mask.h -- missing values: the ONLY statement of the three rules (the entry points of abi_mask.hip, the kernels of
// mask.hip and the host check tests/cpp/mask_check.cpp all use these).  Plain C++: no HIP here.
//
// A masked volume is an ordinary container of the IN-FILLED volume -- every missing sample replaced by one finite
// value F -- and a MASK STREAM that says which samples were missing.
//
//   missing   rule 1 (kMaskRuleNan)    x != x
//             rule 2 (kMaskRuleAbsGe)  !(fabs(x) < threshold), the sample widened to double: the sentinel, both
//                                      infinities and NaN.  threshold is finite and > 0
//   fill      lo and hi are the smallest and largest VALID sample under the total order of the sign-magnitude bit
//             patterns (mask_key: -0.0 < +0.0, so the pair does not depend on the order of evaluation).  Both widened
//             to double, F = 0.5 * lo + 0.5 * hi in double, narrowed once to float for fp32 data.  No valid sample:
//             F = 0.  lo or hi not finite (an infinity under rule 1): the call fails
//   stream    little-endian; a sample's index is its linear index, x fastest; bit 1 means missing
//               0-3 "SPMK" | 4 version 1 | 5 kind | 6-7 0 | 8-15 n | 16-23 nmissing | 24-31 count | 32- payload
//             kind 0  nothing missing: count 0, no payload
//             kind 1  toggles: count ascending uint32 positions p with bit(p) != bit(p - 1), bit(-1) = 0
//             kind 2  bits: count = ceil(n / 64) 64-bit words, sample i is bit i % 64 of word i / 64, tail bits 0
//             nmissing == 0 gives kind 0; otherwise kind 1 when n <= 2^32 and 4 * toggles < 8 * ceil(n / 64);
//             otherwise kind 2
//
// A stream that is handed in has its header checked (mask_parse); its payload is trusted: every lane of every
// reader writes its own sample only, so a damaged payload gives wrong samples and no write outside the output.
#ifndef SPERR_AMD_MASK_H
#define SPERR_AMD_MASK_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "view.h"

namespace sperrhip {

constexpr int kMaskRuleNan = 1, kMaskRuleAbsGe = 2;
constexpr int kMaskKindNone = 0, kMaskKindToggles = 1, kMaskKindBits = 2;
constexpr size_t kMaskHeaderBytes = 32;
constexpr uint8_t kMaskVersion = 1;

// ---- the kernels' constants ------------------------------------------------------------------------------------
// samples one wavefront takes at a time, in every kernel of mask.hip: 16 words of the bit array.  A tile's missing
// and toggle counts depend on its own samples and on the one sample before it, nothing else.
constexpr uint32_t kMaskTile = 1024;
constexpr uint32_t kMaskTileWords = kMaskTile / 64;
constexpr uint32_t kMaskThreads = 256;        // a workgroup: four wavefronts, four tiles at a time
constexpr uint32_t kMaskGroupsPerCU = 8;      // the grid's cap; the tiles beyond it are walked
constexpr uint32_t kMaskPackBytes = 16;       // what the 16-byte forms load and store per lane

// ---- which samples are missing ---------------------------------------------------------------------------------
SPERR_VIEW_FN bool mask_rule_ok(int rule, double threshold)
{
  if (rule == kMaskRuleNan)
    return true;
  return rule == kMaskRuleAbsGe && threshold > 0.0 && threshold <= 1.79769313486231570815e308;
}

template <typename T>
SPERR_VIEW_FN bool mask_missing(T x, int rule, double threshold)
{
  return rule == kMaskRuleNan ? x != x : !(fabs((double)x) < threshold);
}

// ---- the order of the valid samples ----------------------------------------------------------------------------
// the key of a sample: unsigned keys compare as the sign-magnitude bit patterns do
SPERR_VIEW_FN uint64_t mask_key(double x)
{
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | (uint64_t(1) << 63));
}
SPERR_VIEW_FN uint64_t mask_key(float x)   // (a 32-bit key in the low half)
{
  uint32_t u;
  memcpy(&u, &x, 4);
  return (u >> 31) ? (uint32_t)~u : (u | (uint32_t(1) << 31));
}
// ... and back, widened to double
SPERR_VIEW_FN double mask_unkey(uint64_t k, bool is_float)
{
  if (is_float) {
    const uint32_t k32 = (uint32_t)k, u = (k32 >> 31) ? (k32 & 0x7fffffffu) : ~k32;
    float f;
    memcpy(&f, &u, 4);
    return (double)f;
  }
  const uint64_t u = (k >> 63) ? (k & ~(uint64_t(1) << 63)) : ~k;
  double d;
  memcpy(&d, &u, 8);
  return d;
}
constexpr uint64_t kMaskKeyNone = ~uint64_t(0);   // lo of no sample; hi of no sample is 0

// F from the keys of lo and hi; *finite false when either is an infinity (the call then fails).  For fp32 data the
// result is the narrowed float, widened again: the fill pass casts it back without a change
SPERR_VIEW_FN double mask_fill_value(uint64_t lo_key, uint64_t hi_key, bool any_valid, bool is_float, bool* finite)
{
  *finite = true;
  if (!any_valid)
    return 0.0;
  const double lo = mask_unkey(lo_key, is_float), hi = mask_unkey(hi_key, is_float);
  if (!(fabs(lo) <= 1.79769313486231570815e308) || !(fabs(hi) <= 1.79769313486231570815e308)) {
    *finite = false;
    return 0.0;
  }
  const double a = 0.5 * lo, b = 0.5 * hi;
  const double f = a + b;
  return is_float ? (double)(float)f : f;
}

// ---- the stream ------------------------------------------------------------------------------------------------
struct MaskHeader {
  int kind;
  uint64_t n, nmissing, count;
};

SPERR_VIEW_FN uint64_t mask_words(uint64_t n) { return n / 64 + (n % 64 != 0); }
// sperrhip_mask_max_size: a stream of bits; a stream of toggles is chosen only where it is shorter
SPERR_VIEW_FN size_t mask_max_size(size_t n) { return kMaskHeaderBytes + 8 * (size_t)mask_words(n); }

SPERR_VIEW_FN int mask_choose_kind(uint64_t n, uint64_t nmissing, uint64_t toggles)
{
  if (nmissing == 0)
    return kMaskKindNone;
  // (toggles <= n <= 2^32: the product cannot wrap)
  if (n <= (uint64_t(1) << 32) && 4 * toggles < 8 * mask_words(n))
    return kMaskKindToggles;
  return kMaskKindBits;
}

SPERR_VIEW_FN uint64_t mask_payload_bytes(int kind, uint64_t count)
{
  return kind == kMaskKindToggles ? 4 * count : kind == kMaskKindBits ? 8 * count : 0;
}

// the header of a volume of n samples with nmissing missing ones whose bit array has `toggles` toggles
SPERR_VIEW_FN MaskHeader mask_header_of(uint64_t n, uint64_t nmissing, uint64_t toggles)
{
  const int kind = mask_choose_kind(n, nmissing, toggles);
  return MaskHeader{kind, n, nmissing,
                    kind == kMaskKindToggles ? toggles : kind == kMaskKindBits ? mask_words(n) : uint64_t(0)};
}

SPERR_VIEW_FN void mask_put_u64(uint8_t* p, uint64_t v)
{
  for (int i = 0; i < 8; i++)
    p[i] = (uint8_t)(v >> (8 * i));
}
SPERR_VIEW_FN uint64_t mask_get_u64(const uint8_t* p)
{
  uint64_t v = 0;
  for (int i = 0; i < 8; i++)
    v |= (uint64_t)p[i] << (8 * i);
  return v;
}

SPERR_VIEW_FN void mask_write_header(const MaskHeader& h, uint8_t out[kMaskHeaderBytes])
{
  out[0] = 'S';
  out[1] = 'P';
  out[2] = 'M';
  out[3] = 'K';
  out[4] = kMaskVersion;
  out[5] = (uint8_t)h.kind;
  out[6] = out[7] = 0;
  mask_put_u64(out + 8, h.n);
  mask_put_u64(out + 16, h.nmissing);
  mask_put_u64(out + 24, h.count);
}

// The header of a stream of mask_len bytes whose first min(mask_len, 32) bytes are at `head`: magic, version, kind,
// the reserved bytes, nmissing <= n, count against the kind and n, and the payload's length against mask_len exactly.
// false: the stream is refused
SPERR_VIEW_FN bool mask_parse(const uint8_t* head, size_t mask_len, MaskHeader* h)
{
  if (!head || mask_len < kMaskHeaderBytes)
    return false;
  if (head[0] != 'S' || head[1] != 'P' || head[2] != 'M' || head[3] != 'K' || head[4] != kMaskVersion)
    return false;
  if (head[5] > kMaskKindBits || head[6] != 0 || head[7] != 0)
    return false;
  const MaskHeader r{head[5], mask_get_u64(head + 8), mask_get_u64(head + 16), mask_get_u64(head + 24)};
  if (r.n == 0 || r.nmissing > r.n)
    return false;
  if (r.kind == kMaskKindNone && (r.count != 0 || r.nmissing != 0))
    return false;
  if (r.kind == kMaskKindToggles && (r.n > (uint64_t(1) << 32) || r.count == 0 || r.count > r.n || r.nmissing == 0))
    return false;
  if (r.kind == kMaskKindBits && (r.count != mask_words(r.n) || r.nmissing == 0))
    return false;
  if (r.count > (SIZE_MAX - kMaskHeaderBytes) / 8 || mask_len - kMaskHeaderBytes != mask_payload_bytes(r.kind, r.count))
    return false;
  *h = r;
  return true;
}

// ---- words and toggles -----------------------------------------------------------------------------------------
// the toggle bits of a word: bit j set when sample j of the word differs from the sample before it; `carry` is the
// top bit of the previous word (0 before the first); `nbits` (1..64) of the word are samples
SPERR_VIEW_FN uint64_t mask_toggle_bits(uint64_t w, uint64_t carry, uint32_t nbits)
{
  const uint64_t t = w ^ ((w << 1) | carry);
  return nbits >= 64 ? t : t & ((uint64_t(1) << nbits) - 1);
}

// The 64 samples [s, s + 64) of a stream of toggles as a word: `state` is bit(s - 1) on entry and bit(s + 63) on
// return, `idx` the index of the first toggle at or behind s on entry and of the first at or behind s + 64 on return
SPERR_VIEW_FN uint64_t mask_word_from_toggles(const uint32_t* tog, uint64_t count, uint64_t s, uint64_t* idx,
                                              uint64_t* state)
{
  uint64_t w = *state ? ~uint64_t(0) : 0;
  uint64_t i = *idx;
  while (i < count && (uint64_t)tog[i] - s < 64) {   // (tog[i] >= s holds on entry)
    w ^= ~uint64_t(0) << ((uint64_t)tog[i] - s);
    i++;
  }
  *idx = i;
  *state = w >> 63;
  return w;
}

// index of the first toggle at or behind sample s: the number of toggles before s, whose low bit is bit(s - 1)
SPERR_VIEW_FN uint64_t mask_toggle_lower_bound(const uint32_t* tog, uint64_t count, uint64_t s)
{
  uint64_t lo = 0, hi = count;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)tog[mid] < s)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- the 16-byte forms -----------------------------------------------------------------------------------------
// A lane of the 16-byte forms holds P = 4 (float) or 2 (double) consecutive samples, so ballot j of a wavefront has
// the bits of samples P * lane + j.  Word w of the P words a wavefront's load covers is lanes [64 / P * w, ...) of
// every ballot, interleaved: mask_spread puts bit i of a 64 / P-bit piece at bit P * i.
template <uint32_t P>
SPERR_VIEW_FN uint64_t mask_spread(uint64_t x);
template <>
SPERR_VIEW_FN uint64_t mask_spread<1>(uint64_t x)
{
  return x;
}
template <>
SPERR_VIEW_FN uint64_t mask_spread<2>(uint64_t x)   // 32 bits
{
  x &= 0xffffffffull;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}
template <>
SPERR_VIEW_FN uint64_t mask_spread<4>(uint64_t x)   // 16 bits
{
  x &= 0xffffull;
  x = (x | (x << 24)) & 0x000000ff000000ffull;
  x = (x | (x << 12)) & 0x000f000f000f000full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}
// word w (< P) of the samples a wavefront's 16-byte loads cover, from its P ballots
template <uint32_t P>
SPERR_VIEW_FN uint64_t mask_word_of_ballots(const uint64_t* ballot, uint32_t w)
{
  uint64_t r = 0;
  for (uint32_t j = 0; j < P; j++)
    r |= mask_spread<P>(ballot[j] >> (64 / P * w)) << j;
  return r;
}

// ---- the device side (mask.hip) --------------------------------------------------------------------------------
// what k_mask_finish leaves for the one read-back of a call that makes a mask
struct MaskResult {
  uint64_t mask_len, nmissing, finite, kind;
};

// bytes of workspace mask_scan_run needs for n samples (0: n is 0 or the sizes overflow), and mask_compact_run
size_t mask_workspace_bytes(size_t n);
// in that workspace: the bit array k_mask_survey stores, and MaskResult::finite of the read-back record (NULL: n is
// refused).  mask_fill.hip reads the one and sets the other
const uint64_t* mask_bit_words(void* ws, size_t n);
uint64_t* mask_result_finite(void* ws, size_t n);

// what stands at the missing samples (mask_fill.h: the kinds, the smooth rule).  kMaskFillValue: `value` as the
// samples hold it.  kMaskFillSmooth: the levels of the volume and the pyramid buffer, plan->bytes of device memory
struct MaskFillPlan;
struct MaskFill {
  int kind;
  double value;
  const MaskFillPlan* plan;
  void* pyr;
};

// The first half of making a mask: k_mask_survey and k_mask_finish on `hip_stream` -- and behind them the pull of a
// smooth fill (mask_fill_pull_run) --, then ONE host wait for *res.  res->finite is the midrange rule's refusal, and
// under a smooth fill the smooth rule's.
// `ws`: mask_workspace_bytes(n) of device memory, 256-byte aligned; it keeps the bit array, the fill value and the
// header for the second half.  0 ok, -1 a HIP error
int mask_scan_run(const void* d_src, int is_float, size_t n, int rule, double threshold, void* ws, MaskResult* res,
                  void* hip_stream, const MaskFill* fill = nullptr);
// The second half, no host wait: the stream of res.mask_len bytes into d_mask (k_mask_pack; NULL: none) and the
// in-filled samples into d_filled (NULL: none; may be d_src): k_mask_fill with F (`fill` NULL or the midrange) or
// with the caller's value, or the push of a smooth fill (mask_fill_push_run)
int mask_pack_fill_run(const void* d_src, int is_float, size_t n, const void* ws, const MaskResult& res, void* d_mask,
                       void* d_filled, void* hip_stream, const MaskFill* fill = nullptr);

// ---- a bit array another unit's kernel made (rel.hip: the signs of a volume) ----------------------------------------
// Where such a kernel leaves what k_mask_survey would, in a workspace `ws` of mask_workspace_bytes(n): the words of the
// bit array (tail bits 0), every tile's toggle count against the sample before the tile, and per workgroup the record
// {lo key, hi key, bits set} -- mask_key of doubles; a kernel with no order of its own writes mask_key(0.0) twice.
// *res is the device address of the read-back record.  At most kMaskBitsMaxGroups workgroups.  false: n is refused
constexpr uint32_t kMaskBitsMaxGroups = 8192;
struct MaskBitsParts {
  uint64_t* words;
  uint32_t* tileTog;
  uint64_t* partials;
  const MaskResult* res;
};
bool mask_bits_parts(void* ws, size_t n, MaskBitsParts* parts);
// k_mask_finish over `ngroups` such records on `hip_stream`: the kind, the tiles' toggle offsets, the header and *res.
// No host wait; mask_pack_fill_run with the record read back (d_src any non-null pointer, d_filled NULL) then writes
// the stream
int mask_bits_finish_run(void* ws, size_t n, uint32_t ngroups, void* hip_stream);

// a stream on the device, header already parsed: d_payload is d_mask + 32 (8-byte aligned)
struct MaskStream {
  MaskHeader h;
  const void* d_payload;
};
// `value` into the missing samples of the box [lo, lo + dims) of a volume of dims vol, which d_box holds densely;
// nothing else is stored.  Kind 0 launches nothing.  No host wait
int mask_apply_run(void* d_box, int is_float, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                   const MaskStream& m, double value, void* hip_stream);
// the mask as n bytes of 0 / 1
int mask_expand_run(const MaskStream& m, unsigned char* d_out, void* hip_stream);
// The valid samples of nsrc (1 or 2) arrays of h.n samples in linear order into d_dst[i]; `ws` as above.  No host wait
int mask_compact_run(const void* const* d_src, void* const* d_dst, int nsrc, int is_float, const MaskStream& m,
                     void* ws, void* hip_stream);

}  // namespace sperrhip

#endif
