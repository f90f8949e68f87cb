// rel_walk.h -- what the kernels of the two map kinds of point-wise relative error share (rel.hip: the linear kind, the
// header and the check; rel_log.hip: the log kind): the 16-byte packs, the grid, the readers of an SPMK stream and the
// box a decode walks.  Device code of those two units only; everything is private to the unit that includes it.
#ifndef SPERR_AMD_REL_WALK_H
#define SPERR_AMD_REL_WALK_H

#include "common.h"
#include "rel.h"

namespace sperrhip {

namespace {

constexpr uint32_t kWavesPerGroup = kMaskThreads / 64;

typedef float Float4 __attribute__((ext_vector_type(4)));
typedef double Double2 __attribute__((ext_vector_type(2)));
template <typename T>
struct RelPack;
template <>
struct RelPack<float> {
  typedef Float4 type;
};
template <>
struct RelPack<double> {
  typedef Double2 type;
};

inline int rel_grid(uint64_t items, uint32_t* groups)
{
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const uint64_t cap = std::min<uint64_t>((uint64_t)std::max(cus, 1) * kMaskGroupsPerCU, kMaskBitsMaxGroups);
  const uint64_t want = (items + kWavesPerGroup - 1) / kWavesPerGroup;
  *groups = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
  return 0;
}

// ---- readers of an SPMK stream, as mask.hip's kernels read one (its MaskSrc, mask_cursor and mask_next64 are private to
// that unit, whose code object this one leaves as it is) --------------------------------------------------------------
struct BitSrc {
  const uint64_t* words;   // kind 2
  const uint32_t* tog;     // kind 1
  uint64_t count;
  int kind;
};

struct BitCursor {
  uint64_t idx, state;
};

__device__ __forceinline__ BitCursor bit_cursor(const BitSrc& m, uint64_t s)
{
  BitCursor c{0, 0};
  if (m.kind == kMaskKindToggles) {
    c.idx = mask_toggle_lower_bound(m.tog, m.count, s);
    c.state = c.idx & 1;
  }
  return c;
}

// the samples [s, s + 64) as a word (the bits at or behind n mean nothing); calls of a cursor go upwards in s
__device__ __forceinline__ uint64_t bit_next64(const BitSrc& m, BitCursor& c, uint64_t s)
{
  if (m.kind == kMaskKindBits) {
    const uint64_t wi = s >> 6;
    const uint32_t sh = (uint32_t)(s & 63);
    uint64_t w = m.words[wi] >> sh;
    if (sh && wi + 1 < m.count)
      w |= m.words[wi + 1] << (64 - sh);
    return w;
  }
  if (m.kind == kMaskKindToggles)
    return mask_word_from_toggles(m.tog, m.count, s, &c.idx, &c.state);
  return 0;
}

inline BitSrc bit_src(const MaskStream& m)
{
  return BitSrc{static_cast<const uint64_t*>(m.d_payload), static_cast<const uint32_t*>(m.d_payload), m.h.count,
                m.h.kind};
}

struct RelBox {
  uint64_t vx, vy;          // the volume's row and slice extents
  uint64_t lx, ly, lz;      // the box's origin
  uint64_t bx, by, rows;    // the box's row length, rows per slice, rows in all
  uint64_t pieces;          // kMaskTile pieces of a row
};

// the box [lo, lo + dims) of a volume of dims vol whose streams name n samples; the whole volume is one row of n
inline RelBox rel_box_of(const size_t vol[3], const size_t lo[3], const size_t dims[3], uint64_t n)
{
  RelBox g;
  const bool whole = dims[0] == vol[0] && dims[1] == vol[1] && dims[2] == vol[2];
  if (whole)
    g = RelBox{n, 1, 0, 0, 0, n, 1, 1, 0};
  else
    g = RelBox{vol[0], vol[1], lo[0], lo[1], lo[2], dims[0], dims[1], (uint64_t)dims[1] * dims[2], 0};
  g.pieces = (g.bx + kMaskTile - 1) / kMaskTile;
  return g;
}

}  // namespace

// ---- rel_log.hip: the log kind's kernels, which rel_forward_run and rel_inverse_run launch for kind = kRelLog --------
// k_rel_log_forward in k_rel_forward's place: the same arguments, the same results
int rel_log_forward_launch(const void* d_src, int is_float, size_t n, double* d_y, const MaskBitsParts& w,
                           uint32_t* d_nonfinite, uint32_t groups, void* hip_stream);
// rel_inverse_run with k_rel_log_inverse
int rel_log_inverse_run(const double* d_y, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                        const MaskStream& zero, const MaskStream& sign, int src_float, int output_float, void* d_dst,
                        void* hip_stream);

}  // namespace sperrhip

#endif
