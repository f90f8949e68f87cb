// boxes.h -- a box per entry out of a batch of containers: the ONLY statement of which chunks such a call decodes,
// what each of them writes and where (the entry points of abi.hip, the copy kernel of boxes.hip and the host check
// tests/cpp/boxes_check.cpp all use these).  Plain C++: no HIP here.
//
// A call names `ncont` containers and `nbox` entries.  Entry e is the box [lo_e, lo_e + box) of container which[e]
// (which == NULL: container e), every entry with the same `box` dims, and box e of the output is its element
// e * bx * by * bz: the output is one dense array of dims (bx, by, nbox * bz), x fastest.
//
// The rule is stated on a GRID: `full`, the dims of what the boxes are cut from -- the same for every container -- and
// per container `cell`, the extent of the pieces that tile it, in chunk_volume's manner (all but the last segment of
// an axis start at multiples of the cell, the last one runs to the end of `full`).  At full resolution `full` is the
// volume and `cell` the container's chunk dims; for level h of the hierarchy `full` is the level's dims and `cell` the
// chunks' corner cres[h] (level_select, decode.hip), origins and box dims in the level's coordinates.  Either way cell
// id i of container c is chunk i of that container.
//
//   slots    the distinct (container, cell id) pairs that any entry's box meets (box_chunks per entry).  A slot is
//            decoded once.  ORDER, both forms: ascending by container, then by cell id.
//   pairs    every (entry, slot) that meet, with the window [lo, hi) of the slot's cell that lies in the entry's box
//            (the cell's coordinates) and `at`, where that window starts in box e (the box's coordinates).  ORDER: by
//            entry, within an entry in box_chunks order.  The windows of an entry's pairs tile its box exactly once.
//   shared   some slot belongs to more than one pair: two entries meet the same chunk of the same container.
//   geom     per slot, what the decoder's crop writers take (BoxCrop: the fields of CropGeom, common.h):
//            DIRECT (not shared): the slot's one pair -- rel = cell origin - lo_e with rel[2] + e * bz, lo and hi the
//              pair's window -- so the writers place every chunk in its entry's box themselves and the call's output
//              is the decoder's.  For one entry this is what Window::place + crop_geom give for that box.
//            STAGED (shared): every slot whole -- lo = 0, hi = the cell's extent, rel = (0, 0, z_k) -- into a staging
//              array of dims (largest extent in x, largest extent in y, sum of the slots' z extents), slot k at
//              (0, 0, z_k), z_k the sum of the z extents of the slots before it.  k_boxes_copy (boxes.hip) then moves
//              every pair's window into its box, one launch.
//   refused  nbox or ncont of 0 or beyond 2^32 - 1, a `which` index out of range, which == NULL with nbox != ncont, an
//            extent of 0, a box that leaves `full`, a box dim or nbox * bz or the staging array's z extent beyond
//            INT32_MAX (CropGeom::rel), a cell origin relative to its box that does not fit int32, more than 2^32 - 1
//            pairs (hence slots: both are indexed with 32 bits), an output or a staging array whose value count
//            overflows size_t.  All of this is known before anything is enqueued.
#ifndef SPERR_AMD_BOXES_H
#define SPERR_AMD_BOXES_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "host_container.hpp"

namespace sperrhip {

using hostc::Dims;

// CropGeom's fields (common.h, which needs HIP's headers): cell origin minus box origin, and the cell's window [lo, hi)
struct BoxCrop {
  int32_t rel[3];
  uint32_t lo[3], hi[3];
};

struct BoxesSlot {
  uint32_t cont, id;   // container, and the cell's (the chunk's) id in chunk_volume order
  Dims org, ext;       // the cell on the grid
  size_t stageZ;       // staged form: z of the slot in the staging array
};

struct BoxesPair {
  uint32_t entry, slot;
  uint32_t lo[3], hi[3];   // the window of the slot's cell, the cell's coordinates
  Dims at;                 // where the window starts in box `entry`, the box's coordinates
};

struct BoxesPlan {
  Dims box{0, 0, 0};
  size_t nbox = 0;
  std::vector<BoxesSlot> slots;
  std::vector<BoxesPair> pairs;
  bool shared = false;
  std::vector<BoxCrop> geom;    // per slot: direct or staged, as `shared` says
  Dims outDims{0, 0, 0};        // (bx, by, nbox * bz)
  Dims stageDims{0, 0, 0};      // staged form only
  size_t outVals = 0, stageVals = 0;
};

// the segments [s0, s1] per axis that the box [lo, lo + dims) of `full` meets; false for what box_chunks refuses
inline bool boxes_segments(const Dims& full, const Dims& cell, const Dims& lo, const Dims& dims, size_t s0[3], size_t s1[3])
{
  size_t nseg[3];
  for (int a = 0; a < 3; a++)
    if (full[a] == 0 || cell[a] == 0 || dims[a] == 0 || lo[a] >= full[a] || dims[a] > full[a] - lo[a])
      return false;
  hostc::chunk_segments(full, cell, nseg);
  for (int a = 0; a < 3; a++) {
    s0[a] = std::min(lo[a] / cell[a], nseg[a] - 1);
    s1[a] = std::min((lo[a] + dims[a] - 1) / cell[a], nseg[a] - 1);
  }
  return true;
}

// cell `id` of the grid (chunk_volume order): its origin and extent
inline void boxes_cell(const Dims& full, const Dims& cell, uint32_t id, Dims& org, Dims& ext)
{
  size_t nseg[3];
  hostc::chunk_segments(full, cell, nseg);
  const size_t idx[3] = {id % nseg[0], id / nseg[0] % nseg[1], id / nseg[0] / nseg[1]};
  for (int a = 0; a < 3; a++) {
    org[a] = idx[a] * cell[a];
    ext[a] = idx[a] + 1 == nseg[a] ? full[a] - org[a] : cell[a];
  }
}

inline bool boxes_mul(size_t a, size_t b, size_t* out)
{
  const unsigned __int128 p = (unsigned __int128)a * b;
  *out = (size_t)p;
  return p <= (unsigned __int128)SIZE_MAX;
}

// The plan of a call, or false for everything the header's `refused` lists.  cell: ncont entries; lo: 3 per entry
inline bool boxes_plan(size_t ncont, const Dims& full, const Dims* cell, const uint32_t* which, const size_t* lo,
                       size_t nbox, const Dims& box, BoxesPlan& P)
{
  P = BoxesPlan{};
  if (ncont == 0 || nbox == 0 || ncont > 0xffffffffull || nbox > 0xffffffffull || !cell || !lo)
    return false;
  if (!which && nbox != ncont)
    return false;
  for (int a = 0; a < 3; a++)
    if (box[a] == 0 || box[a] > (size_t)INT32_MAX)
      return false;
  if (nbox > (size_t)INT32_MAX / box[2])
    return false;
  // how many pairs there will be, before any of them is listed
  unsigned __int128 npairs = 0;
  for (size_t e = 0; e < nbox; e++) {
    const size_t c = which ? which[e] : e;
    if (c >= ncont)
      return false;
    size_t s0[3], s1[3];
    if (!boxes_segments(full, cell[c], Dims{lo[3 * e], lo[3 * e + 1], lo[3 * e + 2]}, box, s0, s1))
      return false;
    npairs += (unsigned __int128)(s1[0] - s0[0] + 1) * (s1[1] - s0[1] + 1) * (s1[2] - s0[2] + 1);
    if (npairs > 0xffffffffull)
      return false;
  }
  P.box = box;
  P.nbox = nbox;
  P.outDims = Dims{box[0], box[1], box[2] * nbox};
  if (!boxes_mul(box[0], box[1], &P.outVals) || !boxes_mul(P.outVals, P.outDims[2], &P.outVals))
    return false;
  // the pairs, each with its slot's key for now; the slots are the distinct keys in order
  std::vector<uint64_t> keys;
  std::vector<uint32_t> ids;
  keys.reserve((size_t)npairs);
  P.pairs.reserve((size_t)npairs);
  for (size_t e = 0; e < nbox; e++) {
    const size_t c = which ? which[e] : e;
    if (!hostc::box_chunks(full, cell[c], Dims{lo[3 * e], lo[3 * e + 1], lo[3 * e + 2]}, box, ids))
      return false;
    for (uint32_t id : ids) {
      keys.push_back((uint64_t)c << 32 | id);
      BoxesPair p{};
      p.entry = (uint32_t)e;
      P.pairs.push_back(p);
    }
  }
  std::vector<uint64_t> distinct = keys;
  std::sort(distinct.begin(), distinct.end());
  distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
  P.shared = distinct.size() < keys.size();
  P.slots.resize(distinct.size());
  for (size_t k = 0; k < distinct.size(); k++) {
    BoxesSlot& s = P.slots[k];
    s.cont = (uint32_t)(distinct[k] >> 32);
    s.id = (uint32_t)distinct[k];
    s.stageZ = 0;
    boxes_cell(full, cell[s.cont], s.id, s.org, s.ext);
  }
  for (size_t i = 0; i < P.pairs.size(); i++) {
    BoxesPair& p = P.pairs[i];
    p.slot = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), keys[i]) - distinct.begin());
    const BoxesSlot& s = P.slots[p.slot];
    for (int a = 0; a < 3; a++) {
      const size_t b0 = lo[3 * (size_t)p.entry + a], b1 = b0 + box[a];
      const size_t w0 = std::max(b0, s.org[a]), w1 = std::min(b1, s.org[a] + s.ext[a]);
      p.lo[a] = (uint32_t)(w0 - s.org[a]);
      p.hi[a] = (uint32_t)(w1 - s.org[a]);
      p.at[a] = w0 - b0;
    }
  }
  P.geom.resize(P.slots.size());
  if (!P.shared) {
    for (const BoxesPair& p : P.pairs) {
      const BoxesSlot& s = P.slots[p.slot];
      BoxCrop& g = P.geom[p.slot];
      for (int a = 0; a < 3; a++) {
        int64_t rel = (int64_t)s.org[a] - (int64_t)lo[3 * (size_t)p.entry + a];
        if (a == 2)
          rel += (int64_t)((size_t)p.entry * box[2]);
        if (rel < (int64_t)INT32_MIN || rel > (int64_t)INT32_MAX)
          return false;
        g.rel[a] = (int32_t)rel;
        g.lo[a] = p.lo[a];
        g.hi[a] = p.hi[a];
      }
    }
    return true;
  }
  size_t z = 0;
  for (size_t k = 0; k < P.slots.size(); k++) {
    BoxesSlot& s = P.slots[k];
    BoxCrop& g = P.geom[k];
    s.stageZ = z;
    for (int a = 0; a < 3; a++) {
      if (s.ext[a] > (size_t)INT32_MAX)
        return false;
      g.rel[a] = a == 2 ? (int32_t)z : 0;
      g.lo[a] = 0;
      g.hi[a] = (uint32_t)s.ext[a];
    }
    P.stageDims[0] = std::max(P.stageDims[0], s.ext[0]);
    P.stageDims[1] = std::max(P.stageDims[1], s.ext[1]);
    z += s.ext[2];
    if (z > (size_t)INT32_MAX)
      return false;
  }
  P.stageDims[2] = z;
  return boxes_mul(P.stageDims[0], P.stageDims[1], &P.stageVals) && boxes_mul(P.stageVals, z, &P.stageVals);
}

// ---- the copy kernel's side (boxes.hip) ------------------------------------------------------------------------
// One pair as k_boxes_copy reads it: the element offsets of its window's first sample in the staging array and in the
// output, and the window's extent.  The window's samples, x fastest, are the elements [first[p], first[p + 1]) of the
// run of all pairs' samples, which is what the kernel's workgroups share out
struct BoxesCopyPair {
  uint64_t src, dst;
  uint32_t w[3], pad;
};

struct BoxesCopyGeom {
  uint64_t srcRow, srcSlice, dstRow, dstSlice;   // elements from row to row and from slice to slice, either side
  uint64_t total;                                // samples of all pairs: the output's
  uint32_t npairs;
};

constexpr uint32_t kBoxesThreads = 256;
constexpr uint32_t kBoxesSliceBytes = 16384;   // of the output, per workgroup
constexpr uint32_t kBoxesPackBytes = 16;       // what the kVec form loads and stores at a time

// the staged plan as the kernel takes it: pairs, first (npairs + 1 entries) and the geometry
inline void boxes_copy_args(const BoxesPlan& P, std::vector<BoxesCopyPair>& pairs, std::vector<uint64_t>& first,
                            BoxesCopyGeom& g)
{
  g.srcRow = P.stageDims[0];
  g.srcSlice = (uint64_t)P.stageDims[0] * P.stageDims[1];
  g.dstRow = P.box[0];
  g.dstSlice = (uint64_t)P.box[0] * P.box[1];
  g.npairs = (uint32_t)P.pairs.size();
  pairs.resize(P.pairs.size());
  first.assign(P.pairs.size() + 1, 0);
  for (size_t i = 0; i < P.pairs.size(); i++) {
    const BoxesPair& p = P.pairs[i];
    const BoxesSlot& s = P.slots[p.slot];
    BoxesCopyPair& c = pairs[i];
    c.src = (uint64_t)(s.stageZ + p.lo[2]) * g.srcSlice + (uint64_t)p.lo[1] * g.srcRow + p.lo[0];
    c.dst = (uint64_t)((size_t)p.entry * P.box[2] + p.at[2]) * g.dstSlice + (uint64_t)p.at[1] * g.dstRow + p.at[0];
    for (int a = 0; a < 3; a++)
      c.w[a] = p.hi[a] - p.lo[a];
    c.pad = 0;
    first[i + 1] = first[i] + (uint64_t)c.w[0] * c.w[1] * c.w[2];
  }
  g.total = first[P.pairs.size()];
}

// The kVec form moves 16-byte packs: every row of every window must start on a 16-byte boundary on both sides and be
// a whole number of packs long.  That is so when both arrays start on one and every window's first sample, its width
// and the four pitches are whole packs
inline bool boxes_vec_ok(uintptr_t stage, uintptr_t out, const std::vector<BoxesCopyPair>& pairs, const BoxesCopyGeom& g,
                         size_t elem_size)
{
  const size_t pack = kBoxesPackBytes / elem_size;
  if (stage % kBoxesPackBytes || out % kBoxesPackBytes || g.srcRow % pack || g.srcSlice % pack || g.dstRow % pack ||
      g.dstSlice % pack)
    return false;
  for (const BoxesCopyPair& c : pairs)
    if (c.src % pack || c.dst % pack || c.w[0] % pack)
      return false;
  return true;
}

// One launch of k_boxes_copy on `hip_stream` (a hipStream_t), no host wait: d_pairs and d_first are the device copies
// of what boxes_copy_args made.  elem_size 4 or 8: the kernel moves bits.  0 ok; -1, with nothing launched, for a NULL
// pointer, no pairs, or more workgroups than a grid's x holds.
int boxes_copy_run(const void* d_stage, void* d_out, size_t elem_size, const BoxesCopyPair* d_pairs,
                   const uint64_t* d_first, const BoxesCopyGeom& g, bool vec, void* hip_stream);

}  // namespace sperrhip

#endif
