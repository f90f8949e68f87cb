// engine_parts.h -- what engine.hip (plans, shared state) gives to the encode call (encode.hip) and the decode call
// (decode.hip), and to nobody else: the C ABI and the chunk farm do not include this.  Declarations only; what belongs
// to one direction -- its workspace layout, its call struct -- stays in that direction's unit.
#ifndef SPERR_AMD_ENGINE_PARTS_H
#define SPERR_AMD_ENGINE_PARTS_H

#include "engine_core.h"

namespace sperrhip {

// LiftFuse of pass k (xform.h) as the plan keeps it (LiftSchedule::pass): 0 when no sample of the pass's region is
// left alone by the later passes, 1 when some are (inner = the later passes' box), -1 when it cannot be told
int pass_fuse(const ShapePlan& P, size_t k, uint32_t inner[3]);

// The arena rules.  How much workspace a call may use, given what the engine holds and what is free now: 80 % of the
// two together, capped by SPERR_HIP_ARENA_MAX_MB (arena_cap_env) -- as room for more, or as a budget of at least `have`
size_t arena_room(size_t have, size_t freeNow);
size_t arena_budget(size_t have, size_t freeNow);
// SPERR_HIP_ARENA_DEBUG=1: every array of a batch's workspace with its size, on stderr
bool arena_debug();

// a bit budget as the coder takes it: whole bytes, and none (0) as no limit
uint64_t rounded_budget(uint64_t raw);

// list storage of the 1D coder: level l holds at most 2^l runs, and never more than `most`
void speck1d_level_offsets(OutlierBufs& ob, uint32_t N, uint64_t most);

// The brick inverse: what a decoder reconstructs of a batch, in the conditioned domain, as doubles in the chunk buffer
// -- for the encoder's point-wise error stage and for the decoder's outlier correctors, which both need the values
// before the mean is added.  By the decoder's own fused kernels: the coarser levels (passes k >= 3) in a compact
// buffer of their box, dequantising as they load (LiftFuse mode 2), the finest level by k_lift_xyz_inv writing doubles
// into the chunk buffer as if it were a volume of bricks (a chunk's offset rides in org[0], hence the 32-bit guard; no
// mean added) -- instead of an inverse quantiser pass and fifteen per-axis passes over the whole chunk (14.9 of the
// 56 ms a 1024^3 volume took to compress in PWE mode; 12.7 ms for 64 chunks of 256^3 with correctors to decode).
// Never the second level as one launch: the box is one buffer, and k_lift2_inv cannot work in place.
// A caller adds its own conditions to brick_inverse_fits: no chunk of the batch may have 64-bit coefficients.
bool brick_inverse_fits(const ShapePlan& P, uint32_t nb, size_t valsStride);
// box: the engine's buffer for the coarser levels' box and the bricks; bricks: the host copy of the latter, which has
// to live until the stream has taken it
int enqueue_brick_inverse(hipStream_t st, const ShapePlan& P, DevBuf& box, std::vector<ChunkGeom>& bricks, uint32_t nb,
                          double* vals, size_t valsStride, CoderState* cst, const ChunkGeom* geom, const DequantSrc& src);

// f(float{}) or f(double{}): the element type an entry point's is_float / output_float names
template <typename F>
int with_elem(int is_float, F&& f)
{
  return is_float ? f(float{}) : f(double{});
}

}  // namespace sperrhip

#endif
