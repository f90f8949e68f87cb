// mask_calls.h -- what the C ABI of missing values (abi_mask.hip) and of relative error (abi_rel.hip) share: a mask
// stream's header read from the device, how such a call ends, the first half of making a mask, a call's fill.  Internal.
#ifndef SPERR_AMD_MASK_CALLS_H
#define SPERR_AMD_MASK_CALLS_H

#include "decode_request.h"
#include "mask.h"
#include "mask_fill.h"

namespace sperrhip {

// the header of a stream on the device, checked (mask_parse); d_mask must be 8-byte aligned: its payload is words
inline int read_mask_stream(const void* d_mask, size_t mask_len, MaskStream& m, hipStream_t st)
{
  if (!d_mask || mask_len < kMaskHeaderBytes || (uintptr_t)d_mask % 8 != 0)
    return -1;
  uint8_t head[kMaskHeaderBytes];
  HIP_CHECK(hipMemcpyAsync(head, d_mask, kMaskHeaderBytes, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (!mask_parse(head, mask_len, &m.h))
    return -1;
  m.d_payload = static_cast<const uint8_t*>(d_mask) + kMaskHeaderBytes;
  return 0;
}

// A call whose kernels read nothing of the engine's (apply, expand: the caller's stream and buffers only) ends
// without a host wait, unless the profiler wants its events
inline int end_call(Engine& E, hipStream_t st)
{
  if (E.prof.on) {
    HIP_CHECK(hipStreamSynchronize(st));
    E.prof.collect();
  }
  return 0;
}

// A call whose kernels read or write the engine's buffers (maskWork, maskStage) waits for its stream before the engine
// goes back to the pool: the next call on another stream gets the same buffers.  `rtn` passes through
inline int drain_call(Engine& E, hipStream_t st, int rtn)
{
  if (hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    rtn = -1;
  }
  E.prof.collect();
  return rtn;
}

// The first half of making a mask of the n samples at d_src: the survey, under a smooth fill the pull, and the ONE host
// wait.  0 ok; 1 mask_cap too small (*res names the size); -1 otherwise.  Nothing of the caller's is written yet
inline int mask_survey(Engine& E, const void* d_src, int is_float, size_t n, int rule, double threshold, const void* d_mask,
                size_t mask_cap, MaskResult* res, hipStream_t st, MaskFill* fill = nullptr)
{
  const size_t ws = mask_workspace_bytes(n);
  if (ws == 0 || (uintptr_t)d_mask % 8 != 0 || E.maskWork.ensure(ws))
    return -1;
  if (fill && fill->kind == kMaskFillSmooth) {
    if (E.maskPyramid.ensure(fill->plan->bytes))
      return -1;
    fill->pyr = E.maskPyramid.p;
  }
  if (mask_scan_run(d_src, is_float, n, rule, threshold, E.maskWork.p, res, st, fill))
    return -1;
  // (lo and hi belong to the midrange rule: a caller's value does not look at them, the smooth rule has its own refusal)
  if (!res->finite && !(fill && fill->kind == kMaskFillValue))
    return -1;
  return res->mask_len > mask_cap ? 1 : 0;
}

// The fill of a call: false when the kind is unknown or the caller's value is not finite as the samples hold it.  A
// smooth fill needs the volume's dims (`plan` receives its levels); of one sample it is the value 0.0
inline bool fill_of(int kind, double value, int is_float, size_t dimx, size_t dimy, size_t dimz, MaskFillPlan* plan,
             MaskFill* fill)
{
  *fill = MaskFill{kind, 0.0, nullptr, nullptr};
  if (!mask_fill_kind_ok(kind))
    return false;
  if (kind == kMaskFillValue)
    return mask_fill_value_ok(value, is_float != 0, &fill->value);
  if (kind == kMaskFillSmooth) {
    if (!mask_fill_plan(dimx, dimy, dimz, plan))
      return false;
    if (plan->L == 0)
      *fill = MaskFill{kMaskFillValue, 0.0, nullptr, nullptr};
    else
      fill->plan = plan;
  }
  return true;
}

inline bool volume_count(size_t dimx, size_t dimy, size_t dimz, size_t* n)
{
  return dimx && dimy && dimz && view_mul(dimx, dimy, n) && view_mul(*n, dimz, n) && *n <= SIZE_MAX / 8;
}


}  // namespace sperrhip

#endif
