// abi_mask.hip -- the C ABI of missing values (include/sperr_hip.h; mask.h has the rules, mask.hip the kernels).
// A masked volume is an ordinary container of the in-filled volume and a mask stream: the compress call stages the
// in-filled volume in a buffer the engine owns and runs the dense encoder on it unchanged, the decode call runs the
// dense, box or portion decode through DecodeRequest and then stores `value` at the missing samples.
#include "mask_calls.h"
#include "quality.h"

using namespace sperrhip;


extern "C" {

size_t sperrhip_mask_max_size(size_t n)
{
  return mask_max_size(n);
}

int sperrhip_mask_make_dev(const void* d_src, int is_float, size_t n, int rule, double threshold, void* d_filled,
                           void* d_mask, size_t mask_cap, size_t* mask_len, size_t* nmissing, void* hip_stream)
{
  return sperrhip_mask_make_vol_dev(d_src, is_float, n, 1, 1, rule, threshold, SPERRHIP_FILL_MIDRANGE, 0.0, d_filled,
                                    d_mask, mask_cap, mask_len, nmissing, hip_stream);
}

int sperrhip_mask_make_vol_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, int rule,
                               double threshold, int fill, double fill_value, void* d_filled, void* d_mask,
                               size_t mask_cap, size_t* mask_len, size_t* nmissing, void* hip_stream)
{
  return guarded("sperrhip_mask_make_vol_dev", [&]() -> int {
    size_t n = 0;
    MaskFillPlan plan;
    MaskFill mf;
    if (!d_src || !d_mask || !mask_len || !nmissing || !volume_count(dimx, dimy, dimz, &n) ||
        !mask_rule_ok(rule, threshold) || !fill_of(fill, fill_value, is_float, dimx, dimy, dimz, &plan, &mf))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    MaskResult res{};
    // (without d_filled a smooth fill has nothing to fill: its pull, and its refusal, are left out)
    if (!d_filled && mf.kind == kMaskFillSmooth)
      mf = MaskFill{kMaskFillValue, 0.0, nullptr, nullptr};
    int rtn = mask_survey(*L.e, d_src, is_float, n, rule, threshold, d_mask, mask_cap, &res, st, &mf);
    if (rtn >= 0)
      *mask_len = (size_t)res.mask_len;
    if (rtn == 0) {
      *nmissing = (size_t)res.nmissing;
      // (nothing missing and the fill in place: the samples are what they were)
      void* filled = res.nmissing == 0 && d_filled == d_src ? nullptr : d_filled;
      rtn = mask_pack_fill_run(d_src, is_float, n, L.e->maskWork.p, res, d_mask, filled, st, &mf) ? -1 : 0;
    }
    // (k_mask_pack and the fill kernels read the engine's word array, offsets, fill value and pyramid)
    return drain_call(*L.e, st, rtn);
  });
}

int sperrhip_mask_parse_dev(const void* d_mask, size_t mask_len, size_t* n, size_t* nmissing, int* kind)
{
  return sperrhip_mask_parse_stream_dev(d_mask, mask_len, n, nmissing, kind, nullptr);
}

// (read behind what `hip_stream` still has to do; see sperrhip_parse_header_stream_dev)
int sperrhip_mask_parse_stream_dev(const void* d_mask, size_t mask_len, size_t* n, size_t* nmissing, int* kind,
                                   void* hip_stream)
{
  return guarded("sperrhip_mask_parse_stream_dev", [&]() -> int {
    MaskStream m;
    if (read_mask_stream(d_mask, mask_len, m, static_cast<hipStream_t>(hip_stream)))
      return -1;
    if (n)
      *n = (size_t)m.h.n;
    if (nmissing)
      *nmissing = (size_t)m.h.nmissing;
    if (kind)
      *kind = m.h.kind;
    return 0;
  });
}

int sperrhip_mask_apply_dev(void* d_vol, int is_float, const size_t vol_dims[3], const size_t box_lo[3],
                            const size_t box_dims[3], const void* d_mask, size_t mask_len, double value,
                            void* hip_stream)
{
  return guarded("sperrhip_mask_apply_dev", [&]() -> int {
    size_t n = 0;
    if (!d_vol || !vol_dims || (box_lo == nullptr) != (box_dims == nullptr) ||
        !volume_count(vol_dims[0], vol_dims[1], vol_dims[2], &n))
      return -1;
    const size_t zero[3] = {0, 0, 0};
    const size_t* lo = box_lo ? box_lo : zero;
    const size_t* dims = box_dims ? box_dims : vol_dims;
    for (int a = 0; a < 3; a++)
      if (dims[a] == 0 || lo[a] >= vol_dims[a] || dims[a] > vol_dims[a] - lo[a])
        return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    MaskStream m;
    if (read_mask_stream(d_mask, mask_len, m, st) || m.h.n != n)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    if (mask_apply_run(d_vol, is_float, vol_dims, lo, dims, m, value, st))
      return -1;
    return end_call(*L.e, st);
  });
}

int sperrhip_mask_expand_dev(const void* d_mask, size_t mask_len, unsigned char* d_out, size_t n, void* hip_stream)
{
  return guarded("sperrhip_mask_expand_dev", [&]() -> int {
    if (!d_out)
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    MaskStream m;
    if (read_mask_stream(d_mask, mask_len, m, st) || m.h.n != n)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    if (mask_expand_run(m, d_out, st))
      return -1;
    return end_call(*L.e, st);
  });
}

int sperrhip_compress_masked_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                 size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality, int rule,
                                 double threshold, void* d_dst, size_t dst_cap, size_t* dst_len, void* d_mask,
                                 size_t mask_cap, size_t* mask_len, size_t* nmissing, void* hip_stream)
{
  return sperrhip_compress_masked_fill_dev(d_src, is_float, dimx, dimy, dimz, chunk_x, chunk_y, chunk_z, mode, quality,
                                           rule, threshold, SPERRHIP_FILL_MIDRANGE, 0.0, d_dst, dst_cap, dst_len, d_mask,
                                           mask_cap, mask_len, nmissing, hip_stream);
}

int sperrhip_compress_masked_fill_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                      size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality, int rule,
                                      double threshold, int fill, double fill_value, void* d_dst, size_t dst_cap,
                                      size_t* dst_len, void* d_mask, size_t mask_cap, size_t* mask_len,
                                      size_t* nmissing, void* hip_stream)
{
  return guarded("sperrhip_compress_masked_fill_dev", [&]() -> int {
    if (quality <= 0.0 || mode < 1 || mode > 3)   // (before any -1, as every compress entry point)
      return 2;
    size_t n = 0;
    MaskFillPlan plan;
    MaskFill mf;
    if (!d_src || !d_dst || !dst_len || !d_mask || !mask_len || !nmissing || !volume_count(dimx, dimy, dimz, &n) ||
        !mask_rule_ok(rule, threshold) || !fill_of(fill, fill_value, is_float, dimx, dimy, dimz, &plan, &mf))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const size_t esz = is_float ? sizeof(float) : sizeof(double);
    MaskResult res{};
    const int made = mask_survey(E, d_src, is_float, n, rule, threshold, d_mask, mask_cap, &res, st, &mf);
    if (made >= 0)
      *mask_len = (size_t)res.mask_len;
    if (made != 0)
      return drain_call(E, st, made);
    *nmissing = (size_t)res.nmissing;
    // (with nothing missing the source is the in-filled volume: no staged copy is made of it)
    if (res.nmissing && E.maskStage.ensure(n * esz))
      return drain_call(E, st, -1);
    void* stage = res.nmissing ? E.maskStage.p : nullptr;
    if (mask_pack_fill_run(d_src, is_float, n, E.maskWork.p, res, d_mask, stage, st, &mf))
      return drain_call(E, st, -1);
    // (compress_to waits for the stream at its end, behind the pack and the fill)
    const void* filled = stage ? stage : d_src;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    return compress_to(E, filled, is_float, vol, ch, mode, quality, static_cast<uint8_t*>(d_dst), dst_cap, dst_len,
                       st);
  });
}

int sperrhip_decompress_masked_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                   const size_t box_lo[3], const size_t box_dims[3], const void* d_mask,
                                   size_t mask_len, double value, void* d_dst, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_masked_dev", [&]() -> int {
    if (!d_src || !d_dst || (box_lo == nullptr) != (box_dims == nullptr))
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    MaskStream m;
    if (read_mask_stream(d_mask, mask_len, m, st))
      return -1;
    // (the lease, the stream, the container's header: what every device decode begins with)
    Lease L(static_cast<hipStream_t>(hip_stream));
    ContainerInfo ci;
    if (!L.e || read_container_info(static_cast<const uint8_t*>(d_src), src_len, ci, st) != 0)
      return -1;
    if (m.h.n != ci.nvals)
      return -1;
    keep_portion(ci, pct);
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    const size_t vol[3] = {ci.vol[0], ci.vol[1], ci.vol[2]}, zero[3] = {0, 0, 0};
    int rtn;
    if (box_lo) {
      Window w;
      if (box_select(ci, box_lo, box_dims, w))
        return -1;
      rtn = decode_window(*L.e, d_src, output_float, d_dst, dst_cap_bytes, ci, st, w);
    }
    else {
      if (dst_cap_bytes / esz < ci.nvals)
        return -1;
      rtn = decode_to(*L.e, d_src, output_float, d_dst, dst_cap_bytes, ci, st, DecodeRequest{});
    }
    if (rtn != 0)
      return rtn;
    if (mask_apply_run(d_dst, output_float, vol, box_lo ? box_lo : zero, box_lo ? box_dims : vol, m, value, st))
      return -1;
    return end_call(*L.e, st);
  });
}

int sperrhip_quality_masked_dev(const void* d_orig, const void* d_recon, int is_float, size_t n, const void* d_mask,
                                size_t mask_len, double* out, void* hip_stream)
{
  return guarded("sperrhip_quality_masked_dev", [&]() -> int {
    if (!d_orig || !d_recon || !out || n == 0 || n > SIZE_MAX / 8)
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    MaskStream m;
    if (read_mask_stream(d_mask, mask_len, m, st) || m.h.n != n || m.h.nmissing >= n)
      return -1;
    const size_t nvalid = n - (size_t)m.h.nmissing, esz = is_float ? sizeof(float) : sizeof(double);
    const size_t need = quality_workspace_bytes(1, nvalid, is_float), ws = mask_workspace_bytes(n);
    if (need == 0 || ws == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    // (the stages hold n samples: a payload that disagrees with its header still writes inside them)
    if (E.arena.ensure(need) || E.maskWork.ensure(ws) || E.maskStage.ensure(n * esz) || E.maskStage2.ensure(n * esz))
      return -1;
    const void* srcs[2] = {d_orig, d_recon};
    void* dsts[2] = {E.maskStage.p, E.maskStage2.p};
    if (mask_compact_run(srcs, dsts, 2, is_float, m, E.maskWork.p, st))
      return drain_call(E, st, -1);
    // (quality_run waits for the stream at its end, behind the compaction)
    const int rtn = quality_run(E.maskStage.p, E.maskStage2.p, is_float, 1, nvalid, E.arena.p, out, hip_stream);
    E.prof.collect();
    return rtn;
  });
}

}  // extern "C"
