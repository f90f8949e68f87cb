// abi_rel.hip -- the C ABI of point-wise relative error (include/sperr_hip.h; rel.h has the rule, rel.hip the kernels).
// The composite calls chain what is there: compress is k_rel_forward into a buffer the engine owns and then the body of
// the masked compress call on y (doubles, point-wise error mode at t, NaN the missing value); decode is the body of
// the masked decode call as doubles into that buffer -- without its last step: nothing reads an in-filled sample as a
// value -- and then k_rel_inverse.  Host waits: compress has the masked call's (the sign record arrives with the
// survey's); decode has one more than the masked call, at its end, because k_rel_inverse reads the engine's buffer.
// The map kind (rel.h: linear or log) is an argument of the *_kind calls going in -- the calls without it mean the
// linear kind -- and the side stream's magic coming back.
#include "mask_calls.h"
#include "rel.h"

using namespace sperrhip;

namespace {

// a side stream on the device, its three headers checked
struct RelSide {
  RelHeader h;
  MaskStream zero, sign;
  uint8_t signHead[kMaskHeaderBytes];
};

// The first half: the header and the zero stream's header with ONE host wait, and the copy of the sign stream's header
// queued behind it: rel_side_end after the stream's next host wait.  d_side must be 8-byte aligned
int rel_side_begin(const void* d_side, size_t side_len, RelSide& s, hipStream_t st)
{
  constexpr size_t kHead = kRelHeaderBytes + kMaskHeaderBytes;
  if (!d_side || side_len < kHead + kMaskHeaderBytes || (uintptr_t)d_side % 8 != 0)
    return -1;
  const uint8_t* side = static_cast<const uint8_t*>(d_side);
  uint8_t head[kHead];
  HIP_CHECK(hipMemcpyAsync(head, side, kHead, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (!rel_parse(head, side_len, &s.h) || !mask_parse(head + kRelHeaderBytes, (size_t)s.h.zero_len, &s.zero.h) ||
      s.zero.h.n != s.h.n)
    return -1;
  s.zero.d_payload = side + kRelHeaderBytes + kMaskHeaderBytes;
  s.sign.d_payload = side + rel_sign_offset(s.h) + kMaskHeaderBytes;
  HIP_CHECK(hipMemcpyAsync(s.signHead, side + rel_sign_offset(s.h), kMaskHeaderBytes, hipMemcpyDeviceToHost, st));
  return 0;
}
int rel_side_end(RelSide& s)
{
  return mask_parse(s.signHead, (size_t)s.h.sign_len, &s.sign.h) && s.sign.h.n == s.h.n ? 0 : -1;
}
// both halves, two host waits
int read_rel_side(const void* d_side, size_t side_len, RelSide& s, hipStream_t st)
{
  if (rel_side_begin(d_side, side_len, s, st))
    return -1;
  HIP_CHECK(hipStreamSynchronize(st));
  return rel_side_end(s);
}

// a box of a volume, or with both NULL the volume: false when it leaves the volume
bool box_of(const size_t vol[3], const size_t box_lo[3], const size_t box_dims[3], size_t lo[3], size_t dims[3])
{
  for (int a = 0; a < 3; a++) {
    lo[a] = box_lo ? box_lo[a] : 0;
    dims[a] = box_lo ? box_dims[a] : vol[a];
    if (dims[a] == 0 || lo[a] >= vol[a] || dims[a] > vol[a] - lo[a])
      return false;
  }
  return true;
}

// What a forward call knows after the survey's host wait: 0 ok, `h` the side stream's header; 1 side_cap too small;
// -1 a sample that is not finite.  *side_len is set unless -1
int side_header(const RelForward& fwd, const MaskResult& zero, int is_float, double eps, size_t n, int kind,
                size_t side_cap, size_t* side_len, RelHeader* h)
{
  if (fwd.nonfinite)
    return -1;
  *h = RelHeader{is_float != 0, eps, n, zero.mask_len, fwd.sign.mask_len, kind};
  *side_len = (size_t)rel_stream_bytes(*h);
  return *side_len > side_cap ? 1 : 0;
}

}  // namespace

extern "C" {

int sperrhip_rel_tolerance_kind(double eps, int is_float, int kind, double* t)
{
  return t && rel_tolerance(eps, is_float != 0, t, kind) ? 0 : -1;
}

int sperrhip_rel_tolerance(double eps, int is_float, double* t)
{
  return sperrhip_rel_tolerance_kind(eps, is_float, kRelLinear, t);
}

size_t sperrhip_rel_max_size(size_t n)
{
  return rel_max_size(n);
}

int sperrhip_rel_forward_kind_dev(const void* d_src, int is_float, size_t n, int kind, void* d_y, void* d_side,
                                  size_t side_cap, size_t* side_len, size_t* nzero, size_t* nneg, void* hip_stream)
{
  return guarded("sperrhip_rel_forward_kind_dev", [&]() -> int {
    const size_t ws = rel_workspace_bytes(n);
    if (!d_src || !d_y || !d_side || !side_len || !nzero || !nneg || n == 0 || n > SIZE_MAX / 8 || ws == 0 ||
        !rel_kind_ok(kind) || (uintptr_t)d_side % 8 != 0 || (uintptr_t)d_y % 8 != 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // (y goes to the engine's buffer first: a sample that is not finite is known after the wait only, and nothing of
    //  the caller's may be written before)
    if (E.relStage.ensure(n * sizeof(double)) || E.relWork.ensure(ws))
      return -1;
    RelForward fwd{};
    MaskResult zero{};
    if (rel_forward_run(d_src, is_float, n, static_cast<double*>(E.relStage.p), E.relWork.p, &fwd, st, kind))
      return drain_call(E, st, -1);
    if (mask_survey(E, E.relStage.p, 0, n, kMaskRuleNan, 0.0, nullptr, SIZE_MAX, &zero, st) != 0)
      return drain_call(E, st, -1);
    RelHeader h;
    int rtn = side_header(fwd, zero, is_float, 0.0, n, kind, side_cap, side_len, &h);
    if (rtn == 0) {
      *nzero = (size_t)zero.nmissing;
      *nneg = (size_t)fwd.sign.nmissing;
      uint8_t* side = static_cast<uint8_t*>(d_side);
      if (mask_pack_fill_run(E.relStage.p, 0, n, E.maskWork.p, zero, side + kRelHeaderBytes, nullptr, st) ||
          rel_side_run(h, E.relWork.p, fwd.sign, d_side, st) ||
          hipMemcpyAsync(d_y, E.relStage.p, n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
        rtn = -1;
    }
    return drain_call(E, st, rtn);
  });
}

int sperrhip_rel_forward_dev(const void* d_src, int is_float, size_t n, void* d_y, void* d_side, size_t side_cap,
                             size_t* side_len, size_t* nzero, size_t* nneg, void* hip_stream)
{
  return sperrhip_rel_forward_kind_dev(d_src, is_float, n, kRelLinear, d_y, d_side, side_cap, side_len, nzero, nneg,
                                       hip_stream);
}

int sperrhip_rel_inverse_dev(const void* d_y, const size_t vol_dims[3], const size_t box_lo[3],
                             const size_t box_dims[3], const void* d_side, size_t side_len, int output_float,
                             void* d_dst, void* hip_stream)
{
  return guarded("sperrhip_rel_inverse_dev", [&]() -> int {
    size_t n = 0, lo[3], dims[3];
    if (!d_y || !d_dst || !vol_dims || (box_lo == nullptr) != (box_dims == nullptr) ||
        !volume_count(vol_dims[0], vol_dims[1], vol_dims[2], &n) || !box_of(vol_dims, box_lo, box_dims, lo, dims) ||
        (uintptr_t)d_y % 8 != 0 || (d_dst == d_y && output_float))
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RelSide s;
    if (read_rel_side(d_side, side_len, s, st) || s.h.n != n)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    if (rel_inverse_run(static_cast<const double*>(d_y), vol_dims, lo, dims, s.zero, s.sign, s.h.is_float, output_float,
                        d_dst, st, s.h.kind))
      return -1;
    return end_call(*L.e, st);
  });
}

int sperrhip_compress_rel_kind_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                   size_t chunk_x, size_t chunk_y, size_t chunk_z, double eps, int kind, int fill,
                                   double fill_value, void* d_dst, size_t dst_cap, size_t* dst_len, void* d_side,
                                   size_t side_cap, size_t* side_len, void* hip_stream)
{
  return guarded("sperrhip_compress_rel_kind_dev", [&]() -> int {
    size_t n = 0;
    double t = 0.0;
    MaskFillPlan plan;
    MaskFill mf;
    // (the fill is y's: a value in the domain of doubles)
    if (!d_src || !d_dst || !dst_len || !d_side || !side_len || (uintptr_t)d_side % 8 != 0 ||
        !volume_count(dimx, dimy, dimz, &n) || !rel_tolerance(eps, is_float != 0, &t, kind) ||
        !fill_of(fill, fill_value, 0, dimx, dimy, dimz, &plan, &mf))
      return -1;
    const size_t ws = rel_workspace_bytes(n);
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e || ws == 0)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (E.relStage.ensure(n * sizeof(double)) || E.relWork.ensure(ws))
      return -1;
    double* y = static_cast<double*>(E.relStage.p);
    RelForward fwd{};
    if (rel_forward_run(d_src, is_float, n, y, E.relWork.p, &fwd, st, kind))
      return drain_call(E, st, -1);
    // ---- from here the body of sperrhip_compress_masked_fill_dev on y; its one wait brings the sign record too
    MaskResult zero{};
    if (mask_survey(E, y, 0, n, kMaskRuleNan, 0.0, nullptr, SIZE_MAX, &zero, st, &mf) != 0)
      return drain_call(E, st, -1);
    RelHeader h;
    const int made = side_header(fwd, zero, is_float, eps, n, kind, side_cap, side_len, &h);
    if (made != 0)
      return drain_call(E, st, made);
    // (with no zero y is the in-filled volume: no staged copy is made of it)
    if (zero.nmissing && E.maskStage.ensure(n * sizeof(double)))
      return drain_call(E, st, -1);
    void* stage = zero.nmissing ? E.maskStage.p : nullptr;
    if (mask_pack_fill_run(y, 0, n, E.maskWork.p, zero, static_cast<uint8_t*>(d_side) + kRelHeaderBytes, stage, st, &mf) ||
        rel_side_run(h, E.relWork.p, fwd.sign, d_side, st))
      return drain_call(E, st, -1);
    // (compress_to waits for the stream at its end, behind the packs and the fill)
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    return compress_to(E, stage ? stage : y, 0, vol, ch, 3, t, static_cast<uint8_t*>(d_dst), dst_cap, dst_len, st);
  });
}

int sperrhip_compress_rel_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                              size_t chunk_y, size_t chunk_z, double eps, int fill, double fill_value, void* d_dst,
                              size_t dst_cap, size_t* dst_len, void* d_side, size_t side_cap, size_t* side_len,
                              void* hip_stream)
{
  return sperrhip_compress_rel_kind_dev(d_src, is_float, dimx, dimy, dimz, chunk_x, chunk_y, chunk_z, eps, kRelLinear,
                                        fill, fill_value, d_dst, dst_cap, dst_len, d_side, side_cap, side_len,
                                        hip_stream);
}

int sperrhip_decompress_rel_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                const size_t box_lo[3], const size_t box_dims[3], const void* d_side, size_t side_len,
                                void* d_dst, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_rel_dev", [&]() -> int {
    if (!d_src || !d_dst || (box_lo == nullptr) != (box_dims == nullptr))
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RelSide s;
    if (rel_side_begin(d_side, side_len, s, st))
      return -1;
    // (the lease, the stream, the container's header: what every device decode begins with; its wait brings the sign
    //  stream's header)
    Lease L(static_cast<hipStream_t>(hip_stream));
    ContainerInfo ci;
    if (!L.e || read_container_info(static_cast<const uint8_t*>(d_src), src_len, ci, st) != 0) {
      (void)hipStreamSynchronize(st);   // (the queued copy writes into `s`)
      return -1;
    }
    Engine& E = *L.e;
    if (rel_side_end(s) || s.h.n != ci.nvals || ci.is_float)
      return -1;
    keep_portion(ci, pct);
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    const size_t vol[3] = {ci.vol[0], ci.vol[1], ci.vol[2]};
    size_t lo[3], dims[3];
    if (!box_of(vol, box_lo, box_dims, lo, dims))
      return -1;
    const size_t nout = dims[0] * dims[1] * dims[2];   // (<= ci.nvals)
    if (dst_cap_bytes / esz < nout || E.relStage.ensure(nout * sizeof(double)))
      return -1;
    int rtn;
    if (box_lo) {
      Window w;
      if (box_select(ci, box_lo, box_dims, w))
        return -1;
      rtn = decode_window(E, d_src, 0, E.relStage.p, nout * sizeof(double), ci, st, w);
    }
    else
      rtn = decode_to(E, d_src, 0, E.relStage.p, nout * sizeof(double), ci, st, DecodeRequest{});
    if (rtn != 0)
      return rtn;
    if (rel_inverse_run(static_cast<const double*>(E.relStage.p), vol, lo, dims, s.zero, s.sign, s.h.is_float, output_float,
                        d_dst, st, s.h.kind))
      rtn = -1;
    // (k_rel_inverse reads the engine's buffer)
    return drain_call(E, st, rtn);
  });
}

int sperrhip_rel_parse_stream_kind_dev(const void* d_side, size_t side_len, int* is_float, double* eps, size_t* n,
                                       size_t* nzero, size_t* nneg, int* kind, void* hip_stream)
{
  return guarded("sperrhip_rel_parse_stream_kind_dev", [&]() -> int {
    RelSide s;
    if (read_rel_side(d_side, side_len, s, static_cast<hipStream_t>(hip_stream)))
      return -1;
    if (is_float)
      *is_float = s.h.is_float;
    if (eps)
      *eps = s.h.eps;
    if (n)
      *n = (size_t)s.h.n;
    if (nzero)
      *nzero = (size_t)s.zero.h.nmissing;
    if (nneg)
      *nneg = (size_t)s.sign.h.nmissing;
    if (kind)
      *kind = s.h.kind;
    return 0;
  });
}

int sperrhip_rel_parse_stream_dev(const void* d_side, size_t side_len, int* is_float, double* eps, size_t* n,
                                  size_t* nzero, size_t* nneg, void* hip_stream)
{
  return sperrhip_rel_parse_stream_kind_dev(d_side, side_len, is_float, eps, n, nzero, nneg, nullptr, hip_stream);
}

int sperrhip_rel_check_dev(const void* d_orig, const void* d_recon, int is_float, size_t n, double eps, double* out,
                           void* hip_stream)
{
  return guarded("sperrhip_rel_check_dev", [&]() -> int {
    const size_t ws = rel_workspace_bytes(n);
    if (!d_orig || !d_recon || !out || n == 0 || n > SIZE_MAX / 8 || ws == 0 || !(eps >= 0.0) || !(eps <= DBL_MAX))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e || L.e->relWork.ensure(ws))
      return -1;
    uint64_t w[4] = {0, 0, 0, 0};
    const int rtn = rel_check_run(d_orig, d_recon, is_float, n, eps, L.e->relWork.p, w, hip_stream);
    if (rtn != 0)
      return drain_call(*L.e, static_cast<hipStream_t>(hip_stream), -1);
    L.e->prof.collect();
    out[0] = rel_from_bits(w[0]);
    out[1] = (double)w[1];
    out[2] = (double)w[2];
    out[3] = (double)w[3];
    return 0;
  });
}

}  // extern "C"
