// abi_series.hip -- the C ABI of time series (include/sperr_hip.h; series.h has the rule, series.hip the kernels).
// The composite calls chain what is there.  Compress: the series' extremes from the range kernel step by step,
// k_series_fwd into a buffer the engine owns, and then the batch code on every run of bands of one tolerance (the
// bands of groups of one size are neighbours) or, in PSNR mode, the PSNR-of-the-volume flow band by band.  Decode: the
// needed bands as doubles into that buffer with the boxes call's body -- it takes containers anywhere, a box and a pct
// --, then k_series_inv.  The staging buffer is capped (SPERR_HIP_SERIES_MAX_MB): a longer series runs in windows of
// whole groups, and since a band's container depends on that band alone, the containers do not depend on the cap.
#include "decode_request.h"
#include "mask_calls.h"
#include "series_run.h"

using namespace sperrhip;

namespace {

// the staging cap in bytes (the header states the default)
size_t series_cap_bytes()
{
  const char* s = getenv("SPERR_HIP_SERIES_MAX_MB");
  const long long mb = s ? atoll(s) : 2048;
  return (size_t)(mb > 0 ? mb : 1) << 20;
}

bool plan_ok(size_t nsteps, unsigned levels)
{
  return nsteps != 0 && nsteps <= 0xffffffffull && levels <= (unsigned)kSeriesMaxLevels;
}

// the tables of a call in Engine::seriesTab: `count` pointers each, uploaded on `st`.  The host arrays must outlive the
// copies: every call below ends in a wait of the host
int upload_tables(Engine& E, const std::vector<const void*>& a, const std::vector<void*>& b, const void* const** d_a,
                  void* const** d_b, hipStream_t st)
{
  const size_t na = a.size() * sizeof(void*), nb = b.size() * sizeof(void*);
  if (E.seriesTab.ensure(na + nb))
    return -1;
  char* base = static_cast<char*>(E.seriesTab.p);
  HIP_CHECK(hipMemcpyAsync(base, a.data(), na, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(base + na, b.data(), nb, hipMemcpyHostToDevice, st));
  *d_a = reinterpret_cast<const void* const*>(base);
  *d_b = reinterpret_cast<void* const*>(base + na);
  return 0;
}

// the groups of the plan that meet the steps [t0, t0 + nt): [*g0, *g1)
void groups_meeting(size_t nsteps, int levels, size_t t0, size_t nt, size_t* g0, size_t* g1)
{
  const size_t ng = series_group_count(nsteps, levels);
  *g0 = ng;
  *g1 = 0;
  for (size_t i = 0; i < ng; i++) {
    size_t start;
    int l;
    series_group(nsteps, levels, i, &start, &l);
    if (start < t0 + nt && t0 < start + ((size_t)1 << l)) {
      *g0 = std::min(*g0, i);
      *g1 = i + 1;
    }
  }
}

}  // namespace

extern "C" {

int sperrhip_series_plan(size_t nsteps, unsigned levels, size_t* ngroups, size_t* starts, unsigned* group_levels,
                         size_t cap)
{
  if (!ngroups || !plan_ok(nsteps, levels))
    return -1;
  *ngroups = series_group_count(nsteps, (int)levels);
  if (!starts && !group_levels)
    return 0;
  if (cap < *ngroups)
    return 1;
  for (size_t i = 0; i < *ngroups; i++) {
    size_t start;
    int l;
    series_group(nsteps, (int)levels, i, &start, &l);
    if (starts)
      starts[i] = start;
    if (group_levels)
      group_levels[i] = (unsigned)l;
  }
  return 0;
}

int sperrhip_series_needs(size_t nsteps, unsigned levels, size_t t0, size_t nt, unsigned char* need, size_t* count)
{
  if (!need || !plan_ok(nsteps, levels) || !series_needs(nsteps, (int)levels, t0, nt, need))
    return -1;
  if (count) {
    *count = 0;
    for (size_t b = 0; b < nsteps; b++)
      *count += need[b];
  }
  return 0;
}

int sperrhip_series_tolerance(double tol, double maxabs, unsigned levels, double* rho, double* tau)
{
  if (!rho || !tau || levels > (unsigned)kSeriesMaxLevels)
    return -1;
  return series_tolerance(tol, maxabs, (int)levels, rho, tau) ? 0 : -1;
}

int sperrhip_series_parse(const void* info, size_t* nsteps, unsigned* levels, size_t dims[3], int* is_float, int* kind,
                          double* quality, double* range, double* maxabs, double* rho)
{
  SeriesInfo h;
  if (!info || !series_parse_info(static_cast<const uint8_t*>(info), &h))
    return -1;
  if (nsteps)
    *nsteps = (size_t)h.n;
  if (levels)
    *levels = (unsigned)h.levels;
  for (int a = 0; dims && a < 3; a++)
    dims[a] = (size_t)h.dims[a];
  if (is_float)
    *is_float = h.is_float;
  if (kind)
    *kind = h.kind;
  if (quality)
    *quality = h.quality;
  if (range)
    *range = h.range;
  if (maxabs)
    *maxabs = h.M;
  if (rho)
    *rho = h.rho;
  return 0;
}

int sperrhip_series_forward_dev(const void* const* d_steps, int is_float, size_t nsteps, unsigned levels, size_t n,
                                void* d_bands, void* hip_stream)
{
  return guarded("sperrhip_series_forward_dev", [&]() -> int {
    if (!d_steps || !d_bands || !plan_ok(nsteps, levels) || n == 0 || n > SIZE_MAX / 8 / nsteps ||
        (uintptr_t)d_bands % 8 != 0)
      return -1;
    const size_t esz = is_float ? sizeof(float) : sizeof(double);
    const char* lo = static_cast<const char*>(d_bands);
    const char* hi = lo + nsteps * n * sizeof(double);
    for (size_t t = 0; t < nsteps; t++) {
      const char* s = static_cast<const char*>(d_steps[t]);
      if (!s || (uintptr_t)s % esz != 0 || (s < hi && s + n * esz > lo))   // (a step inside the bands)
        return -1;
    }
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::vector<const void*> steps(d_steps, d_steps + nsteps);
    std::vector<void*> bands(nsteps);
    for (size_t b = 0; b < nsteps; b++)
      bands[b] = static_cast<double*>(d_bands) + b * n;
    const void* const* dS;
    void* const* dB;
    if (upload_tables(E, steps, bands, &dS, &dB, st))
      return drain_call(E, st, -1);
    const int rtn = series_forward_run(dS, is_float, reinterpret_cast<double* const*>(dB), nsteps, (int)levels, 0,
                                       series_group_count(nsteps, (int)levels), n, st);
    return drain_call(E, st, rtn);
  });
}

int sperrhip_series_inverse_dev(const void* d_bands, size_t nsteps, unsigned levels, size_t n, size_t t0, size_t nt,
                                int output_float, void* const* d_outs, void* hip_stream)
{
  return guarded("sperrhip_series_inverse_dev", [&]() -> int {
    if (!d_bands || !d_outs || !plan_ok(nsteps, levels) || n == 0 || n > SIZE_MAX / 8 / nsteps ||
        (uintptr_t)d_bands % 8 != 0)
      return -1;
    std::vector<uint8_t> need(nsteps);
    if (!series_needs(nsteps, (int)levels, t0, nt, need.data()))
      return -1;
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    const char* lo = static_cast<const char*>(d_bands);
    const char* hi = lo + nsteps * n * sizeof(double);
    for (size_t t = 0; t < nt; t++) {
      const char* o = static_cast<const char*>(d_outs[t]);
      if (!o || (uintptr_t)o % esz != 0 || (o < hi && o + n * esz > lo))   // (an output inside the bands)
        return -1;
    }
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::vector<const void*> bands(nsteps, nullptr);
    std::vector<void*> outs(nsteps, nullptr);
    for (size_t b = 0; b < nsteps; b++)
      if (need[b])
        bands[b] = static_cast<const double*>(d_bands) + b * n;
    for (size_t t = 0; t < nt; t++)
      outs[t0 + t] = d_outs[t];
    const void* const* dB;
    void* const* dO;
    if (upload_tables(E, bands, outs, &dB, &dO, st))
      return drain_call(E, st, -1);
    size_t g0, g1;
    groups_meeting(nsteps, (int)levels, t0, nt, &g0, &g1);
    const int rtn = series_inverse_run(reinterpret_cast<const double* const*>(dB), dO, output_float, nsteps, (int)levels,
                                       g0, g1, n, st);
    return drain_call(E, st, rtn);
  });
}

int sperrhip_compress_series_dev(const void* const* d_steps, int is_float, size_t nsteps, size_t dimx, size_t dimy,
                                 size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z, unsigned levels, int kind,
                                 double quality, double range, void* d_dst, size_t dst_cap, size_t* offsets, void* info,
                                 void* hip_stream)
{
  return guarded("sperrhip_compress_series_dev", [&]() -> int {
    size_t n = 0;
    if (!d_steps || !d_dst || !offsets || !info || !plan_ok(nsteps, levels) || !volume_count(dimx, dimy, dimz, &n) ||
        dimx > 0xffffffffull || dimy > 0xffffffffull || dimz > 0xffffffffull || nsteps > 0xffffffffull / dimz ||
        (kind != kSeriesKindTol && kind != kSeriesKindPsnr) || !std::isfinite(quality) || !(range >= 0.0) ||
        !std::isfinite(range) || (kind == kSeriesKindTol && !(quality > 0.0)))
      return -1;
    const size_t esz = is_float ? sizeof(float) : sizeof(double);
    for (size_t t = 0; t < nsteps; t++)
      if (!d_steps[t] || (uintptr_t)d_steps[t] % esz != 0)
        return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    const int Lv = (int)levels;

    // ---- the series' extremes: a NaN is refused by the range kernel, an infinity by the range
    double smin = INFINITY, smax = -INFINITY;
    for (size_t t = 0; t < nsteps; t++) {
      double lo, hi;
      if (range_to(E, d_steps[t], is_float, vol, nullptr, &lo, &hi, st))
        return -1;
      smin = std::min(smin, lo);
      smax = std::max(smax, hi);
    }
    const double own = smax - smin;
    if (!std::isfinite(own) || !std::isfinite(smin) || !std::isfinite(smax)) {
      fprintf(stderr, "[sperr_hip] the series' range [%g, %g] is not finite\n", smin, smax);
      return -1;
    }
    SeriesInfo h{Lv, is_float != 0, kind, nsteps, {dimx, dimy, dimz}, quality, range > 0.0 ? range : own,
                 std::max(fabs(smin), fabs(smax)), 0.0};
    double tau[kSeriesMaxLevels + 1] = {};
    if (kind == kSeriesKindTol && !series_tolerance(quality, h.M, Lv, &h.rho, tau))
      return -1;

    // ---- windows of whole groups under the cap; one group alone may exceed it
    const size_t ng = series_group_count(nsteps, Lv), bandBytes = n * sizeof(double);
    const size_t capBands = std::max<size_t>(1, series_cap_bytes() / bandBytes);
    std::vector<const void*> steps(d_steps, d_steps + nsteps);
    std::vector<void*> bands(nsteps, nullptr);
    uint8_t* dst = static_cast<uint8_t*>(d_dst);
    size_t written = 0;
    std::vector<size_t> offs(nsteps + 1, 0), local;
    for (size_t gA = 0; gA < ng;) {
      size_t first, last, gB = gA;
      int l;
      series_group(nsteps, Lv, gA, &first, &l);
      last = first;
      while (gB < ng) {
        size_t s;
        series_group(nsteps, Lv, gB, &s, &l);
        if (gB > gA && s + ((size_t)1 << l) - first > capBands)
          break;
        last = s + ((size_t)1 << l);
        gB++;
      }
      const size_t nb = last - first;
      g_dbg_counter[4]++;
      if (nb > SIZE_MAX / bandBytes || E.seriesStage.ensure(nb * bandBytes))
        return drain_call(E, st, -1);
      double* stage = static_cast<double*>(E.seriesStage.p);
      std::fill(bands.begin(), bands.end(), nullptr);
      for (size_t b = first; b < last; b++)
        bands[b] = stage + (b - first) * n;
      const void* const* dS;
      void* const* dB;
      if (upload_tables(E, steps, bands, &dS, &dB, st) ||
          series_forward_run(dS, is_float, reinterpret_cast<double* const*>(dB), nsteps, Lv, gA, gB, n, st))
        return drain_call(E, st, -1);
      // ---- the coder: runs of bands of one group size share a tolerance
      for (size_t g = gA; g < gB;) {
        size_t s0, s1;
        int l0, l1;
        series_group(nsteps, Lv, g, &s0, &l0);
        size_t gE = g + 1, end = s0 + ((size_t)1 << l0);
        for (; gE < gB; gE++) {
          series_group(nsteps, Lv, gE, &s1, &l1);
          if (l1 != l0)
            break;
          end = s1 + ((size_t)1 << l1);
        }
        int rtn = 0;
        if (kind == kSeriesKindTol) {
          local.assign(end - s0 + 1, 0);
          rtn = compress_batch_to(E, stage + (s0 - first) * n, 0, end - s0, vol, ch, 3, tau[l0], dst + written,
                                  dst_cap - written, local.data(), st);
          for (size_t b = s0; rtn == 0 && b < end; b++)
            offs[b + 1] = written + local[b - s0 + 1];
          if (rtn == 0)
            written = offs[end];
        }
        else {
          // (a constant series has range 0: every band is then constant, and takes its own range of 0)
          for (size_t b = s0; rtn == 0 && b < end; b++) {
            size_t len = 0;
            rtn = compress_psnr_to(E, stage + (b - first) * n, 0, vol, ch, quality, h.range, dst + written,
                                   dst_cap - written, &len, st, nullptr);
            written += rtn == 0 ? len : 0;
            offs[b + 1] = written;
          }
        }
        if (rtn != 0)
          return drain_call(E, st, rtn);
        g = gE;
      }
      gA = gB;
    }
    memcpy(offsets, offs.data(), (nsteps + 1) * sizeof(size_t));
    series_write_info(h, static_cast<uint8_t*>(info));
    return drain_call(E, st, 0);
  });
}

int sperrhip_decompress_series_dev(const void* info, const void* d_src, const size_t* offsets, size_t t0, size_t nt,
                                   const size_t box_lo[3], const size_t box_dims[3], unsigned pct, int output_float,
                                   void* const* d_outs, void* hip_stream)
{
  return guarded("sperrhip_decompress_series_dev", [&]() -> int {
    SeriesInfo h;
    if (!info || !d_src || !offsets || !d_outs || (box_lo == nullptr) != (box_dims == nullptr) ||
        !series_parse_info(static_cast<const uint8_t*>(info), &h))
      return -1;
    const size_t nsteps = (size_t)h.n;
    std::vector<uint8_t> need(nsteps);
    if (!series_needs(nsteps, h.levels, t0, nt, need.data()))
      return -1;
    size_t lo[3], dims[3], n = 1;
    for (int a = 0; a < 3; a++) {
      lo[a] = box_lo ? box_lo[a] : 0;
      dims[a] = box_lo ? box_dims[a] : (size_t)h.dims[a];
      if (dims[a] == 0 || lo[a] >= h.dims[a] || dims[a] > h.dims[a] - lo[a])
        return -1;
      n *= dims[a];   // (at most the volume, whose count the compression call has seen to fit)
    }
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    for (size_t t = 0; t < nt; t++)
      if (!d_outs[t] || (uintptr_t)d_outs[t] % esz != 0)
        return -1;
    std::vector<const void*> srcs;
    std::vector<size_t> lens, boxLo, bandOf;
    for (size_t b = 0; b < nsteps; b++) {
      if (offsets[b + 1] < offsets[b])
        return -1;
      if (need[b]) {
        srcs.push_back(static_cast<const uint8_t*>(d_src) + offsets[b]);
        lens.push_back(offsets[b + 1] - offsets[b]);
        boxLo.insert(boxLo.end(), lo, lo + 3);
        bandOf.push_back(b);
      }
    }
    const size_t nb = srcs.size();
    if (n > SIZE_MAX / 8 / nb)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (E.seriesStage.ensure(nb * n * sizeof(double)))
      return -1;
    double* stage = static_cast<double*>(E.seriesStage.p);
    const Dims vol{(size_t)h.dims[0], (size_t)h.dims[1], (size_t)h.dims[2]};
    // ---- the needed bands, and no other, as doubles into the engine's buffer: the outputs are untouched until it ends well
    int rtn = decode_boxes_to(E, srcs.data(), lens.data(), nb, nullptr, boxLo.data(), nb, dims, nullptr, pct, 0, stage,
                              nb * n * sizeof(double), st, &vol);
    if (rtn != 0)
      return drain_call(E, st, rtn);
    std::vector<const void*> bands(nsteps, nullptr);
    std::vector<void*> outs(nsteps, nullptr);
    for (size_t k = 0; k < nb; k++)
      bands[bandOf[k]] = stage + k * n;
    for (size_t t = 0; t < nt; t++)
      outs[t0 + t] = d_outs[t];
    const void* const* dB;
    void* const* dO;
    if (upload_tables(E, bands, outs, &dB, &dO, st))
      return drain_call(E, st, -1);
    size_t g0, g1;
    groups_meeting(nsteps, h.levels, t0, nt, &g0, &g1);
    rtn = series_inverse_run(reinterpret_cast<const double* const*>(dB), dO, output_float, nsteps, h.levels, g0, g1, n,
                             st);
    return drain_call(E, st, rtn);
  });
}

}  // extern "C"
