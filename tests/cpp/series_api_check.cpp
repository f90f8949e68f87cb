// Drives the time-series calls of include/sperr_hip.hpp -- series_plan, series_needs, series_tolerance,
// series_forward_dev, series_inverse_dev, compress_series_dev, decompress_series_dev -- on one float series;
// tests/test_cpp_series.py compares the outputs with the Python calls.
//   usage: series_api_check <series.f32: (t, z, y, x)> <steps> <dimx> <dimy> <dimz> <chunk x> <chunk y> <chunk z>
//                           <levels> <tol> <containers out> <offsets out: u64 each> <info out> <t0> <nt>
//                           <steps out: nt volumes, f64> <bands out: all bands, f64>
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sperr_hip.hpp"

#define CHECK(cond)                                              \
  if (!(cond)) {                                                 \
    std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
    return 1;                                                    \
  }

static bool read_file(const char* path, std::vector<uint8_t>& out)
{
  std::FILE* f = std::fopen(path, "rb");
  if (!f)
    return false;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;)
    out.insert(out.end(), buf, buf + n);
  return std::fclose(f) == 0;
}

static bool write_file(const char* path, const void* p, size_t bytes)
{
  std::FILE* o = std::fopen(path, "wb");
  return o && std::fwrite(p, 1, bytes, o) == bytes && std::fclose(o) == 0;
}

int main(int argc, char** argv)
{
  if (argc != 18)
    return 2;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const size_t nsteps = std::stoul(argv[2]);
  const sperr::dims_type dims{std::stoul(argv[3]), std::stoul(argv[4]), std::stoul(argv[5])};
  const sperr::dims_type chunks{std::stoul(argv[6]), std::stoul(argv[7]), std::stoul(argv[8])};
  const unsigned levels = (unsigned)std::stoul(argv[9]);
  const double tol = std::stod(argv[10]);
  const size_t t0 = std::stoul(argv[14]), nt = std::stoul(argv[15]);
  const size_t n = dims[0] * dims[1] * dims[2];
  CHECK(raw.size() == nsteps * n * sizeof(float) && t0 + nt <= nsteps && nt > 0);

  // ---- host only
  const auto plan = sperr::series_plan(nsteps, levels);
  size_t covered = 0;
  for (auto& g : plan) {
    CHECK(g.first == covered && g.second <= levels);
    covered += size_t(1) << g.second;
  }
  CHECK(covered == nsteps && sperr::series_plan(0, levels).empty() && sperr::series_plan(nsteps, 5).empty());
  CHECK(sperr::series_needs(nsteps, levels, 0, nsteps).size() == nsteps);
  CHECK(sperr::series_needs(nsteps, levels, nsteps, 1).empty() && sperr::series_needs(nsteps, levels, 0, 0).empty());
  const auto need = sperr::series_needs(nsteps, levels, t0, nt);
  CHECK(!need.empty() && need.size() <= nsteps);
  double rho = -1.0;
  std::vector<double> tau;
  CHECK(sperr::series_tolerance(tol, 1.0, levels, rho, tau) == sperr::RTNType::Good && tau.size() == levels + 1);
  CHECK(rho >= 0.0 && tau[levels] <= tau[0] && tau[0] <= tol);
  CHECK(sperr::series_tolerance(0.0, 1.0, levels, rho, tau) == sperr::RTNType::Error && tau.empty());

  // ---- the device calls; the steps do not lie back to back: one allocation each
  std::vector<const float*> steps(nsteps);
  for (size_t t = 0; t < nsteps; t++) {
    void* p = nullptr;
    CHECK(hipMalloc(&p, n * sizeof(float)) == hipSuccess);
    CHECK(hipMemcpy(p, raw.data() + t * n * sizeof(float), n * sizeof(float), hipMemcpyHostToDevice) == hipSuccess);
    steps[t] = static_cast<const float*>(p);
  }
  const size_t cap = sperrhip_max_compressed_size_batch(nsteps, dims[0], dims[1], dims[2], chunks[0], chunks[1], chunks[2], 3, tol);
  void *d_out = nullptr, *d_bands = nullptr, *d_back = nullptr;
  CHECK(cap > 0 && hipMalloc(&d_out, cap) == hipSuccess && hipMalloc(&d_bands, nsteps * n * 8) == hipSuccess &&
        hipMalloc(&d_back, nt * n * 8) == hipSuccess);
  CHECK(hipMemset(d_back, 0x5a, nt * n * 8) == hipSuccess);

  std::vector<size_t> offsets;
  sperr::series_info_type info{};
  // refusals: nothing is written
  CHECK(sperr::compress_series_dev(steps, dims, chunks, 5, sperr::SeriesKind::tol, tol, d_out, cap, offsets, info) ==
        sperr::RTNType::Error);
  CHECK(sperr::compress_series_dev(steps, dims, chunks, levels, sperr::SeriesKind::tol, -1.0, d_out, cap, offsets, info) ==
        sperr::RTNType::Error);
  CHECK(info[0] == 0);
  CHECK(sperr::compress_series_dev(steps, dims, chunks, levels, sperr::SeriesKind::tol, tol, d_out, cap, offsets, info) ==
        sperr::RTNType::Good);
  CHECK(offsets.size() == nsteps + 1 && offsets[0] == 0 && offsets[nsteps] <= cap && std::memcmp(info.data(), "SPTS", 4) == 0);
  std::vector<uint8_t> host(offsets[nsteps]);
  CHECK(hipMemcpy(host.data(), d_out, host.size(), hipMemcpyDeviceToHost) == hipSuccess);

  std::vector<double*> outs(nt);
  for (size_t t = 0; t < nt; t++)
    outs[t] = static_cast<double*>(d_back) + t * n;
  sperr::series_info_type bad = info;
  bad[0] = 'X';
  std::vector<double> back(nt * n);
  CHECK(sperr::decompress_series_dev(bad, d_out, offsets, t0, outs) == sperr::RTNType::Error);
  CHECK(hipMemcpy(back.data(), d_back, back.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
  for (size_t i = 0; i < back.size(); i++) {
    uint64_t b;
    std::memcpy(&b, &back[i], 8);
    CHECK(b == 0x5a5a5a5a5a5a5a5aull);
  }
  CHECK(sperr::decompress_series_dev(info, d_out, offsets, t0, outs) == sperr::RTNType::Good);
  CHECK(hipMemcpy(back.data(), d_back, back.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);

  // the stages: forward, and the inverse of the range gives the steps back to rounding
  std::vector<double> bands(nsteps * n);
  CHECK(sperr::series_forward_dev(steps, levels, n, static_cast<double*>(d_bands)) == sperr::RTNType::Good);
  CHECK(hipMemcpy(bands.data(), d_bands, bands.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
  std::vector<float*> fouts(nt);
  void* d_f = nullptr;
  CHECK(hipMalloc(&d_f, nt * n * sizeof(float)) == hipSuccess);
  for (size_t t = 0; t < nt; t++)
    fouts[t] = static_cast<float*>(d_f) + t * n;
  CHECK(sperr::series_inverse_dev(static_cast<const double*>(d_bands), nsteps, levels, n, t0, fouts) == sperr::RTNType::Good);
  std::vector<float> fback(nt * n);
  CHECK(hipMemcpy(fback.data(), d_f, fback.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess);
  // (the doubles are within rho of the floats they came from -- rho of a tolerance of M is K 2^-53 M --, and the
  //  narrowing adds half a float's spacing at most)
  const float* orig = reinterpret_cast<const float*>(raw.data());
  double M = 0.0, rhoM = 0.0;
  for (size_t i = 0; i < nsteps * n; i++)
    M = std::fmax(M, std::fabs((double)orig[i]));
  CHECK(M > 0.0 && sperr::series_tolerance(M, M, levels, rhoM, tau) == sperr::RTNType::Good);
  for (size_t i = 0; i < fback.size(); i++) {
    const double x = orig[t0 * n + i];
    CHECK(std::fabs((double)fback[i] - x) <= rhoM + std::fabs(x) * 0x1p-24);
  }

  std::vector<uint64_t> offs64(offsets.begin(), offsets.end());
  CHECK(write_file(argv[11], host.data(), host.size()) && write_file(argv[12], offs64.data(), offs64.size() * 8) &&
        write_file(argv[13], info.data(), info.size()) && write_file(argv[16], back.data(), back.size() * 8) &&
        write_file(argv[17], bands.data(), bands.size() * 8));
  for (auto p : steps)
    CHECK(hipFree(const_cast<float*>(p)) == hipSuccess);
  CHECK(hipFree(d_out) == hipSuccess && hipFree(d_bands) == hipSuccess && hipFree(d_back) == hipSuccess &&
        hipFree(d_f) == hipSuccess);
  sperrhip_release();
  return 0;
}
