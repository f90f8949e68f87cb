// Drives the whole-volume PSNR calls of include/sperr_hip.hpp -- range_dev, compress_psnr_dev -- on one float volume;
// tests/test_cpp_psnr_vol.py compares the outputs with the Python calls.
//   usage: psnr_vol_api_check <volume.f32: (z, y, x)> <dimx> <dimy> <dimz> <chunk x> <chunk y> <chunk z> <psnr>
//                             <container out> <range out: min f64, max f64>
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

int main(int argc, char** argv)
{
  if (argc != 11)
    return 2;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const sperr::dims_type dims{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])};
  const sperr::dims_type chunks{std::stoul(argv[5]), std::stoul(argv[6]), std::stoul(argv[7])};
  const double psnr = std::stod(argv[8]);
  CHECK(raw.size() == dims[0] * dims[1] * dims[2] * sizeof(float));
  const size_t cap = sperrhip_max_compressed_size(dims[0], dims[1], dims[2], chunks[0], chunks[1], chunks[2], 2, psnr);
  void *d_vol = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_vol, raw.size()) == hipSuccess && hipMalloc(&d_out, cap + 16) == hipSuccess);
  CHECK(hipMemcpy(d_vol, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemset(d_out, 0x5a, cap + 16) == hipSuccess);
  const float* vol = static_cast<const float*>(d_vol);

  double lo = 0.0, hi = 0.0;
  CHECK(sperr::range_dev(vol, dims, lo, hi) == sperr::RTNType::Good);
  CHECK(lo < hi);
  // the dense view is the dense volume
  const sperr::view_type dense = sperr::dense_view(dims);
  double lo2 = 0.0, hi2 = 0.0;
  CHECK(sperr::range_dev(vol, dims, lo2, hi2, &dense) == sperr::RTNType::Good && lo2 == lo && hi2 == hi);

  // a target that is not a number: refused, nothing written
  size_t len = 4242;
  CHECK(sperr::compress_psnr_dev(vol, dims, chunks, std::nan(""), d_out, cap, len) == sperr::RTNType::Error && len == 4242);
  CHECK(sperr::compress_psnr_dev(vol, dims, chunks, psnr, d_out, cap, len, -1.0) == sperr::RTNType::Error && len == 4242);
  std::vector<uint8_t> host(cap + 16);
  CHECK(hipMemcpy(host.data(), d_out, host.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (uint8_t b : host)
    CHECK(b == 0x5a);

  CHECK(sperr::compress_psnr_dev(vol, dims, chunks, psnr, d_out, cap, len) == sperr::RTNType::Good);
  CHECK(len > 0 && len <= cap);
  CHECK(hipMemcpy(host.data(), d_out, host.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (size_t i = cap; i < host.size(); i++)
    CHECK(host[i] == 0x5a);   // (nothing behind the capacity)
  // the volume's own range given explicitly, through the dense view: the same bytes
  void* d_out2 = nullptr;
  size_t len2 = 0;
  CHECK(hipMalloc(&d_out2, cap) == hipSuccess);
  CHECK(sperr::compress_psnr_dev(vol, dims, chunks, psnr, d_out2, cap, len2, hi - lo, &dense) == sperr::RTNType::Good);
  std::vector<uint8_t> host2(len2);
  CHECK(len2 == len && hipMemcpy(host2.data(), d_out2, len2, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(std::memcmp(host.data(), host2.data(), len) == 0);

  std::FILE* o = std::fopen(argv[9], "wb");
  CHECK(o && std::fwrite(host.data(), 1, len, o) == len && std::fclose(o) == 0);
  o = std::fopen(argv[10], "wb");
  CHECK(o && std::fwrite(&lo, 8, 1, o) == 1 && std::fwrite(&hi, 8, 1, o) == 1 && std::fclose(o) == 0);
  CHECK(hipFree(d_vol) == hipSuccess && hipFree(d_out) == hipSuccess && hipFree(d_out2) == hipSuccess);
  return 0;
}
