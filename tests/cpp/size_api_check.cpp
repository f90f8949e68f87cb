// Drives the size mode's calls of include/sperr_hip.hpp -- size_survey_dev, compress_size_dev -- on one float volume;
// tests/test_cpp_size.py compares the outputs with the Python calls.
//   usage: size_api_check <volume.f32: (z, y, x)> <dimx> <dimy> <dimz> <chunk x> <chunk y> <chunk z> <target bytes>
//                         <container out> <budgets.u64 out> <survey out: q f64, nbp i32, end u64 x 32, is_const u8>
#include <hip/hip_runtime_api.h>

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
  if (argc != 12)
    return 2;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const sperr::dims_type dims{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])};
  const sperr::dims_type chunks{std::stoul(argv[5]), std::stoul(argv[6]), std::stoul(argv[7])};
  const size_t target = std::stoul(argv[8]);
  CHECK(raw.size() == dims[0] * dims[1] * dims[2] * sizeof(float));
  void *d_vol = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_vol, raw.size()) == hipSuccess && hipMalloc(&d_out, target + 16) == hipSuccess);
  CHECK(hipMemcpy(d_vol, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemset(d_out, 0x5a, target + 16) == hipSuccess);
  const float* vol = static_cast<const float*>(d_vol);

  sperr::SizeSurvey sv;
  CHECK(sperr::size_survey_dev(vol, dims, chunks, sv) == sperr::RTNType::Good);
  const size_t n = sv.q.size();
  CHECK(n > 0 && n == sperrhip_chunk_count(dims[0], dims[1], dims[2], chunks[0], chunks[1], chunks[2]));
  CHECK(sv.end.size() == n * 32 && sv.nbp.size() == n && sv.is_const.size() == n);

  // a target that does not hold the headers: refused, nothing written
  size_t len = 0;
  std::vector<uint64_t> budgets;
  CHECK(sperr::compress_size_dev(vol, dims, chunks, 40, d_out, target, len, &budgets) == sperr::RTNType::Error);
  std::vector<uint8_t> host(target + 16);
  CHECK(hipMemcpy(host.data(), d_out, host.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (uint8_t b : host)
    CHECK(b == 0x5a);

  CHECK(sperr::compress_size_dev(vol, dims, chunks, target, d_out, target, len, &budgets) == sperr::RTNType::Good);
  CHECK(len <= target && budgets.size() == n);
  CHECK(hipMemcpy(host.data(), d_out, host.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (size_t i = target; i < host.size(); i++)
    CHECK(host[i] == 0x5a);   // (nothing behind the capacity)

  std::FILE* o = std::fopen(argv[9], "wb");
  CHECK(o && std::fwrite(host.data(), 1, len, o) == len && std::fclose(o) == 0);
  o = std::fopen(argv[10], "wb");
  CHECK(o && std::fwrite(budgets.data(), 8, n, o) == n && std::fclose(o) == 0);
  o = std::fopen(argv[11], "wb");
  CHECK(o && std::fwrite(sv.q.data(), 8, n, o) == n && std::fwrite(sv.nbp.data(), 4, n, o) == n &&
        std::fwrite(sv.end.data(), 8, n * 32, o) == n * 32 && std::fwrite(sv.is_const.data(), 1, n, o) == n &&
        std::fclose(o) == 0);
  CHECK(hipFree(d_vol) == hipSuccess && hipFree(d_out) == hipSuccess);
  return 0;
}
