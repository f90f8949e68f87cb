// Drives the mask calls of include/sperr_hip.hpp on one small volume with NaNs: mask_make_dev alone, then
// compress_masked_dev, decompress_masked_dev whole and as a box, mask_apply_dev on a dense decode and
// quality_masked_dev.  tests/test_cpp_mask.py compares the outputs with the model, the oracle and the Python calls.
//   usage: mask_api_check <volume.f32: (z, y, x) with NaNs> <dimx> <dimy> <dimz> <container out> <mask out>
//                         <decoded.f32 out> <box.f32 out> <figures.f64 out>
// The box is (3, 5, 7) + (20, 9, 20); the decoded volume carries -7.5 at the missing samples, the box 1e20.
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

static bool write_file(const char* path, const void* p, size_t bytes)
{
  std::FILE* o = std::fopen(path, "wb");
  if (!o || std::fwrite(p, 1, bytes, o) != bytes)
    return false;
  return std::fclose(o) == 0;
}

int main(int argc, char** argv)
{
  if (argc != 10)
    return 2;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const sperr::dims_type dims{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])}, chunks{32, 32, 32};
  const sperr::dims_type lo{3, 5, 7}, bd{20, 9, 20};
  const size_t n = dims[0] * dims[1] * dims[2], nbox = bd[0] * bd[1] * bd[2];
  CHECK(raw.size() == n * sizeof(float));

  const size_t cap = sperrhip_max_compressed_size(dims[0], dims[1], dims[2], 32, 32, 32, 1, 2.5);
  const size_t mcap = sperrhip_mask_max_size(n);
  CHECK(mcap == 32 + 8 * ((n + 63) / 64));
  void *d_vol = nullptr, *d_out = nullptr, *d_mask = nullptr, *d_mask2 = nullptr, *d_dec = nullptr, *d_box = nullptr,
       *d_dense = nullptr;
  CHECK(hipMalloc(&d_vol, raw.size()) == hipSuccess && hipMalloc(&d_out, cap) == hipSuccess &&
        hipMalloc(&d_mask, mcap) == hipSuccess && hipMalloc(&d_mask2, mcap) == hipSuccess &&
        hipMalloc(&d_dec, n * 4) == hipSuccess && hipMalloc(&d_box, nbox * 4) == hipSuccess &&
        hipMalloc(&d_dense, n * 4) == hipSuccess);
  CHECK(hipMemcpy(d_vol, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess);
  const float* vol = static_cast<const float*>(d_vol);

  // the mask alone; a capacity one byte short names the size
  size_t mlen = 0, nmiss = 0, mlen2 = 0, nmiss2 = 0;
  CHECK(sperr::mask_make_dev(vol, n, sperr::MissingRule::NaN, 0.0, static_cast<float*>(nullptr), d_mask2, mcap, mlen2,
                             nmiss2) == sperr::RTNType::Good);
  size_t need = 0, dummy = 0;
  CHECK(sperr::mask_make_dev(vol, n, sperr::MissingRule::NaN, 0.0, static_cast<float*>(nullptr), d_mask, mlen2 - 1, need,
                             dummy) == sperr::RTNType::WrongLength && need == mlen2);
  CHECK(sperr::mask_make_dev(vol, n, sperr::MissingRule::AbsGE, -1.0, static_cast<float*>(nullptr), d_mask, mcap, need,
                             dummy) == sperr::RTNType::Error);

  size_t clen = 0;
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, sperr::CompMode::Unknown, 2.5, sperr::MissingRule::NaN, 0.0, d_out,
                                   cap, clen, d_mask, mcap, mlen, nmiss) == sperr::RTNType::CompModeUnknown);
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, sperr::CompMode::Rate, 2.5, sperr::MissingRule::NaN, 0.0, d_out,
                                   cap, clen, d_mask, mcap, mlen, nmiss) == sperr::RTNType::Good);
  CHECK(mlen == mlen2 && nmiss == nmiss2 && nmiss > 0 && nmiss < n && clen <= cap);
  std::vector<uint8_t> container(clen), mask(mlen), mask2(mlen2);
  CHECK(hipMemcpy(container.data(), d_out, clen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(mask.data(), d_mask, mlen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(mask2.data(), d_mask2, mlen2, hipMemcpyDeviceToHost) == hipSuccess && mask == mask2);

  // the decode, whole and as a box; a stream one byte short is refused
  float* dec = static_cast<float*>(d_dec);
  float* box = static_cast<float*>(d_box);
  CHECK(sperr::decompress_masked_dev(d_out, clen, d_mask, mlen - 1, -7.5, dec, n * 4) == sperr::RTNType::Error);
  CHECK(sperr::decompress_masked_dev(d_out, clen, d_mask, mlen, -7.5, dec, n * 4) == sperr::RTNType::Good);
  CHECK(sperr::decompress_masked_dev(d_out, clen, d_mask, mlen, 1e20, box, nbox * 4, &lo, &bd) == sperr::RTNType::Good);
  // mask_apply_dev on the dense decode gives the same volume
  float* dense = static_cast<float*>(d_dense);
  CHECK(sperrhip_decompress_dev(d_out, clen, 1, dense, n * 4, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(sperr::mask_apply_dev(dense, dims, nullptr, nullptr, d_mask, mlen, -7.5) == sperr::RTNType::Good);
  std::vector<float> h_dec(n), h_dense(n), h_box(nbox);
  CHECK(hipMemcpy(h_dec.data(), d_dec, n * 4, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(h_dense.data(), d_dense, n * 4, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(h_box.data(), d_box, nbox * 4, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(std::memcmp(h_dec.data(), h_dense.data(), n * 4) == 0);

  std::array<double, 8> fig{};
  CHECK(sperr::quality_masked_dev(vol, static_cast<const float*>(d_dec), n - 1, d_mask, mlen, fig) == sperr::RTNType::Error);
  CHECK(sperr::quality_masked_dev(vol, static_cast<const float*>(d_dec), n, d_mask, mlen, fig) == sperr::RTNType::Good);

  CHECK(write_file(argv[5], container.data(), clen) && write_file(argv[6], mask.data(), mlen) &&
        write_file(argv[7], h_dec.data(), n * 4) && write_file(argv[8], h_box.data(), nbox * 4) &&
        write_file(argv[9], fig.data(), 64));
  for (void* p : {d_vol, d_out, d_mask, d_mask2, d_dec, d_box, d_dense})
    CHECK(hipFree(p) == hipSuccess);
  return 0;
}
