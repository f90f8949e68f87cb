// Drives the fill overloads of include/sperr_hip.hpp on one small volume with NaNs: mask_make_dev with a smooth fill
// and with a value, compress_masked_dev with each fill kind, and the refusals.  tests/test_cpp_mask_fill.py compares
// the outputs with the models and the oracle.
//   usage: mask_fill_api_check <volume.f32: (z, y, x) with NaNs> <dimx> <dimy> <dimz> <smooth filled.f32 out>
//                              <value filled.f32 out> <smooth container out> <value container out> <mask out>
// The value is 3.5, the chunks are 32^3, the mode is a rate of 2.5 bits per sample.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sperr_hip.hpp"

#define CHECK(cond)                                         \
  if (!(cond)) {                                            \
    std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    return 1;                                               \
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
  using sperr::CompMode;
  using sperr::FillKind;
  using sperr::MissingRule;
  using sperr::RTNType;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const sperr::dims_type dims{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])}, chunks{32, 32, 32};
  const size_t n = dims[0] * dims[1] * dims[2];
  CHECK(raw.size() == n * sizeof(float));
  const size_t cap = sperrhip_max_compressed_size(dims[0], dims[1], dims[2], 32, 32, 32, 1, 2.5);
  const size_t mcap = sperrhip_mask_max_size(n);
  void *d_vol = nullptr, *d_fill = nullptr, *d_out = nullptr, *d_mask = nullptr, *d_mask2 = nullptr;
  CHECK(hipMalloc(&d_vol, raw.size()) == hipSuccess && hipMalloc(&d_fill, raw.size()) == hipSuccess &&
        hipMalloc(&d_out, cap) == hipSuccess && hipMalloc(&d_mask, mcap) == hipSuccess &&
        hipMalloc(&d_mask2, mcap) == hipSuccess);
  CHECK(hipMemcpy(d_vol, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess);
  const float* vol = static_cast<const float*>(d_vol);
  float* fill = static_cast<float*>(d_fill);

  // the mask and the in-filled volume, smooth and with a value; the stream is the same, and that of the call without a fill
  size_t mlen = 0, nmiss = 0, mlen2 = 0, nmiss2 = 0;
  std::vector<float> smooth(n), valued(n);
  CHECK(sperr::mask_make_dev(vol, dims, MissingRule::NaN, 0.0, FillKind::Smooth, 0.0, fill, d_mask, mcap, mlen, nmiss) ==
        RTNType::Good);
  CHECK(hipMemcpy(smooth.data(), d_fill, n * 4, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(sperr::mask_make_dev(vol, dims, MissingRule::NaN, 0.0, FillKind::Value, 3.5, fill, d_mask2, mcap, mlen2, nmiss2) ==
        RTNType::Good);
  CHECK(hipMemcpy(valued.data(), d_fill, n * 4, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(mlen == mlen2 && nmiss == nmiss2 && nmiss > 0 && nmiss < n);
  std::vector<uint8_t> mask(mlen), mask2(mlen);
  CHECK(hipMemcpy(mask.data(), d_mask, mlen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(mask2.data(), d_mask2, mlen, hipMemcpyDeviceToHost) == hipSuccess && mask == mask2);
  CHECK(sperr::mask_make_dev(vol, n, MissingRule::NaN, 0.0, static_cast<float*>(nullptr), d_mask2, mcap, mlen2, nmiss2) ==
        RTNType::Good);
  CHECK(mlen2 == mlen && hipMemcpy(mask2.data(), d_mask2, mlen, hipMemcpyDeviceToHost) == hipSuccess && mask == mask2);

  // refusals: a value that is not finite, or not as a float; a capacity one byte short names the size
  size_t need = 0, dummy = 0;
  const double inf = std::numeric_limits<double>::infinity();
  CHECK(sperr::mask_make_dev(vol, dims, MissingRule::NaN, 0.0, FillKind::Value, inf, fill, d_mask2, mcap, need, dummy) ==
        RTNType::Error);
  CHECK(sperr::mask_make_dev(vol, dims, MissingRule::NaN, 0.0, FillKind::Value, 1e39, fill, d_mask2, mcap, need, dummy) ==
        RTNType::Error);
  CHECK(sperr::mask_make_dev(vol, dims, MissingRule::NaN, 0.0, static_cast<FillKind>(3), 0.0, fill, d_mask2, mcap, need,
                             dummy) == RTNType::Error);
  CHECK(sperr::mask_make_dev(vol, dims, MissingRule::NaN, 0.0, FillKind::Smooth, 0.0, fill, d_mask2, mlen - 1, need,
                             dummy) == RTNType::WrongLength && need == mlen);

  // the containers: smooth, a value, and the midrange spelled out against the call without a fill
  size_t clen = 0, clen2 = 0;
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, CompMode::Unknown, 2.5, MissingRule::NaN, 0.0, FillKind::Smooth, 0.0,
                                   d_out, cap, clen, d_mask2, mcap, mlen2, nmiss2) == RTNType::CompModeUnknown);
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, CompMode::Rate, 2.5, MissingRule::NaN, 0.0, FillKind::Value, -inf,
                                   d_out, cap, clen, d_mask2, mcap, mlen2, nmiss2) == RTNType::Error);
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, CompMode::Rate, 2.5, MissingRule::NaN, 0.0, FillKind::Smooth, 0.0,
                                   d_out, cap, clen, d_mask2, mcap, mlen2, nmiss2) == RTNType::Good);
  CHECK(mlen2 == mlen && nmiss2 == nmiss && clen <= cap);
  std::vector<uint8_t> c_smooth(clen);
  CHECK(hipMemcpy(c_smooth.data(), d_out, clen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, CompMode::Rate, 2.5, MissingRule::NaN, 0.0, FillKind::Value, 3.5,
                                   d_out, cap, clen, d_mask2, mcap, mlen2, nmiss2) == RTNType::Good);
  std::vector<uint8_t> c_value(clen);
  CHECK(hipMemcpy(c_value.data(), d_out, clen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, CompMode::Rate, 2.5, MissingRule::NaN, 0.0, FillKind::Midrange, 0.0,
                                   d_out, cap, clen, d_mask2, mcap, mlen2, nmiss2) == RTNType::Good);
  std::vector<uint8_t> c_mid(clen);
  CHECK(hipMemcpy(c_mid.data(), d_out, clen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(sperr::compress_masked_dev(vol, dims, chunks, CompMode::Rate, 2.5, MissingRule::NaN, 0.0, d_out, cap, clen2,
                                   d_mask2, mcap, mlen2, nmiss2) == RTNType::Good);
  std::vector<uint8_t> c_old(clen2);
  CHECK(hipMemcpy(c_old.data(), d_out, clen2, hipMemcpyDeviceToHost) == hipSuccess && c_old == c_mid);

  CHECK(write_file(argv[5], smooth.data(), n * 4) && write_file(argv[6], valued.data(), n * 4) &&
        write_file(argv[7], c_smooth.data(), c_smooth.size()) && write_file(argv[8], c_value.data(), c_value.size()) &&
        write_file(argv[9], mask.data(), mlen));
  for (void* p : {d_vol, d_fill, d_out, d_mask, d_mask2})
    CHECK(hipFree(p) == hipSuccess);
  return 0;
}
