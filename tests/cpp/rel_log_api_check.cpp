// Drives the relative error calls of include/sperr_hip.hpp with RelMap::log on one small float volume with zeros:
// rel_tolerance, rel_forward_dev and compress_rel_dev with the trailing map argument, then decompress_rel_dev whole and
// as a box and rel_inverse_dev in place, which take the kind from the side stream; the same calls without the argument
// stay the linear kind's.  tests/test_cpp_rel_log.py compares the outputs with the model and the Python calls.
//   usage: rel_log_api_check <volume.f32: (z, y, x)> <dimx> <dimy> <dimz> <eps> <container out> <side out> <y.f64 out>
//                            <decoded.f32 out> <box.f64 out> <linear container out>
// Chunks are (20, 18, 16), the box is (3, 5, 7) + (21, 17, 13).
#include <hip/hip_runtime_api.h>

#include <algorithm>
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
  using sperr::RelMap;
  using sperr::RTNType;
  if (argc != 12)
    return 2;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const sperr::dims_type dims{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])}, chunks{20, 18, 16};
  const sperr::dims_type lo{3, 5, 7}, bd{21, 17, 13};
  const double eps = std::stod(argv[5]);
  const size_t n = dims[0] * dims[1] * dims[2], nbox = bd[0] * bd[1] * bd[2];
  CHECK(raw.size() == n * sizeof(float));

  // the tolerance of the two kinds: the log kind's is the larger, and its floor the lower
  double t = 0.0, tlin = 0.0, none = 0.0;
  CHECK(sperr::rel_tolerance<float>(eps, t, RelMap::log) == RTNType::Good &&
        sperr::rel_tolerance<float>(eps, tlin) == RTNType::Good && t > 1.4 * tlin && t < 1.5 * eps);
  CHECK(sperr::rel_tolerance<float>(eps, none, RelMap::linear) == RTNType::Good && none == tlin);
  CHECK(sperr::rel_tolerance<float>(0.75, none, RelMap::log) == RTNType::Error);
  CHECK(sperr::rel_tolerance<float>(0x1.8p-22, none, RelMap::log) == RTNType::Good &&
        sperr::rel_tolerance<float>(0x1.8p-22, none) == RTNType::Error);
  CHECK(sperr::rel_tolerance<float>(eps, none, static_cast<RelMap>(2)) == RTNType::Error);
  const size_t cap = std::max(sperrhip_max_compressed_size(dims[0], dims[1], dims[2], 20, 18, 16, 3, tlin),
                              sperrhip_max_compressed_size(dims[0], dims[1], dims[2], 20, 18, 16, 3, t));
  const size_t scap = sperrhip_rel_max_size(n);
  void *d_vol = nullptr, *d_out = nullptr, *d_lin = nullptr, *d_side = nullptr, *d_side2 = nullptr, *d_y = nullptr,
       *d_dec = nullptr, *d_box = nullptr, *d_dense = nullptr;
  CHECK(hipMalloc(&d_vol, raw.size()) == hipSuccess && hipMalloc(&d_out, cap) == hipSuccess &&
        hipMalloc(&d_lin, cap) == hipSuccess && hipMalloc(&d_side, scap) == hipSuccess &&
        hipMalloc(&d_side2, scap) == hipSuccess && hipMalloc(&d_y, n * 8) == hipSuccess &&
        hipMalloc(&d_dec, n * 4) == hipSuccess && hipMalloc(&d_box, nbox * 8) == hipSuccess &&
        hipMalloc(&d_dense, n * 8) == hipSuccess);
  CHECK(hipMemcpy(d_vol, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess);
  const float* vol = static_cast<const float*>(d_vol);

  // the forward map alone; a capacity one byte short names the size; an unknown kind is refused
  size_t slen2 = 0, nzero = 0, nneg = 0, need = 0, d0 = 0, d1 = 0;
  CHECK(sperr::rel_forward_dev(vol, n, static_cast<double*>(d_y), d_side2, scap, slen2, nzero, nneg, nullptr,
                               RelMap::log) == RTNType::Good);
  CHECK(nzero > 0 && nzero < n && nneg > 0 && nneg < n);
  CHECK(sperr::rel_forward_dev(vol, n, static_cast<double*>(d_dense), d_side, slen2 - 1, need, d0, d1, nullptr,
                               RelMap::log) == RTNType::WrongLength && need == slen2);
  CHECK(sperr::rel_forward_dev(vol, n, static_cast<double*>(d_dense), d_side, scap, need, d0, d1, nullptr,
                               static_cast<RelMap>(2)) == RTNType::Error);

  size_t clen = 0, slen = 0, llen = 0, lslen = 0;
  CHECK(sperr::compress_rel_dev(vol, dims, chunks, 0.75, sperr::FillKind::Smooth, 0.0, d_out, cap, clen, d_side, scap,
                                slen, nullptr, RelMap::log) == RTNType::Error);
  CHECK(sperr::compress_rel_dev(vol, dims, chunks, eps, sperr::FillKind::Smooth, 0.0, d_out, cap, clen, d_side,
                                slen2 - 1, slen, nullptr, RelMap::log) == RTNType::WrongLength && slen == slen2);
  CHECK(sperr::compress_rel_dev(vol, dims, chunks, eps, sperr::FillKind::Smooth, 0.0, d_lin, cap, llen, d_side2, scap,
                                lslen) == RTNType::Good);
  CHECK(sperr::compress_rel_dev(vol, dims, chunks, eps, sperr::FillKind::Smooth, 0.0, d_out, cap, clen, d_side, scap,
                                slen, nullptr, RelMap::log) == RTNType::Good);
  CHECK(slen == slen2 && lslen == slen2 && clen < llen);   // the log kind's container is the smaller
  std::vector<uint8_t> container(clen), linear(llen), side(slen), lside(lslen);
  std::vector<double> h_y(n);
  CHECK(hipMemcpy(container.data(), d_out, clen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(linear.data(), d_lin, llen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(side.data(), d_side, slen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(lside.data(), d_side2, lslen, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(h_y.data(), d_y, n * 8, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(std::memcmp(side.data(), "SPLG", 4) == 0 && std::memcmp(lside.data(), "SPRL", 4) == 0 &&
        std::memcmp(side.data() + 4, lside.data() + 4, slen - 4) == 0);
  int kind = -1;
  CHECK(sperrhip_rel_parse_stream_kind_dev(d_side, slen, nullptr, nullptr, nullptr, nullptr, nullptr, &kind, nullptr) == 0 &&
        kind == SPERRHIP_REL_LOG);
  CHECK(sperrhip_rel_parse_stream_kind_dev(d_side2, lslen, nullptr, nullptr, nullptr, nullptr, nullptr, &kind, nullptr) == 0 &&
        kind == SPERRHIP_REL_LINEAR);

  // the decode, whole as floats and a box as doubles: the kind is the stream's
  float* dec = static_cast<float*>(d_dec);
  double* box = static_cast<double*>(d_box);
  CHECK(sperr::decompress_rel_dev(d_out, clen, d_side, slen - 1, dec, n * 4) == RTNType::Error);
  CHECK(sperr::decompress_rel_dev(d_out, clen, d_side, slen, dec, n * 4) == RTNType::Good);
  CHECK(sperr::decompress_rel_dev(d_out, clen, d_side, slen, box, nbox * 8, &lo, &bd) == RTNType::Good);
  double* dense = static_cast<double*>(d_dense);
  CHECK(sperrhip_decompress_box_dev(d_out, clen, 0, lo.data(), bd.data(), dense, nbox * 8, nullptr) == 0);
  CHECK(sperr::rel_inverse_dev(dense, dims, &lo, &bd, d_side, slen, dense) == RTNType::Good);
  std::vector<float> h_dec(n);
  std::vector<double> h_box(nbox), h_dense(nbox);
  CHECK(hipMemcpy(h_dec.data(), d_dec, n * 4, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(h_box.data(), d_box, nbox * 8, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(h_dense.data(), d_dense, nbox * 8, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(std::memcmp(h_box.data(), h_dense.data(), nbox * 8) == 0);

  std::array<double, 4> fig{};
  CHECK(sperr::rel_check_dev(vol, static_cast<const float*>(d_dec), n, eps, fig) == RTNType::Good);
  CHECK(fig[1] == 0.0 && fig[2] == 0.0 && fig[3] == (double)(n - nzero) && fig[0] <= eps);

  CHECK(write_file(argv[6], container.data(), clen) && write_file(argv[7], side.data(), slen) &&
        write_file(argv[8], h_y.data(), n * 8) && write_file(argv[9], h_dec.data(), n * 4) &&
        write_file(argv[10], h_box.data(), nbox * 8) && write_file(argv[11], linear.data(), llen));
  for (void* p : {d_vol, d_out, d_lin, d_side, d_side2, d_y, d_dec, d_box, d_dense})
    CHECK(hipFree(p) == hipSuccess);
  return 0;
}
