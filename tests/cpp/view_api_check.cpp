// Drives the view calls of include/sperr_hip.hpp the way an application that holds its field on the device with ghost
// cells would: a container is decoded into the interior of a padded device array (decompress_view_dev), and the
// figures of that interior against the interior of another padded array, which holds the original at another pitch,
// are taken where they lie (quality_view_dev).  tests/test_cpp_view.py compares both with the Python results.
//   usage: view_api_check <container> <original.f32> <dimx> <dimy> <dimz> <parent.f32 out> <figures.f64 out>
// The decode's parent has a halo of (2 + 3, 1 + 2, 1 + 1) cells of the bit pattern 0x7fc0beef.
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
  if (argc != 8)
    return 2;
  std::vector<uint8_t> stream, raw;
  CHECK(read_file(argv[1], stream) && read_file(argv[2], raw));
  const sperr::dims_type dims{std::stoul(argv[3]), std::stoul(argv[4]), std::stoul(argv[5])};
  const size_t n = dims[0] * dims[1] * dims[2];
  CHECK(raw.size() == n * sizeof(float));

  // the decode's parent, and the original inside a parent of its own (halo (0 + 5, 3 + 0, 0 + 1))
  const sperr::dims_type pd{dims[0] + 5, dims[1] + 3, dims[2] + 2}, po{dims[0] + 5, dims[1] + 3, dims[2] + 1};
  const sperr::view_type vd{pd[0], pd[0] * pd[1]}, vo{po[0], po[0] * po[1]};
  const size_t firstD = (1 * pd[1] + 1) * pd[0] + 2, firstO = 3 * po[0];
  uint32_t sentinel = 0x7fc0beefu;
  float fill;
  std::memcpy(&fill, &sentinel, 4);
  std::vector<float> parent(pd[0] * pd[1] * pd[2], fill), orig(po[0] * po[1] * po[2], fill);
  for (size_t z = 0; z < dims[2]; z++)
    for (size_t y = 0; y < dims[1]; y++)
      std::memcpy(&orig[firstO + z * vo.pitch_z + y * vo.pitch_y], raw.data() + (z * dims[1] + y) * dims[0] * 4,
                  dims[0] * 4);

  void *d_stream = nullptr, *d_parent = nullptr, *d_orig = nullptr;
  CHECK(hipMalloc(&d_stream, stream.size()) == hipSuccess && hipMalloc(&d_parent, parent.size() * 4) == hipSuccess &&
        hipMalloc(&d_orig, orig.size() * 4) == hipSuccess);
  CHECK(hipMemcpy(d_stream, stream.data(), stream.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_parent, parent.data(), parent.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_orig, orig.data(), orig.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
  float* interior = static_cast<float*>(d_parent) + firstD;
  const float* original = static_cast<const float*>(d_orig) + firstO;
  const size_t room = (parent.size() - firstD) * 4;

  // refusals first: a view that is none, and one float too little room
  const sperr::view_type overlapping{dims[0] - 1, vd.pitch_z};
  CHECK(sperr::decompress_view_dev(d_stream, stream.size(), interior, overlapping, room) == sperr::RTNType::Error);
  const size_t extent = (dims[2] - 1) * vd.pitch_z + (dims[1] - 1) * vd.pitch_y + dims[0];
  CHECK(sperr::decompress_view_dev(d_stream, stream.size(), interior, vd, extent * 4 - 4) == sperr::RTNType::Error);
  std::array<double, 8> fig{};
  CHECK(sperr::quality_view_dev(original, &overlapping, interior, &vd, dims, fig) == sperr::RTNType::Error);

  CHECK(sperr::decompress_view_dev(d_stream, stream.size(), interior, vd, extent * 4) == sperr::RTNType::Good);
  CHECK(sperr::quality_view_dev(original, &vo, interior, &vd, dims, fig) == sperr::RTNType::Good);
  // the same figures with the decode on the other side of the call, and dense views of packed copies
  std::array<double, 8> self{};
  CHECK(sperr::quality_view_dev(interior, &vd, interior, &vd, dims, self) == sperr::RTNType::Good);
  CHECK(self[0] == 0.0 && self[1] == 0.0 && self[2] > 1e300 && self[7] == 0.0);

  CHECK(hipMemcpy(parent.data(), d_parent, parent.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
  std::FILE* o = std::fopen(argv[6], "wb");
  CHECK(o && std::fwrite(parent.data(), 4, parent.size(), o) == parent.size());
  CHECK(std::fclose(o) == 0);
  o = std::fopen(argv[7], "wb");
  CHECK(o && std::fwrite(fig.data(), 8, 8, o) == 8);
  CHECK(std::fclose(o) == 0);
  CHECK(hipFree(d_stream) == hipSuccess && hipFree(d_parent) == hipSuccess && hipFree(d_orig) == hipSuccess);
  return 0;
}
