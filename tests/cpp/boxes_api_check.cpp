// Drives sperr::decompress_boxes_dev of include/sperr_hip.hpp the way a reader of a time series would: the containers
// of a file are put into device allocations of their own, the same box is decoded out of every one of them as floats
// (no chunk shared: the direct form), then three boxes of which two overlap as doubles (the staged form), then one box
// per container of the coarsest level.  tests/test_cpp_boxes.py compares all three with the oracle.
//   usage: boxes_api_check <containers in> <offsets.u64 in: n + 1> <direct.f32 out> <staged.f64 out> <level.f64 out>
// Boxes (x, y, z): direct (5, 6, 7) + (20, 10, 9) of every container; staged the same dims at (5, 6, 7) and (6, 7, 8)
// of container 0 and at (0, 0, 0) of the last one; level 0, one sample at (1, 0, 1) of every container.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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
  if (argc != 6)
    return 2;
  std::vector<uint8_t> raw, offRaw;
  CHECK(read_file(argv[1], raw) && read_file(argv[2], offRaw) && offRaw.size() >= 16 && offRaw.size() % 8 == 0);
  std::vector<uint64_t> offs(offRaw.size() / 8);
  std::memcpy(offs.data(), offRaw.data(), offRaw.size());
  const size_t n = offs.size() - 1;
  CHECK(n >= 2 && offs[n] == raw.size());

  std::vector<const void*> streams(n);
  std::vector<size_t> lens(n);
  for (size_t c = 0; c < n; c++) {   // every container in an allocation of its own, the last one first
    const size_t k = n - 1 - c;
    void* d = nullptr;
    lens[k] = offs[k + 1] - offs[k];
    CHECK(hipMalloc(&d, lens[k]) == hipSuccess &&
          hipMemcpy(d, raw.data() + offs[k], lens[k], hipMemcpyHostToDevice) == hipSuccess);
    streams[k] = d;
  }
  const sperr::dims_type box{20, 10, 9}, at{5, 6, 7};
  const size_t vals = box[0] * box[1] * box[2];

  // direct: the same box of every container
  std::vector<float> direct(n * vals + 16);
  uint32_t sentinel = 0x7fc0beefu;
  float fill;
  std::memcpy(&fill, &sentinel, 4);
  std::fill(direct.begin(), direct.end(), fill);
  void* d_out = nullptr;
  CHECK(hipMalloc(&d_out, direct.size() * 4) == hipSuccess &&
        hipMemcpy(d_out, direct.data(), direct.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
  const std::vector<sperr::dims_type> same(n, at);
  // refusals first: too little room, a `which` of another length, a box that leaves the volume
  CHECK(sperr::decompress_boxes_dev({}, lens, {}, same, box, static_cast<float*>(d_out), n * vals * 4) == sperr::RTNType::Error);
  CHECK(sperr::decompress_boxes_dev(streams, lens, {}, same, box, static_cast<float*>(d_out), n * vals * 4 - 4) ==
        sperr::RTNType::Error);
  CHECK(sperr::decompress_boxes_dev(streams, lens, {0}, same, box, static_cast<float*>(d_out), n * vals * 4) ==
        sperr::RTNType::Error);
  CHECK(sperr::decompress_boxes_dev(streams, lens, {}, same, {20, 10, 1000}, static_cast<float*>(d_out), n * vals * 4) ==
        sperr::RTNType::Error);
  std::vector<float> untouched(direct.size());
  CHECK(hipMemcpy(untouched.data(), d_out, direct.size() * 4, hipMemcpyDeviceToHost) == hipSuccess &&
        std::memcmp(untouched.data(), direct.data(), direct.size() * 4) == 0);
  CHECK(sperr::decompress_boxes_dev(streams, lens, {}, same, box, static_cast<float*>(d_out), n * vals * 4) ==
        sperr::RTNType::Good);
  CHECK(hipMemcpy(direct.data(), d_out, direct.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
  for (size_t i = n * vals; i < direct.size(); i++)
    CHECK(std::memcmp(&direct[i], &fill, 4) == 0);

  // staged: two overlapping boxes of container 0 and one of the last container, as doubles
  std::vector<double> staged(3 * vals);
  void* d_staged = nullptr;
  CHECK(hipMalloc(&d_staged, staged.size() * 8) == hipSuccess);
  CHECK(sperr::decompress_boxes_dev(streams, lens, {0, 0, (uint32_t)(n - 1)}, {at, {6, 7, 8}, {0, 0, 0}}, box,
                                    static_cast<double*>(d_staged), staged.size() * 8) == sperr::RTNType::Good);
  CHECK(hipMemcpy(staged.data(), d_staged, staged.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);

  // a level: one sample of level 0 per container
  std::vector<double> level(n);
  void* d_level = nullptr;
  const size_t h = 0;
  CHECK(hipMalloc(&d_level, n * 8) == hipSuccess);
  const std::vector<sperr::dims_type> corner(n, sperr::dims_type{1, 0, 1});
  CHECK(sperr::decompress_boxes_dev(streams, lens, {}, corner, {1, 1, 1}, static_cast<double*>(d_level), n * 8, &h) ==
        sperr::RTNType::Good);
  CHECK(hipMemcpy(level.data(), d_level, n * 8, hipMemcpyDeviceToHost) == hipSuccess);

  CHECK(write_file(argv[3], direct.data(), n * vals * 4) && write_file(argv[4], staged.data(), staged.size() * 8) &&
        write_file(argv[5], level.data(), n * 8));
  for (const void* s : streams)
    CHECK(hipFree(const_cast<void*>(s)) == hipSuccess);
  CHECK(hipFree(d_out) == hipSuccess && hipFree(d_staged) == hipSuccess && hipFree(d_level) == hipSuccess);
  return 0;
}
