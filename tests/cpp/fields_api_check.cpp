// Drives the fields calls of include/sperr_hip.hpp the way a solver that keeps (z, y, x, nvar) on the device would:
// three interleaved fields are compressed into three containers (compress_fields_dev), the containers are decoded into
// fields 1..3 of a five-wide record of a parent with padded rows and slices (decompress_fields_dev), and the figures
// of the decode against the original are taken where both lie (quality_fields_dev).  tests/test_cpp_fields.py
// compares all three with the oracle and the Python results.
//   usage: fields_api_check <original.f32: (z, y, x, 3)> <dimx> <dimy> <dimz> <containers out> <offsets.u64 out>
//                           <parent.f32 out> <figures.f64 out>
// The parent is (dimz, dimy + 1 rows, (dimx + 2) records of 5) plus 3 floats per slice, of the bit pattern 0x7fc0beef;
// sample (0, 0, 0) is its record 1 of row 0 of slice 0.
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
  if (argc != 9)
    return 2;
  std::vector<uint8_t> raw;
  CHECK(read_file(argv[1], raw));
  const sperr::dims_type dims{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])}, chunks{32, 32, 32};
  const size_t nf = 3, n = dims[0] * dims[1] * dims[2];
  CHECK(raw.size() == nf * n * sizeof(float));

  const sperr::fields_type wide{5, (dims[0] + 2) * 5, (dims[0] + 2) * 5 * (dims[1] + 1) + 3};
  const size_t first = 1 * 5 + 1;   // record 1, field 1
  const size_t parentLen = wide.pitch_z * dims[2];
  const size_t extent = (dims[2] - 1) * wide.pitch_z + (dims[1] - 1) * wide.pitch_y + (dims[0] - 1) * 5 + nf;
  CHECK(first + extent <= parentLen);
  uint32_t sentinel = 0x7fc0beefu;
  float fill;
  std::memcpy(&fill, &sentinel, 4);
  std::vector<float> parent(parentLen, fill);

  const size_t cap = sperrhip_max_compressed_size_batch(nf, dims[0], dims[1], dims[2], 32, 32, 32, 1, 2.5);
  void *d_orig = nullptr, *d_parent = nullptr, *d_streams = nullptr;
  CHECK(cap != 0 && hipMalloc(&d_orig, raw.size()) == hipSuccess && hipMalloc(&d_parent, parentLen * 4) == hipSuccess &&
        hipMalloc(&d_streams, cap) == hipSuccess);
  CHECK(hipMemcpy(d_orig, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_parent, parent.data(), parentLen * 4, hipMemcpyHostToDevice) == hipSuccess);
  const float* original = static_cast<const float*>(d_orig);
  float* target = static_cast<float*>(d_parent) + first;
  const size_t room = (parentLen - first) * 4;

  // refusals first: more fields than the record holds, rows that overlap
  std::vector<size_t> offsets;
  const sperr::fields_type narrow{2, dims[0] * 2, dims[0] * dims[1] * 2}, overlapping{3, dims[0] * 3 - 1, n * 3};
  CHECK(sperr::compress_fields_dev(original, &narrow, nf, dims, chunks, sperr::CompMode::Rate, 2.5, d_streams, cap,
                                   offsets) == sperr::RTNType::Error);
  CHECK(sperr::compress_fields_dev(original, &overlapping, nf, dims, chunks, sperr::CompMode::Rate, 2.5, d_streams, cap,
                                   offsets) == sperr::RTNType::Error);
  CHECK(sperr::compress_fields_dev(original, nullptr, nf, dims, chunks, sperr::CompMode::Unknown, 2.5, d_streams, cap,
                                   offsets) == sperr::RTNType::CompModeUnknown);

  // a null layout is the dense interleave; so is dense_fields()
  CHECK(sperr::compress_fields_dev(original, nullptr, nf, dims, chunks, sperr::CompMode::Rate, 2.5, d_streams, cap,
                                   offsets) == sperr::RTNType::Good);
  CHECK(offsets.size() == nf + 1 && offsets[0] == 0 && offsets[nf] <= cap);
  std::vector<uint8_t> streams(offsets[nf]);
  CHECK(hipMemcpy(streams.data(), d_streams, streams.size(), hipMemcpyDeviceToHost) == hipSuccess);
  const sperr::fields_type dense = sperr::dense_fields(nf, dims);
  std::vector<size_t> again;
  void* d_again = nullptr;
  CHECK(hipMalloc(&d_again, cap) == hipSuccess);
  CHECK(sperr::compress_fields_dev(original, &dense, nf, dims, chunks, sperr::CompMode::Rate, 2.5, d_again, cap,
                                   again) == sperr::RTNType::Good && again == offsets);
  std::vector<uint8_t> streams2(again[nf]);
  CHECK(hipMemcpy(streams2.data(), d_again, streams2.size(), hipMemcpyDeviceToHost) == hipSuccess && streams2 == streams);

  // the decode: one float too little room is refused, the extent exactly is enough
  CHECK(sperr::decompress_fields_dev(d_streams, offsets, dims, target, &wide, extent * 4 - 4) == sperr::RTNType::Error);
  CHECK(sperr::decompress_fields_dev(d_streams, offsets, {dims[1], dims[0], dims[2]}, target, &wide, room) ==
        sperr::RTNType::Error);
  CHECK(sperr::decompress_fields_dev(d_streams, offsets, dims, target, &wide, extent * 4) == sperr::RTNType::Good);
  (void)room;

  std::vector<std::array<double, 8>> fig;
  CHECK(sperr::quality_fields_dev(original, &narrow, target, &wide, nf, dims, fig) == sperr::RTNType::Error);
  CHECK(sperr::quality_fields_dev(original, nullptr, target, &wide, nf, dims, fig) == sperr::RTNType::Good);
  CHECK(fig.size() == nf);
  std::vector<std::array<double, 8>> self;
  CHECK(sperr::quality_fields_dev(target, &wide, target, &wide, nf, dims, self) == sperr::RTNType::Good);
  for (size_t f = 0; f < nf; f++)
    CHECK(self[f][0] == 0.0 && self[f][1] == 0.0 && self[f][2] > 1e300 && self[f][7] == 0.0);

  CHECK(hipMemcpy(parent.data(), d_parent, parentLen * 4, hipMemcpyDeviceToHost) == hipSuccess);
  const std::vector<uint64_t> offs64(offsets.begin(), offsets.end());
  CHECK(write_file(argv[5], streams.data(), streams.size()) && write_file(argv[6], offs64.data(), offs64.size() * 8) &&
        write_file(argv[7], parent.data(), parentLen * 4) && write_file(argv[8], fig.data(), fig.size() * 64));
  CHECK(hipFree(d_orig) == hipSuccess && hipFree(d_parent) == hipSuccess && hipFree(d_streams) == hipSuccess &&
        hipFree(d_again) == hipSuccess);
  return 0;
}
