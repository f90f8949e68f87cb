// Drives the portion methods of the C++ mirror (include/sperr_hip.hpp) the way code written against the reference's
// classes would -- SPERR3D_OMP_D::decompress_portion and the trailing pct of decompress_box / decompress_level,
// SPERR3D_Stream_Tools::progressive_truncate_dev -- and dumps what they give; tests/test_cpp_portion.py compares
// the files with the oracle's results.
//   usage: portion_check <container> <pct> <out prefix>
//   writes <prefix>.whole.f64, .box.f64 (the box 5 7 9 + 40 30 21), .level.f64 (level 0), .trunc (the truncated
//   container, made in device memory)
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <string>

#include "sperr_hip.hpp"

#define CHECK(cond)                                              \
  if (!(cond)) {                                                 \
    std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
    return 1;                                                    \
  }

static bool dump(const std::string& name, const void* p, size_t bytes)
{
  std::FILE* o = std::fopen(name.c_str(), "wb");
  if (!o)
    return false;
  const bool ok = std::fwrite(p, 1, bytes, o) == bytes;
  return std::fclose(o) == 0 && ok;
}

int main(int argc, char** argv)
{
  if (argc != 4)
    return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f);
  sperr::vec8_type stream;
  for (int c; (c = std::fgetc(f)) != EOF;)
    stream.push_back((uint8_t)c);
  std::fclose(f);
  const unsigned pct = (unsigned)std::stoul(argv[2]);
  const std::string prefix = argv[3];
  const sperr::dims_type lo{5, 7, 9}, dims{40, 30, 21};

  sperr::SPERR3D_OMP_D d;
  CHECK(d.use_bitstream(stream.data(), stream.size()) == sperr::RTNType::Good);
  // refusals, as the C calls refuse: another pointer, a box that leaves the volume, a level that is not there
  const sperr::vec8_type copy = stream;
  CHECK(d.decompress_portion(copy.data(), pct) == sperr::RTNType::Error);
  CHECK(d.decompress_box(stream.data(), {60, 0, 0}, {5, 1, 1}, pct) == sperr::RTNType::Error);
  CHECK(d.decompress_level(stream.data(), 16, pct) == sperr::RTNType::Error);

  CHECK(d.decompress_portion(stream.data(), pct) == sperr::RTNType::Good);
  const sperr::vecd_type whole = d.view_decoded_data();
  CHECK(whole.size() == d.get_dims()[0] * d.get_dims()[1] * d.get_dims()[2]);
  CHECK(dump(prefix + ".whole.f64", whole.data(), whole.size() * 8));
  CHECK(d.decompress_box(stream.data(), lo, dims, pct) == sperr::RTNType::Good);
  CHECK(d.view_decoded_data().size() == dims[0] * dims[1] * dims[2]);
  CHECK(dump(prefix + ".box.f64", d.view_decoded_data().data(), d.view_decoded_data().size() * 8));
  CHECK(d.decompress_level(stream.data(), 0, pct) == sperr::RTNType::Good);
  CHECK(d.view_hierarchy().empty());
  const sperr::vecd_type level = d.view_decoded_data();
  CHECK(dump(prefix + ".level.f64", level.data(), level.size() * 8));
  CHECK(d.decompress_level(stream.data(), 0, {1, 0, 1}, {2, 3, 1}, pct) == sperr::RTNType::Good);
  CHECK(d.view_decoded_data().size() == 6);
  // the whole streams: pct 0 takes the calls that were there before, 100 the portion call; both are the plain decode
  CHECK(d.decompress(stream.data()) == sperr::RTNType::Good);
  const sperr::vecd_type plain = d.view_decoded_data();
  CHECK(plain != whole);
  CHECK(d.decompress_portion(stream.data(), 100) == sperr::RTNType::Good && d.view_decoded_data() == plain);
  CHECK(d.decompress_portion(stream.data(), 0) == sperr::RTNType::Good && d.view_decoded_data() == plain);

  // truncating in device memory, then decoding what it made: the portion again
  sperr::SPERR3D_Stream_Tools tools;
  void *d_in = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_in, stream.size()) == hipSuccess && hipMalloc(&d_out, stream.size()) == hipSuccess);
  CHECK(hipMemcpy(d_in, stream.data(), stream.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(tools.progressive_truncate_dev(d_in, stream.size(), pct, d_out, 20) == 0);
  CHECK(tools.progressive_truncate_dev(d_in, stream.size() - 1, pct, d_out, stream.size()) == 0);
  const size_t len = tools.progressive_truncate_dev(d_in, stream.size(), pct, d_out, stream.size());
  CHECK(len > 0 && len < stream.size());
  sperr::vec8_type cut(len);
  CHECK(hipMemcpy(cut.data(), d_out, len, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(cut == tools.progressive_truncate(stream.data(), stream.size(), pct));
  CHECK(tools.get_stream_header(cut.data()).is_portion);
  CHECK(dump(prefix + ".trunc", cut.data(), cut.size()));
  sperr::SPERR3D_OMP_D e;
  CHECK(e.use_bitstream(cut.data(), cut.size()) == sperr::RTNType::Good);
  CHECK(e.decompress(cut.data()) == sperr::RTNType::Good && e.view_decoded_data() == whole);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return 0;
}
