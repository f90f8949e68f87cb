// Drives SPERR3D_OMP_D::decompress_box (include/sperr_hip.hpp) the way code written against the
// reference's classes would, and dumps the box as doubles; tests/test_cpp_box.py compares it with the
// oracle's whole decode, cut to the box.
//   usage: box_check <container> <lo x> <lo y> <lo z> <dims x> <dims y> <dims z> <out.f64>
#include <cstdio>
#include <string>

#include "sperr_hip.hpp"

#define CHECK(cond)                                              \
  if (!(cond)) {                                                 \
    std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
    return 1;                                                    \
  }

int main(int argc, char** argv)
{
  if (argc != 9)
    return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f);
  sperr::vec8_type stream;
  for (int c; (c = std::fgetc(f)) != EOF;)
    stream.push_back((uint8_t)c);
  std::fclose(f);
  const sperr::dims_type lo{std::stoul(argv[2]), std::stoul(argv[3]), std::stoul(argv[4])};
  const sperr::dims_type dims{std::stoul(argv[5]), std::stoul(argv[6]), std::stoul(argv[7])};

  sperr::SPERR3D_OMP_D d;
  CHECK(d.use_bitstream(stream.data(), stream.size()) == sperr::RTNType::Good);
  // refusals: another pointer, an empty box, a box that leaves the volume
  const sperr::vec8_type copy = stream;
  CHECK(d.decompress_box(copy.data(), lo, dims) == sperr::RTNType::Error);
  CHECK(d.decompress_box(stream.data(), lo, {0, 1, 1}) == sperr::RTNType::Error);
  const auto vd = d.get_dims();
  CHECK(d.decompress_box(stream.data(), {vd[0], 0, 0}, {1, 1, 1}) == sperr::RTNType::Error);
  // the box, then the whole volume, then the box again: each call replaces the decoded data
  CHECK(d.decompress_box(stream.data(), lo, dims) == sperr::RTNType::Good);
  const sperr::vecd_type box = d.view_decoded_data();
  CHECK(box.size() == dims[0] * dims[1] * dims[2]);
  CHECK(d.decompress(stream.data()) == sperr::RTNType::Good);
  CHECK(d.view_decoded_data().size() == vd[0] * vd[1] * vd[2]);
  CHECK(d.decompress_box(stream.data(), lo, dims) == sperr::RTNType::Good);
  CHECK(d.view_decoded_data() == box);

  std::FILE* o = std::fopen(argv[8], "wb");
  CHECK(o && std::fwrite(box.data(), 8, box.size(), o) == box.size());
  CHECK(std::fclose(o) == 0);
  return 0;
}
