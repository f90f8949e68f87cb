// Drives SPERR3D_OMP_D::decompress_level (include/sperr_hip.hpp) the way code written against the
// reference's classes would, and dumps the level -- or the box of it -- as doubles; tests/test_cpp_level.py
// compares it with the oracle's hierarchy.
//   usage: level_check <container> <level> <out.f64>
//          level_check <container> <level> <lo x> <lo y> <lo z> <dims x> <dims y> <dims z> <out.f64>
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
  if (argc != 4 && argc != 10)
    return 2;
  const bool boxed = argc == 10;
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f);
  sperr::vec8_type stream;
  for (int c; (c = std::fgetc(f)) != EOF;)
    stream.push_back((uint8_t)c);
  std::fclose(f);
  const size_t level = std::stoul(argv[2]);
  sperr::dims_type lo{0, 0, 0}, dims{0, 0, 0};
  if (boxed) {
    lo = {std::stoul(argv[3]), std::stoul(argv[4]), std::stoul(argv[5])};
    dims = {std::stoul(argv[6]), std::stoul(argv[7]), std::stoul(argv[8])};
  }
  auto run = [&](sperr::SPERR3D_OMP_D& d) {
    return boxed ? d.decompress_level(stream.data(), level, lo, dims) : d.decompress_level(stream.data(), level);
  };

  sperr::SPERR3D_OMP_D d;
  CHECK(d.use_bitstream(stream.data(), stream.size()) == sperr::RTNType::Good);
  // refusals: another pointer, a level the container does not have, an empty box
  const sperr::vec8_type copy = stream;
  CHECK(d.decompress_level(copy.data(), level) == sperr::RTNType::Error);
  CHECK(d.decompress_level(stream.data(), 16) == sperr::RTNType::Error);
  CHECK(d.decompress_level(stream.data(), level, {0, 0, 0}, {0, 1, 1}) == sperr::RTNType::Error);
  // the level, then the whole hierarchy, then the level again: each call replaces the decoded data
  CHECK(run(d) == sperr::RTNType::Good);
  const sperr::vecd_type got = d.view_decoded_data();
  CHECK(d.view_hierarchy().empty());
  if (boxed)
    CHECK(got.size() == dims[0] * dims[1] * dims[2]);
  CHECK(d.decompress(stream.data(), true) == sperr::RTNType::Good);
  CHECK(level < d.view_hierarchy().size());
  if (!boxed)
    CHECK(d.view_hierarchy()[level] == got);
  CHECK(run(d) == sperr::RTNType::Good);
  CHECK(d.view_decoded_data() == got);

  std::FILE* o = std::fopen(argv[argc - 1], "wb");
  CHECK(o && std::fwrite(got.data(), 8, got.size(), o) == got.size());
  CHECK(std::fclose(o) == 0);
  return 0;
}
