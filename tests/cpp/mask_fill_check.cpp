// Host check of sperr_amd/csrc/mask_fill.h, the smooth in-fill of missing values: the rule as the header's plain loops
// on volumes read from files, the levels and the pyramid's byte count, the P / Q index rule at both ends of odd and even
// dims, the fill kinds and the caller's value, and the refusal of a sum that is not finite.
//   mask_fill_check                                               runs the checks, prints "mask_fill_check ok"
//   mask_fill_check plan <dimx> <dimy> <dimz>                     prints "L G bytes ldsCells" and a line "x y z" per level
//   mask_fill_check fill <f32|f64> <dimx> <dimy> <dimz> <volume> <bits> <out>
//                                                                 <bits>: n bytes of 0 / 1; writes the in-filled volume,
//                                                                 or prints "refused" and writes nothing
// Built with the address and undefined sanitizers by tests/test_mask_fill_host.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <string_view>
#include <vector>

#include "mask_fill.h"

using namespace sperrhip;

#define CHECK(cond)                                           \
  do {                                                        \
    if (!(cond)) {                                            \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      return 1;                                               \
    }                                                         \
  } while (0)

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

static int plan_mode(char** argv)
{
  MaskFillPlan p;
  CHECK(mask_fill_plan(std::stoull(argv[2]), std::stoull(argv[3]), std::stoull(argv[4]), &p));
  std::printf("%u %u %zu %llu\n", p.L, p.G, p.bytes, (unsigned long long)p.ldsCells);
  for (uint32_t l = 0; l <= p.L; l++)
    std::printf("%llu %llu %llu\n", (unsigned long long)p.dim[l][0], (unsigned long long)p.dim[l][1],
                (unsigned long long)p.dim[l][2]);
  return 0;
}

template <typename T>
static int fill_typed(const MaskFillPlan& p, const std::vector<uint8_t>& raw, const std::vector<uint8_t>& bits,
                      const char* out_path)
{
  const size_t n = (size_t)p.cells[0];
  CHECK(raw.size() == n * sizeof(T) && bits.size() == n);
  std::vector<T> src(n), dst(n);
  std::memcpy(src.data(), raw.data(), raw.size());
  std::vector<double> work((size_t)mask_fill_host_cells(p) + 1);
  if (!mask_fill_smooth_host(src.data(), bits.data(), p, work.data(), dst.data())) {
    std::printf("refused\n");
    return 0;
  }
  // in place gives the same bytes
  std::vector<T> inplace = src;
  CHECK(mask_fill_smooth_host(inplace.data(), bits.data(), p, work.data(), inplace.data()));
  CHECK(std::memcmp(inplace.data(), dst.data(), n * sizeof(T)) == 0);
  std::FILE* o = std::fopen(out_path, "wb");
  CHECK(o && std::fwrite(dst.data(), sizeof(T), n, o) == n && std::fclose(o) == 0);
  return 0;
}

static int fill_mode(char** argv)
{
  const bool is_float = std::string_view(argv[2]) == "f32";
  CHECK(is_float || std::string_view(argv[2]) == "f64");
  MaskFillPlan p;
  CHECK(mask_fill_plan(std::stoull(argv[3]), std::stoull(argv[4]), std::stoull(argv[5]), &p));
  std::vector<uint8_t> raw, bits;
  CHECK(read_file(argv[6], raw) && read_file(argv[7], bits));
  return is_float ? fill_typed<float>(p, raw, bits, argv[8]) : fill_typed<double>(p, raw, bits, argv[8]);
}

static int check_pq()
{
  uint64_t P = 9, Q = 9;
  // a coarser level of 4 cells under a finer one of 8 (even) and of 7 (odd)
  const uint64_t wantP[8] = {0, 0, 1, 1, 2, 2, 3, 3}, wantQ[8] = {0, 1, 0, 2, 1, 3, 2, 3};
  for (uint64_t i = 0; i < 8; i++) {
    mask_fill_pq<uint64_t>(i, 4, &P, &Q);
    CHECK(P == wantP[i] && Q == wantQ[i]);
  }
  // the odd dim's last coordinate is even: it looks back, not past the end
  mask_fill_pq<uint64_t>(6, 4, &P, &Q);
  CHECK(P == 3 && Q == 2);
  // a finer level of 5 over a coarser one of 3; of 2 over 1; of 1 over 1
  mask_fill_pq<uint64_t>(4, 3, &P, &Q);
  CHECK(P == 2 && Q == 1);
  mask_fill_pq<uint64_t>(3, 3, &P, &Q);
  CHECK(P == 1 && Q == 2);
  mask_fill_pq<uint64_t>(1, 1, &P, &Q);
  CHECK(P == 0 && Q == 0);
  mask_fill_pq<uint64_t>(0, 1, &P, &Q);
  CHECK(P == 0 && Q == 0);
  uint32_t p32 = 9, q32 = 9;
  mask_fill_pq<uint32_t>(7, 4, &p32, &q32);
  CHECK(p32 == 3 && q32 == 3);
  return 0;
}

static int check_plan()
{
  MaskFillPlan p;
  CHECK(!mask_fill_plan(0, 1, 1, &p) && !mask_fill_plan(SIZE_MAX, 2, 1, &p));
  CHECK(mask_fill_plan(1, 1, 1, &p) && p.L == 0 && p.G == 0 && p.bytes == 0);
  CHECK(mask_fill_plan(2, 2, 2, &p) && p.L == 1 && p.G == 1 && p.ldsCells == 0 && p.bytes == kMaskFillHeadBytes + 8);
  CHECK(mask_fill_plan(37, 44, 30, &p) && p.L == 6 && p.G == 1 && p.cells[1] == 19 * 22 * 15 &&
        p.bytes == kMaskFillHeadBytes + 8 * 6270 && p.dim[2][0] == 10 && p.dim[2][1] == 11 && p.dim[2][2] == 8);
  CHECK(mask_fill_plan(65, 66, 70, &p) && p.L == 7 && p.G == 2 && p.off[2] == p.cells[1] &&
        p.bytes == kMaskFillHeadBytes + 8 * (33 * 33 * 35 + 17 * 17 * 18));
  // the levels in LDS fit for the shapes that stress them: a line, a slab, a cube at the threshold
  const size_t shapes[][3] = {{1, 1, 70}, {1, 1, 4097}, {1, 1, 1000003}, {3, 3, 455}, {2049, 2, 1}, {128, 128, 128},
                              {129, 127, 255}, {4096, 1, 1}, {4097, 1, 1}};
  for (const auto& s : shapes) {
    CHECK(mask_fill_plan(s[0], s[1], s[2], &p));
    CHECK(p.ldsCells <= kMaskTopLdsCells && p.G >= 1 && p.G <= p.L);
    CHECK(p.cells[p.G] <= 8ull * kMaskTopCells);
    CHECK(p.G == p.L || p.cells[p.G + 1] <= kMaskTopCells);
    for (uint32_t l = 1; l < p.G; l++)
      CHECK(p.cells[l] > kMaskTopCells);
  }
  return 0;
}

static int check_kinds_and_value()
{
  CHECK(mask_fill_kind_ok(0) && mask_fill_kind_ok(1) && mask_fill_kind_ok(2) && !mask_fill_kind_ok(3) &&
        !mask_fill_kind_ok(-1));
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double stored = 0.0;
  CHECK(mask_fill_value_ok(3.5, true, &stored) && stored == 3.5);
  CHECK(mask_fill_value_ok(0.1, true, &stored) && stored == (double)0.1f);
  CHECK(mask_fill_value_ok(0.1, false, &stored) && stored == 0.1);
  CHECK(!mask_fill_value_ok(inf, false, &stored) && !mask_fill_value_ok(-inf, true, &stored) &&
        !mask_fill_value_ok(nan, false, &stored));
  CHECK(mask_fill_value_ok(1e39, false, &stored) && !mask_fill_value_ok(1e39, true, &stored));
  CHECK(!mask_fill_known(mask_fill_unknown()) && mask_fill_known(0.0) && mask_fill_known(inf));
  return 0;
}

static int check_refusal_and_small()
{
  MaskFillPlan p;
  // two adjacent valid samples of 1.7e308: their sum is not finite
  CHECK(mask_fill_plan(4, 1, 1, &p));
  const double big[4] = {1.7e308, 1.7e308, 0.0, 0.0};
  const uint8_t bits[4] = {0, 0, 1, 1};
  double out[4] = {7.0, 7.0, 7.0, 7.0}, work[8];
  CHECK(!mask_fill_smooth_host(big, bits, p, work, out));
  CHECK(out[0] == 7.0 && out[3] == 7.0);
  // ... in cells of their own they meet one level up, and fail there
  const double apart[4] = {1.7e308, 0.0, 1.7e308, 0.0};
  const uint8_t bits2[4] = {0, 1, 0, 1};
  CHECK(!mask_fill_smooth_host(apart, bits2, p, work, out) && out[0] == 7.0);
  // ... and one of them with small neighbours is fine
  const double alone[4] = {1.7e308, 0.0, 5.0, 0.0};
  CHECK(mask_fill_smooth_host(alone, bits2, p, work, out) && out[0] == 1.7e308 && out[2] == 5.0);
  // one sample: L = 0, the fill is 0.0
  CHECK(mask_fill_plan(1, 1, 1, &p));
  const float one = 5.0f;
  float got = 1.0f;
  const uint8_t miss = 1, valid = 0;
  CHECK(mask_fill_smooth_host(&one, &miss, p, work, &got) && got == 0.0f);
  CHECK(mask_fill_smooth_host(&one, &valid, p, work, &got) && got == 5.0f);
  // nothing valid: zeros; one valid sample: its value everywhere
  CHECK(mask_fill_plan(3, 2, 2, &p));
  float v[12], o[12];
  uint8_t b[12];
  double w2[16];
  for (int i = 0; i < 12; i++) {
    v[i] = 1.0f + (float)i;
    b[i] = 1;
  }
  CHECK(mask_fill_smooth_host(v, b, p, w2, o));
  for (int i = 0; i < 12; i++)
    CHECK(o[i] == 0.0f);
  b[7] = 0;
  CHECK(mask_fill_smooth_host(v, b, p, w2, o));
  for (int i = 0; i < 12; i++)
    CHECK(o[i] == 8.0f);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 5 && std::string_view(argv[1]) == "plan")
    return plan_mode(argv);
  if (argc == 9 && std::string_view(argv[1]) == "fill")
    return fill_mode(argv);
  if (argc != 1)
    return 2;
  static_assert(kMaskTopLdsCells >= 2 * kMaskTopCells + 64, "the levels above the first in LDS fit beside it");
  static_assert(kMaskTopLdsCells * sizeof(double) + 64 <= 64 * 1024, "static LDS of one workgroup");
  if (check_pq() || check_plan() || check_kinds_and_value() || check_refusal_and_small())
    return 1;
  std::printf("mask_fill_check ok\n");
  return 0;
}
