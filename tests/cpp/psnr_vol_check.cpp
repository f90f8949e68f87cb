// psnr_vol_check.cpp -- sperr_amd/csrc/psnr_vol.h as host C++ (tests/test_psnr_vol_host.py builds it with
// -fsanitize=address,undefined): the table, the estimates, the pick and the width rule of a chunk's coefficients read
// from a file, printed as bit patterns for the test to compare with tests/psnr_vol_model.py; and, without arguments,
// the header's small parts against plain statements.
//
//   psnr_vol_check COEFFS RANGE_BITS PSNR     COEFFS: doubles, native endian; RANGE_BITS: the range's bit pattern
//       "ladder <ok> t <bits> q <bits> x 5"
//       "mse <bits> x 5"                      every rung's estimate, taken stride sum by stride sum as the kernels do
//       "pick <rung or -1> width <0 | 1 | -1> maxabs <bits>"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "psnr_vol.h"

using namespace sperrhip;

static uint64_t bits(double v)
{
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

static int fail(const char* what)
{
  printf("psnr_vol_check FAILED: %s\n", what);
  return 1;
}

static int self_check()
{
  PsnrLadder L;
  if (!psnr_vol_ladder(2.0, 60.0, &L) || L.t != (2.0 * 2.0) * pow(10.0, -6.0) || L.q[0] != 2.0 * sqrt(L.t * 3.0))
    return fail("ladder");
  for (int k = 1; k < kPsnrRungs; k++)
    if (L.q[k] != L.q[k - 1] / exp2(0.25))
      return fail("ladder step");
  // the bound: four steps halve q, so the fifth rung's q^2 / 4 is 0.75 t
  if (fabs(L.q[4] / (L.q[0] / 2.0) - 1.0) > 1e-15 || L.q[4] * L.q[4] / 4.0 > 0.7500001 * L.t)
    return fail("five-rung bound");
  if (psnr_vol_ladder(0.0, 60.0, &L) || psnr_vol_ladder(1.0, 7000.0, &L) || psnr_vol_ladder(INFINITY, 60.0, &L) ||
      psnr_vol_ladder(1e200, -3000.0, &L))
    return fail("ladder refusals");
  const double a[kPsnrRungs] = {3.0, 2.0, 1.0, 0.5, 0.25}, nan5[kPsnrRungs] = {NAN, NAN, NAN, NAN, NAN};
  if (psnr_vol_pick(a, 1.0) != 2 || psnr_vol_pick(a, 3.0) != 0 || psnr_vol_pick(a, 0.25) != 4 || psnr_vol_pick(a, 0.2) != -1 ||
      psnr_vol_pick(nan5, 1.0) != -1)
    return fail("pick");
  if (psnr_vol_width(4294967295.4, 1.0) != 0 || psnr_vol_width(4294967295.6, 1.0) != 1 || psnr_vol_width(0x1p63, 1.0) != -1 ||
      psnr_vol_width(nextafter(0x1p63, 0.0), 1.0) != 1 || psnr_vol_width(NAN, 1.0) != -1 || psnr_vol_width(0.0, 1.0) != 0 ||
      psnr_vol_width(1.0, 0.0) != -1)
    return fail("width");
  if (psnr_vol_strides(0) != 1 || psnr_vol_strides(4095) != 1 || psnr_vol_strides(4096) != 2 || psnr_vol_strides(262144) != 65)
    return fail("strides");
  // the estimate of short arrays, by hand: an empty last stride adds nothing
  std::vector<double> v(4096, 1.0);
  const double q = 4.0;   // rint(0.25) = 0: every term is 1
  if (psnr_vol_estimate(v.data(), v.size(), q) != 1.0)
    return fail("estimate");
  v.push_back(3.0);       // rint(0.75) = 1: diff = -1
  if (psnr_vol_estimate(v.data(), v.size(), q) != 4097.0 / 4097.0)
    return fail("estimate, short last stride");
  printf("psnr_vol_check ok\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 1)
    return self_check();
  if (argc != 4)
    return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return fail("cannot open the coefficients");
  std::vector<double> v;
  double buf[4096];
  for (size_t n; (n = fread(buf, 8, 4096, f)) > 0;)
    v.insert(v.end(), buf, buf + n);
  fclose(f);
  if (v.empty())
    return fail("no coefficients");
  const uint64_t rb = strtoull(argv[2], nullptr, 10);
  double range;
  memcpy(&range, &rb, 8);
  const double psnr = strtod(argv[3], nullptr);
  PsnrLadder L;
  const bool ok = psnr_vol_ladder(range, psnr, &L);
  printf("ladder %d t %" PRIu64 " q", ok ? 1 : 0, bits(L.t));
  for (int k = 0; k < kPsnrRungs; k++)
    printf(" %" PRIu64, bits(L.q[k]));
  printf("\n");
  // as the kernels: every stride's sum of every rung in one pass, then the sums in order
  const uint32_t ns = psnr_vol_strides(v.size());
  std::vector<double> part((size_t)kPsnrRungs * ns, 0.0);
  double maxabs = 0.0;
  for (uint32_t s = 0; s < ns; s++) {
    double acc[kPsnrRungs] = {0, 0, 0, 0, 0};
    const size_t beg = (size_t)s * kPsnrStride, end = beg + kPsnrStride < v.size() ? beg + kPsnrStride : v.size();
    for (size_t i = beg; i < end; i++) {
      maxabs = fmax(maxabs, fabs(v[i]));
      for (int k = 0; k < kPsnrRungs; k++)
        acc[k] = psnr_vol_term(acc[k], v[i], L.q[k], 1.0 / L.q[k]);
    }
    for (int k = 0; k < kPsnrRungs; k++)
      part[(size_t)k * ns + s] = acc[k];
  }
  double mse[kPsnrRungs];
  printf("mse");
  for (int k = 0; k < kPsnrRungs; k++) {
    mse[k] = psnr_vol_total(part.data() + (size_t)k * ns, ns, v.size());
    if (mse[k] != psnr_vol_estimate(v.data(), v.size(), L.q[k]) && mse[k] == mse[k])
      return fail("the two walks of the estimate differ");
    printf(" %" PRIu64, bits(mse[k]));
  }
  printf("\n");
  const int rung = psnr_vol_pick(mse, L.t);
  printf("pick %d width %d maxabs %" PRIu64 "\n", rung, rung < 0 ? -1 : psnr_vol_width(maxabs, L.q[rung]), bits(maxabs));
  return 0;
}
