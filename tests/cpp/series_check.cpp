// series_check.cpp -- sperr_amd/csrc/series.h as host C++, a program of its own (tests/test_series_host.py builds it under
// -fsanitize=address,undefined and compares every figure it prints with tests/series_model.py, bit for bit).
//   series_check                              checks of its own; prints "series_check ok"
//   series_check plan N L                     "start l" of every group
//   series_check needs N L                    one line per (t0, nt), nt fastest: the need bytes as 0/1
//   series_check tol TOLBITS MBITS L          "ok rho tau_0 .. tau_L" as bit patterns, or "refused"
//   series_check butterfly l IN OUT           IN: 2^l rows of m doubles; OUT: the forward of every column, then the
//                                             inverse of that
//   series_check info N L X Y Z F KIND QBITS RBITS MBITS RHOBITS     the record in hex, and its fields parsed back
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "series.h"

using namespace sperrhip;

static int fail(const char* what)
{
  printf("FAILED %s\n", what);
  return 1;
}

static int self_checks()
{
  for (int L = 0; L <= kSeriesMaxLevels; L++)
    for (size_t n = 1; n <= 70; n++) {
      const size_t ng = series_group_count(n, L);
      size_t at = 0;
      for (size_t i = 0; i < ng; i++) {
        size_t start, s2;
        int l, l2;
        series_group(n, L, i, &start, &l);
        if (start != at || l > L)
          return fail("plan");
        for (size_t t = start; t < start + ((size_t)1 << l); t++) {
          series_group_of(n, L, t, &s2, &l2);
          if (s2 != start || l2 != l)
            return fail("group_of");
        }
        // the slots' covers: every level tiles the group
        std::vector<int> hits((size_t)1 << l, 0);
        for (size_t slot = 1; slot < (size_t)1 << l; slot++) {
          size_t lo, hi;
          series_slot_cover(l, slot, &lo, &hi);
          if (hi <= lo || hi > (size_t)1 << l)
            return fail("cover");
          for (size_t t = lo; t < hi; t++)
            hits[t]++;
        }
        for (int h : hits)
          if (h != l)
            return fail("cover count");
        at = start + ((size_t)1 << l);
      }
      if (at != n)
        return fail("plan end");
      std::vector<uint8_t> need(n);
      if (series_needs(n, L, n, 1, need.data()) || series_needs(n, L, 0, n + 1, need.data()) ||
          series_needs(n, L, 0, 0, need.data()) || !series_needs(n, L, 0, n, need.data()))
        return fail("needs range");
      for (uint8_t b : need)
        if (!b)
          return fail("needs all");
    }
  double rho, tau[kSeriesMaxLevels + 1];
  if (series_tolerance(0.0, 1.0, 3, &rho, tau) || series_tolerance(1e-3, -1.0, 3, &rho, tau) ||
      series_tolerance(1e-3, 1.0, 5, &rho, tau) || series_tolerance(NAN, 1.0, 3, &rho, tau) ||
      series_tolerance(1e-3, INFINITY, 3, &rho, tau) || !series_tolerance(1e-3, 1.0, 0, &rho, tau) || rho != 0.0 ||
      tau[0] != 1e-3)
    return fail("tolerance");
  uint8_t rec[kSeriesInfoBytes];
  SeriesInfo h{3, 1, kSeriesKindTol, 11, {20, 18, 16}, 1e-4, 2.0, 1.5, 7e-15}, g;
  series_write_info(h, rec);
  if (!series_parse_info(rec, &g) || g.n != 11 || g.dims[2] != 16 || g.rho != 7e-15)
    return fail("info");
  rec[0] = 'X';
  if (series_parse_info(rec, &g))
    return fail("info magic");
  rec[0] = 'S';
  rec[5] = 5;
  if (series_parse_info(rec, &g))
    return fail("info levels");
  printf("series_check ok\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 1)
    return self_checks();
  const std::string cmd = argv[1];
  if (cmd == "plan" && argc == 4) {
    const size_t n = strtoull(argv[2], nullptr, 10);
    const int L = atoi(argv[3]);
    for (size_t i = 0; i < series_group_count(n, L); i++) {
      size_t start;
      int l;
      series_group(n, L, i, &start, &l);
      printf("%zu %d\n", start, l);
    }
    return 0;
  }
  if (cmd == "needs" && argc == 4) {
    const size_t n = strtoull(argv[2], nullptr, 10);
    const int L = atoi(argv[3]);
    std::vector<uint8_t> need(n);
    for (size_t t0 = 0; t0 < n; t0++)
      for (size_t nt = 1; nt <= n - t0; nt++) {
        if (!series_needs(n, L, t0, nt, need.data()))
          return fail("needs");
        for (size_t b = 0; b < n; b++)
          putchar(need[b] ? '1' : '0');
        putchar('\n');
      }
    return 0;
  }
  if (cmd == "tol" && argc == 5) {
    double rho, tau[kSeriesMaxLevels + 1];
    const int L = atoi(argv[4]);
    if (!series_tolerance(series_double(strtoull(argv[2], nullptr, 10)), series_double(strtoull(argv[3], nullptr, 10)), L,
                          &rho, tau)) {
      printf("refused\n");
      return 0;
    }
    printf("ok %llu", (unsigned long long)series_bits(rho));
    for (int l = 0; l <= L; l++)
      printf(" %llu", (unsigned long long)series_bits(tau[l]));
    printf("\n");
    return 0;
  }
  if (cmd == "butterfly" && argc == 5) {
    const int l = atoi(argv[2]);
    const size_t g = (size_t)1 << l;
    FILE* f = fopen(argv[3], "rb");
    if (!f)
      return fail("open");
    std::vector<double> in;
    double buf[4096];
    for (size_t got; (got = fread(buf, 8, 4096, f)) > 0;)
      in.insert(in.end(), buf, buf + got);
    fclose(f);
    if (in.empty() || in.size() % g != 0)
      return fail("size");
    const size_t m = in.size() / g;
    std::vector<double> fwd(in.size()), inv(in.size());
    for (size_t c = 0; c < m; c++) {
      double v[kSeriesMaxGroup];
      for (size_t t = 0; t < g; t++)
        v[t] = in[t * m + c];
      series_forward_l(l, v);
      for (size_t t = 0; t < g; t++)
        fwd[t * m + c] = v[t];
      series_inverse_l(l, v);
      for (size_t t = 0; t < g; t++)
        inv[t * m + c] = v[t];
    }
    FILE* o = fopen(argv[4], "wb");
    if (!o || fwrite(fwd.data(), 8, fwd.size(), o) != fwd.size() || fwrite(inv.data(), 8, inv.size(), o) != inv.size())
      return fail("write");
    fclose(o);
    return 0;
  }
  if (cmd == "info" && argc == 13) {
    SeriesInfo h{atoi(argv[3]), atoi(argv[7]), atoi(argv[8]), strtoull(argv[2], nullptr, 10),
                 {strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10), strtoull(argv[6], nullptr, 10)},
                 series_double(strtoull(argv[9], nullptr, 10)), series_double(strtoull(argv[10], nullptr, 10)),
                 series_double(strtoull(argv[11], nullptr, 10)), series_double(strtoull(argv[12], nullptr, 10))};
    uint8_t rec[kSeriesInfoBytes];
    series_write_info(h, rec);
    for (size_t i = 0; i < kSeriesInfoBytes; i++)
      printf("%02x", rec[i]);
    SeriesInfo g;
    printf("\n%d\n", series_parse_info(rec, &g) ? 1 : 0);
    return 0;
  }
  return fail("usage");
}
