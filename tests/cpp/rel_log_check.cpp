// Host check of the LOG map kind of sperr_amd/csrc/rel.h: rel_log2 and rel_exp2, the tolerance of this kind with its
// floor and refusals, the forward map and the inverse with the clamp's two ends, the side stream "SPLG" with every
// refusal its parser shares with "SPRL", and an eps that only this kind's rule accepts.
//   rel_log_check                                        runs the checks, prints "rel_log_check ok"
//   rel_log_check tolerance <eps as %a> <is_float>       prints t as %a, or "refused"
//   rel_log_check forward <f32|f64> <eps as %a> <in> <y> <side>   <in>: raw samples; writes y (doubles) and the stream
//   rel_log_check inverse <f32|f64> <y> <side> <out>     y' and a side stream OF EITHER KIND into x' of the named type
// Built with the address and undefined sanitizers by tests/test_rel_log_host.py; no GPU, no HIP.
//
// The SPMK stream writer and reader and the file helpers are rel_check.cpp's, taken in whole with its main() renamed
// (and not called: tests/test_rel_host.py runs that program).
#define main rel_check_main
#include "rel_check.cpp"
#undef main

template <typename T>
static bool log_forward_all(const std::vector<T>& x, double eps, std::vector<double>& y, std::vector<uint8_t>& side)
{
  const size_t n = x.size();
  std::vector<uint8_t> zero(n), neg(n);
  y.resize(n);
  for (size_t i = 0; i < n; i++) {
    RelClass c;
    y[i] = rel_forward<kRelLog>(x[i], &c);
    if (!c.finite)
      return false;
    zero[i] = c.zero;
    neg[i] = c.neg;
  }
  const std::vector<uint8_t> zs = mask_stream_of(zero), ss = mask_stream_of(neg);
  const RelHeader h{sizeof(T) == 4, eps, n, zs.size(), ss.size(), kRelLog};
  side.assign((size_t)rel_stream_bytes(h), 0);
  rel_write_header(h, side.data());
  memcpy(side.data() + kRelHeaderBytes, zs.data(), zs.size());
  memcpy(side.data() + rel_sign_offset(h), ss.data(), ss.size());
  return true;
}

template <typename T>
static int log_forward_files(double eps, char** a)
{
  const std::vector<T> x = read_file<T>(a[0]);
  std::vector<double> y;
  std::vector<uint8_t> side;
  if (x.empty() || !log_forward_all(x, eps, y, side)) {
    std::printf("refused\n");
    return 3;
  }
  return write_file(a[1], y) && write_file(a[2], side) ? 0 : 2;
}

template <typename OT>
static int kind_inverse_files(char** a)
{
  const std::vector<double> y = read_file<double>(a[0]);
  const std::vector<uint8_t> side = read_file<uint8_t>(a[1]);
  RelHeader h;
  std::vector<uint8_t> zero, neg;
  if (!side_bits(side, h, zero, neg) || h.n != y.size()) {
    std::printf("refused\n");
    return 3;
  }
  std::vector<OT> out(y.size());
  for (size_t i = 0; i < y.size(); i++)
    out[i] = h.kind == kRelLog ? rel_inverse<OT, kRelLog>(y[i], zero[i] != 0, neg[i] != 0, h.is_float != 0)
                               : rel_inverse<OT>(y[i], zero[i] != 0, neg[i] != 0, h.is_float != 0);
  return write_file(a[2], out) ? 0 : 2;
}

static int log_self_check()
{
  // (no comma of a template argument list inside CHECK)
  auto inv_f = [](double yp, bool zero, bool neg, bool src_float) { return rel_inverse<float, kRelLog>(yp, zero, neg, src_float); };
  auto inv_d = [](double yp, bool zero, bool neg, bool src_float) { return rel_inverse<double, kRelLog>(yp, zero, neg, src_float); };
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double dmax = std::numeric_limits<double>::max();
  const float fmax = std::numeric_limits<float>::max();
  double t = 0.0;
  // the two maps: powers of two exactly, both ways; the ends of the clamp
  for (int e = -1022; e <= 1023; e++) {
    CHECK(rel_log2(ldexp(1.0, e)) == (double)e);
    CHECK(rel_exp2((double)e) == ldexp(1.0, e));
  }
  CHECK(rel_log2(0x1.6a09e667f3bcdp+0) > 0.5 - 0x1p-50 && rel_log2(0x1.6a09e667f3bcdp+0) < 0.5 + 0x1p-50);
  CHECK(rel_log2(0x1.6a09e667f3bccp+0) > 0.5 - 0x1p-50 && rel_log2(0x1.6a09e667f3bccp+0) < 0.5 + 0x1p-50);
  CHECK(fabs(rel_log2(dmax) - 1024.0) <= 0x1p-43 && fabs(rel_log2(3.0) - 0x1.95c01a39fbd68p+0) <= 0x1p-51);
  CHECK(rel_exp2(kRelYMax) <= dmax && rel_exp2(kRelYMax) > 0x1p1023 && rel_exp2(nextafter(kRelYMax, 0.0)) <= rel_exp2(kRelYMax));
  CHECK(rel_exp2(kRelYMin) == 0.0 && rel_exp2(-1074.0) == 0x1p-1074 && rel_exp2(-1075.5) == 0.0);
  CHECK(fabs(rel_exp2(0.5) - 0x1.6a09e667f3bcdp+0) <= 0x1p-51 && fabs(rel_exp2(-0.5) - 0x1.6a09e667f3bcdp-1) <= 0x1p-52);
  // the tolerance: as written, every refusal, an unknown kind, the linear kind as it was
  CHECK(rel_tolerance(1e-2, true, &t, kRelLog) && t == rel_log2(1.0 + 1e-2) - 0x1p-22);
  CHECK(rel_tolerance(1e-2, false, &t, kRelLog) && t == rel_log2(1.0 + 1e-2) - 0x1p-40);
  CHECK(rel_tolerance(0.5, true, &t, kRelLog) && t == rel_log2(1.5) - 0x1p-22 && t > 0.58 && t < 0.585);
  CHECK(!rel_tolerance(nextafter(0.5, 1.0), true, &t, kRelLog) && !rel_tolerance(inf, true, &t, kRelLog) &&
        !rel_tolerance(nan, false, &t, kRelLog) && !rel_tolerance(0.0, true, &t, kRelLog) &&
        !rel_tolerance(-0.0, true, &t, kRelLog) && !rel_tolerance(-1e-2, false, &t, kRelLog) &&
        !rel_tolerance(-1.0, true, &t, kRelLog) && !rel_tolerance(-2.0, true, &t, kRelLog) &&
        !rel_tolerance(-inf, true, &t, kRelLog) && !rel_tolerance(0x1p-60, false, &t, kRelLog));
  CHECK(!rel_tolerance(1e-2, true, &t, 2) && !rel_tolerance(1e-2, true, &t, -1) && !rel_kind_ok(2) && rel_kind_ok(1));
  CHECK(rel_tolerance(1e-2, true, &t, kRelLinear) && t == 1e-2 / (1.0 + 1e-2) - 0x1p-22);
  CHECK(rel_tolerance(1e-2, true, &t) && t == 1e-2 / (1.0 + 1e-2) - 0x1p-22);
  // the floor: the first eps whose t reaches s, between 2 s ln 2 and 2 s: below the linear kind's
  double log_floor[2];
  for (int f = 0; f < 2; f++) {
    const double s = rel_slack(f != 0);
    uint64_t lo = rel_bits(s), hi = rel_bits(2.0 * s);
    CHECK(!rel_tolerance(rel_from_bits(lo), f != 0, &t, kRelLog) && rel_tolerance(rel_from_bits(hi), f != 0, &t, kRelLog));
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      (rel_tolerance(rel_from_bits(mid), f != 0, &t, kRelLog) ? hi : lo) = mid;
    }
    log_floor[f] = rel_from_bits(hi);
    CHECK(rel_tolerance(log_floor[f], f != 0, &t, kRelLog) && t >= s && !rel_tolerance(log_floor[f], f != 0, &t));
    CHECK(log_floor[f] > 2.0 * s * 0.693 && log_floor[f] < 2.0 * s * 0.6932);
  }
  // the classes and y
  RelClass c;
  CHECK(rel_bits(rel_forward<kRelLog>(0.0f, &c)) == kRelNanBits && c.zero && !c.neg && c.finite);
  CHECK(rel_bits(rel_forward<kRelLog>(-0x1p-1023, &c)) == kRelNanBits && c.zero && c.neg);
  CHECK(rel_forward<kRelLog>(0x1p-1022, &c) == -1022.0 && !c.zero);
  CHECK(rel_forward<kRelLog>(0x1p-149f, &c) == -172.0 && rel_forward<kRelLog>(0x1p-149, &c) == -149.0);
  CHECK(rel_forward<kRelLog>(0x1p-126f, &c) == -126.0 && rel_forward<kRelLog>(-4.0f, &c) == 2.0 && c.neg);
  {
    const double ylog = rel_forward<kRelLog>(-0x1.8p-148, &c), ysub = rel_forward<kRelLog>(-0x1.8p-148f, &c);
    CHECK(c.neg && ysub == -126.0 + 2.0 * (ylog + 126.0) && ylog > -147.5 && ylog < -147.4);
  }
  (void)rel_forward<kRelLog>(std::numeric_limits<float>::infinity(), &c);
  CHECK(!c.finite);
  (void)rel_forward<kRelLog>(nan, &c);
  CHECK(!c.finite);
  // the inverse: the clamp, the narrowing, the zeros
  CHECK(inv_d(1.0, false, true, false) == -2.0 && inv_f(-149.0, false, false, false) == 0x1p-149f);
  CHECK(inv_f(-172.0, false, false, true) == 0x1p-149f && inv_d(-128.0, false, false, true) == 0x1p-127);
  CHECK(inv_d(-2000.0, false, false, false) == 0.0 && inv_d(nan, false, true, false) == 0.0);
  CHECK(inv_d(5000.0, false, false, false) == rel_exp2(kRelYMax) &&
        inv_d(inf, false, false, false) == rel_exp2(kRelYMax));
  CHECK(inv_f(1000.0, false, false, false) == fmax && inv_f(128.0, false, true, false) == -fmax);
  CHECK(inv_f(rel_forward<kRelLog>(fmax, &c), false, false, true) == fmax);
  CHECK(rel_bits(inv_d(3.0, true, true, false)) == uint64_t(1) << 63);
  // the side stream of this kind: the round trip, and every refusal of the header that an SPRL stream has
  for (size_t n : {size_t(1), size_t(63), size_t(1024), size_t(1025), size_t(4913)}) {
    std::vector<float> x(n);
    for (size_t i = 0; i < n; i++)
      x[i] = i % 7 == 3 ? 0.0f : (i % 5 == 1 ? -1.0f : 1.0f) * (float)(i + 1) * 0x1p-140f;
    std::vector<double> y, ylin;
    std::vector<uint8_t> side, lin, zero, neg;
    CHECK(log_forward_all(x, 1e-2, y, side) && forward_all(x, 1e-2, ylin, lin) && side.size() == lin.size());
    CHECK(memcmp(side.data(), "SPLG", 4) == 0 && memcmp(lin.data(), "SPRL", 4) == 0 &&
          memcmp(side.data() + 4, lin.data() + 4, side.size() - 4) == 0);
    RelHeader h;
    CHECK(side_bits(side, h, zero, neg) && h.n == n && h.is_float == 1 && h.eps == 1e-2 && h.kind == kRelLog);
    CHECK(rel_parse(lin.data(), lin.size(), &h) && h.kind == kRelLinear);
    for (size_t i = 0; i < n; i++) {
      CHECK(zero[i] == (x[i] == 0.0f) && neg[i] == (std::signbit(x[i]) ? 1 : 0));
      CHECK(inv_f(y[i], zero[i] != 0, neg[i] != 0, true) == x[i]);
    }
    std::vector<uint8_t> bad;
    auto refused = [&](size_t at, uint8_t v) {
      bad = side;
      bad[at] = v;
      RelHeader r;
      return !rel_parse(bad.data(), bad.size(), &r);
    };
    CHECK(refused(0, 'X') && refused(1, 'X') && refused(2, 'X') && refused(3, 'X') && refused(3, 'K'));
    CHECK(refused(2, 'R') /* "SPRG" */ && refused(3, 'L') /* "SPLL" */);
    CHECK(refused(4, 2) && refused(5, 2) && refused(6, 1) && refused(7, 1));
    CHECK(refused(15, 0x7f) /* eps huge */ && refused(15, 0xbf) /* negative */ && refused(40, 1) && refused(47, 1));
    CHECK(refused(24, side[24] + 8) && refused(32, side[32] + 8) && refused(24, 8));
    RelHeader r;
    CHECK(!rel_parse(side.data(), side.size() - 1, &r) && !rel_parse(side.data(), 47, &r) && !rel_parse(nullptr, side.size(), &r));
    bad = side;   // n of 0
    memset(bad.data() + 16, 0, 8);
    CHECK(!rel_parse(bad.data(), bad.size(), &r));
    bad = side;   // eps of +0.0: a forward call's stream
    memset(bad.data() + 8, 0, 8);
    CHECK(rel_parse(bad.data(), bad.size(), &r) && r.eps == 0.0 && r.kind == kRelLog);
    bad = side;
    bad[kRelHeaderBytes + 8] ^= 1;
    CHECK(!side_bits(bad, h, zero, neg));
    // eps at this kind's floor: the log kind's rule accepts it, the linear kind's does not -- under either magic the
    // rule is the magic's
    bad = side;
    mask_put_u64(bad.data() + 8, rel_bits(log_floor[1]));
    CHECK(rel_parse(bad.data(), bad.size(), &r) && r.kind == kRelLog && r.eps == log_floor[1]);
    bad[2] = 'R';
    bad[3] = 'L';
    CHECK(!rel_parse(bad.data(), bad.size(), &r));
  }
  {
    std::vector<double> x{1.0, inf}, y;
    std::vector<uint8_t> side;
    CHECK(!log_forward_all(x, 1e-2, y, side));
  }
  std::printf("rel_log_check ok\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 1)
    return log_self_check();
  const std::string_view cmd = argv[1];
  if (cmd == "tolerance" && argc == 4) {
    double t = 0.0;
    if (rel_tolerance(std::strtod(argv[2], nullptr), std::atoi(argv[3]) != 0, &t, kRelLog))
      std::printf("%a\n", t);
    else
      std::printf("refused\n");
    return 0;
  }
  if (cmd == "forward" && argc == 7) {
    const double eps = std::strtod(argv[3], nullptr);
    return std::string_view(argv[2]) == "f32" ? log_forward_files<float>(eps, argv + 4)
                                              : log_forward_files<double>(eps, argv + 4);
  }
  if (cmd == "inverse" && argc == 6)
    return std::string_view(argv[2]) == "f32" ? kind_inverse_files<float>(argv + 3) : kind_inverse_files<double>(argv + 3);
  std::fprintf(stderr, "usage: rel_log_check [tolerance|forward|inverse ...]\n");
  return 2;
}
