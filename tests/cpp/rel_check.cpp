// Host check of sperr_amd/csrc/rel.h, the rule of point-wise relative error: the tolerance with its floor and every
// refusal, the forward map with the zero class and the signs, the inverse with its clamp and its narrowing, the side
// stream's writer and parser with every refusal, and the figures of the check.
//   rel_check                                        runs the checks, prints "rel_check ok"
//   rel_check tolerance <eps as %a> <is_float>       prints t as %a, or "refused"
//   rel_check forward <f32|f64> <eps as %a> <in> <y> <side>   <in>: raw samples; writes y (doubles) and the side stream
//   rel_check inverse <f32|f64> <y> <side> <out>     y' and a side stream into x' of the named type
// Built with the address and undefined sanitizers by tests/test_rel_host.py; no GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string_view>
#include <vector>

#include "rel.h"

using namespace sperrhip;

#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      return 1;                                             \
    }                                                       \
  } while (0)

// ---- an SPMK stream of bits and back, from the pieces of mask.h -----------------------------------------------------
static std::vector<uint8_t> mask_stream_of(const std::vector<uint8_t>& bits)
{
  const size_t n = bits.size();
  std::vector<uint64_t> w((n + 63) / 64, 0);
  uint64_t nset = 0;
  for (size_t i = 0; i < n; i++)
    if (bits[i]) {
      w[i / 64] |= uint64_t(1) << (i % 64);
      nset++;
    }
  std::vector<uint32_t> tog;
  uint64_t carry = 0;
  for (size_t k = 0; k < w.size(); k++) {
    uint64_t tb = mask_toggle_bits(w[k], carry, (uint32_t)(n - k * 64 < 64 ? n - k * 64 : 64));
    while (tb) {
      tog.push_back((uint32_t)(k * 64 + (size_t)__builtin_ctzll(tb)));
      tb &= tb - 1;
    }
    carry = w[k] >> 63;
  }
  const MaskHeader h = mask_header_of(n, nset, tog.size());
  std::vector<uint8_t> s(kMaskHeaderBytes + mask_payload_bytes(h.kind, h.count));
  mask_write_header(h, s.data());
  if (h.kind == kMaskKindToggles)
    memcpy(s.data() + kMaskHeaderBytes, tog.data(), 4 * tog.size());
  else if (h.kind == kMaskKindBits)
    memcpy(s.data() + kMaskHeaderBytes, w.data(), 8 * w.size());
  return s;
}

static bool bits_of_mask_stream(const uint8_t* s, size_t len, uint64_t n, std::vector<uint8_t>& bits)
{
  MaskHeader h;
  if (!mask_parse(s, len, &h) || h.n != n)
    return false;
  bits.assign(n, 0);
  std::vector<uint32_t> tog;
  std::vector<uint64_t> w;
  if (h.kind == kMaskKindToggles) {
    tog.resize(h.count);
    memcpy(tog.data(), s + kMaskHeaderBytes, 4 * h.count);
  }
  else if (h.kind == kMaskKindBits) {
    w.resize(h.count);
    memcpy(w.data(), s + kMaskHeaderBytes, 8 * h.count);
  }
  uint64_t idx = 0, state = 0;
  for (uint64_t s0 = 0; s0 < n; s0 += 64) {
    const uint64_t word = h.kind == kMaskKindToggles ? mask_word_from_toggles(tog.data(), h.count, s0, &idx, &state)
                          : h.kind == kMaskKindBits  ? w[s0 / 64]
                                                     : 0;
    for (uint64_t j = 0; j < 64 && s0 + j < n; j++)
      bits[s0 + j] = (uint8_t)((word >> j) & 1);
  }
  return true;
}

// ---- the side stream of a volume, and a volume of a side stream -----------------------------------------------------
template <typename T>
static bool forward_all(const std::vector<T>& x, double eps, std::vector<double>& y, std::vector<uint8_t>& side)
{
  const size_t n = x.size();
  std::vector<uint8_t> zero(n), neg(n);
  y.resize(n);
  for (size_t i = 0; i < n; i++) {
    RelClass c;
    y[i] = rel_forward(x[i], &c);
    if (!c.finite)
      return false;
    zero[i] = c.zero;
    neg[i] = c.neg;
  }
  const std::vector<uint8_t> zs = mask_stream_of(zero), ss = mask_stream_of(neg);
  const RelHeader h{sizeof(T) == 4, eps, n, zs.size(), ss.size()};
  side.assign((size_t)rel_stream_bytes(h), 0);
  rel_write_header(h, side.data());
  memcpy(side.data() + kRelHeaderBytes, zs.data(), zs.size());
  memcpy(side.data() + rel_sign_offset(h), ss.data(), ss.size());
  return true;
}

static bool side_bits(const std::vector<uint8_t>& side, RelHeader& h, std::vector<uint8_t>& zero,
                      std::vector<uint8_t>& neg)
{
  return rel_parse(side.data(), side.size(), &h) &&
         bits_of_mask_stream(side.data() + kRelHeaderBytes, (size_t)h.zero_len, h.n, zero) &&
         bits_of_mask_stream(side.data() + rel_sign_offset(h), (size_t)h.sign_len, h.n, neg);
}

template <typename T>
static std::vector<T> read_file(const char* path)
{
  std::vector<T> v;
  FILE* f = std::fopen(path, "rb");
  if (!f)
    return v;
  std::fseek(f, 0, SEEK_END);
  const long len = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)len / sizeof(T));
  if (len > 0 && std::fread(v.data(), sizeof(T), v.size(), f) != v.size())
    v.clear();
  std::fclose(f);
  return v;
}

template <typename T>
static bool write_file(const char* path, const std::vector<T>& v)
{
  FILE* f = std::fopen(path, "wb");
  if (!f)
    return false;
  const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

template <typename T>
static int forward_files(double eps, char** a)
{
  const std::vector<T> x = read_file<T>(a[0]);
  std::vector<double> y;
  std::vector<uint8_t> side;
  if (x.empty() || !forward_all(x, eps, y, side)) {
    std::printf("refused\n");
    return 3;
  }
  return write_file(a[1], y) && write_file(a[2], side) ? 0 : 2;
}

template <typename OT>
static int inverse_files(char** a)
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
    out[i] = rel_inverse<OT>(y[i], zero[i] != 0, neg[i] != 0, h.is_float != 0);
  return write_file(a[2], out) ? 0 : 2;
}

// ---- the checks -----------------------------------------------------------------------------------------------------
static int self_check()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double t = 0.0;
  // the tolerance: as written, and every refusal
  CHECK(rel_tolerance(1e-2, true, &t) && t == 1e-2 / (1.0 + 1e-2) - 0x1p-22);
  CHECK(rel_tolerance(1e-2, false, &t) && t == 1e-2 / (1.0 + 1e-2) - 0x1p-40);
  CHECK(rel_tolerance(0.5, true, &t) && t == 0.5 / 1.5 - 0x1p-22);
  CHECK(!rel_tolerance(nextafter(0.5, 1.0), true, &t) && !rel_tolerance(inf, true, &t) && !rel_tolerance(nan, false, &t));
  CHECK(!rel_tolerance(0.0, true, &t) && !rel_tolerance(-1e-2, false, &t) && !rel_tolerance(-1.0, true, &t) &&
        !rel_tolerance(-inf, true, &t));
  // the floor: the first eps whose t reaches s, by bisection on the bit patterns between 2 s and 4 s
  for (int f = 0; f < 2; f++) {
    const double s = rel_slack(f != 0);
    uint64_t lo = rel_bits(2.0 * s), hi = rel_bits(4.0 * s);   // (2 s / (1 + 2 s) - s < s: refused)
    CHECK(!rel_tolerance(rel_from_bits(lo), f != 0, &t) && rel_tolerance(rel_from_bits(hi), f != 0, &t));
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      (rel_tolerance(rel_from_bits(mid), f != 0, &t) ? hi : lo) = mid;
    }
    const double floor_eps = rel_from_bits(hi);
    CHECK(rel_tolerance(floor_eps, f != 0, &t) && t >= s && !rel_tolerance(nextafter(floor_eps, 0.0), f != 0, &t));
    CHECK(floor_eps > 2.0 * s && floor_eps < 2.0 * s * (1.0 + 8.0 * s));
  }
  // the classes and y
  RelClass c;
  CHECK(rel_bits(rel_forward(0.0f, &c)) == kRelNanBits && c.zero && !c.neg && c.finite);
  CHECK(rel_bits(rel_forward(-0.0, &c)) == kRelNanBits && c.zero && c.neg && c.finite);
  CHECK(rel_bits(rel_forward(-0x1p-1023, &c)) == kRelNanBits && c.zero && c.neg);
  CHECK(rel_forward(0x1p-1022, &c) == -1022.0 && !c.zero);
  // the subnormal floats: a normal double each, stretched by 2 about -126 for fp32 data and for it alone
  CHECK(rel_forward(0x1p-149f, &c) == -172.0 && !c.zero && !c.neg && rel_forward(0x1p-149, &c) == -149.0);
  CHECK(rel_forward(-0x1.8p-148f, &c) == -169.0 && c.neg && rel_forward(-0x1.8p-148, &c) == -147.5);
  CHECK(rel_forward(0x1p-126f, &c) == -126.0 && rel_forward(0x1.fffffcp-127f, &c) == -126.0 - 0x1p-21);
  CHECK(rel_forward(1.0f, &c) == 0.0 && rel_forward(1.5, &c) == 0.5 && rel_forward(-3.0f, &c) == 1.5 && c.neg);
  CHECK(rel_forward(std::numeric_limits<float>::max(), &c) == 127.0 + (double)0x7fffff * 0x1p-23);
  CHECK(rel_forward(std::numeric_limits<double>::max(), &c) == 1024.0);   // (rounded once, upward: the inverse clamps)
  (void)rel_forward(std::numeric_limits<float>::infinity(), &c);
  CHECK(!c.finite);
  (void)rel_forward(nan, &c);
  CHECK(!c.finite);
  // the inverse: exact on y, the clamp, the narrowing, the signs of zeros
  CHECK(rel_inverse<double>(0.5, false, false, false) == 1.5 && rel_inverse<float>(1.5, false, true, false) == -3.0f);
  CHECK(rel_inverse<float>(-149.0, false, false, false) == 0x1p-149f && rel_inverse<float>(-147.5, false, true, false) == -0x1.8p-148f);
  CHECK(rel_inverse<float>(-172.0, false, false, true) == 0x1p-149f && rel_inverse<float>(-169.0, false, true, true) == -0x1.8p-148f);
  CHECK(rel_inverse<double>(-128.0, false, false, true) == 0x1p-127 && rel_inverse<double>(-126.0, false, false, true) == 0x1p-126);
  CHECK(rel_inverse<double>(-125.5, false, false, true) == rel_inverse<double>(-125.5, false, false, false));
  CHECK(rel_inverse<double>(-1022.0, false, false, false) == 0x1p-1022);
  CHECK(rel_inverse<double>(-2000.0, false, false, false) == rel_inverse<double>(-1080.0, false, false, false));
  CHECK(rel_inverse<double>(nan, false, true, false) == -rel_inverse<double>(-1080.0, false, false, false));
  CHECK(rel_inverse<double>(5000.0, false, false, false) == ldexp(2.0 - 0x1p-43, 1023));
  CHECK(rel_inverse<double>(inf, false, false, false) == rel_inverse<double>(1024.0, false, false, false));
  CHECK(rel_inverse<float>(1000.0, false, false, false) == std::numeric_limits<float>::max());
  CHECK(rel_inverse<float>(128.0, false, true, false) == -std::numeric_limits<float>::max());
  CHECK(rel_inverse<float>(127.0 + (double)0x7fffff * 0x1p-23, false, false, true) == std::numeric_limits<float>::max());
  CHECK(rel_bits(rel_inverse<double>(3.0, true, true, false)) == uint64_t(1) << 63 && rel_bits(rel_inverse<double>(nan, true, false, false)) == 0);
  {
    const float z = rel_inverse<float>(nan, true, true, false);
    uint32_t u;
    memcpy(&u, &z, 4);
    CHECK(u == 0x80000000u);
  }
  // the side stream: sizes, the round trip, every refusal of the header
  CHECK(rel_max_size(4913) == 48 + 2 * mask_max_size(4913) && rel_max_size(1) == 48 + 2 * 40);
  for (size_t n : {size_t(1), size_t(63), size_t(1024), size_t(1025), size_t(4913)}) {
    std::vector<float> x(n);
    for (size_t i = 0; i < n; i++)
      x[i] = i % 7 == 3 ? 0.0f : (i % 5 == 1 ? -1.0f : 1.0f) * (float)(i + 1) * 0x1p-140f;
    std::vector<double> y;
    std::vector<uint8_t> side, zero, neg;
    CHECK(forward_all(x, 1e-2, y, side) && side.size() <= rel_max_size(n) && side.size() % 4 == 0);
    RelHeader h;
    CHECK(side_bits(side, h, zero, neg) && h.n == n && h.is_float == 1 && h.eps == 1e-2);
    for (size_t i = 0; i < n; i++) {
      CHECK(zero[i] == (x[i] == 0.0f) && neg[i] == (std::signbit(x[i]) ? 1 : 0));
      CHECK(rel_inverse<float>(y[i], zero[i] != 0, neg[i] != 0, true) == x[i]);
    }
    std::vector<uint8_t> bad;
    auto refused = [&](size_t at, uint8_t v) {
      bad = side;
      bad[at] = v;
      RelHeader r;
      return !rel_parse(bad.data(), bad.size(), &r);
    };
    CHECK(refused(0, 'X') && refused(3, 'K') && refused(4, 2) && refused(5, 2) && refused(6, 1) && refused(7, 1));
    CHECK(refused(15, 0x7f) /* eps huge */ && refused(15, 0xbf) /* negative */ && refused(40, 1) && refused(47, 1));
    CHECK(refused(24, side[24] + 8) && refused(32, side[32] + 8) && refused(24, 8));
    RelHeader r;
    CHECK(!rel_parse(side.data(), side.size() - 1, &r) && !rel_parse(side.data(), 47, &r) && !rel_parse(nullptr, side.size(), &r));
    bad = side;   // n of 0
    memset(bad.data() + 16, 0, 8);
    CHECK(!rel_parse(bad.data(), bad.size(), &r));
    bad = side;   // eps of +0.0: a forward call's stream
    memset(bad.data() + 8, 0, 8);
    CHECK(rel_parse(bad.data(), bad.size(), &r) && r.eps == 0.0);
    // the streams' own n is mask_parse's to hold against the header's
    bad = side;
    bad[kRelHeaderBytes + 8] ^= 1;
    CHECK(!side_bits(bad, h, zero, neg));
  }
  // a sample that is not finite refuses the volume
  {
    std::vector<double> x{1.0, inf}, y;
    std::vector<uint8_t> side;
    CHECK(!forward_all(x, 1e-2, y, side));
  }
  // the check's figures
  {
    RelCheck k = rel_check_pair(2.0, 2.02, 1e-2);
    CHECK(k.counted && !k.mismatch && k.ratio == fabs(2.02 - 2.0) / 2.0 && k.violates == !(fabs(2.02 - 2.0) <= 1e-2 * 2.0));
    k = rel_check_pair(2.0, 2.0, 0.0);
    CHECK(k.counted && !k.violates && k.ratio == 0.0);
    k = rel_check_pair(0.0, -0.0, 1e-2);
    CHECK(!k.counted && k.mismatch && !k.violates && k.ratio == 0.0);
    k = rel_check_pair(1.0, -1.0, 0.5);
    CHECK(k.counted && k.mismatch && k.violates && k.ratio == 2.0);
    k = rel_check_pair(1.0, 0.0, 0.5);
    CHECK(k.mismatch && k.violates);
    k = rel_check_pair(0x1p-1030, 0.0, 0.5);   // both in the zero class
    CHECK(!k.counted && !k.mismatch);
  }
  std::printf("rel_check ok\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 1)
    return self_check();
  const std::string_view cmd = argv[1];
  if (cmd == "tolerance" && argc == 4) {
    double t = 0.0;
    if (rel_tolerance(std::strtod(argv[2], nullptr), std::atoi(argv[3]) != 0, &t))
      std::printf("%a\n", t);
    else
      std::printf("refused\n");
    return 0;
  }
  if (cmd == "forward" && argc == 7) {
    const double eps = std::strtod(argv[3], nullptr);
    return std::string_view(argv[2]) == "f32" ? forward_files<float>(eps, argv + 4) : forward_files<double>(eps, argv + 4);
  }
  if (cmd == "inverse" && argc == 6)
    return std::string_view(argv[2]) == "f32" ? inverse_files<float>(argv + 3) : inverse_files<double>(argv + 3);
  std::fprintf(stderr, "usage: rel_check [tolerance|forward|inverse ...]\n");
  return 2;
}
