// Host check of sperr_amd/csrc/mask.h, the rules of missing values: the predicate, the order of the valid samples and
// the fill value, the header's writer and parser with every refusal, the kind rule at its boundary, words <-> toggles
// both ways against loops written out here, the ballot interleave of the 16-byte forms, and the size bound.
//   mask_check                         runs the checks, prints "mask_check ok"
//   mask_check stream <bits> <out>     <bits>: n bytes of 0 / 1; writes the mask stream mask.h makes of them
// Built with the address and undefined sanitizers by tests/test_mask_host.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string_view>
#include <vector>

#include "mask.h"

using namespace sperrhip;

#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      return 1;                                             \
    }                                                       \
  } while (0)

// ---- written out: what the header's functions have to agree with ---------------------------------------------------
static std::vector<uint64_t> words_by_loop(const std::vector<uint8_t>& bits)
{
  std::vector<uint64_t> w((bits.size() + 63) / 64, 0);
  for (size_t i = 0; i < bits.size(); i++)
    if (bits[i])
      w[i / 64] |= uint64_t(1) << (i % 64);
  return w;
}

static std::vector<uint32_t> toggles_by_loop(const std::vector<uint8_t>& bits)
{
  std::vector<uint32_t> t;
  uint8_t prev = 0;
  for (size_t i = 0; i < bits.size(); i++) {
    if ((bits[i] != 0) != (prev != 0))
      t.push_back((uint32_t)i);
    prev = bits[i];
  }
  return t;
}

// the way the kernels go: toggle bits word by word with the carry, positions by counting trailing zeros
static std::vector<uint32_t> toggles_by_words(const std::vector<uint64_t>& w, size_t n)
{
  std::vector<uint32_t> t;
  uint64_t carry = 0;
  for (size_t k = 0; k < w.size(); k++) {
    const uint32_t nbits = (uint32_t)(n - k * 64 < 64 ? n - k * 64 : 64);
    uint64_t tb = mask_toggle_bits(w[k], carry, nbits);
    while (tb) {
      t.push_back((uint32_t)(k * 64 + (size_t)__builtin_ctzll(tb)));
      tb &= tb - 1;
    }
    carry = w[k] >> 63;
  }
  return t;
}

static std::vector<uint8_t> make_stream(const std::vector<uint8_t>& bits)
{
  const size_t n = bits.size();
  const std::vector<uint64_t> w = words_by_loop(bits);
  const std::vector<uint32_t> t = toggles_by_words(w, n);
  uint64_t nmissing = 0;
  for (uint8_t b : bits)
    nmissing += b ? 1 : 0;
  const MaskHeader h = mask_header_of(n, nmissing, t.size());
  std::vector<uint8_t> s(kMaskHeaderBytes + mask_payload_bytes(h.kind, h.count));
  mask_write_header(h, s.data());
  uint8_t* p = s.data() + kMaskHeaderBytes;
  if (h.kind == kMaskKindToggles)
    for (size_t i = 0; i < t.size(); i++)
      for (int b = 0; b < 4; b++)
        p[4 * i + b] = (uint8_t)(t[i] >> (8 * b));
  if (h.kind == kMaskKindBits)
    for (size_t i = 0; i < w.size(); i++)
      mask_put_u64(p + 8 * i, w[i]);
  return s;
}

static int stream_mode(const char* in, const char* out)
{
  std::FILE* f = std::fopen(in, "rb");
  CHECK(f);
  std::vector<uint8_t> bits;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;)
    bits.insert(bits.end(), buf, buf + n);
  CHECK(std::fclose(f) == 0 && !bits.empty());
  const std::vector<uint8_t> s = make_stream(bits);
  std::FILE* o = std::fopen(out, "wb");
  CHECK(o && std::fwrite(s.data(), 1, s.size(), o) == s.size() && std::fclose(o) == 0);
  return 0;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int check_words_and_toggles()
{
  uint32_t seed = 12345;
  const size_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 512, 1000, 1023, 1024, 1025, 3077};
  for (size_t n : sizes)
    for (int pattern = 0; pattern < 6; pattern++) {
      std::vector<uint8_t> bits(n, 0);
      for (size_t i = 0; i < n; i++)
        bits[i] = pattern == 0   ? 0
                  : pattern == 1 ? 1
                  : pattern == 2 ? (uint8_t)(i & 1)
                  : pattern == 3 ? (uint8_t)(i + 1 == n)
                  : pattern == 4 ? (uint8_t)((lcg(seed) >> 16) % 10 == 0)
                                 : (uint8_t)((i / 61) & 1);
      const std::vector<uint64_t> w = words_by_loop(bits);
      const std::vector<uint32_t> t = toggles_by_loop(bits);
      CHECK(w.size() == mask_words(n));
      CHECK(toggles_by_words(w, n) == t);
      // back: toggles -> words, from the start and from a cursor in the middle
      uint64_t idx = 0, state = 0;
      for (size_t k = 0; k < w.size(); k++) {
        uint64_t got = mask_word_from_toggles(t.data(), t.size(), k * 64, &idx, &state);
        if (n - k * 64 < 64)
          got &= (uint64_t(1) << (n - k * 64)) - 1;
        CHECK(got == w[k]);
      }
      for (size_t s = 0; s < n; s += 37) {
        uint64_t i2 = mask_toggle_lower_bound(t.data(), t.size(), s);
        size_t before = 0;
        for (uint32_t p : t)
          before += p < s ? 1 : 0;
        CHECK(i2 == before);
        CHECK((i2 & 1) == (s > 0 ? (uint64_t)(bits[s - 1] != 0) : 0));
        uint64_t st = i2 & 1;
        const uint64_t got = mask_word_from_toggles(t.data(), t.size(), s, &i2, &st);
        for (size_t j = 0; j < 64 && s + j < n; j++)
          CHECK(((got >> j) & 1) == (uint64_t)(bits[s + j] != 0));
      }
      // the stream and its header
      const std::vector<uint8_t> s = make_stream(bits);
      MaskHeader h;
      CHECK(mask_parse(s.data(), s.size(), &h));
      CHECK(h.n == n && s.size() <= mask_max_size(n));
      size_t nmissing = 0;
      for (uint8_t b : bits)
        nmissing += b ? 1 : 0;
      const int kind = nmissing == 0 ? 0 : 4 * t.size() < 8 * w.size() ? 1 : 2;
      CHECK(h.kind == kind && h.nmissing == nmissing && h.count == (kind == 1 ? t.size() : kind == 2 ? w.size() : 0));
    }
  return 0;
}

static int check_kind_boundary()
{
  // n = 512: eight words, 64 bytes of bits; 15 toggles are 60 bytes, 16 are 64
  CHECK(mask_choose_kind(512, 1, 15) == kMaskKindToggles && mask_choose_kind(512, 1, 16) == kMaskKindBits);
  CHECK(mask_choose_kind(512, 0, 0) == kMaskKindNone);
  for (int nt = 15; nt <= 16; nt++) {
    std::vector<uint8_t> bits(512, 0);
    for (int k = 0; k < nt; k++)
      for (size_t i = 3 * k + 1; i < 512; i++)
        bits[i] ^= 1;
    const std::vector<uint8_t> s = make_stream(bits);
    MaskHeader h;
    CHECK(mask_parse(s.data(), s.size(), &h));
    CHECK(h.kind == (nt == 15 ? kMaskKindToggles : kMaskKindBits));
    CHECK(s.size() == (nt == 15 ? 92u : 96u));
    CHECK(h.count == (nt == 15 ? 15u : 8u));
  }
  // all missing: one toggle; n beyond 2^32: bits whatever the toggles
  CHECK(mask_header_of(48840, 48840, 1).kind == kMaskKindToggles && mask_header_of(48840, 48840, 1).count == 1);
  CHECK(mask_choose_kind((uint64_t(1) << 32) + 1, 5, 1) == kMaskKindBits);
  CHECK(mask_choose_kind(uint64_t(1) << 32, 5, 1) == kMaskKindToggles);
  CHECK(mask_max_size(1) == 40 && mask_max_size(64) == 40 && mask_max_size(65) == 48 && mask_max_size(48840) == 32 + 8 * 764);
  return 0;
}

static int check_refusals()
{
  std::vector<uint8_t> bits(200, 0);
  for (size_t i = 50; i < 120; i++)
    bits[i] = 1;
  const std::vector<uint8_t> good = make_stream(bits);
  MaskHeader h;
  CHECK(mask_parse(good.data(), good.size(), &h) && h.kind == kMaskKindToggles && h.count == 2 && h.nmissing == 70);
  CHECK(!mask_parse(nullptr, good.size(), &h));
  CHECK(!mask_parse(good.data(), 31, &h));
  CHECK(!mask_parse(good.data(), good.size() - 1, &h));   // one byte short
  CHECK(!mask_parse(good.data(), good.size() + 1, &h));
  for (int at = 0; at < 8; at++) {   // magic, version, kind, reserved
    std::vector<uint8_t> bad = good;
    bad[at] = at == 5 ? 3 : (uint8_t)(bad[at] + 1);
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
  }
  {
    std::vector<uint8_t> bad = good;   // kind 2 with the toggles' count
    bad[5] = 2;
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
    bad = good;   // n == 0
    mask_put_u64(bad.data() + 8, 0);
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
    bad = good;   // nmissing > n
    mask_put_u64(bad.data() + 16, 201);
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
    bad = good;   // a count the length does not hold, and one that would wrap
    mask_put_u64(bad.data() + 24, 3);
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
    mask_put_u64(bad.data() + 24, ~uint64_t(0));
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
    bad = good;   // toggles for n > 2^32
    mask_put_u64(bad.data() + 8, (uint64_t(1) << 32) + 1);
    CHECK(!mask_parse(bad.data(), bad.size(), &h));
  }
  {
    uint8_t none[kMaskHeaderBytes];
    mask_write_header(mask_header_of(77, 0, 0), none);
    CHECK(mask_parse(none, sizeof none, &h) && h.kind == kMaskKindNone && h.n == 77 && h.count == 0);
    mask_put_u64(none + 16, 1);   // kind 0 with a missing sample
    CHECK(!mask_parse(none, sizeof none, &h));
  }
  return 0;
}

static int check_predicate_order_and_fill()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(mask_rule_ok(kMaskRuleNan, 0.0) && mask_rule_ok(kMaskRuleAbsGe, 1e20) && !mask_rule_ok(kMaskRuleAbsGe, 0.0));
  CHECK(!mask_rule_ok(kMaskRuleAbsGe, -1.0) && !mask_rule_ok(kMaskRuleAbsGe, (double)inf) &&
        !mask_rule_ok(kMaskRuleAbsGe, (double)nan) && !mask_rule_ok(0, 1.0) && !mask_rule_ok(3, 1.0));
  CHECK(mask_missing(nan, kMaskRuleNan, 0.0) && !mask_missing(inf, kMaskRuleNan, 0.0) && !mask_missing(1.0f, kMaskRuleNan, 0.0));
  CHECK(mask_missing(nan, kMaskRuleAbsGe, 1e20) && mask_missing(inf, kMaskRuleAbsGe, 1e20) &&
        mask_missing(-inf, kMaskRuleAbsGe, 1e20) && mask_missing(1e20f, kMaskRuleAbsGe, 1e20) &&
        mask_missing(-1e20, kMaskRuleAbsGe, 1e20) && !mask_missing(9.9e19, kMaskRuleAbsGe, 1e20));
  // the order: -inf < -1 < -0.0 < +0.0 < denormal < 1 < inf, for both widths, and the way back
  const double ladder[] = {-(double)inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, (double)inf};
  for (size_t i = 0; i + 1 < sizeof ladder / sizeof *ladder; i++) {
    CHECK(mask_key(ladder[i]) < mask_key(ladder[i + 1]));
    CHECK(mask_key((float)ladder[i]) <= mask_key((float)ladder[i + 1]));
    const double back = mask_unkey(mask_key(ladder[i]), false);
    CHECK(memcmp(&back, &ladder[i], 8) == 0);
    const float f = (float)ladder[i];
    const double fb = mask_unkey(mask_key(f), true), fw = (double)f;
    CHECK(memcmp(&fb, &fw, 8) == 0);
  }
  CHECK(mask_key(-0.0f) < mask_key(0.0f) && mask_key(-0.0f) < kMaskKeyNone && mask_key(-inf) > 0);
  bool finite = false;
  CHECK(mask_fill_value(mask_key(-3.0), mask_key(5.0), true, false, &finite) == 1.0 && finite);
  CHECK(mask_fill_value(kMaskKeyNone, 0, false, false, &finite) == 0.0 && finite);
  (void)mask_fill_value(mask_key(-3.0f), mask_key(inf), true, true, &finite);
  CHECK(!finite);
  (void)mask_fill_value(mask_key(-(double)inf), mask_key(2.0), true, false, &finite);
  CHECK(!finite);
  // -0.0 and +0.0 as the extremes: 0.5 * -0.0 + 0.5 * +0.0 = +0.0
  const double z = mask_fill_value(mask_key(-0.0), mask_key(0.0), true, false, &finite);
  const double pz = 0.0;
  CHECK(finite && memcmp(&z, &pz, 8) == 0);
  // fp32: narrowed once
  const double f32 = mask_fill_value(mask_key(0.1f), mask_key(0.7f), true, true, &finite);
  CHECK(f32 == (double)(float)(0.5 * (double)0.1f + 0.5 * (double)0.7f));
  // the largest finite extremes do not overflow: the halves are taken first
  const double big = std::numeric_limits<double>::max();
  CHECK(mask_fill_value(mask_key(big), mask_key(big), true, false, &finite) == big && finite);
  return 0;
}

template <uint32_t P>
static int check_ballots()
{
  // a wavefront's load covers 64 * P samples, lane l holding samples P * l + j: the P ballots against the P words
  uint32_t seed = 99 + P;
  for (int round = 0; round < 50; round++) {
    uint8_t bits[64 * P];
    for (uint32_t i = 0; i < 64 * P; i++)
      bits[i] = (uint8_t)((lcg(seed) >> 20) & 1);
    uint64_t ballot[P] = {};
    for (uint32_t l = 0; l < 64; l++)
      for (uint32_t j = 0; j < P; j++)
        if (bits[P * l + j])
          ballot[j] |= uint64_t(1) << l;
    for (uint32_t w = 0; w < P; w++) {
      uint64_t want = 0;
      for (uint32_t b = 0; b < 64; b++)
        if (bits[64 * w + b])
          want |= uint64_t(1) << b;
      CHECK(mask_word_of_ballots<P>(ballot, w) == want);
    }
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 4 && std::string_view(argv[1]) == "stream")
    return stream_mode(argv[2], argv[3]);
  if (argc != 1)
    return 2;
  static_assert(kMaskTile % 64 == 0 && kMaskTile == kMaskTileWords * 64, "a tile is whole words");
  static_assert(kMaskTile % (64 * (kMaskPackBytes / 4)) == 0, "a tile is whole loads of a wavefront");
  if (check_words_and_toggles() || check_kind_boundary() || check_refusals() || check_predicate_order_and_fill() ||
      check_ballots<1>() || check_ballots<2>() || check_ballots<4>())
    return 1;
  std::printf("mask_check ok\n");
  return 0;
}
