"""CPU: the decoder's coefficient-to-sample rule (sperr_amd/csrc/dequant.h) against the reference's two statements.

Seven kernels turn a decoded integer coefficient into a wavelet sample on their way, and the decoder's output is bit-identical
to the reference only if all of them do it the same way; they all call the header.  The header compiles for the host, with
the library's flags (-ffp-contract=off).  The program below draws cases -- magnitudes with the edge values 0, 1, 2^31 - 1,
2^31, 2^32 - 1 (and up to 2^53 for 64-bit coefficients), both signs, all four combinations of the two masks, every last plane
(0..31, 0..52), q over some 600 binades -- and compares each result's bits with the two statements written out plainly here:
`thr + thr - thr / 2 - 1` (src/SPECK_INT.cpp:462-468) and `q * double(c) * tmpd[bit]` (src/SPECK_FLT.cpp:373-399).  It also
checks that a packed word (coef_scheme_pack, what k_ref_assemble writes) dequantises to what the unpacked magnitude, its sign
and masks give: scheme 1 for magnitudes below 2^31, scheme 2 for odd magnitudes and 0 -- over several q all of them in the lowest and
the highest 2^16 of each range and a few million drawn in between, and for one q every one of them (the plain build only,
on threads: 2^33 words in all) --, and that a sample "found on the plane above plane 31" is
completed with 0, as every copy of the rule did before there was a header.

Scheme 2 stores t for the magnitude 2 t + 1 and keeps t = 0 for the magnitude 0, so the magnitude 1 has no word of its own
(it would come back as 0).  It cannot occur: the scheme is chosen only when every sample of the chunk was last refined on
plane 2 or above, and such a magnitude is at least 2^2 + 2^1 - 1 = 5.  The odd magnitudes checked therefore start at 3, and
the program asserts that 1 is indeed the one odd value that does not survive -- the packing is the parent commit's, unchanged.

The same program runs once more built with -fsanitize=undefined (host code, a program of its own): a shift by the type's width
or more, the one way these few lines can go wrong silently, ends it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "dequant.h"
using namespace sperrhip;

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }
static double next_q()   // a quantisation step: any mantissa, some 600 binades
{
  const double m = 1.0 + (double)(next() >> 12) / 4503599627370496.0;
  return ldexp(m, (int)(next() % 601) - 300);
}
static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

// ---- the reference's statements, written out (no call into the header)
template <typename CT>
static CT ref_init(int plane)   // SPECK_INT.cpp:462-468 with m_threshold = 2^plane
{
  const CT m_threshold = (CT)1 << plane;
  const CT init_val = m_threshold + m_threshold - m_threshold / CT{2} - CT{1};
  return init_val;
}
template <typename CT>
static double ref_sample(double q, CT c, unsigned bit)   // SPECK_FLT.cpp:373-399
{
  const double tmpd[2] = {-1.0, 1.0};
  return q * static_cast<double>(c) * tmpd[bit];
}
// what the decoder leaves of a coefficient that was never refined: 0, and a mask bit -- found during the last decoded plane
// (isNew: threshold 2^lastPlane) or on the plane before (isOld: twice that; no such plane above the type's highest)
template <typename CT>
static CT ref_complete(CT mag, bool isNew, bool isOld, int lastPlane)
{
  if (mag != 0)
    return mag;
  if (isNew)
    return ref_init<CT>(lastPlane);
  if (isOld)
    return lastPlane + 1 < (int)(8 * sizeof(CT)) ? ref_init<CT>(lastPlane + 1) : (CT)0;
  return 0;
}

static long bad = 0, seen = 0;
static void expect(bool ok, const char* what, uint64_t a, uint64_t b, int plane)
{
  seen++;
  if (!ok && bad++ < 20)
    printf("MISMATCH %s: %016llx %016llx (plane %d)\n", what, (unsigned long long)a, (unsigned long long)b, plane);
}

static DecState state(int nbp, int lastPlane, int refPlaneP1)
{
  DecState s;
  memset(&s, 0, sizeof s);
  s.active = 1;
  s.nbp = nbp;
  s.lastPlane = lastPlane;
  s.refPlaneP1 = refPlaneP1;
  return s;
}

// a word of type W with bit `sh` set to `bit`, the others random
template <typename W>
static W word_with(unsigned sh, bool bit) { return (W)((next() & ~((uint64_t)1 << sh)) | ((uint64_t)bit << sh)); }

template <typename CT, typename W>
static void one_masks(const DequantRule<CT>& rule, double q, CT mag, unsigned positive, bool isNew, bool isOld, int lastPlane)
{
  const double want = ref_sample<CT>(q, ref_complete<CT>(mag, isNew, isOld, lastPlane), positive);
  const unsigned sh = (unsigned)(next() % (8 * sizeof(W)));
  const double got = dequant_masks<CT, W>(rule, mag, word_with<W>(sh, isNew), word_with<W>(sh, isOld), word_with<W>(sh, positive != 0), sh);
  expect(bits(got) == bits(want), sizeof(CT) == 4 ? "dequant_masks 32" : "dequant_masks 64", bits(got), bits(want), lastPlane);
  // the two halves used apart (k_inv_quantize, k_dec_finish): the threshold per element, then the multiply
  CT c = mag;
  if (c == 0 && (isNew || (isOld && lastPlane + 1 < (int)(8 * sizeof(CT)))))
    c = never_refined<CT>(lastPlane + (isNew ? 0 : 1));
  expect(bits(dequant_value<CT>(q, c, positive != 0)) == bits(want), "never_refined + dequant_value", 0, bits(want), lastPlane);
}

template <typename CT>
static void masks_cases(int planes, const CT* edges, int nedges, CT randMask)
{
  for (int lastPlane = 0; lastPlane < planes; lastPlane++) {
    const DecState s = state(planes, lastPlane, 0);
    expect(never_refined<CT>(lastPlane) == ref_init<CT>(lastPlane), "never_refined", 0, 0, lastPlane);
    // (the closed form: 1 on plane 0, 1.5 * 2^plane - 1 above)
    expect(never_refined<CT>(lastPlane) == (lastPlane == 0 ? (CT)1 : (CT)3 * ((CT)1 << (lastPlane - 1)) - 1), "1.5 * 2^p - 1", 0, 0, lastPlane);
    for (int rep = 0; rep < 40; rep++) {
      const double q = next_q();
      const DequantRule<CT> rule = dequant_rule<CT>(q, true, &s);
      const DequantRule<CT> bare = dequant_rule<CT>(q, false, nullptr);   // no masks: nothing is completed
      expect(bare.fillNew == 0 && bare.fillOld == 0 && bare.scheme == 0, "rule without masks", bare.fillNew, bare.fillOld, lastPlane);
      for (int e = 0; e < nedges + 3; e++) {
        const CT mag = e < nedges ? edges[e] : (CT)(next() & randMask) >> (next() % (8 * sizeof(CT)));
        for (unsigned positive = 0; positive < 2; positive++)
          for (int m = 0; m < 4; m++) {
            one_masks<CT, uint64_t>(rule, q, mag, positive, (m & 1) != 0, (m & 2) != 0, lastPlane);
            one_masks<CT, uint32_t>(rule, q, mag, positive, (m & 1) != 0, (m & 2) != 0, lastPlane);
            const double got = dequant_masks<CT, uint64_t>(bare, mag, 0ull, 0ull, (uint64_t)positive, 0);
            expect(bits(got) == bits(ref_sample<CT>(q, mag, positive)), "no masks", bits(got), 0, lastPlane);
          }
      }
    }
  }
}

// a packed word against the unpacked magnitude
static void one_packed(const DequantRule<uint32_t>& rule, const DequantRule<uint32_t>& plain, uint32_t mag, int scheme)
{
  for (unsigned positive = 0; positive < 2; positive++) {
    const uint32_t word = coef_scheme_pack(mag, positive != 0, scheme);
    const double got = dequant_signed(rule, word);
    const double want = ref_sample<uint32_t>(rule.q, mag, positive);
    const double viaMasks = dequant_masks<uint32_t, uint64_t>(plain, mag, 0ull, 0ull, (uint64_t)positive, 0);
    expect(bits(got) == bits(want) && bits(got) == bits(viaMasks), scheme == 1 ? "packed, scheme 1" : "packed, scheme 2", bits(got), bits(want), scheme);
  }
}
static void packed_cases()
{
  const DecState s1 = state(31, 4, 3), s2 = state(32, 7, 4), s0 = state(32, 1, 0);
  expect(coef_scheme(s1) == 1 && coef_scheme(s2) == 2 && coef_scheme(s0) == 0, "coef_scheme", 0, 0, 0);
  expect(coef_scheme(state(32, 7, 2)) == 0 && coef_scheme(state(32, 2, 0)) == 2 && coef_scheme(state(32, 9, 3)) == 2, "coef_scheme, q", 0, 0, 0);
  expect(coef_scheme_pack(0x12345u, false, 0) == 0x12345u, "scheme 0 packs nothing", 0, 0, 0);
  for (int scheme = 1; scheme <= 2; scheme++) {
    const DecState& s = scheme == 1 ? s1 : s2;
    for (int rep = 0; rep < 8; rep++) {
      const double q = next_q();
      const DequantRule<uint32_t> rule = dequant_rule<uint32_t>(q, true, &s, true), plain = dequant_rule<uint32_t>(q, true, &s);
      expect(rule.scheme == scheme && plain.scheme == 0, "rule.scheme", (uint64_t)rule.scheme, (uint64_t)scheme, 0);
      one_packed(rule, plain, 0u, scheme);
      for (uint32_t k = 0; k < 65536u; k++) {
        if (scheme == 1) {   // every magnitude below 2^31: the lowest and the highest 2^16, 2^18 in between
          one_packed(rule, plain, k, 1);
          one_packed(rule, plain, 0x7fffffffu - k, 1);
          for (int j = 0; j < 4; j++)
            one_packed(rule, plain, (uint32_t)next() & 0x7fffffffu, 1);
        }
        else {               // every odd magnitude from 3 on (and 0, above; 1 has no word: see the test's docstring)
          one_packed(rule, plain, 2u * k + 3u, 2);
          one_packed(rule, plain, 0xffffffffu - 2u * k, 2);
          for (int j = 0; j < 4; j++)
            one_packed(rule, plain, (uint32_t)next() | 3u, 2);
        }
      }
    }
  }
}

#ifdef EXHAUSTIVE
// every word of a scheme's domain, both signs, one q: scheme 1 the magnitudes below 2^31, scheme 2 the odd ones from 3 to
// 2^32 - 1 (0 is checked above, 1 has no word).  Threads share the range; each counts what differs
#include <thread>
#include <vector>
static long exhaustive_range(const DequantRule<uint32_t>& rule, const DequantRule<uint32_t>& plain, int scheme, uint64_t lo, uint64_t hi)
{
  long differing = 0;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t mag = scheme == 1 ? (uint32_t)i : (uint32_t)(2 * i + 3);
    for (unsigned positive = 0; positive < 2; positive++) {
      const uint64_t got = bits(dequant_signed(rule, coef_scheme_pack(mag, positive != 0, scheme)));
      differing += got != bits(ref_sample<uint32_t>(rule.q, mag, positive)) ||
                   got != bits(dequant_masks<uint32_t, uint64_t>(plain, mag, 0ull, 0ull, (uint64_t)positive, 0));
    }
  }
  return differing;
}
static void packed_exhaustive()
{
  const DecState s1 = state(31, 4, 3), s2 = state(32, 7, 4);
  const double q = next_q();
  const unsigned nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  for (int scheme = 1; scheme <= 2; scheme++) {
    const DecState& s = scheme == 1 ? s1 : s2;
    const DequantRule<uint32_t> rule = dequant_rule<uint32_t>(q, true, &s, true), plain = dequant_rule<uint32_t>(q, true, &s);
    const uint64_t n = scheme == 1 ? (1ull << 31) : (1ull << 31) - 1;
    std::vector<long> differing(nt, 0);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; t++)
      pool.emplace_back([&, t] { differing[t] = exhaustive_range(rule, plain, scheme, n * t / nt, n * (t + 1) / nt); });
    long sum = 0;
    for (unsigned t = 0; t < nt; t++) {
      pool[t].join();
      sum += differing[t];
    }
    seen += (long)(2 * n);
    expect(sum == 0, scheme == 1 ? "every packed word, scheme 1" : "every packed word, scheme 2", (uint64_t)sum, 0, scheme);
  }
}
#endif

int main()
{
  const uint32_t e32[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  const uint64_t e64[] = {0ull, 1ull, 0x7fffffffull, 0x80000000ull, 0xffffffffull, (1ull << 53) - 1, 1ull << 53};
  masks_cases<uint32_t>(32, e32, 5, 0xffffffffu);
  masks_cases<uint64_t>(53, e64, 7, (1ull << 53) - 1);
  // found "on the plane above plane 31": no such plane, the value is 0 (and the sample a signed zero)
  {
    const DecState s = state(32, 31, 0);
    const DequantRule<uint32_t> rule = dequant_rule<uint32_t>(0.75, true, &s);
    expect(rule.fillOld == 0u && rule.fillNew == 0xbfffffffu, "fill at plane 31", rule.fillOld, rule.fillNew, 31);
    expect(bits(dequant_masks<uint32_t, uint64_t>(rule, 0u, 0ull, 1ull, 1ull, 0)) == bits(0.0), "+0", 0, 0, 31);
    expect(bits(dequant_masks<uint32_t, uint64_t>(rule, 0u, 0ull, 1ull, 0ull, 0)) == bits(-0.0), "-0", 0, 0, 31);
  }
  packed_cases();
#ifdef EXHAUSTIVE
  packed_exhaustive();
#endif
  expect(coef_scheme_mag(coef_scheme_pack(1u, true, 2), true) == 0u && coef_scheme_mag(coef_scheme_pack(3u, true, 2), true) == 3u,
         "scheme 2 below its domain", 0, 0, 2);
  printf("cases: %ld differing: %ld\n", seen, bad);
  return bad != 0;
}
"""

FLAGS = ["--cuda-host-only", "-O3", "-ffp-contract=off", "-std=c++17", "-Wno-unused-value", "-I", CSRC, "-I", os.path.join(ROOT, "include")]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan"])
def test_every_form_of_the_rule_matches_the_reference_statements(tmp_path, sanitize):
    src, exe = tmp_path / "dequant_host.hip", tmp_path / "dequant_host"
    src.write_text(PROGRAM)
    extra = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-DEXHAUSTIVE", "-pthread"]
    r = subprocess.run(["hipcc", *FLAGS, *extra, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0 and " differing: 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
