"""CPU: the token grammar of the decoder's list kernels (sperr_amd/csrc/lis_token.h) against a bit-by-bit parse.

A set found significant is split into its eight children, coded in order (src/SPECK3D_INT.cpp:140-212): a child is a test
bit -- which the last child does not have when none of its siblings was significant: it is significant -- followed, when
the child is significant, by its own code: a pixel's sign bit, a set's split.  The kernels never parse like that.  They
take the length of a 2x2x2 set's split and its pixel masks from the 32 stream bits at its start with shifts
(pixel_split_len, split8_pixels), and the length of a larger set's split from the tables of the class below
(parent_split_len: seven coded children, then the last with or without its test bit).  The header compiles for the
host with the library's flags; the program below

  * runs the 2x2x2 functions over all 2^16 values of the low 16 bits (a 2x2x2 split is at most 16 bits), with the upper
    16 bits all zero, all one and random: they must be ignored;
  * builds the tables T0/U0/T1/U1 serially with the helpers the kernels call, over random bit strings of 8192 bits
    (more than the 4096 + 1097 + 128 a block of k_lis_l2 looks at) at three densities of ones, and compares the split
    length of a class-1 and a class-2 set at every start position with a recursive bit-by-bit parse;
  * checks that no token is longer than the kernels' kL1MaxTok = 137 and kL2MaxTok = 1097."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# (tests/test_lis_region_host.py parses with it as well)
PARSE = r"""
// ---- the bit-by-bit parse
struct Parse {
  const uint32_t* w;
  uint32_t pos;
  uint32_t bit() { const uint32_t b = (w[pos >> 5] >> (pos & 31)) & 1u; pos++; return b; }
  // the split of a set of n pixels: significance and sign masks by pixel
  void pixels(int n, uint32_t& sigm, uint32_t& negm)
  {
    uint32_t counter = 0;
    sigm = negm = 0;
    for (int k = 0; k < n; k++) {
      const bool need_decide = counter != 0 || k + 1 != n;
      const uint32_t sig = need_decide ? bit() : 1u;
      if (sig) {
        counter++;
        sigm |= 1u << k;
        if (!bit())   // the sign bit: '1' is positive
          negm |= 1u << k;
      }
    }
  }
  // the split of a set of class cls (0: its children are pixels)
  void split(int cls)
  {
    if (cls == 0) {
      uint32_t s, n;
      pixels(8, s, n);
      return;
    }
    uint32_t counter = 0;
    for (int k = 0; k < 8; k++) {
      const bool need_decide = counter != 0 || k != 7;
      if (need_decide ? bit() : 1u) {
        counter++;
        split(cls - 1);
      }
    }
  }
};
"""

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "lis_token.h"
using namespace sperrhip;

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static uint64_t next64()
{
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  return rng;
}

""" + PARSE + r"""
static long check_pixels()
{
  long bad = 0;
  for (int upper = 0; upper < 3; upper++)
    for (uint32_t low = 0; low < 65536u; low++) {
      const uint32_t hi = upper == 0 ? 0u : upper == 1 ? 0xffffu : (uint32_t)next64() & 0xffffu;
      const uint32_t w[2] = {low | (hi << 16), (uint32_t)next64()};
      uint32_t s, n, s2, n2;
      Parse p8{w, 0};
      p8.pixels(8, s, n);
      split8_pixels(w[0], s2, n2);
      bad += split8_len(w[0]) != p8.pos || s2 != s || n2 != n || p8.pos > 16;
      Parse p4{w, 0}, p2{w, 0};
      p4.pixels(4, s, n);
      p2.pixels(2, s, n);
      bad += pixel_split_len<4>(w[0]) != p4.pos || pixel_split_len<2>(w[0]) != p2.pos;
    }
  printf("2x2x2 splits: 3 x 65536 values, differing=%ld\n", bad);
  return bad;
}

constexpr uint32_t NBITS = 8192, P0 = NBITS - 32, P1 = P0 - 137, P2 = P1 - 1097;
static_assert(NBITS >= 4096 + 1097 + 128 && P2 >= 4096, "a block of k_lis_l2 and what its tokens reach");

static long check_tables(double ones, uint32_t& max1, uint32_t& max2)
{
  std::vector<uint32_t> w(NBITS / 32 + 2, 0u);
  for (uint32_t r = 0; r < NBITS; r++)
    if ((double)(next64() >> 11) / 9007199254740992.0 < ones)
      w[r >> 5] |= 1u << (r & 31);
  const LdsBits bits{w.data(), 0};
  // the tables, the way the kernels fill them: T = split of a set that starts here, U = a coded item that starts here
  std::vector<uint8_t> T0(P0), U0(P0), T1(P1), U1(P1);
  for (uint32_t r = 0; r < P0; r++)
    T0[r] = (uint8_t)split8_len(bits.bits32(r));
  for (uint32_t r = 0; r < P0; r++)
    U0[r] = (uint8_t)((bits.bit_at(r) && r + 1 < P0) ? 1u + T0[r + 1] : 1u);
  for (uint32_t r = 0; r < P1; r++)
    T1[r] = (uint8_t)parent_split_len(U0.data(), T0.data(), r);
  for (uint32_t r = 0; r < P1; r++)
    U1[r] = (uint8_t)((bits.bit_at(r) && r + 1 < P1) ? 1u + T1[r + 1] : 1u);
  long bad = 0;
  uint32_t m1 = 0, m2 = 0;
  for (uint32_t r = 0; r + 1 < P1; r++) {
    Parse p{w.data(), r};
    p.split(1);
    const uint32_t len = parent_split_len(U0.data(), T0.data(), r);
    bad += len != p.pos - r;
    m1 = len > m1 ? len : m1;
  }
  for (uint32_t r = 0; r < P2; r++) {
    Parse p{w.data(), r};
    p.split(2);
    const uint32_t len = parent_split_len(U1.data(), T1.data(), r);
    bad += len != p.pos - r;
    m2 = len > m2 ? len : m2;
  }
  // a token is the entry's '1' and its split
  printf("ones=%.2f: longest class-1 token %u, class-2 token %u, differing=%ld\n", ones, 1 + m1, 1 + m2, bad);
  max1 = 1 + m1 > max1 ? 1 + m1 : max1;
  max2 = 1 + m2 > max2 ? 1 + m2 : max2;
  return bad;
}

int main()
{
  long bad = check_pixels();
  uint32_t max1 = 0, max2 = 0;
  for (int rep = 0; rep < 2; rep++)
    for (double ones : {0.05, 0.30, 0.60})
      bad += check_tables(ones, max1, max2);
  const bool within = max1 <= 137 && max2 <= 1097;
  printf("longest tokens %u / %u within 137 / 1097: %s\n", max1, max2, within ? "yes" : "NO");
  printf("differing in all: %ld\n", bad);
  return bad != 0 || !within;
}
"""


def test_token_grammar_matches_a_bit_by_bit_parse(tmp_path):
    src, exe = tmp_path / "lis_token_host.hip", tmp_path / "lis_token_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["hipcc", "--cuda-host-only", "-O3", "-ffp-contract=off", "-std=c++17", "-Wno-unused-value", "-I", CSRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "differing in all: 0" in r.stdout and "within 137 / 1097: yes" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-1000:]
