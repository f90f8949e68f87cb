"""CPU: the y and x passes of the fused finest-level kernels lift a row window by window (lift_window,
sperr_amd/csrc/lift_window.h).  A window of W samples gives W - 8 results; the kernels were written for W = 16 (lift16)
and now also run W = 12 and W = 10.  That this changes no bit rests on one claim: a result depends on the four samples
to each side of it and on nothing else, so it is the same whatever the width of the window and wherever in the window's
middle it lies.  The header compiles for the host, with the library's flags (-ffp-contract=off): the program below
lifts random rows window by window, in both directions, at every width and every even window position, and compares
each result's bits with lift16's at two different positions of the 16-sample window."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "lift_window.h"
using namespace sperrhip;

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static double next_sample()
{
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  const double u = (double)(rng >> 11) / 9007199254740992.0 - 0.5;
  return u * ((rng & 7) == 0 ? 1e6 : (rng & 7) == 1 ? 1e-6 : 1.0);
}

static const LiftConsts K = {-1.58613434201888022056773, -0.05298011857604780601431, 0.88291107549260031282806,
                             0.44350685204939829327158, 1.14960439885900000000000, 1.0 / 1.14960439885900000000000};
constexpr int N = 300;   // the rows of the kernels have up to 256 samples and an apron of 4 on each side
static double row[N];

template <bool FWD>
static void ref16(int start, double (&r)[16])
{
  memcpy(r, row + start, sizeof r);
  lift16<FWD>(r, K);
}

template <bool FWD, int W>
static long check()
{
  long bad = 0, seen = 0;
  for (int s = 4; s + 20 <= N; s += 2) {
    double w[W], a[16], b[16];
    memcpy(w, row + s, sizeof w);
    lift_window<FWD, W>(w, K);
    ref16<FWD>(s, a);       // the same sample is result 4 + k of this window
    ref16<FWD>(s - 4, b);   // ... and result 8 + k of this one (k < 4)
    for (int k = 0; k < W - 8; k++) {
      bad += memcmp(&w[4 + k], &a[4 + k], 8) != 0;
      if (k < 4)
        bad += memcmp(&w[4 + k], &b[8 + k], 8) != 0;
      seen++;
    }
  }
  printf("%s W=%d results=%ld differing=%ld\n", FWD ? "forward" : "inverse", W, seen, bad);
  return bad;
}

int main()
{
  long bad = 0;
  for (int rep = 0; rep < 50; rep++) {
    for (int i = 0; i < N; i++)
      row[i] = next_sample();
    bad += check<true, 10>() + check<true, 12>() + check<true, 14>() + check<true, 16>();
    bad += check<false, 10>() + check<false, 12>() + check<false, 14>() + check<false, 16>();
  }
  printf("differing in all: %ld\n", bad);
  return bad != 0;
}
"""


def test_window_results_do_not_depend_on_the_window(tmp_path):
    src, exe = tmp_path / "lift_window_host.hip", tmp_path / "lift_window_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["hipcc", "--cuda-host-only", "-O3", "-ffp-contract=off", "-std=c++17", "-Wno-unused-value", "-I", CSRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "differing in all: 0" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
