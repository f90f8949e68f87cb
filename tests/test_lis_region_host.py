"""CPU: the protocol half of the decoder's region kernels (sperr_amd/csrc/lis_region.h; k_lis_hi, k_lis_mx and the kernels
that read what they leave) and the run-time-arity token functions of lis_token.h, in a program of its own under the
address and undefined sanitizers (the host pass of hipcc: lis_token.h includes the HIP runtime's header).

The header's arithmetic compiles for the host; what the kernels add are the atomics, which the program replays one
claim after the other on plain counters (claim_births / claim_leaf below repeat region_claim_births / region_claim_leaf
line by line).  Over small arrays -- a shared part of 5 slots, segments of 3, 1 to 8 groups -- it draws random sequences
of claims of 1 to 4 slots per group, long enough that every segment and then the shared part run over, one claim that
straddles a segment's end among them, and checks that

  * every slot that is written is written once and lies inside the pitch;
  * after the groups have published their counts and the shared counter is clamped, the rank-to-slot walk over
    [0, total) gives exactly the slots that were written -- so none that the "may be written" test refused;
  * the pitch is the shared part plus the groups' segments, with the segment size carve_dec takes from the tree's sets.

The token functions: for n = 1 .. 8 children, all 2^16 values of the low 16 bits (upper bits zero, one, random) against
the bit-by-bit parse of tests/test_lis_token_host.py, and the leaf-event word packed and unpacked again."""
import os
import shutil
import subprocess

import pytest

from test_lis_token_host import PARSE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sperr_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "lis_region.h"
#include "lis_token.h"
using namespace sperrhip;

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static uint64_t next64()
{
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  return rng;
}
""" + PARSE + r"""
// ---- the segmented array
struct Counters {
  uint32_t count = 0, refused = 0xffffffffu;   // a workgroup's LDS counters
};

static uint32_t claim_births(const SegGroup& a, Counters& c, uint32_t& shared, uint32_t n)
{
  const uint32_t k = c.count;
  c.count += n;
  if (a.in_segment(k, n))
    return a.base + k;
  if (k < c.refused)
    c.refused = k;
  const uint32_t s = shared;
  shared += n;
  return s;
}

static uint32_t claim_leaf(const SegGroup& a, Counters& c, uint32_t& shared)
{
  const uint32_t k = c.count++;
  if (a.in_segment(k, 1u))
    return (a.base + k) & ~kSegOwn;
  const uint32_t s = shared++;
  return s < a.cap ? s : kSegNoSlot;
}

struct Tally {
  long bad = 0, trials = 0, claims = 0, straddles = 0, refusedSlots = 0, sharedOverruns = 0, written = 0;
};

// one sequence of claims over `groups` groups; leaf: claims of one through claim_leaf
static void run_sequence(uint32_t groups, bool leaf, Tally& t)
{
  const SegArray a{5u, 3u, groups};
  const uint32_t pitch = (uint32_t)a.pitch();
  t.bad += a.pitch() != 5u + 3u * groups;
  std::vector<int> written(pitch, 0);
  Counters cnt[kRegionGroups];
  uint32_t shared = 0;
  long asked = 0, put = 0, refusedHere = 0;
  // (claims of 1 to 4 slots: at full length about 15 slots a group against its 3, and 5 shared; shorter sequences
  //  stop before one or the other runs over)
  const uint32_t nclaims = 2u + (uint32_t)(next64() % (6u * groups + 7u));
  for (uint32_t i = 0; i < nclaims; i++) {
    uint32_t g = (uint32_t)(next64() % groups), n = leaf ? 1u : 1u + (uint32_t)(next64() & 3u);
    if (!leaf && i < 2) {   // group 0 asks for 2 and 2: the second claim straddles the end of its three slots
      g = 0;
      n = 2;
    }
    const SegGroup sg = seg_group(a, g);
    t.bad += (sg.base & ~kSegOwn) != a.base(g) || a.base(g) + a.seg > pitch;
    const uint32_t k = cnt[g].count;
    t.straddles += !leaf && k < a.seg && k + n > a.seg;
    t.claims++;
    asked += n;
    if (leaf) {
      const uint32_t slot = claim_leaf(sg, cnt[g], shared);
      if (slot == kSegNoSlot) {
        refusedHere++;
        continue;
      }
      t.bad += slot >= pitch || written[slot < pitch ? slot : 0];
      if (slot < pitch)
        written[slot] = 1;
      put++;
      continue;
    }
    const uint32_t first = claim_births(sg, cnt[g], shared, n);
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t slot = first + j;
      if (!sg.may_write(slot)) {
        refusedHere++;
        continue;
      }
      const uint32_t idx = slot & ~kSegOwn;
      t.bad += idx >= pitch || written[idx < pitch ? idx : 0];
      if (idx < pitch)
        written[idx] = 1;
      put++;
    }
  }
  t.bad += put + refusedHere != asked;
  t.refusedSlots += refusedHere;
  t.sharedOverruns += shared > a.cap;
  t.written += put;
  // what the kernels leave behind: the groups' counts (the words of groups that do not exist hold anything), the
  // clamped shared counter
  uint32_t groupCount[kRegionGroups];
  for (uint32_t g = 0; g < kRegionGroups; g++)
    groupCount[g] = g < groups ? a.published(cnt[g].count, cnt[g].refused) : 0xdeadu;
  const SegRanks r = a.ranks(a.shared_count(shared), groupCount);
  t.bad += (long)r.total() != put;
  std::vector<int> seen(pitch, 0);
  for (uint32_t kk = 0; kk < r.total(); kk++) {
    const uint32_t slot = a.slot_of_rank(r, kk);
    t.bad += slot >= pitch || !written[slot < pitch ? slot : 0] || seen[slot < pitch ? slot : 0];
    if (slot < pitch)
      seen[slot] = 1;
  }
  t.trials++;
}

static long check_segments()
{
  Tally t;
  for (uint32_t groups = 1; groups <= kRegionGroups; groups++)
    for (int rep = 0; rep < 400; rep++) {
      run_sequence(groups, false, t);
      run_sequence(groups, true, t);
    }
  // the sizing carve_dec does: the shared part holds every set (+ 8), a segment a sixteenth of that + 64
  for (size_t nsets : {(size_t)0, (size_t)7, (size_t)8, (size_t)585, (size_t)2396745}) {
    const SegArray a{(uint32_t)(nsets + 8), region_seg_slots(nsets), kRegionGroups};
    t.bad += region_seg_slots(nsets) != (nsets + 8) / 16 + 64;
    t.bad += a.pitch() != (nsets + 8) + (size_t)kRegionGroups * ((nsets + 8) / 16 + 64);
    t.bad += a.pitch() >= kSegOwn;
  }
  printf("segments: %ld sequences, %ld claims (%ld straddle a segment's end), %ld slots written, %ld refused, "
         "%ld sequences ran the shared part over, differing=%ld\n",
         t.trials, t.claims, t.straddles, t.written, t.refusedSlots, t.sharedOverruns, t.bad);
  // (the cases the checks are about did occur)
  return t.bad + (t.straddles == 0) + (t.refusedSlots == 0) + (t.sharedOverruns == 0);
}

// ---- the token functions
static long check_tokens()
{
  long bad = 0;
  for (uint32_t n = 1; n <= 8; n++)
    for (int upper = 0; upper < 3; upper++)
      for (uint32_t low = 0; low < 65536u; low++) {
        const uint32_t hi = upper == 0 ? 0u : upper == 1 ? 0xffffu : (uint32_t)next64() & 0xffffu;
        const uint32_t w[2] = {low | (hi << 16), (uint32_t)next64()};
        uint32_t s, g, s2, g2;
        Parse p{w, 0};
        p.pixels((int)n, s, g);
        split_pixels_n(w[0], n, s2, g2);
        bad += pixel_split_len_n(w[0], n) != p.pos || s2 != s || g2 != g || p.pos > 2 * n;
        if (n == 8)
          bad += pixel_split_len_n(w[0], n) != split8_len(w[0]);
      }
  printf("leaf parents of 1 .. 8 pixels: 8 x 3 x 65536 values, differing=%ld\n", bad);
  long badEv = 0;
  for (int i = 0; i < 100000; i++) {
    const uint64_t x = next64();
    const uint32_t fid = i == 0 ? 0xffffffffu : (uint32_t)x, sigm = (uint32_t)(x >> 32) & 0xffu, negm = (uint32_t)(x >> 40) & 0xffu;
    uint32_t f2, s2, g2;
    const uint64_t ev = leaf_event_pack(fid, sigm, negm);
    leaf_event_unpack(ev, f2, s2, g2);
    badEv += f2 != fid || s2 != sigm || g2 != negm || ev != ((uint64_t)fid | ((uint64_t)sigm << 32) | ((uint64_t)negm << 40));
  }
  printf("leaf-event words: 100000 round trips, differing=%ld\n", badEv);
  return bad + badEv;
}

int main()
{
  const long bad = check_segments() + check_tokens();
  printf("differing in all: %ld\n", bad);
  return bad != 0;
}
"""


def test_region_protocol_and_run_time_arity_tokens(tmp_path):
    src, exe = tmp_path / "lis_region_host.hip", tmp_path / "lis_region_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["hipcc", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wno-unused-value",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "differing in all: 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
