// budget.h -- the size mode's DEAL: a byte target of a whole volume into one budget per chunk, so that all chunks stop
// at (nearly) the same ABSOLUTE threshold.  The ONLY statement of the rule: the kernel k_budget_deal (encode.hip), the
// host check tests/cpp/size_check.cpp and, in numpy, tests/size_model.py (which states it again; every budget is
// compared).  Plain C++: no HIP here.
//
// Fixed-rate mode gives every chunk the same bits per sample and quantises each with a step of its own,
// q_c = maxabs_c / (2^32 - 1): every chunk then stops at the same depth RELATIVE to its largest coefficient.  A chunk's
// stream is embedded, and coding plane p to its end leaves an error of the order of the threshold q_c 2^p.  The deal
// stops all chunks at the same threshold instead.
//
//   inputs    per chunk c that is not constant: the step q_c, the plane count nbp_c (at most kBudgetPlanes) and the plane
//             table end_c[p], p in [0, nbp_c): the stream's bits at the end of plane p under an unlimited budget
//             (launch_speck_plane_table); end_c[nbp_c] := 0.  W: the bits there are for the payloads,
//               W = 8 (target - container header - 26 #nonconst - 17 #const)                        (budget_payload_bits)
//             refused when the header and the chunk headers do not fit, or W < 8 #nonconst
//   depth     P_c(T) = the smallest p >= 0 with ldexp(q_c, p) >= T, capped at nbp_c: the planes >= P_c(T) are the ones
//             whose threshold is at least T.  F_c(T) = max(8, end_c[P_c(T)]).  Compared with ldexp and >= only
//   T*        the candidates are all ldexp(q_c, p), p in [0, nbp_c), distinct, in descending order, behind a first one
//             of +infinity (every chunk at the 8-bit floor, which the refusal above makes fit).  sum_c F_c(T) grows as T
//             falls; T* is the last candidate with sum_c F_c(T*) <= W
//   the rest  T' is the next candidate below T* (none: every chunk is coded in full).  rem = W - sum_c F_c(T*) goes to
//             the chunks whose next plane's threshold is T', in proportion to those planes' sizes,
//               plane_c = F_c(T') - F_c(T*),   share_c = min(plane_c, floor(rem plane_c / sum plane))
//             (replicated chunks share a q: a homogeneous volume comes out nearly uniform)
//   rounding  budget_c = max(8, 8 floor(min(F_c(T*) + share_c, end_c[0]) / 8)): a multiple of 8 bits, never beyond the
//             chunk's full depth -- except for the floor of 8 bits, one payload byte, of a chunk whose whole stream is
//             shorter than that.  A constant chunk gets 0
//
// sum_c budget_c <= W, and it falls short of W by less than 8 bits a chunk (the rounding down, and the floors of the
// shares, which sum to less than one bit a tied chunk) unless every chunk is coded in full.
//
// How T* is found.  Positive doubles order like their bit patterns.  S(T) = sum_c F_c(T) is a step function that rises
// exactly AT the candidates (P_c falls when T reaches ldexp(q_c, p) from above), so {T : S(T) > W} is (0, T'] with T' a
// candidate: the largest bit pattern with S > W, found by bisection between the smallest and the largest candidate --
// 64 sums over the chunks, no sort.  T* is the smallest candidate above T'.  The sums are taken by a TEAM: one thread on
// the host, a workgroup in the kernel (the same code: every member walks its share of the chunks and the team adds up).
#ifndef SPERR_AMD_BUDGET_H
#define SPERR_AMD_BUDGET_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BUDGET_HD __host__ __device__ inline
#else
#define BUDGET_HD inline
#endif

namespace sperrhip {

constexpr int kBudgetPlanes = 32;   // planes of the 32-bit coefficient pass: a table row

// the table of a volume, one entry per chunk (a constant chunk's q, nbp and row are not read)
struct BudgetTable {
  uint32_t nchunks;
  const double* q;
  const int32_t* nbp;
  const uint64_t* end;        // [nchunks][kBudgetPlanes]
  const uint8_t* is_const;
};

// one member of the team that takes the sums; the host's team of one
struct BudgetSolo {
  uint32_t rank = 0, size = 1;
  uint64_t sum(uint64_t v) { return v; }
  uint64_t min(uint64_t v) { return v; }
  uint64_t max(uint64_t v) { return v; }
};

BUDGET_HD uint64_t budget_bits_of(double v)
{
  uint64_t u;
  __builtin_memcpy(&u, &v, 8);
  return u;
}
BUDGET_HD double budget_double_of(uint64_t u)
{
  double v;
  __builtin_memcpy(&v, &u, 8);
  return v;
}
constexpr uint64_t kBudgetInfBits = 0x7ff0000000000000ull;

// bytes of a container's header in front of its chunk streams (SPERR3D_OMP_C.cpp:163-234)
BUDGET_HD uint64_t budget_header_bytes(uint64_t nchunks)
{
  return (nchunks > 1 ? 20ull : 14ull) + 4ull * nchunks;
}

// W; false: the target does not hold the headers and a payload byte per chunk that is not constant
BUDGET_HD bool budget_payload_bits(uint64_t target_bytes, uint64_t nchunks, uint64_t nconst, uint64_t* W)
{
  const uint64_t nonconst = nchunks - nconst;
  const uint64_t fixed = budget_header_bytes(nchunks) + 26ull * nonconst + 17ull * nconst;
  if (target_bytes < fixed || target_bytes - fixed < nonconst)
    return false;
  *W = 8ull * (target_bytes - fixed);
  return true;
}

// P_c(T)
BUDGET_HD int budget_depth(double q, int nbp, double T)
{
  int p = 0;
  while (p < nbp && !(ldexp(q, p) >= T))
    p++;
  return p;
}

// F_c(T); row: the chunk's kBudgetPlanes table entries
BUDGET_HD uint64_t budget_floor_bits(const uint64_t* row, double q, int nbp, double T)
{
  const int p = budget_depth(q, nbp, T);
  const uint64_t e = p < nbp ? row[p] : 0ull;
  return e < 8ull ? 8ull : e;
}

// floor(a b / d), d > 0, a b / d < 2^64: the 128-bit product, then a division bit by bit
BUDGET_HD uint64_t budget_muldiv(uint64_t a, uint64_t b, uint64_t d)
{
  const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
  uint64_t lo = (p00 & 0xffffffffull) | (mid << 32);
  uint64_t hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  if (hi == 0)
    return lo / d;
  uint64_t r = 0, quo = 0;   // (r < d <= 2^63 is not assumed: the carry out of r is kept)
  for (int k = 127; k >= 0; k--) {
    const uint64_t carry = r >> 63;
    r = (r << 1) | (hi >> 63);
    hi = (hi << 1) | (lo >> 63);
    lo <<= 1;
    quo <<= 1;
    if (carry || r >= d) {
      r -= d;
      quo |= 1ull;
    }
  }
  return quo;
}

// S(T) over the team
template <class Team>
BUDGET_HD uint64_t budget_sum(const BudgetTable& t, double T, Team& team)
{
  uint64_t s = 0;
  for (uint32_t c = team.rank; c < t.nchunks; c += team.size)
    if (!t.is_const[c])
      s += budget_floor_bits(t.end + (size_t)c * kBudgetPlanes, t.q[c], t.nbp[c], T);
  return team.sum(s);
}

// The deal.  budgets[c] for every chunk (written by the member that owns c); thresholds[0..1] = the bit patterns of T*
// and T' (+infinity: every chunk at the floor; 0: no plane is left), written by rank 0 when not null.  Every member of
// the team calls it with the same arguments.  0 ok, -1: W < 8 #nonconst
template <class Team>
BUDGET_HD int budget_deal(const BudgetTable& t, uint64_t W, uint64_t* budgets, uint64_t* thresholds, Team& team)
{
  // the candidates' range; a chunk takes part when it has a plane and a step one can scale
  uint64_t cnt = 0, loBits = ~0ull, hiBits = 0;
  for (uint32_t c = team.rank; c < t.nchunks; c += team.size) {
    if (t.is_const[c])
      continue;
    cnt++;
    const double q = t.q[c];
    if (t.nbp[c] > 0 && q > 0.0 && budget_bits_of(ldexp(q, t.nbp[c] - 1)) < kBudgetInfBits) {
      const uint64_t a = budget_bits_of(q), b = budget_bits_of(ldexp(q, t.nbp[c] - 1));
      loBits = a < loBits ? a : loBits;
      hiBits = b > hiBits ? b : hiBits;
    }
  }
  cnt = team.sum(cnt);
  loBits = team.min(loBits);
  hiBits = team.max(hiBits);
  if (W < 8ull * cnt)
    return -1;
  uint64_t starBits = kBudgetInfBits, nextBits = 0;   // T*, T'
  if (loBits <= hiBits) {
    if (budget_sum(t, budget_double_of(loBits), team) <= W)
      starBits = loBits;   // every plane of every chunk fits
    else {
      uint64_t l = loBits, h = hiBits + 1;   // S(l) > W; S(h) <= W, h = hiBits + 1 standing for +infinity
      if (budget_sum(t, budget_double_of(hiBits), team) > W)
        l = hiBits;
      while (h - l > 1) {
        const uint64_t mid = l + (h - l) / 2;
        if (budget_sum(t, budget_double_of(mid), team) > W)
          l = mid;
        else
          h = mid;
      }
      nextBits = l;
      // T*: the smallest candidate above T'
      const double Tn = budget_double_of(nextBits);
      uint64_t best = kBudgetInfBits;
      for (uint32_t c = team.rank; c < t.nchunks; c += team.size) {
        // (the chunks that have candidates: as above)
        if (t.is_const[c] || !(t.q[c] > 0.0) || t.nbp[c] <= 0 ||
            !(budget_bits_of(ldexp(t.q[c], t.nbp[c] - 1)) < kBudgetInfBits))
          continue;
        for (int p = 0; p < t.nbp[c]; p++) {
          const double v = ldexp(t.q[c], p);
          if (v > Tn) {
            const uint64_t vb = budget_bits_of(v);
            best = vb < best ? vb : best;
            break;
          }
        }
      }
      starBits = team.min(best);
    }
  }
  const double Ts = budget_double_of(starBits), Tn = budget_double_of(nextBits);
  // the rest: what is left of W, and the sizes of the planes it goes to
  uint64_t base = 0, planes = 0;
  for (uint32_t c = team.rank; c < t.nchunks; c += team.size) {
    if (t.is_const[c])
      continue;
    const uint64_t* row = t.end + (size_t)c * kBudgetPlanes;
    const uint64_t f0 = budget_floor_bits(row, t.q[c], t.nbp[c], Ts);
    base += f0;
    if (nextBits)
      planes += budget_floor_bits(row, t.q[c], t.nbp[c], Tn) - f0;
  }
  base = team.sum(base);
  planes = team.sum(planes);
  const uint64_t rem = W - base;   // (S(T*) <= W)
  for (uint32_t c = team.rank; c < t.nchunks; c += team.size) {
    if (t.is_const[c]) {
      budgets[c] = 0;
      continue;
    }
    const uint64_t* row = t.end + (size_t)c * kBudgetPlanes;
    uint64_t b = budget_floor_bits(row, t.q[c], t.nbp[c], Ts);
    if (nextBits && planes) {
      const uint64_t plane = budget_floor_bits(row, t.q[c], t.nbp[c], Tn) - b;
      const uint64_t share = budget_muldiv(rem, plane, planes);
      b += share < plane ? share : plane;
    }
    const uint64_t full = t.nbp[c] > 0 ? row[0] : 0ull;
    b = b < full ? b : full;
    b &= ~7ull;
    budgets[c] = b < 8ull ? 8ull : b;
  }
  if (thresholds && team.rank == 0) {
    thresholds[0] = starBits;
    thresholds[1] = nextBits;
  }
  return 0;
}

}  // namespace sperrhip
#endif
