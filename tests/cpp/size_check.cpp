// size_check.cpp -- sperr_amd/csrc/budget.h as host C++ (tests/test_size_host.py builds it with
// -fsanitize=address,undefined): the deal of a table read from a file, for every W given, printed for the test to compare
// with tests/size_model.py; and, without arguments, the header's small parts against plain statements.
//
//   size_check TABLE W...     TABLE: u64 n, then n doubles q, n i32 nbp, n * 32 u64 end, n u8 is_const (native endian)
//                             one line per W: "W <W> rc <rc> T <bits of T*> <bits of T'> :" and the n budgets
//   size_check payload TARGET NCHUNKS NCONST     "W <bits>" or "refused"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "budget.h"

using namespace sperrhip;

static int fail(const char* what)
{
  printf("size_check FAILED: %s\n", what);
  return 1;
}

static int self_check()
{
  // muldiv against unsigned __int128 (the host has it; the kernel does not)
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  for (int k = 0; k < 200000; k++) {
    const int sa = (int)(next() % 64), sb = (int)(next() % 64);
    uint64_t a = next() >> sa, b = next() >> sb, d = (next() >> (next() % 64)) | 1ull;
    if (k % 7 == 0)
      d = b ? b : 1;   // (the quotient is a)
    const unsigned __int128 prod = (unsigned __int128)a * b;
    if ((uint64_t)((prod / d) >> 64) != 0)
      continue;   // (outside the function's domain)
    if (budget_muldiv(a, b, d) != (uint64_t)(prod / d))
      return fail("budget_muldiv");
  }
  if (budget_muldiv(~0ull, ~0ull, ~0ull) != ~0ull || budget_muldiv(0, 5, 3) != 0 || budget_muldiv(7, 1ull << 63, 1ull << 63) != 7)
    return fail("budget_muldiv edge");
  // P_c(T): the smallest p with q 2^p >= T, capped
  if (budget_depth(1.0, 5, 4.0) != 2 || budget_depth(1.0, 5, 4.0000001) != 3 || budget_depth(1.0, 5, 1e9) != 5 ||
      budget_depth(1.0, 5, 0.5) != 0 || budget_depth(3.0, 0, 1.0) != 0 ||
      budget_depth(1.0, 5, budget_double_of(kBudgetInfBits)) != 5)
    return fail("budget_depth");
  uint64_t W = 0;
  if (budget_payload_bits(20 + 8 + 26 + 17 + 1, 2, 1, &W) != true || W != 8 || budget_payload_bits(20 + 8 + 26 + 17, 2, 1, &W) ||
      budget_payload_bits(3, 1, 0, &W) || budget_header_bytes(1) != 18 || budget_header_bytes(8) != 52)
    return fail("budget_payload_bits");
  printf("size_check ok\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 1)
    return self_check();
  if (argc == 5 && !strcmp(argv[1], "payload")) {
    uint64_t W = 0;
    if (budget_payload_bits(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), &W))
      printf("W %" PRIu64 "\n", W);
    else
      printf("refused\n");
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return fail("cannot open the table");
  uint64_t n = 0;
  if (fread(&n, 8, 1, f) != 1 || n > (1u << 20))
    return fail("table header");
  std::vector<double> q(n);
  std::vector<int32_t> nbp(n);
  std::vector<uint64_t> end(n * kBudgetPlanes);
  std::vector<uint8_t> ic(n);
  if (fread(q.data(), 8, n, f) != n || fread(nbp.data(), 4, n, f) != n || fread(end.data(), 8, n * kBudgetPlanes, f) != n * kBudgetPlanes ||
      fread(ic.data(), 1, n, f) != n)
    return fail("table body");
  fclose(f);
  const BudgetTable t{(uint32_t)n, q.data(), nbp.data(), end.data(), ic.data()};
  for (int a = 2; a < argc; a++) {
    const uint64_t W = strtoull(argv[a], nullptr, 10);
    std::vector<uint64_t> budgets(n, ~0ull);
    uint64_t thr[2] = {0, 0};
    BudgetSolo solo;
    const int rc = budget_deal(t, W, budgets.data(), thr, solo);
    printf("W %" PRIu64 " rc %d T %" PRIu64 " %" PRIu64 " :", W, rc, thr[0], thr[1]);
    if (rc == 0)
      for (uint64_t c = 0; c < n; c++)
        printf(" %" PRIu64, budgets[c]);
    printf("\n");
  }
  return 0;
}
