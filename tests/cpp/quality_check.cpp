// quality_check -- the host half of the device quality figures (sperr_amd/csrc/quality.h) without a GPU: block
// partials formed with plain loops from quality_plan, fed to quality_finish, and compared bit for bit with
// sperr::calc_stats / sperr::calc_mean_var of include/compat/sperr_helper.h.
//
//   quality_check plan                   checks quality_plan at the block edges
//   quality_check f32|f64 a.bin b.bin    prints the eight figures as hex bit patterns, one line
//
// Exit code 0: everything agreed.  Built with -ffp-contract=off and the address / undefined sanitizers.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "quality.h"
#include "sperr_helper.h"

using sperrhip::quality_plan;
using sperrhip::QualityPlan;

static int fails = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      fails++;                                                         \
    }                                                                  \
  } while (0)

static void check_plan()
{
  struct Want { size_t n, sqb, sqt, mvb, mvt; };
  const Want want[] = {{0, 0, 0, 0, 0},          {1, 0, 1, 0, 1},          {8191, 0, 8191, 0, 8191},
                       {8192, 1, 0, 0, 8192},    {8193, 1, 1, 0, 8193},    {16384, 2, 0, 1, 0},
                       {16385, 2, 1, 1, 1},      {(size_t(1) << 33) + 5, size_t(1) << 20, 5, size_t(1) << 19, 5}};
  for (const Want& w : want) {
    const QualityPlan p = quality_plan(w.n);
    CHECK(p.n == w.n && p.sq_blocks == w.sqb && p.sq_tail == w.sqt && p.mv_blocks == w.mvb && p.mv_tail == w.mvt);
    CHECK(p.sq_partials() == w.sqb + 1 && p.mv_partials() == w.mvb + 1);
    CHECK(p.sq_blocks * sperrhip::kQualSqBlock + p.sq_tail == w.n);
    CHECK(p.mv_blocks * sperrhip::kQualMvBlock + p.mv_tail == w.n);
  }
}

template <typename T>
static uint64_t bits(T v)
{
  typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type u;
  std::memcpy(&u, &v, sizeof(T));
  return u;
}

// sum of f(i) over one block, left to right
template <typename T, typename F>
static T block_sum(size_t lo, size_t hi, F f)
{
  T s = 0;
  for (size_t i = lo; i < hi; i++)
    s += f(i);
  return s;
}

template <typename T>
static int check_pair(const char* fa, const char* fb)
{
  const std::vector<T> a = sperr::read_whole_file<T>(fa), b = sperr::read_whole_file<T>(fb);
  if (a.empty() || a.size() != b.size()) {
    std::printf("cannot read the arrays\n");
    return 2;
  }
  const size_t n = a.size();
  const QualityPlan plan = quality_plan(n);
  auto partials = [&](size_t block, size_t blocks, auto f) {
    std::vector<T> p;
    for (size_t k = 0; k < blocks; k++)
      p.push_back(block_sum<T>(k * block, (k + 1) * block, f));
    p.push_back(block_sum<T>(blocks * block, n, f));   // the tail block, possibly empty
    return p;
  };
  const std::vector<T> sq = partials(sperrhip::kQualSqBlock, plan.sq_blocks, [&](size_t i) {
    const T d = std::abs(a[i] - b[i]);
    return d * d;
  });
  const std::vector<T> as = partials(sperrhip::kQualMvBlock, plan.mv_blocks, [&](size_t i) { return a[i]; });
  const T mean = sperrhip::quality_sum_partials(as.data(), as.size()) / T(n);
  const std::vector<T> var =
      partials(sperrhip::kQualMvBlock, plan.mv_blocks, [&](size_t i) { return (a[i] - mean) * (a[i] - mean); });
  CHECK(sq.size() == plan.sq_partials() && as.size() == plan.mv_partials() && var.size() == plan.mv_partials());
  T linf = 0, lo = a[0], hi = a[0];
  bool differ = false;
  for (size_t i = 0; i < n; i++) {
    linf = std::max(linf, std::abs(a[i] - b[i]));
    lo = std::min(lo, a[i]);
    hi = std::max(hi, a[i]);
    differ |= a[i] != b[i];
  }
  const sperrhip::QualityPartials<T> p{sq.data(), var.data(), mean, linf, lo, hi, differ};
  const std::array<T, 8> f = sperrhip::quality_finish(plan, p);

  const std::array<T, 5> st = sperr::calc_stats(a.data(), b.data(), n);
  const std::array<T, 2> mv = sperr::calc_mean_var(a.data(), n);
  for (int k = 0; k < 5; k++)
    if (k == 3 || k == 4)
      CHECK(f[k] == st[k]);                    // min, max: by value (the sign of a zero is not pinned)
    else
      CHECK(bits(f[k]) == bits(st[k]));
  CHECK(bits(f[5]) == bits(mv[0]) && bits(f[6]) == bits(mv[1]));
  CHECK(bits(std::sqrt(f[7])) == bits(f[0]));  // mse is the value rmse is the root of
  for (int k = 0; k < 8; k++)
    std::printf("%" PRIx64 "%c", bits(f[k]), k == 7 ? '\n' : ' ');
  return 0;
}

int main(int argc, char** argv)
{
  int rtn = 2;
  if (argc == 2 && std::string(argv[1]) == "plan") {
    check_plan();
    rtn = 0;
  }
  else if (argc == 4 && std::string(argv[1]) == "f32")
    rtn = check_pair<float>(argv[2], argv[3]);
  else if (argc == 4 && std::string(argv[1]) == "f64")
    rtn = check_pair<double>(argv[2], argv[3]);
  else
    std::printf("usage: quality_check plan | f32|f64 a.bin b.bin\n");
  if (rtn == 0 && fails == 0 && argc == 2)
    std::printf("ok\n");
  return rtn ? rtn : (fails ? 1 : 0);
}
