// slice_forest_check.cpp -- host only: every slice's forest (spk::build_tree(x, y, 1, twoD)) fits k_lis_mx, the
// only list kernel with the 2D coder's type-I phase.  Checks the structural conditions use_mixed() and use_tables()
// (engine.hip) test, for every "x y" line of the shape file, and prints the largest counts it met.
//   slice_forest_check SHAPES.txt NTHREADS  -> exit 0: all shapes pass; 1: the failing shapes are listed
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "speck_tree_host.hpp"

int main(int argc, char** argv)
{
  if (argc < 3)
    return 2;
  std::vector<std::pair<size_t, size_t>> shapes;
  FILE* f = fopen(argv[1], "r");
  if (!f)
    return 2;
  size_t x, y;
  while (fscanf(f, "%zu %zu", &x, &y) == 2)
    shapes.push_back({x, y});
  fclose(f);
  const int nthreads = std::max(1, atoi(argv[2]));
  std::atomic<size_t> next{0}, bad{0};
  std::mutex m;
  size_t maxRoots = 0, maxGrids = 0, maxCls = 0;
  auto work = [&]() {
    for (size_t i = next++; i < shapes.size(); i = next++) {
      const spk::HostTree h = spk::build_tree(shapes[i].first, shapes[i].second, 1, /*twoD=*/true);
      const bool ok = !h.cls.empty() && h.roots.size() <= 48 && h.grids.size() <= 352 &&
                      h.mxSlot.size() == h.cls.size() && !h.allRegular && (h.flags & spk::kTree2D);
      std::lock_guard<std::mutex> g(m);
      maxRoots = std::max(maxRoots, h.roots.size());
      maxGrids = std::max(maxGrids, h.grids.size());
      maxCls = std::max(maxCls, h.cls.size());
      if (!ok) {
        bad++;
        printf("FAIL %zu x %zu: cls %zu roots %zu grids %zu mxSlot %zu allRegular %d flags %u\n", shapes[i].first,
               shapes[i].second, h.cls.size(), h.roots.size(), h.grids.size(), h.mxSlot.size(), (int)h.allRegular,
               h.flags);
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; t++)
    pool.emplace_back(work);
  for (auto& t : pool)
    t.join();
  printf("shapes %zu failed %zu max_roots %zu max_grids %zu max_cls %zu\n", shapes.size(), bad.load(), maxRoots,
         maxGrids, maxCls);
  return bad ? 1 : 0;
}
