// Host check of sperr_amd/csrc/view.h, the one statement of what a strided view is: the validity rule with its
// refusals and its overflow guards, the extent, and the index-to-address map -- view_offset, and the cursor the
// quality kernel walks with -- against three nested loops.  tests/test_view_host.py builds it under the address and
// undefined sanitizers and runs it; it prints "view_check ok" and returns 0 when everything holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "view.h"

using namespace sperrhip;

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      failures++;                                                  \
    }                                                              \
  } while (0)

static void check_rule()
{
  const size_t big = SIZE_MAX;
  size_t e = 0;
  // the dense volume, and a padded one
  CHECK(view_valid(40, 48, 56, view_dense(40, 48)));
  CHECK(view_extent(40, 48, 56, view_dense(40, 48), &e) && e == size_t(40) * 48 * 56);
  CHECK(view_extent(40, 48, 56, ViewPitch{47, 47 * 52}, &e) && e == size_t(55) * 47 * 52 + 47 * 47 + 40);
  CHECK(view_extent(1, 1, 1, ViewPitch{1, 1}, &e) && e == 1);
  CHECK(view_extent(1, 1, 1, ViewPitch{9, 27}, &e) && e == 1);
  CHECK(view_extent(5, 1, 3, ViewPitch{7, 21}, &e) && e == 2 * 21 + 5);
  // every refusal: an empty dim, rows that overlap, slices that overlap, a slice pitch that is no multiple of the rows'
  CHECK(!view_valid(0, 4, 4, ViewPitch{4, 16}));
  CHECK(!view_valid(4, 0, 4, ViewPitch{4, 16}));
  CHECK(!view_valid(4, 4, 0, ViewPitch{4, 16}));
  CHECK(!view_valid(4, 4, 4, ViewPitch{3, 16}));
  CHECK(!view_valid(4, 4, 4, ViewPitch{0, 0}));
  CHECK(!view_valid(4, 4, 4, ViewPitch{5, 19}));
  CHECK(view_valid(4, 4, 4, ViewPitch{5, 20}));
  CHECK(!view_valid(4, 4, 4, ViewPitch{5, 21}));
  CHECK(!view_valid(4, 4, 4, ViewPitch{5, 24}));
  CHECK(view_valid(4, 4, 4, ViewPitch{5, 25}));
  CHECK(!view_valid(40, 48, 56, ViewPitch{47, 47 * 52 + 1}));
  // sizes around SIZE_MAX: pitch_y * dimy, (dimz - 1) * pitch_z and the sums, each just below and just above
  const size_t half = (big >> 1) + 1;   // 2^63
  CHECK(!view_valid(1, 2, 1, ViewPitch{half, half}));              // pitch_y * dimy = 2^64
  CHECK(view_extent(1, 1, 1, ViewPitch{big, big}, &e) && e == 1);
  CHECK(view_extent(1, 1, 2, ViewPitch{big - 1, big - 1}, &e) && e == big);   // the largest extent there is
  CHECK(!view_valid(2, 1, 2, ViewPitch{big - 1, big - 1}));        // ... plus one
  CHECK(!view_valid(1, 1, 3, ViewPitch{half, half}));              // (dimz - 1) * pitch_z = 2^64
  CHECK(view_extent(1, 1, 2, ViewPitch{half, half}, &e) && e == half + 1);
  CHECK(!view_valid(1, 2, 2, ViewPitch{half / 2 - 1, half - 1}));   // pitch_z = 2 pitch_y + 1: no multiple
  CHECK(view_extent(1, 2, 2, ViewPitch{half / 2 - 1, half - 2}, &e) && e == half - 2 + half / 2 - 1 + 1);
  CHECK(!view_valid(4, 2, 3, ViewPitch{half / 2, half}));          // 2 * 2^63
  CHECK(!view_valid(half, 1, 1, ViewPitch{half - 1, half}));
  // a capacity is compared with the extent, in elements of the type
  CHECK(view_fits(40, 48, 56, ViewPitch{47, 47 * 52}, 4, (size_t(55) * 47 * 52 + 47 * 47 + 40) * 4));
  CHECK(!view_fits(40, 48, 56, ViewPitch{47, 47 * 52}, 4, (size_t(55) * 47 * 52 + 47 * 47 + 40) * 4 - 1));
  CHECK(!view_fits(40, 48, 56, ViewPitch{47, 47 * 52}, 8, (size_t(55) * 47 * 52 + 47 * 47 + 40) * 8 - 8));
  CHECK(!view_fits(4, 4, 4, ViewPitch{5, 21}, 4, big));
  // the helpers
  size_t r = 0;
  CHECK(view_mul(big, 1, &r) && r == big);
  CHECK(!view_mul(big, 2, &r));
  CHECK(view_mul(0, big, &r) && r == 0);
  CHECK(view_add(big - 1, 1, &r) && r == big);
  CHECK(!view_add(big, 1, &r));
}

// the map against three nested loops over a parent that is touched nowhere else: every element of the view is met
// once, in order, inside the extent
static void check_map(size_t dx, size_t dy, size_t dz, ViewPitch p)
{
  size_t ext = 0;
  CHECK(view_extent(dx, dy, dz, p, &ext));
  std::vector<uint8_t> hit(ext, 0);
  const ViewWalk w = view_walk(dx, dy, p);
  ViewCursor one = view_cursor(0, w);   // walks element by element
  size_t i = 0;
  for (size_t z = 0; z < dz; z++)
    for (size_t y = 0; y < dy; y++)
      for (size_t x = 0; x < dx; x++, i++) {
        const size_t want = z * p.z + y * p.y + x;
        CHECK(want < ext);
        CHECK(view_offset(i, dx, dy, p) == want);
        CHECK(one.row + one.x == want && one.x == x && one.y == y);
        const ViewCursor placed = view_cursor(i, w);
        CHECK(placed.x == one.x && placed.y == one.y && placed.row == one.row);
        hit[want]++;
        view_next(one, w);
      }
  size_t met = 0;
  for (uint8_t h : hit) {
    CHECK(h <= 1);
    met += h;
  }
  CHECK(met == dx * dy * dz && hit[ext - 1] == 1 && hit[0] == 1);
  // steps as the kernel takes them (a segment of 128, a pack, and odd ones) from every 37th start; a cursor may
  // come to stand behind the last element, where it is compared but never read
  const size_t n = dx * dy * dz;
  for (uint32_t step : {128u, 1u, 2u, 4u, 3u, 16384u, 20001u})
    for (size_t s = 0; s < n; s += 37) {
      ViewCursor c = view_cursor(s, w);
      for (size_t at = s + step, k = 0; k < 6; at += step, k++) {
        view_advance(c, w, step);
        const ViewCursor ref = view_cursor(at, w);
        CHECK(c.x == ref.x && c.y == ref.y && c.row == ref.row);
        if (at < n)
          CHECK(c.row + c.x == view_offset(at, dx, dy, p));
      }
    }
}

int main()
{
  check_rule();
  check_map(1, 1, 1, ViewPitch{3, 6});
  check_map(1, 7, 5, ViewPitch{2, 18});
  check_map(3, 5, 7, ViewPitch{8, 48});
  check_map(130, 3, 2, ViewPitch{131, 131 * 5});
  check_map(20000, 2, 1, ViewPitch{20003, 20003 * 3});
  // ... and the dense views of the same dims
  check_map(3, 5, 7, view_dense(3, 5));
  check_map(130, 3, 2, view_dense(130, 3));
  if (failures) {
    std::fprintf(stderr, "view_check: %d checks failed\n", failures);
    return 1;
  }
  std::puts("view_check ok");
  return 0;
}
