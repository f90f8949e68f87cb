// Host check of sperr_amd/csrc/fields.h, the one statement of what interleaved fields are: the validity rule with its
// refusals and its overflow guards, the extent, the offset map against four nested loops, the stacked side's size
// with the batch limit, the condition of the 16-byte forms, and -- for every stride_x that goes through LDS -- that
// the slot map the two kernels use is a bijection of the tile into the allocation.  tests/test_fields_host.py builds
// it under the address and undefined sanitizers and runs it; it prints "fields_check ok" and returns 0 when
// everything holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fields.h"

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
  const size_t big = SIZE_MAX, half = (big >> 1) + 1;   // 2^63
  size_t e = 0;
  // the dense interleave, a subset of a wider record, padded rows and slices
  CHECK(fields_extent(4, 40, 48, 56, fields_dense(4, 40, 48), &e) && e == size_t(4) * 40 * 48 * 56);
  CHECK(fields_extent(2, 40, 48, 56, FieldsLayout{5, 203, 203 * 48 + 7}, &e) &&
        e == size_t(55) * (203 * 48 + 7) + 47 * 203 + 39 * 5 + 2);
  CHECK(fields_extent(1, 1, 1, 1, FieldsLayout{1, 1, 1}, &e) && e == 1);
  CHECK(fields_extent(1, 1, 1, 1, FieldsLayout{64, 640, 6400}, &e) && e == 1);
  CHECK(fields_extent(3, 1, 1, 1, FieldsLayout{3, 3, 3}, &e) && e == 3);
  CHECK(fields_extent(3, 5, 1, 3, FieldsLayout{4, 21, 22}, &e) && e == 2 * 22 + 4 * 4 + 3);
  // a slice pitch that is no multiple of the row pitch is fine here (view.h refuses it)
  CHECK(fields_valid(2, 4, 4, 4, FieldsLayout{2, 9, 37}));
  CHECK(!view_valid(8, 4, 4, ViewPitch{9, 37}));
  // every refusal: an empty dim, no field, more fields than the record holds, rows that overlap, slices that overlap
  CHECK(!fields_valid(2, 0, 4, 4, FieldsLayout{2, 8, 32}));
  CHECK(!fields_valid(2, 4, 0, 4, FieldsLayout{2, 8, 32}));
  CHECK(!fields_valid(2, 4, 4, 0, FieldsLayout{2, 8, 32}));
  CHECK(!fields_valid(0, 4, 4, 4, FieldsLayout{2, 8, 32}));
  CHECK(fields_valid(2, 4, 4, 4, FieldsLayout{2, 8, 32}));
  CHECK(!fields_valid(3, 4, 4, 4, FieldsLayout{2, 8, 32}));
  CHECK(!fields_valid(1, 4, 4, 4, FieldsLayout{0, 8, 32}));
  CHECK(!fields_valid(2, 4, 4, 4, FieldsLayout{2, 7, 32}));
  CHECK(!fields_valid(2, 4, 4, 4, FieldsLayout{2, 8, 31}));
  CHECK(!fields_valid(2, 4, 4, 4, FieldsLayout{3, 11, 44}));
  CHECK(fields_valid(2, 4, 4, 4, FieldsLayout{3, 12, 48}));
  // sizes around SIZE_MAX: dimx * stride_x, pitch_y * dimy, (dimz - 1) * pitch_z and the sums
  CHECK(!fields_valid(1, 2, 1, 1, FieldsLayout{half, big, big}));            // dimx * stride_x = 2^64
  CHECK(fields_extent(1, 1, 1, 1, FieldsLayout{big, big, big}, &e) && e == 1);
  CHECK(!fields_valid(1, 1, 2, 1, FieldsLayout{1, half, big}));              // pitch_y * dimy = 2^64
  CHECK(!fields_valid(1, 1, 1, 3, FieldsLayout{1, 1, half}));                // (dimz - 1) * pitch_z = 2^64
  CHECK(fields_extent(1, 1, 1, 2, FieldsLayout{1, 1, big - 1}, &e) && e == big);   // the largest extent there is
  CHECK(!fields_valid(2, 1, 1, 2, FieldsLayout{2, 2, big - 1}));             // ... plus one
  CHECK(fields_extent(1, 1, 1, 2, FieldsLayout{1, 1, half}, &e) && e == half + 1);
  CHECK(!fields_valid(1, 1, 2, 2, FieldsLayout{1, half - 1, big - 1}));      // z part + y part overflows
  CHECK(fields_extent(1, 1, 2, 2, FieldsLayout{1, half / 2, half}, &e) && e == half + half / 2 + 1);
  CHECK(!fields_valid(big, 1, 1, 2, FieldsLayout{big, big, big}));           // ... + nfields overflows
  // a capacity is compared with the extent, in elements of the type
  const FieldsLayout pad{5, 203, 203 * 48 + 7};
  const size_t ext = size_t(55) * (203 * 48 + 7) + 47 * 203 + 39 * 5 + 2;
  CHECK(fields_fits(2, 40, 48, 56, pad, 4, ext * 4));
  CHECK(!fields_fits(2, 40, 48, 56, pad, 4, ext * 4 - 1));
  CHECK(!fields_fits(2, 40, 48, 56, pad, 8, ext * 8 - 8));
  CHECK(!fields_fits(6, 40, 48, 56, pad, 4, big));
  // the stacked side and the batch calls' limit nfields * dimz <= 2^32 - 1
  size_t n = 0;
  CHECK(fields_stacked(3, 5, 7, 11, &n) && n == 3 * 5 * 7 * 11);
  CHECK(fields_stacked(0xffffffffull, 1, 1, 1, &n) && n == 0xffffffffull);
  CHECK(!fields_stacked(0x100000000ull, 1, 1, 1, &n));
  CHECK(fields_stacked(0xffff, 1, 1, 0x10001, &n));
  CHECK(!fields_stacked(0x10000, 1, 1, 0x10000, &n));
  CHECK(!fields_stacked(2, half, 1, 1, &n));
  CHECK(!fields_stacked(1, half, 2, 1, &n));
  CHECK(!fields_stacked(0, 4, 4, 4, &n) && !fields_stacked(1, 4, 0, 4, &n));
  // the 16-byte forms: both first elements, both pitches and dimx
  const FieldsLayout a4{4, 64, 1024};
  CHECK(fields_vec_ok(0x1000, 0x2000, 16, a4, 4) && fields_vec_ok(0x1000, 0x2000, 16, a4, 8));
  CHECK(!fields_vec_ok(0x1004, 0x2000, 16, a4, 4) && !fields_vec_ok(0x1000, 0x2008, 16, a4, 4));
  CHECK(!fields_vec_ok(0x1000, 0x2000, 18, a4, 4) && fields_vec_ok(0x1000, 0x2000, 18, FieldsLayout{4, 72, 1024}, 8));
  CHECK(!fields_vec_ok(0x1000, 0x2000, 16, FieldsLayout{4, 66, 1024}, 4));
  CHECK(fields_vec_ok(0x1000, 0x2000, 16, FieldsLayout{4, 66, 1024}, 8));
  CHECK(!fields_vec_ok(0x1000, 0x2000, 16, FieldsLayout{4, 64, 1025}, 8));
  CHECK(fields_vec_ok(0x1000, 0x2000, 16, FieldsLayout{3, 48, 1024}, 4));   // (an odd record: the tile's span still starts on a pack)
}

// the map against four nested loops over a parent that is touched nowhere else: every selected element is met once,
// inside the extent, and the extent's last element is one of them
static void check_map(size_t nf, size_t dx, size_t dy, size_t dz, FieldsLayout l)
{
  size_t ext = 0;
  CHECK(fields_extent(nf, dx, dy, dz, l, &ext));
  std::vector<uint8_t> hit(ext, 0);
  for (size_t z = 0; z < dz; z++)
    for (size_t y = 0; y < dy; y++)
      for (size_t x = 0; x < dx; x++)
        for (size_t f = 0; f < nf; f++) {
          const size_t want = z * l.pitch_z + y * l.pitch_y + x * l.stride_x + f;
          CHECK(want < ext);
          CHECK(fields_offset(f, x, y, z, l) == want);
          if (want < ext)
            hit[want]++;
        }
  size_t met = 0;
  for (uint8_t h : hit) {
    CHECK(h <= 1);
    met += h;
  }
  CHECK(met == nf * dx * dy * dz && hit[ext - 1] == 1 && hit[0] == 1);
}

// the LDS image of a tile: every element of the largest span of a stride has a slot of its own inside the allocation,
// and the allocation of the widest stride is what the kernels' launch asks for
static void check_lds()
{
  for (uint32_t stride = 1; stride <= kFieldsMaxLdsStride; stride++) {
    const uint32_t span = kFieldsTileX * stride, slots = fields_lds_slots(stride);
    std::vector<uint8_t> used(slots, 0);
    uint32_t prev = 0;
    for (uint32_t i = 0; i < span; i++) {
      const uint32_t s = fields_lds_slot(i);
      CHECK(s < slots);
      CHECK(i == 0 || s > prev);   // (strictly increasing: one to one)
      prev = s;
      if (s < slots)
        used[s]++;
    }
    uint32_t met = 0;
    for (uint8_t u : used) {
      CHECK(u <= 1);
      met += u;
    }
    CHECK(met == span);
    CHECK(slots - span <= span / kFieldsLdsRun + 1);   // (the skew costs one slot per run, no more)
  }
  CHECK(kFieldsTileX % (kFieldsPackBytes / 4) == 0 && kFieldsTileX % (kFieldsPackBytes / 8) == 0);
  CHECK((size_t)fields_lds_slots(kFieldsMaxLdsStride) * 8 <= 64 * 1024);   // a workgroup's LDS without opting in for more
}

int main()
{
  check_rule();
  check_map(1, 1, 1, 1, FieldsLayout{3, 6, 12});
  check_map(1, 7, 5, 3, FieldsLayout{1, 9, 47});
  check_map(3, 5, 7, 2, fields_dense(3, 5, 7));
  check_map(2, 5, 3, 4, FieldsLayout{5, 26, 83});
  check_map(3, 4, 2, 3, FieldsLayout{8, 37, 79});
  check_map(17, 3, 2, 2, fields_dense(17, 3, 2));
  check_map(1, 300, 2, 2, FieldsLayout{17, 5101, 10207});
  check_lds();
  if (failures) {
    std::fprintf(stderr, "fields_check: %d checks failed\n", failures);
    return 1;
  }
  std::puts("fields_check ok");
  return 0;
}
