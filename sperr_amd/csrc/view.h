// view.h -- a strided view of a device array: the ONLY statement of what one is (the entry points of abi.hip, the
// view form of k_quality_rows and the host check tests/cpp/view_check.cpp all use these).  Plain C++: no HIP here.
//
// A view is a volume of dims (dimx, dimy, dimz), x fastest with unit x stride, given by the address of its first
// element and two pitches in elements: pitch_y from one row to the next, pitch_z from one slice to the next.  The
// dense volume is the view with pitch_y = dimx and pitch_z = dimx * dimy.
//
//   valid    dims > 0, pitch_y >= dimx, pitch_z >= pitch_y * dimy, pitch_z % pitch_y == 0 (the coder kernels address
//            a volume as (z * rows + y) * pitch + x: their VolDesc is {pitch_y, pitch_z / pitch_y, dimz}), and no
//            product on the way to the extent overflows size_t
//   extent   (dimz - 1) * pitch_z + (dimy - 1) * pitch_y + dimx elements from the first one: what a capacity is
//            compared with
//   offset   of linear index i of the view's own x-fastest order: z * pitch_z + y * pitch_y + x with
//            x = i % dimx, y = (i / dimx) % dimy, z = i / (dimx * dimy)
//
// ViewCursor walks that order without dividing by 64-bit numbers: view_cursor() places it (the divisions), view_advance()
// moves it forward by a step below 2^31 with 32-bit arithmetic.  It needs dims below 2^31.
#ifndef SPERR_AMD_VIEW_H
#define SPERR_AMD_VIEW_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SPERR_VIEW_FN __host__ __device__ inline
#else
#define SPERR_VIEW_FN inline
#endif

namespace sperrhip {

struct ViewPitch {
  size_t y, z;   // elements from row to row, from slice to slice
};

constexpr size_t kViewCursorMaxDim = size_t(1) << 31;   // (exclusive) what ViewCursor's 32-bit counters hold

// a * b into *out; false when it overflows
SPERR_VIEW_FN bool view_mul(size_t a, size_t b, size_t* out)
{
  if (a != 0 && b > ~size_t(0) / a)
    return false;
  *out = a * b;
  return true;
}

SPERR_VIEW_FN bool view_add(size_t a, size_t b, size_t* out)
{
  if (b > ~size_t(0) - a)
    return false;
  *out = a + b;
  return true;
}

// the extent in elements into *extent; false when the view is not valid
SPERR_VIEW_FN bool view_extent(size_t dimx, size_t dimy, size_t dimz, ViewPitch p, size_t* extent)
{
  size_t rows = 0, zpart = 0, ypart = 0, e = 0;
  if (dimx == 0 || dimy == 0 || dimz == 0 || p.y < dimx)
    return false;
  if (!view_mul(p.y, dimy, &rows) || p.z < rows || p.z % p.y != 0)
    return false;
  if (!view_mul(dimz - 1, p.z, &zpart) || !view_mul(dimy - 1, p.y, &ypart) || !view_add(zpart, ypart, &e) ||
      !view_add(e, dimx, &e))
    return false;
  *extent = e;   // (>= dimx * dimy * dimz, so that product fits as well)
  return true;
}

SPERR_VIEW_FN bool view_valid(size_t dimx, size_t dimy, size_t dimz, ViewPitch p)
{
  size_t e = 0;
  return view_extent(dimx, dimy, dimz, p, &e);
}

// the view can hold its elements in a buffer of cap_bytes that starts at its first element
SPERR_VIEW_FN bool view_fits(size_t dimx, size_t dimy, size_t dimz, ViewPitch p, size_t elem_size, size_t cap_bytes)
{
  size_t e = 0;
  return view_extent(dimx, dimy, dimz, p, &e) && e <= cap_bytes / elem_size;
}

SPERR_VIEW_FN ViewPitch view_dense(size_t dimx, size_t dimy) { return ViewPitch{dimx, dimx * dimy}; }

// element offset of linear index i (i < dimx * dimy * dimz) of a valid view
SPERR_VIEW_FN size_t view_offset(size_t i, size_t dimx, size_t dimy, ViewPitch p)
{
  const size_t x = i % dimx, r = i / dimx;
  return (r / dimy) * p.z + (r % dimy) * p.y + x;
}

// Where a walk through the view's linear order stands: (x, y) of the element and the offset of its row's first
// element.  The element's own offset is row + x.  Positions behind the view's last element are legal to stand on
// (they are z >= dimz) and must not be read.
struct ViewCursor {
  uint32_t x, y;
  uint64_t row;
};

// what view_advance() needs of a view beside the cursor
struct ViewWalk {
  uint32_t dimx, dimy;
  uint64_t pitch_y;
  uint64_t zskip;   // pitch_z - dimy * pitch_y: what a step from the last row of a slice to the next slice adds
};

SPERR_VIEW_FN ViewWalk view_walk(size_t dimx, size_t dimy, ViewPitch p)
{
  return ViewWalk{(uint32_t)dimx, (uint32_t)dimy, (uint64_t)p.y, (uint64_t)(p.z - dimy * p.y)};
}

SPERR_VIEW_FN ViewCursor view_cursor(uint64_t i, const ViewWalk& w)
{
  const uint64_t r = i / w.dimx, z = r / w.dimy;
  const uint32_t y = (uint32_t)(r - z * w.dimy);
  return ViewCursor{(uint32_t)(i - r * w.dimx), y, z * ((uint64_t)w.dimy * w.pitch_y + w.zskip) + y * w.pitch_y};
}

// one element forward
SPERR_VIEW_FN void view_next(ViewCursor& c, const ViewWalk& w)
{
  if (++c.x == w.dimx) {
    c.x = 0;
    c.row += w.pitch_y;
    if (++c.y == w.dimy) {
      c.y = 0;
      c.row += w.zskip;
    }
  }
}

// `step` elements forward, step < 2^31.  A row that is at least a step long is left at most once; shorter rows take
// two 32-bit divisions.
SPERR_VIEW_FN void view_advance(ViewCursor& c, const ViewWalk& w, uint32_t step)
{
  const uint32_t x = c.x + step;   // (< 2^32: both below 2^31)
  if (w.dimx >= step) {
    if (x < w.dimx) {
      c.x = x;
      return;
    }
    c.x = x - w.dimx;
    c.row += w.pitch_y;
    if (++c.y == w.dimy) {
      c.y = 0;
      c.row += w.zskip;
    }
    return;
  }
  const uint32_t q = x / w.dimx;   // rows left behind: <= step
  c.x = x - q * w.dimx;
  const uint32_t y = c.y + q;      // (< 2^32 likewise)
  const uint32_t qz = y / w.dimy;
  c.y = y - qz * w.dimy;
  c.row += (uint64_t)q * w.pitch_y + (uint64_t)qz * w.zskip;
}

}  // namespace sperrhip

#endif
