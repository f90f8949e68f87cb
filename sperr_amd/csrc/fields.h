// fields.h -- interleaved fields of a device array: the ONLY statement of the layout (the entry points of abi.hip,
// the two kernels of fields.hip and the host check tests/cpp/fields_check.cpp all use these).  Plain C++: no HIP here.
//
// An interleaved array keeps several variables per sample, the variables innermost: (z, y, x, nvar), a detector's
// (y, x, channel), a channels-last tensor.  Its layout is {stride_x, pitch_y, pitch_z} in elements: stride_x from
// one sample to the next along x (the record's width), pitch_y from row to row, pitch_z from slice to slice.  A call
// names nfields consecutive fields of it; its data pointer is the address of the FIRST SELECTED field at (0, 0, 0).
//
//   offset   field f (f < nfields), sample (x, y, z):  z * pitch_z + y * pitch_y + x * stride_x + f
//   valid    dims > 0, 1 <= nfields <= stride_x, pitch_y >= dimx * stride_x, pitch_z >= pitch_y * dimy, and no
//            product on the way to the extent overflows size_t.  pitch_z need NOT be a multiple of pitch_y: no coder
//            kernel addresses this array (view.h has that clause for them), only the two kernels of fields.hip do
//   extent   (dimz - 1) * pitch_z + (dimy - 1) * pitch_y + (dimx - 1) * stride_x + nfields elements from the data
//            pointer: what a capacity is compared with
//   dense    {nfields, dimx * nfields, dimx * dimy * nfields}: what a NULL layout means
//   batch    nfields * dimz <= 2^32 - 1, the batch calls' limit (chunk origins of the stacked volumes are 32-bit)
//
// The stacked side of both kernels is nfields dense volumes of dims (dimx, dimy, dimz) back to back, field f first
// element at f * dimx * dimy * dimz: what the batch calls take and return.
#ifndef SPERR_AMD_FIELDS_H
#define SPERR_AMD_FIELDS_H

#include <stddef.h>
#include <stdint.h>

#include "view.h"

namespace sperrhip {

struct FieldsLayout {
  size_t stride_x, pitch_y, pitch_z;   // elements from sample to sample along x, from row to row, from slice to slice
};

// ---- the kernels' constants ------------------------------------------------------------------------------------
// x positions of one (y, z) row that a workgroup moves at a time: a contiguous span of kFieldsTileX * stride_x
// elements of the interleaved array, and kFieldsTileX consecutive values of every selected field's stacked volume.
// It is the workgroup's thread count, and a multiple of every pack (16 bytes: 4 floats, 2 doubles).
constexpr uint32_t kFieldsTileX = 256;
// the largest stride_x whose span goes through LDS (kFieldsTileX * 16 doubles and the pad are 33 KiB); wider records
// -- one field of a 64-wide record -- are moved piece by piece without LDS
constexpr uint32_t kFieldsMaxLdsStride = 16;
// The LDS image of a span keeps one empty slot after every kFieldsLdsRun elements.  A lane reads the image at an
// element stride of stride_x (or a pack's multiple of it); ds_read_b32 has 32 banks of 4 bytes and ds_read_b64 64, so
// for both element sizes an even stride would meet gcd(stride, 32) times fewer banks than lanes, and one slot of
// skew per 32 elements moves every run of lanes that wrapped onto the next bank.
constexpr uint32_t kFieldsLdsRun = 32;
constexpr uint32_t kFieldsPackBytes = 16;   // what the kVec forms load and store at a time

// slot of element i of a span in the LDS image (i < kFieldsTileX * stride_x)
SPERR_VIEW_FN uint32_t fields_lds_slot(uint32_t i) { return i + i / kFieldsLdsRun; }
// slots the image of a span of stride_x allocates
SPERR_VIEW_FN uint32_t fields_lds_slots(uint32_t stride_x)
{
  const uint32_t span = kFieldsTileX * stride_x;
  return span + (span + kFieldsLdsRun - 1) / kFieldsLdsRun;
}

// ---- the rule --------------------------------------------------------------------------------------------------
SPERR_VIEW_FN FieldsLayout fields_dense(size_t nfields, size_t dimx, size_t dimy)
{
  return FieldsLayout{nfields, dimx * nfields, dimx * dimy * nfields};
}

// the extent in elements into *extent; false when the layout is not valid
SPERR_VIEW_FN bool fields_extent(size_t nfields, size_t dimx, size_t dimy, size_t dimz, FieldsLayout l, size_t* extent)
{
  size_t row = 0, rows = 0, zpart = 0, ypart = 0, xpart = 0, e = 0;
  if (dimx == 0 || dimy == 0 || dimz == 0 || nfields == 0 || nfields > l.stride_x)
    return false;
  if (!view_mul(dimx, l.stride_x, &row) || l.pitch_y < row)
    return false;
  if (!view_mul(l.pitch_y, dimy, &rows) || l.pitch_z < rows)
    return false;
  if (!view_mul(dimz - 1, l.pitch_z, &zpart) || !view_mul(dimy - 1, l.pitch_y, &ypart) ||
      !view_mul(dimx - 1, l.stride_x, &xpart) || !view_add(zpart, ypart, &e) || !view_add(e, xpart, &e) ||
      !view_add(e, nfields, &e))
    return false;
  *extent = e;   // (>= nfields * dimx * dimy * dimz is NOT implied: see fields_stacked)
  return true;
}

SPERR_VIEW_FN bool fields_valid(size_t nfields, size_t dimx, size_t dimy, size_t dimz, FieldsLayout l)
{
  size_t e = 0;
  return fields_extent(nfields, dimx, dimy, dimz, l, &e);
}

// the layout can hold its elements in a buffer of cap_bytes that starts at the data pointer
SPERR_VIEW_FN bool fields_fits(size_t nfields, size_t dimx, size_t dimy, size_t dimz, FieldsLayout l, size_t elem_size,
                               size_t cap_bytes)
{
  size_t e = 0;
  return fields_extent(nfields, dimx, dimy, dimz, l, &e) && e <= cap_bytes / elem_size;
}

// elements of the stacked side, nfields * dimx * dimy * dimz, into *count; false when that overflows, when a dim is
// empty or when the batch calls' limit nfields * dimz <= 2^32 - 1 does not hold
SPERR_VIEW_FN bool fields_stacked(size_t nfields, size_t dimx, size_t dimy, size_t dimz, size_t* count)
{
  size_t n = 0;
  if (nfields == 0 || dimx == 0 || dimy == 0 || dimz == 0 || nfields > size_t(0xffffffffull) / dimz)
    return false;
  if (!view_mul(dimx, dimy, &n) || !view_mul(n, dimz, &n) || !view_mul(n, nfields, &n))
    return false;
  *count = n;
  return true;
}

// element offset of field f, sample (x, y, z) of a valid layout
SPERR_VIEW_FN size_t fields_offset(size_t f, size_t x, size_t y, size_t z, FieldsLayout l)
{
  return z * l.pitch_z + y * l.pitch_y + x * l.stride_x + f;
}

// The kVec forms move 16-byte packs: every row's span and every destination row must start on a 16-byte boundary.
// That is so when both first elements are, the pitches and the record are whole packs' worth of bytes apart -- a
// tile starts kFieldsTileX records into its row, which then is -- and dimx is a whole number of packs (the stacked
// rows are dimx elements apart).  The scatter has one more condition, which its caller adds: nfields == stride_x
// (a 16-byte store into a subset would write a neighbour's bytes).
SPERR_VIEW_FN bool fields_vec_ok(uintptr_t interleaved, uintptr_t stacked, size_t dimx, FieldsLayout l, size_t elem_size)
{
  const size_t pack = kFieldsPackBytes / elem_size;
  return interleaved % kFieldsPackBytes == 0 && stacked % kFieldsPackBytes == 0 && l.pitch_y % pack == 0 &&
         l.pitch_z % pack == 0 && dimx % pack == 0;
}

// ---- the device side (fields.hip) ------------------------------------------------------------------------------
// One launch each on `hip_stream` (a hipStream_t), no host wait.  d_inter is the data pointer of the interleaved
// array, d_stacked the first of nfields dense volumes back to back.  0 ok; -1, with nothing launched, for a NULL
// pointer, a layout that is not valid, sizes that overflow, the batch limit, or dimx, dimy, stride_x or the blocks of
// one slice (ceil(dimx / kFieldsTileX) * dimy) at or beyond 2^31.
int fields_gather_run(const void* d_inter, FieldsLayout l, size_t nfields, int is_float, size_t dimx, size_t dimy,
                      size_t dimz, void* d_stacked, void* hip_stream);
int fields_scatter_run(const void* d_stacked, size_t nfields, int is_float, size_t dimx, size_t dimy, size_t dimz,
                       void* d_inter, FieldsLayout l, void* hip_stream);

}  // namespace sperrhip

#endif
