// mask_fill.h -- missing values: what stands at the missing samples of the in-filled volume.  The fill kinds, and the
// ONLY statement of the smooth rule (the kernels of mask_fill.hip, the entry points of abi_mask.hip and the host
// check tests/cpp/mask_fill_check.cpp all use these).  Plain C++: no HIP here.  mask.h states the other three rules --
// which samples are missing, the midrange value F, the stream.
//
//   kMaskFillMidrange  F of mask.h, bit for bit
//   kMaskFillValue     a finite double of the caller's, narrowed once to float for fp32 data (it must still be finite)
//   kMaskFillSmooth    a pull-push fill: averages of the valid samples on a pyramid of half resolutions, pulled up to
//                      one cell, and pushed back down into the cells no valid sample reached
//
// The smooth rule.  Every operation is one IEEE double operation, each product and each sum rounded on its own; no fma.
//   levels   level 0 has the volume's dims (x, y, z); level l + 1 has ceil(d / 2) along each axis; L is the first level
//            whose dims are all 1.  A one-sample volume has L = 0 and its fill is 0.0
//   pull     l = 0 .. L - 1.  A level-0 cell is KNOWN when its sample is valid, its value the sample widened to double.
//            Cell (X, Y, Z) of level l + 1 looks at its children (2X + a, 2Y + b, 2Z + c), a, b, c in {0, 1}, that lie
//            inside level l: s = +0.0, k = 0; through c, then b, then a (x fastest), each ascending, every known child
//            gives s = s + v, k++.  The cell is known when k > 0, with value s / (double)k
//   top      with no valid sample the top cell is unknown: it becomes 0.0, known
//   refusal  a sum s that is not finite fails the call (fp64 data near DBL_MAX; an infinity that rule 1 calls valid).
//            Under this kind it takes the place of the midrange rule's refusal of a non-finite lo / hi
//   push     l = L - 1 .. 0.  Known cells keep their value.  An unknown cell (x, y, z) of level l is interpolated from
//            eight cells of level l + 1, all known by then.  Per axis with coordinate i: P = i >> 1 and
//            Q = (i odd) ? min(P + 1, dim - 1) : (P == 0 ? 0 : P - 1), dim being level l + 1's.  Along x first, for
//            the pairs (Y, Z) in {Py, Qy} x {Pz, Qz}: t = 0.75 * v(Px, Y, Z) + 0.25 * v(Qx, Y, Z); then along y:
//            u = 0.75 * t(Py, Z) + 0.25 * t(Qy, Z); then along z: w = 0.75 * u(Pz) + 0.25 * u(Qz).  A missing sample
//            of level 0 becomes w, narrowed once to float for fp32 data; valid samples are copied bit for bit
//
// On the device the levels 1 .. G of the pyramid are doubles in global memory (MaskFillPlan) and the levels above G
// live in the LDS of k_mask_top.  AN UNKNOWN CELL HOLDS A NaN (mask_fill_unknown): a known cell of a call that is not
// refused is finite, and in a refused call nothing of the pyramid is used.
#ifndef SPERR_AMD_MASK_FILL_H
#define SPERR_AMD_MASK_FILL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "view.h"

namespace sperrhip {

constexpr int kMaskFillMidrange = 0, kMaskFillValue = 1, kMaskFillSmooth = 2;

// ---- the kernels' constants ------------------------------------------------------------------------------------
// The levels k_mask_top keeps in LDS begin with one of at most kMaskTopCells cells.  Every level above it has at least
// one axis halved (rounded up), so all of them together hold fewer than kMaskTopCells + 64 cells:
// kMaskTopLdsCells doubles, 33 280 bytes of LDS.
constexpr uint32_t kMaskTopCells = 2048;
constexpr uint32_t kMaskTopLdsCells = 2 * kMaskTopCells + 64;
constexpr uint32_t kMaskTopThreads = 1024;
constexpr uint32_t kMaskFillMaxLevels = 64;     // dims below 2^64: L <= 64
constexpr size_t kMaskFillHeadBytes = 256;      // the pyramid buffer begins with the non-finite flag word

SPERR_VIEW_FN bool mask_fill_kind_ok(int fill) { return fill >= kMaskFillMidrange && fill <= kMaskFillSmooth; }
SPERR_VIEW_FN bool mask_fill_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }
// the caller's value as the samples will hold it; false: not finite, or not finite as a float
SPERR_VIEW_FN bool mask_fill_value_ok(double value, bool is_float, double* stored)
{
  *stored = is_float ? (double)(float)value : value;
  return mask_fill_finite(value) && mask_fill_finite(*stored);
}

SPERR_VIEW_FN double mask_fill_unknown()
{
  const uint64_t u = 0x7ff8000000000000ull;
  double d;
  memcpy(&d, &u, 8);
  return d;
}
SPERR_VIEW_FN bool mask_fill_known(double v) { return v == v; }

// ---- the levels ------------------------------------------------------------------------------------------------
SPERR_VIEW_FN uint64_t mask_fill_half(uint64_t d) { return d / 2 + (d & 1); }

// G' levels l >= 1 hold more than kMaskTopCells cells; G = max(1, G') levels are kept in global memory, level l at
// off[l] doubles behind the head.  k_mask_top reads level G and keeps the levels G + 1 .. L in LDS: level G + 1 has at
// most kMaskTopCells cells (for G' = 0 because level 1 has).  L = 0: no pyramid, bytes is 0
struct MaskFillPlan {
  uint32_t L, G;
  uint64_t dim[kMaskFillMaxLevels + 1][3];
  uint64_t cells[kMaskFillMaxLevels + 1];
  uint64_t off[kMaskFillMaxLevels + 1];
  uint64_t ldsCells;   // the cells of the levels G + 1 .. L
  size_t bytes;        // of the pyramid buffer: the head and the levels 1 .. G, exactly
};

// false: a dim is 0 or the sample count overflows
SPERR_VIEW_FN bool mask_fill_plan(size_t dimx, size_t dimy, size_t dimz, MaskFillPlan* p)
{
  size_t n = 0;
  if (!dimx || !dimy || !dimz || !view_mul(dimx, dimy, &n) || !view_mul(n, dimz, &n) || n > SIZE_MAX / 8)
    return false;
  p->dim[0][0] = dimx;
  p->dim[0][1] = dimy;
  p->dim[0][2] = dimz;
  p->cells[0] = n;
  p->off[0] = 0;
  uint32_t l = 0, gprime = 0;
  while (p->dim[l][0] > 1 || p->dim[l][1] > 1 || p->dim[l][2] > 1) {
    for (int a = 0; a < 3; a++)
      p->dim[l + 1][a] = mask_fill_half(p->dim[l][a]);
    l++;
    p->cells[l] = p->dim[l][0] * p->dim[l][1] * p->dim[l][2];
    if (p->cells[l] > kMaskTopCells)
      gprime++;
  }
  p->L = l;
  p->G = gprime > 1 ? gprime : 1;
  p->ldsCells = 0;
  p->bytes = 0;
  if (l == 0) {
    p->G = 0;
    return true;
  }
  uint64_t at = 0;
  for (uint32_t k = 1; k <= l; k++) {
    p->off[k] = k <= p->G ? at : 0;
    if (k <= p->G)
      at += p->cells[k];
    else
      p->ldsCells += p->cells[k];
  }
  p->bytes = kMaskFillHeadBytes + 8 * (size_t)at;
  return true;
}

// ---- a cell of the pull ----------------------------------------------------------------------------------------
// Cell (X, Y, Z) of the level above one of dims (dx, dy, dz); child(x, y, z) is that level's cell, a NaN when unknown.
// *finite is cleared when the sum is not finite, and left alone otherwise
template <typename I, typename F>
SPERR_VIEW_FN double mask_fill_pull_cell(I X, I Y, I Z, I dx, I dy, I dz, F child, bool* finite)
{
  double s = 0.0;
  uint32_t k = 0;
  for (I c = 0; c < 2; c++) {
    const I z = 2 * Z + c;
    if (z >= dz)
      break;
    for (I b = 0; b < 2; b++) {
      const I y = 2 * Y + b;
      if (y >= dy)
        break;
      for (I a = 0; a < 2; a++) {
        const I x = 2 * X + a;
        if (x >= dx)
          break;
        const double v = child(x, y, z);
        if (mask_fill_known(v)) {
          s = s + v;
          k++;
        }
      }
    }
  }
  if (!mask_fill_finite(s))
    *finite = false;
  return k ? s / (double)k : mask_fill_unknown();
}

// ---- a cell of the push ----------------------------------------------------------------------------------------
// the two cells of the coarser level, of extent dim along this axis, that coordinate i of the finer one lies between
template <typename I>
SPERR_VIEW_FN void mask_fill_pq(I i, I dim, I* P, I* Q)
{
  const I p = i >> 1;
  *P = p;
  *Q = (i & 1) ? (p + 1 < dim - 1 ? p + 1 : dim - 1) : (p == 0 ? 0 : p - 1);
}

SPERR_VIEW_FN double mask_fill_lerp(double vp, double vq)
{
  const double a = 0.75 * vp;
  const double b = 0.25 * vq;
  return a + b;
}

// what the unknown cell (x, y, z) gets from the complete level above it, whose dims are (cx, cy, cz) and whose cells
// coarse(X, Y, Z) returns
template <typename I, typename F>
SPERR_VIEW_FN double mask_fill_interp(I x, I y, I z, I cx, I cy, I cz, F coarse)
{
  I px, qx, py, qy, pz, qz;
  mask_fill_pq(x, cx, &px, &qx);
  mask_fill_pq(y, cy, &py, &qy);
  mask_fill_pq(z, cz, &pz, &qz);
  const double tpp = mask_fill_lerp(coarse(px, py, pz), coarse(qx, py, pz));
  const double tqp = mask_fill_lerp(coarse(px, qy, pz), coarse(qx, qy, pz));
  const double tpq = mask_fill_lerp(coarse(px, py, qz), coarse(qx, py, qz));
  const double tqq = mask_fill_lerp(coarse(px, qy, qz), coarse(qx, qy, qz));
  const double up = mask_fill_lerp(tpp, tqp);
  const double uq = mask_fill_lerp(tpq, tqq);
  return mask_fill_lerp(up, uq);
}

// ---- the rule on the host, as plain loops --------------------------------------------------------------------------
// dst (may be src) from the n samples at src and their n bytes of 0 / 1 at `missing`; `work` holds the levels 1 .. L:
// mask_fill_host_cells(plan) doubles.  false: a sum was not finite, and dst is not written
SPERR_VIEW_FN uint64_t mask_fill_host_cells(const MaskFillPlan& p)
{
  uint64_t c = 0;
  for (uint32_t l = 1; l <= p.L; l++)
    c += p.cells[l];
  return c;
}

template <typename T>
inline bool mask_fill_smooth_host(const T* src, const uint8_t* missing, const MaskFillPlan& p, double* work, T* dst)
{
  if (p.L == 0) {
    dst[0] = missing[0] ? T(0) : src[0];
    return true;
  }
  uint64_t at[kMaskFillMaxLevels + 1] = {0, 0};
  for (uint32_t l = 2; l <= p.L; l++)
    at[l] = at[l - 1] + p.cells[l - 1];
  bool finite = true;
  for (uint32_t l = 0; l < p.L; l++) {
    const uint64_t dx = p.dim[l][0], dy = p.dim[l][1], dz = p.dim[l][2];
    const uint64_t cx = p.dim[l + 1][0], cy = p.dim[l + 1][1], cz = p.dim[l + 1][2];
    const double* fine = work + at[l];
    double* out = work + at[l + 1];
    for (uint64_t Z = 0; Z < cz; Z++)
      for (uint64_t Y = 0; Y < cy; Y++)
        for (uint64_t X = 0; X < cx; X++)
          out[(Z * cy + Y) * cx + X] = mask_fill_pull_cell<uint64_t>(
              X, Y, Z, dx, dy, dz,
              [&](uint64_t x, uint64_t y, uint64_t z) {
                const uint64_t i = (z * dy + y) * dx + x;
                if (l > 0)
                  return fine[i];
                return missing[i] ? mask_fill_unknown() : (double)src[i];
              },
              &finite);
  }
  if (!finite)
    return false;
  double* top = work + at[p.L];
  if (!mask_fill_known(*top))
    *top = 0.0;
  for (uint32_t l = p.L; l-- > 0;) {
    const uint64_t dx = p.dim[l][0], dy = p.dim[l][1], dz = p.dim[l][2];
    const uint64_t cx = p.dim[l + 1][0], cy = p.dim[l + 1][1], cz = p.dim[l + 1][2];
    const double* coarse = work + at[l + 1];
    double* lev = work + at[l];
    for (uint64_t z = 0; z < dz; z++)
      for (uint64_t y = 0; y < dy; y++)
        for (uint64_t x = 0; x < dx; x++) {
          const uint64_t i = (z * dy + y) * dx + x;
          const bool unknown = l > 0 ? !mask_fill_known(lev[i]) : missing[i] != 0;
          if (!unknown) {
            if (l == 0)
              dst[i] = src[i];
            continue;
          }
          const double w = mask_fill_interp<uint64_t>(
              x, y, z, cx, cy, cz, [&](uint64_t X, uint64_t Y, uint64_t Z) { return coarse[(Z * cy + Y) * cx + X]; });
          if (l > 0)
            lev[i] = w;
          else
            dst[i] = (T)w;
        }
  }
  return true;
}

// ---- the device side (mask_fill.hip) ---------------------------------------------------------------------------
// bytes of the pyramid buffer of a volume (0: one sample, or the dims are refused): mask_fill_plan's
size_t mask_fill_workspace_bytes(size_t dimx, size_t dimy, size_t dimz);

// The pull of a smooth fill, queued on `hip_stream` behind k_mask_survey and k_mask_finish and in front of the call's
// read-back: k_mask_pull0, k_mask_pull G - 1 times, k_mask_top.  `ws` is the workspace of mask_scan_run (the bit array,
// and MaskResult::finite, which k_mask_top sets from the flag word), `pyr` mask_fill_workspace_bytes of device memory,
// 256-byte aligned.  No host wait.  L = 0 launches nothing
int mask_fill_pull_run(const void* d_src, int is_float, const MaskFillPlan& plan, void* ws, void* pyr, void* hip_stream);
// The push: k_mask_push G - 1 times, then k_mask_fill_smooth into d_filled (may be d_src).  No host wait
int mask_fill_push_run(const void* d_src, int is_float, const MaskFillPlan& plan, const void* ws, void* pyr,
                       void* d_filled, void* hip_stream);

}  // namespace sperrhip

#endif
