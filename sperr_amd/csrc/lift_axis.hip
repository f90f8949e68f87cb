// lift_axis.hip -- the CDF 9/7 lifting DWT and IDWT of the chunk pipeline, one axis a launch (k_lift_axis: every
// level of every shape) and the finest level's x and y passes fused with the volume access (k_lift_xy), as HIP kernels
// for gfx950; the lifting constants.  The three passes of a level in one kernel: lift_xyz_fwd.hip, lift_xyz_inv.hip,
// lift_xyz_inv_crop.hip.  Everything is fp64 with the reference's exact operation order; compile with
// -ffp-contract=off (every fused multiply-add of the canonical reference build is an explicit fma(), see SURVEY.md
// Appendix B).
//
// Reference behaviour restated (file:line of the reference):
//   src/CDF97.cpp:132-148,284-302,345-474,598-666   dyadic / wavelet-packet 3D transform
#include <type_traits>

#include "xform.h"
#include "lift_dev.h"
#include "lift_window.h"
#include "dequant.h"

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// CDF 9/7 lifting along one axis, LDS-staged line tiles
// ------------------------------------------------------------------------------------------
//
// A workgroup stages NL adjacent lines of length `len` in LDS as sm[pos * (NL+1) + line] with the
// samples already de-interleaved ([even | odd], src/CDF97.cpp:476-519), runs the four lifting
// steps + scaling with a barrier between dependent steps, and writes the lines back.  For the Y
// and Z axes the NL lines are NL consecutive x positions, so every global access is a coalesced
// NL*8-byte segment; for the X axis the lines are NL consecutive rows and lanes run along x.

// IO: 0 = in place on the fp64 chunk buffer; 1 / 2 = the pass also moves the chunk between the
// float / double VOLUME and the chunk buffer: the first forward pass reads the volume through the
// gather map and subtracts the mean (src/SPERR3D_OMP_C.cpp:236-261, Conditioner.cpp:48-50), the
// last inverse pass adds the mean, narrows and scatters (Conditioner.cpp:66-96,
// SPERR3D_OMP_D.cpp:167-184, SPERR_C_API.cpp:246-250).  Both passes cover the whole chunk.
constexpr int kLoadBatch = 8;

// kCrop (inverse, IO != 0 only): the pass writes the chunk's window into the box; a tile with no line
// in the window has nothing to do
template <bool FORWARD, int IO, bool kCrop = false>
__global__ void __launch_bounds__(kThreads)
k_lift_axis(double* vals, size_t valsStride, uint32_t cx, uint32_t cy, int axis, uint32_t rx,
            uint32_t ry, uint32_t rz, int NL, LiftConsts K, CoderState* st, void* volume,
            VolDesc vd, const GeomOf<kCrop>* geom, LiftFuse F)
{
  static_assert(!kCrop || (!FORWARD && IO != 0), "the crop variant is a last inverse pass");
  const uint32_t c = blockIdx.y;
  const bool is_const = st[c].is_const != 0;
  if (is_const && !(IO != 0 && !FORWARD))
    return;
  double* sm = reinterpret_cast<double*>(dyn_smem);
  double* buf = vals + c * valsStride;
  const uint32_t region[3] = {rx, ry, rz};
  const uint32_t bx = (!FORWARD && F.bufx) ? F.bufx : cx, by = (!FORWARD && F.bufy) ? F.bufy : cy;   // (compact buffer)
  const size_t stride[3] = {1, bx, (size_t)bx * by};
  const int ua = (axis == 0) ? 1 : 0;            // axis along which the NL lines are adjacent
  const int wa = (axis == 2) ? 1 : 2;            // remaining axis
  const uint32_t len = region[axis];
  const uint32_t ntu = (region[ua] + NL - 1) / NL;
  const uint32_t tu = blockIdx.x % ntu, tw = blockIdx.x / ntu;
  const uint32_t u0 = tu * NL;
  const uint32_t nl = min((uint32_t)NL, region[ua] - u0);  // valid lines in this tile
  double* tile = buf + (size_t)u0 * stride[ua] + (size_t)tw * stride[wa];
  const size_t sl = stride[axis], su = stride[ua];
  const int NLP = NL + 1;
  const uint32_t even_len = len - len / 2, odd_len = len / 2;
  const int tid = threadIdx.x;

  // volume address of chunk sample (line l, position p) of this tile
  using VT = typename std::conditional<IO == 1, float, double>::type;
  VT* vol = reinterpret_cast<VT*>(volume);
  size_t vbase = 0, vsl = 0, vsu = 0;
  double mean = 0.0;
  CropGeom cg{};
  if constexpr (kCrop) {   // (uniform)
    cg = geom[c];
    if (tw - cg.lo[wa] >= cg.hi[wa] - cg.lo[wa] || u0 >= cg.hi[ua] || u0 + nl <= cg.lo[ua])
      return;
    mean = st[c].mean;
  }
  else if (IO != 0) {
    const ChunkGeom g = geom[c];
    const size_t vstride[3] = {1, (size_t)vd.dims[0], (size_t)vd.dims[0] * vd.dims[1]};
    vbase = (size_t)g.org[0] * vstride[0] + (size_t)g.org[1] * vstride[1] +
            (size_t)g.org[2] * vstride[2] + (size_t)u0 * vstride[ua] + (size_t)tw * vstride[wa];
    vsl = vstride[axis];
    vsu = vstride[ua];
    mean = st[c].mean;
  }

  // ---- load: a thread issues kLoadBatch loads before it uses the first value (one at a time
  // leaves the pass waiting on HBM latency) ----
  using LT = typename std::conditional<(IO != 0 && FORWARD), VT, double>::type;
  // (l, p) of this tile as chunk coordinates, and whether a later pass of the forward order
  // touches the sample (LiftFuse)
  auto outside_inner = [&](uint32_t l, uint32_t p, size_t& idx) -> bool {
    uint32_t xyz[3];
    xyz[axis] = p;
    xyz[ua] = u0 + l;
    xyz[wa] = tw;
    idx = ((size_t)xyz[2] * cy + xyz[1]) * cx + xyz[0];
    return !(xyz[0] < F.inner[0] && xyz[1] < F.inner[1] && xyz[2] < F.inner[2]);
  };
  const bool dequant = !FORWARD && F.mode == 2 && !st[c].wide;
  const DequantSrc& Q = F.src;
  const bool haveMasks = dequant && Q.has_masks();
  const DequantRule<uint32_t> rule =
      dequant_rule<uint32_t>(dequant ? st[c].q : 0.0, haveMasks, haveMasks ? Q.dst + c : nullptr, Q.coefSigned != 0);
  auto fetch = [&](uint32_t l, uint32_t p) -> LT {
    if (IO != 0 && FORWARD)
      return (LT)vol[vbase + l * vsu + p * vsl];
    if (!FORWARD && dequant) {
      size_t idx;
      if (outside_inner(l, p, idx)) {   // this one sample from its coefficient (dequant.h); the loads are independent
        const uint32_t v = Q.coefs<uint32_t>(c)[idx];
        if (rule.scheme)   // (the sign in bit 31, the value complete: DequantSrc::coefSigned)
          return (LT)dequant_signed(rule, v);
        const uint32_t w = (uint32_t)(idx >> 6), sh = (uint32_t)(idx & 63);
        const uint64_t sgw = Q.sign[c * Q.signStride + w];
        const uint64_t mnw = haveMasks ? Q.sigNew[c * Q.maskStride + w] : 0ull;
        const uint64_t mow = haveMasks ? Q.sigOld[c * Q.maskStride + w] : 0ull;
        return (LT)dequant_masks(rule, v, mnw, mow, sgw, sh);
      }
    }
    return (LT)tile[l * su + p * sl];
  };
  auto deposit = [&](uint32_t l, uint32_t p, LT v) {
    const uint32_t dst = FORWARD ? ((p & 1) ? even_len + (p >> 1) : (p >> 1)) : p;
    sm[dst * NLP + l] = (IO != 0 && FORWARD) ? (double)v - mean : (double)v;
  };
  if (!(is_const && !(IO != 0 && FORWARD))) {
    if (axis == 0) {  // lanes along the line: a wavefront moves 64 consecutive samples of a line
      const uint32_t nseg = (len + 63) / 64, nsg = nl * nseg, step = kThreads / 64;
      for (uint32_t sg0 = tid / 64; sg0 < nsg; sg0 += step * kLoadBatch) {
        LT v[kLoadBatch];
#pragma unroll
        for (int u = 0; u < kLoadBatch; u++) {
          const uint32_t sg = sg0 + u * step, l = sg / nseg, p = (sg % nseg) * 64 + tid % 64;
          v[u] = (sg < nsg && p < len) ? fetch(l, p) : (LT)0;
        }
#pragma unroll
        for (int u = 0; u < kLoadBatch; u++) {
          const uint32_t sg = sg0 + u * step, l = sg / nseg, p = (sg % nseg) * 64 + tid % 64;
          if (sg < nsg && p < len)
            deposit(l, p, v[u]);
        }
      }
    }
    else {            // lanes across the lines
      const uint32_t l = tid % NL, k0 = tid / NL, kg = kThreads / NL;
      if (l < nl)
        for (uint32_t p0 = k0; p0 < len; p0 += kg * kLoadBatch) {
          LT v[kLoadBatch];
#pragma unroll
          for (int u = 0; u < kLoadBatch; u++)
            v[u] = p0 + u * kg < len ? fetch(l, p0 + u * kg) : (LT)0;
#pragma unroll
          for (int u = 0; u < kLoadBatch; u++)
            if (p0 + u * kg < len)
              deposit(l, p0 + u * kg, v[u]);
        }
    }
  }
  __syncthreads();

  // ---- lift ----
  if (!is_const) {
    const uint32_t l = tid % NL, k0 = tid / NL, kg = kThreads / NL;
    double* E = sm + l;
    double* O = sm + (size_t)even_len * NLP + l;
#define EV(i) E[(size_t)(i) * NLP]
#define OD(i) O[(size_t)(i) * NLP]
    auto odd_step = [&](double k) {
      if (l < nl)
        for (uint32_t i = k0; i < odd_len; i += kg) {
          const uint32_t r = min(i + 1, even_len - 1);
          OD(i) = fma(k, EV(i) + EV(r), OD(i));
        }
      __syncthreads();
    };
    auto even_step = [&](double k) {
      if (l < nl)
        for (uint32_t i = k0; i < even_len; i += kg) {
          const uint32_t a = max(i, 1u) - 1, b = min(i, odd_len - 1);
          EV(i) = fma(k, OD(a) + OD(b), EV(i));
        }
      __syncthreads();
    };
    if (FORWARD) {  // src/CDF97.cpp:598-631
      odd_step(K.alpha);
      even_step(K.beta);
      odd_step(K.gamma);
      if (l < nl) {
        for (uint32_t i = k0; i < even_len; i += kg) {
          const uint32_t a = max(i, 1u) - 1, b = min(i, odd_len - 1);
          EV(i) = K.eps * fma(K.delta, OD(a) + OD(b), EV(i));
        }
      }
      __syncthreads();
      if (l < nl)
        for (uint32_t i = k0; i < odd_len; i += kg)
          OD(i) = (-K.inv_eps) * OD(i);
      __syncthreads();
    }
    else {          // src/CDF97.cpp:633-666
      if (l < nl)
        for (uint32_t i = k0; i < odd_len; i += kg)
          OD(i) = (-K.eps) * OD(i);
      __syncthreads();
      if (l < nl)
        for (uint32_t i = k0; i < even_len; i += kg) {
          const uint32_t a = max(i, 1u) - 1, b = min(i, odd_len - 1);
          const double t = K.delta * (OD(a) + OD(b));
          EV(i) = fma(EV(i), K.inv_eps, -t);
        }
      __syncthreads();
      odd_step(-K.gamma);
      even_step(-K.beta);
      odd_step(-K.alpha);
    }
#undef EV
#undef OD
  }

  // ---- store ----
  // (crop variant: sample (line l, position p) goes to the box when it lies in the chunk's window)
  auto crop_store = [&](uint32_t l, uint32_t p, VT v) {
    uint32_t xyz[3];
    xyz[axis] = p;
    xyz[ua] = u0 + l;
    xyz[wa] = tw;
    if (crop_has(cg, xyz[0], xyz[1], xyz[2]))
      vol[crop_addr(cg, vd, xyz[0], xyz[1], xyz[2])] = v;
  };
  (void)crop_store;
  const bool wantMax = FORWARD && F.mode == 1 && !is_const;
  double vmax = 0.0;
  if (axis == 0) {
    const uint32_t nseg = (len + 63) / 64;
    for (uint32_t sg = tid / 64; sg < nl * nseg; sg += kThreads / 64) {
      const uint32_t l = sg / nseg, p = (sg % nseg) * 64 + tid % 64;
      if (p >= len)
        continue;
      const uint32_t src = FORWARD ? p : ((p & 1) ? even_len + (p >> 1) : (p >> 1));
      if constexpr (kCrop)
        crop_store(l, p, (VT)(is_const ? mean : sm[src * NLP + l] + mean));
      else if (IO != 0 && !FORWARD)
        vol[vbase + l * vsu + p * vsl] = (VT)(is_const ? mean : sm[src * NLP + l] + mean);
      else {
        const double v = sm[src * NLP + l];
        tile[l * su + p] = v;
        size_t idx;
        if (wantMax && outside_inner(l, p, idx))
          vmax = fmax(vmax, fabs(v));
      }
    }
  }
  else {
    const uint32_t l = tid % NL, k0 = tid / NL, kg = kThreads / NL;
    if (l < nl)
      for (uint32_t p = k0; p < len; p += kg) {
        const uint32_t src = FORWARD ? p : ((p & 1) ? even_len + (p >> 1) : (p >> 1));
        if constexpr (kCrop)
          crop_store(l, p, (VT)(is_const ? mean : sm[src * NLP + l] + mean));
        else if (IO != 0 && !FORWARD)
          vol[vbase + l * vsu + p * vsl] = (VT)(is_const ? mean : sm[src * NLP + l] + mean);
        else {
          const double v = sm[src * NLP + l];
          tile[l * su + p * sl] = v;
          size_t idx;
          if (wantMax && outside_inner(l, p, idx))
            vmax = fmax(vmax, fabs(v));
        }
      }
  }
  if (FORWARD && F.mode == 1) {   // (uniform: every wavefront reduces, one atomic each)
    for (int d = 32; d > 0; d >>= 1)
      vmax = fmax(vmax, __shfl_xor(vmax, d, 64));
    if ((tid & 63) == 0 && vmax > 0.0)  // non-negative doubles order like their bit patterns
      atomicMax(reinterpret_cast<unsigned long long*>(&st[c].maxabs),
                (unsigned long long)__double_as_longlong(vmax));
  }
}

// ------------------------------------------------------------------------------------------
// The two passes of the finest level that touch the volume, fused: forward x-lift then y-lift
// (volume -> fp64 buffer), inverse y-lift then x-lift (fp64 buffer -> volume).  A workgroup owns
// R rows of one z-slice and stages them in LDS together with a halo of 4 rows on each side: the
// four lifting steps reach one row further each, so rows y0-4 .. y0+R+3 determine the R rows
// exactly (the symmetric boundary rule only ever refers to rows of the slice itself).  Every
// sample goes through the very same operations as in k_lift_axis; halo rows are recomputed by the
// neighbouring tiles.  Saves one full read + write of the fp64 buffer per direction.
// The lifting itself runs in registers (lift16): the first version kept every intermediate in LDS
// and was bound by LDS bandwidth (about 40 eight-byte LDS accesses per sample against 12 bytes of
// HBM traffic); now a sample costs about 6.
// ------------------------------------------------------------------------------------------
constexpr int kXYThreads = 512;    // two workgroups per CU (LDS) = 4 waves per SIMD: 128 VGPRs each
constexpr int kStage = 16;         // global loads a lane has in flight while staging
constexpr int kSeg = 8;            // samples a thread produces per pass (plus 4 + 4 halo = 16 registers)

// (lift16, lift_window: lift_window.h; kXYHalo, reflect_index, dyn_smem: lift_dev.h)

// kCrop (inverse only): the tile's rows of the chunk's window go to the box; a tile without one returns
template <bool FORWARD, int IO, bool kCrop = false>
__global__ void __launch_bounds__(kXYThreads)
k_lift_xy(double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz, int R,
          LiftConsts K, const CoderState* st, void* volume, VolDesc vd, const GeomOf<kCrop>* geom)
{
  static_assert(IO == 1 || IO == 2, "float or double volume");
  static_assert(!kCrop || !FORWARD, "the crop variant is a last inverse pass");
  using VT = typename std::conditional<IO == 1, float, double>::type;
  const uint32_t c = blockIdx.y;
  const bool is_const = st[c].is_const != 0;
  if (is_const && FORWARD)
    return;
  double* sm = reinterpret_cast<double*>(dyn_smem);
  const uint32_t ntile = (cy + R - 1) / R;
  const uint32_t z = blockIdx.x / ntile, y0 = (blockIdx.x % ntile) * R;
  const uint32_t ylo = y0 >= (uint32_t)kXYHalo ? y0 - kXYHalo : 0u;
  const uint32_t yhi = min(cy, y0 + R + kXYHalo);       // rows [ylo, yhi) are staged
  const uint32_t yend = min(cy, y0 + R);                // rows [y0, yend) are this tile's output
  const uint32_t nrow = yhi - ylo;
  const uint32_t RS = cx + 1;                           // row stride in LDS
  const uint32_t xe = cx - cx / 2, ye = cy - cy / 2;    // even samples of a row / of a column
  const GeomOf<kCrop> g = geom[c];
  VT* vol = reinterpret_cast<VT*>(volume);
  const size_t vsy = vd.dims[0], vsz = (size_t)vd.dims[0] * vd.dims[1];
  size_t vbase = 0;
  // rows [wy0, wy1) and columns [wx0, wx1) of the tile are written (all of them but in the crop variant)
  uint32_t wy0 = y0, wy1 = yend, wx0 = 0, wx1 = cx;
  if constexpr (kCrop) {   // (uniform)
    wy0 = max(y0, g.lo[1]);
    wy1 = min(yend, g.hi[1]);
    wx0 = g.lo[0];
    wx1 = g.hi[0];
    if (z - g.lo[2] >= g.hi[2] - g.lo[2] || wy0 >= wy1)
      return;
  }
  else
    vbase = (size_t)(g.org[2] + z) * vsz + (size_t)g.org[1] * vsy + g.org[0];
  // address of sample (x, y) of the tile's slice
  auto out_at = [&](uint32_t x, uint32_t y) -> size_t {
    if constexpr (kCrop)
      return crop_addr(g, vd, x, y, z);
    else
      return vbase + (size_t)y * vsy + x;
  };
  double* buf = vals + c * valsStride + (size_t)z * cx * cy;
  const double mean = st[c].mean;
  const uint32_t tid = threadIdx.x;

  if (is_const) {   // inverse only: the chunk is its constant
    if constexpr (kCrop) {
      const uint32_t w = wx1 - wx0;
      for (uint32_t k = tid; k < (wy1 - wy0) * w; k += kXYThreads)
        vol[out_at(wx0 + k % w, wy0 + k / w)] = (VT)mean;
    }
    else
      for (uint32_t k = tid; k < (yend - y0) * cx; k += kXYThreads)
        vol[vbase + (size_t)(y0 + k / cx) * vsy + k % cx] = (VT)mean;
    return;
  }

  // ---- stage the rows.  In LDS everything is interleaved (sample x of row y at [y - ylo][x]).
  // One wavefront per row, 64 samples per load; a lane issues kStage loads before it touches the
  // first value, so a workgroup keeps its whole tile in flight (one load at a time per wavefront
  // left the kernel waiting on HBM latency).
  const uint32_t lane = tid & 63u, wave = tid >> 6, nwaves = kXYThreads / 64;
  {
    using ST = typename std::conditional<FORWARD, VT, double>::type;
    const uint32_t nxb = (cx + 63) / 64;
    const uint32_t rowsW = nrow > wave ? (nrow - wave + nwaves - 1) / nwaves : 0;
    const uint32_t items = rowsW * nxb;        // (row, 64-sample block) pairs of this wavefront
    uint32_t ri = 0, bi = 0;                   // pair m = (row wave + nwaves * ri, block bi)
    for (uint32_t m0 = 0; m0 < items; m0 += kStage) {
      ST v[kStage];
      uint32_t ri2 = ri, bi2 = bi;
#pragma unroll
      for (int u = 0; u < kStage; u++) {
        const uint32_t j = wave + nwaves * ri2, x = lane + 64 * bi2;
        v[u] = 0;
        if (m0 + u < items && x < cx) {
          const uint32_t y = ylo + j;
          if (FORWARD)
            v[u] = (ST)vol[vbase + (size_t)y * vsy + x];
          else   // the buffer holds low | high halves along x and along y
            v[u] = (ST)buf[(size_t)((y & 1) ? ye + (y >> 1) : (y >> 1)) * cx + ((x & 1) ? xe + (x >> 1) : (x >> 1))];
        }
        if (++bi2 == nxb) {
          bi2 = 0;
          ri2++;
        }
      }
#pragma unroll
      for (int u = 0; u < kStage; u++) {
        const uint32_t j = wave + nwaves * ri, x = lane + 64 * bi;
        if (m0 + u < items && x < cx)
          sm[j * RS + x] = FORWARD ? (double)v[u] - mean : (double)v[u];
        if (++bi == nxb) {
          bi = 0;
          ri++;
        }
      }
    }
  }
  __syncthreads();

  // ---- the passes.  A thread takes 8 consecutive samples of a row (or of a column) together
  // with a halo of 4 on each side into registers (lift16) and writes only its 8 results back.
  // Rows are independent in the x pass and columns in the y pass, so one round handles whole rows
  // (columns): all loads of a round precede its stores.
  const uint32_t nseg = (cx + kSeg - 1) / kSeg;
  auto lift_x = [&](uint32_t jlo, uint32_t jhi) {          // staged rows [jlo, jhi), in place
    // lanes of a wavefront take different rows: addresses differ by the (odd) row stride
    const uint32_t rpr = min(32u, (uint32_t)kXYThreads / nseg);
    const uint32_t l = tid % rpr, sg = tid / rpr;
    for (uint32_t rb = jlo; rb < jhi; rb += rpr) {
      const bool on = sg < nseg && rb + l < jhi;
      double* row = sm + (size_t)(rb + l) * RS;
      const int s = (int)(sg * kSeg);
      double r[16];
      if (on) {
        if (s >= 4 && s + 12 <= (int)cx) {
#pragma unroll
          for (int k = 0; k < 16; k++)
            r[k] = row[s - 4 + k];
        }
        else {
#pragma unroll
          for (int k = 0; k < 16; k++)
            r[k] = row[reflect_index(s - 4 + k, (int)cx)];
        }
        lift16<FORWARD>(r, K);
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int k = 0; k < kSeg; k++)
          if ((uint32_t)(s + k) < cx)
            row[s + k] = r[4 + k];
      }
      __syncthreads();
    }
  };

  // y direction: thread = (column, 8 rows of the tile); lanes take consecutive columns
  const uint32_t nq = (yend - y0 + kSeg - 1) / kSeg;
  const uint32_t cpr = (uint32_t)kXYThreads / nq;          // columns per round
  auto load_column = [&](uint32_t x, uint32_t q, double (&r)[16]) {
    const int s = (int)(y0 + q * kSeg);
    const double* col = sm + x;
    if (s - 4 >= (int)ylo && s + 12 <= (int)yhi) {   // all 16 rows are staged rows of the slice
      const double* top = col + (size_t)(s - 4 - (int)ylo) * RS;
#pragma unroll
      for (int k = 0; k < 16; k++)
        r[k] = top[(size_t)k * RS];
    }
    else {
#pragma unroll
      for (int k = 0; k < 16; k++) {
        // rows outside the slice mirror into it; what lies outside the staged rows is clamped
        // into them: it cannot reach the tile's own rows (see above)
        const uint32_t yy = min(max(reflect_index(s - 4 + k, (int)cy), ylo), yhi - 1);
        r[k] = col[(size_t)(yy - ylo) * RS];
      }
    }
  };

  if (FORWARD) {
    lift_x(0, nrow);
    // y pass straight from LDS into the buffer: low | high halves along both axes
    for (uint32_t xb = 0; xb < cx; xb += cpr) {
      const uint32_t x = xb + tid % cpr, q = tid / cpr;
      if (x < cx && q < nq) {
        double r[16];
        load_column(x, q, r);
        lift16<true>(r, K);
        const uint32_t dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
#pragma unroll
        for (int k = 0; k < kSeg; k++) {
          const uint32_t y = y0 + q * kSeg + k;
          if (y < yend)
            buf[(size_t)((y & 1) ? ye + (y >> 1) : (y >> 1)) * cx + dcol] = r[4 + k];
        }
      }
    }
  }
  else {
    for (uint32_t xb = 0; xb < cx; xb += cpr) {
      const uint32_t x = xb + tid % cpr, q = tid / cpr;
      const bool on = x < cx && q < nq;
      double r[16];
      if (on) {
        load_column(x, q, r);
        lift16<false>(r, K);
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int k = 0; k < kSeg; k++) {
          const uint32_t y = y0 + q * kSeg + k;
          if (y < yend)
            sm[(size_t)(y - ylo) * RS + x] = r[4 + k];
        }
      }
    }
    __syncthreads();
    lift_x(y0 - ylo, yend - ylo);   // (only the tile's own rows go on)
    if constexpr (kCrop) {
      for (uint32_t y = wy0 + wave; y < wy1; y += nwaves) {
        VT* dstrow = vol + out_at(wx0, y);   // (any x origin: one sample per lane)
        const double* srow = sm + (size_t)(y - ylo) * RS;
        for (uint32_t x = wx0 + lane; x < wx1; x += 64)
          dstrow[x - wx0] = (VT)(srow[x] + mean);
      }
    }
    else
    for (uint32_t y = y0 + wave; y < yend; y += nwaves) {
      VT* dstrow = vol + vbase + (size_t)y * vsy;
      const double* srow = sm + (size_t)(y - ylo) * RS;
      for (uint32_t x = lane; x < cx; x += 64)
        dstrow[x] = (VT)(srow[x] + mean);
    }
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------

LiftConsts lift_consts()
{
  // include/CDF97.h:136-147 evaluated in IEEE fp64 (bit patterns: SURVEY.md Appendix B)
  auto bits = [](uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
  };
  LiftConsts k;
  k.alpha = bits(0xbff960ce676352c0ull);
  k.beta = bits(0xbfab2035c938c1f9ull);
  k.gamma = bits(0x3fec40ceba5579b7ull);
  k.delta = bits(0x3fdc626a9045727dull);
  k.eps = bits(0x3ff264c795071559ull);
  k.inv_eps = bits(0x3febd5edf975cca4ull);
  return k;
}

// Lines per tile.  The kernel is HBM-bound and synchronises between lifting steps, so it wants
// several workgroups per CU: measured on MI355X (256-sample lines) 8 lines per tile are best along
// x, where a wavefront reads along the line, and 16 across (128-byte rows); larger tiles halve the
// throughput.
static int pick_nl(uint32_t len, int axis, size_t* smem)
{
  // (measured again with the dequantising inverse passes, SPERR_HIP_LIFT_LDS_KB: 20 / 36 / 72 KB
  //  along y and z give 9.1 / 8.3 / 11.5 ms for the 13 inverse passes of the bench volume)
  static const int capYZ = tune_getenv("SPERR_HIP_LIFT_LDS_KB") ? atoi(tune_getenv("SPERR_HIP_LIFT_LDS_KB")) : 36;
  const size_t cap = (size_t)(axis == 0 ? 20 : capYZ) * 1024;
  for (int nl = 32; nl >= 1; nl >>= 1) {
    const size_t bytes = (size_t)len * (nl + 1) * sizeof(double);
    if (bytes <= cap || nl == 1) {
      *smem = bytes;
      return nl;
    }
  }
  return 1;
}

int launch_lift(hipStream_t stream, bool forward, double* vals, size_t valsStride,
                uint32_t nchunks, const uint32_t cdims[3], int axis, const uint32_t region[3],
                CoderState* st, int io, void* volume, VolDesc vd, const ChunkGeom* geom,
                const LiftFuse* fuse, const CropGeom* crop)
{
  const LiftFuse F = fuse ? *fuse : LiftFuse{};
  if (crop && (forward || io == 0))
    return -1;
  {
    const void* fns[8] = {reinterpret_cast<const void*>(&k_lift_axis<true, 0>),
                          reinterpret_cast<const void*>(&k_lift_axis<true, 1>),
                          reinterpret_cast<const void*>(&k_lift_axis<true, 2>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 0>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 1>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 2>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 1, true>),
                          reinterpret_cast<const void*>(&k_lift_axis<false, 2, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const uint32_t len = region[axis];
  if (len < 2)
    return io ? -1 : 0;
  size_t smem = 0;
  const int NL = pick_nl(len, axis, &smem);
  if (smem > 160 * 1024) {
    fprintf(stderr, "[sperr_hip] line of %u samples does not fit in LDS\n", len);
    return -1;
  }
  const int ua = (axis == 0) ? 1 : 0, wa = (axis == 2) ? 1 : 2;
  const uint32_t ntu = (region[ua] + NL - 1) / NL;
  dim3 grid(ntu * region[wa], nchunks);
  const LiftConsts K = lift_consts();
#define LIFT_ARGS vals, valsStride, cdims[0], cdims[1], axis, region[0], region[1], region[2], NL, K, st, volume, vd, geom, F
  if (forward) {
    if (io == 1)
      LAUNCH_K((k_lift_axis<true, 1>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else if (io == 2)
      LAUNCH_K((k_lift_axis<true, 2>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else
      LAUNCH_K((k_lift_axis<true, 0>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
  }
  else if (crop) {
#define CROP_ARGS vals, valsStride, cdims[0], cdims[1], axis, region[0], region[1], region[2], NL, K, st, volume, vd, crop, F
    if (io == 1)
      LAUNCH_K((k_lift_axis<false, 1, true>), grid, dim3(kThreads), smem, stream, CROP_ARGS);
    else
      LAUNCH_K((k_lift_axis<false, 2, true>), grid, dim3(kThreads), smem, stream, CROP_ARGS);
#undef CROP_ARGS
  }
  else {
    if (io == 1)
      LAUNCH_K((k_lift_axis<false, 1>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else if (io == 2)
      LAUNCH_K((k_lift_axis<false, 2>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
    else
      LAUNCH_K((k_lift_axis<false, 0>), grid, dim3(kThreads), smem, stream, LIFT_ARGS);
  }
#undef LIFT_ARGS
  HIP_CHECK(hipGetLastError());
  return 0;
}

// rows per tile of k_lift_xy for rows of cx samples, 0 when the fused kernel does not apply
static int xy_rows(uint32_t cx, uint32_t cy)
{
  if (cx < 2 || cy < 2)
    return 0;
  const size_t rowBytes = (size_t)(cx + 1) * sizeof(double);
  static const int ldsKB = tune_getenv("SPERR_HIP_XY_LDS_KB") ? atoi(tune_getenv("SPERR_HIP_XY_LDS_KB")) : 68;
  static const int maxRows = tune_getenv("SPERR_HIP_XY_ROWS") ? atoi(tune_getenv("SPERR_HIP_XY_ROWS")) : 32;
  int rows = (int)(((size_t)ldsKB * 1024) / rowBytes);
  if (rows > maxRows)
    rows = maxRows;
  int R = (rows - 2 * kXYHalo) & ~1;
  if (R <= 0)   // (rows of 1088 samples and more leave no tile: a negative R must not pass for a large one below)
    return 0;
  if ((uint32_t)R > cy)
    R = (int)((cy + 1) & ~1u);
  return R >= 8 ? R : 0;
}

bool lift_xy_applicable(const uint32_t cdims[3])
{
  return xy_rows(cdims[0], cdims[1]) > 0;
}

int launch_lift_xy(hipStream_t stream, bool forward, double* vals, size_t valsStride,
                   uint32_t nchunks, const uint32_t cdims[3], const CoderState* st, int io,
                   void* volume, VolDesc vd, const ChunkGeom* geom, const CropGeom* crop)
{
  if (crop && forward)
    return -1;
  {
    const void* fns[6] = {reinterpret_cast<const void*>(&k_lift_xy<true, 1>),
                          reinterpret_cast<const void*>(&k_lift_xy<true, 2>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 1>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 2>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 1, true>),
                          reinterpret_cast<const void*>(&k_lift_xy<false, 2, true>)};
    for (const void* f : fns)
      if (set_max_dyn_lds(f, 160 * 1024))
        return -1;
  }
  const int R = xy_rows(cdims[0], cdims[1]);
  if (R <= 0 || (io != 1 && io != 2))
    return -1;
  const size_t smem = (size_t)(R + 2 * kXYHalo) * (cdims[0] + 1) * sizeof(double);
  const uint32_t ntile = (cdims[1] + R - 1) / R;
  const dim3 grid(ntile * cdims[2], nchunks);
  const LiftConsts K = lift_consts();
#define XY_ARGS vals, valsStride, cdims[0], cdims[1], cdims[2], R, K, st, volume, vd, geom
  if (forward) {
    if (io == 1)
      LAUNCH_K((k_lift_xy<true, 1>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
    else
      LAUNCH_K((k_lift_xy<true, 2>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
  }
  else if (crop) {
#define CROP_ARGS vals, valsStride, cdims[0], cdims[1], cdims[2], R, K, st, volume, vd, crop
    if (io == 1)
      LAUNCH_K((k_lift_xy<false, 1, true>), grid, dim3(kXYThreads), smem, stream, CROP_ARGS);
    else
      LAUNCH_K((k_lift_xy<false, 2, true>), grid, dim3(kXYThreads), smem, stream, CROP_ARGS);
#undef CROP_ARGS
  }
  else {
    if (io == 1)
      LAUNCH_K((k_lift_xy<false, 1>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
    else
      LAUNCH_K((k_lift_xy<false, 2>), grid, dim3(kXYThreads), smem, stream, XY_ARGS);
  }
#undef XY_ARGS
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace sperrhip
