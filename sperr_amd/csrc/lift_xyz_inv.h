// lift_xyz_inv.h -- the body of the inverse three-pass lifting kernels and the finest level's kernel template.  Its ten
// instantiations are most of what the float stages take to compile, so two units share them: k_lift_xyz_inv<IO, SG>
// through the chunk map and the second level's k_lift2_inv<SG> in lift_xyz_inv.hip, the crop variants <IO, SG, true>
// in lift_xyz_inv_crop.hip (the split that compiles evenly: profiles/xform_units_codeobj.txt).  A unit instantiates
// (and launches) only its own.
//
// Reference behaviour restated (file:line of the reference):
//   src/CDF97.cpp:132-148,284-302,345-474,598-666   dyadic / wavelet-packet 3D transform (inverse lifting: 633-666)
#ifndef SPERR_AMD_LIFT_XYZ_INV_H
#define SPERR_AMD_LIFT_XYZ_INV_H

#include <type_traits>

#include "lift_xyz.h"
#include "dequant.h"

namespace sperrhip {

// SG: the coefficients carry their sign where the chunk allows it (DequantSrc::coefSigned, coef_scheme), a kernel of its own -- with both fast paths in
// one function the register allocator spilled inside the slice loop (88 registers against 38) and the kernel took 5.4 ms
// instead of 3.7
// kCrop: the rows of the chunk's window go to the box; a tile with no row in the window returns at once
// The body of the inverse kernels.  NPOS: positions per thread (kXYZStaged * cx <= NPOS * threads).
// L2: the second level (k_lift2_inv) -- `volume` is the chunk's own output box (rows and slices as `vd` says, no chunk
// map, nothing written for a constant chunk), and the coefficient, sign and mask arrays, which keep the CHUNK's dims, have
// rows of `qrowL2` samples and slices of `qsliceL2`; otherwise they are the region's, cx and cx * cy.
template <int IO, bool SG, bool kCrop, int NPOS, bool L2>
__device__ __forceinline__ void xyz_inv_body(const double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz,
                                             const LiftConsts& K, const CoderState* st, void* volume, const VolDesc& vd,
                                             const GeomOf<kCrop>* geom, const LiftFuse& F, uint32_t nseg, uint32_t qrowL2,
                                             size_t qsliceL2)
{
  static_assert(IO == 1 || IO == 2, "float or double volume");
  static_assert(!L2 || (IO == 2 && !kCrop), "the second level writes doubles into a box");
  constexpr int NGRP = NPOS < kXYZGroupI ? NPOS : kXYZGroupI;   // positions whose loads are in flight together
  using VT = typename std::conditional<IO == 1, float, double>::type;
  const uint32_t c = blockIdx.y;
  const uint32_t tid = threadIdx.x;
  // (small batches: `nseg` workgroups per tile share the slices, see k_lift_xyz_fwd; segment g finishes
  //  the slices that the pairs [mA, mB) complete, the last one also the end of the lines, and runs
  //  its pipelines six pairs ahead of that)
  const uint32_t seg = blockIdx.x % nseg, npairsAll = cz / 2;
  const uint32_t mA = seg == 0 ? 0u : (uint32_t)((uint64_t)npairsAll * seg / nseg);
  const uint32_t mB = seg + 1 == nseg ? npairsAll : (uint32_t)((uint64_t)npairsAll * (seg + 1) / nseg);
  const uint32_t mFirst = mA >= 6 ? mA - 6 : 0u;
  const uint32_t y0 = (blockIdx.x / nseg) * kXYZRows;
  const uint32_t nt = min((uint32_t)kXYZRows, cy - y0);
  const uint32_t RS = xyz_row_stride(cx);
  double* sm = reinterpret_cast<double*>(dyn_smem);
  const uint32_t bufN = (uint32_t)kXYZStaged * RS;
  const uint32_t xe = cx - cx / 2, ye = cy - cy / 2, ze = cz - cz / 2;
  VT* vol = reinterpret_cast<VT*>(volume);
  const size_t vsy = vd.dims[0], vsz = (size_t)vd.dims[0] * vd.dims[1];
  VT* volc = vol;
  CropGeom cg{};
  uint32_t wy0 = 0, wy1 = 0;   // crop variant: the tile's rows [y0 + wy0, y0 + wy1) lie in the window
  if constexpr (kCrop) {   // (uniform)
    cg = geom[c];
    wy0 = max(y0, cg.lo[1]) - y0;
    wy1 = min(y0 + nt, cg.hi[1]);
    if (y0 + wy0 >= wy1)
      return;
    wy1 -= y0;
  }
  else if constexpr (!L2)
    volc = vol + ((size_t)geom[c].org[2] * vsz + (size_t)geom[c].org[1] * vsy + geom[c].org[0]);
  // crop variant: row y0 + r of slice z -> the box row that holds its window, x = wx0 at its start
  auto crop_row = [&](uint32_t z, uint32_t r) -> VT* { return vol + crop_addr(cg, vd, cg.lo[0], y0 + r, z); };
  (void)crop_row;
  const double* buf = vals + c * valsStride;
  const uint32_t qrow = L2 ? qrowL2 : cx;                    // the coefficient arrays' rows and slices
  const size_t sliceN = L2 ? qsliceL2 : (size_t)cx * cy;
  const uint32_t bufx = F.bufx ? F.bufx : cx;                       // the chunk buffer may be compact:
  const size_t bufSlice = (size_t)bufx * (F.bufy ? F.bufy : cy);   // only the next level's box
  const double mean = st[c].mean;
  const uint32_t lane = tid & 63u, nwaves = kXYZThreadsI / 64;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (a scalar, and what is made of it)

  if constexpr (!L2) {   // (k_lift2_inv has returned for a constant chunk)
  if (st[c].is_const != 0) {   // the chunk is its constant
    if constexpr (kCrop) {
      const uint32_t w = cg.hi[0] - cg.lo[0], nr = wy1 - wy0;
      for (uint32_t z = cg.lo[2] + seg; z < cg.hi[2]; z += nseg)
        for (uint32_t k = tid; k < nr * w; k += kXYZThreadsI)
          crop_row(z, wy0 + k / w)[k % w] = (VT)mean;
    }
    else
    for (uint32_t z = seg; z < cz; z += nseg)
      for (uint32_t k = tid; k < nt * cx; k += kXYZThreadsI)
        volc[(size_t)z * vsz + (size_t)(y0 + k / cx) * vsy + k % cx] = (VT)mean;
    return;
  }
  }

  // position k of this thread: sample x of LDS row j = row ysrc of a slice (j << 27 | ysrc << 12 | x);
  // in the transformed chunk that is sample (dcol, drow): low | high halves along x and y
  const uint32_t npos = (uint32_t)kXYZStaged * cx;
  uint32_t pk[NPOS];
  uint32_t innerMask = 0;   // bit k: inside the next level's box along x and y
#pragma unroll
  for (int k = 0; k < NPOS; k++) {
    const uint32_t q = tid + (uint32_t)k * kXYZThreadsI;
    const uint32_t j = q / cx, x = q - j * cx, y = reflect_index((int)y0 - kXYHalo + (int)j, (int)cy);
    const uint32_t drow = (y & 1) ? ye + (y >> 1) : (y >> 1), dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
    pk[k] = (j << 27) | (y << 12) | x;
    if (dcol < F.inner[0] && drow < F.inner[1])
      innerMask |= 1u << k;
  }
  const bool dequant = F.mode == 2 && !st[c].wide;
  const double fq = dequant ? st[c].q : 0.0;
  const DequantSrc& Q = F.src;
  const uint32_t* coef = Q.coefs<uint32_t>(c);
  const uint64_t* sign = Q.sign + c * Q.signStride;
  // a coefficient that became significant on the last decoded plane / the one before and was never refined still
  // holds 0: its value comes from the decoder's masks.  (Without masks the rule completes nothing: the mask words
  // read are the sign's then, whatever they hold.)
  const bool haveMasks = dequant && Q.has_masks();
  const uint64_t* mNew = haveMasks ? Q.sigNew + c * Q.maskStride : sign;
  const uint64_t* mOld = haveMasks ? Q.sigOld + c * Q.maskStride : sign;
  // SG: the sign in bit 31, the value complete (k_ref_assemble, DequantSrc::coefSigned): neither the sign nor the mask
  // words are read (scheme 0: this chunk keeps magnitudes and masks)
  const DequantRule<uint32_t> rule = dequant_rule<uint32_t>(fq, haveMasks, haveMasks ? Q.dst + c : nullptr, SG);
  const int scheme = rule.scheme;
  auto sg_value = [&](uint32_t sv) -> double { return dequant_signed(rule, sv); };
  // sample (dcol, drow, zp): straight from the decoder (dequant.h) unless a coarser level's passes have produced it
  auto fetch = [&](int k, uint32_t zp) -> double {
    const uint32_t y = (pk[k] >> 12) & 0x7fffu, x = pk[k] & 0xfffu;
    const uint32_t drow = (y & 1) ? ye + (y >> 1) : (y >> 1), dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
    const size_t idx = (size_t)zp * sliceN + drow * qrow + dcol;
    const bool inBox = ((innerMask >> k) & 1u) && zp < F.inner[2];
    if (!dequant && !inBox && F.bufx)
      return 0.0;   // (a compact buffer holds the box only; the host asks for one only when every chunk dequantises here)
    if (dequant && !inBox) {
      if (SG && scheme)
        return sg_value(coef[idx]);
      const uint32_t v = coef[idx];
      const uint32_t sh = (uint32_t)(idx & 63);
      const uint64_t sgw = sign[idx >> 6], mnw = mNew[idx >> 6], mow = mOld[idx >> 6];   // (independent loads)
      return dequant_masks(rule, v, mnw, mow, sgw, sh);
    }
    return buf[(size_t)zp * bufSlice + drow * bufx + dcol];
  };
  // The slice of z-inverted samples staged in X (all staged rows) -> y pass into Y, x pass into the volume (kDirect,
  // see finish_slice) or, the box variant, back into X and from there into the box: X and Y then swap from slice
  // to slice, three barriers per slice.
  uint32_t flip = 0;
  // sample k of the slice that is finished next (its staging buffer is free: see finish_slice)
  auto stage = [&](int k, double v) {
    uint32_t p = pk[k];
    asm volatile("" : "+v"(p));   // (keeps the LDS address from being computed ahead and spilled)
    (sm + (flip ? bufN : 0u))[(p >> 27) * RS + 4 + (p & 0xfffu)] = v;
  };
  auto stage_all = [&](const double (&v)[NPOS]) {
#pragma unroll
    for (int k = 0; k < NPOS; k++)
      if ((tid + (uint32_t)k * kXYZThreadsI) < npos)
        stage(k, v[k]);
  };
  // rows of a finished slice (in staging buffer `which`) -> volume, mean added, narrowed
  auto store_rows = [&](uint32_t z, uint32_t which) {
    const double* X = sm + (which ? bufN : 0u);
    // (the lane's addresses are made anew for every slice: computed once, ahead of the loop, they are spilled, and a
    //  reload here waits for every load and store in flight)
    uint32_t lanev = lane;
    asm volatile("" : "+v"(lanev));
    if constexpr (kCrop) {   // (any x origin: one sample per lane)
      if (z - cg.lo[2] >= cg.hi[2] - cg.lo[2])
        return;
      for (uint32_t r = wy0 + wave; r < wy1; r += nwaves) {
        VT* dstrow = crop_row(z, r);
        const double* srow = X + (size_t)(kXYHalo + r) * RS + 4;
        for (uint32_t x = cg.lo[0] + lanev; x < cg.hi[0]; x += 64)
          dstrow[x - cg.lo[0]] = (VT)(F.noMean ? srow[x] : srow[x] + mean);
      }
      return;
    }
    if (xyz_off<XYZ_INV_OFF>(4, nseg))
      return;
    for (uint32_t r = wave; r < nt; r += nwaves) {
      VT* dstrow = volc + (size_t)z * vsz + (size_t)(y0 + r) * vsy;
      const double* srow = X + (size_t)(kXYHalo + r) * RS + 4;
      if (F.noMean) {   // (uniform)
        for (uint32_t x = lanev; x < cx; x += 64)
          dstrow[x] = (VT)srow[x];
      }
      else
        for (uint32_t x = lanev; x < cx; x += 64)
          dstrow[x] = (VT)(srow[x] + mean);
    }
  };
  // kDirect: the x pass writes the volume itself.  The slices are then all staged in the first buffer: its y pass has
  // read it when the barrier in front of the x pass is behind a wavefront, and the second buffer, which the x pass
  // reads, is written again only behind the next slice's first barrier.  Two barriers per slice.
  constexpr bool kDirect = !kCrop && XYZ_INV_XSTORE != 0;
  auto finish_slice = [&](uint32_t z) {
    uint32_t RSv = RS, tidv = tid;   // (see k_lift_xyz_fwd)
    asm volatile("" : "+s"(RSv), "+v"(tidv));
    const uint32_t which = flip;
    double* X = sm + (flip ? bufN : 0u);
    double* Y = sm + (flip ? 0u : bufN);
    if constexpr (!kDirect)
      flip ^= 1u;
    XYZ_LDS_BARRIER();
    if (!xyz_off<XYZ_INV_OFF>(2, nseg))
      xyz_lift_y<false, true, kXYZThreadsI, kXYZOutIY>(X, Y, RSv, cx, nt, tidv, K);
    XYZ_LDS_BARRIER();
    if constexpr (kDirect) {
      if (!xyz_off<XYZ_INV_OFF>(2, nseg))
        xyz_lift_x_store<kXYZThreadsI, kXYZOutIX>(Y, volc + (size_t)z * vsz + (size_t)y0 * vsy, vsy, RSv, cx, kXYHalo, kXYHalo + nt,
                                                   tidv, K, mean, F.noMean != 0, !xyz_off<XYZ_INV_OFF>(4, nseg));
      else   // (timing builds: the rows as they are)
        store_rows(z, which ^ 1u);
    }
    else {
      if (!xyz_off<XYZ_INV_OFF>(2, nseg))
        xyz_lift_x<false, kXYZThreadsI, kXYZOutIX>(Y, X, RSv, cx, kXYHalo, kXYHalo + nt, tidv, K);
      XYZ_LDS_BARRIER();
      store_rows(z, which);
      // (the next slice is staged into Y, which nobody reads any more; its y pass writes X only after
      //  the barrier behind that staging, when every row above has been stored)
    }
  };

  double o1p[NPOS], e1p[NPOS], o2p[NPOS], e2p[NPOS];
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    o1p[k] = e1p[k] = o2p[k] = e2p[k] = 0.0;
  const uint32_t npairs = cz / 2;
  // one pair (low[m], high[m]) of position k enters its pipeline; slice 2m-3's sample is staged
  auto zstep = [&](int k, uint32_t m, bool mine, bool active, double E, double O) {
    const double o1 = (-K.eps) * O;                                        // o1[m]
    const double t = K.delta * ((m == 0 ? o1 : o1p[k]) + o1);
    const double e1 = fma(E, K.inv_eps, -t);                               // e1[m]
    if (m >= 1) {
      const double o2 = fma(-K.gamma, e1p[k] + e1, o1p[k]);                // o2[m-1]
      const double e2 = fma(-K.beta, (m == 1 ? o2 : o2p[k]) + o2, e1p[k]); // e2[m-1]
      if (m >= 2 && mine && active)
        stage(k, fma(-K.alpha, e2p[k] + e2, o2p[k]));                      // o3[m-2]: slice 2m-3
      o2p[k] = o2;
      e2p[k] = e2;
    }
    o1p[k] = o1;
    e1p[k] = e1;
  };
#if XYZ_INV_PREFETCH == 2
  // Round 4.  The kernel spent half its time waiting for loads, one after the other: every sample's sign and
  // mask words sat behind a branch of their own (box or not), so a pair was some thirty-six dependent round
  // trips.  Now (chunks that dequantise here):
  //  * pair m + 1's coefficients travel from HBM straight into LDS (global_load_lds: no register holds them)
  //    while pair m's two slices go through the y and x passes; every wavefront has its own 64-dword row
  //    per (position, low / high half) behind the two staging buffers.  They are issued AFTER the pair's
  //    own loads: the memory counter retires in order, a wait for those would wait for these too;
  //  * the sign / mask dwords and the fp64 samples of the coarser levels' box (an eighth of all) are loaded
  //    without any branch -- a lane that does not need one reads a harmless address --, three positions'
  //    worth at a time: two round trips per pair.
  // The arithmetic per sample is what it was.
  uint32_t* myPre = reinterpret_cast<uint32_t*>(sm + 2 * (size_t)bufN) + (size_t)wave * (NPOS * 2 * 64);
  const uint32_t* sign32 = reinterpret_cast<const uint32_t*>(sign);
  const uint32_t* mNew32 = reinterpret_cast<const uint32_t*>(mNew);
  const uint32_t* mOld32 = reinterpret_cast<const uint32_t*>(mOld);
  uint32_t activeMask = 0;
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    if ((tid + (uint32_t)k * kXYZThreadsI) < npos)
      activeMask |= 1u << k;
    else
      pk[k] = pk[0];   // (a valid position: its loads are harmless, nothing of it is staged)
  uint32_t boxAny = 0;   // bit k: some lane of this wavefront has position k inside the coarser levels' box (along x and y)
#pragma unroll
  for (int k = 0; k < NPOS; k++)
    boxAny |= __ballot((innerMask >> k) & 1u) != 0ull ? 1u << k : 0u;
  boxAny = (uint32_t)__builtin_amdgcn_readfirstlane((int)boxAny);
  auto pos_off = [&](int k, uint32_t& drow, uint32_t& dcol) {
    const uint32_t y = (pk[k] >> 12) & 0x7fffu, x = pk[k] & 0xfffu;
    drow = (y & 1) ? ye + (y >> 1) : (y >> 1);
    dcol = (x & 1) ? xe + (x >> 1) : (x >> 1);
  };
  // (a high-half sample never lies in the next level's box when that box ends at or before the low half)
  const bool fastLoads = dequant && F.inner[2] <= ze && (!SG || scheme != 0);
  // The fp64 samples of the coarser levels' box THROUGH LDS as well (sign-in-word kernel, round 5): where the lanes of
  // a wavefront that are in the box are exactly its even ones -- rows of a multiple of 64 samples: 32 doubles in a row
  // of the chunk buffer --, the 256 bytes travel like a row of coefficients, a pair ahead (lane i fetches dword i),
  // and lane 2 i reads double i.  Two load round trips per pair in half the wavefronts, with the other half waiting
  // for them at the barrier, before.  A slot per (wavefront, position) that has a box row: 12 rows x cx / 64 <= 48.
  uint32_t boxLds = 0, boxSlot0 = 0;   // (wave-uniform) bit k: position k's box samples come through LDS; the wavefront's first slot
  uint32_t* boxRows = reinterpret_cast<uint32_t*>(sm + 2 * (size_t)bufN) + (size_t)nwaves * (NPOS * 2 * 64);
  if (SG && fastLoads) {
    uint32_t reg = 0;
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      const uint64_t inb = __ballot((innerMask >> k) & 1u), act = __ballot((activeMask >> k) & 1u);
      if (inb == 0x5555555555555555ull && act == ~0ull && (cx & 63u) == 0)
        reg |= 1u << k;
    }
    reg = (uint32_t)__builtin_amdgcn_readfirstlane((int)reg);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(sm);   // (the staging buffers are not in use yet)
    if (lane == 0)
      cnt[wave] = (uint32_t)__popc(reg);
    XYZ_LDS_BARRIER();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < nwaves; w++) {
      const uint32_t v = cnt[w];
      before += w < wave ? v : 0u;
      total += v;
    }
    XYZ_LDS_BARRIER();
    if (total <= (uint32_t)kXYZBoxSlots && reg == (1u << NPOS) - 1u) {   // (all of the wavefront's positions or none)
      boxLds = reg;
      boxSlot0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
    }
  }
  uint32_t* myBox = boxRows + (size_t)boxSlot0 * 64;   // position k's row: myBox + k * 64
  auto pre_issue = [&](uint32_t m) {
    if (xyz_off<XYZ_INV_OFF>(1, nseg))
      return;
    // (the box rows first: what their addresses are made of may have to come back from scratch, and behind the
    //  coefficients' loads that reload would wait for every one of them -- the memory counter retires in order)
    if (SG && boxLds != 0 && m < F.inner[2]) {   // (uniform)
#pragma unroll
      for (int k = 0; k < NPOS; k++) {
        uint32_t drow, dcol;
        pos_off(k, drow, dcol);
        const uint32_t x0h = ((pk[k] & 0xfffu) - lane) >> 1;   // the box column of the wavefront's first lane
        const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + ((size_t)m * bufSlice + (size_t)drow * bufx + x0h)) + lane;
        __builtin_amdgcn_global_load_lds(src, myBox + k * 64, 4, 0, 0);
      }
    }
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      uint32_t drow, dcol;
      pos_off(k, drow, dcol);
      const uint32_t off = drow * qrow + dcol;
      __builtin_amdgcn_global_load_lds(coef + ((size_t)m * sliceN + off), myPre + (k * 2) * 64, 4, 0, 0);
      __builtin_amdgcn_global_load_lds(coef + ((size_t)(ze + m) * sliceN + off), myPre + (k * 2 + 1) * 64, 4, 0, 0);
    }
  };
  if (fastLoads && mFirst < mB)
    pre_issue(mFirst);
#endif
  for (uint32_t m = mFirst; m < mB; m++) {
    const bool mine = m >= mA;   // (else: the segment's run-up)
#pragma unroll
    for (int k = 0; k < NPOS; k++)
      asm volatile("" : "+v"(pk[k]));
#if XYZ_INV_PREFETCH == 2
    if (SG && fastLoads) {
      // (round 5) the coefficients carry their sign and are complete: a pair's global loads are the fp64 samples of
      // the coarser levels' box alone -- and only in the wavefronts that have a lane in the box (with 256 samples a
      // row: those whose rows are the even ones)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this pair's coefficients have landed in LDS (and its box rows)
      const bool boxWave = boxAny != 0 && m < F.inner[2];   // (uniform)
      const bool zOn = !xyz_off<XYZ_INV_OFF>(8, nseg);
      if (zOn && boxWave && boxLds != 0) {   // the box samples were prefetched with the coefficients
#pragma unroll
        for (int k = 0; k < NPOS; k++) {
          const double lo = sg_value(myPre[(k * 2) * 64 + lane]);
          const double hi = sg_value(myPre[(k * 2 + 1) * 64 + lane]);
          const double bxv = reinterpret_cast<const double*>(myBox + k * 64)[lane >> 1];
          zstep(k, m, mine, true, (lane & 1u) ? lo : bxv, hi);   // (the even lanes are the ones in the box)
        }
      }
      else if (zOn) {
#pragma unroll
      for (int g = 0; g < NPOS; g += NGRP) {
        __builtin_amdgcn_sched_barrier(0);   // (NGRP positions' loads in flight at a time)
        double bx[NGRP];
        uint32_t boxm = 0;
        if (boxWave) {
#pragma unroll
          for (int kk = 0; kk < NGRP; kk++) {
            const int k = g + kk;
            if (k >= NPOS)
              continue;
            uint32_t drow, dcol;
            pos_off(k, drow, dcol);
            const bool inBox = ((innerMask >> k) & 1u) != 0;
            boxm |= inBox ? 1u << kk : 0u;
            bx[kk] = buf[inBox ? (size_t)m * bufSlice + drow * bufx + dcol : (size_t)0];
          }
        }
#pragma unroll
        for (int kk = 0; kk < NGRP; kk++) {
          const int k = g + kk;
          if (k >= NPOS)
            continue;
          const double lo = sg_value(myPre[(k * 2) * 64 + lane]);
          const double hi = sg_value(myPre[(k * 2 + 1) * 64 + lane]);
          zstep(k, m, mine, ((activeMask >> k) & 1u) != 0, ((boxm >> kk) & 1u) ? bx[kk] : lo, hi);
        }
      }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (m + 1 < mB)
        pre_issue(m + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    else if (!SG && fastLoads) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this pair's coefficients have landed in LDS
#pragma unroll
      for (int g = 0; g < NPOS; g += NGRP) {
        __builtin_amdgcn_sched_barrier(0);   // (NGRP positions' loads in flight at a time)
        constexpr int NV = 2 * NGRP;
        uint32_t sgw[NV], mnw[NV], mow[NV], cv[NV], shv[NV], boxm = 0;
        double bx[NGRP];   // (only a low-half sample can lie in the box: fastLoads)
#pragma unroll
        for (int j = 0; j < NV; j++) {
          const int k = g + j / 2;
          if (k >= NPOS)
            continue;
          const uint32_t zp = (j & 1) ? ze + m : m;
          uint32_t drow, dcol;
          pos_off(k, drow, dcol);
          const size_t idx = (size_t)zp * sliceN + drow * qrow + dcol;
          sgw[j] = sign32[idx >> 5];
          mnw[j] = mNew32[idx >> 5];
          mow[j] = mOld32[idx >> 5];
          if ((j & 1) == 0) {
            const bool inBox = ((innerMask >> k) & 1u) && zp < F.inner[2];
            boxm |= inBox ? 1u << j : 0u;
            bx[j / 2] = buf[inBox ? (size_t)zp * bufSlice + drow * bufx + dcol : (size_t)0];
          }
          cv[j] = myPre[(k * 2 + (j & 1)) * 64 + lane];
          shv[j] = (uint32_t)idx & 31u;
        }
        double val[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) {
          if (g + j / 2 >= NPOS)
            continue;
          const double dq = dequant_masks(rule, cv[j], mnw[j], mow[j], sgw[j], shv[j]);
          val[j] = ((j & 1) == 0 && ((boxm >> j) & 1u)) ? bx[j / 2] : dq;
        }
#pragma unroll
        for (int kk = 0; kk < NGRP; kk++)
          if (g + kk < NPOS)
            zstep(g + kk, m, mine, ((activeMask >> (g + kk)) & 1u) != 0, val[2 * kk], val[2 * kk + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (m + 1 < mB)
        pre_issue(m + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    else
#endif
    {
#pragma unroll
      for (int k = 0; k < NPOS; k++) {
        if ((k % 3) == 0)
          __builtin_amdgcn_sched_barrier(0);   // (four positions' loads in flight at a time, not all twelve)
        if ((tid + (uint32_t)k * kXYZThreadsI) >= npos)
          continue;
        const double E = fetch(k, m), O = fetch(k, ze + m);
        zstep(k, m, mine, true, E, O);
      }
    }
    if (m >= 2 && mine)
      finish_slice(2 * m - 3);
    if (m >= 1 && mine) {
      stage_all(e2p);
      finish_slice(2 * m - 2);
    }
  }
  // ---- the end of the lines (the last segment's)
  if (seg + 1 != nseg)
    return;
  if ((cz & 1) == 0) {   // pairs 0 .. M, M = cz / 2 - 1
    const uint32_t M = npairs - 1;
    double outC[NPOS];
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      outC[k] = 0.0;
      if ((tid + (uint32_t)k * kXYZThreadsI) >= npos)
        continue;
      const double o2 = fma(-K.gamma, e1p[k] + e1p[k], o1p[k]);              // o2[M]
      const double e2 = fma(-K.beta, o2p[k] + o2, e1p[k]);                   // e2[M]
      stage(k, fma(-K.alpha, e2p[k] + e2, o2p[k]));                          // o3[M-1]: slice 2M-1
      e2p[k] = e2;                                                           // slice 2M
      outC[k] = fma(-K.alpha, e2 + e2, o2);                                  // o3[M]: slice 2M+1
    }
    finish_slice(2 * M - 1);
    stage_all(e2p);
    finish_slice(2 * M);
    stage_all(outC);
    finish_slice(2 * M + 1);
  }
  else {                 // pairs 0 .. M-1 and the lone even sample low[M], M = cz / 2
    const uint32_t M = npairs;
    double outC[NPOS], outD[NPOS];
#pragma unroll
    for (int k = 0; k < NPOS; k++) {
      outC[k] = outD[k] = 0.0;
      if ((tid + (uint32_t)k * kXYZThreadsI) >= npos)
        continue;
      const double E = fetch(k, M);
      const double t = K.delta * (o1p[k] + o1p[k]);
      const double e1 = fma(E, K.inv_eps, -t);                               // e1[M]
      const double o2 = fma(-K.gamma, e1p[k] + e1, o1p[k]);                  // o2[M-1]
      const double e2 = fma(-K.beta, o2p[k] + o2, e1p[k]);                   // e2[M-1]
      stage(k, fma(-K.alpha, e2p[k] + e2, o2p[k]));                          // o3[M-2]: slice 2M-3
      e2p[k] = e2;                                                           // slice 2M-2
      const double e2L = fma(-K.beta, o2 + o2, e1);                          // e2[M]: slice 2M
      outC[k] = fma(-K.alpha, e2 + e2L, o2);                                 // o3[M-1]: slice 2M-1
      outD[k] = e2L;
    }
    finish_slice(2 * M - 3);
    stage_all(e2p);
    finish_slice(2 * M - 2);
    stage_all(outC);
    finish_slice(2 * M - 1);
    stage_all(outD);
    finish_slice(2 * M);
  }
}

template <int IO, bool SG, bool kCrop = false>
__global__ void __launch_bounds__(kXYZThreadsI) __attribute__((amdgpu_waves_per_eu(kXYZThreadsI / 256, kXYZThreadsI / 256)))
k_lift_xyz_inv(const double* vals, size_t valsStride, uint32_t cx, uint32_t cy, uint32_t cz, LiftConsts K,
               const CoderState* st, void* volume, VolDesc vd, const GeomOf<kCrop>* geom, LiftFuse F, uint32_t nseg)
{
  xyz_inv_body<IO, SG, kCrop, kXYZPosI, false>(vals, valsStride, cx, cy, cz, K, st, volume, vd, geom, F, nseg, 0u, 0);
}

}  // namespace sperrhip

#endif

