// quality.hip -- the quality figures of a reconstruction for arrays that live on the device: the block partials of
// sperr::calc_stats<T> and sperr::calc_mean_var<T> (src/sperr_helper.cpp:429-518,594-641 of the reference) as HIP
// kernels for gfx950, and the host finish of quality.h.  Every operation is in T with the reference's order; compile
// with -ffp-contract=off (the reference build fuses nothing here).  Denormals are kept (hipcc's default for gfx9):
// squares of differences around 1e-21 are subnormal floats and count.
//
// One ROW is a block of 16384 values -- the unit of the mean and variance sums, and two blocks of 8192 of the squared
// differences -- or the tail of an array.  An array of n values has n / 16384 + 1 rows, the last one its tail (which
// may be empty); a batch is the rows of all its arrays in one list, so the array index is part of the grid.
//
//   k_quality_rows<T, false>   a, b -> per row: sum of a, two sums of d * d, max d, min / max of a, any a != b
//   k_quality_mean<T>          per array: the row sums of a in order -> mean; max d, min, max, differ over its rows
//   k_quality_rows<T, true>    a, mean -> per row: sum of (a - mean) * (a - mean)
//
// k_quality_rows<T, kVar, true> is the same kernel over two strided views (view.h) of one shape: the rows are those
// of the views' own linear order, so every sum has the addends and the order of the dense kernel on packed copies;
// only the addresses the values are loaded from differ.
//
// The sums over the rows' squared differences and variance partials are not needed on the device: the host adds them
// in order after the call's one read-back (quality_finish).
#include "common.h"
#include "quality.h"
#include "view.h"

#include <type_traits>
#include <vector>

namespace sperrhip {

// A workgroup takes kQualRows rows and walks them kQualSeg values at a time: all threads load the segment of every
// row with 16-byte loads, consecutive lanes on consecutive addresses, do everything that has no order (d, d * d, max,
// min, !=) and put the addends into LDS; then one lane per row adds its row of the tile in order (k_stride_sums'
// shape).  The next segment's loads are issued before the adds, so that they fly while one wavefront adds.
constexpr int kQualRows = 16, kQualSeg = 128, kQualThreads = 256;
constexpr int kQualStage = 1024;   // row sums k_quality_mean stages in LDS per round
constexpr int kQualGroup = 16;     //   ... and reads from there at a time (kQualStage is a multiple)

// 16 bytes of T that need only T's alignment: neither array's base is promised more (a slice of a batch of odd n, a
// tensor view), and the two may differ.  gfx950 takes a global_load_dwordx4 at any dword address.
template <typename T>
struct QualPack {
  T v[16 / sizeof(T)];
};

// the same 16 bytes in the LDS tile, whose rows are 16-byte aligned
template <typename T>
struct alignas(16) QualTile {
  T v[16 / sizeof(T)];
};

__device__ __forceinline__ float qual_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double qual_abs(double v) { return __builtin_fabs(v); }

template <typename T>
struct QualWs {
  T* hdr;        // [nvol][8]: mean, max d, min, max, differ (0 / 1)
  T* sq;         // [rows][2]: sums of d * d of the row's two blocks of 8192
  T* var;        // [rows]
  T* asum;       // [rows]
  T* stats;      // [rows][4]: max d, min, max, differ
};

// how the view form walks its two arrays (they share the dims; the pitches may differ); the dense form takes none
struct QualViews {
  ViewWalk a, b;
};
struct QualNoViews {};

// A thread's pack of a view: the 16 bytes at the cursor when they lie in one x-row of the view and in the row of
// 16384 (`e` is the pack's place in it, `len` its length), else value by value with the carry into the next x-row and
// slice; +0 past the row's end, where nothing is read.  Consecutive lanes stand on consecutive elements, so within an
// x-row their addresses are consecutive too.
template <typename T>
__device__ __forceinline__ void qual_load_view(QualPack<T>& p, const T* __restrict__ base, const ViewCursor& c,
                                               const ViewWalk& w, uint32_t e, uint32_t len)
{
  constexpr uint32_t V = 16 / sizeof(T);
  if (e + V <= len && c.x + V <= w.dimx) {
    __builtin_memcpy(&p, base + c.row + c.x, 16);
    return;
  }
  ViewCursor k = c;
#pragma unroll
  for (uint32_t j = 0; j < V; j++) {
    p.v[j] = e + j < len ? base[k.row + k.x] : T(0);
    view_next(k, w);
  }
}

template <typename T, bool kVar, bool kView = false>
__global__ void __launch_bounds__(kQualThreads)
k_quality_rows(const T* __restrict__ a, const T* __restrict__ b, uint64_t n, uint64_t nrow, uint64_t totalRows,
               QualWs<T> ws, typename std::conditional<kView, QualViews, QualNoViews>::type vw)
{
  constexpr int V = 16 / sizeof(T);                        // values per pack
  constexpr int PPR = kQualSeg / V;                        // packs per row and segment
  constexpr int NP = kQualRows * PPR / kQualThreads;       // packs per thread and segment
  constexpr int RSTEP = kQualThreads / PPR;                // rows between a thread's packs
  constexpr int LD = kQualSeg + V;                         // (rows stay 16-byte aligned; lanes of a column spread over banks)
  static_assert(kQualThreads % PPR == 0 && NP >= 1 && kQualSqBlock % kQualSeg == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) T shA[kQualRows][LD];                  // a, or (a - mean)^2
  __shared__ __attribute__((aligned(16))) T shS[kVar ? 1 : kQualRows][LD];       // d * d
  __shared__ uint32_t shLen[kQualRows];

  const uint32_t t = threadIdx.x;
  const uint32_t col = (t % PPR) * V;
  const uint64_t g0 = (uint64_t)blockIdx.x * kQualRows;

  // this thread's rows: where they start, how long they are
  const T* pa[NP];
  const T* pb[NP];
  uint32_t len[NP];
  T mean[NP];
  ViewCursor ca[kView ? NP : 1], cb[kView ? NP : 1];   // (kView: where this thread's next pack of each row starts)
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const uint32_t rr = t / PPR + i * RSTEP;
    const uint64_t g = g0 + rr;
    len[i] = 0;
    pa[i] = a;
    pb[i] = b;
    mean[i] = 0;
    if constexpr (kView)
      ca[i] = cb[i] = ViewCursor{0, 0, 0};
    if (g < totalRows) {
      const uint64_t v = g / nrow, r = g - v * nrow;
      const uint64_t start = r * kQualMvBlock;               // <= n: the last row is the tail
      const uint64_t left = n - start;
      len[i] = (uint32_t)(left < kQualMvBlock ? left : kQualMvBlock);
      if constexpr (kView) {   // (one array each: v is 0.  The row's only 64-bit divisions)
        ca[i] = view_cursor(start + col, vw.a);
        if (!kVar)
          cb[i] = view_cursor(start + col, vw.b);
      }
      else {
        pa[i] = a + v * n + start;
        if (!kVar)
          pb[i] = b + v * n + start;
      }
      if (kVar)
        mean[i] = ws.hdr[v * 8];
    }
    if (t % PPR == 0)
      shLen[rr] = len[i];
  }
  __syncthreads();
  uint32_t maxLen = 0;
#pragma unroll
  for (int r = 0; r < kQualRows; r++)
    maxLen = max(maxLen, shLen[r]);

  QualPack<T> x[NP], y[NP];
  // the packs of segment `seg`; what lies past a row's end reads as +0.  (kView: the segments are asked for in order,
  // and the cursors move on to the same columns of the next one)
  auto load_seg = [&](uint32_t seg) {
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const uint32_t e = seg + col;
      if constexpr (kView) {
        qual_load_view(x[i], a, ca[i], vw.a, e, len[i]);
        view_advance(ca[i], vw.a, kQualSeg);
        if (!kVar) {
          qual_load_view(y[i], b, cb[i], vw.b, e, len[i]);
          view_advance(cb[i], vw.b, kQualSeg);
        }
      }
      else if (e + V <= len[i]) {
        __builtin_memcpy(&x[i], pa[i] + e, 16);
        if (!kVar)
          __builtin_memcpy(&y[i], pb[i] + e, 16);
      }
      else {
#pragma unroll
        for (int k = 0; k < V; k++) {
          const bool ok = e + k < len[i];
          x[i].v[k] = ok ? pa[i][e + k] : T(0);
          if (!kVar)
            y[i].v[k] = ok ? pb[i][e + k] : T(0);
        }
      }
    }
  };

  T linf[NP], mn[NP], mx[NP];
  bool ne[NP];
#pragma unroll
  for (int i = 0; i < NP; i++) {
    linf[i] = 0;
    mn[i] = INFINITY;
    mx[i] = -INFINITY;
    ne[i] = false;
  }
  // the adding lane of row t (t < kQualRows).  A value past a row's end is +0 in the tile and is added like any
  // other: x + (+0) == x for every x but -0, and a sum that starts at +0 is never -0 (round to nearest gives -0
  // only from two negative zeros).
  T accA = 0, accS = 0, sq0 = 0;
  bool pastHalf = false;

  if (maxLen > 0)
    load_seg(0);
  for (uint32_t seg = 0; seg < maxLen; seg += kQualSeg) {
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const uint32_t rr = t / PPR + i * RSTEP;
      const uint32_t e = seg + col;
      QualTile<T> pA, pS;
#pragma unroll
      for (int k = 0; k < V; k++) {
        const T xa = x[i].v[k];
        if (kVar) {
          const T c = xa - mean[i];
          pA.v[k] = e + k < len[i] ? c * c : T(0);
        }
        else {
          const T xb = y[i].v[k];
          const T d = qual_abs(xa - xb);
          pA.v[k] = xa;
          pS.v[k] = d * d;
          if (e + k < len[i]) {
            linf[i] = d > linf[i] ? d : linf[i];
            mn[i] = xa < mn[i] ? xa : mn[i];
            mx[i] = xa > mx[i] ? xa : mx[i];
            ne[i] |= xa != xb;
          }
        }
      }
      *reinterpret_cast<QualTile<T>*>(&shA[rr][col]) = pA;
      if (!kVar)
        *reinterpret_cast<QualTile<T>*>(&shS[rr][col]) = pS;
    }
    __syncthreads();
    if (seg + kQualSeg < maxLen)
      load_seg(seg + kQualSeg);
    if (t < (uint32_t)kQualRows) {
#pragma unroll 8
      for (int j = 0; j < kQualSeg; j += V) {
        const QualTile<T> qa = *reinterpret_cast<const QualTile<T>*>(&shA[t][j]);
#pragma unroll
        for (int k = 0; k < V; k++)
          accA += qa.v[k];
        if (!kVar) {
          const QualTile<T> qs = *reinterpret_cast<const QualTile<T>*>(&shS[t][j]);
#pragma unroll
          for (int k = 0; k < V; k++)
            accS += qs.v[k];
        }
      }
      if (!kVar && seg + kQualSeg == (uint32_t)kQualSqBlock) {   // the row's first block of 8192 ends here
        sq0 = accS;
        accS = 0;
        pastHalf = true;
      }
    }
    __syncthreads();
  }

  if (t < (uint32_t)kQualRows && g0 + t < totalRows) {
    const uint64_t g = g0 + t;
    if (kVar)
      ws.var[g] = accA;
    else {
      ws.asum[g] = accA;
      ws.sq[2 * g] = pastHalf ? sq0 : accS;
      ws.sq[2 * g + 1] = pastHalf ? accS : T(0);
    }
  }
  if (!kVar) {
#pragma unroll
    for (int i = 0; i < NP; i++) {
      T l = linf[i], lo = mn[i], hi = mx[i];
      int df = ne[i] ? 1 : 0;
#pragma unroll
      for (int d = PPR / 2; d > 0; d >>= 1) {            // the PPR consecutive lanes of one row
        const T l2 = __shfl_xor(l, d, 64), lo2 = __shfl_xor(lo, d, 64), hi2 = __shfl_xor(hi, d, 64);
        df |= __shfl_xor(df, d, 64);
        l = l2 > l ? l2 : l;
        lo = lo2 < lo ? lo2 : lo;
        hi = hi2 > hi ? hi2 : hi;
      }
      const uint64_t g = g0 + t / PPR + i * RSTEP;
      if (t % PPR == 0 && g < totalRows) {
        T* s = ws.stats + 4 * g;
        s[0] = l;
        s[1] = lo;
        s[2] = hi;
        s[3] = df ? T(1) : T(0);
      }
    }
  }
}

// Per array: the rows' sums of a added in order -- one lane, out of LDS, where the workgroup has put them with
// coalesced loads (k_mean_finalize's shape) -- and divided by T(n): the mean, which the variance pass reads from
// device memory.  The figures that have no order are reduced over the rows by all threads.
template <typename T>
__global__ void __launch_bounds__(kQualThreads)
k_quality_mean(uint64_t n, uint64_t nrow, QualWs<T> ws)
{
  __shared__ T stage[kQualStage];
  __shared__ T red[3][kQualThreads / 64];
  __shared__ int redNe;
  const uint64_t v = blockIdx.x;
  const T* rs = ws.asum + v * nrow;
  const T* st = ws.stats + v * nrow * 4;
  const uint32_t t = threadIdx.x;
  if (t == 0)
    redNe = 0;
  T total = 0;
  for (uint64_t base = 0; base < nrow; base += kQualStage) {
    const uint32_t cnt = (uint32_t)(nrow - base < (uint64_t)kQualStage ? nrow - base : (uint64_t)kQualStage);
    const uint32_t cntPad = (cnt + kQualGroup - 1) / kQualGroup * kQualGroup;   // (+0 past the end changes no sum: k_quality_rows)
    __syncthreads();
    for (uint32_t k = t; k < cntPad; k += kQualThreads)
      stage[k] = k < cnt ? rs[base + k] : T(0);
    __syncthreads();
    if (t == 0)
      for (uint32_t k = 0; k < cntPad; k += kQualGroup) {   // a group's reads fly together; the adds wait for each other
        T x[kQualGroup];
#pragma unroll
        for (int j = 0; j < kQualGroup; j++)
          x[j] = stage[k + j];
#pragma unroll
        for (int j = 0; j < kQualGroup; j++)
          total += x[j];
      }
  }
  T l = 0, lo = INFINITY, hi = -INFINITY;
  int df = 0;
  for (uint64_t r = t; r < nrow; r += kQualThreads) {
    const T l2 = st[4 * r], lo2 = st[4 * r + 1], hi2 = st[4 * r + 2];
    l = l2 > l ? l2 : l;
    lo = lo2 < lo ? lo2 : lo;
    hi = hi2 > hi ? hi2 : hi;
    df |= st[4 * r + 3] != T(0);
  }
  for (int d = 32; d > 0; d >>= 1) {
    const T l2 = __shfl_xor(l, d, 64), lo2 = __shfl_xor(lo, d, 64), hi2 = __shfl_xor(hi, d, 64);
    df |= __shfl_xor(df, d, 64);
    l = l2 > l ? l2 : l;
    lo = lo2 < lo ? lo2 : lo;
    hi = hi2 > hi ? hi2 : hi;
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = l;
    red[1][t >> 6] = lo;
    red[2][t >> 6] = hi;
    if (df)
      atomicOr(&redNe, 1);
  }
  __syncthreads();
  if (t != 0)
    return;
  for (int w = 1; w < kQualThreads / 64; w++) {
    l = red[0][w] > l ? red[0][w] : l;
    lo = red[1][w] < lo ? red[1][w] : lo;
    hi = red[2][w] > hi ? red[2][w] : hi;
  }
  T* h = ws.hdr + v * 8;
  h[0] = total / (T)n;
  h[1] = l;
  h[2] = lo;
  h[3] = hi;
  h[4] = redNe ? T(1) : T(0);
  h[5] = h[6] = h[7] = T(0);
}

namespace {

inline size_t qual_round(size_t b) { return (b + 255) / 256 * 256; }

// the workspace's arrays in values of T: hdr, sq and var first (what the host reads back), then asum and stats
struct QualLayout {
  size_t rows, total, hdr, sq, var, asum, stats, back, all;   // offsets and sizes in bytes
  bool ok;
};

QualLayout qual_layout(size_t nvol, size_t n, size_t esz)
{
  QualLayout L{};
  if (nvol == 0 || n == 0)
    return L;
  const size_t lim = ~size_t(0) / 64;
  if (n > lim / esz / nvol)                                // nvol * n * esz (and what follows) fits
    return L;
  L.rows = n / kQualMvBlock + 1;
  if (L.rows > lim / esz / nvol)
    return L;
  L.total = nvol * L.rows;
  if ((L.total + kQualRows - 1) / kQualRows > 0x7fffffffull || nvol > 0x7fffffffull)
    return L;
  L.hdr = 0;
  L.sq = L.hdr + qual_round(nvol * 8 * esz);
  L.var = L.sq + qual_round(L.total * 2 * esz);
  L.back = L.var + qual_round(L.total * esz);
  L.asum = L.back;
  L.stats = L.asum + qual_round(L.total * esz);
  L.all = L.stats + qual_round(L.total * 4 * esz);
  L.ok = true;
  return L;
}

// `vw`: a and b are one array each, read through these views (null: nvol dense arrays back to back)
template <typename T>
int quality_run_t(const T* a, const T* b, size_t nvol, size_t n, char* base, const QualLayout& L, double* out,
                  hipStream_t st, const QualViews* vw = nullptr)
{
  QualWs<T> ws;
  ws.hdr = reinterpret_cast<T*>(base + L.hdr);
  ws.sq = reinterpret_cast<T*>(base + L.sq);
  ws.var = reinterpret_cast<T*>(base + L.var);
  ws.asum = reinterpret_cast<T*>(base + L.asum);
  ws.stats = reinterpret_cast<T*>(base + L.stats);
  const uint32_t blocks = (uint32_t)((L.total + kQualRows - 1) / kQualRows);
  // (LAUNCH_K with names of their own: the template arguments would end up in the profile's kernel names)
  prof_begin("k_quality_rows", st);
  if (vw)
    hipLaunchKernelGGL((k_quality_rows<T, false, true>), dim3(blocks), dim3(kQualThreads), 0, st, a, b, (uint64_t)n,
                       (uint64_t)L.rows, (uint64_t)L.total, ws, *vw);
  else
    hipLaunchKernelGGL((k_quality_rows<T, false>), dim3(blocks), dim3(kQualThreads), 0, st, a, b, (uint64_t)n,
                       (uint64_t)L.rows, (uint64_t)L.total, ws, QualNoViews{});
  prof_end(st);
  LAUNCH_K(k_quality_mean<T>, dim3((uint32_t)nvol), dim3(kQualThreads), 0, st, (uint64_t)n, (uint64_t)L.rows, ws);
  prof_begin("k_quality_rows_var", st);
  if (vw)
    hipLaunchKernelGGL((k_quality_rows<T, true, true>), dim3(blocks), dim3(kQualThreads), 0, st, a, a, (uint64_t)n,
                       (uint64_t)L.rows, (uint64_t)L.total, ws, *vw);
  else
    hipLaunchKernelGGL((k_quality_rows<T, true>), dim3(blocks), dim3(kQualThreads), 0, st, a, a, (uint64_t)n,
                       (uint64_t)L.rows, (uint64_t)L.total, ws, QualNoViews{});
  prof_end(st);
  HIP_CHECK(hipGetLastError());
  std::vector<char> host(L.back);
  HIP_CHECK(hipMemcpyAsync(host.data(), base, L.back, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));   // the call's one wait
  const T* hdr = reinterpret_cast<const T*>(host.data() + L.hdr);
  const T* sq = reinterpret_cast<const T*>(host.data() + L.sq);
  const T* var = reinterpret_cast<const T*>(host.data() + L.var);
  const QualityPlan plan = quality_plan(n);
  for (size_t v = 0; v < nvol; v++) {
    const T* h = hdr + v * 8;
    // a row's two sums of d * d are the array's blocks 2r and 2r + 1: the first sq_partials() of them are the whole
    // blocks and then the tail's (one more slot may follow the tail; it is 0 and is not read)
    const QualityPartials<T> p{sq + v * L.rows * 2, var + v * L.rows, h[0], h[1], h[2], h[3], h[4] != T(0)};
    const std::array<T, 8> f = quality_finish(plan, p);
    for (int k = 0; k < 8; k++)
      out[v * 8 + k] = (double)f[k];
  }
  return 0;
}

}  // namespace

size_t quality_workspace_bytes(size_t nvol, size_t n, int is_float)
{
  const QualLayout L = qual_layout(nvol, n, is_float ? sizeof(float) : sizeof(double));
  return L.ok ? L.all : 0;
}

int quality_run(const void* d_orig, const void* d_recon, int is_float, size_t nvol, size_t n, void* ws, double* out,
                void* hip_stream)
{
  const QualLayout L = qual_layout(nvol, n, is_float ? sizeof(float) : sizeof(double));
  if (!L.ok || !d_orig || !d_recon || !ws || !out)
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (is_float)
    return quality_run_t(static_cast<const float*>(d_orig), static_cast<const float*>(d_recon), nvol, n,
                         static_cast<char*>(ws), L, out, st);
  return quality_run_t(static_cast<const double*>(d_orig), static_cast<const double*>(d_recon), nvol, n,
                       static_cast<char*>(ws), L, out, st);
}

// the values of a view of these dims, for the workspace and the rows; 0: none, too many, or a dim ViewCursor cannot hold
static size_t qual_view_vals(size_t dimx, size_t dimy, size_t dimz)
{
  size_t n = 0;
  if (dimx == 0 || dimy == 0 || dimz == 0 || dimx >= kViewCursorMaxDim || dimy >= kViewCursorMaxDim)
    return 0;
  if (!view_mul(dimx, dimy, &n) || !view_mul(n, dimz, &n))
    return 0;
  return n;
}

size_t quality_view_workspace_bytes(size_t dimx, size_t dimy, size_t dimz, int is_float)
{
  return quality_workspace_bytes(1, qual_view_vals(dimx, dimy, dimz), is_float);
}

int quality_view_run(const void* d_orig, ViewPitch p_orig, const void* d_recon, ViewPitch p_recon, int is_float,
                     size_t dimx, size_t dimy, size_t dimz, void* ws, double* out, void* hip_stream)
{
  const size_t n = qual_view_vals(dimx, dimy, dimz);
  const QualLayout L = qual_layout(1, n, is_float ? sizeof(float) : sizeof(double));
  if (!L.ok || !d_orig || !d_recon || !ws || !out || !view_valid(dimx, dimy, dimz, p_orig) ||
      !view_valid(dimx, dimy, dimz, p_recon))
    return -1;
  const QualViews vw{view_walk(dimx, dimy, p_orig), view_walk(dimx, dimy, p_recon)};
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (is_float)
    return quality_run_t(static_cast<const float*>(d_orig), static_cast<const float*>(d_recon), 1, n,
                         static_cast<char*>(ws), L, out, st, &vw);
  return quality_run_t(static_cast<const double*>(d_orig), static_cast<const double*>(d_recon), 1, n,
                       static_cast<char*>(ws), L, out, st, &vw);
}

}  // namespace sperrhip
