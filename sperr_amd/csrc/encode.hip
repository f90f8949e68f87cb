// encode.hip -- the encode call of the HIP engine: batches of equally shaped chunks through the float stages and the
// integer coder, the PSNR search, the outlier stage of point-wise error mode, container assembly; and the encoder's
// front (engine_core.h).  Plans and what the decoder shares come from engine.hip through engine_parts.h.
//
// Host logic restated from the reference (file:line):
//   src/SPERR3D_OMP_C.cpp:23-30,61-141      chunk loop  -> batches of equally shaped chunks
//   src/SPERR3D_OMP_C.cpp:145-234           container header + concatenated chunk streams
//   src/SPECK_FLT.cpp:401-541               per-chunk pipeline order and the fixed-rate retry
#include <chrono>
#include <deque>

#include "budget.h"
#include "engine_parts.h"

namespace sperrhip {

namespace {

uint64_t max_payload_bits(const ShapePlan& P, uint64_t raw_budget)
{
  // every plane of a uint64 coded in full: a sample gives at most one bit per plane plus its birth
  // test and its sign, a set one test per plane
  const uint64_t unlimited = (uint64_t)P.N * 66ull + (uint64_t)P.ht.nsets * 64ull + 64ull;
  const uint64_t b = rounded_budget(raw_budget);
  return std::min(b, unlimited);
}

// ------------------------------------------------------------------------------------------
// kernels of the container layer
// ------------------------------------------------------------------------------------------

// chunk stream = conditioner header (17) [+ SPECK header (9) + payload]  (SPECK_FLT.cpp:111-124,
// Conditioner.cpp:28-63, SPECK_INT.cpp:284-308) written into the chunk's slot
__global__ void __launch_bounds__(kThreads)
k_write_slot(const CoderState* cst, const EncState* est, const uint64_t* stream,
             size_t streamStride, const uint32_t* globalId, uint8_t* slots, const uint64_t* slotOff,
             uint64_t* lens, uint32_t nvals, int wide_pass)
{
  const uint32_t c = blockIdx.y;
  const CoderState& cs = cst[c];
  if (cs.is_const ? wide_pass : ((int)cs.wide != wide_pass || (!wide_pass && cs.need_retry)))
    return;
  const uint32_t g = globalId[c];
  uint8_t* out = slots + slotOff[g];
  const uint64_t len = cs.stream_len;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    lens[g] = len;
    if (cs.is_const) {
      out[0] = 0x81;
      const uint64_t nval = nvals;
      memcpy(out + 1, &nval, 8);
      memcpy(out + 9, &cs.mean, 8);
    }
    else {
      out[0] = 0x80;
      memcpy(out + 1, &cs.mean, 8);
      memcpy(out + 9, &cs.q, 8);
      out[17] = (uint8_t)cs.nbp;
      memcpy(out + 18, &cs.total_bits, 8);
    }
  }
  if (cs.is_const)
    return;
  (void)est;
  const uint64_t payload = len - 26;
  const uint64_t* w = stream + c * streamStride;
  copy_bytes_wide(out + 26, reinterpret_cast<const uint8_t*>(w), payload,
                  (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}

// container header (SPERR3D_OMP_C.cpp:163-234) + chunk offsets
// (lens2: bytes of the outlier stream that follows each chunk's SPECK stream, PWE mode)
__global__ void k_container_header(uint8_t* dst, const uint64_t* lens, const uint64_t* lens2,
                                   uint64_t* offs, uint32_t nchunks, uint32_t vx, uint32_t vy,
                                   uint32_t vz, uint32_t cx, uint32_t cy, uint32_t cz,
                                   int is_float, uint64_t* total)
{
  if (blockIdx.x || threadIdx.x)
    return;
  const bool multi = nchunks > 1;
  dst[0] = 0;  // SPERR_VERSION_MAJOR (CMakeLists.txt:5)
  dst[1] = (uint8_t)(0x40 | (is_float ? 0x20 : 0) | (multi ? 0x10 : 0));
  size_t pos = 2;
  const uint32_t v3[3] = {vx, vy, vz};
  memcpy(dst + pos, v3, 12);
  pos += 12;
  if (multi) {
    const uint16_t c3[3] = {(uint16_t)cx, (uint16_t)cy, (uint16_t)cz};
    memcpy(dst + pos, c3, 6);
    pos += 6;
  }
  uint64_t off = pos + 4ull * nchunks;
  for (uint32_t i = 0; i < nchunks; i++) {
    const uint64_t both = lens[i] + lens2[i];
    const uint32_t l = (uint32_t)both;
    memcpy(dst + pos, &l, 4);
    pos += 4;
    offs[i] = off;
    off += both;
  }
  *total = off;
}

// The containers of a batch of nvol volumes of one shape (sperrhip_compress_batch_dev), back to back: container v
// holds chunks [v cpv, (v + 1) cpv), and every container has the same header of H = 14 | 20 + 4 cpv bytes, so chunk g
// of container v starts at (v + 1) H + the bytes (SPECK + outlier) of the chunks before g, and container v at its
// first chunk's offset minus H.  One workgroup: an exclusive scan of the batch's chunk lengths in tiles of
// kBatchThreads (wave64 shuffles, then the waves' sums), then every header and chunk-length table.  Writes past
// dst_cap are dropped (the host refuses the batch then).  bases[0..nvol]: each container's start, then the total
constexpr uint32_t kBatchThreads = 1024;
__global__ void __launch_bounds__(kBatchThreads)
k_batch_container(uint8_t* dst, uint64_t dst_cap, const uint64_t* lens, const uint64_t* lens2, uint64_t* offs,
                  uint32_t nchunks, uint32_t cpv, uint32_t vx, uint32_t vy, uint32_t vz, uint32_t cx, uint32_t cy,
                  uint32_t cz, int is_float, uint64_t* bases)
{
  __shared__ uint64_t waveSum[kBatchThreads / 64];
  __shared__ uint64_t carry;
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const bool multi = cpv > 1;
  const uint32_t pos = multi ? 20u : 14u;
  const uint64_t H = pos + 4ull * cpv;
  const uint32_t nvol = nchunks / cpv;
  if (t == 0)
    carry = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < nchunks; t0 += kBatchThreads) {
    const uint32_t g = t0 + t;
    const uint64_t both = g < nchunks ? lens[g] + lens2[g] : 0;
    uint64_t x = both;   // inclusive scan of the wavefront
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d)
        x += y;
    }
    if (lane == 63)
      waveSum[w] = x;
    __syncthreads();
    uint64_t before = carry;
    for (uint32_t i = 0; i < w; i++)
      before += waveSum[i];
    if (g < nchunks) {
      const uint32_t v = g / cpv;
      const uint64_t at = (uint64_t)(v + 1) * H + before + x - both;
      offs[g] = at;
      if (g == v * cpv)
        bases[v] = at - H;
    }
    __syncthreads();   // (everyone has read carry and waveSum)
    if (t == kBatchThreads - 1)
      carry = before + x;
    __syncthreads();
  }
  if (t == 0)
    bases[nvol] = (uint64_t)nvol * H + carry;
  __syncthreads();   // (bases[] of this workgroup's writes are read below)
  for (uint32_t g = t; g < nchunks; g += kBatchThreads) {
    const uint32_t v = g / cpv;
    const uint64_t at = bases[v] + pos + 4ull * (g - v * cpv);
    const uint32_t l = (uint32_t)(lens[g] + lens2[g]);
    if (at + 4 <= dst_cap)
      memcpy(dst + at, &l, 4);
  }
  for (uint32_t v = t; v < nvol; v += kBatchThreads) {   // k_container_header's bytes
    uint8_t* h = dst + bases[v];
    if (bases[v] + pos > dst_cap)
      continue;
    h[0] = 0;
    h[1] = (uint8_t)(0x40 | (is_float ? 0x20 : 0) | (multi ? 0x10 : 0));
    const uint32_t v3[3] = {vx, vy, vz};
    memcpy(h + 2, v3, 12);
    if (multi) {
      const uint16_t c3[3] = {(uint16_t)cx, (uint16_t)cy, (uint16_t)cz};
      memcpy(h + 14, c3, 6);
    }
  }
}

// The streams of a batch of n slices of one shape (sperrhip_compress_2d_batch_dev), back to back: a slice is one
// chunk, there is no chunk-length table, and the optional 10-byte header {version, flags, u32 dimx, u32 dimy}
// (k_slice_header's bytes) is per stream.  Stream s starts at bases[s] = H s + the bytes (SPECK + outlier) of the
// slices before s, its chunk at offs[s] = bases[s] + H, H = 10 with headers and 0 without; bases[n] is the total.
// One workgroup whatever n is: an exclusive scan of lens + lens2 in tiles of kBatchThreads -- wave64 shuffles, the 16
// waves' sums through LDS (scanned by the first wavefront, read back as one broadcast word per wavefront: no bank
// conflict), a carry between tiles.  Writes past dst_cap are dropped (the host refuses the batch then).
__global__ void __launch_bounds__(kBatchThreads)
k_slice_batch_layout(uint8_t* dst, uint64_t dst_cap, const uint64_t* lens, const uint64_t* lens2, uint64_t* offs,
                     uint32_t n, uint32_t vx, uint32_t vy, int is_float, int with_header, uint64_t* bases)
{
  constexpr uint32_t kWaves = kBatchThreads / 64;
  __shared__ uint64_t waveBefore[kWaves + 1];   // (exclusive sums of the tile's waves, then the tile's sum)
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t H = with_header ? 10u : 0u;
  uint64_t carry = 0;   // (every thread keeps its own copy: the same value in all of them)
  for (uint32_t t0 = 0; t0 < n; t0 += kBatchThreads) {
    const uint32_t s = t0 + t;
    const uint64_t both = s < n ? lens[s] + lens2[s] : 0;
    uint64_t x = both;   // inclusive scan of the wavefront
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d)
        x += y;
    }
    __syncthreads();   // (the previous tile's waveBefore has been read)
    if (lane == 63)
      waveBefore[w + 1] = x;
    __syncthreads();
    if (w == 0) {   // the waves' sums: an inclusive scan in the first wavefront
      uint64_t ws = lane < kWaves ? waveBefore[lane + 1] : 0;
      for (int d = 1; d < (int)kWaves; d <<= 1) {
        const uint64_t y = __shfl_up(ws, d, 64);
        if (lane >= (uint32_t)d)
          ws += y;
      }
      if (lane < kWaves)
        waveBefore[lane + 1] = ws;
      if (lane == 0)
        waveBefore[0] = 0;
    }
    __syncthreads();
    if (s < n) {
      const uint64_t at = carry + waveBefore[w] + x - both + H * s;
      bases[s] = at;
      offs[s] = at + H;
      if (with_header && at + 10 <= dst_cap) {
        uint8_t* h = dst + at;
        h[0] = 0;
        h[1] = (uint8_t)(is_float ? 0x20 : 0);
        const uint32_t d2[2] = {vx, vy};
        memcpy(h + 2, d2, 8);
      }
    }
    carry += waveBefore[kWaves];
  }
  if (t == 0)
    bases[n] = carry + H * n;
}

__global__ void __launch_bounds__(kThreads)
k_copy_slots(uint8_t* dst, uint64_t dst_cap, const uint8_t* slots, const uint64_t* slotOff,
             const uint64_t* lens, const uint64_t* offs, uint32_t nchunks)
{
  for (uint32_t g = blockIdx.y; g < nchunks; g += gridDim.y) {   // (grid.y is limited to 65535)
    const uint64_t len = lens[g];
    if (offs[g] + len > dst_cap)
      continue;
    const uint8_t* in = slots + slotOff[g];
    uint8_t* out = dst + offs[g];
    copy_bytes_wide(out, in, len, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
  }
}

// outlier streams of one batch (local index b): they follow the chunk's SPECK stream
__global__ void __launch_bounds__(kThreads)
k_copy_slots2(uint8_t* dst, uint64_t dst_cap, const uint8_t* slots2, const uint64_t* slotOff2,
              const uint32_t* gids, const uint64_t* lens, const uint64_t* lens2,
              const uint64_t* offs)
{
  const uint32_t b = blockIdx.y, g = gids[b];
  const uint64_t len = lens2[g], at = offs[g] + lens[g];
  if (len == 0 || at + len > dst_cap)
    return;
  const uint8_t* in = slots2 + slotOff2[b];
  uint8_t* out = dst + at;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = in[i];
}

// ------------------------------------------------------------------------------------------
// compression
// ------------------------------------------------------------------------------------------
struct ChunkRef {
  uint32_t gid;
  uint32_t org[3];
};

// ---- the size mode (budget.h) ----
// a volume's survey on the device, by chunk number: the deal's table
struct SizeSurveyDev {
  double* q;
  int32_t* nbp;
  uint64_t* end;       // [nchunks][kBudgetPlanes]
  uint8_t* is_const;
};
// arena bytes a chunk of a size-mode batch takes beside the coder's arrays (EncodeCall::code)
constexpr size_t kSizeBytesPerChunk = (3 * kMaxPlanes + kMaxPlanes) * 8 + 1024;

// a batch's plane table (rows of kMaxPlanes, by local index) into the volume's (rows of kBudgetPlanes, by chunk number).
// The 32-bit pass has at most 32 planes: a fixed-rate step is maxabs / (2^32 - 1)
__global__ void k_survey_gather(const CoderState* cst, const uint64_t* end, const int32_t* nbp, const uint32_t* gids,
                                uint32_t nb, SizeSurveyDev sv)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb)
    return;
  const uint32_t g = gids[c];
  const CoderState& cs = cst[c];
  sv.is_const[g] = cs.is_const ? 1 : 0;
  sv.q[g] = cs.is_const ? 0.0 : cs.q;
  sv.nbp[g] = cs.is_const ? 0 : nbp[c];
  for (int p = 0; p < kBudgetPlanes; p++)
    sv.end[(size_t)g * kBudgetPlanes + p] = cs.is_const ? 0ull : end[(size_t)c * kMaxPlanes + p];
}

// the deal on the device: one workgroup is budget.h's team
struct BudgetBlock {
  uint32_t rank, size;
  uint64_t* sm;   // [kThreads / 64 + 1]
  template <class Op>
  __device__ uint64_t reduce(uint64_t v, Op op)
  {
    for (int d = 32; d > 0; d >>= 1) {
      const uint64_t o = __shfl_xor(v, d, 64);
      v = op(v, o);
    }
    __syncthreads();   // (the words of the reduction before this one have been read)
    if ((threadIdx.x & 63) == 0)
      sm[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = sm[0];
    for (uint32_t w = 1; w < blockDim.x / 64; w++)
      r = op(r, sm[w]);
    return r;
  }
  __device__ uint64_t sum(uint64_t v) { return reduce(v, [](uint64_t a, uint64_t b) { return a + b; }); }
  __device__ uint64_t min(uint64_t v) { return reduce(v, [](uint64_t a, uint64_t b) { return a < b ? a : b; }); }
  __device__ uint64_t max(uint64_t v) { return reduce(v, [](uint64_t a, uint64_t b) { return a > b ? a : b; }); }
};

// out[0]: 0 ok, 1 refused; out[1..2]: the bit patterns of T* and T'
__global__ void __launch_bounds__(kThreads) k_budget_deal(SizeSurveyDev sv, uint32_t nchunks, uint64_t W, uint64_t* budgets, uint64_t* out)
{
  __shared__ uint64_t sm[kThreads / 64 + 1];
  BudgetBlock team{threadIdx.x, blockDim.x, sm};
  const BudgetTable t{nchunks, sv.q, sv.nbp, sv.end, sv.is_const};
  const int rc = budget_deal(t, W, budgets, out + 1, team);
  if (threadIdx.x == 0)
    out[0] = rc ? 1ull : 0ull;
}

struct EncBatchBufs {
  EncBuffers eb;
  ChunkGeom* geom;
  uint32_t* gids;
  double* vals;
  size_t valsStride;
  double* strideMean;
  size_t strideMeanStride;
  uint32_t* coef32;
  int8_t* msb;
  size_t bytesPerChunk;
  bool aliased;        // the coder's node arrays, birth records and second list lie over `vals` (carve_enc_coder)
  bool fusedHead;      // the 32-bit pass takes k_head_fused: M, E and leafDesc have memory of their own
  size_t coderBytes;   // ... and take this many bytes for the batch
};

// the arrays of the integer coder that nothing reads or writes before the quantiser is done: each from
// `first` when it fits there, else from `second` (may be null)
// ownLeaf: M, E and leafDesc from `second` whatever room `first` has (the fused head writes them while other workgroups
// still read the chunk buffer)
bool carve_enc_coder(Arena& first, Arena* second, const ShapePlan& P, uint32_t B, EncBuffers& e, bool ownLeaf = false)
{
  const size_t nn = P.dtree.nnodes;
#define TAKE(dst, T, count)                            \
  dst = first.take<T>((size_t)(count));                \
  if (!dst && second)                                  \
    dst = second->take<T>((size_t)(count));            \
  if (!dst)                                            \
    return false;
  e.nodeStride = nn;
  e.bornStride = P.ht.nsets + 8;
  // (the large ones first: what does not fit any more is small)
  TAKE(e.opos, uint64_t, nn * B);
  TAKE(e.chain, uint64_t, nn * B);
  TAKE(e.bornPacked, uint64_t, e.bornStride * B);
  TAKE(e.bornPosLev, uint64_t, e.bornStride * B);
  TAKE(e.lis[1], uint64_t, P.lisEntries * B);
  if (!(ownLeaf && second))
    TAKE(e.E, uint32_t, nn * B);
  TAKE(e.bucket, uint32_t, nn * B);
  TAKE(e.koff, uint32_t, nn * B);
  if (ownLeaf && second) {
    e.E = second->take<uint32_t>(nn * B);
    e.leafDesc = second->take<uint16_t>(nn * B);
    e.M = second->take<int8_t>(nn * B);
    return e.E && e.leafDesc && e.M;
  }
  TAKE(e.leafDesc, uint16_t, nn * B);
  TAKE(e.M, int8_t, nn * B);
#undef TAKE
  return true;
}

// Does the 32-bit pass of this shape take the fused head (SPERR_HIP_ENC_FUSED_HEAD=0: the three kernels, for A/B runs and
// tests)?  Decides the memory layout (carve_enc) and the launches (EncodeCall::quantise) alike.
bool enc_fused_head(const ShapePlan& P)
{
  static const bool on = !(getenv("SPERR_HIP_ENC_FUSED_HEAD") && atoi(getenv("SPERR_HIP_ENC_FUSED_HEAD")) == 0);
  return on && P.d_fusedRoots != nullptr;
}

// carve the arrays of one batch out of the arena; returns false when it does not fit
// alias: the coder's arrays over the chunk buffer (not in point-wise error mode, whose outlier stage writes the chunk buffer
// while the coder runs: compress_impl)
bool carve_enc(Arena& A, const ShapePlan& P, uint32_t B, uint64_t raw_budget, EncBatchBufs& o, bool alias = true)
{
  const size_t N = P.N, Npad = round_up(N, 256);
  const size_t nn = P.dtree.nnodes;
  const uint64_t payloadBits = max_payload_bits(P, raw_budget);
  const size_t streamWords = (size_t)((payloadBits + 63) / 64) + 4;
  const uint64_t maskBits = std::min<uint64_t>(P.maxPhaseBits, payloadBits + 64);
  const size_t maskWords = (size_t)((maskBits + 63) / 64) + 2;
  EncBuffers& e = o.eb;
  memset(&e, 0, sizeof(e));
  e.tree = P.dtree;
  e.nchunks = B;
#define TAKE(dst, T, count)                                                            \
  dst = A.take<T>((size_t)(count));                                                    \
  if (!dst)                                                                            \
    return false;                                                                      \
  if (arena_debug())                                                                   \
    fprintf(stderr, "[sperr_hip] arena %-18s %10.2f MB\n", #dst, (double)((size_t)(count) * sizeof(T)) / 1048576.0);
  TAKE(e.cst, CoderState, B);
  TAKE(e.st, EncState, B);
  TAKE(o.geom, ChunkGeom, B);
  TAKE(o.gids, uint32_t, B);
  o.valsStride = Npad;
  TAKE(o.vals, double, Npad * B);
  o.strideMeanStride = round_up(std::max<size_t>(P.nstrides, P.N / 4096 + 2), 32);   // (also the PSNR-mode mse partials)
  TAKE(o.strideMean, double, o.strideMeanStride * B);
  e.coefStride = Npad;
  TAKE(o.coef32, uint32_t, Npad * B);
  e.coef = o.coef32;
  e.signStride = Npad / 64;
  uint64_t* sign;
  TAKE(sign, uint64_t, e.signStride * B);
  e.sign = sign;
  e.pixStride = Npad;
  TAKE(o.msb, int8_t, Npad * B);
  e.msb = o.msb;
  TAKE(e.bplane, int8_t, Npad * B);
  // The coder's node arrays, birth records and second list are written after the quantiser has read
  // the chunk buffer for the last time: they lie over it (round 3; 127 of the 421 MB a 256^3 chunk
  // took).  A batch that needs the 64-bit retry transforms its chunks again and gives these arrays
  // memory of their own (Engine::wideScratch, compress_impl).
  {
    Arena over;
    over.base = reinterpret_cast<char*>(o.vals);
    over.cap = alias ? Npad * B * sizeof(double) : 0;
    const size_t before = A.used;
    o.fusedHead = enc_fused_head(P);
    if (!carve_enc_coder(over, &A, P, B, e, o.fusedHead))
      return false;
    o.aliased = over.used != 0;
    o.coderBytes = over.used + (A.used - before);
    if (arena_debug())
      fprintf(stderr, "[sperr_hip] arena %-18s %10.2f MB, %.2f MB of them over o.vals\n", "coder arrays",
              (double)o.coderBytes / 1048576.0, (double)over.used / 1048576.0);
  }
  e.lisStride = P.lisEntries;
  TAKE(e.lis[0], uint64_t, P.lisEntries * B);
  e.levelOff = P.d_levelOff;
  e.nListTiles = P.nListTiles;
  e.tileLevel = P.d_tileLevel;
  e.tileStart = P.d_tileStart;
  e.levelFirstTile = P.d_levelFirstTile;
  e.levelNumTiles = P.d_levelNumTiles;
  e.tileStride = round_up(P.nListTiles, 32);
  TAKE(e.tileBits, uint64_t, e.tileStride * B);
  TAKE(e.tileSurv, uint32_t, e.tileStride * B);
  TAKE(e.tileBitsOff, uint64_t, e.tileStride * B);
  TAKE(e.tileSurvOff, uint32_t, e.tileStride * B);
  e.iRoots = P.d_iRoots;
  e.iLevels = P.ht.iLevels;
  e.levelSlot = P.d_levelSlot;
  e.slotLevel = P.d_slotLevel;
  e.nSlots = P.nSlots;
  e.maskWords = (uint32_t)maskWords;
  e.maskStride = (size_t)P.nSlots * maskWords;
  TAKE(e.mask, uint64_t, std::max<size_t>(e.maskStride, 1) * B);
  e.prefWords = (uint32_t)((maskWords + 3) / 4);
  e.prefStride = (size_t)P.nSlots * e.prefWords;
  TAKE(e.maskPrefix, uint32_t, std::max<size_t>(e.prefStride, 1) * B);
  e.nPixTiles = P.nPixTiles;
  e.pixCntStride = (size_t)kMaxPlanes * 2 * P.nPixTiles;
  TAKE(e.pixCnt, uint32_t, e.pixCntStride * B);
  TAKE(e.pixOff, uint32_t, e.pixCntStride * B);
  e.streamStride = streamWords;
  TAKE(e.stream, uint64_t, streamWords * B);
#undef TAKE
  return true;
}

// bytes carve_enc takes for a batch of B chunks.  Probed with the batch's own B: which coder arrays
// find room over the chunk buffer (carve_enc_coder, first fit) depends on the 256-byte rounding of
// B arrays, so B times the one-chunk figure can fall short for small chunks.
size_t enc_bytes_for(const ShapePlan& P, uint32_t B, uint64_t raw_budget, bool alias = true)
{
  Arena probe;
  probe.base = reinterpret_cast<char*>(uintptr_t(4096));  // never dereferenced: size probe only
  probe.cap = ~size_t(0) / 2;
  EncBatchBufs tmp;
  carve_enc(probe, P, std::max<uint32_t>(B, 1), raw_budget, tmp, alias);
  return probe.used;
}
size_t enc_bytes_per_chunk(const ShapePlan& P, uint64_t raw_budget, bool alias = true)
{
  return enc_bytes_for(P, 1, raw_budget, alias);
}

// (fusedHead: k_head_fused writes the birth plane of EVERY sample of every chunk that takes part in the pass, and whatever
//  reads bplane -- k_pyramid, k_census, k_emit_pixels -- leaves the other chunks alone (EncState::active): no fill)
int reset_enc_pass(hipStream_t st, const EncBatchBufs& bb, uint32_t B, bool fusedHead = false)
{
  const EncBuffers& e = bb.eb;
  if (!fusedHead)
    HIP_CHECK(hipMemsetAsync(e.bplane, 0xff, e.pixStride * B, st));
  HIP_CHECK(hipMemsetAsync(e.M, 0xff, e.nodeStride * B, st));
  HIP_CHECK(hipMemsetAsync(e.mask, 0, std::max<size_t>(e.maskStride, 1) * B * sizeof(uint64_t), st));
  HIP_CHECK(hipMemsetAsync(e.stream, 0, e.streamStride * B * sizeof(uint64_t), st));
  return 0;
}

// conditioner + forward transform of one batch: volume -> bb.vals (mean, constness, largest magnitude
// in CoderState).  Run once per batch -- and once more before a 64-bit retry when the coder's arrays
// lay over the chunk buffer (carve_enc): the same launches on the same input give the same bits.
template <typename T>
int float_stages(hipStream_t ss, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb, const uint32_t cd[3],
                 const T* d_src, VolDesc vd, bool orgAligned, bool wantRange, bool level2 = true)
{
  EncBuffers& e = bb.eb;
  // the first lifting pass covers the whole chunk: it reads the volume itself (gather, widen,
  // subtract the mean); chunks too small to be transformed take the plain gather kernel
  const bool fuse = !P.fwd.empty();
  const int io = std::is_same<T, float>::value ? 1 : 2;
  if (launch_condition<T>(ss, d_src, vd, bb.geom, nb, cd, P.nstrides, bb.strideMean, bb.strideMeanStride,
                          bb.vals, bb.valsStride, e.cst, !fuse, wantRange, orgAligned))
    return -1;
  // The forward walk: the head, the second level as one launch where the schedule has it, then pass by pass.
  // The passes after which samples have their final value also collect the largest magnitude
  // (src/SPECK_FLT.cpp:282-301): no pass over the coefficients of its own
  const LiftSchedule& sch = P.schedule;
  auto collect_max = [&](size_t k, LiftFuse& lf) {
    if (sch.fusable && pass_fuse(P, k, lf.inner) > 0)
      lf.mode = 1;
  };
  const bool l2 = level2 && sch.level2;
  if (sch.head == LiftSchedule::kHeadXYZ) {   // the three full-size passes in one kernel, straight from the volume
    LiftFuse lf;
    collect_max(2, lf);
    // The second level fused (plan_level2): the finest-level kernel writes the next level's box compact into the 32-bit
    // coefficient array, which only the quantiser writes, after the transform (one sample in eight, 8 of the array's 32 bytes for them); the
    // level-2 launch reads it and writes the corner of the chunk buffer.  (Not in front of the 64-bit retry: the
    // chunks that keep their 32-bit coefficients keep them there.)
    double* box = l2 ? reinterpret_cast<double*>(bb.coef32) : nullptr;
    const size_t boxStride = e.coefStride / 2;
    if (l2 && (e.coefStride % 2 != 0 || (size_t)lf.inner[0] * lf.inner[1] * lf.inner[2] > boxStride))
      return -1;
    if (launch_lift_xyz(ss, true, bb.vals, bb.valsStride, nb, cd, e.cst, io, const_cast<T*>(d_src), vd,
                        bb.geom, &lf, nullptr, box, boxStride))
      return -1;
    if (l2) {
      LiftFuse l5;
      collect_max(5, l5);
      if (launch_lift2_fwd(ss, box, boxStride, bb.vals, bb.valsStride, nb, cd, P.fwd[3].region, e.cst, &l5))
        return -1;
    }
  }
  else if (sch.head == LiftSchedule::kHeadXY) {   // the full-size x and y passes in one kernel, straight from the volume
    if (launch_lift_xy(ss, true, bb.vals, bb.valsStride, nb, cd, e.cst, io, const_cast<T*>(d_src), vd,
                       bb.geom))
      return -1;
  }
  for (size_t k = LiftSchedule::fused_passes(sch.head, l2); k < P.fwd.size(); k++) {
    const LiftPass& ps = P.fwd[k];
    LiftFuse lf;
    collect_max(k, lf);
    if (launch_lift(ss, true, bb.vals, bb.valsStride, nb, cd, ps.axis, ps.region, e.cst, k == 0 ? io : 0,
                    const_cast<T*>(d_src), vd, bb.geom, &lf))
      return -1;
  }
  return 0;
}

// before the 64-bit retry of a batch whose coder arrays lay over the chunk buffer: those arrays move
// to memory of their own and the buffer gets its DWT coefficients back
// the coder's arrays off the chunk buffer, into scratch memory of the engine (64-bit magnitudes are
// about to live in the buffer)
int unalias_coder(hipStream_t ss, Engine& E, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb)
{
  HIP_CHECK(hipStreamSynchronize(ss));   // (the scratch buffer may grow: nothing of this stream may still use it)
  if (E.wideScratch.ensure(bb.coderBytes + 4096))
    return -1;
  Arena W;
  W.base = static_cast<char*>(E.wideScratch.p);
  W.cap = E.wideScratch.n;
  if (!carve_enc_coder(W, nullptr, P, nb, bb.eb))
    return -1;
  bb.aliased = false;
  return 0;
}

template <typename T>
int wide_retry_prepare(hipStream_t ss, Engine& E, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb,
                       const uint32_t cd[3], const T* d_src, VolDesc vd, bool orgAligned, bool wantRange)
{
  if (unalias_coder(ss, E, P, bb, nb))
    return -1;
  g_dbg_counter[0]++;
  return float_stages<T>(ss, P, bb, nb, cd, d_src, vd, orgAligned, wantRange, false);
}

// PSNR mode (src/SPECK_FLT.cpp:268-279,431-435): per chunk q = 2 sqrt(3 t), t = range^2 10^(-psnr/10),
// divided by 2^(1/4) until the estimated quantisation error is at most t.  The libm calls run on
// the host (the same libm the reference uses), the error estimate on the device with the
// reference's summation order; chunks whose largest coefficient needs more than 32 bits are
// flagged for the 64-bit pass (SPECK_FLT.cpp:324-337).
// (`hc`, `got`: the caller's, alive until the call's last wait)
int psnr_q_search(hipStream_t st, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb, double psnr,
                  std::vector<CoderState>& hc, std::vector<CoderState>& got)
{
  EncBuffers& e = bb.eb;
  hc.assign(nb, CoderState{});
  HIP_CHECK(hipMemcpyAsync(hc.data(), e.cst, nb * sizeof(CoderState), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  std::vector<double> tmse(nb, 0.0);
  bool any = false;
  for (uint32_t i = 0; i < nb; i++) {
    CoderState& c = hc[i];
    c.mse_active = 0;
    if (c.is_const)
      continue;
    const double vmax = order_key_value(c.vmaxKey), vmin = -order_key_value(c.vnegmaxKey);
    const double range = (vmax - c.mean) - (vmin - c.mean);   // of the conditioned samples
    tmse[i] = (range * range) * std::pow(10.0, -psnr / 10.0);
    c.q = 2.0 * std::sqrt(tmse[i] * 3.0);
    if (!(c.q > 0.0))
      return -1;   // (the reference asserts q > 0)
    c.mse_active = 1;
    any = true;
  }
  const double step = std::exp2(0.25);
  while (any) {
    HIP_CHECK(hipMemcpyAsync(e.cst, hc.data(), nb * sizeof(CoderState), hipMemcpyHostToDevice, st));
    if (launch_mse(st, bb.vals, bb.valsStride, nb, P.N, bb.strideMean, bb.strideMeanStride, e.cst))
      return -1;
    got.assign(nb, CoderState{});
    HIP_CHECK(hipMemcpyAsync(got.data(), e.cst, nb * sizeof(CoderState), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    any = false;
    for (uint32_t i = 0; i < nb; i++) {
      if (!hc[i].mse_active)
        continue;
      if (got[i].mse > tmse[i]) {
        hc[i].q /= step;   // four adjustments halve q
        any = true;
      }
      else
        hc[i].mse_active = 0;
    }
  }
  for (uint32_t i = 0; i < nb; i++) {
    CoderState& c = hc[i];
    c.mse_active = 0;
    c.wide = 0;
    c.need_retry = 0;
    if (c.is_const)
      continue;
    const double m = c.maxabs / c.q;
    if (!(m < 0x1p63))
      return -1;   // llrint would raise FE_INVALID (SPECK_FLT.cpp:323-327): exactly from 2^63 on, and for a NaN
    c.need_retry = std::llrint(m) > (long long)0xffffffffll ? 1u : 0u;
  }
  HIP_CHECK(hipMemcpyAsync(e.cst, hc.data(), nb * sizeof(CoderState), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

// diagnostics: SPERR_HIP_TIMING=1 prints host-side wall-clock marks of the PWE stages
struct HostMarks {
  bool on = getenv("SPERR_HIP_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char* what, hipStream_t st)
  {
    if (!on)
      return;
    (void)hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[sperr_hip] %-28s %8.2f ms\n", what,
            std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

// PWE mode (src/SPECK_FLT.cpp:280-281): q = 1.5 tol for every chunk; chunks whose largest
// coefficient needs more than 32 bits are flagged for the 64-bit pass (SPECK_FLT.cpp:324-337)
// (`hc`: the caller's, alive until the call's last wait -- the upload at the end is not waited for: round 6, one of the
//  four host round trips per batch that went, see pwe_stage_finish)
int pwe_q_setup(hipStream_t st, EncBatchBufs& bb, uint32_t nb, double tol, std::vector<CoderState>& hc, bool* anyWide = nullptr)
{
  EncBuffers& e = bb.eb;
  hc.assign(nb, CoderState{});
  HIP_CHECK(hipMemcpyAsync(hc.data(), e.cst, nb * sizeof(CoderState), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (uint32_t i = 0; i < nb; i++) {
    CoderState& c = hc[i];
    c.wide = 0;
    c.need_retry = 0;
    if (c.is_const)
      continue;
    c.q = 1.5 * tol;
    const double m = c.maxabs / c.q;
    if (!(m < 0x1p63))
      return -1;   // llrint would raise FE_INVALID (SPECK_FLT.cpp:323-327): exactly from 2^63 on, and for a NaN
    c.need_retry = std::llrint(m) > (long long)0xffffffffll ? 1u : 0u;
    if (anyWide && c.need_retry)
      *anyWide = true;   // (this mode chooses the width before coding: nothing else sets the flag, k_enc_finalize)
  }
  HIP_CHECK(hipMemcpyAsync(e.cst, hc.data(), nb * sizeof(CoderState), hipMemcpyHostToDevice, st));
  return 0;
}

// outlier streams of one batch, kept on the device until the container is assembled
struct PweKeep {
  void* mem = nullptr;
  uint32_t nb = 0;
  uint32_t* gids = nullptr;
  uint64_t* slotOff = nullptr;
  uint8_t* slots = nullptr;
  std::vector<uint64_t> off2;   // host copy of slotOff: uploaded without a wait, lives until the container is out
};
// (the memory belongs to the engine, Engine::pweBufs, and is reused by later calls: a hipFree per
//  batch waits for every stream of the device, which stalls the other workers of the chunk farm)
using PweKeepList = std::vector<PweKeep>;

// PWE mode, after the integer coder (src/SPECK_FLT.cpp:461-486): rebuild the values the decoder
// will see (inverse quantiser + inverse transform, in the chunk buffer), compare them with the
// conditioned input, and code every error above the tolerance with the 1D coder.
// The stage in two halves (round 5): `begin` -- the reconstruction, the first outlier pass and its read-back, enqueued,
// not waited for -- needs nothing of the 3D coder, only the quantiser's coefficients, so it can run on a stream of its
// own BESIDE the coder (compress_impl); `finish` waits for it and does the rest.
struct PweStage {
  OutlierBufs ob;
  std::vector<OutlierChunk> hoc;
  std::vector<ChunkGeom> bricks;   // (enqueue_brick_inverse; lives until the stage's next wait for the stream)
  HostMarks hm;
};
// The encoder's own coefficients, for its reconstruction of what the decoder will see: complete, so no masks and no
// decoder state.  wide: the 64-bit ones, which live in the fp64 buffer and are converted in place
static DequantSrc enc_dequant_src(const EncBatchBufs& bb, bool wide)
{
  DequantSrc s;
  s.coef = wide ? static_cast<const void*>(bb.vals) : bb.coef32;
  s.coefStride = wide ? bb.valsStride : bb.eb.coefStride;
  s.sign = bb.eb.sign;
  s.signStride = bb.eb.signStride;
  return s;
}

// `begin` itself in two parts: what the decoder will reconstruct (pwe_recon_begin), and the first pass over it and the
// input (pwe_scan_begin) -- which with pwe_stage_finish is the whole outlier coder, and is where
// sperrhip_outlier_encode_dev enters with a reconstruction of the caller's.
int pwe_recon_begin(hipStream_t st, Engine& E, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb, VolDesc vd,
                    const uint32_t cd[3], bool anyWide, PweStage& S)
{
  EncBuffers& e = bb.eb;
  HostMarks& hm = S.hm;
  hm.mark("(3D coder done)", st);
  // What the decoder will reconstruct, in the conditioned domain (src/SPECK_FLT.cpp:461-486): by the brick inverse
  // where the plan allows it and no chunk has 64-bit coefficients, else by an inverse quantiser pass and the per-axis
  // passes over the whole chunk
  if (!anyWide && brick_inverse_fits(P, nb, bb.valsStride)) {
    if (enqueue_brick_inverse(st, P, E.pweBox, S.bricks, nb, bb.vals, bb.valsStride, e.cst, bb.geom, enc_dequant_src(bb, false)))
      return -1;
  }
  else {
    if (launch_inv_quantize(st, false, enc_dequant_src(bb, false), nb, P.N, bb.vals, bb.valsStride, e.cst) ||
        launch_inv_quantize(st, true, enc_dequant_src(bb, true), nb, P.N, bb.vals, bb.valsStride, e.cst))
      return -1;
    for (size_t k = P.fwd.size(); k-- > 0;) {
      const LiftPass& ps = P.fwd[k];
      if (launch_lift(st, false, bb.vals, bb.valsStride, nb, cd, ps.axis, ps.region, e.cst, 0, nullptr,
                      vd, bb.geom))
        return -1;
    }
  }
  hm.mark("inverse path", st);
  return 0;
}

template <typename T>
int pwe_scan_begin(hipStream_t st, Engine& E, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb,
                   const T* d_src, VolDesc vd, const uint32_t cd[3], double tol, PweStage& S)
{
  EncBuffers& e = bb.eb;
  OutlierBufs& ob = S.ob;
  std::vector<OutlierChunk>& hoc = S.hoc;
  memset(&ob, 0, sizeof(ob));
  ob.nchunks = nb;
  ob.N = P.N;
  ob.nw = (P.N + 63) / 64;
  ob.wordStride = round_up((size_t)ob.nw + 2, 32);
  {
    const size_t bytes = round_up(nb * sizeof(OutlierChunk), 256) + (size_t)nb * ob.wordStride * (4 * 8 + 2 * 4) + 4096;
    if (E.outlFixed.ensure(bytes))
      return -1;
    Arena A;
    A.base = static_cast<char*>(E.outlFixed.p);
    A.cap = E.outlFixed.n;
    ob.oc = A.take<OutlierChunk>(nb);
    ob.lip = A.take<uint64_t>(nb * ob.wordStride);
    ob.signMask = A.take<uint64_t>(nb * ob.wordStride);
    ob.maskGE = A.take<uint64_t>(nb * ob.wordStride);
    ob.maskEQ = A.take<uint64_t>(nb * ob.wordStride);
    ob.outPre = A.take<uint32_t>(nb * ob.wordStride);
    ob.cpos = A.take<uint32_t>(nb * ob.wordStride);
    if (!ob.oc || !ob.lip || !ob.signMask || !ob.maskGE || !ob.maskEQ || !ob.outPre || !ob.cpos)
      return -1;
  }
  HIP_CHECK(hipMemsetAsync(ob.oc, 0, nb * sizeof(OutlierChunk), st));
  ob.kStride = 1;
  if (launch_outlier_scan<T>(st, 0, d_src, vd, bb.geom, cd, bb.vals, bb.valsStride, e.cst, tol, ob))
    return -1;
  hoc.assign(nb, OutlierChunk{});
  {   // (into pinned memory: the call returns at once and the 3D coder can be enqueued meanwhile)
    const size_t bytes = nb * sizeof(OutlierChunk);
    if (E.pweHostBytes < bytes) {
      if (E.pweHost)
        (void)hipHostFree(E.pweHost);
      E.pweHost = nullptr;
      E.pweHostBytes = 0;
      HIP_CHECK(hipHostMalloc(&E.pweHost, round_up(bytes, 4096), hipHostMallocDefault));
      E.pweHostBytes = round_up(bytes, 4096);
    }
    HIP_CHECK(hipMemcpyAsync(E.pweHost, ob.oc, bytes, hipMemcpyDeviceToHost, st));
  }
  return 0;
}

template <typename T>
int pwe_stage_begin(hipStream_t st, Engine& E, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb,
                    const T* d_src, VolDesc vd, const uint32_t cd[3], double tol, bool anyWide, PweStage& S)
{
  if (E.pweLastStream) {   // (a second batch of one call: the first one's stage is not waited for at its end any more)
    HIP_CHECK(hipStreamSynchronize(E.pweLastStream));
    E.pweLastStream = nullptr;
  }
  return pwe_recon_begin(st, E, P, bb, nb, vd, cd, anyWide, S) || pwe_scan_begin<T>(st, E, P, bb, nb, d_src, vd, cd, tol, S);
}

template <typename T>
int pwe_stage_finish(hipStream_t st, Engine& E, const ShapePlan& P, EncBatchBufs& bb, uint32_t nb,
                     const T* d_src, VolDesc vd, const uint32_t cd[3], double tol,
                     uint64_t* d_lens2, PweKeepList& keep, PweStage& S)
{
  EncBuffers& e = bb.eb;
  HostMarks& hm = S.hm;
  OutlierBufs& ob = S.ob;
  std::vector<OutlierChunk>& hoc = S.hoc;
  HIP_CHECK(hipStreamSynchronize(st));
  memcpy(hoc.data(), E.pweHost, nb * sizeof(OutlierChunk));
  hm.mark("outlier pass 0", st);
  bool any = false;
  for (auto& o : hoc) {
    if (!o.flagged)
      continue;
    any = true;
    // the integer type the reference keeps the magnitudes in comes from the largest ERROR, not
    // from the largest magnitude (Outlier_Coder.cpp:82-100); magnitudes wrap to that width
    double maxerr;
    memcpy(&maxerr, &o.maxErrKey, 8);
    if (!(maxerr < 0x1p63))
      return -1;   // llrint would raise FE_INVALID (Outlier_Coder.cpp:88-91): the reference refuses the chunk
    const long long mi = std::llrint(maxerr);
    o.widthMask = mi <= 0xffll ? 0xffull : mi <= 0xffffll ? 0xffffull : mi <= 0xffffffffll ? 0xffffffffull : ~0ull;
  }
  if (!any)
    return 0;   // (d_lens2 stays zero for these chunks)
  // Round 6: everything from here to the 1D coder's result is enqueued behind ONE wait.  Until then the host came
  // back after the counting pass (for the number of outliers: the arrays' size), after the compaction (for the
  // largest magnitude: the stream's size) and after the stream's copy -- a device call went back to the host a dozen
  // times per batch, and the farm's pipeline (two workers a device) ran at the rate of those round trips.  The first
  // pass has counted the samples beyond the tolerance (`flagged`: at least the outliers that survive the wrap to
  // the integer width, Outlier_Coder.cpp:82-100) and found the largest error: both bounds are known now.
  uint32_t kmax = 0;
  int maxPlanes = 1;
  for (auto& o : hoc) {
    if (!o.flagged)
      continue;
    kmax = std::max(kmax, o.flagged);
    double maxerr;
    memcpy(&maxerr, &o.maxErrKey, 8);
    // (a magnitude is llrint(error / tol) cut to the width: below both)
    const double mq = std::min(maxerr / tol + 2.0, 1.8e19);
    const unsigned long long bound = std::min<unsigned long long>(o.widthMask, (unsigned long long)mq);
    maxPlanes = std::max(maxPlanes, 64 - __builtin_clzll(bound | 1ull));
  }
  HIP_CHECK(hipMemcpyAsync(ob.oc, hoc.data(), nb * sizeof(OutlierChunk), hipMemcpyHostToDevice, st));
  if (launch_outlier_scan<T>(st, 1, d_src, vd, bb.geom, cd, bb.vals, bb.valsStride, e.cst, tol, ob))
    return -1;
  ob.kStride = P.N;   // (only the overflow check of the prefix kernel reads it here)
  if (launch_outlier_prefix(st, ob))
    return -1;
  hm.mark("outlier pass 1 + prefix", st);
  ob.kStride = round_up(std::max<size_t>(kmax, 1), 64);
  speck1d_level_offsets(ob, P.N, 2ull * kmax + 2);
  const size_t varFixed = (size_t)nb * (ob.kStride * (4 + 8 + 1 + 1 + 4 + 1) + ob.runStride * 8) + 8192;
  if (E.outlVar.n < varFixed)
    HIP_CHECK(hipStreamSynchronize(st));   // (the buffer grows: nothing enqueued may still point into the old one)
  if (E.outlVar.ensure(varFixed))
    return -1;
  {
    Arena A;
    A.base = static_cast<char*>(E.outlVar.p);
    A.cap = E.outlVar.n;
    ob.mag = A.take<uint64_t>(nb * ob.kStride);
    ob.runs = A.take<uint64_t>(nb * ob.runStride);
    ob.pos = A.take<uint32_t>(nb * ob.kStride);
    ob.posGE = A.take<uint32_t>(nb * ob.kStride);
    ob.sgn = A.take<uint8_t>(nb * ob.kStride);
    ob.msb = A.take<uint8_t>(nb * ob.kStride);
    ob.sgnGE = A.take<uint8_t>(nb * ob.kStride);
    if (!ob.mag || !ob.runs || !ob.pos || !ob.posGE || !ob.sgn || !ob.msb || !ob.sgnGE)
      return -1;
  }
  if (launch_outlier_scan<T>(st, 2, d_src, vd, bb.geom, cd, bb.vals, bb.valsStride, e.cst, tol, ob))
    return -1;
  hm.mark("alloc + outlier pass 2", st);
  // bits of one chunk's stream: every outlier has at most nlists sets above it, each with a
  // sibling, and every one of those (and the value itself) gives at most one bit per plane, plus
  // the value's sign; and never more than every node of the whole tree doing so
  const uint64_t perOutlier = (uint64_t)(2 * ob.nlists + 2) * maxPlanes + 1;
  const uint64_t sparse = (uint64_t)kmax * perOutlier + 2ull * maxPlanes;
  const uint64_t dense = (uint64_t)P.N * (4ull * maxPlanes + 1);
  const uint64_t maxBits = std::min(sparse, dense) + 64;
  ob.streamStride = round_up((size_t)(maxBits / 64) + 4, 32);
  if (E.outlStream.n < (size_t)nb * ob.streamStride * 8 + 256)
    HIP_CHECK(hipStreamSynchronize(st));
  if (E.outlStream.ensure((size_t)nb * ob.streamStride * 8 + 256))
    return -1;
  ob.stream = static_cast<uint64_t*>(E.outlStream.p);
  HIP_CHECK(hipMemsetAsync(ob.stream, 0, (size_t)nb * ob.streamStride * 8, st));
  HIP_CHECK(hipMemsetAsync(ob.lip, 0, (size_t)nb * ob.wordStride * 8, st));
  HIP_CHECK(hipMemsetAsync(ob.maskGE, 0, (size_t)nb * ob.wordStride * 8, st));
  if (launch_speck1d_encode(st, ob))
    return -1;
  HIP_CHECK(hipMemcpyAsync(hoc.data(), ob.oc, nb * sizeof(OutlierChunk), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  hm.mark("1D coder", st);
  std::vector<uint64_t> off2(nb + 1, 0);
  for (uint32_t i = 0; i < nb; i++) {
    if (hoc[i].flagged && hoc[i].count > ob.kStride) {   // (cannot be: count <= flagged)
      fprintf(stderr, "[sperr_hip] outlier coder: more outliers than the first pass counted (chunk %u)\n", i);
      return -1;
    }
    if (hoc[i].error) {
      fprintf(stderr, "[sperr_hip] outlier coder failed (chunk %u, code %u)\n", i, hoc[i].error);
      return -1;
    }
    const uint64_t len = hoc[i].flagged ? 9 + (hoc[i].total_bits + 7) / 8 : 0;
    off2[i + 1] = off2[i] + round_up(len, 16);
  }
  PweKeep K;
  K.nb = nb;
  const size_t headBytes = round_up((size_t)nb * 8, 256) + round_up((size_t)nb * 4, 256);
  if (keep.size() >= E.pweBufs.size())
    E.pweBufs.push_back(std::make_unique<DevBuf>());
  DevBuf& kb = *E.pweBufs[keep.size()];
  if (kb.ensure(headBytes + off2[nb] + 256))
    return -1;
  K.mem = kb.p;
  keep.push_back(K);
  PweKeep& kk = keep.back();
  kk.slotOff = reinterpret_cast<uint64_t*>(kk.mem);
  kk.gids = reinterpret_cast<uint32_t*>(static_cast<char*>(kk.mem) + round_up((size_t)nb * 8, 256));
  kk.slots = reinterpret_cast<uint8_t*>(static_cast<char*>(kk.mem) + headBytes);
  kk.off2 = std::move(off2);   // (alive until the container is assembled: compress_impl waits for its stream at the end)
  HIP_CHECK(hipMemcpyAsync(kk.slotOff, kk.off2.data(), nb * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(kk.gids, bb.gids, nb * 4, hipMemcpyDeviceToDevice, st));
  if (launch_outlier_stream_out(st, ob, kk.gids, kk.slots, kk.slotOff, d_lens2))
    return -1;
  E.pweLastStream = st;
  hm.mark("stream out", st);
  return 0;
}

// ---- 2D slices (sperr_comp_2d / sperr_decomp_2d, src/SPERR_C_API.cpp:7-134): a slice is a
// one-chunk batch of dims (x, y, 1) -- its transform plan already is dwt2d -- coded by the 3D coder's
// kernels on the 2D coder's forest (the plan of key (x, y, 0))
// optional 10-byte header {version, flags, u32 dimx, u32 dimy} (SPERR_C_API.cpp:45-83), then the
// chunk stream and its outlier stream
__global__ void k_slice_header(uint8_t* dst, const uint64_t* lens, const uint64_t* lens2,
                               uint64_t* offs, uint32_t vx, uint32_t vy, int is_float,
                               int with_header, uint64_t* total)
{
  if (blockIdx.x || threadIdx.x)
    return;
  uint64_t pos = 0;
  if (with_header) {
    dst[0] = 0;
    dst[1] = (uint8_t)(is_float ? 0x20 : 0);
    const uint32_t d2[2] = {vx, vy};
    memcpy(dst + 2, d2, 8);
    pos = 10;
  }
  offs[0] = pos;
  *total = pos + lens[0] + lens2[0];
}

// The outlier stage of point-wise error mode on a reconstruction of the caller's: the batch is the nchunks chunks of
// a volume (x, y, z * nchunks) cut along z, its chunk buffer holds d_recon, and from there on it is what compress runs
// -- pwe_scan_begin, pwe_stage_finish -- with every chunk's mean 0 and none constant.
template <typename T>
int outlier_encode_impl(Engine& E, hipStream_t st, const ShapePlan& P, const T* d_orig, const double* d_recon,
                               uint32_t nb, double tol, uint8_t* d_dst, size_t dst_cap, size_t* lens)
{
  const size_t N = P.N;
  if (E.arena.ensure(enc_bytes_for(P, nb, 0, false) + 4096) || E.misc.ensure(round_up((size_t)nb * 8, 256) + 256))
    return -1;
  Arena A;
  A.base = static_cast<char*>(E.arena.p);
  A.cap = E.arena.n;
  EncBatchBufs bb;
  if (!carve_enc(A, P, nb, 0, bb, false))
    return -1;
  const uint32_t cd[3] = {P.dims[0], P.dims[1], P.dims[2]};
  const VolDesc vd{{cd[0], cd[1], (uint64_t)cd[2] * nb}};
  std::vector<CoderState> hcs(nb);
  std::vector<ChunkGeom> hg(nb);
  std::vector<uint32_t> hid(nb);
  memset(hcs.data(), 0, nb * sizeof(CoderState));
  for (uint32_t i = 0; i < nb; i++) {
    hg[i].org[0] = hg[i].org[1] = 0;
    hg[i].org[2] = i * cd[2];
    hid[i] = i;
  }
  uint64_t* d_lens2 = static_cast<uint64_t*>(E.misc.p);
  std::vector<uint64_t> hl(nb, 0);
  PweStage S;
  PweKeepList keep;
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(bb.eb.cst, hcs.data(), nb * sizeof(CoderState), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(bb.geom, hg.data(), nb * sizeof(ChunkGeom), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(bb.gids, hid.data(), nb * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpy2DAsync(bb.vals, bb.valsStride * 8, d_recon, N * 8, N * 8, nb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemsetAsync(d_lens2, 0, (size_t)nb * 8, st));
    if (pwe_scan_begin<T>(st, E, P, bb, nb, d_orig, vd, cd, tol, S) ||
        pwe_stage_finish<T>(st, E, P, bb, nb, d_orig, vd, cd, tol, d_lens2, keep, S))
      return -1;
    HIP_CHECK(hipMemcpyAsync(hl.data(), d_lens2, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    size_t pos = 0;
    for (uint32_t i = 0; i < nb; i++) {
      lens[i] = (size_t)hl[i];
      if (!hl[i])
        continue;
      if (keep.empty() || hl[i] > dst_cap - std::min(pos, dst_cap))
        return -1;
      HIP_CHECK(hipMemcpyAsync(d_dst + pos, keep.back().slots + keep.back().off2[i], hl[i], hipMemcpyDeviceToDevice, st));
      pos += hl[i];
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
  };
  const int rtn = run();
  if (rtn)
    drain_after_error(E, st);   // (queued copies read and write the vectors above)
  E.pweLastStream = nullptr;
  E.prof.collect();
  return rtn;
}

// One compression call (compress_impl), stage by stage.  mode 1: fixed rate, `quality` bits per value; mode 2: fixed
// PSNR and mode 3: fixed point-wise error, every bit plane is coded
template <typename T>
struct EncodeCall {
  using GKey = std::array<size_t, 4>;   // chunk extents + part
  // a batch of one shape group's chunks; kept until the call's end: its host arrays are what queued copies
  // read and write, and a group side by side has its plane loop and 64-bit retry enqueued after every group
  struct Batch {
    ShapePlan* P;
    EncBatchBufs bb;
    uint32_t nb, wblocks = 0;
    uint64_t raw_budget;
    hipStream_t ss;
    std::vector<CoderState> hc;
    std::vector<ChunkGeom> hg;
    std::vector<uint32_t> hid;
    std::vector<uint64_t> hbud;   // (size mode: the batch's budgets, the source of a queued copy)
    uint64_t* d_bud = nullptr;    //   ... and where they land: EncPlanHost::d_budgets of every head of the batch
    double* d_ladder = nullptr;   // (PSNR of the whole volume: the ladder's partials, [chunk][rung][stride])
    bool orgAligned = true;
    EncPlanHost ph;
  };
  Engine& E;
  const T* d_src;
  const Dims vol;
  const int mode;
  const double quality;
  uint8_t* d_dst;
  size_t dst_cap;
  hipStream_t st;
  const Coded what;
  // a batch (sperrhip_compress_batch_dev): nvol volumes of dims `vol` back to back in d_src, read as one volume of
  // (x, y, nvol z) -- the stacked view -- whose chunks are each volume's, and coded into nvol containers.  With
  // `slice` (sperrhip_compress_2d_batch_dev): nvol slices, chunk s of dims (x, y, 1) at (0, 0, s), one shape group on
  // the 2D coder's forest, coded into nvol streams (k_slice_batch_layout)
  const size_t nvol = 1;
  // d_src is the first element of a strided view of the volume (sperrhip_compress_view_dev; valid, one volume):
  // every reader of the volume takes rows and slices from `vd`, `vol` stays what the chunks, the header and the
  // size checks see
  const ViewPitch* srcView = nullptr;
  const bool slice = what != Coded::Container;
  const bool rate = mode == 1;
  const double bpp = rate ? quality : 0.0;
  const VolDesc vd = srcView ? view_desc(*srcView, vol[2]) : VolDesc{{vol[0], vol[1], vol[2] * nvol}};
  Dims cdim;
  uint32_t nchunks = 0;
  std::map<GKey, std::vector<ChunkRef>> groups;
  std::vector<ShapePlan*> groupPlan;
  std::vector<uint64_t> slotOff;       // slots for the finished chunk streams
  uint64_t *d_slotOff = nullptr, *d_lens = nullptr, *d_offs = nullptr, *d_lens2 = nullptr, *d_total = nullptr;
  bool sideBySide = false;
  std::vector<size_t> groupOff;        // (side by side: each group's piece of the arena)
  std::deque<Batch> batches;
  std::vector<Batch*> late;            // (side by side: each group's batch)
  PweKeepList pweKeep;
  std::deque<std::vector<CoderState>> hcKeep;   // chunk states of PSNR / PWE setups (one host thread: no lock)
  std::deque<PweStage> pweStages;
  uint64_t total = 0;
  std::vector<uint64_t> bases;   // (a batch: where each container starts, then the total)
  bool ok = false;
  // The size mode (compress_size_impl; budget.h), two calls over the same volume in fixed-rate mode.  sizePass 1, the
  // SURVEY: float stages and the coder's head per batch, then the plane table instead of the plane loop -- every chunk's
  // q, plane count, table row and constness land in `sv`, by chunk number; no stream, no slot, no container.  sizePass 2:
  // the fixed-rate flow with a budget per chunk, hBudgets[chunk number] in bits, which each batch uploads for
  // k_enc_state_init; a group's workspace is sized by its largest budget.  Both run one shape group after the other
  // and a group in one part: the survey's read-back and the deal stand between the passes anyway
  int sizePass = 0;
  SizeSurveyDev sv{};
  const uint64_t* hBudgets = nullptr;
  // PSNR of the whole volume (compress_psnr_impl; psnr_vol.h): mode 2's flow, but every chunk's q comes from the ladder
  // of ONE target, made once per call -- k_mse_ladder and k_mse_ladder_pick decide q, width and refusal on the device,
  // quantise() waits for nothing, and the refusal rides the read-back behind code().  No per-chunk range is taken
  const PsnrLadder* volLadder = nullptr;
  bool chunk_range() const { return mode == 2 && !volLadder; }
  // the ladder's partials of one chunk, [rung][stride], beside the coder's arrays
  static size_t ladder_stride(const ShapePlan& P) { return round_up((size_t)psnr_vol_strides(P.N), 32); }
  size_t ladder_bytes(const ShapePlan& P) const { return volLadder ? round_up(kPsnrRungs * ladder_stride(P) * sizeof(double), 256) : 0; }
  // a shape group's raw budget in bits (src/SPECK_FLT.cpp:491), which sizes its streams, masks and slots
  uint64_t raw_of(const ShapePlan& P, const std::vector<ChunkRef>& refs) const
  {
    if (sizePass == 1)
      return 8;   // (nothing is written)
    if (sizePass == 2) {
      uint64_t m = 8;
      for (auto& r : refs)
        m = std::max(m, hBudgets[r.gid]);
      return m;
    }
    return (uint64_t)(bpp * (double)P.N);
  }
  ~EncodeCall() { if (!ok) drain_after_error(E, st); }
  // (a slice is coded on the 2D coder's forest, the plan with z extent 0)
  ShapePlan* plan_of(const GKey& d) { return E.plan(d[0], d[1], slice ? 0 : d[2]); }
  int run(const Dims& chunkPref)
  {
    for (int a = 0; a < 3; a++)  // SPERR3D_OMP_C.cpp:23-30
      cdim[a] = std::min(std::max<size_t>(1, chunkPref[a]), vol[a]);
    auto chunks = chunk_volume(vol, cdim);
    for (int a = 0; a < 3; a++)
      if (vol[a] > 0xffffffffull || cdim[a] > 0xffff)
        return -1;
    if (nvol > 1) {   // (each volume's own chunks, z origins shifted: the tall volume's remainders would differ)
      const size_t per = chunks.size();
      if (nvol > 0xffffffffull / vol[2] || per > 0xffffffffull / nvol)
        return -1;
      chunks.reserve(per * nvol);
      for (size_t v = 1; v < nvol; v++)
        for (size_t i = 0; i < per; i++) {
          auto c = chunks[i];
          c[4] += v * vol[2];
          chunks.push_back(c);
        }
    }
    nchunks = (uint32_t)chunks.size();
    group_chunks(chunks);
    if (size_slots() || plan_side_by_side())
      return -1;
    late.assign(groups.size(), nullptr);
    uint32_t gi = 0;
    for (auto& g : groups)
      if (encode_group(gi++, g.second))
        return -1;
    if (late_planes() || late_retry())
      return -1;
    if (sizePass == 1) {   // (the caller reads the survey back)
      ok = true;
      return 0;
    }
    if (sideBySide)
      for (uint32_t q = 0; q < kSubStreams; q++) {
        HIP_CHECK(hipEventRecord(E.evJoin[q], E.sub[q]));
        HIP_CHECK(hipStreamWaitEvent(st, E.evJoin[q], 0));
      }
    return container();
  }
  // Group chunks by shape, keeping chunk order inside a group.  In fixed-rate mode a group of 64 and more chunks
  // is cut into parts (four: round 5, 16 chunks each of the bench volume -- three before; five and more fall under
  // the sixteen chunks the capped grids want) that run side by side like the shape groups of a ragged volume do:
  // the per-plane chains of small launches of one part overlap the bandwidth-bound kernels of the other
  // (SPERR_HIP_ENC_PARTS=1: one part)
  void group_chunks(const std::vector<std::array<size_t, 6>>& chunks)
  {
    std::map<Dims, uint32_t> count, seen;
    for (uint32_t i = 0; i < nchunks; i++)
      count[Dims{chunks[i][1], chunks[i][3], chunks[i][5]}]++;
    static const uint32_t partsEnv = getenv("SPERR_HIP_ENC_PARTS") ? (uint32_t)std::max(1, atoi(getenv("SPERR_HIP_ENC_PARTS"))) : 4u;
    for (uint32_t i = 0; i < nchunks; i++) {
      const auto& c = chunks[i];
      const Dims d{c[1], c[3], c[5]};
      const uint32_t n = count[d], k = seen[d]++;
      static const uint32_t partsMin = tune_getenv("SPERR_HIP_ENC_PARTS_MIN") ? (uint32_t)std::max(2, atoi(tune_getenv("SPERR_HIP_ENC_PARTS_MIN"))) : 64u;
      const uint32_t parts = (mode == 1 && !slice && !sizePass && n >= partsMin && n <= 512) ? std::min<uint32_t>(std::min<uint32_t>(partsEnv, n / 4), kSubStreams) : 1u;
      groups[GKey{c[1], c[3], c[5], (size_t)((uint64_t)k * parts / n)}].push_back(
          {i, {(uint32_t)c[0], (uint32_t)c[2], (uint32_t)c[4]}});
    }
  }
  // a slot per chunk for its finished stream, and the call's offsets and lengths
  int size_slots()
  {
    slotOff.assign(nchunks + 1, 0);
    std::vector<uint64_t> slotLen(nchunks, 0);
    for (auto& g : groups) {
      ShapePlan* P = plan_of(g.first);
      if (!P)
        return -1;
      groupPlan.push_back(P);
      const uint64_t raw = raw_of(*P, g.second);
      const uint64_t len = 26 + (max_payload_bits(*P, raw) + 7) / 8;
      for (auto& r : g.second)
        slotLen[r.gid] = round_up(len, 256);
    }
    for (uint32_t i = 0; i < nchunks; i++)
      slotOff[i + 1] = slotOff[i] + slotLen[i];
    if (E.slots.ensure(slotOff[nchunks] + 256))
      return -1;
    if (E.misc.ensure(round_up((size_t)nchunks * 8, 256) * 4 + round_up((nvol + 1) * 8, 256)))
      return -1;
    d_slotOff = reinterpret_cast<uint64_t*>(E.misc.p);
    d_lens = d_slotOff + round_up(nchunks, 32);
    d_offs = d_lens + round_up(nchunks, 32);
    d_lens2 = d_offs + round_up(nchunks, 32);   // outlier streams (PWE mode)
    d_total = d_lens2 + round_up(nchunks, 32);
    HIP_CHECK(hipMemsetAsync(d_lens2, 0, (size_t)nchunks * 8, st));
    HIP_CHECK(hipMemcpyAsync(d_slotOff, slotOff.data(), nchunks * 8, hipMemcpyHostToDevice, st));
    return 0;
  }
  // Shape groups side by side (fixed-rate mode, a volume the chunk size does not divide): every group gets a
  // piece of the arena and a sub-stream of its own, the check for the rare 64-bit retry (one read-back per group)
  // waits until all groups are enqueued
  int plan_side_by_side()
  {
    sideBySide = mode == 1 && !slice && !sizePass && groups.size() > 1;
    if (!sideBySide)
      return 0;
    size_t fr = 0, tot = 0, need = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t budgetBytes = arena_budget(E.arena.n, fr);
    for (auto& g : groups) {
      ShapePlan* P = plan_of(g.first);
      groupOff.push_back(need);
      need += round_up(enc_bytes_for(*P, (uint32_t)g.second.size(), (uint64_t)(bpp * (double)P->N)) + 4096, 4096);
      sideBySide = sideBySide && g.second.size() <= 256;
    }
    sideBySide = sideBySide && need <= budgetBytes;
    if (sideBySide) {
      if (E.arena.ensure(need))
        return -1;
      HIP_CHECK(hipEventRecord(E.evFork, st));
      for (uint32_t q = 0; q < kSubStreams; q++)
        HIP_CHECK(hipStreamWaitEvent(E.sub[q], E.evFork, 0));
    }
    return 0;
  }
  int encode_group(uint32_t gi, const std::vector<ChunkRef>& refs)
  {
    hipStream_t ss = sideBySide ? E.sub[gi % kSubStreams] : st;
    ShapePlan* P = groupPlan[gi];
    const uint64_t raw_budget = raw_of(*P, refs);  // SPECK_FLT.cpp:491
    // (point-wise error mode: the coder's arrays get memory of their own -- 127 MB more per 256^3 chunk --, so that the
    //  outlier stage's reconstruction can be written into the chunk buffer while the coder runs, see below)
    const bool encAlias = mode != 3;
    // (the size mode's per-chunk words beside the coder's arrays: the plane table's accumulators and rows, or a budget)
    const size_t per = enc_bytes_per_chunk(*P, raw_budget, encAlias) + (sizePass ? kSizeBytesPerChunk : 0) + ladder_bytes(*P);
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t budgetBytes = arena_budget(E.arena.n, fr);
    uint32_t B = (uint32_t)std::min<size_t>(refs.size(), std::max<size_t>(1, budgetBytes / per));
    B = std::min<uint32_t>(B, 256);
    if (sideBySide)
      B = (uint32_t)refs.size();
    else if (E.arena.ensure(std::max((size_t)B * per, enc_bytes_for(*P, B, raw_budget, encAlias) + (sizePass ? B * kSizeBytesPerChunk : 0) + B * ladder_bytes(*P)) + 4096))
      return -1;
    for (size_t b0 = 0; b0 < refs.size(); b0 += B) {
      Batch& b = batches.emplace_back(Batch{P, {}, (uint32_t)std::min<size_t>(B, refs.size() - b0), 0, raw_budget, ss});
      if (encode_batch(gi, refs, b0, b, encAlias))
        return -1;
    }
    return 0;
  }
  // one batch: conditioner, transform and quantiser; the coder, in point-wise error mode beside the outlier
  // stage; and the 64-bit retry where a chunk asks for it
  int encode_batch(uint32_t gi, const std::vector<ChunkRef>& refs, size_t b0, Batch& b, bool encAlias)
  {
    const uint32_t nb = b.nb;
    const uint32_t* cd = b.P->dims;
    // (a further batch of workspace lies over the earlier one's, whose work this stream is behind: under the poison
    //  switch the arena is filled again.  Groups side by side have a piece each, carved once)
    if (!sideBySide && batches.size() > 1 && E.poison_arena(b.ss))
      return -1;
    Arena A;
    A.base = static_cast<char*>(E.arena.p) + (sideBySide ? groupOff[gi] : 0);
    A.cap = E.arena.n - (sideBySide ? groupOff[gi] : 0);
    if (!carve_enc(A, *b.P, nb, b.raw_budget, b.bb, encAlias))
      return -1;
    if (b.bb.aliased)
      g_dbg_counter[1]++;
    b.hg.resize(nb);
    b.hid.resize(nb);
    for (uint32_t i = 0; i < nb; i++) {
      const ChunkRef& r = refs[b0 + i];
      b.hid[i] = r.gid;
      for (int a = 0; a < 3; a++)
        b.hg[i].org[a] = r.org[a];
      b.orgAligned = b.orgAligned && r.org[0] % (16 / sizeof(T)) == 0;   // (lets the conditioner stream rows with 16-byte loads)
    }
    if (sizePass == 2) {   // (in front of the quantiser: the fused head initialises the chunks' states)
      b.hbud.resize(nb);
      for (uint32_t i = 0; i < nb; i++)
        b.hbud[i] = hBudgets[b.hid[i]];
      b.d_bud = A.take<uint64_t>(nb);
      if (!b.d_bud)
        return -1;
      HIP_CHECK(hipMemcpyAsync(b.d_bud, b.hbud.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, b.ss));
    }
    if (volLadder) {
      b.d_ladder = A.take<double>(kPsnrRungs * ladder_stride(*b.P) * nb);
      if (!b.d_ladder)
        return -1;
    }
    bool pweWide = false;
    if (quantise(b, &pweWide))
      return -1;
    // Point-wise error mode: what the decoder will reconstruct, and which samples miss the tolerance, follows from
    // the quantiser's coefficients alone -- the first half of the outlier stage (reconstruction, first outlier
    // pass) runs on a stream of its own BESIDE the 3D coder (round 5; behind it, one stream, before: the 1D coder
    // alone is 3.2 of the 11.8 ms a batch of eight chunks took).  Not when the coder's arrays lie over the chunk
    // buffer the reconstruction is written to, and given up when a chunk turns out to need 64-bit coefficients.
    hipStream_t pweQ = E.outlQ[1];
    const bool pweEarly = mode == 3 && !b.bb.aliased && !pweWide;
    if (pweEarly) {
      HIP_CHECK(hipEventRecord(E.evPweFork, b.ss));
      HIP_CHECK(hipStreamWaitEvent(pweQ, E.evPweFork, 0));
      if (pwe_stage_begin<T>(pweQ, E, *b.P, b.bb, nb, d_src, vd, cd, quality, false, pweStages.emplace_back()))
        return -1;
    }
    if (code(gi, A, b))
      return -1;
    // (point-wise error mode: the outlier stage's second half -- its waits are for its own stream -- while the plane
    //  loop above runs)
    if (pweEarly) {
      if (pwe_stage_finish<T>(pweQ, E, *b.P, b.bb, nb, d_src, vd, cd, quality, d_lens2, pweKeep, pweStages.back()))
        return -1;
      // (the stage no longer ends in a wait of the host: what follows on the batch's stream -- the container's
      //  kernels read the outlier streams and their lengths -- waits for it on the device)
      HIP_CHECK(hipEventRecord(E.evPweJoin, pweQ));
      HIP_CHECK(hipStreamWaitEvent(b.ss, E.evPweJoin, 0));
    }
    if (sideBySide) {   // (a read-back into pageable memory would block the host until this group's stream has
      late[gi] = &b;    //  drained: the retry is looked at once every group is enqueued, late_retry)
      return 0;
    }
    if (sizePass == 1) {   // (the next batch carves the arena again)
      HIP_CHECK(hipStreamSynchronize(b.ss));
      return 0;
    }
    b.hc.resize(nb);
    HIP_CHECK(hipMemcpyAsync(b.hc.data(), b.bb.eb.cst, nb * sizeof(CoderState), hipMemcpyDeviceToHost, b.ss));
    HIP_CHECK(hipStreamSynchronize(b.ss));
    bool retry = false;
    for (auto& c : b.hc)
      retry |= (c.need_retry != 0);
    if (volLadder)   // (the pick's refusals: the chunk was coded with a stand-in q, nothing of it has left the workspace)
      for (uint32_t i = 0; i < nb; i++)
        if (!b.hc[i].is_const && b.hc[i].mse_active != 0) {
          fprintf(stderr, b.hc[i].mse_active == kPsnrRefusedNoRung
                              ? "[sperr_hip] chunk %u: no rung of the ladder brings its error estimate under the target\n"
                              : "[sperr_hip] chunk %u: its largest coefficient is 2^63 steps or more, or not a number\n",
                  b.hid[i]);
          return -1;
        }
    if (retry) {
      if (pweEarly) {   // (cannot be: this mode knows the width before it codes, pwe_q_setup)
        fprintf(stderr, "[sperr_hip] a chunk asked for 64-bit coefficients after its outlier stage had run\n");
        return -1;
      }
      if (retry_wide(b, b.ph))
        return -1;
    }
    if (mode == 3 && !pweEarly) {   // (a chunk that was coded again has 64-bit coefficients)
      PweStage& S = pweStages.emplace_back();
      if (pwe_stage_begin<T>(b.ss, E, *b.P, b.bb, nb, d_src, vd, cd, quality, retry, S) ||
          pwe_stage_finish<T>(b.ss, E, *b.P, b.bb, nb, d_src, vd, cd, quality, d_lens2, pweKeep, S))
        return -1;
    }
    return 0;
  }
  // ---- float stages: the first lifting pass covers the whole chunk: it reads the volume itself (gather, widen,
  // subtract the mean); chunks too small to be transformed take the plain gather kernel.  Then the quantiser ----
  int quantise(Batch& b, bool* pweWide)
  {
    EncBatchBufs& bb = b.bb;
    EncBuffers& e = bb.eb;
    const uint32_t nb = b.nb;
    HIP_CHECK(hipMemcpyAsync(bb.geom, b.hg.data(), nb * sizeof(ChunkGeom), hipMemcpyHostToDevice, b.ss));
    HIP_CHECK(hipMemcpyAsync(bb.gids, b.hid.data(), nb * 4, hipMemcpyHostToDevice, b.ss));
    HIP_CHECK(hipMemsetAsync(e.cst, 0, nb * sizeof(CoderState), b.ss));
    if (float_stages<T>(b.ss, *b.P, bb, nb, b.P->dims, d_src, vd, b.orgAligned, chunk_range()))
      return -1;
    if (launch_maxabs_q(b.ss, bb.vals, bb.valsStride, nb, b.P->N, e.cst, b.P->schedule.fusable))
      return -1;
    if (chunk_range() && psnr_q_search(b.ss, *b.P, bb, nb, quality, hcKeep.emplace_back(), hcKeep.emplace_back()))
      return -1;
    if (volLadder && launch_mse_ladder(b.ss, bb.vals, bb.valsStride, nb, b.P->N, b.d_ladder, ladder_stride(*b.P), e.cst, *volLadder))
      return -1;
    if (mode == 3 && pwe_q_setup(b.ss, bb, nb, quality, hcKeep.emplace_back(), pweWide))
      return -1;
    if (bb.fusedHead) {
      // quantiser, leaf level of the pyramid and census in one kernel: the fills first (M, E and leafDesc, which the
      // kernel writes, have memory of their own; what else lies over the chunk buffer is written after it)
      if (reset_enc_pass(b.ss, bb, nb, true))
        return -1;
      EncPlanHost ph{b.P->d_initLIS, b.P->d_initLen, b.P->d_depthBlocks, b.P->depthBlockOff, b.P->ht.nsets};
      ph.d_budgets = b.d_bud;
      g_dbg_counter[3]++;
      return launch_speck_encode_fused_head(b.ss, e, ph, b.raw_budget, bb.vals, bb.valsStride, b.P->d_fusedRoots);
    }
    if (launch_quantize(b.ss, false, bb.vals, bb.valsStride, nb, b.P->N, bb.coef32, e.coefStride,
                        const_cast<uint64_t*>(e.sign), e.signStride, bb.msb, e.pixStride, e.cst))
      return -1;
    // (only now: the coder's arrays may lie over the chunk buffer the quantiser has just read)
    return reset_enc_pass(b.ss, bb, nb);
  }
  // ---- integer coder, 32-bit coefficients ----
  int code(uint32_t gi, Arena& A, Batch& b)
  {
    const ShapePlan& P = *b.P;
    EncBuffers& e = b.bb.eb;
    EncPlanHost& ph = b.ph = EncPlanHost{P.d_initLIS, P.d_initLen, P.d_depthBlocks, P.depthBlockOff, P.ht.nsets};
    ph.fusedHead = b.bb.fusedHead;   // (quantise() has run k_head_fused)
    // (the census of the pixel passes on a stream of its own beside the pyramid's upper levels: the
    //  decoder's outlier streams and events are idle during a compression call)
    ph.side = E.sideQ[gi % kSubStreams];
    ph.evFork = E.evOutlFork[gi % kSubStreams];
    ph.evJoin = E.evOutl[gi % kSubStreams];
    // the planes that can hold work are asked of the device before the plane loop is enqueued (speck_enc.h;
    // the decoder's pinned words and events are idle during a compression call)
    ph.d_bound = A.take<uint32_t>(64);
    // (a pinned word pair and an event per GROUP: groups gi and gi + kSubStreams share a stream, and every head
    //  is enqueued before any plane loop reads its bounds back -- a ragged volume has up to 4 parts + 7 border
    //  shapes = 11 groups.  Past kSubStreams * kLiveSlots / 2 groups: all planes are launched)
    const uint32_t lane = gi % kSubStreams, turn = gi / kSubStreams;
    if (turn < (uint32_t)kLiveSlots / 2) {
      ph.h_bound = E.liveHost[lane] + 2 * turn;
      ph.evBound = E.liveEv[lane][turn];
    }
    if (!ph.d_bound)
      ph.h_bound = nullptr;
    if (sizePass == 1) {
      // the survey: the head alone (no bound: no plane loop follows), then the table, dealt out by chunk number
      ph.d_bound = nullptr;
      ph.h_bound = nullptr;
      ph.evBound = nullptr;
      uint64_t* d_acc = A.take<uint64_t>((size_t)b.nb * speck_plane_table_acc_words());
      uint64_t* d_end = A.take<uint64_t>((size_t)b.nb * kMaxPlanes);
      int32_t* d_nbp = A.take<int32_t>(b.nb);
      if (!d_acc || !d_end || !d_nbp)
        return -1;
      if (launch_speck_encode_head(b.ss, e, ph, 0, false, false) || launch_speck_plane_table(b.ss, e, ph, d_acc, d_end, d_nbp))
        return -1;
      LAUNCH_K(k_survey_gather, dim3((b.nb + 63) / 64), dim3(64), 0, b.ss, e.cst, d_end, d_nbp, b.bb.gids, b.nb, sv);
      HIP_CHECK(hipGetLastError());
      return 0;
    }
    ph.d_budgets = b.d_bud;   // (size mode: the batch's budgets, uploaded in front of the quantiser; null otherwise)
    if (sideBySide && ph.h_bound
            ? launch_speck_encode_head(b.ss, e, ph, b.raw_budget, rate, false)   // (its planes: late_planes)
            : launch_speck_encode(b.ss, e, ph, b.raw_budget, rate, false))
      return -1;
    b.wblocks = (uint32_t)std::min<size_t>(4096, (e.streamStride * 8 + kThreads - 1) / kThreads);
    if (!(sideBySide && ph.h_bound))
      write_slots(b, 0);
    return 0;
  }
  void write_slots(const Batch& b, int wide)
  {
    const EncBuffers& e = b.bb.eb;
    LAUNCH_K(k_write_slot, dim3(std::max(1u, b.wblocks), b.nb), dim3(kThreads), 0, b.ss, e.cst, e.st, e.stream,
             e.streamStride, b.bb.gids, static_cast<uint8_t*>(E.slots.p), d_slotOff, d_lens, b.P->N, wide);
  }
  // ---- retry with 64-bit coefficients (SPECK_FLT.cpp:530-538) ----
  // fixed rate: a finer q for the flagged chunks; PSNR: the same q, coefficients need 64 bits
  int retry_wide(Batch& b, const EncPlanHost& ph)
  {
    EncBatchBufs& bb = b.bb;
    EncBuffers& e = bb.eb;
    // the DWT coefficients again when the coder's arrays were written over them, and memory of
    // their own for those arrays (the 64-bit magnitudes live in the chunk buffer)
    if (bb.aliased && wide_retry_prepare<T>(b.ss, E, *b.P, bb, b.nb, b.P->dims, d_src, vd, b.orgAligned, chunk_range()))
      return -1;
    if ((rate ? launch_make_q_wide(b.ss, b.nb, e.cst) : launch_mark_wide(b.ss, b.nb, e.cst)) ||
        reset_enc_pass(b.ss, bb, b.nb))
      return -1;
    // 64-bit magnitudes overwrite the DWT coefficients in place (same element size)
    if (launch_quantize(b.ss, true, bb.vals, bb.valsStride, b.nb, b.P->N, bb.vals, bb.valsStride,
                        const_cast<uint64_t*>(e.sign), e.signStride, bb.msb, e.pixStride, e.cst))
      return -1;
    EncBuffers ew = e;
    ew.coef = bb.vals;
    ew.coefStride = bb.valsStride;
    if (launch_speck_encode(b.ss, ew, ph, b.raw_budget, rate, true))
      return -1;
    write_slots(b, 1);
    return 0;
  }
  // the groups that ran side by side: their plane loops, each over the planes that can hold work
  int late_planes()
  {
    for (Batch* L : late) {
      if (!L || !L->ph.h_bound)
        continue;
      if (launch_speck_encode_planes(L->ss, L->bb.eb, L->ph, L->raw_budget, rate, false))
        return -1;
      write_slots(*L, 0);
    }
    return 0;
  }
  // the groups side by side: the 64-bit retry, where a chunk asked for it
  int late_retry()
  {
    for (Batch* L : late) {
      if (!L)
        continue;
      L->hc.resize(L->nb);
      HIP_CHECK(hipMemcpyAsync(L->hc.data(), L->bb.eb.cst, L->nb * sizeof(CoderState), hipMemcpyDeviceToHost, L->ss));
      HIP_CHECK(hipStreamSynchronize(L->ss));
      bool retry = false;
      for (auto& cs : L->hc)
        retry |= (cs.need_retry != 0);
      if (!retry)
        continue;
      const ShapePlan& P = *L->P;
      const EncPlanHost ph{P.d_initLIS, P.d_initLen, P.d_depthBlocks, P.depthBlockOff, P.ht.nsets};
      // (retry_wide clears bb.aliased: the scratch memory is the engine's, one group at a time -- the next
      //  retrying group takes it over once this group's stream is through)
      const bool wasAliased = L->bb.aliased;
      if (retry_wide(*L, ph))
        return -1;
      if (wasAliased)
        HIP_CHECK(hipStreamSynchronize(L->ss));
    }
    return 0;
  }
  // ---- container ----
  int container()
  {
    // (the header kernels write before any length is known to them: check its room here)
    const uint32_t cpv = (uint32_t)(nchunks / nvol);   // chunks per container
    if (dst_cap < (slice ? (what == Coded::SliceWithHeader ? 10u : 0u) : ((cpv > 1 ? 20u : 14u) + 4ull * cpv) * nvol)) {
      fprintf(stderr, "[sperr_hip] output buffer too small for the container header (%zu bytes)\n", dst_cap);
      return -1;
    }
    if (nvol > 1 && slice)   // (a batch of slices: no length tables, a header per stream if any)
      LAUNCH_K(k_slice_batch_layout, dim3(1), dim3(kBatchThreads), 0, st, d_dst, (uint64_t)dst_cap, d_lens, d_lens2,
               d_offs, nchunks, (uint32_t)vol[0], (uint32_t)vol[1], std::is_same<T, float>::value ? 1 : 0,
               what == Coded::SliceWithHeader ? 1 : 0, d_total);
    else if (nvol > 1)   // (one container: k_container_header, as before)
      LAUNCH_K(k_batch_container, dim3(1), dim3(kBatchThreads), 0, st, d_dst, (uint64_t)dst_cap, d_lens, d_lens2,
               d_offs, nchunks, cpv, (uint32_t)vol[0], (uint32_t)vol[1], (uint32_t)vol[2], (uint32_t)cdim[0],
               (uint32_t)cdim[1], (uint32_t)cdim[2], std::is_same<T, float>::value ? 1 : 0, d_total);
    else if (slice)
      LAUNCH_K(k_slice_header, dim3(1), dim3(1), 0, st, d_dst, d_lens, d_lens2, d_offs,
               (uint32_t)vol[0], (uint32_t)vol[1], std::is_same<T, float>::value ? 1 : 0,
               what == Coded::SliceWithHeader ? 1 : 0, d_total);
    else
      LAUNCH_K(k_container_header, dim3(1), dim3(1), 0, st, d_dst, d_lens, d_lens2, d_offs, nchunks,
               (uint32_t)vol[0], (uint32_t)vol[1], (uint32_t)vol[2], (uint32_t)cdim[0],
               (uint32_t)cdim[1], (uint32_t)cdim[2], std::is_same<T, float>::value ? 1 : 0, d_total);
    const uint32_t gy = std::min<uint32_t>(nchunks, 32768u);
    const uint32_t gx = nchunks >= 4096 ? 4u : nchunks >= 256 ? 64u : 1024u;
    LAUNCH_K(k_copy_slots, dim3(gx, gy), dim3(kThreads), 0, st, d_dst, (uint64_t)dst_cap,
             static_cast<const uint8_t*>(E.slots.p), d_slotOff, d_lens, d_offs, nchunks);
    for (auto& k : pweKeep)
      LAUNCH_K(k_copy_slots2, dim3(256, k.nb), dim3(kThreads), 0, st, d_dst, (uint64_t)dst_cap, k.slots,
               k.slotOff, k.gids, d_lens, d_lens2, d_offs);
    if (nvol > 1) {
      bases.resize(nvol + 1);
      HIP_CHECK(hipMemcpyAsync(bases.data(), d_total, (nvol + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    else
      HIP_CHECK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    E.pweLastStream = nullptr;
    E.prof.collect();
    if (nvol > 1)
      total = bases[nvol];
    if (total > dst_cap) {
      fprintf(stderr, "[sperr_hip] output buffer too small (%zu < %llu)\n", dst_cap, (unsigned long long)total);
      return -1;
    }
    ok = true;
    return 0;
  }
};

template <typename T>
int compress_impl(Engine& E, const T* d_src, const Dims& vol, const Dims& chunkPref, int mode, double quality,
                  uint8_t* d_dst, size_t dst_cap, size_t* dst_len, hipStream_t st, Coded what = Coded::Container,
                  const ViewPitch* srcView = nullptr)
{
  EncodeCall<T> call{E, d_src, vol, mode, quality, d_dst, dst_cap, st, what, 1, srcView};
  if (call.run(chunkPref))
    return -1;
  *dst_len = (size_t)call.total;
  return 0;
}

// nvol volumes of dims `vol` back to back into nvol containers back to back: container v at
// [offsets[v], offsets[v + 1])
template <typename T>
int compress_batch_impl(Engine& E, const T* d_src, size_t nvol, const Dims& vol, const Dims& chunkPref, int mode,
                        double quality, uint8_t* d_dst, size_t dst_cap, size_t* offsets, hipStream_t st,
                        Coded what = Coded::Container)
{
  EncodeCall<T> call{E, d_src, vol, mode, quality, d_dst, dst_cap, st, what, nvol};
  if (call.run(chunkPref))
    return -1;
  if (nvol == 1) {
    offsets[0] = 0;
    offsets[1] = (size_t)call.total;
  }
  else
    for (size_t v = 0; v <= nvol; v++)
      offsets[v] = (size_t)call.bases[v];
  return 0;
}

// ------------------------------------------------------------------------------------------
// stage access (parity tests): helpers
// ------------------------------------------------------------------------------------------
template <typename CT>
__global__ void k_msb_of(const CT* coef, int8_t* msb, uint32_t n)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const unsigned long long v = coef[i];
  msb[i] = v ? (int8_t)(63 - __clzll((long long)v)) : (int8_t)-1;
}

// {u8 planes, u64 total_bits, payload} (SPECK_INT.cpp:284-308)
__global__ void __launch_bounds__(kThreads)
k_speck_stream_out(const CoderState* cst, const uint64_t* stream, uint8_t* dst, uint64_t cap,
                   uint64_t* len_out)
{
  const CoderState& cs = cst[0];
  const uint64_t len = cs.stream_len - 17;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *len_out = len;
  if (len > cap)
    return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dst[0] = (uint8_t)cs.nbp;
    memcpy(dst + 1, &cs.total_bits, 8);
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 9 < len;
       i += (uint64_t)gridDim.x * blockDim.x)
    dst[9 + i] = (uint8_t)(stream[i >> 3] >> (8 * (i & 7)));
}

}  // namespace

// ------------------------------------------------------------------------------------------
// the front (engine_core.h): the element type is chosen here, no template leaves this unit
// ------------------------------------------------------------------------------------------
int compress_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, int mode,
                double quality, uint8_t* d_dst, size_t dst_cap, size_t* dst_len, hipStream_t st, Coded what,
                const ViewPitch* srcView)
{
  return with_elem(is_float, [&](auto t) {
    return compress_impl(E, static_cast<const decltype(t)*>(d_src), vol, chunkPref, mode, quality, d_dst, dst_cap,
                         dst_len, st, what, srcView);
  });
}

int compress_batch_to(Engine& E, const void* d_src, int is_float, size_t nvol, const Dims& vol, const Dims& chunkPref,
                      int mode, double quality, uint8_t* d_dst, size_t dst_cap, size_t* offsets, hipStream_t st,
                      Coded what)
{
  return with_elem(is_float, [&](auto t) {
    return compress_batch_impl(E, static_cast<const decltype(t)*>(d_src), nvol, vol, chunkPref, mode, quality, d_dst,
                               dst_cap, offsets, st, what);
  });
}

// ---- the size mode's front ----
namespace {

// the survey's arrays and the deal's words in Engine::sizeWork, for a volume of n chunks
struct SizeWork {
  SizeSurveyDev sv;
  uint64_t* budgets;
  uint64_t* out;   // k_budget_deal's three words
};
int size_work(Engine& E, uint32_t n, SizeWork& w)
{
  const size_t bytes = round_up((size_t)n * 8, 256) * 2 + round_up((size_t)n * kBudgetPlanes * 8, 256) +
                       round_up((size_t)n * 4, 256) + round_up((size_t)n, 256) + 256;
  if (E.sizeWork.ensure(bytes))
    return -1;
  Arena A;
  A.base = static_cast<char*>(E.sizeWork.p);
  A.cap = E.sizeWork.n;
  w.sv.q = A.take<double>(n);
  w.sv.end = A.take<uint64_t>((size_t)n * kBudgetPlanes);
  w.budgets = A.take<uint64_t>(n);
  w.sv.nbp = A.take<int32_t>(n);
  w.sv.is_const = A.take<uint8_t>(n);
  w.out = A.take<uint64_t>(4);
  return w.sv.q && w.sv.end && w.budgets && w.sv.nbp && w.sv.is_const && w.out ? 0 : -1;
}

uint32_t size_chunk_count(const Dims& vol, const Dims& chunkPref)
{
  const size_t n = container_chunk_count(vol, chunkPref);
  return n > 0xffffffffull ? 0u : (uint32_t)n;   // (0: refused)
}

// pass 1: the survey of the volume into w (device)
template <typename T>
int survey_pass(Engine& E, const T* d_src, const Dims& vol, const Dims& chunkPref, hipStream_t st, const SizeWork& w)
{
  EncodeCall<T> call{E, d_src, vol, 1, 0.0, nullptr, 0, st, Coded::Container, 1, nullptr};
  call.sizePass = 1;
  call.sv = w.sv;
  return call.run(chunkPref) ? -1 : 0;
}

template <typename T>
int size_survey_impl(Engine& E, const T* d_src, const Dims& vol, const Dims& chunkPref, double* q, int32_t* nbp,
                     uint64_t* end, uint8_t* is_const, hipStream_t st)
{
  const uint32_t n = size_chunk_count(vol, chunkPref);
  SizeWork w;
  if (n == 0 || size_work(E, n, w) || survey_pass(E, d_src, vol, chunkPref, st, w))
    return -1;
  HIP_CHECK(hipMemcpyAsync(q, w.sv.q, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(nbp, w.sv.nbp, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(end, w.sv.end, (size_t)n * kBudgetPlanes * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(is_const, w.sv.is_const, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  E.prof.collect();
  return 0;
}

template <typename T>
int compress_size_impl(Engine& E, const T* d_src, const Dims& vol, const Dims& chunkPref, size_t target_bytes,
                       uint8_t* d_dst, size_t dst_cap, size_t* dst_len, uint64_t* budgets_out, hipStream_t st)
{
  const uint32_t n = size_chunk_count(vol, chunkPref);
  SizeWork w;
  if (n == 0 || budget_header_bytes(n) > target_bytes || size_work(E, n, w) || survey_pass(E, d_src, vol, chunkPref, st, w))
    return -1;
  // the deal: constness decides W, which the host states (budget_payload_bits) -- a first, small read-back --; the
  // kernel deals; a second read-back brings the budgets, which size pass 2's buffers
  std::vector<uint8_t> hconst(n);
  HIP_CHECK(hipMemcpyAsync(hconst.data(), w.sv.is_const, n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  uint64_t nconst = 0, W = 0;
  for (uint8_t c : hconst)
    nconst += c ? 1 : 0;
  if (!budget_payload_bits(target_bytes, n, nconst, &W)) {
    fprintf(stderr, "[sperr_hip] a target of %zu bytes does not hold the headers of %u chunks and a byte of each\n", target_bytes, n);
    return -1;
  }
  LAUNCH_K(k_budget_deal, dim3(1), dim3(kThreads), 0, st, w.sv, n, W, w.budgets, w.out);
  std::vector<uint64_t> hb(n);
  uint64_t hout[3] = {1, 0, 0};
  HIP_CHECK(hipMemcpyAsync(hb.data(), w.budgets, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hout, w.out, sizeof(hout), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  if (hout[0] != 0)
    return -1;
  uint64_t sum = 0;
  for (uint32_t c = 0; c < n; c++) {
    if (hconst[c] ? hb[c] != 0 : (hb[c] < 8 || hb[c] % 8 != 0))
      return -1;   // (not a deal)
    sum += hb[c];
  }
  if (sum > W)
    return -1;
  // pass 2: the fixed-rate flow on those budgets
  EncodeCall<T> call{E, d_src, vol, 1, 0.0, d_dst, dst_cap, st, Coded::Container, 1, nullptr};
  call.sizePass = 2;
  call.hBudgets = hb.data();
  if (call.run(chunkPref))
    return -1;
  if (call.total > target_bytes) {
    fprintf(stderr, "[sperr_hip] the dealt container has %llu bytes, beyond the target of %zu\n", (unsigned long long)call.total, target_bytes);
    return -1;
  }
  *dst_len = (size_t)call.total;
  if (budgets_out)
    memcpy(budgets_out, hb.data(), (size_t)n * 8);
  return 0;
}

}  // namespace

int size_survey_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, double* q, int32_t* nbp,
                   uint64_t* end, uint8_t* is_const, hipStream_t st)
{
  return with_elem(is_float, [&](auto t) {
    return size_survey_impl(E, static_cast<const decltype(t)*>(d_src), vol, chunkPref, q, nbp, end, is_const, st);
  });
}

int compress_size_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, size_t target_bytes,
                     uint8_t* d_dst, size_t dst_cap, size_t* dst_len, uint64_t* budgets_out, hipStream_t st)
{
  return with_elem(is_float, [&](auto t) {
    return compress_size_impl(E, static_cast<const decltype(t)*>(d_src), vol, chunkPref, target_bytes, d_dst, dst_cap, dst_len,
                              budgets_out, st);
  });
}

// ---- PSNR of the whole volume: the front ----
int compress_psnr_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, double psnr,
                     double range, uint8_t* d_dst, size_t dst_cap, size_t* dst_len, hipStream_t st,
                     const ViewPitch* srcView)
{
  // the volume's own range, also when the caller gives one: a NaN or an infinity among the samples is refused here,
  // before anything is coded, and a constant volume is known
  double vmin = 0.0, vmax = 0.0;
  if (range_to(E, d_src, is_float, vol, srcView, &vmin, &vmax, st))
    return -1;
  const double own = vmax - vmin;
  if (!std::isfinite(own)) {
    fprintf(stderr, "[sperr_hip] the volume's range [%g, %g] is not finite\n", vmin, vmax);
    return -1;
  }
  PsnrLadder L;
  // (a constant volume has constant chunks only, which take no q: the table is not looked at)
  if (!psnr_vol_ladder(range > 0.0 ? range : own, psnr, &L) && own != 0.0) {
    fprintf(stderr, "[sperr_hip] a range of %g at %g dB gives no quantisation step\n", range > 0.0 ? range : own, psnr);
    return -1;
  }
  return with_elem(is_float, [&](auto t) {
    EncodeCall<decltype(t)> call{E, static_cast<const decltype(t)*>(d_src), vol, 2, psnr, d_dst, dst_cap, st, Coded::Container, 1, srcView};
    call.volLadder = &L;
    if (call.run(chunkPref))
      return -1;
    *dst_len = (size_t)call.total;
    return 0;
  });
}

int outlier_encode_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_orig, int is_float,
                         const double* d_recon, uint32_t nb, double tol, uint8_t* d_dst, size_t dst_cap, size_t* lens)
{
  return with_elem(is_float, [&](auto t) {
    return outlier_encode_impl(E, st, P, static_cast<const decltype(t)*>(d_orig), d_recon, nb, tol, d_dst, dst_cap, lens);
  });
}

int speck3d_encode_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_coef, bool wide,
                         const uint64_t* d_sign, uint64_t raw_budget, uint8_t* d_dst, size_t dst_cap, size_t* dst_len)
{
  if (E.arena.ensure(enc_bytes_per_chunk(P, raw_budget) + 4096) || E.misc.ensure(4096))
    return -1;
  Arena A;
  A.base = static_cast<char*>(E.arena.p);
  A.cap = E.arena.n;
  EncBatchBufs bb;
  if (!carve_enc(A, P, 1, raw_budget, bb))
    return -1;
  if (wide && bb.aliased && unalias_coder(st, E, P, bb, 1))   // (the 64-bit magnitudes go into the chunk buffer)
    return -1;
  EncBuffers e = bb.eb;
  CoderState hcs;
  memset(&hcs, 0, sizeof(hcs));
  hcs.need_retry = wide ? 1u : 0u;  // the 64-bit pass only encodes chunks flagged for it
  hcs.wide = wide ? 1u : 0u;
  HIP_CHECK(hipMemcpyAsync(e.cst, &hcs, sizeof(CoderState), hipMemcpyHostToDevice, st));
  if (reset_enc_pass(st, bb, 1))
    return -1;
  const uint32_t n = P.N;
  HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t*>(e.sign), d_sign, ((n + 63) / 64) * 8,
                           hipMemcpyDeviceToDevice, st));
  if (wide) {
    HIP_CHECK(hipMemcpyAsync(bb.vals, d_coef, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    e.coef = bb.vals;
    e.coefStride = bb.valsStride;
    LAUNCH_K(k_msb_of<uint64_t>, dim3((n + 255) / 256), dim3(256), 0, st,
             reinterpret_cast<const uint64_t*>(bb.vals), bb.msb, n);
  }
  else {
    HIP_CHECK(hipMemcpyAsync(bb.coef32, d_coef, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    LAUNCH_K(k_msb_of<uint32_t>, dim3((n + 255) / 256), dim3(256), 0, st,
             reinterpret_cast<const uint32_t*>(bb.coef32), bb.msb, n);
  }
  EncPlanHost ph{P.d_initLIS, P.d_initLen, P.d_depthBlocks, P.depthBlockOff, P.ht.nsets};
  if (launch_speck_encode(st, e, ph, raw_budget, false, wide))
    return -1;
  uint64_t* d_len = static_cast<uint64_t*>(E.misc.p);
  LAUNCH_K(k_speck_stream_out, dim3(1024), dim3(kThreads), 0, st, e.cst, e.stream, d_dst, (uint64_t)dst_cap, d_len);
  uint64_t len = 0;
  HIP_CHECK(hipMemcpyAsync(&len, d_len, 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  E.prof.collect();
  if (len > dst_cap)
    return -1;
  *dst_len = (size_t)len;
  return 0;
}

// The plane table of one chunk's integer coefficients: the head of the 32-bit pass (pyramid, chain, census) and
// launch_speck_plane_table; no plane loop, no stream.  end[0 .. 63] and *nbp are the host's
int speck3d_plane_bits_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_coef, const uint64_t* d_sign,
                             uint64_t* end, int* nbp)
{
  if (P.dtree.flags & spk::kTree2D)
    return -1;
  const uint64_t raw_budget = 8;   // (sizes the stream and the birth masks, which nothing here writes)
  const size_t accWords = speck_plane_table_acc_words();
  if (E.arena.ensure(enc_bytes_per_chunk(P, raw_budget) + 8192) || E.misc.ensure(4096))
    return -1;
  Arena A;
  A.base = static_cast<char*>(E.arena.p);
  A.cap = E.arena.n;
  EncBatchBufs bb;
  if (!carve_enc(A, P, 1, raw_budget, bb))
    return -1;
  uint64_t* d_acc = A.take<uint64_t>(accWords);
  uint64_t* d_end = A.take<uint64_t>(kMaxPlanes);
  int32_t* d_nbp = A.take<int32_t>(1);
  if (!d_acc || !d_end || !d_nbp)
    return -1;
  EncBuffers e = bb.eb;
  CoderState hcs;
  memset(&hcs, 0, sizeof(hcs));
  HIP_CHECK(hipMemcpyAsync(e.cst, &hcs, sizeof(CoderState), hipMemcpyHostToDevice, st));
  if (reset_enc_pass(st, bb, 1))
    return -1;
  const uint32_t n = P.N;
  HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t*>(e.sign), d_sign, ((n + 63) / 64) * 8, hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(bb.coef32, d_coef, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  LAUNCH_K(k_msb_of<uint32_t>, dim3((n + 255) / 256), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(bb.coef32), bb.msb, n);
  EncPlanHost ph{P.d_initLIS, P.d_initLen, P.d_depthBlocks, P.depthBlockOff, P.ht.nsets};
  if (launch_speck_encode_head(st, e, ph, 0, false, false) || launch_speck_plane_table(st, e, ph, d_acc, d_end, d_nbp))
    return -1;
  int32_t hn = 0;
  HIP_CHECK(hipMemcpyAsync(end, d_end, kMaxPlanes * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&hn, d_nbp, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  E.prof.collect();
  *nbp = hn;
  return 0;
}

}  // namespace sperrhip
