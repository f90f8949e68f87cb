// mask.hip -- the kernels of missing values (mask.h: the rules, the stream, the constants).
//
//   k_mask_survey<T, kVec>   one read of the volume: the bit array, lo / hi of the valid samples, the counts
//                            (k_mask_scan is taken: the encoder's, speck_enc.hip)
//   k_mask_finish            one workgroup: F, the kind, the tiles' toggle offsets, the header, the read-back record
//   k_mask_pack              the stream: header, and toggles at tile offset + rank (kind 1) or the words (kind 2)
//   k_mask_fill<T, kVec>     dst[i] = missing ? F : src[i], F the midrange value or the caller's; dst may be src
//                            (the smooth fill's kernels are mask_fill.hip's)
//   k_mask_apply<T>          `value` into the missing samples of a box of a volume, and nothing else
//   k_mask_expand            the mask as bytes of 0 / 1
//   k_mask_unpack            a stream of toggles as the bit array
//   k_mask_count, k_mask_offsets, k_mask_compact<T>   the valid samples of an array, in order: count, scan, scatter
//
// A wavefront takes a tile of kMaskTile samples at a time -- 16 words of the bit array -- and walks the tiles beyond
// the grid, which is capped at kMaskGroupsPerCU workgroups per CU.  No kernel waits on another workgroup: what needs
// a prefix over tiles is count -> scan -> scatter in separate launches.  No float atomics: lo and hi are reduced on
// their integer keys by shuffles, then LDS, then one partial per workgroup.
// kVec loads (and in k_mask_fill stores) 16 bytes per lane; the host chooses it when the pointers are 16-byte aligned.
// The other form moves element by element and needs the alignment of T only.
#include "common.h"
#include "mask.h"
#include "mask_fill.h"

namespace sperrhip {

namespace {

constexpr uint32_t kWavesPerGroup = kMaskThreads / 64;
constexpr uint32_t kFinishThreads = 1024, kFinishPer = 8;   // k_mask_finish / k_mask_offsets: entries per round

template <typename T>
struct MaskPack;
template <>
struct MaskPack<float> {
  typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct MaskPack<double> {
  typedef double type __attribute__((ext_vector_type(2)));
};

// what the first half of a call leaves on the device for the second
struct MaskFin {
  double fill;
  uint64_t toggles;
  MaskResult res;
  uint8_t header[kMaskHeaderBytes];
};

// the workspace: the bit array, the tiles' counts and offsets, the workgroups' partials, MaskFin
struct MaskWs {
  uint64_t* words;
  uint32_t* tileCnt;
  uint64_t* tileOff;
  uint64_t* partials;   // {lo key, hi key, missing} per workgroup
  MaskFin* fin;
  size_t bytes;
};

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

bool mask_ws(size_t n, void* base, uint32_t maxGroups, MaskWs& w)
{
  if (n == 0 || n > SIZE_MAX / 2)
    return false;
  const size_t nwords = (size_t)mask_words(n), ntiles = (n + kMaskTile - 1) / kMaskTile;
  char* p = static_cast<char*>(base);
  size_t at = 0;
  w.words = reinterpret_cast<uint64_t*>(p + at);
  at += up256(nwords * 8);
  w.tileCnt = reinterpret_cast<uint32_t*>(p + at);
  at += up256(ntiles * 4);
  w.tileOff = reinterpret_cast<uint64_t*>(p + at);
  at += up256(ntiles * 8);
  w.partials = reinterpret_cast<uint64_t*>(p + at);
  at += up256((size_t)maxGroups * 3 * 8);
  w.fin = reinterpret_cast<MaskFin*>(p + at);
  at += up256(sizeof(MaskFin));
  w.bytes = at;
  return true;
}

// the most workgroups any grid here has: a bound that needs no device query (the workspace is sized with it)
constexpr uint32_t kMaskMaxGroups = 8192;

// workgroups for `items` wavefront-sized pieces of work
int mask_grid(uint64_t items, uint32_t* groups)
{
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const uint64_t cap = std::min<uint64_t>((uint64_t)std::max(cus, 1) * kMaskGroupsPerCU, kMaskMaxGroups);
  const uint64_t want = (items + kWavesPerGroup - 1) / kWavesPerGroup;
  *groups = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
  return 0;
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    v = min(v, (uint64_t)__shfl_xor((unsigned long long)v, d, 64));
  return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    v = max(v, (uint64_t)__shfl_xor((unsigned long long)v, d, 64));
  return v;
}

template <typename T, bool kVec>
__global__ __launch_bounds__(kMaskThreads) void k_mask_survey(const T* __restrict__ src, uint64_t n, int rule,
                                                              double threshold, uint64_t* __restrict__ words,
                                                              uint32_t* __restrict__ tileTog,
                                                              uint64_t* __restrict__ partials)
{
  constexpr uint32_t P = kVec ? kMaskPackBytes / sizeof(T) : 1;
  constexpr uint32_t kIter = kMaskTile / (64 * P);   // loads of a lane per tile
  using Pack = typename MaskPack<T>::type;
  __shared__ uint64_t s_part[kWavesPerGroup][3];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ntiles = (n + kMaskTile - 1) / kMaskTile;
  uint64_t lo = kMaskKeyNone, hi = 0, miss = 0;   // (miss: the same in every lane)
  for (uint64_t tile = (uint64_t)blockIdx.x * kWavesPerGroup + wave; tile < ntiles;
       tile += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t s0 = tile * kMaskTile;
    // the sample before the tile, not the word before it: tiles stay independent
    uint64_t carry = s0 > 0 && mask_missing(src[s0 - 1], rule, threshold) ? 1 : 0;
    T v[kIter][P];
#pragma unroll
    for (uint32_t it = 0; it < kIter; it++) {
      const uint64_t i = s0 + (uint64_t)(it * 64 + lane) * P;
      if (kVec && i + P <= n) {
        const Pack pk = *reinterpret_cast<const Pack*>(src + i);
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          v[it][j] = pk[j];
      }
      else {
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          v[it][j] = i + j < n ? src[i + j] : T(0);
      }
    }
    uint32_t tog = 0;
#pragma unroll
    for (uint32_t it = 0; it < kIter; it++) {
      const uint64_t i = s0 + (uint64_t)(it * 64 + lane) * P;
      uint64_t ballot[P];
#pragma unroll
      for (uint32_t j = 0; j < P; j++) {
        const bool in = i + j < n;
        const bool m = in && mask_missing(v[it][j], rule, threshold);
        ballot[j] = __ballot(m);
        if (in && !m) {
          const uint64_t k = mask_key(v[it][j]);
          lo = min(lo, k);
          hi = max(hi, k);
        }
      }
#pragma unroll
      for (uint32_t w = 0; w < P; w++) {
        const uint64_t sw = s0 + (uint64_t)(it * P + w) * 64;
        if (sw < n) {
          const uint64_t word = mask_word_of_ballots<P>(ballot, w);
          const uint32_t nbits = (uint32_t)min((uint64_t)64, n - sw);
          tog += __popcll(mask_toggle_bits(word, carry, nbits));
          miss += __popcll(word);
          carry = word >> 63;
          if (lane == w)
            words[sw >> 6] = word;
        }
      }
    }
    if (lane == 0)
      tileTog[tile] = tog;
  }
  lo = wave_min64(lo);
  hi = wave_max64(hi);
  if (lane == 0) {
    s_part[wave][0] = lo;
    s_part[wave][1] = hi;
    s_part[wave][2] = miss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kWavesPerGroup; w++) {
      lo = min(lo, s_part[w][0]);
      hi = max(hi, s_part[w][1]);
      miss += s_part[w][2];
    }
    partials[(uint64_t)blockIdx.x * 3 + 0] = lo;
    partials[(uint64_t)blockIdx.x * 3 + 1] = hi;
    partials[(uint64_t)blockIdx.x * 3 + 2] = miss;
  }
}

// exclusive offsets of `count` tile counts, by one workgroup of kFinishThreads; the total comes back in every thread
__device__ uint64_t mask_scan_tiles(const uint32_t* __restrict__ cnt, uint64_t* __restrict__ off, uint64_t count,
                                    uint64_t* smem)
{
  uint64_t running = 0;
  for (uint64_t base = 0; base < count; base += (uint64_t)kFinishThreads * kFinishPer) {
    const uint64_t i0 = base + (uint64_t)threadIdx.x * kFinishPer;
    uint32_t c[kFinishPer];
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFinishPer; j++) {
      c[j] = i0 + j < count ? cnt[i0 + j] : 0;
      mine += c[j];
    }
    uint64_t total = 0;
    uint64_t at = running + block_exclusive_scan<uint64_t>(mine, smem, &total);
#pragma unroll
    for (uint32_t j = 0; j < kFinishPer; j++) {
      if (i0 + j < count)
        off[i0 + j] = at;
      at += c[j];
    }
    running += total;
  }
  return running;
}

__global__ __launch_bounds__(kFinishThreads) void k_mask_finish(const uint64_t* __restrict__ partials, uint32_t nparts,
                                                                const uint32_t* __restrict__ tileTog,
                                                                uint64_t* __restrict__ tileOff, uint64_t ntiles,
                                                                uint64_t n, int is_float, MaskFin* __restrict__ fin)
{
  __shared__ uint64_t s_scan[kFinishThreads / 64 + 1];
  __shared__ uint64_t s_red[kFinishThreads / 64][3];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t lo = kMaskKeyNone, hi = 0, miss = 0;
  for (uint32_t p = threadIdx.x; p < nparts; p += kFinishThreads) {
    lo = min(lo, partials[(uint64_t)p * 3 + 0]);
    hi = max(hi, partials[(uint64_t)p * 3 + 1]);
    miss += partials[(uint64_t)p * 3 + 2];
  }
  lo = wave_min64(lo);
  hi = wave_max64(hi);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    miss += (uint64_t)__shfl_xor((unsigned long long)miss, d, 64);
  if (lane == 0) {
    s_red[wave][0] = lo;
    s_red[wave][1] = hi;
    s_red[wave][2] = miss;
  }
  __syncthreads();
  const uint64_t toggles = mask_scan_tiles(tileTog, tileOff, ntiles, s_scan);
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kFinishThreads / 64; w++) {
      lo = min(lo, s_red[w][0]);
      hi = max(hi, s_red[w][1]);
      miss += s_red[w][2];
    }
    bool finite = true;
    fin->fill = mask_fill_value(lo, hi, miss < n, is_float != 0, &finite);
    fin->toggles = toggles;
    const MaskHeader h = mask_header_of(n, miss, toggles);
    mask_write_header(h, fin->header);
    fin->res = MaskResult{kMaskHeaderBytes + mask_payload_bytes(h.kind, h.count), miss, finite ? 1ull : 0ull,
                          (uint64_t)h.kind};
  }
}

// lane per word: a wavefront takes 64 words, four tiles
__global__ __launch_bounds__(kMaskThreads) void k_mask_pack(const uint64_t* __restrict__ words,
                                                            const uint64_t* __restrict__ tileOff,
                                                            const MaskFin* __restrict__ fin, uint64_t n, int kind,
                                                            uint8_t* __restrict__ d_mask)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x < kMaskHeaderBytes)
    d_mask[threadIdx.x] = fin->header[threadIdx.x];
  const uint64_t nwords = mask_words(n);
  if (kind == kMaskKindBits) {
    uint64_t* out = reinterpret_cast<uint64_t*>(d_mask + kMaskHeaderBytes);
    for (uint64_t w = (uint64_t)blockIdx.x * kMaskThreads + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * kMaskThreads)
      out[w] = words[w];
    return;
  }
  if (kind != kMaskKindToggles)
    return;
  uint32_t* out = reinterpret_cast<uint32_t*>(d_mask + kMaskHeaderBytes);
  const uint64_t nruns = (nwords + 63) / 64;
  for (uint64_t run = (uint64_t)blockIdx.x * kWavesPerGroup + wave; run < nruns;
       run += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t w = run * 64 + lane;
    uint64_t t = 0;
    if (w < nwords) {
      const uint64_t carry = w > 0 ? words[w - 1] >> 63 : 0;
      t = mask_toggle_bits(words[w], carry, (uint32_t)min((uint64_t)64, n - w * 64));
    }
    const uint32_t c = __popcll(t);
    const uint32_t before = wave_inclusive_scan<uint32_t>(c) - c;
    // the rank inside the word's tile: the prefix less that of the tile's first word
    const uint32_t rank = before - __shfl(before, lane & ~(kMaskTileWords - 1), 64);
    if (t) {
      uint64_t at = tileOff[w / kMaskTileWords] + rank;
      while (t) {
        out[at++] = (uint32_t)(w * 64 + __builtin_ctzll(t));
        t &= t - 1;
      }
    }
  }
}

template <typename T, bool kVec>
__global__ __launch_bounds__(kMaskThreads) void k_mask_fill(const T* src, T* dst, uint64_t n,
                                                            const uint64_t* __restrict__ words,
                                                            const MaskFin* __restrict__ fin, double value)
{
  constexpr uint32_t P = kVec ? kMaskPackBytes / sizeof(T) : 1;
  using Pack = typename MaskPack<T>::type;
  const T fill = (T)(fin ? fin->fill : value);   // (fin NULL: the caller's value)
  const uint64_t npacks = (n + P - 1) / P;
  for (uint64_t p = (uint64_t)blockIdx.x * kMaskThreads + threadIdx.x; p < npacks; p += (uint64_t)gridDim.x * kMaskThreads) {
    const uint64_t i = p * P;
    const uint32_t bits = (uint32_t)(words[i >> 6] >> (i & 63));   // (P divides 64: a pack lies in one word)
    if (kVec && i + P <= n) {
      Pack pk = *reinterpret_cast<const Pack*>(src + i);
#pragma unroll
      for (uint32_t j = 0; j < P; j++)
        if ((bits >> j) & 1)
          pk[j] = fill;
      *reinterpret_cast<Pack*>(dst + i) = pk;
    }
    else {
      for (uint32_t j = 0; j < P && i + j < n; j++)
        dst[i + j] = ((bits >> j) & 1) ? fill : src[i + j];
    }
  }
}

// ---- readers of a stream -------------------------------------------------------------------------------------------
struct MaskSrc {
  const uint64_t* words;   // kind 2
  const uint32_t* tog;     // kind 1
  uint64_t count, n;
  int kind;
};

struct MaskCursor {
  uint64_t idx, state;
};

// a cursor at sample s: for toggles, the first one at or behind s by binary search; its index's low bit is bit(s - 1)
__device__ __forceinline__ MaskCursor mask_cursor(const MaskSrc& m, uint64_t s)
{
  MaskCursor c{0, 0};
  if (m.kind == kMaskKindToggles) {
    c.idx = mask_toggle_lower_bound(m.tog, m.count, s);
    c.state = c.idx & 1;
  }
  return c;
}

// the samples [s, s + 64) as a word (s < n; the bits at or behind n mean nothing); calls of a cursor go upwards in s
__device__ __forceinline__ uint64_t mask_next64(const MaskSrc& m, MaskCursor& c, uint64_t s)
{
  if (m.kind == kMaskKindBits) {
    const uint64_t wi = s >> 6;
    const uint32_t sh = (uint32_t)(s & 63);
    uint64_t w = m.words[wi] >> sh;
    if (sh && wi + 1 < m.count)
      w |= m.words[wi + 1] << (64 - sh);
    return w;
  }
  if (m.kind == kMaskKindToggles)
    return mask_word_from_toggles(m.tog, m.count, s, &c.idx, &c.state);
  return 0;
}

struct MaskBox {
  uint64_t vx, vy;          // the volume's row and slice extents
  uint64_t lx, ly, lz;      // the box's origin
  uint64_t bx, by, rows;    // the box's row length, rows per slice, rows in all
  uint64_t pieces;          // kMaskTile pieces of a row
};

template <typename T>
__global__ __launch_bounds__(kMaskThreads) void k_mask_apply(T* __restrict__ dst, MaskBox g, MaskSrc m, T value)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t items = g.rows * g.pieces;
  for (uint64_t item = (uint64_t)blockIdx.x * kWavesPerGroup + wave; item < items;
       item += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t row = item / g.pieces, piece = item - row * g.pieces;
    const uint64_t z = row / g.by, y = row - z * g.by;
    // the row is the bit range [base, base + bx) of the volume
    const uint64_t base = ((g.lz + z) * g.vy + g.ly + y) * g.vx + g.lx;
    const uint64_t x0 = piece * kMaskTile, x1 = min(g.bx, x0 + kMaskTile);
    T* d = dst + row * g.bx;
    MaskCursor c = mask_cursor(m, base + x0);
    for (uint64_t x = x0; x < x1; x += 64) {
      const uint64_t w = mask_next64(m, c, base + x);
      if (((w >> lane) & 1) && x + lane < x1)
        d[x + lane] = value;
    }
  }
}

__global__ __launch_bounds__(kMaskThreads) void k_mask_expand(unsigned char* __restrict__ out, MaskSrc m)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ntiles = (m.n + kMaskTile - 1) / kMaskTile;
  for (uint64_t tile = (uint64_t)blockIdx.x * kWavesPerGroup + wave; tile < ntiles;
       tile += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t s0 = tile * kMaskTile, s1 = min(m.n, s0 + kMaskTile);
    MaskCursor c = mask_cursor(m, s0);
    for (uint64_t s = s0; s < s1; s += 64) {
      const uint64_t w = mask_next64(m, c, s);
      if (s + lane < s1)
        out[s + lane] = (unsigned char)((w >> lane) & 1);
    }
  }
}

// toggles -> the bit array (tail bits 0)
__global__ __launch_bounds__(kMaskThreads) void k_mask_unpack(uint64_t* __restrict__ words, MaskSrc m)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ntiles = (m.n + kMaskTile - 1) / kMaskTile;
  for (uint64_t tile = (uint64_t)blockIdx.x * kWavesPerGroup + wave; tile < ntiles;
       tile += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t s0 = tile * kMaskTile, s1 = min(m.n, s0 + kMaskTile);
    MaskCursor c = mask_cursor(m, s0);
    uint64_t mine = 0;
    uint32_t k = 0;
    for (uint64_t s = s0; s < s1; s += 64, k++) {
      uint64_t w = mask_next64(m, c, s);
      if (s1 - s < 64)
        w &= (uint64_t(1) << (s1 - s)) - 1;
      if (lane == k)
        mine = w;
    }
    if (lane < k)
      words[tile * kMaskTileWords + lane] = mine;
  }
}

// the valid samples of every tile: lane per word, as k_mask_pack
__global__ __launch_bounds__(kMaskThreads) void k_mask_count(const uint64_t* __restrict__ words, uint64_t n,
                                                             uint32_t* __restrict__ tileCnt)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t nwords = mask_words(n), nruns = (nwords + 63) / 64;
  for (uint64_t run = (uint64_t)blockIdx.x * kWavesPerGroup + wave; run < nruns;
       run += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t w = run * 64 + lane;
    uint32_t c = 0;
    if (w < nwords) {
      const uint64_t left = n - w * 64;
      c = __popcll(~words[w] & (left >= 64 ? ~uint64_t(0) : (uint64_t(1) << left) - 1));
    }
#pragma unroll
    for (uint32_t d = 1; d < kMaskTileWords; d <<= 1)
      c += __shfl_xor(c, d, 64);
    if (w < nwords && lane % kMaskTileWords == 0)
      tileCnt[w / kMaskTileWords] = c;
  }
}

__global__ __launch_bounds__(kFinishThreads) void k_mask_offsets(const uint32_t* __restrict__ tileCnt,
                                                                 uint64_t* __restrict__ tileOff, uint64_t ntiles)
{
  __shared__ uint64_t s_scan[kFinishThreads / 64 + 1];
  (void)mask_scan_tiles(tileCnt, tileOff, ntiles, s_scan);
}

template <typename T>
__global__ __launch_bounds__(kMaskThreads) void k_mask_compact(const T* __restrict__ src, T* __restrict__ dst,
                                                               uint64_t n, const uint64_t* __restrict__ words,
                                                               const uint64_t* __restrict__ tileOff)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ntiles = (n + kMaskTile - 1) / kMaskTile;
  for (uint64_t tile = (uint64_t)blockIdx.x * kWavesPerGroup + wave; tile < ntiles;
       tile += (uint64_t)gridDim.x * kWavesPerGroup) {
    const uint64_t s0 = tile * kMaskTile, s1 = min(n, s0 + kMaskTile);
    uint64_t at = tileOff[tile];
    for (uint64_t s = s0; s < s1; s += 64) {
      uint64_t valid = ~words[s >> 6];
      if (s1 - s < 64)
        valid &= (uint64_t(1) << (s1 - s)) - 1;
      if ((valid >> lane) & 1)
        dst[at + __popcll(valid & ((uint64_t(1) << lane) - 1))] = src[s + lane];
      at += __popcll(valid);
    }
  }
}

MaskSrc mask_src(const MaskStream& m)
{
  return MaskSrc{static_cast<const uint64_t*>(m.d_payload), static_cast<const uint32_t*>(m.d_payload), m.h.count, m.h.n,
                 m.h.kind};
}

template <typename T>
int scan_launch(const T* src, size_t n, int rule, double threshold, const MaskWs& w, uint32_t groups, hipStream_t st)
{
  if ((uintptr_t)src % kMaskPackBytes == 0)
    LAUNCH_K((k_mask_survey<T, true>), dim3(groups), dim3(kMaskThreads), 0, st, src, (uint64_t)n, rule, threshold,
             w.words, w.tileCnt, w.partials);
  else
    LAUNCH_K((k_mask_survey<T, false>), dim3(groups), dim3(kMaskThreads), 0, st, src, (uint64_t)n, rule, threshold,
             w.words, w.tileCnt, w.partials);
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int fill_launch(const T* src, T* dst, size_t n, const MaskWs& w, const MaskFill* fill, hipStream_t st)
{
  const MaskFin* fin = fill && fill->kind == kMaskFillValue ? nullptr : w.fin;
  const double value = fill ? fill->value : 0.0;
  const bool vec = (uintptr_t)src % kMaskPackBytes == 0 && (uintptr_t)dst % kMaskPackBytes == 0;
  const uint64_t packs = vec ? (n + kMaskPackBytes / sizeof(T) - 1) / (kMaskPackBytes / sizeof(T)) : n;
  uint32_t groups = 0;
  if (mask_grid((packs + 63) / 64, &groups))
    return -1;
  if (vec)
    LAUNCH_K((k_mask_fill<T, true>), dim3(groups), dim3(kMaskThreads), 0, st, src, dst, (uint64_t)n, w.words, fin,
             value);
  else
    LAUNCH_K((k_mask_fill<T, false>), dim3(groups), dim3(kMaskThreads), 0, st, src, dst, (uint64_t)n, w.words, fin,
             value);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

size_t mask_workspace_bytes(size_t n)
{
  MaskWs w;
  return mask_ws(n, nullptr, kMaskMaxGroups, w) ? w.bytes : 0;
}

const uint64_t* mask_bit_words(void* ws, size_t n)
{
  MaskWs w;
  return ws && mask_ws(n, ws, kMaskMaxGroups, w) ? w.words : nullptr;
}

uint64_t* mask_result_finite(void* ws, size_t n)
{
  MaskWs w;
  return ws && mask_ws(n, ws, kMaskMaxGroups, w) ? &w.fin->res.finite : nullptr;
}

static_assert(kMaskBitsMaxGroups == kMaskMaxGroups, "the workspace holds a record per workgroup");

bool mask_bits_parts(void* ws, size_t n, MaskBitsParts* parts)
{
  MaskWs w;
  if (!ws || !parts || !mask_ws(n, ws, kMaskMaxGroups, w))
    return false;
  *parts = MaskBitsParts{w.words, w.tileCnt, w.partials, &w.fin->res};
  return true;
}

int mask_bits_finish_run(void* ws, size_t n, uint32_t ngroups, void* hip_stream)
{
  MaskWs w;
  if (!ws || ngroups == 0 || ngroups > kMaskMaxGroups || !mask_ws(n, ws, kMaskMaxGroups, w))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  LAUNCH_K(k_mask_finish, dim3(1), dim3(kFinishThreads), 0, st, w.partials, ngroups, w.tileCnt, w.tileOff,
           (uint64_t)((n + kMaskTile - 1) / kMaskTile), (uint64_t)n, 0, w.fin);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int mask_scan_run(const void* d_src, int is_float, size_t n, int rule, double threshold, void* ws, MaskResult* res,
                  void* hip_stream, const MaskFill* fill)
{
  MaskWs w;
  if (!d_src || !ws || !res || !mask_rule_ok(rule, threshold) || !mask_ws(n, ws, kMaskMaxGroups, w))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t ntiles = (n + kMaskTile - 1) / kMaskTile;
  uint32_t groups = 0;
  if (mask_grid(ntiles, &groups))
    return -1;
  if (is_float ? scan_launch(static_cast<const float*>(d_src), n, rule, threshold, w, groups, st)
               : scan_launch(static_cast<const double*>(d_src), n, rule, threshold, w, groups, st))
    return -1;
  LAUNCH_K(k_mask_finish, dim3(1), dim3(kFinishThreads), 0, st, w.partials, groups, w.tileCnt, w.tileOff, ntiles,
           (uint64_t)n, is_float, w.fin);
  HIP_CHECK(hipGetLastError());
  // (k_mask_top, behind k_mask_finish, sets res.finite anew: the smooth rule's refusal in the place of the midrange's)
  if (fill && fill->kind == kMaskFillSmooth &&
      (!fill->plan || fill->plan->cells[0] != n ||
       mask_fill_pull_run(d_src, is_float, *fill->plan, ws, fill->pyr, hip_stream)))
    return -1;
  HIP_CHECK(hipMemcpyAsync(res, &w.fin->res, sizeof(MaskResult), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

int mask_pack_fill_run(const void* d_src, int is_float, size_t n, const void* ws, const MaskResult& res, void* d_mask,
                       void* d_filled, void* hip_stream, const MaskFill* fill)
{
  MaskWs w;
  if (!d_src || !ws || !mask_ws(n, const_cast<void*>(ws), kMaskMaxGroups, w))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (d_mask) {
    if ((uintptr_t)d_mask % 8 != 0)
      return -1;
    const uint64_t nwords = mask_words(n);
    // kind 1: a wavefront per 64 words; kind 2: a lane per word; kind 0: the header alone
    const uint64_t items = res.kind == kMaskKindNone ? 1 : (nwords + 63) / 64;
    uint32_t groups = 0;
    if (mask_grid(items, &groups))
      return -1;
    LAUNCH_K(k_mask_pack, dim3(groups), dim3(kMaskThreads), 0, st, w.words, w.tileOff, w.fin, (uint64_t)n, (int)res.kind,
             static_cast<uint8_t*>(d_mask));
    HIP_CHECK(hipGetLastError());
  }
  if (d_filled && fill && fill->kind == kMaskFillSmooth) {
    if (!fill->plan || fill->plan->cells[0] != n ||
        mask_fill_push_run(d_src, is_float, *fill->plan, ws, fill->pyr, d_filled, hip_stream))
      return -1;
  }
  else if (d_filled) {
    if (is_float ? fill_launch(static_cast<const float*>(d_src), static_cast<float*>(d_filled), n, w, fill, st)
                 : fill_launch(static_cast<const double*>(d_src), static_cast<double*>(d_filled), n, w, fill, st))
      return -1;
  }
  return 0;
}

int mask_apply_run(void* d_box, int is_float, const size_t vol[3], const size_t lo[3], const size_t dims[3],
                   const MaskStream& m, double value, void* hip_stream)
{
  if (!d_box || !m.d_payload)
    return -1;
  if (m.h.kind == kMaskKindNone)
    return 0;
  MaskBox g;
  const bool whole = dims[0] == vol[0] && dims[1] == vol[1] && dims[2] == vol[2];
  if (whole)   // one row of n samples
    g = MaskBox{m.h.n, 1, 0, 0, 0, m.h.n, 1, 1, 0};
  else
    g = MaskBox{vol[0], vol[1], lo[0], lo[1], lo[2], dims[0], dims[1], (uint64_t)dims[1] * dims[2], 0};
  g.pieces = (g.bx + kMaskTile - 1) / kMaskTile;
  uint32_t groups = 0;
  if (mask_grid(g.rows * g.pieces, &groups))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (is_float)
    LAUNCH_K((k_mask_apply<float>), dim3(groups), dim3(kMaskThreads), 0, st, static_cast<float*>(d_box), g, mask_src(m),
             (float)value);
  else
    LAUNCH_K((k_mask_apply<double>), dim3(groups), dim3(kMaskThreads), 0, st, static_cast<double*>(d_box), g,
             mask_src(m), value);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int mask_expand_run(const MaskStream& m, unsigned char* d_out, void* hip_stream)
{
  if (!d_out || !m.d_payload)
    return -1;
  uint32_t groups = 0;
  if (mask_grid((m.h.n + kMaskTile - 1) / kMaskTile, &groups))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  LAUNCH_K(k_mask_expand, dim3(groups), dim3(kMaskThreads), 0, st, d_out, mask_src(m));
  HIP_CHECK(hipGetLastError());
  return 0;
}

int mask_compact_run(const void* const* d_src, void* const* d_dst, int nsrc, int is_float, const MaskStream& m,
                     void* ws, void* hip_stream)
{
  MaskWs w;
  const size_t n = (size_t)m.h.n;
  if (!d_src || !d_dst || nsrc < 1 || !m.d_payload || !mask_ws(n, ws, kMaskMaxGroups, w))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t ntiles = (n + kMaskTile - 1) / kMaskTile, nwords = mask_words(n);
  uint32_t groups = 0;
  if (mask_grid(ntiles, &groups))
    return -1;
  const uint64_t* words = static_cast<const uint64_t*>(m.d_payload);
  if (m.h.kind == kMaskKindToggles) {
    LAUNCH_K(k_mask_unpack, dim3(groups), dim3(kMaskThreads), 0, st, w.words, mask_src(m));
    HIP_CHECK(hipGetLastError());
    words = w.words;
  }
  else if (m.h.kind == kMaskKindNone) {
    HIP_CHECK(hipMemsetAsync(w.words, 0, nwords * 8, st));
    words = w.words;
  }
  uint32_t cgroups = 0;
  if (mask_grid((nwords + 63) / 64, &cgroups))
    return -1;
  LAUNCH_K(k_mask_count, dim3(cgroups), dim3(kMaskThreads), 0, st, words, (uint64_t)n, w.tileCnt);
  HIP_CHECK(hipGetLastError());
  LAUNCH_K(k_mask_offsets, dim3(1), dim3(kFinishThreads), 0, st, w.tileCnt, w.tileOff, ntiles);
  HIP_CHECK(hipGetLastError());
  for (int a = 0; a < nsrc; a++) {
    if (!d_src[a] || !d_dst[a])
      return -1;
    if (is_float)
      LAUNCH_K((k_mask_compact<float>), dim3(groups), dim3(kMaskThreads), 0, st, static_cast<const float*>(d_src[a]),
               static_cast<float*>(d_dst[a]), (uint64_t)n, words, w.tileOff);
    else
      LAUNCH_K((k_mask_compact<double>), dim3(groups), dim3(kMaskThreads), 0, st, static_cast<const double*>(d_src[a]),
               static_cast<double*>(d_dst[a]), (uint64_t)n, words, w.tileOff);
    HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace sperrhip
