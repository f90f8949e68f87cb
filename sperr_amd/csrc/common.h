// common.h -- shared declarations of the HIP engine (device state structs, launch helpers).
#ifndef SPERR_AMD_COMMON_H
#define SPERR_AMD_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <stdlib.h>
#include <type_traits>
#include "speck_tree.h"

#define HIP_CHECK(expr)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      fprintf(stderr, "[sperr_hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),    \
              __FILE__, __LINE__);                                                            \
      return -1;                                                                              \
    }                                                                                         \
  } while (0)

namespace sperrhip {

// per-kernel profiling hooks (engine.hip): no-ops unless sperrhip_profile_enable(1)
void prof_begin(const char* name, hipStream_t stream);
void prof_end(hipStream_t stream);
// allow `bytes` of dynamic LDS for a kernel on the current device (engine.hip; once per device)
int set_max_dyn_lds(const void* fn, int bytes);
#define LAUNCH_K(kern, grid, block, smem, stream, ...)                \
  do {                                                                \
    ::sperrhip::prof_begin(#kern, stream);                            \
    hipLaunchKernelGGL(kern, grid, block, smem, stream, __VA_ARGS__); \
    ::sperrhip::prof_end(stream);                                     \
  } while (0)

constexpr int kMaxPlanes = 64;     // bit planes of a uint64 coefficient
constexpr int kPixPer = 16;        // consecutive samples per thread in the pixel passes
constexpr int kPixTile = 4096;     // samples per pixel-pass tile (256 threads x kPixPer)
constexpr int kListTile = 1024;    // list entries per list-pass tile (256 threads x 4)
constexpr int kThreads = 256;
// Per-plane kernels are launched with at most this many workgroups over all chunks and stride
// over their work: most planes hold little work, and a grid sized for the worst case costs more
// in empty workgroups than the plane's real work.
constexpr uint32_t kGridCap = 4096;        // kernels that do little per item
constexpr uint32_t kGridCapWide = 16384;   // latency-bound kernels that want every wave slot
inline uint32_t capped_blocks(uint32_t nblocks, uint32_t nchunks, uint32_t total = kGridCap)
{
  uint32_t cap = total / (nchunks ? nchunks : 1u);
  if (cap < 1u)
    cap = 1u;
  if (nblocks < 1u)
    nblocks = 1u;
  return nblocks < cap ? nblocks : cap;
}

// ---- geometry of one batch: `nchunks` chunks of identical dims cut from one volume ------------
struct ChunkGeom {         // one entry per chunk of the batch (device array)
  uint32_t org[3];         // origin inside the volume
};

struct VolDesc {
  uint64_t dims[3];        // volume dims (x fastest)
};

// The crop variant of the last writers (kCrop kernels, decoding a sub-box): the output is a box of the
// volume (VolDesc then holds the box's dims) and a chunk writes only its samples in [lo, hi) (chunk
// coordinates), at the chunk's origin relative to the box -- negative where the chunk starts before it.
struct CropGeom {          // one entry per chunk of the batch (device array)
  int32_t rel[3];          // chunk origin minus box origin
  uint32_t lo[3], hi[3];   // the chunk's window inside the box, [lo, hi) per axis
};

// the geometry record a writer reads: ChunkGeom, or CropGeom in the crop variant
template <bool kCrop>
using GeomOf = typename std::conditional<kCrop, CropGeom, ChunkGeom>::type;

// ---- per-chunk state, device resident -----------------------------------------------------------
struct PlaneRec {
  uint64_t baseLIP, baseLIS, baseREF;
  uint32_t didSort, didREF;
};

// results of the float stages + what the container needs to know about the chunk
struct CoderState {
  double mean;                   // or the constant value of a constant chunk
  double q;
  double maxabs;                 // max |coefficient| after the DWT (bits compared as uint64)
  uint32_t is_const;             // constant field (src/Conditioner.cpp:28-44)
  uint32_t not_const_flag;       // scratch for the constant test
  uint32_t wide;                 // coefficients are uint64 (high-precision retry / >32 planes)
  uint32_t need_retry;           // fixed-rate stream too short at 32 planes (SPECK_FLT.cpp:530-538)
  int32_t nbp;                   // SPECK header: number of bit planes
  uint32_t mse_active;           // PSNR mode: this chunk's q is still being searched
  // PSNR mode (src/SPECK_FLT.cpp:237-279,431-435): range of the input as order-preserving keys
  // of max(v) and max(-v), and the quantisation error estimate of the current q
  uint64_t vmaxKey, vnegmaxKey;
  double mse;
  uint64_t total_bits;           // SPECK header: bits of the complete stream
  uint64_t stream_len;           // bytes of this chunk's stream (17 or 17 + 9 + payload)
  uint64_t stream_off;           // byte offset of the chunk stream inside the container
};

// encoder internals
struct EncState {
  uint32_t active;               // this chunk takes part in the current encode pass
  int32_t nbp;                   // number of bit planes
  int32_t done;                  // budget reached / all planes coded
  int32_t plast;                 // lowest plane whose sorting pass ran
  uint32_t bornCount;            // newborn insignificant sets of the current plane
  uint32_t cur;                  // which of the two list buffers is current
  uint64_t pos;                  // running bit position
  uint64_t total_bits;
  uint64_t budget;               // rounded up to a multiple of 8, or ~0
  uint64_t lisBits;              // bits of the current LIS phase
  uint32_t iPart, iPad;          // 2D coder: part_level of what is left of the type-I set (0: nothing)
  PlaneRec rec[kMaxPlanes];
  uint64_t lipTot[kMaxPlanes], refTot[kMaxPlanes];
  uint32_t listLen[2][spk::kMaxLevels];
  uint32_t bornTot[spk::kMaxLevels];
  uint32_t bucketCnt[kMaxPlanes];   // sets that split at each plane
  uint32_t bucketOff[kMaxPlanes];
  uint32_t bucketCur[kMaxPlanes];
};

// ---- block-level exclusive scan over kThreads threads ------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    T o = __shfl_up(v, d, 64);
    if (lane >= d)
      v += o;
  }
  return v;
}

// returns the exclusive prefix of `v` over the block; *total receives the block sum.
// `smem` must hold blockDim.x/64 + 1 elements of T.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* smem, T* total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const T inc = wave_inclusive_scan(v);
  __syncthreads();  // protect smem reuse between consecutive calls
  if (lane == 63)
    smem[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (int w = 0; w < nw; w++) {
    const T s = smem[w];
    if (w < wave)
      base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every global load,
// store and atomic the wavefront has in flight (s_waitcnt vmcnt(0)); a kernel whose threads talk
// through LDS while results stream out to memory pays a round trip to HBM / L2 per barrier for that.
#define LDS_ONLY_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// block_exclusive_scan with such barriers
template <typename T>
__device__ __forceinline__ T block_exclusive_scan_lds(T v, T* smem, T* total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const T inc = wave_inclusive_scan(v);
  LDS_ONLY_BARRIER();  // protect smem reuse between consecutive calls
  if (lane == 63)
    smem[wave] = inc;
  LDS_ONLY_BARRIER();
  T base = 0, tot = 0;
  for (int w = 0; w < nw; w++) {
    const T s = smem[w];
    if (w < wave)
      base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

// out[0, len) = in[0, len) with 8-byte stores (and two 8-byte loads per store when the two are
// aligned differently); thread `tid` of `nthreads`.  Up to 7 bytes past in + len are READ (never used):
// the caller's source has that slack (stream words, 256-byte slots).  A copy byte by byte moved a
// chunk stream of 4 MB at 0.2 TB/s.
__device__ __forceinline__ void copy_bytes_wide(uint8_t* out, const uint8_t* in, uint64_t len, uint64_t tid,
                                                uint64_t nthreads)
{
  const uint64_t head = min(len, (uint64_t)((8u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 7u)) & 7u));
  for (uint64_t i = tid; i < head; i += nthreads)
    out[i] = in[i];
  const uint64_t nb = (len - head) / 8;
  const uint8_t* src = in + head;
  uint64_t* dst64 = reinterpret_cast<uint64_t*>(out + head);
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 7u) * 8u;
  const uint64_t* s64 = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(src) & ~(uintptr_t)7);
  if (sh == 0)
    for (uint64_t j = tid; j < nb; j += nthreads)
      dst64[j] = s64[j];
  else
    for (uint64_t j = tid; j < nb; j += nthreads)
      dst64[j] = (s64[j] >> sh) | (s64[j + 1] << (64u - sh));
  for (uint64_t i = head + nb * 8 + tid; i < len; i += nthreads)
    out[i] = in[i];
}

// Tuning knobs whose sweeps are settled (round 5: the workgroup counts of the list kernels, k_lis_hi's table shape, the
// lifting tiles, which experiments of rounds 2-5 stay switched on ...) are constants of the product build -- it reads
// about twenty environment variables instead of fifty -- and environment variables only of the diagnostics build
// (`make -C sperr_amd/csrc diag` -> sperr_amd/libsperr_hip_diag.so, -DSPERR_HIP_DIAG; SPERR_HIP_LIB loads it: the
// sweeps under tools/ use that one).  What selects a code path tests exercise, places the farm's threads or caps memory
// stays an environment variable of both.
inline const char* tune_getenv(const char* name)
{
#ifdef SPERR_HIP_DIAG
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// A look-back wait (one workgroup waiting for the state its predecessor publishes: k_lis_l0 / _l1 / _hi, k_lis_mx) is
// bounded by WALL TIME, not by a spin count: the protocols are deadlock-free (a waiter always waits for a running
// workgroup), so the bound only guards against a device that has stopped making progress -- and a slow predecessor
// (a shared or time-sliced device, a profiler, a debugger) must not turn a valid stream into a decode error, which a
// count of 2^22 polls could.  s_memrealtime counts at 100 MHz whatever the shader clock does.  Callers set
// DecState::error = kErrLookBackTimeout, which the host reports apart from a damaged stream.
constexpr uint64_t kSpinLimitTicks = 60ull * 100000000ull;   // one minute
constexpr uint32_t kErrCorrupt = 1u, kErrLookBackTimeout = 2u;
__device__ __forceinline__ bool spin_expired(uint32_t spins, uint64_t& t0)
{
  if ((spins & 0x3fffu) != 0)
    return false;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t now = __builtin_amdgcn_s_memrealtime();
#else
  const uint64_t now = 0;   // (the host pass only parses this)
#endif
  if (t0 == 0) {
    t0 = now | 1ull;
    return false;
  }
  return now - t0 > kSpinLimitTicks;
}

__device__ __forceinline__ void atomic_or64(uint64_t* p, uint64_t v)
{
  if (v)
    atomicOr(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// OR `nbits` (<= 64) bits of `val` into a zero-initialised LSB-first bit buffer at `pos`,
// dropping everything at or past `limit`.
__device__ __forceinline__ void put_bits(uint64_t* words, uint64_t pos, uint64_t val, int nbits,
                                         uint64_t limit)
{
  if (nbits <= 0 || pos >= limit)
    return;
  if (pos + (uint64_t)nbits > limit) {
    nbits = (int)(limit - pos);
  }
  if (nbits < 64)
    val &= (uint64_t(1) << nbits) - 1;
  const int sh = (int)(pos & 63);
  atomic_or64(words + (pos >> 6), val << sh);
  if (sh && sh + nbits > 64)
    atomic_or64(words + (pos >> 6) + 1, val >> (64 - sh));
}

__device__ __forceinline__ int get_bit(const uint64_t* words, uint64_t pos, uint64_t avail)
{
  return pos < avail ? (int)((words[pos >> 6] >> (pos & 63)) & 1) : 0;
}

}  // namespace sperrhip

#endif
