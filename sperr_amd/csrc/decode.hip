// decode.hip -- the decode call of the HIP engine: container headers on the device, truncation, a call's workspace
// (carve_dec), the decoder's launch loop, the window and level writers; and the decoder's front (decode_request.h).
// Plans and what the encoder shares come from engine.hip through engine_parts.h.
//
// Host logic restated from the reference (file:line):
//   src/SPERR3D_Stream_Tools.cpp:46-105     container header parsing
//   src/SPERR3D_OMP_D.cpp:23-135            decompress driver
#include <chrono>
#include <deque>
#include <thread>

#include "decode_request.h"
#include "engine_parts.h"

namespace sperrhip {

namespace {

// ------------------------------------------------------------------------------------------
// kernels of the container layer
// ------------------------------------------------------------------------------------------
// bytes [srcOff[i], srcOff[i] + len[i]) of every container of a batch, packed at dstOff[i] (the full headers,
// sperrhip_decompress_batch_dev)
__global__ void __launch_bounds__(kThreads)
k_gather_bytes(const uint8_t* src, const uint64_t* srcOff, const uint64_t* len, const uint64_t* dstOff, uint8_t* dst,
               uint32_t n)
{
  for (uint32_t i = blockIdx.y; i < n; i += gridDim.y)
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < len[i]; k += (uint64_t)gridDim.x * blockDim.x)
      dst[dstOff[i] + k] = src[srcOff[i] + k];
}

// first 26 bytes of every chunk stream, gathered for the host
__global__ void k_gather_heads(const uint8_t* container, const uint64_t* offs, const uint64_t* lens,
                               uint8_t* heads, uint32_t nchunks)
{
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks)
    return;
  for (int i = 0; i < 32; i++)
    heads[c * 32 + i] = (i < 26 && (uint64_t)i < lens[c]) ? container[offs[c] + i] : 0;
}

// sperrhip_trunc_dev / sperrhip_trunc_batch_dev: the output of a truncation -- for every container its header, then the
// kept prefix of every chunk stream -- is one run of bytes cut into `n` pieces: piece i is the bytes
// [outOff[i], outOff[i + 1]) of dst and comes from the device address srcAddr[i] (a container's leading bytes and a
// chunk's stream in the source, a rewritten length table in the call's upload).  The work is split by OUTPUT BYTES:
// workgroup b moves the bytes [b kTruncSlice, (b + 1) kTruncSlice) and finds the pieces under them by binary search,
// so 64 streams of 2 MB and 70 000 of 100 bytes load the device alike and the grid has one dimension.  A slice
// under few pieces is copied piece by piece by the whole workgroup, one under many (short streams) wave by wave.
// Pieces of no bytes share their start with the next one and are passed over.  Any alignment on either side
constexpr uint32_t kTruncSlice = 8192;
__global__ void __launch_bounds__(kThreads)
k_trunc_container(uint8_t* dst, const uint64_t* srcAddr, const uint64_t* outOff, uint32_t n, uint64_t total)
{
  const uint64_t lo = (uint64_t)blockIdx.x * kTruncSlice;
  if (lo >= total)
    return;
  const uint64_t hi = min(lo + kTruncSlice, total);
  uint32_t a = 0, e = n;   // outOff[a] <= lo < outOff[e]  (outOff[0] = 0, outOff[n] = total)
  while (e - a > 1) {
    const uint32_t m = a + (e - a) / 2;
    if (outOff[m] <= lo)
      a = m;
    else
      e = m;
  }
  uint32_t f = a, g = n;   // outOff[f] < hi <= outOff[g]: the pieces a .. g - 1 have bytes in the slice
  while (g - f > 1) {
    const uint32_t m = f + (g - f) / 2;
    if (outOff[m] < hi)
      f = m;
    else
      g = m;
  }
  constexpr uint32_t kWaves = kThreads / 64;
  const bool byWave = g - a >= 2 * kWaves;
  const uint32_t first = byWave ? a + (threadIdx.x >> 6) : a, step = byWave ? kWaves : 1u;
  const uint64_t tid = byWave ? (threadIdx.x & 63u) : threadIdx.x, nthr = byWave ? 64u : (uint32_t)kThreads;
  for (uint32_t i = first; i < g; i += step) {
    const uint64_t at = outOff[i], s = max(at, lo), t = min(outOff[i + 1], hi);
    if (t > s)
      copy_bytes_wide(dst + s, reinterpret_cast<const uint8_t*>(srcAddr[i]) + (s - at), t - s, tid, nthr);
  }
}

// ------------------------------------------------------------------------------------------
// decompression
// ------------------------------------------------------------------------------------------
// what a chunk's DecState::error says (common.h): a stream that does not add up, or a look-back wait that ran into
// its wall-time bound -- the second is the device's trouble (shared, stalled), not the container's
void report_dec_error(uint32_t code)
{
  if (code == kErrLookBackTimeout)
    fprintf(stderr, "[sperr_hip] decoder: a look-back wait timed out after %llu s (device shared, paused or stalled?) -- "
                    "the container may be fine\n", (unsigned long long)(kSpinLimitTicks / 100000000ull));
  else
    fprintf(stderr, "[sperr_hip] decoder: a chunk stream does not add up (damaged or truncated container)\n");
}

}  // namespace

int read_container_info(const uint8_t* d_src, size_t src_len, ContainerInfo& ci, hipStream_t st)
{
  std::vector<uint8_t> h(std::min<size_t>(src_len, 20));
  HIP_CHECK(hipMemcpyAsync(h.data(), d_src, h.size(), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  size_t need = 0;
  int r = parse_container_host(h.data(), h.size(), src_len, ci, &need);
  if (r == 1) {
    if (need > src_len)
      return -1;
    h.resize(need);
    HIP_CHECK(hipMemcpyAsync(h.data(), d_src, need, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    r = parse_container_host(h.data(), h.size(), src_len, ci, &need);
  }
  return r == 0 ? 0 : -1;
}

// The headers of the containers of a batch, container v at [offs[v], offs[v + 1]) of d_src: every header's prefix in
// one gather and one read-back, then the full headers of those with more to read in a second, each parsed by
// parse_container_host into ci[v] (offsets relative to the container).  heads: 32 bytes per container, its first 26
// (or fewer) and zeros.  No container base is assumed aligned: the gathers read bytes
int read_headers_at(Engine& E, const uint8_t* d_src, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len,
                    std::vector<ContainerInfo>& ci, std::vector<uint8_t>& heads, hipStream_t st);
static int read_batch_headers(Engine& E, const uint8_t* d_src, const size_t* offs, size_t nvol, std::vector<ContainerInfo>& ci,
                       std::vector<uint8_t>& heads, hipStream_t st)
{
  if (nvol == 0 || nvol > 0xffffffffull)
    return -1;
  std::vector<uint64_t> off(nvol), len(nvol);
  for (size_t v = 0; v < nvol; v++) {
    if (offs[v + 1] < offs[v])
      return -1;
    off[v] = offs[v];
    len[v] = offs[v + 1] - offs[v];
  }
  return read_headers_at(E, d_src, off, len, ci, heads, st);
}

// The same for containers that lie anywhere: container v is the len[v] bytes at d_src + off[v] (the boxes call: d_src
// is the lowest of its containers' addresses)
int read_headers_at(Engine& E, const uint8_t* d_src, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len,
                    std::vector<ContainerInfo>& ci, std::vector<uint8_t>& heads, hipStream_t st)
{
  const size_t nvol = off.size();
  if (nvol == 0 || nvol > 0xffffffffull || len.size() != nvol)
    return -1;
  const uint32_t n = (uint32_t)nvol;
  std::vector<uint64_t> need(nvol, 0), at(nvol + 1, 0);
  const size_t arr = round_up(nvol * 8, 256);
  if (E.misc.ensure(arr * 3 + nvol * 32 + 256))
    return -1;
  uint64_t* d_off = reinterpret_cast<uint64_t*>(E.misc.p);
  uint64_t* d_len = d_off + arr / 8;
  uint64_t* d_at = d_len + arr / 8;
  uint8_t* d_bytes = reinterpret_cast<uint8_t*>(d_at + arr / 8);
  heads.assign(nvol * 32, 0);
  HIP_CHECK(hipMemcpyAsync(d_off, off.data(), nvol * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_len, len.data(), nvol * 8, hipMemcpyHostToDevice, st));
  LAUNCH_K(k_gather_heads, dim3((n + 63) / 64), dim3(64), 0, st, d_src, d_off, d_len, d_bytes, n);
  HIP_CHECK(hipMemcpyAsync(heads.data(), d_bytes, heads.size(), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  ci.assign(nvol, ContainerInfo{});
  for (size_t v = 0; v < nvol; v++) {
    size_t nd = 0;
    const int r = parse_container_host(heads.data() + v * 32, std::min<uint64_t>(len[v], 26), len[v], ci[v], &nd);
    if (r < 0 || (r == 1 && nd > len[v]))
      return -1;
    need[v] = r == 1 ? nd : 0;
    at[v + 1] = at[v] + need[v];
  }
  if (at[nvol]) {   // the chunk-length tables
    if (E.misc.ensure(arr * 3 + round_up(at[nvol], 256) + 256))
      return -1;
    d_off = reinterpret_cast<uint64_t*>(E.misc.p);
    d_len = d_off + arr / 8;
    d_at = d_len + arr / 8;
    d_bytes = reinterpret_cast<uint8_t*>(d_at + arr / 8);
    std::vector<uint8_t> hdr(at[nvol]);
    HIP_CHECK(hipMemcpyAsync(d_off, off.data(), nvol * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_len, need.data(), nvol * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_at, at.data(), nvol * 8, hipMemcpyHostToDevice, st));
    LAUNCH_K(k_gather_bytes, dim3(4, std::min<uint32_t>(n, 65535u)), dim3(kThreads), 0, st, d_src, d_off, d_len, d_at,
             d_bytes, n);
    HIP_CHECK(hipMemcpyAsync(hdr.data(), d_bytes, hdr.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (size_t v = 0; v < nvol; v++) {
      size_t nd = 0;
      if (need[v] && parse_container_host(hdr.data() + at[v], need[v], len[v], ci[v], &nd) != 0)
        return -1;
    }
  }
  return 0;
}

// The containers of a batch (sperrhip_decompress_batch_dev) as one: all of them must describe the same volume.  `all`
// becomes the stacked view, (x, y, nvol z) with every chunk's absolute offset and length; `list` its chunks (each
// container's chunk_volume, z origins shifted by v z)
int read_batch_info(Engine& E, const uint8_t* d_src, const size_t* offs, size_t nvol, ContainerInfo& all,
                    std::vector<std::array<size_t, 6>>& list, hipStream_t st)
{
  std::vector<ContainerInfo> ci;
  std::vector<uint8_t> heads;
  if (read_batch_headers(E, d_src, offs, nvol, ci, heads, st))
    return -1;
  const Dims vol = ci[0].vol;
  for (size_t v = 1; v < nvol; v++)
    if (ci[v].vol != vol)
      return -1;
  if (nvol > 0xffffffffull / vol[2] || ci[0].nvals > SIZE_MAX / 8 / nvol)   // (uint32_t z origins)
    return -1;
  all.vol = {vol[0], vol[1], vol[2] * nvol};
  all.chunk = ci[0].chunk;
  all.nvals = ci[0].nvals * nvol;
  all.off.clear();
  all.len.clear();
  list.clear();
  for (size_t v = 0; v < nvol; v++) {
    const auto per = chunk_volume(ci[v].vol, ci[v].chunk);
    if (per.size() != ci[v].off.size() || list.size() + per.size() > 0xffffffffull)
      return -1;
    for (size_t i = 0; i < per.size(); i++) {
      auto c = per[i];
      c[4] += v * vol[2];
      list.push_back(c);
      all.off.push_back(offs[v] + ci[v].off[i]);
      all.len.push_back(ci[v].len[i]);
    }
  }
  return 0;
}

// sperrhip_trunc_dev / sperrhip_trunc_batch_dev: the containers at [offs[v], offs[v + 1]) of d_src, each as
// hostc::truncate_container writes it, back to back into d_dst.  The host has every length table (read_batch_headers):
// it works out the kept lengths, where every piece of the output comes from and where it goes, writes the new headers
// -- the leading bytes with the portion flag, the table of kept lengths -- and uploads all that; one launch of
// k_trunc_container then moves every byte, the headers' included.  outOffs: nvol + 1 entries
int trunc_impl(Engine& E, const uint8_t* d_src, const size_t* offs, size_t nvol, unsigned pct, uint8_t* d_dst,
               size_t dst_cap, size_t* outOffs, hipStream_t st)
{
  std::vector<ContainerInfo> ci;
  std::vector<uint8_t> heads;
  if (read_batch_headers(E, d_src, offs, nvol, ci, heads, st))
    return -1;
  const bool whole = pct == 0 || pct >= 100;
  size_t npieces = 0, hdrBytes = 0;
  for (const ContainerInfo& c : ci) {
    npieces += 1 + c.len.size();
    hdrBytes += (c.multi ? 20 : 14) + 4 * c.len.size();
  }
  if (npieces >= 0xffffffffull)
    return -1;
  // the upload: the source addresses, the output offsets, then the new headers
  const size_t addrBytes = round_up(npieces * 8, 256), offBytes = round_up((npieces + 1) * 8, 256);
  if (E.misc.ensure(addrBytes + offBytes + hdrBytes + 256))
    return -1;
  uint8_t* d_up = static_cast<uint8_t*>(E.misc.p);
  std::vector<uint8_t> up(addrBytes + offBytes + hdrBytes, 0);
  uint64_t* srcAddr = reinterpret_cast<uint64_t*>(up.data());
  uint64_t* outOff = reinterpret_cast<uint64_t*>(up.data() + addrBytes);
  uint8_t* hdr = up.data() + addrBytes + offBytes;
  size_t k = 0, hat = 0;
  uint64_t out = 0;
  for (size_t v = 0; v < nvol; v++) {
    const ContainerInfo& c = ci[v];
    const size_t pos = c.multi ? 20 : 14, hlen = pos + 4 * c.len.size();
    uint8_t* h = hdr + hat;
    memcpy(h, heads.data() + v * 32, pos);
    if (!whole) {
      h[0] = 0;       // SPERR_VERSION_MAJOR
      h[1] |= 0x80;   // the portion flag (hostc::truncate_container)
    }
    outOffs[v] = (size_t)out;
    srcAddr[k] = reinterpret_cast<uint64_t>(d_up + addrBytes + offBytes + hat);
    outOff[k++] = out;
    out += hlen;
    for (size_t i = 0; i < c.len.size(); i++) {
      const uint32_t keep = (uint32_t)hostc::portion_len((size_t)c.len[i], pct);
      memcpy(h + pos + 4 * i, &keep, 4);
      srcAddr[k] = reinterpret_cast<uint64_t>(d_src + offs[v] + c.off[i]);
      outOff[k++] = out;
      out += keep;
    }
    hat += hlen;
  }
  outOff[k] = out;
  outOffs[nvol] = (size_t)out;
  if (!d_dst || out > dst_cap)
    return 1;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src) + offs[0], s1 = reinterpret_cast<uintptr_t>(d_src) + offs[nvol];
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(d_dst), d1 = d0 + out;
  if (s0 < d1 && d0 < s1)
    return -1;
  const uint64_t nblocks = (out + kTruncSlice - 1) / kTruncSlice;
  if (nblocks > 0x7fffffffull)
    return -1;
  HIP_CHECK(hipMemcpyAsync(d_up, up.data(), up.size(), hipMemcpyHostToDevice, st));
  LAUNCH_K(k_trunc_container, dim3((uint32_t)nblocks), dim3(kThreads), 0, st, d_dst,
           reinterpret_cast<const uint64_t*>(d_up), reinterpret_cast<const uint64_t*>(d_up + addrBytes), (uint32_t)npieces,
           out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));   // (also: `up` may go only once the copy has read it)
  E.prof.collect();
  return 0;
}

namespace {

struct DecBatchBufs {
  DecBuffers db;
  ChunkGeom* geom;
  CropGeom* crop;   // the chunks' windows of a sub-box (null: the whole volume is decoded)
  uint64_t *chunkOff, *chunkLen;
  double* vals;
  size_t valsStride;
  double* vals2;    // a second compact box of the same layout: the fused second level writes it (null: no such launch)
  uint32_t* coef32;
  uint32_t* live;   // chunks that still decode (DecPlanHost::d_live)
};

// valsElems: fp64 samples per chunk of the chunk buffer (0: the whole chunk; compact_box() otherwise)
// refNPlanes: refinement bit planes per chunk (DecBuffers::refPlanes; 0: the coefficients are updated plane by plane)
// crop: a sub-box is decoded (DecBatchBufs::crop)
// box2: the second level runs fused (Batch::level2): a second compact box
bool carve_dec(Arena& A, const ShapePlan& P, uint32_t B, uint64_t maxPayloadBytes, DecBatchBufs& o,
               size_t valsElems = 0, uint32_t refNPlanes = 0, bool crop = false, bool box2 = false)
{
  const size_t N = P.N, Npad = round_up(N, 512);   // (512: k_ref_assemble takes eight mask words per round)
  DecBuffers& d = o.db;
  memset(&d, 0, sizeof(d));
  d.tree = P.dtree;
  d.treeTabLen = (uint32_t)P.ht.tab.size();
  d.nchunks = B;
#define TAKE(dst, T, count)                                                            \
  dst = A.take<T>((size_t)(count));                                                    \
  if (!dst)                                                                            \
    return false;                                                                      \
  if (arena_debug())                                                                   \
    fprintf(stderr, "[sperr_hip] arena %-18s %10.2f MB\n", #dst, (double)((size_t)(count) * sizeof(T)) / 1048576.0);
  TAKE(d.cst, CoderState, B);
  TAKE(d.st, DecState, B);
  TAKE(o.geom, ChunkGeom, B);
  o.crop = nullptr;
  if (crop) {
    TAKE(o.crop, CropGeom, B);
  }
  TAKE(o.chunkOff, uint64_t, B);
  TAKE(o.chunkLen, uint64_t, B);
  TAKE(o.live, uint32_t, 64);
  o.valsStride = valsElems ? round_up(valsElems, 256) : Npad;
  TAKE(o.vals, double, o.valsStride * B);
  o.vals2 = nullptr;
  if (box2 && valsElems) {
    TAKE(o.vals2, double, o.valsStride * B);
  }
  d.coefStride = Npad;
  TAKE(o.coef32, uint32_t, Npad * B);
  d.coef = o.coef32;
  d.signStride = Npad / 64;
  TAKE(d.sign, uint64_t, d.signStride * B);
  d.maskPixStride = Npad / 64;
  d.refPlanes = nullptr;
  d.refMask = nullptr;
  d.wordTop = nullptr;
  d.refNPlanes = 0;
  d.refPlaneStride = d.wordTopStride = 0;
  if (refNPlanes) {
    // (round 6: the planes live in the coefficient array -- 32 plane slots x 8 bytes per mask word = the 64 x 4 bytes
    //  of its coefficients, speck_dec.h; Npad is a multiple of 512: whole tiles of eight mask words)
    d.refNPlanes = std::min<uint32_t>(refNPlanes, 32u);
    d.refPlaneStride = d.coefStride / 2;
    d.wordTopStride = round_up(d.maskPixStride, 64);
    d.refPlanes = reinterpret_cast<uint64_t*>(o.coef32);
    TAKE(d.refMask, uint64_t, d.maskPixStride * B);
    TAKE(d.wordTop, uint8_t, d.wordTopStride * B);
  }
  TAKE(d.bornM, uint64_t, d.maskPixStride * B);
  TAKE(d.sigOld, uint64_t, d.maskPixStride * B);
  TAKE(d.sigNew, uint64_t, d.maskPixStride * B);
  d.lisStride = P.lisEntries;
  TAKE(d.lis[0], uint64_t, P.lisEntries * B);
  TAKE(d.lis[1], uint64_t, P.lisEntries * B);
  d.levelOff = P.d_levelOff;
  d.nPixTiles = (uint32_t)((Npad / 64 + kThreads - 1) / kThreads);   // 256 mask words per tile
  d.tileStride = round_up(d.nPixTiles, 32);
  TAKE(d.tileLip, uint32_t, d.tileStride * B);
  TAKE(d.tileRef, uint32_t, d.tileStride * B);
  TAKE(d.tileLipOff, uint32_t, d.tileStride * B);
  TAKE(d.tileRefOff, uint32_t, d.tileStride * B);
  {
    // (only for the regular trees: there every birth of a sample comes through a leaf event; k_lis_mixed and
    //  k_lis_walk set mask bits themselves)
    uint8_t* tb = nullptr;
    TAKE(tb, uint8_t, d.tileStride * B);
    d.tileBorn = P.dec.tables ? tb : nullptr;
  }
  d.lipResStride = Npad / 64 + 2;
  TAKE(d.lipSig, uint64_t, d.lipResStride * B);
  TAKE(d.lipNeg, uint64_t, d.lipResStride * B);
  d.tokStride = (2 * N + 1 + 63) / 64 + 2;
  TAKE(d.tokMask, uint64_t, d.tokStride * B);
  TAKE(d.tokCnt, uint32_t, d.tokStride * B);
  TAKE(d.tokOff, uint32_t, d.tokStride * B);
  d.tokSegStride = round_up(d.tokStride / 2048 + 2, 32);   // (kLipSeg words a segment, speck_dec.hip)
  TAKE(d.tokSegSum, uint32_t, d.tokSegStride * B);
  TAKE(d.tokSegBase, uint32_t, d.tokSegStride * B);
  d.streamStride = (size_t)(maxPayloadBytes / 8) + 4;
  TAKE(d.stream, uint64_t, d.streamStride * B);
  // table-driven LIS phase
  d.levelClass = P.d_levelClass;
  d.levelSlot = P.d_levelSlot;
  d.slotLevel = P.d_slotLevel;
  d.nSlots = P.nSlots;
  d.maskWords = (uint32_t)d.streamStride;
  d.maskStride = (size_t)P.nSlots * d.maskWords;
  TAKE(d.mask, uint64_t, std::max<size_t>(d.maskStride, 1) * B);
  d.prefWords = (d.maskWords + 3u) / 4u;
  d.prefStride = (size_t)P.nSlots * d.prefWords;
  TAKE(d.maskPrefix, uint32_t, std::max<size_t>(d.prefStride, 1) * B);
  d.bornStride = P.ht.nsets + 8;
  d.hiGroupsMax = kRegionGroups;
  // (a segment that fills up sends the rest to the shared part, which holds the worst case: eight
  //  segments of a twelfth of it each were never seen to fill up at 2 to 4.5 bits per sample; round 6: a
  //  sixteenth -- a set is born once, so a plane's births are a fraction of the sets, and the lists of the three
  //  smallest set sizes, whose kernels claim slots of the shared part, hold most of them: 9.7 MB less per 256^3 chunk)
  d.bornSeg = region_seg_slots(P.ht.nsets);
  d.bornPitch = born_array(d).pitch();
  TAKE(d.bornPacked, uint64_t, d.bornPitch * B);
  TAKE(d.bornPosLev, uint64_t, d.bornPitch * B);
  d.lisStamps = nullptr;
  if (g_lis_stamps_on) {
    TAKE(d.lisStamps, uint64_t, 64 * B);
  }
  d.queueCap = 28672 + 64;
  // k_lis_hi: a pair of queues per workgroup, up to hiGroupsMax workgroups per chunk
  // k_lis_hi keeps tables for the classes of the smallest sets only (2^3 .. 32^3 by default: SPERR_HIP_HI_KCAP);
  // larger sets are walked into bit by bit, which leaves the LDS to longer regions of the stream
  static const int hiKcap = tune_getenv("SPERR_HIP_HI_KCAP") ? std::max(2, atoi(tune_getenv("SPERR_HIP_HI_KCAP"))) : 5;
  d.hiK = (uint32_t)std::min(std::max(2, P.maxK), hiKcap);
  static const uint32_t ahead = tune_getenv("SPERR_HIP_HI_AHEAD") ? (uint32_t)atoi(tune_getenv("SPERR_HIP_HI_AHEAD")) : 512u;   // (round 5, with regions of 6912 positions: eight chunks 38.9 -> 39.7 GB/s, 64 chunks the same)
  d.hiAhead = ahead;
  static const uint32_t extra = tune_getenv("SPERR_HIP_HI_EXTRA") ? (uint32_t)atoi(tune_getenv("SPERR_HIP_HI_EXTRA")) : 1u;
  d.hiExtra = extra;
  d.hiHop2 = 0;   // (no second table, round 5: bench volume decompression 91.5 -> 94.5 GB/s)
  d.hiCand = 1;   // (round 6: 64 chunks decompress at 115.0 against 113.0 GB/s, profiles/r6_hi_candidates_ab.txt)
  d.hiSmemBytes = 148 * 1024;   // (k_lis_hi has 11.5 KB of static LDS)
  d.hiW = hi_window((int)d.hiK, d.hiSmemBytes, d.hiHop2);
  d.queueStride = (size_t)d.queueCap * 4 * d.hiGroupsMax;
  TAKE(d.queue, uint64_t, d.queueStride * B);
  d.hiAhead = std::min(d.hiAhead / 64 * 64, d.hiW / 2);
  d.hiFlagStride = ((d.streamStride * 64 + N) / std::max<uint32_t>(512u, d.hiW - d.hiAhead) + 12) * 4;   // (+ the short first regions of a phase)
  d.mxSlot = P.d_mxSlot;
  d.mxLevelGroup = P.d_mxLevelGroup;
  d.mxS = kMxS;
  d.mxM = kMxM;
  d.mxQ = kMxQ;
  d.mxSmemBytes = mx_smem_bytes(kMxS, kMxM, kMxQ);
  if (P.dec.mixed)   // (k_lis_mx keeps its look-back words in the same array: kMxWordsPerRegion per region of mxS bits)
    d.hiFlagStride = std::max<size_t>(d.hiFlagStride, ((d.streamStride * 64 + N) / kMxS + 4) * kMxWordsPerRegion);
  TAKE(d.hiFlags, unsigned long long, d.hiFlagStride * B);
  d.iRoots = P.d_iRoots;
  d.iLevels = P.ht.iLevels;
  d.leafCap = P.ht.nsets + 8;
  d.leafSeg = region_seg_slots(P.ht.nsets);
  d.leafStride = leaf_array(d).pitch();
  TAKE(d.leafEv, uint64_t, d.leafStride * B);
  d.sigbitsStride = P.lisEntries / 64 + 4;
  TAKE(d.sigbits, uint64_t, d.sigbitsStride * B);
  d.l0FlagStride = (d.streamStride * 64 + N) / 4096 + 4;   // (zero padding may be walked)
  TAKE(d.l0Flags, unsigned long long, d.l0FlagStride * B);
  TAKE(d.l0Tab, unsigned long long, d.l0FlagStride * 17 * B);
  d.l0Level = P.l0Level;
  TAKE(d.l1Flags, unsigned long long, d.l0FlagStride * B);
  d.l1Level = P.l1Level;
  TAKE(d.l2Flags, unsigned long long, d.l0FlagStride * B);
  d.l2Level = P.l2Level;
  d.wordLeaf = P.d_wordLeaf;
  d.leafStateStride = round_up(P.ht.nnodes, 64);
  TAKE(d.leafState, uint16_t, d.leafStateStride * B);
  d.leafDirtyStride = d.leafStateStride / 32 + 1;
  TAKE(d.leafDirty, uint8_t, d.leafDirtyStride * B);
#undef TAKE
  return true;
}

// What a decode call clears of the arrays carve_dec hands out, for nb chunks: once per call ...
int reset_dec_call(const DecBuffers& d, uint32_t nb, hipStream_t ss)
{
  HIP_CHECK(hipMemsetAsync(d.cst, 0, nb * sizeof(CoderState), ss));
  HIP_CHECK(hipMemsetAsync(d.st, 0, nb * sizeof(DecState), ss));
  HIP_CHECK(hipMemsetAsync(d.mask, 0, std::max<size_t>(d.maskStride, 1) * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.l0Flags, 0, d.l0FlagStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.l0Tab, 0, d.l0FlagStride * 17 * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.l1Flags, 0, d.l0FlagStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.l2Flags, 0, d.l0FlagStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.hiFlags, 0, d.hiFlagStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.sigbits, 0, d.sigbitsStride * nb * 8, ss));
  if (d.lisStamps)
    HIP_CHECK(hipMemsetAsync(d.lisStamps, 0, 64 * 8 * nb, ss));
  return 0;
}

// ... and before each width pass (wide: 64-bit magnitudes, which are decoded into the fp64 buffer; else the
// refinement bit planes -- k_ref_assemble writes every coefficient, a plane's words are valid from wordTop down --
// or the 32-bit coefficients)
int reset_dec_pass(const DecBatchBufs& bb, uint32_t nb, bool wide, hipStream_t ss)
{
  const DecBuffers& d = bb.db;
  HIP_CHECK(hipMemsetAsync(d.bornM, 0, d.maskPixStride * nb * 8, ss));
  if (d.tileBorn)
    HIP_CHECK(hipMemsetAsync(d.tileBorn, 0, d.tileStride * nb, ss));
  HIP_CHECK(hipMemsetAsync(d.sigOld, 0, d.maskPixStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.sigNew, 0, d.maskPixStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.sign, 0xff, d.signStride * nb * 8, ss));
  HIP_CHECK(hipMemsetAsync(d.leafState, 0, d.leafStateStride * nb * 2, ss));
  HIP_CHECK(hipMemsetAsync(d.leafDirty, 0, d.leafDirtyStride * nb, ss));
  HIP_CHECK(hipMemsetAsync(d.stream, 0, d.streamStride * nb * 8, ss));
  if (wide)
    HIP_CHECK(hipMemsetAsync(bb.vals, 0, bb.valsStride * nb * 8, ss));
  else if (d.refPlanes)
    HIP_CHECK(hipMemsetAsync(d.wordTop, 0, d.wordTopStride * nb, ss));
  else
    HIP_CHECK(hipMemsetAsync(bb.coef32, 0, d.coefStride * nb * 4, ss));
  return 0;
}

}  // namespace

int multires_levels(const Dims& vol, const Dims& cdim, MultiRes& m)
{
  m.nlev = 0;
  size_t levels = 0;
  for (int a = 0; a < 3; a++)
    if (cdim[a] == 0 || vol[a] % cdim[a] != 0)
      return 0;
  if (!spk::can_use_dyadic({cdim[0], cdim[1], cdim[2]}, levels) || levels > 16)
    return 0;
  for (int a = 0; a < 3; a++)
    m.grid[a] = (uint32_t)(vol[a] / cdim[a]);
  for (size_t lev = levels; lev > 0; lev--)
    for (int a = 0; a < 3; a++)
      m.cres[levels - lev][a] = (uint32_t)spk::approx_detail_len(cdim[a], lev)[0];
  m.nlev = levels;
  return 0;
}

// a slice: one level per level of dwt2d (src/sperr_helper.cpp:86-95, src/CDF97.cpp:114-130)
void multires_levels_2d(size_t dx, size_t dy, MultiRes& m)
{
  const size_t levels = std::min<size_t>(spk::num_of_xforms(std::min(dx, dy)), 16);
  m.grid = {1, 1, 1};
  for (size_t lev = levels; lev > 0; lev--)
    m.cres[levels - lev] = {(uint32_t)spk::approx_detail_len(dx, lev)[0],
                            (uint32_t)spk::approx_detail_len(dy, lev)[0], 1u};
  m.nlev = levels;
}

namespace {

// the approximation corner of every chunk (src/CDF97.cpp:150-168,581-593), mean added back
// (src/SPECK_FLT.cpp:592-603), placed at the chunk's position in the level's volume
__global__ void __launch_bounds__(kThreads)
k_sub_volume(const double* vals, size_t valsStride, const CoderState* cst, const ChunkGeom* geom,
             uint32_t cx, uint32_t cy, uint32_t cdx, uint32_t cdy, uint32_t cdz, uint32_t sx,
             uint32_t sy, uint32_t sz, uint32_t gx, uint32_t gy, double* level)
{
  const uint32_t c = blockIdx.y;
  const CoderState& cs = cst[c];
  const ChunkGeom g = geom[c];
  const uint32_t gi[3] = {g.org[0] / cdx, g.org[1] / cdy, g.org[2] / cdz};
  const size_t ldx = (size_t)sx * gx, ldy = (size_t)sy * gy;
  const double* in = vals + c * valsStride;
  const uint32_t n = sx * sy * sz;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t x = i % sx, r = i / sx;
    const uint32_t y = r % sy, z = r / sy;
    const double v = cs.is_const ? cs.mean : in[((size_t)z * cy + y) * cx + x] + cs.mean;
    level[(((size_t)gi[2] * sz + z) * ldy + (size_t)gi[1] * sy + y) * ldx + (size_t)gi[0] * sx + x] = v;
  }
}

// The window [lo, lo + dims) of `full`, which chunks of `chunk` tile: false when it is empty, leaves `full`, or is too
// long along an axis for a chunk's origin relative to it (CropGeom::rel).  One that is all of `full` crops nothing
bool window_select(const Dims& full, const Dims& chunk, const size_t lo[3], const size_t dims[3], Window& w)
{
  for (int a = 0; a < 3; a++) {
    if (dims[a] > (size_t)INT32_MAX)
      return false;
    w.lo[a] = lo[a];
    w.dims[a] = dims[a];
  }
  w.crop = !(w.lo == Dims{0, 0, 0} && w.dims == full);
  return box_chunks(full, chunk, w.lo, w.dims, w.ids);
}

// The coarsest level's corner: no inverse pass runs before it is read, so nothing has dequantised it (LiftFuse mode 2
// does that as a pass loads).  The samples of the corner box [0, s) of every chunk with 32-bit coefficients, into
// the chunk buffer with rows of bx and slices of by rows; one sample per lane, nothing outside the corner is touched.
// The arithmetic is dequant.h's: dequant_masks, or dequant_signed where k_ref_assemble left the word complete with
// its sign in bit 31
__global__ void __launch_bounds__(kThreads)
k_dequant_corner(double* vals, size_t valsStride, uint32_t bx, uint32_t by, uint32_t cx, uint32_t cy, uint32_t sx,
                 uint32_t sy, uint32_t sz, const CoderState* cst, DequantSrc Q)
{
  const uint32_t c = blockIdx.y;
  const CoderState& cs = cst[c];
  if (cs.is_const || cs.wide)   // (64-bit coefficients: k_inv_quantize has converted the chunk buffer)
    return;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= sx * sy * sz)
    return;
  const uint32_t x = i % sx, r = i / sx;
  const uint32_t y = r % sy, z = r / sy;
  const size_t idx = ((size_t)z * cy + y) * cx + x;
  const DequantRule<uint32_t> rule = dequant_rule<uint32_t>(cs.q, true, Q.dst + c, Q.coefSigned != 0);   // (the decoder's: masks and state are there)
  const uint32_t v = Q.coefs<uint32_t>(c)[idx];
  double out;
  if (rule.scheme)
    out = dequant_signed(rule, v);
  else {
    const uint32_t w = (uint32_t)(idx >> 6), sh = (uint32_t)(idx & 63);
    const uint64_t sgw = Q.sign[c * Q.signStride + w];
    const uint64_t mnw = Q.sigNew[c * Q.maskStride + w], mow = Q.sigOld[c * Q.maskStride + w];
    out = dequant_masks(rule, v, mnw, mow, sgw, sh);
  }
  vals[c * valsStride + ((size_t)z * by + y) * bx + x] = out;
}

// The writer of one level (k_sub_volume's sibling): the corner [0, s) of every chunk, read with the buffer's row
// strides (bx, by), mean added (a constant chunk: the mean alone), narrowed once when OT is float, stored at the
// chunk's place in the level -- or, kCrop, the chunk's window of the box (CropGeom in the level's coordinates; `vd`
// holds the output's dims either way).  One sample per lane, x fastest; a workgroup covers kThreads consecutive
// samples of the corner, whole rows or pieces of one, and returns before it loads when none of its rows is in the window
template <typename OT, bool kCrop>
__global__ void __launch_bounds__(kThreads)
k_level_write(const double* vals, size_t valsStride, const CoderState* cst, const GeomOf<kCrop>* geom, uint32_t bx,
              uint32_t by, uint32_t cdx, uint32_t cdy, uint32_t cdz, uint32_t sx, uint32_t sy, uint32_t sz,
              VolDesc vd, OT* out)
{
  const uint32_t c = blockIdx.y;
  const uint32_t n = sx * sy * sz, i0 = blockIdx.x * kThreads;
  const GeomOf<kCrop> g = geom[c];
  if constexpr (kCrop) {   // (uniform) rows r = z * sy + y of this workgroup: r0 .. r1
    const uint32_t r0 = i0 / sx, r1 = (min(i0 + (uint32_t)kThreads, n) - 1) / sx;
    const uint32_t z0 = r0 / sy, y0 = r0 % sy, z1 = r1 / sy, y1 = r1 % sy;
    auto zin = [&](uint32_t z) { return z >= g.lo[2] && z < g.hi[2]; };
    auto ymeet = [&](uint32_t a, uint32_t b) { return a < g.hi[1] && b >= g.lo[1]; };   // [a, b] meets [lo, hi)
    bool any = zin(z0) && ymeet(y0, z1 > z0 ? sy - 1 : y1);
    any = any || (z1 > z0 && zin(z1) && ymeet(0, y1));
    any = any || (max(z0 + 1, g.lo[2]) < min(z1, g.hi[2]));   // a whole slice in between
    if (!any)
      return;
  }
  const uint32_t i = i0 + threadIdx.x;
  if (i >= n)
    return;
  const uint32_t x = i % sx, r = i / sx;
  const uint32_t y = r % sy, z = r / sy;
  size_t o;
  if constexpr (kCrop) {
    if (x < g.lo[0] || x >= g.hi[0] || y < g.lo[1] || y >= g.hi[1] || z < g.lo[2] || z >= g.hi[2])
      return;
    o = ((size_t)((int64_t)g.rel[2] + z) * vd.dims[1] + (size_t)((int64_t)g.rel[1] + y)) * vd.dims[0] +
        (size_t)((int64_t)g.rel[0] + x);
  }
  else
    o = (((size_t)(g.org[2] / cdz) * sz + z) * vd.dims[1] + (size_t)(g.org[1] / cdy) * sy + y) * vd.dims[0] +
        (size_t)(g.org[0] / cdx) * sx + x;
  const CoderState& cs = cst[c];
  const double v = cs.is_const ? cs.mean : vals[c * valsStride + ((size_t)z * by + y) * bx + x] + cs.mean;
  out[o] = (OT)v;
}

// bytes carve_dec takes for one chunk
size_t dec_bytes_per_chunk(const ShapePlan& P, uint64_t maxPayload, size_t valsElems, uint32_t refNPlanes, bool crop,
                           bool box2 = false)
{
  Arena probe;
  probe.base = reinterpret_cast<char*>(uintptr_t(4096));  // size probe only
  probe.cap = ~size_t(0) / 2;
  DecBatchBufs tmp;
  carve_dec(probe, P, 1, maxPayload, tmp, valsElems, refNPlanes, crop, box2);
  return probe.used;
}

// the list kernels a chunk shape takes: the plan's copy, for the caller to complete with what its call decides
const DecPlanHost& dec_plan_host(const ShapePlan& P) { return P.dec; }

// One decompression call (decompress_impl), stage by stage.  What is decoded and where it goes is `req`'s to say
// (DecodeRequest: its source and its output); no stage asks anything else
template <typename T>
struct DecodeCall {
  struct Ref {
    uint32_t gid;    // container chunk (ci.off / ci.len)
    uint32_t slot;   // this call's slot (heads, outHead)
    uint32_t org[3];
  };
  // PWE streams: a chunk's SPECK stream may be followed by an outlier stream, which counts only
  // when all of it is there (src/SPECK_FLT.cpp:88-103)
  struct OutHead {
    bool has = false;
    uint64_t off = 0, total_bits = 0;
    int nbp = 0;
  };
  // a sub-batch; kept until the call's end: its host arrays are what queued copies read and write
  struct SubHost {
    std::vector<ChunkGeom> hg, bricks;
    std::vector<CropGeom> hc;
    std::vector<uint64_t> ho, hl;
    std::vector<DecState> hs;
    std::vector<OutlierChunk> hoc;   // (the outlier streams' heads)
    DecBatchBufs bb;
    OutlierBufs ob;
    uint32_t nb = 0;
    size_t first = 0;
    int maxNarrow = 0, maxWide = 0;
    bool outliers = false;
  };
  // a batch of a shape group: what the group's sizing decided, and the batch's sub-batches
  struct Batch {
    const std::vector<Ref>* refs;
    ShapePlan* P;
    uint32_t cbox[3], refNPlanes, nsub = 1;
    uint64_t maxPayload = 0;
    size_t compactElems;
    bool level2 = false;   // passes 5, 4 and 3 as one launch into a second compact box (level2_of)
    bool deferG, fuseDq;
    hipStream_t deferStream = nullptr;
    std::vector<SubHost>* subs = nullptr;
    int devId = 0;
  };
  Engine& E;
  const uint8_t* d_src;
  T* d_dst;
  const ContainerInfo& ci;
  hipStream_t st;
  const DecodeRequest& req;
  const VolDesc vd = req.out_desc(ci);
  // The chunks of this call, slot by slot (DecodeRequest::slots).  Heads, outlier heads and batches are per slot;
  // offsets and lengths come from the container.
  std::vector<uint32_t> sel;
  std::vector<uint64_t> selOff, selLen, tailOff, tailLen;
  std::vector<uint8_t> heads, tails;
  std::vector<OutHead> outHead;
  bool anyOutlier = false;
  std::map<Dims, std::vector<Ref>> groups;
  uint32_t mxGroupsCall = 0;
  std::deque<std::vector<SubHost>> subHosts;   // every batch's sub-batches
  // Small groups (the border shapes of a volume that the chunk size does not divide; their chunks
  // decode through the serial walk, one wavefront each) are not waited for one by one: each gets
  // its own piece of the arena and one of the sub-streams, and all of them are drained together.
  bool deferOK = false, deferSized = false, deferForked = false;
  bool arenaCarved = false;   // a batch of this call has carved the arena (decode_batch: the poison fill of the next)
  std::vector<SubHost*> pending;
  size_t deferOff = 0;
  uint32_t deferNext = 0;
  hipEvent_t timingFork = nullptr;
  std::vector<std::pair<hipEvent_t, std::array<uint32_t, 4>>> timingEnds;
  bool ok = false;
  ~DecodeCall() { if (!ok) drain_after_error(E, st); }
  int run(size_t dst_cap_vals)
  {
    if (!req.valid())
      return -1;
    const auto chunks = req.chunks(ci);
    sel = req.slots(chunks.size());
    const uint32_t nchunks = (uint32_t)sel.size();
    const size_t outVals = req.out_vals(ci);
    if (outVals == 0 || outVals > dst_cap_vals || nchunks == 0)
      return -1;
    for (uint32_t i = 0; i < nchunks; i++) {
      const auto& c = chunks[sel[i]];
      selOff.push_back(ci.off[sel[i]]);
      selLen.push_back(ci.len[sel[i]]);
      groups[Dims{c[1], c[3], c[5]}].push_back({sel[i], i, {(uint32_t)c[0], (uint32_t)c[2], (uint32_t)c[4]}});
    }
    if (read_heads())
      return -1;
    deferOK = !anyOutlier && !req.levels && !req.slices && groups.size() > 1;
    count_mx_groups();
    for (int pass = 0; pass < 2; pass++)
      for (auto& g : groups)
        if (decode_group(g.first, g.second, pass))
          return -1;
    if (drain())
      return -1;
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    E.prof.collect();
    ok = true;
    return 0;
  }
  // the chunk heads (flags, number of planes) decide the integer width and the plane count; and the heads of
  // the outlier streams behind them
  int read_heads()
  {
    const uint32_t nchunks = (uint32_t)sel.size();
    if (E.misc.ensure(round_up((size_t)nchunks * 8, 256) * 4 + (size_t)nchunks * 64 + 256))
      return -1;
    uint64_t* d_off = reinterpret_cast<uint64_t*>(E.misc.p);
    uint64_t* d_len = d_off + round_up(nchunks, 32);
    uint64_t* d_hoff = d_len + round_up(nchunks, 32);   // (req.sliceHdr: where each stream's 10-byte header starts)
    uint64_t* d_hlen = d_hoff + round_up(nchunks, 32);
    uint8_t* d_heads = reinterpret_cast<uint8_t*>(d_hlen + round_up(nchunks, 32));
    // (withHdr: a second launch gathers the 10 bytes in front of every stream behind the heads, for the same read-back)
    auto gather = [&](const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, std::vector<uint8_t>& out,
                      bool withHdr) -> int {
      HIP_CHECK(hipMemcpyAsync(d_off, off.data(), nchunks * 8, hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(d_len, len.data(), nchunks * 8, hipMemcpyHostToDevice, st));
      LAUNCH_K(k_gather_heads, dim3((nchunks + 63) / 64), dim3(64), 0, st, d_src, d_off, d_len, d_heads, nchunks);
      std::vector<uint64_t> hoff, hlen;
      if (withHdr) {
        hoff.resize(nchunks);
        hlen.assign(nchunks, 10);
        for (uint32_t i = 0; i < nchunks; i++)
          hoff[i] = off[i] - 10;
        HIP_CHECK(hipMemcpyAsync(d_hoff, hoff.data(), nchunks * 8, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_hlen, hlen.data(), nchunks * 8, hipMemcpyHostToDevice, st));
        LAUNCH_K(k_gather_heads, dim3((nchunks + 63) / 64), dim3(64), 0, st, d_src, d_hoff, d_hlen,
                 d_heads + (size_t)nchunks * 32, nchunks);
      }
      out.resize((size_t)nchunks * (withHdr ? 64 : 32));
      HIP_CHECK(hipMemcpyAsync(out.data(), d_heads, out.size(), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      return 0;
    };
    if (gather(selOff, selLen, heads, req.sliceHdr != nullptr))
      return -1;
    if (const uint32_t* sliceHdr = req.sliceHdr)   // {version, flags, u32 dimx, u32 dimy} of every stream of a slice batch: the dims must be the call's
      for (uint32_t i = 0; i < nchunks; i++) {
        uint32_t d2[2];
        memcpy(d2, heads.data() + (size_t)(nchunks + i) * 32 + 2, 8);
        if (d2[0] != sliceHdr[0] || d2[1] != sliceHdr[1]) {
          fprintf(stderr, "[sperr_hip] slice %u of the batch: its header says %u x %u, the call %u x %u\n", i, d2[0], d2[1],
                  sliceHdr[0], sliceHdr[1]);
          return -1;
        }
      }
    outHead.resize(nchunks);
    tailOff.assign(nchunks, 0);
    tailLen.assign(nchunks, 0);
    bool anyTail = false;
    if (!req.reads_outliers())
      return 0;
    for (uint32_t i = 0; i < nchunks; i++) {
      const uint8_t* hd = heads.data() + (size_t)i * 32;
      if (selLen[i] < 26 || (hd[0] & 0x01))
        continue;
      uint64_t tb;
      memcpy(&tb, hd + 18, 8);
      const uint64_t speckLen = std::min<uint64_t>(9 + bytes_of_bits(tb), selLen[i] - 17);
      if (17 + speckLen + 9 <= selLen[i]) {
        tailOff[i] = selOff[i] + 17 + speckLen;
        tailLen[i] = selLen[i] - 17 - speckLen;
        anyTail = true;
      }
    }
    if (!anyTail)
      return 0;
    if (gather(tailOff, tailLen, tails, false))
      return -1;
    for (uint32_t i = 0; i < nchunks; i++) {
      if (tailLen[i] < 9)
        continue;
      const uint8_t* t = tails.data() + (size_t)i * 32;
      uint64_t ob;
      memcpy(&ob, t + 1, 8);
      if (tailLen[i] != 9 + bytes_of_bits(ob))   // no wrap for ob near 2^64
        continue;
      outHead[i].has = true;
      outHead[i].off = tailOff[i];
      outHead[i].total_bits = ob;
      outHead[i].nbp = t[0];
      anyOutlier = true;
    }
    return 0;
  }
  // Chunks of this call that decode through k_lis_mx, whatever their shape group: they run side by side, each with
  // several one-per-CU workgroups (the rows of a chunk's regions take about four workgroups to keep its serial walk
  // fed), so the groups share one budget of workgroups (SPERR_HIP_MX_WGS; with more workgroups than CUs the chunks
  // launched last wait for the first ones to END: 1000^3 in 256^3 chunks, 37 such chunks at 8 workgroups each,
  // decoded no faster than with one workgroup per chunk)
  // (a slice is decoded on the 2D coder's forest, the plan with z extent 0)
  ShapePlan* plan_of(const Dims& d) { return E.plan(d[0], d[1], req.slices ? 0 : d[2]); }
  void count_mx_groups()
  {
    size_t nmx = 0;
    for (auto& h : groups) {
      ShapePlan* Q = plan_of(h.first);
      if (Q && Q->dec.mixed)
        nmx += h.second.size();
    }
    static const uint32_t mxBudget = getenv("SPERR_HIP_MX_WGS") ? (uint32_t)atoi(getenv("SPERR_HIP_MX_WGS")) : 208u;
    // (calls that share the device -- the chunk farm's workers, several host threads -- share the budget: each of these
    //  workgroups has a CU to itself for as long as its chunk's phase lasts)
    size_t sharers = 1;
    int devNow = 0;
    if (hipGetDevice(&devNow) == hipSuccess)
      sharers = std::max<size_t>(1, g_pool.busy_on(devNow));
    if (nmx)
      mxGroupsCall = std::min<uint32_t>(kRegionGroups, std::max<uint32_t>(2u, (uint32_t)(mxBudget / (nmx * sharers))));
  }
  // (groups of 32 and more chunks of a shape the table kernels take keep the sub-batch scheme)
  static bool deferrable(const ShapePlan& P, size_t nchunksOfShape) { return nchunksOfShape < 32 || !P.dec.tables; }
  // Refinement bit planes (speck_dec.h, DecBuffers::refPlanes): as many as the chunks of a group with 32-bit
  // coefficients have planes (byte 17 of a chunk: src/SPECK_INT.cpp:284-308)
  uint32_t ref_planes_of(const ShapePlan& P, const std::vector<Ref>& refs) const
  {
    uint32_t n = 0;
    for (const Ref& r : refs) {
      const uint8_t* hd = heads.data() + (size_t)r.slot * 32;
      if (ci.len[r.gid] >= 26 && !(hd[0] & 0x01) && hd[17] <= 32)
        n = std::max<uint32_t>(n, hd[17]);
    }
    return n;
  }
  // The fp64 chunk buffer of a group can be COMPACT (round 3): when the finest level runs as the fused
  // x-y-z kernel and every inverse pass dequantises the samples no coarser level produces straight
  // from the integer coefficients, the buffer only ever holds the box of the second level (an eighth
  // of the chunk: 17 MB instead of 134 MB for 256^3).  Not with 64-bit coefficients (they live in the
  // buffer), outlier correctors (every pass stays in the buffer), the resolution hierarchy or slices.
  size_t compact_box(const ShapePlan& P, const std::vector<Ref>& refs, uint32_t cbox[3]) const
  {
    cbox[0] = cbox[1] = cbox[2] = 0;
    if (!P.schedule.brick || req.levels || req.slices || anyOutlier)
      return 0;
    for (const Ref& r : refs) {
      const uint8_t* hd = heads.data() + (size_t)r.slot * 32;
      if (ci.len[r.gid] >= 26 && !(hd[0] & 0x01) && hd[17] > 32)
        return 0;   // a chunk with 64-bit coefficients
    }
    for (int a = 0; a < 3; a++)
      cbox[a] = P.schedule.coarseBox[a];
    if (const Window* lvl = req.level())   // (a chunk with one level of transform has no coarser pass: the box still holds the level's corner)
      for (int a = 0; a < 3; a++)
        cbox[a] = std::max(cbox[a], lvl->m.cres[lvl->h][a]);
    return (size_t)cbox[0] * cbox[1] * cbox[2];
  }
  // The second level of a group runs as one launch (plan_level2) where the group works in the compact box, whose every
  // pass dequantises on the way; a single level's decode (enqueue_level) never reaches that launch
  bool level2_of(const ShapePlan& P, size_t compactElems) const { return P.schedule.level2 && compactElems != 0 && !req.level(); }
  // room for all the small groups at once, if the memory is there
  int size_deferred()
  {
    deferSized = true;
    size_t sum = 0;
    for (auto& h : groups) {
      ShapePlan* Q = E.plan(h.first[0], h.first[1], h.first[2]);
      if (!Q)
        return -1;
      if (!deferrable(*Q, h.second.size()))
        continue;
      uint64_t mp = 0;
      for (auto& r : h.second)
        mp = std::max<uint64_t>(mp, ci.len[r.gid]);
      uint32_t qbox[3];
      const size_t qelems = compact_box(*Q, h.second, qbox);
      sum += round_up(h.second.size() * dec_bytes_per_chunk(*Q, mp, qelems, ref_planes_of(*Q, h.second), req.cropped(), level2_of(*Q, qelems)) + (1 << 20), 4096);
    }
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t room = arena_room(E.arena.n, fr);
    return E.arena.ensure(std::min(sum, room)) ? -1 : 0;
  }
  // a shape group: its plan, buffer layout and batch size, then batch after batch.  Pass 0 decodes the groups that
  // are not deferred, pass 1 the deferred ones
  int decode_group(const Dims& shape, const std::vector<Ref>& refs, int pass)
  {
    // a slice is decoded by the kernels of the 3D decoder on the 2D coder's forest (k_lis_mx and its
    // type-I phase)
    ShapePlan* P = plan_of(shape);
    if (!P)
      return -1;
    if (req.slices && !P->dec.mixed) {   // (no slice has such a forest, DESIGN.md section 4c: k_lis_walk has no type-I phase)
      fprintf(stderr, "[sperr_hip] slice of %u x %u: its forest does not fit k_lis_mx\n", P->dims[0], P->dims[1]);
      return -1;
    }
    Batch b{&refs, P};
    b.deferG = deferOK && deferrable(*P, refs.size());
    if (b.deferG != (pass == 1))
      return 0;
    if (b.deferG && !deferSized && size_deferred())
      return -1;
    for (auto& r : refs)
      b.maxPayload = std::max<uint64_t>(b.maxPayload, ci.len[r.gid]);
    b.compactElems = compact_box(*P, refs, b.cbox);
    b.refNPlanes = ref_planes_of(*P, refs);
    // the inverse passes dequantise on the way (not for the resolution hierarchy, whose coarsest
    // level is read before any pass has run)
    b.fuseDq = P->schedule.fusable && !req.levels && !req.slices;
    b.level2 = level2_of(*P, b.compactElems) && b.fuseDq;
    const size_t per = dec_bytes_per_chunk(*P, b.maxPayload, b.compactElems, b.refNPlanes, req.cropped(), b.level2);
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t budgetBytes = arena_budget(E.arena.n, fr);
    uint32_t B = (uint32_t)std::min<size_t>(refs.size(), std::max<size_t>(1, budgetBytes / per));
    B = std::min<uint32_t>(B, 256);
    const size_t needBytes = (size_t)B * per + (1 << 20);
    if (b.deferG && deferOff + needBytes > E.arena.n && drain())   // no room beside the groups in flight
      return -1;
    if (E.arena.ensure(needBytes))   // (grows only when nothing is in flight: deferOff == 0 here)
      return -1;
    for (size_t b0 = 0; b0 < refs.size(); b0 += B) {
      const uint32_t nbAll = (uint32_t)std::min<size_t>(B, refs.size() - b0);
      if (b.deferG && deferOff + needBytes > E.arena.n && drain())
        return -1;
      if (decode_batch(b, b0, nbAll, needBytes))
        return -1;
    }
    return 0;
  }
  int decode_batch(Batch& b, size_t b0, uint32_t nbAll, size_t needBytes)
  {
    Arena A;
    A.base = static_cast<char*>(E.arena.p) + (b.deferG ? deferOff : 0);
    A.cap = E.arena.n - (b.deferG ? deferOff : 0);
    b.deferStream = nullptr;
    // A batch at the arena's start lies over what the call carved before, and nothing of that is in flight: a batch that
    // is not deferred ends in a wait (collect_states), the deferred ones have been drained.  Under the poison switch
    // the arena is filled again on the caller's stream, which the sub-streams are forked from (again, below).  Deferred
    // groups further in lie beside groups in flight, over memory that fill has covered
    if (!b.deferG || deferOff == 0) {
      bool filled = false;
      if (arenaCarved && E.poison_arena(st, &filled))
        return -1;
      if (filled)
        deferForked = false;
      arenaCarved = true;
    }
    if (b.deferG) {
      if (!deferForked) {   // the sub-streams start behind what the caller's stream holds
        HIP_CHECK(hipEventRecord(E.evFork, st));
        for (uint32_t q = 0; q < kSubStreams; q++)
          HIP_CHECK(hipStreamWaitEvent(E.sub[q], E.evFork, 0));
        HIP_CHECK(hipStreamWaitEvent(E.outlQ[1], E.evFork, 0));
        deferForked = true;
      }
      // (a group of regular chunks beside groups that decode through k_lis_mx: those hold most CUs for the whole
      //  call with workgroups that mostly wait for their turn on a chunk's serial walk, and eight groups on the
      //  eight normal-priority hardware queues -- one of which the caller's stream has -- put two groups on one
      //  queue, one behind the other.  The regular chunks take the 1D decoder's idle high-priority stream: a queue
      //  pool of its own, 1000^3 in 256^3 chunks 178 -> see DESIGN.md section 9)
      b.deferStream = (mxGroupsCall != 0 && b.P->dec.tables) ? E.outlQ[1] : E.sub[deferNext++ % kSubStreams];
      deferOff += round_up(needBytes, 4096);
    }
    if (pick_sub_batches(b, A, b0, nbAll))
      return -1;
    std::vector<SubHost>& subs = *b.subs;
    if (b.nsub == 1) {
      static const bool enqTiming = getenv("SPERR_HIP_ENQ_TIMING") != nullptr;
      const auto tq0 = std::chrono::steady_clock::now();
      if (enqueue(b, 0))
        return -1;
      if (enqTiming) {
        fprintf(stderr, "[sperr_hip] group %u x %u x %u, %u chunks: enqueued in %.2f ms\n", b.P->dims[0], b.P->dims[1], b.P->dims[2], nbAll,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq0).count());
        // (diagnostics: when the group's stream is through, measured from the caller's stream at the fork)
        hipEvent_t evEnd = nullptr;
        if (b.deferStream && hipEventCreate(&evEnd) == hipSuccess) {
          if (!timingFork && hipEventCreate(&timingFork) == hipSuccess)
            (void)hipEventRecord(timingFork, st);
          (void)hipEventRecord(evEnd, b.deferStream);
          timingEnds.push_back({evEnd, {b.P->dims[0], b.P->dims[1], b.P->dims[2], nbAll}});
        }
      }
      if (b.deferG) {   // waited for in drain()
        pending.push_back(&subs[0]);
        return 0;
      }
    }
    else {
      // one host thread per sub-batch: one thread would start the last sub-batch only after launching all kernels
      // of the others (about 1300 launches each).  By itself no gain on MI355X, but a thread of its own may wait for
      // its stream, which lets the launcher stop at the plane where the chunks run out of bits (DecPlanHost::d_live)
      std::vector<int> rc(b.nsub, 0);
      std::vector<std::thread> workers;
      for (uint32_t q = 0; q < b.nsub; q++)
        workers.emplace_back([&, q]() { rc[q] = enqueue(b, q); });
      for (auto& w : workers)
        w.join();
      for (uint32_t q = 0; q < b.nsub; q++) {
        if (rc[q])
          return -1;
        if (subs[q].nb)
          HIP_CHECK(hipStreamWaitEvent(st, E.evJoin[q], 0));
      }
    }
    return collect_states(b);
  }
  // The LIS phase of a plane keeps one latency-bound workgroup per chunk busy; sub-batches on
  // separate streams let the bandwidth-bound kernels of one sub-batch run beside the LIS
  // kernels of another.  Measured on MI355X, 64 chunks of 256^3, decompression only: 1 stream
  // 60.4 ms, 2 streams 58.0 ms, 3 streams 57.9 ms (round 1, with one workgroup per chunk in the
  // LIS phase of the larger sets: 1 stream 74 ms, 3 streams 65 ms).
  // SPERR_HIP_SUBSTREAMS=n overrides the choice (1 = a single stream).
  int pick_sub_batches(Batch& b, Arena& A, size_t b0, uint32_t nbAll)
  {
    static const int subEnv = getenv("SPERR_HIP_SUBSTREAMS") ? atoi(getenv("SPERR_HIP_SUBSTREAMS")) : 0;
    uint32_t nsub = nbAll >= 32 ? 2u : 1u;
    // A call that has the device to itself cuts a smaller batch finer (round 3): the chunks' serial
    // chains bound it, and four sub-batches side by side decode 8 chunks in 14.4 ms instead of 16.5,
    // 27 chunks in 26.7 instead of 30.1 (64 chunks: two 85.0, three 83.3, four 82.1 GB/s).  Not when
    // other calls run on the device (the chunk farm's workers: their items already overlap, and
    // sub-batches on top took its decompression from 40 to 26 GB/s).
    int devNow = 0;
    if (!t_shared_device && hipGetDevice(&devNow) == hipSuccess && g_pool.busy_on(devNow) <= 1)
      nsub = nbAll >= 56 ? 3u : nbAll >= 8 ? 4u : nbAll >= 4 ? 2u : 1u;   // (round 6: three from 56 chunks on -- with this round's
                                                                           //  shorter k_lis_hi 64 chunks decode at 117.0 GB/s
                                                                           //  against 115.5 with two, 110.4 with four)
    if (subEnv > 0)
      nsub = std::min<uint32_t>(kSubStreams, (uint32_t)subEnv);
    if (nbAll < 2 * nsub || b.deferG)   // (eight sub-batches of one chunk each: 29.5 ms for 8 chunks against 14.1 with four)
      nsub = 1;
    b.nsub = nsub;
    b.subs = &subHosts.emplace_back(nsub);
    if (nsub > 1) {
      HIP_CHECK(hipEventRecord(E.evFork, st));
      for (uint32_t q = 0; q < nsub; q++)
        HIP_CHECK(hipStreamWaitEvent(E.sub[q], E.evFork, 0));
    }
    uint32_t done = 0;
    for (uint32_t q = 0; q < nsub; q++) {
      SubHost& S = (*b.subs)[q];
      S.nb = (nbAll - done + (nsub - q) - 1) / (nsub - q);
      S.first = b0 + done;
      done += S.nb;
      if (S.nb && !carve_dec(A, *b.P, S.nb, b.maxPayload, S.bb, b.compactElems, b.refNPlanes, req.cropped(), b.level2))
        return -1;
      if (S.nb && b.compactElems)
        g_dbg_counter[2]++;
    }
    HIP_CHECK(hipGetDevice(&b.devId));
    return 0;
  }
  // everything one sub-batch enqueues on its stream (with several sub-batches: from a host thread of its own)
  int enqueue(const Batch& b, uint32_t q)
  {
    SubHost& S = (*b.subs)[q];
    const uint32_t nb = S.nb;
    if (nb == 0)
      return 0;
    if (b.nsub > 1) {
      HIP_CHECK(hipSetDevice(b.devId));
      t_prof = &E.prof;   // (this may be a thread of its own)
    }
    const hipStream_t ss = b.deferStream ? b.deferStream : (b.nsub > 1 ? E.sub[q] : st);
    S.hg.resize(nb);
    S.ho.resize(nb);
    S.hl.resize(nb);
    for (uint32_t i = 0; i < nb; i++) {
      const Ref& r = (*b.refs)[S.first + i];
      for (int a = 0; a < 3; a++)
        S.hg[i].org[a] = r.org[a];
      S.ho[i] = ci.off[r.gid];
      S.hl[i] = ci.len[r.gid];
      const uint8_t* hd = heads.data() + (size_t)r.slot * 32;
      if (S.hl[i] >= 26 && !(hd[0] & 0x01)) {
        const int nbp = hd[17];
        if (nbp > 32)
          S.maxWide = std::max(S.maxWide, nbp);
        else
          S.maxNarrow = std::max(S.maxNarrow, nbp);
      }
      S.outliers |= outHead[r.slot].has;
    }
    if (S.maxWide > kMaxPlanes || (b.compactElems && S.maxWide))
      return -1;
    if (enqueue_outlier_decode(b, S, q, ss) || enqueue_lists(b, S, q, ss) || enqueue_inverse(b, S, q, ss))
      return -1;
    if (b.nsub > 1)
      HIP_CHECK(hipEventRecord(E.evJoin[q], ss));
    return 0;
  }
  // Outlier streams (point-wise error mode) are decoded by the 1D coder on a stream of its own,
  // beside everything below: it needs the container only; the correctors are added at the end
  int enqueue_outlier_decode(const Batch& b, SubHost& S, uint32_t q, hipStream_t ss)
  {
    if (!S.outliers)
      return 0;
    const uint32_t nb = S.nb, N = b.P->N;
    hipStream_t so = E.outlQ[q];
    HIP_CHECK(hipEventRecord(E.evOutlFork[q], ss));
    HIP_CHECK(hipStreamWaitEvent(so, E.evOutlFork[q], 0));
    S.hoc.assign(nb, OutlierChunk{});
    memset(S.hoc.data(), 0, nb * sizeof(OutlierChunk));
    uint64_t maxBits = 0;
    int maxNbp = 1;
    for (uint32_t i = 0; i < nb; i++) {
      const OutHead& oh = outHead[(*b.refs)[S.first + i].slot];
      if (!oh.has)
        continue;
      S.hoc[i].has = 1;
      S.hoc[i].streamOff = oh.off;
      S.hoc[i].total_bits = oh.total_bits;
      S.hoc[i].nbp = oh.nbp;
      if (oh.nbp > kMaxPlanes)
        return -1;
      maxBits = std::max(maxBits, oh.total_bits);
      maxNbp = std::max(maxNbp, oh.nbp);
    }
    OutlierBufs& ob = S.ob;
    memset(&ob, 0, sizeof(ob));
    ob.nchunks = nb;
    ob.N = N;
    ob.nw = (N + 63) / 64;
    ob.wordStride = round_up((size_t)ob.nw + 2, 32);
    // every value found costs at least its sign bit, every run kept on a list its test bit
    ob.kStride = round_up((size_t)std::min<uint64_t>(N, maxBits) + 1, 64);
    speck1d_level_offsets(ob, N, std::min<uint64_t>(maxBits + 2, 2ull * N));
    ob.streamStride = (size_t)(maxBits / 64) + 4;
    ob.planeStride = (size_t)maxNbp * ob.wordStride;
    const size_t bytes = round_up(nb * sizeof(OutlierChunk), 256) +
                         (size_t)nb * (ob.wordStride * 16 + ob.kStride * 5 + ob.runStride * 8 +
                                       ob.streamStride * 8 + ob.planeStride * 8) + 8192;
    if (E.outlDec[q].ensure(bytes))   // (its own buffer: the sub-batches are enqueued by separate threads)
      return -1;
    Arena OA;
    OA.base = static_cast<char*>(E.outlDec[q].p);
    OA.cap = E.outlDec[q].n;
    ob.oc = OA.take<OutlierChunk>(nb);
    ob.lip = OA.take<uint64_t>(nb * ob.wordStride);
    ob.lsp = OA.take<uint64_t>(nb * ob.wordStride);
    ob.runs = OA.take<uint64_t>(nb * ob.runStride);
    ob.stream = OA.take<uint64_t>(nb * ob.streamStride);
    ob.planeBits = OA.take<uint64_t>(nb * ob.planeStride);
    ob.pos = OA.take<uint32_t>(nb * ob.kStride);
    ob.sgn = OA.take<uint8_t>(nb * ob.kStride);
    if (!ob.oc || !ob.lip || !ob.lsp || !ob.runs || !ob.stream || !ob.planeBits || !ob.pos || !ob.sgn)
      return -1;
    HIP_CHECK(hipMemcpyAsync(ob.oc, S.hoc.data(), nb * sizeof(OutlierChunk), hipMemcpyHostToDevice, so));
    HIP_CHECK(hipMemsetAsync(ob.lip, 0, (size_t)nb * ob.wordStride * 16, so));   // lip + lsp
    if (launch_speck1d_decode(so, ob, d_src))
      return -1;
    HIP_CHECK(hipEventRecord(E.evOutl[q], so));
    return 0;
  }
  // the chunks' geometry, then the list phase of every plane: 64-bit chunks first, their magnitudes are decoded
  // into (and converted inside) the fp64 buffer, which the 32-bit pass then fills for the remaining chunks
  int enqueue_lists(const Batch& b, SubHost& S, uint32_t q, hipStream_t ss)
  {
    const ShapePlan& P = *b.P;
    const uint32_t nb = S.nb;
    DecBatchBufs& bb = S.bb;
    DecBuffers& d = bb.db;
    HIP_CHECK(hipMemcpyAsync(bb.geom, S.hg.data(), nb * sizeof(ChunkGeom), hipMemcpyHostToDevice, ss));
    if (req.cropped()) {   // each chunk's piece of the window and its origin relative to the window
      S.hc.resize(nb);
      for (uint32_t i = 0; i < nb; i++)
        S.hc[i] = req.window->geom_of((*b.refs)[S.first + i].slot, S.hg[i].org, P.dims);
      HIP_CHECK(hipMemcpyAsync(bb.crop, S.hc.data(), nb * sizeof(CropGeom), hipMemcpyHostToDevice, ss));
    }
    HIP_CHECK(hipMemcpyAsync(bb.chunkOff, S.ho.data(), nb * 8, hipMemcpyHostToDevice, ss));
    HIP_CHECK(hipMemcpyAsync(bb.chunkLen, S.hl.data(), nb * 8, hipMemcpyHostToDevice, ss));
    DecPlanHost ph = dec_plan_host(P);
    ph.skipFinish = true;   // launch_inv_quantize / the dequantising inverse passes complete the coefficients
    ph.mxGroups = mxGroupsCall;
    if (!ph.tables && !ph.mixed) {
      // (a tree neither the table kernels nor k_lis_mx take -- more than 288 / 352 grids or 48 roots: chunks of
      //  2^30 samples and more -- decodes correctly, through one serial wavefront per chunk: say so, once)
      static std::atomic<bool> warned{false};
      if (!warned.exchange(true))
        fprintf(stderr, "[sperr_hip] note: chunks of %u x %u x %u decode through the serial walk (k_lis_walk): their tree "
                        "(%zu grids, %zu roots) exceeds what the parallel list kernels hold in LDS -- expect it to be slow\n",
                b.P->dims[0], b.P->dims[1], b.P->dims[2], P.ht.grids.size(), P.ht.roots.size());
    }
    static const uint32_t gdivEnv = tune_getenv("SPERR_HIP_MX_GRID_DIV") ? (uint32_t)atoi(tune_getenv("SPERR_HIP_MX_GRID_DIV")) : 4u;
    ph.gridDiv = (b.deferStream && mxGroupsCall != 0 && groups.size() >= 4) ? std::max<uint32_t>(1u, gdivEnv) : 1u;
    // (the host thread may wait for this stream: it is the call's only one, or has a thread of its own)
    ph.d_live = !b.deferStream ? bb.live : nullptr;
    ph.h_live = E.liveHost[q % kSubStreams];
    ph.liveEv = E.liveEv[q % kSubStreams];
    // diagnostics: SPERR_HIP_LIS_GPUWIDE=0 leaves every list to k_lis_hi
    static const bool gpuWide = !(getenv("SPERR_HIP_LIS_GPUWIDE") && atoi(getenv("SPERR_HIP_LIS_GPUWIDE")) == 0);
    if (!gpuWide)
      ph.l0 = ph.l1 = ph.l2 = false;
    if (reset_dec_call(d, nb, ss))
      return -1;
    for (int wide = 1; wide >= 0; wide--) {
      if (wide && S.maxWide == 0)
        continue;
      if (reset_dec_pass(bb, nb, wide != 0, ss))
        return -1;
      DecBuffers dw = d;
      if (wide) {  // 64-bit magnitudes live in the fp64 buffer, converted in place afterwards
        dw.coef = bb.vals;
        dw.coefStride = bb.valsStride;
        dw.refPlanes = nullptr;
      }
      else   // (read by the dequantising inverse passes only: DequantSrc::coefSigned)
        dw.coefSigned = packed_signs(b, bb, false) ? 1u : 0u;
      // the header kernel must run even when no plane does (constant / all-zero chunks)
      if (launch_speck_decode(ss, dw, ph, d_src, bb.chunkOff, bb.chunkLen, wide != 0, wide ? S.maxWide : S.maxNarrow))
        return -1;
      // (32-bit coefficients are dequantised by the inverse passes as they load them, LiftFuse)
      if ((wide || !b.fuseDq) &&
          launch_inv_quantize(ss, wide != 0, dequant_src(b, bb, wide != 0), nb, P.N, bb.vals, bb.valsStride, d.cst))
        return -1;
    }
    return 0;
  }
  // Where the decoder left a sub-batch's coefficients, with the masks and the state that complete them.  wide: the
  // 64-bit ones, which live in the fp64 buffer and are converted in place.  The 32-bit words carry their sign exactly
  // where enqueue_lists asked k_ref_assemble for it (DecBuffers::coefSigned)
  DequantSrc dequant_src(const Batch& b, const DecBatchBufs& bb, bool wide) const
  {
    const DecBuffers& d = bb.db;
    DequantSrc s;
    s.coef = wide ? static_cast<const void*>(bb.vals) : bb.coef32;
    s.coefStride = wide ? bb.valsStride : d.coefStride;
    s.sign = d.sign;
    s.signStride = d.signStride;
    s.sigNew = d.sigNew;
    s.sigOld = d.sigOld;
    s.maskStride = d.maskPixStride;
    s.dst = d.st;
    s.coefSigned = packed_signs(b, bb, wide) ? 1 : 0;
    return s;
  }
  static bool packed_signs(const Batch& b, const DecBatchBufs& bb, bool wide) { return !wide && bb.db.refPlanes && b.fuseDq; }
  // LiftFuse of inverse pass k: the pass dequantises the samples no coarser level produces as it loads them, where
  // the group allows it, and works in the compact buffer where the group has one
  void pass_dequant(const Batch& b, const DecBatchBufs& bb, size_t k, LiftFuse& lf) const
  {
    if (b.fuseDq && pass_fuse(*b.P, k, lf.inner) > 0) {
      lf.mode = 2;
      lf.src = dequant_src(b, bb, false);
    }
    if (b.compactElems) {
      lf.bufx = b.cbox[0];
      lf.bufy = b.cbox[1];
    }
  }
  // The inverse transform.  Its last pass covers the whole chunk: it adds the mean, narrows and scatters --
  // unless outlier correctors have to be added to the transformed values first (src/SPECK_FLT.cpp:573-590), in
  // which case every pass stays in the chunk buffer
  int enqueue_inverse(const Batch& b, SubHost& S, uint32_t q, hipStream_t ss)
  {
    if (const Window* lvl = req.level())
      return enqueue_level(b, S, ss, *lvl);
    const ShapePlan& P = *b.P;
    const uint32_t nb = S.nb;
    const uint32_t* cd = P.dims;
    DecBatchBufs& bb = S.bb;
    DecBuffers& d = bb.db;
    const int io = std::is_same<T, float>::value ? 1 : 2;
    // The inverse walk: the per-axis passes from the coarsest down to where the fused launches take over, then the
    // second level as one launch where the batch has it, then the head.
    // With outlier correctors the transformed values have to stay doubles a little longer, so no head writes the
    // volume -- but they can still come from the fused kernels: the brick inverse, where the group dequantises on the
    // way, has 32-bit coefficients only and no compact buffer.  The correctors and the scatter pass follow either way
    const bool fbrick = S.outliers && b.fuseDq && S.maxWide == 0 && b.compactElems == 0 &&
                        brick_inverse_fits(P, nb, bb.valsStride);
    const LiftSchedule::Head head = S.outliers ? LiftSchedule::kNoHead : P.schedule.head;
    const bool fxyz = head == LiftSchedule::kHeadXYZ, fxy = head == LiftSchedule::kHeadXY;
    // a level of the inverse transform is 3 passes (z y x) of a dyadic chunk, 2 (y x) of a slice
    const size_t perLevel = req.slices ? 2 : 3;
    auto sub_volume = [&](size_t k) -> int {   // before pass k, the first of its level
      const MultiRes* mr = req.levels;
      if (!mr || !mr->nlev)
        return 0;
      const size_t h = mr->nlev - (k / perLevel + 1);
      const auto& r = mr->cres[h];
      const uint32_t blocks = capped_blocks((r[0] * r[1] * r[2] + kThreads - 1) / kThreads, nb);
      LAUNCH_K(k_sub_volume, dim3(blocks, nb), dim3(kThreads), 0, ss, bb.vals, bb.valsStride, d.cst, bb.geom,
               cd[0], cd[1], cd[0], cd[1], cd[2], r[0], r[1], r[2], mr->grid[0], mr->grid[1], mr->d_level[h]);
      return 0;
    };
    // (the second level fused: its three passes are one launch from the compact box into a second one, which the
    //  finest level then reads -- in place a tile's outputs would land in rows other tiles still read)
    const bool l2 = b.level2 && fxyz && bb.vals2 != nullptr;
    if (fbrick) {   // every pass, into the chunk buffer, as doubles
      if (enqueue_brick_inverse(ss, P, E.decBox[q], S.bricks, nb, bb.vals, bb.valsStride, d.cst, bb.geom,
                                dequant_src(b, bb, false)))
        return -1;
    }
    else
      for (size_t k = P.fwd.size(); k-- > LiftSchedule::fused_passes(head, l2);) {
        const LiftPass& ps = P.fwd[k];
        if (k % perLevel == perLevel - 1 && sub_volume(k))
          return -1;
        LiftFuse lf;
        pass_dequant(b, bb, k, lf);
        const bool last = k == 0 && !S.outliers;   // (the pass that writes the volume / the box)
        if (launch_lift(ss, false, bb.vals, bb.valsStride, nb, cd, ps.axis, ps.region, d.cst, last ? io : 0, d_dst, vd,
                        bb.geom, &lf, last ? bb.crop : nullptr))
          return -1;
      }
    if (fxyz) {   // the finest level: z, y and x pass in one kernel, into the volume
      if (sub_volume(2))
        return -1;
      if (l2) {
        LiftFuse l5;
        pass_dequant(b, bb, 5, l5);
        if (launch_lift2_inv(ss, bb.vals, bb.valsStride, bb.vals2, bb.valsStride, nb, cd, P.fwd[3].region, d.cst, &l5))
          return -1;
      }
      LiftFuse lf;
      pass_dequant(b, bb, 2, lf);
      if (launch_lift_xyz(ss, false, l2 ? bb.vals2 : bb.vals, bb.valsStride, nb, cd, d.cst, io, d_dst, vd, bb.geom, &lf, bb.crop))
        return -1;
    }
    if (fxy && req.slices && sub_volume(1))   // the finest level of a slice is the fused pair
      return -1;
    if (fxy && launch_lift_xy(ss, false, bb.vals, bb.valsStride, nb, cd, d.cst, io, d_dst, vd, bb.geom, bb.crop))
      return -1;
    if (S.outliers) {   // the correctors of the values the 1D decoder found meanwhile
      HIP_CHECK(hipStreamWaitEvent(ss, E.evOutl[q], 0));
      if (launch_outlier_apply(ss, S.ob, d.cst, bb.vals, bb.valsStride))
        return -1;
      HIP_CHECK(hipMemcpyAsync(S.hoc.data(), S.ob.oc, nb * sizeof(OutlierChunk), hipMemcpyDeviceToHost, ss));
      HIP_CHECK(hipStreamSynchronize(ss));
      for (auto& o : S.hoc)
        if (o.error) {
          fprintf(stderr, "[sperr_hip] outlier decoder failed (code %u)\n", o.error);
          return -1;
        }
    }
    if ((P.fwd.empty() || S.outliers) &&
        launch_scatter<T>(ss, d_dst, vd, bb.geom, nb, cd, bb.vals, bb.valsStride, d.cst, bb.crop))
      return -1;
    return 0;
  }
  // One level alone: the passes of the levels coarser than it, in the compact buffer or the chunk buffer as the group
  // has it (compact_box, fuseDq), then the writer.  The coarsest level has no pass: its corner is dequantised by a
  // kernel of its own where the passes would have (chunks with 64-bit coefficients: k_inv_quantize has).  The finest
  // level's kernels and the scatter pass are never reached
  int enqueue_level(const Batch& b, SubHost& S, hipStream_t ss, const Window& lvl)
  {
    const ShapePlan& P = *b.P;
    const uint32_t nb = S.nb;
    const uint32_t* cd = P.dims;
    DecBatchBufs& bb = S.bb;
    DecBuffers& d = bb.db;
    const size_t h = lvl.h, nlev = lvl.m.nlev;
    if (P.fwd.size() != 3 * nlev)   // (a level of the transform is the three passes z y x of a dyadic chunk)
      return -1;
    const uint32_t bx = b.compactElems ? b.cbox[0] : cd[0], by = b.compactElems ? b.cbox[1] : cd[1];
    const auto& r = lvl.m.cres[h];
    if (b.compactElems && (r[0] > b.cbox[0] || r[1] > b.cbox[1] || r[2] > b.cbox[2]))
      return -1;
    for (size_t k = P.fwd.size(); k-- > 3 * (nlev - h);) {
      const LiftPass& ps = P.fwd[k];
      LiftFuse lf;
      pass_dequant(b, bb, k, lf);
      if (launch_lift(ss, false, bb.vals, bb.valsStride, nb, cd, ps.axis, ps.region, d.cst, 0, d_dst, vd, bb.geom, &lf))
        return -1;
    }
    const uint32_t blocks = (r[0] * r[1] * r[2] + kThreads - 1) / kThreads;
    if (h == 0 && b.fuseDq)
      LAUNCH_K(k_dequant_corner, dim3(blocks, nb), dim3(kThreads), 0, ss, bb.vals, bb.valsStride, bx, by, cd[0], cd[1],
               r[0], r[1], r[2], d.cst, dequant_src(b, bb, false));
    if (lvl.crop)
      LAUNCH_K((k_level_write<T, true>), dim3(blocks, nb), dim3(kThreads), 0, ss, bb.vals, bb.valsStride, d.cst, bb.crop,
               bx, by, cd[0], cd[1], cd[2], r[0], r[1], r[2], vd, d_dst);
    else
      LAUNCH_K((k_level_write<T, false>), dim3(blocks, nb), dim3(kThreads), 0, ss, bb.vals, bb.valsStride, d.cst, bb.geom,
               bx, by, cd[0], cd[1], cd[2], r[0], r[1], r[2], vd, d_dst);
    HIP_CHECK(hipGetLastError());
    return 0;
  }
  // read-backs only after every sub-batch is enqueued: a device-to-host copy into pageable
  // memory blocks the host until its stream has drained
  int collect_states(const Batch& b)
  {
    for (uint32_t q = 0; q < b.nsub; q++) {
      SubHost& S = (*b.subs)[q];
      if (S.nb == 0)
        continue;
      hipStream_t ss = b.nsub > 1 ? E.sub[q] : st;
      if (S.bb.db.lisStamps && q == 0) {
        g_lis_stamps_host.assign(64, 0);
        // (SPERR_HIP_STAMP_CHUNK=i: the counters of the batch's i-th chunk instead of the first)
        const uint32_t sc = getenv("SPERR_HIP_STAMP_CHUNK")
                                ? std::min<uint32_t>(S.nb - 1, (uint32_t)atoi(getenv("SPERR_HIP_STAMP_CHUNK")))
                                : 0u;
        HIP_CHECK(hipMemcpyAsync(g_lis_stamps_host.data(), S.bb.db.lisStamps + (size_t)sc * 64, 64 * 8,
                                 hipMemcpyDeviceToHost, ss));
      }
      S.hs.resize(S.nb);   // stream errors (wrong lengths) surface here
      HIP_CHECK(hipMemcpyAsync(S.hs.data(), S.bb.db.st, S.nb * sizeof(DecState), hipMemcpyDeviceToHost, ss));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (b.nsub > 1)
      for (uint32_t q = 0; q < b.nsub; q++)
        HIP_CHECK(hipStreamSynchronize(E.sub[q]));
    for (auto& S : *b.subs)
      for (auto& hsx : S.hs)
        if (hsx.error) {
          report_dec_error(hsx.error);
          return -1;
        }
    return 0;
  }
  // waits for the deferred groups, and reads their states back
  int drain()
  {
    int rc = 0;
    for (uint32_t q = 0; q < kSubStreams; q++)
      HIP_CHECK(hipStreamSynchronize(E.sub[q]));
    HIP_CHECK(hipStreamSynchronize(E.outlQ[1]));
    for (auto& te : timingEnds) {
      float ms = 0.f;
      if (timingFork && hipEventElapsedTime(&ms, timingFork, te.first) == hipSuccess)
        fprintf(stderr, "[sperr_hip] group %u x %u x %u, %u chunks: through %.2f ms after the first group's fork\n",
                te.second[0], te.second[1], te.second[2], te.second[3], ms);
      (void)hipEventDestroy(te.first);
    }
    timingEnds.clear();
    if (timingFork) {
      (void)hipEventDestroy(timingFork);
      timingFork = nullptr;
    }
    for (SubHost* S : pending) {   // stream errors (wrong lengths) surface here
      S->hs.resize(S->nb);
      HIP_CHECK(hipMemcpy(S->hs.data(), S->bb.db.st, S->nb * sizeof(DecState), hipMemcpyDeviceToHost));
      for (auto& hsx : S->hs)
        if (hsx.error) {
          report_dec_error(hsx.error);
          rc = -1;
        }
    }
    pending.clear();
    deferOff = 0;
    return rc;
  }
};

template <typename T>
int decompress_impl(Engine& E, const uint8_t* d_src, T* d_dst, size_t dst_cap_vals, const ContainerInfo& ci,
                    hipStream_t st, const DecodeRequest& req)
{
  DecodeCall<T> call{E, d_src, d_dst, ci, st, req};
  return call.run(dst_cap_vals);
}

// ------------------------------------------------------------------------------------------
// stage access (parity tests): helpers
// ------------------------------------------------------------------------------------------
__global__ void k_fake_condi_header(uint8_t* dst)
{
  if (threadIdx.x || blockIdx.x)
    return;
  const double zero = 0.0, one = 1.0;
  dst[0] = 0x80;
  memcpy(dst + 1, &zero, 8);
  memcpy(dst + 9, &one, 8);
}

}  // namespace

// The box [lo, lo + dims) of a container's volume and the chunks it meets; -1 when window_select refuses it
int box_select(const ContainerInfo& ci, const size_t lo[3], const size_t dims[3], Window& w)
{
  return window_select(ci.vol, ci.chunk, lo, dims, w) ? 0 : -1;
}

// Level `level` of the container `ci` describes, whole (lo and dims null) or the box [lo, lo + dims) of it, and the
// chunks it meets; -1 when the container has no such level or window_select refuses the box
int level_select(const ContainerInfo& ci, size_t level, const size_t* lo, const size_t* dims, Window& w)
{
  multires_levels(ci.vol, ci.chunk, w.m);
  if (level >= w.m.nlev || (lo == nullptr) != (dims == nullptr))
    return -1;
  w.level = true;
  w.h = level;
  const Dims zero{0, 0, 0};
  Dims ld, cr;
  for (int a = 0; a < 3; a++) {
    cr[a] = w.m.cres[level][a];
    ld[a] = cr[a] * w.m.grid[a];
  }
  return window_select(ld, cr, lo ? lo : zero.data(), dims ? dims : ld.data(), w) ? 0 : -1;
}

// `req` of the container at d_src (described by `ci`) into d_dst (x fastest), which holds dst_cap_bytes
int decode_to(Engine& E, const void* d_src, int output_float, void* d_dst, size_t dst_cap_bytes,
              const ContainerInfo& ci, hipStream_t st, const DecodeRequest& req)
{
  return with_elem(output_float, [&](auto t) {
    using T = decltype(t);
    return decompress_impl<T>(E, static_cast<const uint8_t*>(d_src), static_cast<T*>(d_dst), dst_cap_bytes / sizeof(T),
                              ci, st, req);
  });
}

// the window `w` of it, once d_dst is seen to hold the window
int decode_window(Engine& E, const void* d_src, int output_float, void* d_dst, size_t dst_cap_bytes,
                  const ContainerInfo& ci, hipStream_t st, const Window& w, const ViewPitch* outView)
{
  const size_t esz = output_float ? sizeof(float) : sizeof(double);
  if (outView ? !view_fits(w.dims[0], w.dims[1], w.dims[2], *outView, esz, dst_cap_bytes)
              : dst_cap_bytes / esz < w.dims[0] * w.dims[1] * w.dims[2])
    return -1;
  DecodeRequest req;
  req.set_window(w);
  req.outView = outView;
  return decode_to(E, d_src, output_float, d_dst, dst_cap_bytes, ci, st, req);
}

// stage access (engine_core.h): the integer decoder alone, on a bare SPECK stream
int speck3d_decode_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_stream, size_t stream_len,
                         void* d_coef, uint64_t* d_sign, int* width_out)
{
  uint8_t head[9];
  HIP_CHECK(hipMemcpyAsync(head, d_stream, 9, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const int nbp = head[0];
  const bool wide = nbp > 32;
  if (nbp > kMaxPlanes)
    return -1;
  // wrap the bare SPECK stream into a chunk stream with a dummy conditioner header
  if (E.misc.ensure(round_up(17 + stream_len + 64, 256)))
    return -1;
  uint8_t* wrap = static_cast<uint8_t*>(E.misc.p);
  LAUNCH_K(k_fake_condi_header, dim3(1), dim3(1), 0, st, wrap);
  HIP_CHECK(hipMemcpyAsync(wrap + 17, d_stream, stream_len, hipMemcpyDeviceToDevice, st));
  const uint32_t refNPlanes = !wide ? (uint32_t)nbp : 0u;   // (refinement bit planes like decompress_impl's)
  if (E.arena.ensure(dec_bytes_per_chunk(P, 17 + stream_len, 0, refNPlanes, false) + 4096))
    return -1;
  Arena A;
  A.base = static_cast<char*>(E.arena.p);
  A.cap = E.arena.n;
  DecBatchBufs bb;
  if (!carve_dec(A, P, 1, 17 + stream_len, bb, 0, refNPlanes))
    return -1;
  DecBuffers d = bb.db;
  const uint64_t off = 0, len = 17 + stream_len;
  HIP_CHECK(hipMemcpyAsync(bb.chunkOff, &off, 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(bb.chunkLen, &len, 8, hipMemcpyHostToDevice, st));
  if (reset_dec_call(d, 1, st) || reset_dec_pass(bb, 1, wide, st))
    return -1;
  const uint32_t n = P.N;
  if (wide) {
    d.coef = bb.vals;
    d.coefStride = bb.valsStride;
  }
  const DecPlanHost ph = dec_plan_host(P);
  if (launch_speck_decode(st, d, ph, wrap, bb.chunkOff, bb.chunkLen, wide, nbp))
    return -1;
  HIP_CHECK(hipMemcpyAsync(d_coef, d.coef, (size_t)n * (wide ? 8 : 4), hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_sign, d.sign, ((n + 63) / 64) * 8, hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  E.prof.collect();
  *width_out = wide ? 8 : 4;
  return 0;
}

}  // namespace sperrhip
