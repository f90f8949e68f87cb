// abi.hip -- the C ABI declared in include/sperr_hip.h, but for the stage access of the parity tests (abi_stages.hip).
// An entry point checks its arguments, leases an engine and calls the encoder's front (engine_core.h), the decoder's
// (decode_request.h) or a feature's (view.h, fields.h, boxes.h, quality.h, outlier.h); nothing here is a template
// of the element type.
//
// Host logic restated from the reference (file:line under /root/reference):
//   src/SPERR_C_API.cpp:135-258             C API semantics (ownership, return codes)
//   src/SPERR_C_API.cpp:7-134               the 2D entry points
#include "decode_request.h"
#include "quality.h"
#include "fields.h"
#include "boxes.h"

namespace sperrhip {
namespace {

// The host entry points of a sub-box and of a level: the streams of the chunks `ids` of the host container at `h`
// travel to the calling thread's device packed, in their order (one copy per run of chunks that lie back to back in
// the container), `decode` runs the device path on that buffer -- `packed` is `ci` with those chunks' offsets
// pointing into it -- and the result comes back in one copy, into a malloc'd buffer
template <typename F>
int decode_packed_host(const uint8_t* h, const ContainerInfo& ci, const std::vector<uint32_t>& ids, size_t outBytes,
                       void** dst, F&& decode)
{
  ContainerInfo packed = ci;
  size_t total = 0;
  for (uint32_t id : ids) {
    packed.off[id] = total;
    total += ci.len[id];
  }
  void *d_in = nullptr, *d_out = nullptr;
  auto release = [&]() {
    if (d_in)
      (void)hipFree(d_in);
    if (d_out)
      (void)hipFree(d_out);
  };
  if (hipMalloc(&d_in, std::max<size_t>(total, 1)) != hipSuccess || hipMalloc(&d_out, outBytes) != hipSuccess) {
    (void)hipGetLastError();
    fprintf(stderr, "[sperr_hip] device allocation failed\n");
    release();
    return -1;
  }
  int rtn = 0;
  for (size_t i = 0; rtn == 0 && i < ids.size();) {
    size_t j = i + 1;
    while (j < ids.size() && ci.off[ids[j]] == ci.off[ids[j - 1]] + ci.len[ids[j - 1]])
      j++;
    const size_t bytes = ci.off[ids[j - 1]] + ci.len[ids[j - 1]] - ci.off[ids[i]];
    if (bytes && hipMemcpy(static_cast<uint8_t*>(d_in) + packed.off[ids[i]], h + ci.off[ids[i]], bytes,
                           hipMemcpyHostToDevice) != hipSuccess)
      rtn = -1;
    i = j;
  }
  if (rtn == 0) {
    Lease L(nullptr);   // (the host entry points run on stream 0)
    rtn = L.e ? decode(*L.e, d_in, packed, d_out) : -1;
  }
  if (rtn == 0) {
    void* buf = malloc(outBytes);
    if (buf && hipMemcpy(buf, d_out, outBytes, hipMemcpyDeviceToHost) == hipSuccess)
      *dst = buf;
    else {
      free(buf);
      rtn = -1;
    }
  }
  release();
  return rtn;
}

// The host entry points of the hierarchy, the same way: the stream at `src` travels to the calling thread's device,
// `decode` runs the device call on it -- d_out takes the outBytes of the volume (the slice), d_lv[h] the lvn[h]
// doubles of level h -- and the volume and every level come back into malloc'd buffers
template <typename F>
int decode_multires_host(const void* src, size_t src_len, size_t outBytes, const std::vector<size_t>& lvn, void** dst,
                         double** levels, F&& decode)
{
  std::vector<void*> dev;
  auto release = [&]() {
    for (void* p : dev)
      (void)hipFree(p);
  };
  auto dalloc = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess)
      return nullptr;
    dev.push_back(p);
    return p;
  };
  void* d_in = dalloc(src_len);
  void* d_out = dalloc(outBytes);
  std::vector<double*> d_lv(lvn.size(), nullptr);
  bool ok = d_in && d_out;
  for (size_t h = 0; ok && h < lvn.size(); h++) {
    d_lv[h] = static_cast<double*>(dalloc(lvn[h] * 8));
    ok = d_lv[h] != nullptr;
  }
  if (!ok) {
    fprintf(stderr, "[sperr_hip] device allocation failed\n");
    release();
    return -1;
  }
  int rtn = -1;
  if (hipMemcpy(d_in, src, src_len, hipMemcpyHostToDevice) == hipSuccess)
    rtn = decode(d_in, d_out, d_lv.data());
  if (rtn == 0) {
    void* buf = malloc(outBytes);
    if (buf && hipMemcpy(buf, d_out, outBytes, hipMemcpyDeviceToHost) == hipSuccess)
      *dst = buf;
    else {
      free(buf);
      rtn = -1;
    }
    for (size_t h = 0; rtn == 0 && h < lvn.size(); h++) {
      levels[h] = static_cast<double*>(malloc(lvn[h] * 8));
      if (!levels[h] || hipMemcpy(levels[h], d_lv[h], lvn[h] * 8, hipMemcpyDeviceToHost) != hipSuccess)
        rtn = -1;
    }
  }
  release();
  return rtn;
}

}  // namespace
}  // namespace sperrhip

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace sperrhip;

// what the device decode entry points begin with: an engine leased, the caller's stream, the container's header read
struct DevDecode {
  hipStream_t st;   // (before the lease, which takes it)
  Lease L;
  ContainerInfo ci;
  const bool ok;
  DevDecode(const void* d_src, size_t src_len, void* hip_stream)
      : st(static_cast<hipStream_t>(hip_stream)),
        L(st),
        ok(L.e && read_container_info(static_cast<const uint8_t*>(d_src), src_len, ci, st) == 0)
  {
  }
};

// a slice's stream (without the 10-byte header) described as a container of one chunk
static ContainerInfo one_slice_info(size_t dimx, size_t dimy, size_t src_len, int output_float)
{
  ContainerInfo ci;
  ci.vol = {dimx, dimy, 1};
  ci.nvals = dimx * dimy;
  ci.chunk = ci.vol;
  ci.is_float = output_float != 0;
  ci.off = {0};
  ci.len = {src_len};
  return ci;
}

// what every compress entry point refuses first, with code 2: a quality that is not positive, a mode that is none of
// the three.  Before any -1: a null pointer with a bad mode still answers 2
static bool bad_quality_or_mode(int mode, double quality)
{
  return quality <= 0.0 || mode < 1 || mode > 3;
}

extern "C" {

// Gives back what the library keeps between calls: the workspaces and shape tables of every idle
// engine, the staging and device buffers of every idle farm worker, the calling thread's slice
// buffers.  Engines and workers in use by other threads are left alone.  For hosts that embed the
// library (an HDF5 filter, a long-running service) and call it rarely.
static void thread_slice_bufs_drop();
void sperrhip_release(void)
{
  (void)guarded("sperrhip_release", [&]() -> int {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    // The idle engines are picked (and marked busy, so nobody leases them) under the pool's lock;
    // their memory goes with the lock released.  `all` may grow meanwhile (acquire() on another
    // thread): only the raw pointers collected here are used, the engines themselves never move.
    std::vector<Engine*> idle;
    {
      std::lock_guard<std::mutex> lock(g_pool.mu);
      idle.reserve(g_pool.all.size());
      for (auto& e : g_pool.all)
        if (!e->busy && e->dev >= 0) {
          e->busy = true;
          idle.push_back(e.get());
        }
    }
    for (Engine* e : idle)
      if (hipSetDevice(e->dev) == hipSuccess)
        e->drop_memory();
    {
      std::lock_guard<std::mutex> lock(g_pool.mu);
      for (Engine* e : idle)
        e->busy = false;
    }
    g_pool.cv.notify_all();
    farm_release_idle();
    if (have)
      (void)hipSetDevice(cur);
    thread_slice_bufs_drop();
    return 0;
  });
}

const char* sperrhip_version(void)
{
  return "sperr_hip 0.1 (gfx950; SPERR bitstream major version 0)";
}

void sperrhip_profile_enable(int on)
{
  std::lock_guard<std::mutex> lock(g_prof_cfg_mu);
  g_prof_on = on != 0;
}
void sperrhip_profile_only(const char* kernel)
{
  std::lock_guard<std::mutex> lock(g_prof_cfg_mu);
  g_prof_only = kernel ? kernel : "";
}
unsigned long long sperrhip_debug_counter(int which)
{
  if (which == 3) {   // bytes of the largest workspace arena an engine of this process holds
    std::lock_guard<std::mutex> lock(g_pool.mu);
    size_t most = 0;
    for (auto& e : g_pool.all)
      most = std::max(most, e->arena.n);
    return (unsigned long long)most;
  }
  if (which == 6) {   // bytes of ALL device buffers of the engine that holds most (arena + slots + the PWE buffers)
    std::lock_guard<std::mutex> lock(g_pool.mu);
    size_t most = 0;
    for (auto& e : g_pool.all)
      most = std::max(most, e->device_bytes());
    return (unsigned long long)most;
  }
  if (which == 4 || which == 5)   // pinned staging / device bytes the farm's workers hold right now
    return farm_footprint(which == 4);
  if (which == 7)   // batches whose 32-bit pass took the fused encoder head (k_head_fused)
    return g_dbg_counter[3].load();
  if (which == 8)   // windows of bands the series compression calls ran (abi_series.hip)
    return g_dbg_counter[4].load();
  return which >= 0 && which < 3 ? g_dbg_counter[which].load() : 0ull;
}
void sperrhip_debug_lis_stamps(int on, unsigned long long* out64)
{
  g_lis_stamps_on = on != 0;
  if (out64)
    for (size_t i = 0; i < 64; i++)
      out64[i] = i < g_lis_stamps_host.size() ? g_lis_stamps_host[i] : 0;
}
void sperrhip_profile_reset(void)
{
  std::lock_guard<std::mutex> lock(g_pool.mu);
  for (auto& e : g_pool.all) {
    std::lock_guard<std::mutex> l2(e->prof.mu);
    e->prof.acc.clear();
  }
}
int sperrhip_profile_get(const char** names, double* millis, int* launches, int cap)
{
  return guarded("sperrhip_profile_get", [&]() -> int {
    return sperrhip_profile_get2(names, millis, nullptr, launches, cap);
  });
}
int sperrhip_profile_get2(const char** names, double* busy_millis, double* sum_millis, int* launches,
                          int cap)
{
  return guarded("sperrhip_profile_get2", [&]() -> int {
    // the engines' tables merged; the names stay valid until the next call
    static std::mutex mu;
    static std::map<std::string, ProfEntry> merged;
    std::lock_guard<std::mutex> lock(mu);
    merged.clear();
    {
      std::lock_guard<std::mutex> lp(g_pool.mu);
      for (auto& e : g_pool.all) {
        std::lock_guard<std::mutex> l2(e->prof.mu);
        for (auto& kv : e->prof.acc) {
          ProfEntry& m = merged[kv.first];
          m.ms += kv.second.ms;
          m.busy += kv.second.busy;
          m.launches += kv.second.launches;
        }
      }
    }
    int i = 0;
    for (auto& kv : merged) {
      if (i < cap) {
        names[i] = kv.first.c_str();
        busy_millis[i] = kv.second.busy;
        if (sum_millis)
          sum_millis[i] = kv.second.ms;
        launches[i] = kv.second.launches;
      }
      i++;
    }
    return i;
  });
}

size_t sperrhip_max_compressed_size(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                                    size_t chunk_y, size_t chunk_z, int mode, double quality)
{
  const Dims vol{dimx, dimy, dimz};
  Dims cd{chunk_x, chunk_y, chunk_z};
  for (int a = 0; a < 3; a++)
    cd[a] = std::min(std::max<size_t>(1, cd[a]), vol[a]);
  const auto chunks = chunk_volume(vol, cd);
  size_t total = 20 + 4 * chunks.size();
  for (auto& c : chunks)
    total += host_chunk_stream_bound(c[1] * c[3] * c[5], mode, quality);
  return total;
}

int sperrhip_compress_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                          size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                          void* d_dst, size_t dst_cap, size_t* dst_len, void* hip_stream)
{
  return guarded("sperrhip_compress_dev", [&]() -> int {
    if (bad_quality_or_mode(mode, quality))
      return 2;
    if (!d_src || !d_dst || !dst_len || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return compress_to(E, d_src, is_float, vol, ch, mode, quality, static_cast<uint8_t*>(d_dst), dst_cap, dst_len, st);
  });
}

// ---- the size mode (budget.h) ----
size_t sperrhip_chunk_count(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z)
{
  const size_t n = container_chunk_count(Dims{dimx, dimy, dimz}, Dims{chunk_x, chunk_y, chunk_z});
  return n == SIZE_MAX ? 0 : n;
}

int sperrhip_size_survey_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                             size_t chunk_y, size_t chunk_z, size_t nchunks_cap, double* q, int32_t* nbp, uint64_t* end,
                             uint8_t* is_const, void* hip_stream)
{
  return guarded("sperrhip_size_survey_dev", [&]() -> int {
    if (!d_src || !q || !nbp || !end || !is_const || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    if (nchunks_cap < sperrhip_chunk_count(dimx, dimy, dimz, chunk_x, chunk_y, chunk_z))
      return -1;   // (the caller's arrays are too short)
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    return size_survey_to(*L.e, d_src, is_float, vol, ch, q, nbp, end, is_const, static_cast<hipStream_t>(hip_stream));
  });
}

int sperrhip_compress_size_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                               size_t chunk_y, size_t chunk_z, size_t target_bytes, void* d_dst, size_t dst_cap,
                               size_t* dst_len, uint64_t* budgets, size_t budgets_cap, void* hip_stream)
{
  return guarded("sperrhip_compress_size_dev", [&]() -> int {
    if (!d_src || !d_dst || !dst_len || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    if (budgets && budgets_cap < sperrhip_chunk_count(dimx, dimy, dimz, chunk_x, chunk_y, chunk_z))
      return -1;   // (the caller's array is too short)
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    return compress_size_to(*L.e, d_src, is_float, vol, ch, target_bytes, static_cast<uint8_t*>(d_dst), dst_cap, dst_len,
                            budgets, static_cast<hipStream_t>(hip_stream));
  });
}

// ---- PSNR of the whole volume (psnr_vol.h) ----
int sperrhip_psnr_ladder(double range, double psnr, double* t, double* q)
{
  PsnrLadder L;
  if (!t || !q || !std::isfinite(psnr) || !(range > 0.0) || !std::isfinite(range) || !psnr_vol_ladder(range, psnr, &L))
    return -1;
  *t = L.t;
  for (int k = 0; k < kPsnrRungs; k++)
    q[k] = L.q[k];
  return 0;
}

int sperrhip_range_dev(const void* d_src, const sperrhip_view* view, int is_float, size_t dimx, size_t dimy, size_t dimz,
                       double* vmin, double* vmax, void* hip_stream)
{
  return guarded("sperrhip_range_dev", [&]() -> int {
    if (!d_src || !vmin || !vmax || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    const ViewPitch pitch = view ? ViewPitch{view->pitch_y, view->pitch_z} : view_dense(dimx, dimy);
    if (!view_valid(dimx, dimy, dimz, pitch))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    return range_to(*L.e, d_src, is_float, Dims{dimx, dimy, dimz}, view ? &pitch : nullptr, vmin, vmax,
                    static_cast<hipStream_t>(hip_stream));
  });
}

int sperrhip_compress_psnr_dev(const void* d_src, const sperrhip_view* view, int is_float, size_t dimx, size_t dimy,
                               size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z, double psnr, double range,
                               void* d_dst, size_t dst_cap, size_t* dst_len, void* hip_stream)
{
  return guarded("sperrhip_compress_psnr_dev", [&]() -> int {
    if (!d_src || !d_dst || !dst_len || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    if (!std::isfinite(psnr) || !(range >= 0.0) || !std::isfinite(range))
      return -1;
    const ViewPitch pitch = view ? ViewPitch{view->pitch_y, view->pitch_z} : view_dense(dimx, dimy);
    if (!view_valid(dimx, dimy, dimz, pitch))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    return compress_psnr_to(*L.e, d_src, is_float, vol, ch, psnr, range, static_cast<uint8_t*>(d_dst), dst_cap, dst_len,
                            static_cast<hipStream_t>(hip_stream), view ? &pitch : nullptr);
  });
}

int sperrhip_compress_view_dev(const void* d_src, const sperrhip_view* view, int is_float, size_t dimx, size_t dimy,
                               size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                               void* d_dst, size_t dst_cap, size_t* dst_len, void* hip_stream)
{
  return guarded("sperrhip_compress_view_dev", [&]() -> int {
    if (bad_quality_or_mode(mode, quality))
      return 2;
    if (!d_src || !view || !d_dst || !dst_len)
      return -1;
    const ViewPitch pitch{view->pitch_y, view->pitch_z};
    if (!view_valid(dimx, dimy, dimz, pitch))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return compress_to(E, d_src, is_float, vol, ch, mode, quality, static_cast<uint8_t*>(d_dst), dst_cap, dst_len, st,
                       Coded::Container, &pitch);
  });
}

int sperrhip_parse_header_dev(const void* d_src, size_t src_len, size_t* dimx, size_t* dimy,
                              size_t* dimz, int* is_float, size_t* chunk_x, size_t* chunk_y,
                              size_t* chunk_z)
{
  return sperrhip_parse_header_stream_dev(d_src, src_len, dimx, dimy, dimz, is_float, chunk_x, chunk_y, chunk_z,
                                          nullptr);
}

// (the header is read behind whatever `hip_stream` still has to do: the NULL stream does not wait for a non-blocking
// stream, so a container that is still being written there would be parsed from the bytes before it)
int sperrhip_parse_header_stream_dev(const void* d_src, size_t src_len, size_t* dimx, size_t* dimy,
                                     size_t* dimz, int* is_float, size_t* chunk_x, size_t* chunk_y,
                                     size_t* chunk_z, void* hip_stream)
{
  return guarded("sperrhip_parse_header_stream_dev", [&]() -> int {
    DevDecode d(d_src, src_len, hip_stream);
    if (!d.ok)
      return -1;
    const ContainerInfo& ci = d.ci;
    *dimx = ci.vol[0];
    *dimy = ci.vol[1];
    *dimz = ci.vol[2];
    *is_float = ci.is_float ? 1 : 0;
    if (chunk_x)
      *chunk_x = ci.chunk[0];
    if (chunk_y)
      *chunk_y = ci.chunk[1];
    if (chunk_z)
      *chunk_z = ci.chunk[2];
    return 0;
  });
}

int sperrhip_decompress_dev(const void* d_src, size_t src_len, int output_float, void* d_dst,
                            size_t dst_cap_bytes, size_t* dimx, size_t* dimy, size_t* dimz,
                            void* hip_stream)
{
  return guarded("sperrhip_decompress_dev", [&]() -> int {
    if (!d_src || !d_dst)
      return -1;
    DevDecode d(d_src, src_len, hip_stream);
    if (!d.ok)
      return -1;
    if (dimx)
      *dimx = d.ci.vol[0];
    if (dimy)
      *dimy = d.ci.vol[1];
    if (dimz)
      *dimz = d.ci.vol[2];
    return decode_to(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, DecodeRequest{});
  });
}

size_t sperrhip_max_compressed_size_batch(size_t nvol, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                                          size_t chunk_y, size_t chunk_z, int mode, double quality)
{
  const size_t one = sperrhip_max_compressed_size(dimx, dimy, dimz, chunk_x, chunk_y, chunk_z, mode, quality);
  if (nvol != 0 && one > SIZE_MAX / nvol)
    return 0;
  return nvol * one;
}

int sperrhip_compress_batch_dev(const void* d_src, int is_float, size_t nvol, size_t dimx, size_t dimy, size_t dimz,
                                size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                                void* d_dst, size_t dst_cap, size_t* offsets, void* hip_stream)
{
  return guarded("sperrhip_compress_batch_dev", [&]() -> int {
    if (bad_quality_or_mode(mode, quality))
      return 2;
    if (!d_src || !d_dst || !offsets || nvol == 0 || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    if (nvol > 0xffffffffull / dimz)   // (chunk origins of the stacked view are 32-bit)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return compress_batch_to(E, d_src, is_float, nvol, vol, ch, mode, quality, static_cast<uint8_t*>(d_dst), dst_cap,
                             offsets, st);
  });
}

int sperrhip_decompress_batch_dev(const void* d_src, const size_t* offsets, size_t nvol, int output_float,
                                  void* d_dst, size_t dst_cap_bytes, size_t* dimx, size_t* dimy, size_t* dimz,
                                  void* hip_stream)
{
  return guarded("sperrhip_decompress_batch_dev", [&]() -> int {
    if (!d_src || !offsets || !d_dst || nvol == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    ContainerInfo all;
    std::vector<std::array<size_t, 6>> list;
    if (read_batch_info(E, src, offsets, nvol, all, list, st))
      return -1;
    if (all.nvals > dst_cap_bytes / (output_float ? sizeof(float) : sizeof(double)))
      return -1;
    if (dimx)
      *dimx = all.vol[0];
    if (dimy)
      *dimy = all.vol[1];
    if (dimz)
      *dimz = all.vol[2] / nvol;
    DecodeRequest req;
    req.stacked = &list;
    return decode_to(E, src, output_float, d_dst, dst_cap_bytes, all, st, req);
  });
}

int sperrhip_box_chunks(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y,
                        size_t chunk_z, const size_t box_lo[3], const size_t box_dims[3], uint32_t* ids,
                        size_t cap, size_t* count)
{
  return guarded("sperrhip_box_chunks", [&]() -> int {
    if (!box_lo || !box_dims || !count)
      return -1;
    std::vector<uint32_t> v;
    if (!box_chunks(Dims{dimx, dimy, dimz}, Dims{chunk_x, chunk_y, chunk_z}, Dims{box_lo[0], box_lo[1], box_lo[2]},
                    Dims{box_dims[0], box_dims[1], box_dims[2]}, v))
      return -1;
    *count = v.size();
    if (!ids || cap < v.size())
      return 1;
    memcpy(ids, v.data(), v.size() * sizeof(uint32_t));
    return 0;
  });
}

int sperrhip_decompress_box_dev(const void* d_src, size_t src_len, int output_float, const size_t box_lo[3],
                                const size_t box_dims[3], void* d_dst, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_box_dev", [&]() -> int {
    if (!d_src || !d_dst || !box_lo || !box_dims)
      return -1;
    DevDecode d(d_src, src_len, hip_stream);
    Window w;
    if (!d.ok || box_select(d.ci, box_lo, box_dims, w))
      return -1;
    return decode_window(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, w);
  });
}

int sperrhip_decompress_level_dev(const void* d_src, size_t src_len, int output_float, size_t level,
                                  const size_t box_lo[3], const size_t box_dims[3], void* d_dst,
                                  size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_level_dev", [&]() -> int {
    if (!d_src || !d_dst)
      return -1;
    DevDecode d(d_src, src_len, hip_stream);
    Window w;
    if (!d.ok || level_select(d.ci, level, box_lo, box_dims, w))
      return -1;
    return decode_window(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, w);
  });
}

int sperrhip_multires_levels(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y,
                             size_t chunk_z, size_t* nlev, size_t* level_dims)
{
  return guarded("sperrhip_multires_levels", [&]() -> int {
    const Dims vol{dimx, dimy, dimz};
    Dims cd{chunk_x, chunk_y, chunk_z};
    if (!nlev || dimx == 0 || dimy == 0 || dimz == 0)
      return -1;
    for (int a = 0; a < 3; a++)
      cd[a] = std::min(std::max<size_t>(1, cd[a]), vol[a]);
    MultiRes m;
    multires_levels(vol, cd, m);
    *nlev = m.nlev;
    if (level_dims)
      for (size_t h = 0; h < m.nlev; h++)
        for (int a = 0; a < 3; a++)
          level_dims[3 * h + a] = (size_t)m.cres[h][a] * m.grid[a];
    return 0;
  });
}

int sperrhip_decompress_multires_dev(const void* d_src, size_t src_len, int output_float,
                                     void* d_dst, size_t dst_cap_bytes, size_t nlev,
                                     double* const* d_levels, void* hip_stream)
{
  return guarded("sperrhip_decompress_multires_dev", [&]() -> int {
    if (!d_src || !d_dst || (nlev && !d_levels))
      return -1;
    DevDecode d(d_src, src_len, hip_stream);
    if (!d.ok)
      return -1;
    MultiRes m;
    multires_levels(d.ci.vol, d.ci.chunk, m);
    if (m.nlev != nlev)
      return -1;   // (sperrhip_multires_levels tells how many there are)
    for (size_t h = 0; h < nlev; h++) {
      if (!d_levels[h])
        return -1;
      m.d_level[h] = d_levels[h];
    }
    DecodeRequest req;
    req.levels = &m;
    return decode_to(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, req);
  });
}

// What a host thread that codes slices keeps: a stream of its own (calls of several threads then run
// side by side; on the null stream they would queue behind each other) and two device buffers that
// only grow (hipMalloc / hipFree per call would synchronise the device; the stream-ordered allocator
// handed out blocks whose contents the next call did not see: not used).  Freed with the thread.
struct ThreadSliceBufs {
  int dev = -1;          // the device the stream and the buffers belong to
  hipStream_t s = nullptr;
  void* p[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};
  hipStream_t stream()
  {
    if (!s && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
      s = nullptr;
    return s;
  }
  void* get(int i, size_t bytes)
  {
    if (bytes > cap[i]) {
      if (p[i])
        (void)hipFree(p[i]);
      p[i] = nullptr;
      cap[i] = 0;
      if (hipMalloc(&p[i], round_up(bytes, 1 << 20)) != hipSuccess)
        return nullptr;
      cap[i] = round_up(bytes, 1 << 20);
    }
    return p[i];
  }
  void drop()
  {
    for (int i = 0; i < 2; i++) {
      if (p[i])
        (void)hipFree(p[i]);
      p[i] = nullptr;
      cap[i] = 0;
    }
    if (s)
      (void)hipStreamDestroy(s);
    s = nullptr;
  }
};
// One set per device the thread has coded slices on: a thread that moves to another device
// (hipSetDevice between two calls) leases an engine of THAT device, whose arena, sub-streams and
// events must not meet a stream or buffers of the device it came from.
struct ThreadSliceCache {
  std::vector<ThreadSliceBufs> sets;
  ThreadSliceBufs& of_current_device()
  {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
      dev = 0;
    for (auto& b : sets)
      if (b.dev == dev)
        return b;
    sets.emplace_back();
    sets.back().dev = dev;
    return sets.back();
  }
  ~ThreadSliceCache()
  {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto& b : sets) {
      if (have && b.dev != cur)
        (void)hipSetDevice(b.dev);
      b.drop();
    }
    if (have)
      (void)hipSetDevice(cur);
  }
};
static ThreadSliceCache& thread_slice_cache()
{
  static thread_local ThreadSliceCache t;
  return t;
}
static ThreadSliceBufs& thread_slice_bufs()
{
  return thread_slice_cache().of_current_device();
}
static void thread_slice_bufs_drop()
{
  ThreadSliceCache& c = thread_slice_cache();
  int cur = 0;
  const bool have = hipGetDevice(&cur) == hipSuccess;
  for (auto& b : c.sets) {
    if (have && b.dev != cur)
      (void)hipSetDevice(b.dev);
    if (b.s)
      (void)hipStreamSynchronize(b.s);
    b.drop();
  }
  c.sets.clear();
  if (have)
    (void)hipSetDevice(cur);
}

// ---- 2D slices (include/SPERR_C_API.h:53-81, src/SPERR_C_API.cpp:7-134) ------------------------
size_t sperrhip_max_compressed_size_2d(size_t dimx, size_t dimy, int mode, double quality)
{
  return 10 + sperrhip_max_compressed_size(dimx, dimy, 1, dimx, dimy, 1, mode, quality);
}

int sperrhip_compress_2d_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, int mode,
                             double quality, int out_inc_header, void* d_dst, size_t dst_cap,
                             size_t* dst_len, void* hip_stream)
{
  return guarded("sperrhip_compress_2d_dev", [&]() -> int {
    if (bad_quality_or_mode(mode, quality))
      return 2;
    if (!d_src || !d_dst || !dst_len || dimx == 0 || dimy == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    const Dims vol{dimx, dimy, 1};
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const Coded what = out_inc_header ? Coded::SliceWithHeader : Coded::Slice;
    return compress_to(E, d_src, is_float, vol, vol, mode, quality, static_cast<uint8_t*>(d_dst), dst_cap, dst_len, st,
                       what);
  });
}

// d_src: the stream WITHOUT the optional 10-byte header, as sperr_decomp_2d takes it
int sperrhip_decompress_2d_dev(const void* d_src, size_t src_len, int output_float, size_t dimx,
                               size_t dimy, void* d_dst, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_2d_dev", [&]() -> int {
    if (!d_src || !d_dst || dimx == 0 || dimy == 0 || src_len < 17)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    DecodeRequest req;
    req.slices = true;
    return decode_to(E, d_src, output_float, d_dst, dst_cap_bytes, one_slice_info(dimx, dimy, src_len, output_float),
                     st, req);
  });
}

// ---- a batch of same-shape slices (the stacked view of DESIGN.md section 0c: N slices read as one volume of
// (x, y, N) whose chunk s is slice s, one shape group on the 2D coder's forest) ------------------------------------
size_t sperrhip_max_compressed_size_2d_batch(size_t nslice, size_t dimx, size_t dimy, int mode, double quality)
{
  const size_t one = sperrhip_max_compressed_size_2d(dimx, dimy, mode, quality);
  if (nslice != 0 && one > SIZE_MAX / nslice)
    return 0;
  return nslice * one;
}

int sperrhip_compress_2d_batch_dev(const void* d_src, int is_float, size_t nslice, size_t dimx, size_t dimy,
                                   int mode, double quality, int out_inc_header,
                                   void* d_dst, size_t dst_cap, size_t* offsets, void* hip_stream)
{
  return guarded("sperrhip_compress_2d_batch_dev", [&]() -> int {
    if (bad_quality_or_mode(mode, quality))
      return 2;
    if (!d_src || !d_dst || !offsets || nslice == 0 || dimx == 0 || dimy == 0)
      return -1;
    if (nslice > 0xffffffffull)   // (chunk origins of the stacked view are 32-bit)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    const Dims vol{dimx, dimy, 1};
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const Coded what = out_inc_header ? Coded::SliceWithHeader : Coded::Slice;
    return compress_batch_to(E, d_src, is_float, nslice, vol, vol, mode, quality, static_cast<uint8_t*>(d_dst), dst_cap,
                             offsets, st, what);
  });
}

int sperrhip_decompress_2d_batch_dev(const void* d_src, const size_t* offsets, size_t nslice, int has_header,
                                     int output_float, size_t dimx, size_t dimy,
                                     void* d_dst, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_2d_batch_dev", [&]() -> int {
    if (!d_src || !offsets || !d_dst || nslice == 0 || dimx == 0 || dimy == 0)
      return -1;
    if (nslice > 0xffffffffull || dimx > 0xffffffffull || dimy > 0xffffffffull)
      return -1;
    const size_t H = has_header ? 10 : 0, esz = output_float ? sizeof(float) : sizeof(double);
    if (dimx > SIZE_MAX / dimy || dimx * dimy > SIZE_MAX / 8 / nslice)
      return -1;
    const size_t per = dimx * dimy;
    if (per * nslice > dst_cap_bytes / esz)
      return -1;
    ContainerInfo all;
    all.vol = {dimx, dimy, nslice};
    all.chunk = {dimx, dimy, 1};
    all.nvals = per * nslice;
    all.is_float = output_float != 0;
    std::vector<std::array<size_t, 6>> list(nslice);
    for (size_t s = 0; s < nslice; s++) {
      if (offsets[s + 1] < offsets[s] || offsets[s + 1] - offsets[s] < H + 17)   // (as sperrhip_decompress_2d_dev)
        return -1;
      all.off.push_back(offsets[s] + H);
      all.len.push_back(offsets[s + 1] - offsets[s] - H);
      list[s] = {0, dimx, 0, dimy, s, 1};
    }
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint32_t hdrDims[2] = {(uint32_t)dimx, (uint32_t)dimy};
    DecodeRequest req;
    req.stacked = &list;
    req.slices = true;
    req.sliceHdr = has_header ? hdrDims : nullptr;
    return decode_to(E, d_src, output_float, d_dst, dst_cap_bytes, all, st, req);
  });
}

// ---- reference-compatible host API (src/SPERR_C_API.cpp:135-258) ---------------------------

void sperr_parse_header(const void* src, size_t* dimx, size_t* dimy, size_t* dimz, int* is_float)
{
  const uint8_t* p = static_cast<const uint8_t*>(src);
  const bool is_3d = (p[1] & 0x40) != 0;
  *is_float = (p[1] & 0x20) ? 1 : 0;
  uint32_t d[3] = {1, 1, 1};
  memcpy(d, p + 2, is_3d ? 12 : 8);
  *dimx = d[0];
  *dimy = d[1];
  *dimz = d[2];
}

// include/SPERR_C_API.h:138-156, src/SPERR_C_API.cpp:260-280,
// src/SPERR3D_Stream_Tools.cpp:134-226: host-side byte surgery, no GPU involved.  Every chunk
// stream keeps `pct` percent of its bytes (at least 64, at most what it has), the container is
// flagged as a portion and the chunk lengths are rewritten; the decoder zero-pads what is missing.
int sperr_trunc_3d(const void* src, size_t src_len, unsigned pct, void** dst, size_t* dst_len)
{
  return guarded("sperr_trunc_3d", [&]() -> int {
    return hostc::truncate_container(static_cast<const uint8_t*>(src), src_len, pct, dst, dst_len);
  });
}

// include/SPERR_C_API.h:53-62, src/SPERR_C_API.cpp:7-97
int sperr_comp_2d(const void* src, int is_float, size_t dimx, size_t dimy, int mode, double quality,
                  int out_inc_header, void** dst, size_t* dst_len)
{
  return guarded("sperr_comp_2d", [&]() -> int {
    if (*dst != nullptr)
      return 1;
    if (bad_quality_or_mode(mode, quality))
      return 2;
    const size_t n = dimx * dimy, esz = is_float ? 4 : 8;
    const size_t cap = sperrhip_max_compressed_size_2d(dimx, dimy, mode, quality);
    // on the calling thread's own stream, with its own device buffers: slices coded from several host
    // threads run side by side
    ThreadSliceBufs& tb = thread_slice_bufs();
    hipStream_t ts = tb.stream();
    void *d_in = tb.get(0, n * esz), *d_out = tb.get(1, cap);
    if (!d_in || !d_out) {
      fprintf(stderr, "[sperr_hip] device allocation failed\n");
      return -1;
    }
    int rtn = -1;
    size_t len = 0;
    if (hipMemcpyAsync(d_in, src, n * esz, hipMemcpyHostToDevice, ts) == hipSuccess)
      rtn = sperrhip_compress_2d_dev(d_in, is_float, dimx, dimy, mode, quality, out_inc_header, d_out,
                                     cap, &len, ts);
    if (rtn == 0) {
      void* buf = malloc(len);
      if (buf && hipMemcpyAsync(buf, d_out, len, hipMemcpyDeviceToHost, ts) == hipSuccess &&
          hipStreamSynchronize(ts) == hipSuccess) {
        *dst = buf;
        *dst_len = len;
      }
      else {
        free(buf);
        rtn = -1;
      }
    }
    (void)hipStreamSynchronize(ts);
    return rtn;
  });
}

// include/SPERR_C_API.h:75-81, src/SPERR_C_API.cpp:99-134
int sperrhip_multires_levels_2d(size_t dimx, size_t dimy, size_t* nlev, size_t* level_dims)
{
  return guarded("sperrhip_multires_levels_2d", [&]() -> int {
    if (!nlev || !level_dims || dimx == 0 || dimy == 0 || dimx > 0xffff || dimy > 0xffff)
      return -1;
    MultiRes m;
    multires_levels_2d(dimx, dimy, m);
    *nlev = m.nlev;
    for (size_t h = 0; h < m.nlev; h++) {
      level_dims[2 * h] = m.cres[h][0];
      level_dims[2 * h + 1] = m.cres[h][1];
    }
    return 0;
  });
}

int sperrhip_decompress_2d_multires_dev(const void* d_src, size_t src_len, int output_float, size_t dimx,
                                        size_t dimy, void* d_dst, size_t dst_cap_bytes, size_t nlev,
                                        double* const* d_levels, void* hip_stream)
{
  return guarded("sperrhip_decompress_2d_multires_dev", [&]() -> int {
    if (!d_src || !d_dst || dimx == 0 || dimy == 0 || src_len < 17 || (nlev && !d_levels))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    MultiRes m;
    multires_levels_2d(dimx, dimy, m);
    if (m.nlev != nlev)
      return -1;   // (sperrhip_multires_levels_2d tells how many there are)
    for (size_t h = 0; h < nlev; h++) {
      if (!d_levels[h])
        return -1;
      m.d_level[h] = d_levels[h];
    }
    DecodeRequest req;
    req.slices = true;
    req.levels = &m;
    return decode_to(E, d_src, output_float, d_dst, dst_cap_bytes, one_slice_info(dimx, dimy, src_len, output_float),
                     st, req);
  });
}

int sperrhip_decomp_2d_multires(const void* src, size_t src_len, int output_float, size_t dimx,
                                size_t dimy, void** dst, size_t* nlev, size_t* level_dims, double** levels)
{
  return guarded("sperrhip_decomp_2d_multires", [&]() -> int {
    if (!dst || *dst != nullptr)
      return 1;
    if (src_len < 17 || !nlev || !level_dims || !levels ||
        sperrhip_multires_levels_2d(dimx, dimy, nlev, level_dims))
      return -1;
    const size_t outBytes = dimx * dimy * (output_float ? 4 : 8);
    std::vector<size_t> lvn(*nlev);
    for (size_t h = 0; h < *nlev; h++)
      lvn[h] = level_dims[2 * h] * level_dims[2 * h + 1];
    return decode_multires_host(src, src_len, outBytes, lvn, dst, levels, [&](void* d_in, void* d_out, double** d_lv) {
      return sperrhip_decompress_2d_multires_dev(d_in, src_len, output_float, dimx, dimy, d_out, outBytes, *nlev, d_lv,
                                                 nullptr);
    });
  });
}

int sperr_decomp_2d(const void* src, size_t src_len, int output_float, size_t dimx, size_t dimy,
                    void** dst)
{
  return guarded("sperr_decomp_2d", [&]() -> int {
    if (*dst != nullptr)
      return 1;
    const size_t n = dimx * dimy, esz = output_float ? 4 : 8;
    ThreadSliceBufs& tb = thread_slice_bufs();   // (see sperr_comp_2d)
    hipStream_t ts = tb.stream();
    void *d_in = src_len >= 17 ? tb.get(0, src_len) : nullptr, *d_out = tb.get(1, n * esz);
    if (!d_in || !d_out)
      return -1;
    int rtn = -1;
    if (hipMemcpyAsync(d_in, src, src_len, hipMemcpyHostToDevice, ts) == hipSuccess)
      rtn = sperrhip_decompress_2d_dev(d_in, src_len, output_float, dimx, dimy, d_out, n * esz, ts);
    if (rtn == 0) {
      void* buf = malloc(n * esz);
      if (buf && hipMemcpyAsync(buf, d_out, n * esz, hipMemcpyDeviceToHost, ts) == hipSuccess &&
          hipStreamSynchronize(ts) == hipSuccess)
        *dst = buf;
      else {
        free(buf);
        rtn = -1;
      }
    }
    (void)hipStreamSynchronize(ts);
    return rtn;
  });
}

// host buffers in, malloc'd host buffers out: the volume and the levels of the hierarchy
// (SPERR3D_OMP_D::decompress(p, true) + release_decoded_data / release_hierarchy)
int sperrhip_decomp_3d_multires(const void* src, size_t src_len, int output_float, size_t* dimx,
                                size_t* dimy, size_t* dimz, void** dst, size_t* nlev,
                                size_t* level_dims, double** levels)
{
  return guarded("sperrhip_decomp_3d_multires", [&]() -> int {
    if (!dst || *dst != nullptr)
      return 1;
    if (src_len < 18 || !nlev || !level_dims || !levels)
      return -1;
    ContainerInfo ci;
    size_t need = 0;
    if (parse_container_host(static_cast<const uint8_t*>(src), src_len, src_len, ci, &need) != 0)
      return -1;
    if (sperrhip_multires_levels(ci.vol[0], ci.vol[1], ci.vol[2], ci.chunk[0], ci.chunk[1], ci.chunk[2],
                                 nlev, level_dims))
      return -1;
    const size_t outBytes = ci.nvals * (output_float ? 4 : 8);
    std::vector<size_t> lvn(*nlev);
    for (size_t h = 0; h < *nlev; h++)
      lvn[h] = level_dims[3 * h] * level_dims[3 * h + 1] * level_dims[3 * h + 2];
    const int rtn =
        decode_multires_host(src, src_len, outBytes, lvn, dst, levels, [&](void* d_in, void* d_out, double** d_lv) {
          return sperrhip_decompress_multires_dev(d_in, src_len, output_float, d_out, outBytes, *nlev, d_lv, nullptr);
        });
    if (rtn == 0) {
      *dimx = ci.vol[0];
      *dimy = ci.vol[1];
      *dimz = ci.vol[2];
    }
    return rtn;
  });
}

}  // extern "C"

// ---- a box per entry out of a batch of containers (boxes.h) -------------------------------------
// The grid a boxes call cuts along: the volume and every container's chunk dims, or with a level -- which the
// containers must then share chunk dims for, and have -- the level's dims and the chunks' corner cres[h] (level_select)
static int boxes_grid(const Dims& vol, const std::vector<Dims>& chunk, const size_t* level, Dims& full,
                      std::vector<Dims>& cell, MultiRes& m)
{
  full = vol;
  cell = chunk;
  if (!level)
    return 0;
  for (const Dims& c : chunk)
    if (c != chunk[0])
      return -1;
  multires_levels(vol, chunk[0], m);
  if (*level >= m.nlev)
    return -1;
  Dims cr;
  for (int a = 0; a < 3; a++) {
    cr[a] = m.cres[*level][a];
    full[a] = cr[a] * m.grid[a];
  }
  cell.assign(chunk.size(), cr);
  return 0;
}

// sperrhip_decompress_boxes_dev behind its refusals of arguments and its lease (decode_request.h); abi_series.hip
// decodes a series' bands with it.
// The containers are read where they lie: every offset of the call is one from the lowest of their addresses.  Each
// header is read once; the plan (boxes.h) names the slots, whose chunks become the call's stacked list -- one chunk per
// slot, in the slots' order -- with the plan's geometry on the window.  Direct form: the crop writers fill d_dst.
// Staged form: they fill the engine's staging array, typed as the output, and one launch of k_boxes_copy moves every
// pair's window into its box
int sperrhip::decode_boxes_to(Engine& E, const void* const* d_srcs, const size_t* src_lens, size_t ncont,
                              const uint32_t* which, const size_t* box_lo, size_t nbox, const size_t box_dims[3],
                              const size_t* level, unsigned pct, int output_float, void* d_dst, size_t dst_cap_bytes,
                              hipStream_t st, const Dims* vol)
{
  uintptr_t base = UINTPTR_MAX;
  for (size_t c = 0; c < ncont; c++)
    base = std::min(base, reinterpret_cast<uintptr_t>(d_srcs[c]));
  const uint8_t* src = reinterpret_cast<const uint8_t*>(base);
  const size_t esz = output_float ? sizeof(float) : sizeof(double);
  std::vector<uint64_t> off(ncont), len(ncont);
  for (size_t c = 0; c < ncont; c++) {
    off[c] = reinterpret_cast<uintptr_t>(d_srcs[c]) - base;
    len[c] = src_lens[c];
  }
  std::vector<ContainerInfo> ci;
  std::vector<uint8_t> heads;
  if (read_headers_at(E, src, off, len, ci, heads, st))
    return -1;
  std::vector<Dims> chunk(ncont), cell;
  for (size_t c = 0; c < ncont; c++) {
    if (ci[c].vol != ci[0].vol || (vol && ci[c].vol != *vol))   // (the batch decode's rule)
      return -1;
    chunk[c] = ci[c].chunk;
    keep_portion(ci[c], pct);
  }
  Dims full;
  Window w;
  BoxesPlan P;
  if (boxes_grid(ci[0].vol, chunk, level, full, cell, w.m) ||
      !boxes_plan(ncont, full, cell.data(), which, box_lo, nbox, Dims{box_dims[0], box_dims[1], box_dims[2]}, P))
    return -1;
  if (P.outVals > dst_cap_bytes / esz || P.stageVals > SIZE_MAX / 8)
    return -1;
  // the call's chunks: slot k is chunk P.slots[k].id of its container
  const size_t nslots = P.slots.size();
  ContainerInfo all;
  std::vector<std::array<size_t, 6>> list(nslots), per;
  all.chunk = ci[0].chunk;
  all.off.resize(nslots);
  all.len.resize(nslots);
  w.ids.resize(nslots);
  w.slotGeom.resize(nslots);
  for (size_t k = 0, have = SIZE_MAX; k < nslots; k++) {
    const BoxesSlot& s = P.slots[k];
    if (s.cont != have) {   // (the slots are in container order)
      per = chunk_volume(ci[s.cont].vol, ci[s.cont].chunk);
      have = s.cont;
      if (per.size() != ci[s.cont].off.size())
        return -1;
    }
    if (s.id >= per.size())
      return -1;
    list[k] = per[s.id];
    all.off[k] = off[s.cont] + ci[s.cont].off[s.id];
    all.len[k] = ci[s.cont].len[s.id];
    w.ids[k] = (uint32_t)k;
    CropGeom& g = w.slotGeom[k];
    for (int a = 0; a < 3; a++) {
      g.rel[a] = P.geom[k].rel[a];
      g.lo[a] = P.geom[k].lo[a];
      g.hi[a] = P.geom[k].hi[a];
    }
  }
  w.crop = true;
  w.level = level != nullptr;
  w.h = level ? *level : 0;
  w.lo = Dims{0, 0, 0};
  w.dims = P.shared ? P.stageDims : P.outDims;
  all.vol = w.dims;
  all.nvals = P.shared ? P.stageVals : P.outVals;
  void* d_out = d_dst;
  size_t outBytes = dst_cap_bytes;
  if (P.shared) {
    outBytes = P.stageVals * esz;
    if (E.boxesStage.ensure(outBytes))
      return -1;
    d_out = E.boxesStage.p;
  }
  DecodeRequest req;
  req.stacked = &list;
  req.window = &w;
  const int rtn = decode_to(E, src, output_float, d_out, outBytes, all, st, req);
  if (rtn || !P.shared)
    return rtn;
  std::vector<BoxesCopyPair> pairs;
  std::vector<uint64_t> first;
  BoxesCopyGeom g;
  boxes_copy_args(P, pairs, first, g);
  const size_t pairBytes = round_up(pairs.size() * sizeof(BoxesCopyPair), 256);
  if (E.misc.ensure(pairBytes + first.size() * 8))
    return -1;
  BoxesCopyPair* d_pairs = static_cast<BoxesCopyPair*>(E.misc.p);
  uint64_t* d_first = reinterpret_cast<uint64_t*>(static_cast<char*>(E.misc.p) + pairBytes);
  const bool vec = boxes_vec_ok(reinterpret_cast<uintptr_t>(d_out), reinterpret_cast<uintptr_t>(d_dst), pairs, g, esz);
  auto copy = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(d_pairs, pairs.data(), pairs.size() * sizeof(BoxesCopyPair), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_first, first.data(), first.size() * 8, hipMemcpyHostToDevice, st));
    if (boxes_copy_run(d_out, d_dst, esz, d_pairs, d_first, g, vec, st))
      return -1;
    HIP_CHECK(hipStreamSynchronize(st));   // (also: the uploads' host arrays may go only once the copies have read them)
    return 0;
  };
  const int rc = copy();
  if (rc)
    drain_after_error(E, st);   // (as ~DecodeCall: queued copies read the vectors above)
  E.prof.collect();
  return rc;
}

extern "C" {

int sperrhip_boxes_plan(size_t ncont, const size_t vol_dims[3], const size_t* chunk_dims, const uint32_t* which,
                        const size_t* box_lo, size_t nbox, const size_t box_dims[3], const size_t* level, size_t out[5])
{
  return guarded("sperrhip_boxes_plan", [&]() -> int {
    if (!vol_dims || !chunk_dims || !box_lo || !box_dims || !out || ncont == 0 || ncont > 0xffffffffull)
      return -1;
    std::vector<Dims> chunk(ncont), cell;
    for (size_t c = 0; c < ncont; c++)
      chunk[c] = Dims{chunk_dims[3 * c], chunk_dims[3 * c + 1], chunk_dims[3 * c + 2]};
    Dims full;
    MultiRes m;
    BoxesPlan P;
    if (boxes_grid(Dims{vol_dims[0], vol_dims[1], vol_dims[2]}, chunk, level, full, cell, m) ||
        !boxes_plan(ncont, full, cell.data(), which, box_lo, nbox, Dims{box_dims[0], box_dims[1], box_dims[2]}, P))
      return -1;
    out[0] = P.slots.size();
    out[1] = P.pairs.size();
    out[2] = P.shared ? 1 : 0;
    out[3] = P.stageVals;
    out[4] = P.outVals;
    return 0;
  });
}

// (the refusals of arguments and the lease; the rest is decode_boxes_to)
int sperrhip_decompress_boxes_dev(const void* const* d_srcs, const size_t* src_lens, size_t ncont, const uint32_t* which,
                                  const size_t* box_lo, size_t nbox, const size_t box_dims[3], const size_t* level,
                                  unsigned pct, int output_float, void* d_dst, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_boxes_dev", [&]() -> int {
    if (!d_srcs || !src_lens || !box_lo || !box_dims || !d_dst || ncont == 0 || nbox == 0 || ncont > 0xffffffffull ||
        nbox > 0xffffffffull || (!which && nbox != ncont))
      return -1;
    for (size_t c = 0; c < ncont; c++)
      if (!d_srcs[c])
        return -1;
    for (size_t e = 0; which && e < nbox; e++)
      if (which[e] >= ncont)
        return -1;
    for (int a = 0; a < 3; a++)
      if (box_dims[a] == 0)
        return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    return decode_boxes_to(*L.e, d_srcs, src_lens, ncont, which, box_lo, nbox, box_dims, level, pct, output_float, d_dst,
                           dst_cap_bytes, static_cast<hipStream_t>(hip_stream), nullptr);
  });
}

// host container in, malloc'd host box out: only the chunks the box meets travel to the device (decode_packed_host),
// are decoded there by the device path on the calling thread's device and stream 0, and the box comes back in one copy
int sperrhip_decomp_3d_box(const void* src, size_t src_len, int output_float, const size_t box_lo[3],
                           const size_t box_dims[3], void** dst)
{
  return guarded("sperrhip_decomp_3d_box", [&]() -> int {
    if (!dst || *dst != nullptr)
      return 1;
    if (!src || !box_lo || !box_dims)
      return -1;
    ContainerInfo ci;
    size_t need = 0;
    if (parse_container_host(static_cast<const uint8_t*>(src), src_len, src_len, ci, &need) != 0)
      return -1;
    Window w;
    if (box_select(ci, box_lo, box_dims, w))
      return -1;
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    const size_t outBytes = w.dims[0] * w.dims[1] * w.dims[2] * esz;
    return decode_packed_host(static_cast<const uint8_t*>(src), ci, w.ids, outBytes, dst,
                              [&](Engine& E, const void* d_in, const ContainerInfo& packed, void* d_out) {
                                return decode_window(E, d_in, output_float, d_out, outBytes, packed, nullptr, w);
                              });
  });
}

// host container in, malloc'd host level (or box of it) out, the same way
int sperrhip_decomp_3d_level(const void* src, size_t src_len, int output_float, size_t level, const size_t box_lo[3],
                             const size_t box_dims[3], size_t out_dims[3], void** dst)
{
  return guarded("sperrhip_decomp_3d_level", [&]() -> int {
    if (!dst || *dst != nullptr)
      return 1;
    if (!src || !out_dims)
      return -1;
    ContainerInfo ci;
    size_t need = 0;
    if (parse_container_host(static_cast<const uint8_t*>(src), src_len, src_len, ci, &need) != 0)
      return -1;
    Window w;
    if (level_select(ci, level, box_lo, box_dims, w))
      return -1;
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    const size_t outBytes = w.dims[0] * w.dims[1] * w.dims[2] * esz;
    const int rtn = decode_packed_host(static_cast<const uint8_t*>(src), ci, w.ids, outBytes, dst,
                                       [&](Engine& E, const void* d_in, const ContainerInfo& packed, void* d_out) {
                                         return decode_window(E, d_in, output_float, d_out, outBytes, packed, nullptr, w);
                                       });
    if (rtn == 0)
      for (int a = 0; a < 3; a++)
        out_dims[a] = w.dims[a];
    return rtn;
  });
}

// ---- a portion: decoding, and truncating on the device ------------------------------------------
size_t sperrhip_portion_len(size_t chunk_len, unsigned pct)
{
  return hostc::portion_len(chunk_len, pct);
}

// The decodes of sperrhip_decompress_dev / _box_dev / _level_dev of the first `pct` percent of every chunk stream: the
// call's own ContainerInfo takes the kept lengths (keep_portion) and the existing path runs on it, so nothing behind
// a kept prefix is read, the workspace follows the kept lengths and no copy of the container is made
int sperrhip_decompress_portion_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                    const size_t* level, const size_t box_lo[3], const size_t box_dims[3], void* d_dst,
                                    size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_portion_dev", [&]() -> int {
    if (!d_src || !d_dst || (box_lo == nullptr) != (box_dims == nullptr))
      return -1;
    DevDecode d(d_src, src_len, hip_stream);
    if (!d.ok)
      return -1;
    keep_portion(d.ci, pct);
    if (!level && !box_lo)
      return decode_to(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, DecodeRequest{});
    Window w;
    if (level ? level_select(d.ci, *level, box_lo, box_dims, w) : box_select(d.ci, box_lo, box_dims, w))
      return -1;
    return decode_window(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, w);
  });
}

// The volume or a box of it, of the first `pct` percent of every chunk stream, into a strided view of d_dst: the
// request names the view, and every writer takes its pitches from DecodeRequest::out_desc
int sperrhip_decompress_view_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                 const size_t box_lo[3], const size_t box_dims[3], void* d_dst,
                                 const sperrhip_view* view, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_view_dev", [&]() -> int {
    if (!d_src || !d_dst || !view || (box_lo == nullptr) != (box_dims == nullptr))
      return -1;
    const ViewPitch pitch{view->pitch_y, view->pitch_z};
    DevDecode d(d_src, src_len, hip_stream);
    if (!d.ok)
      return -1;
    keep_portion(d.ci, pct);
    if (box_lo) {
      Window w;
      if (box_select(d.ci, box_lo, box_dims, w))
        return -1;
      return decode_window(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, w, &pitch);
    }
    if (!view_fits(d.ci.vol[0], d.ci.vol[1], d.ci.vol[2], pitch, output_float ? sizeof(float) : sizeof(double),
                   dst_cap_bytes))
      return -1;
    DecodeRequest req;
    req.outView = &pitch;
    return decode_to(*d.L.e, d_src, output_float, d_dst, dst_cap_bytes, d.ci, d.st, req);
  });
}

// host container in, malloc'd host volume, box or level out: only the kept prefixes of the chosen chunks travel to the
// device (decode_packed_host; the prefixes do not lie back to back, so each is a copy of its own)
int sperrhip_decomp_3d_portion(const void* src, size_t src_len, unsigned pct, int output_float, const size_t* level,
                               const size_t box_lo[3], const size_t box_dims[3], size_t out_dims[3], void** dst)
{
  return guarded("sperrhip_decomp_3d_portion", [&]() -> int {
    if (!dst || *dst != nullptr)
      return 1;
    if (!src || (box_lo == nullptr) != (box_dims == nullptr))
      return -1;
    ContainerInfo ci;
    size_t need = 0;
    if (parse_container_host(static_cast<const uint8_t*>(src), src_len, src_len, ci, &need) != 0)
      return -1;
    keep_portion(ci, pct);
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    const bool all = !level && !box_lo;
    Window w;
    std::vector<uint32_t> every;
    if (all) {
      if (ci.len.size() > 0xffffffffull)
        return -1;
      every.resize(ci.len.size());
      for (size_t i = 0; i < every.size(); i++)
        every[i] = (uint32_t)i;
    }
    else if (level ? level_select(ci, *level, box_lo, box_dims, w) : box_select(ci, box_lo, box_dims, w))
      return -1;
    const Dims od = all ? ci.vol : w.dims;
    const size_t outBytes = od[0] * od[1] * od[2] * esz;
    const int rtn = decode_packed_host(
        static_cast<const uint8_t*>(src), ci, all ? every : w.ids, outBytes, dst,
        [&](Engine& E, const void* d_in, const ContainerInfo& packed, void* d_out) {
          return all ? decode_to(E, d_in, output_float, d_out, outBytes, packed, nullptr, DecodeRequest{})
                     : decode_window(E, d_in, output_float, d_out, outBytes, packed, nullptr, w);
        });
    if (rtn == 0 && out_dims)
      for (int a = 0; a < 3; a++)
        out_dims[a] = od[a];
    return rtn;
  });
}

int sperrhip_trunc_batch_dev(const void* d_src, const size_t* offsets, size_t nvol, unsigned pct, void* d_dst,
                             size_t dst_cap, size_t* out_offsets, void* hip_stream)
{
  return guarded("sperrhip_trunc_batch_dev", [&]() -> int {
    if (!d_src || !offsets || !out_offsets || nvol == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    return trunc_impl(*L.e, static_cast<const uint8_t*>(d_src), offsets, nvol, pct, static_cast<uint8_t*>(d_dst),
                      dst_cap, out_offsets, static_cast<hipStream_t>(hip_stream));
  });
}

int sperrhip_trunc_dev(const void* d_src, size_t src_len, unsigned pct, void* d_dst, size_t dst_cap, size_t* dst_len,
                       void* hip_stream)
{
  if (!dst_len)
    return -1;
  const size_t offs[2] = {0, src_len};
  size_t out[2] = {0, 0};
  const int rtn = sperrhip_trunc_batch_dev(d_src, offs, 1, pct, d_dst, dst_cap, out, hip_stream);
  if (rtn >= 0)
    *dst_len = out[1];
  return rtn;
}

// the figures of nvol reconstructions against their originals (quality.hip); the partials' workspace is the
// leased engine's arena, like every other call's
int sperrhip_quality_batch_dev(const void* d_orig, const void* d_recon, int is_float, size_t nvol, size_t n,
                               double* out, void* hip_stream)
{
  return guarded("sperrhip_quality_batch_dev", [&]() -> int {
    if (!d_orig || !d_recon || !out || nvol == 0 || n == 0)
      return -1;
    const size_t need = quality_workspace_bytes(nvol, n, is_float);
    if (need == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e || L.e->arena.ensure(need))
      return -1;
    const int rtn = quality_run(d_orig, d_recon, is_float, nvol, n, L.e->arena.p, out, hip_stream);
    L.e->prof.collect();
    return rtn;
  });
}

int sperrhip_quality_dev(const void* d_orig, const void* d_recon, int is_float, size_t n, double* out,
                         void* hip_stream)
{
  return sperrhip_quality_batch_dev(d_orig, d_recon, is_float, 1, n, out, hip_stream);
}

// the same of two arrays read through strided views (a NULL view: dense), by the view form of the rows kernel
int sperrhip_quality_view_dev(const void* d_orig, const sperrhip_view* view_orig, const void* d_recon,
                              const sperrhip_view* view_recon, int is_float, size_t dimx, size_t dimy, size_t dimz,
                              double* out, void* hip_stream)
{
  return guarded("sperrhip_quality_view_dev", [&]() -> int {
    if (!d_orig || !d_recon || !out)
      return -1;
    const size_t need = quality_view_workspace_bytes(dimx, dimy, dimz, is_float);
    if (need == 0)
      return -1;
    const ViewPitch dense = view_dense(dimx, dimy);   // (its products fit: the workspace's size has multiplied them)
    const ViewPitch po = view_orig ? ViewPitch{view_orig->pitch_y, view_orig->pitch_z} : dense;
    const ViewPitch pr = view_recon ? ViewPitch{view_recon->pitch_y, view_recon->pitch_z} : dense;
    if (!view_valid(dimx, dimy, dimz, po) || !view_valid(dimx, dimy, dimz, pr))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e || L.e->arena.ensure(need))
      return -1;
    const int rtn = quality_view_run(d_orig, po, d_recon, pr, is_float, dimx, dimy, dimz, L.e->arena.p, out, hip_stream);
    L.e->prof.collect();
    return rtn;
  });
}

// ---- interleaved fields (fields.h) -----------------------------------------------------------------------------
// The fields calls stage: the selected fields are gathered into stacked volumes in a buffer the engine owns
// (k_fields_gather), or scattered from it (k_fields_scatter), and the batch code works on that buffer.

// the layout a call means (NULL: the dense interleave), once the stacked side's size is known not to overflow
static FieldsLayout fields_layout_of(const sperrhip_fields* layout, size_t nfields, size_t dimx, size_t dimy)
{
  return layout ? FieldsLayout{layout->stride_x, layout->pitch_y, layout->pitch_z} : fields_dense(nfields, dimx, dimy);
}

int sperrhip_fields_gather_dev(const void* d_src, const sperrhip_fields* layout, size_t nfields, int is_float,
                               size_t dimx, size_t dimy, size_t dimz, void* d_dst, size_t dst_cap_bytes,
                               void* hip_stream)
{
  return guarded("sperrhip_fields_gather_dev", [&]() -> int {
    size_t count = 0;
    const size_t esz = is_float ? sizeof(float) : sizeof(double);
    if (!d_src || !d_dst || !fields_stacked(nfields, dimx, dimy, dimz, &count) || count > dst_cap_bytes / esz)
      return -1;
    const FieldsLayout l = fields_layout_of(layout, nfields, dimx, dimy);
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (fields_gather_run(d_src, l, nfields, is_float, dimx, dimy, dimz, d_dst, st))
      return -1;
    HIP_CHECK(hipStreamSynchronize(st));
    L.e->prof.collect();
    return 0;
  });
}

int sperrhip_fields_scatter_dev(const void* d_src, size_t nfields, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                void* d_dst, const sperrhip_fields* layout, size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_fields_scatter_dev", [&]() -> int {
    size_t count = 0;
    const size_t esz = is_float ? sizeof(float) : sizeof(double);
    if (!d_src || !d_dst || !fields_stacked(nfields, dimx, dimy, dimz, &count))
      return -1;
    const FieldsLayout l = fields_layout_of(layout, nfields, dimx, dimy);
    if (!fields_fits(nfields, dimx, dimy, dimz, l, esz, dst_cap_bytes))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (fields_scatter_run(d_src, nfields, is_float, dimx, dimy, dimz, d_dst, l, st))
      return -1;
    HIP_CHECK(hipStreamSynchronize(st));
    L.e->prof.collect();
    return 0;
  });
}

int sperrhip_compress_fields_dev(const void* d_src, const sperrhip_fields* layout, size_t nfields, int is_float,
                                 size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z,
                                 int mode, double quality, void* d_dst, size_t dst_cap, size_t* offsets,
                                 void* hip_stream)
{
  return guarded("sperrhip_compress_fields_dev", [&]() -> int {
    if (bad_quality_or_mode(mode, quality))
      return 2;
    size_t count = 0;
    if (!d_src || !d_dst || !offsets || !fields_stacked(nfields, dimx, dimy, dimz, &count) || count > SIZE_MAX / 8)
      return -1;
    const FieldsLayout l = fields_layout_of(layout, nfields, dimx, dimy);
    if (!fields_valid(nfields, dimx, dimy, dimz, l))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    const Dims vol{dimx, dimy, dimz}, ch{chunk_x, chunk_y, chunk_z};
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (E.fieldsStage.ensure(count * (is_float ? sizeof(float) : sizeof(double))) ||
        fields_gather_run(d_src, l, nfields, is_float, dimx, dimy, dimz, E.fieldsStage.p, st))
      return -1;
    return compress_batch_to(E, E.fieldsStage.p, is_float, nfields, vol, ch, mode, quality, static_cast<uint8_t*>(d_dst),
                             dst_cap, offsets, st);
  });
}

int sperrhip_decompress_fields_dev(const void* d_src, const size_t* offsets, size_t nfields, int output_float,
                                   size_t dimx, size_t dimy, size_t dimz, void* d_dst, const sperrhip_fields* layout,
                                   size_t dst_cap_bytes, void* hip_stream)
{
  return guarded("sperrhip_decompress_fields_dev", [&]() -> int {
    size_t count = 0;
    const size_t esz = output_float ? sizeof(float) : sizeof(double);
    if (!d_src || !offsets || !d_dst || !fields_stacked(nfields, dimx, dimy, dimz, &count) || count > SIZE_MAX / 8)
      return -1;
    const FieldsLayout l = fields_layout_of(layout, nfields, dimx, dimy);
    if (!fields_fits(nfields, dimx, dimy, dimz, l, esz, dst_cap_bytes))
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    ContainerInfo all;
    std::vector<std::array<size_t, 6>> list;
    if (read_batch_info(E, src, offsets, nfields, all, list, st))
      return -1;
    if (all.vol != Dims{dimx, dimy, dimz * nfields})   // (every container names the call's dims)
      return -1;
    // the decode goes to the staging buffer: whatever it runs into, d_dst is as it was
    if (E.fieldsStage.ensure(count * esz))
      return -1;
    DecodeRequest req;
    req.stacked = &list;
    const int rtn = decode_to(E, src, output_float, E.fieldsStage.p, count * esz, all, st, req);
    if (rtn)
      return rtn;
    if (fields_scatter_run(E.fieldsStage.p, nfields, output_float, dimx, dimy, dimz, d_dst, l, st))
      return -1;
    HIP_CHECK(hipStreamSynchronize(st));
    E.prof.collect();
    return 0;
  });
}

int sperrhip_quality_fields_dev(const void* d_orig, const sperrhip_fields* layout_orig, const void* d_recon,
                                const sperrhip_fields* layout_recon, size_t nfields, int is_float, size_t dimx,
                                size_t dimy, size_t dimz, double* out, void* hip_stream)
{
  return guarded("sperrhip_quality_fields_dev", [&]() -> int {
    size_t count = 0;
    const size_t esz = is_float ? sizeof(float) : sizeof(double);
    if (!d_orig || !d_recon || !out || !fields_stacked(nfields, dimx, dimy, dimz, &count) || count > SIZE_MAX / 8)
      return -1;
    const FieldsLayout lo = fields_layout_of(layout_orig, nfields, dimx, dimy);
    const FieldsLayout lr = fields_layout_of(layout_recon, nfields, dimx, dimy);
    if (!fields_valid(nfields, dimx, dimy, dimz, lo) || !fields_valid(nfields, dimx, dimy, dimz, lr))
      return -1;
    const size_t n = count / nfields, need = quality_workspace_bytes(nfields, n, is_float);
    if (need == 0)
      return -1;
    Lease L(static_cast<hipStream_t>(hip_stream));
    if (!L.e)
      return -1;
    Engine& E = *L.e;
    if (E.arena.ensure(need) || E.fieldsStage.ensure(count * esz) || E.fieldsStage2.ensure(count * esz))
      return -1;
    if (fields_gather_run(d_orig, lo, nfields, is_float, dimx, dimy, dimz, E.fieldsStage.p, hip_stream) ||
        fields_gather_run(d_recon, lr, nfields, is_float, dimx, dimy, dimz, E.fieldsStage2.p, hip_stream))
      return -1;
    const int rtn = quality_run(E.fieldsStage.p, E.fieldsStage2.p, is_float, nfields, n, E.arena.p, out, hip_stream);
    E.prof.collect();
    return rtn;
  });
}

}  // extern "C"
