// engine_core.h -- what engine.hip (plans, pool), encode.hip and decode.hip (the two calls) share with the C ABI
// (abi.hip, abi_stages.hip): the profiler, device buffers and arenas, a chunk shape's plan, the engine, the pool and a call's
// lease; the file-scope state; and the encoder's front, which abi.hip calls the way it calls the decoder's
// (decode_request.h).  Internal: farm.hip sees engine_internal.h only.
//
// Host logic restated from the reference (file:line under /root/reference):
//   src/SPERR3D_OMP_C.cpp:61-92             one compressor object per thread -> an engine per concurrent caller
#ifndef SPERR_AMD_ENGINE_CORE_H
#define SPERR_AMD_ENGINE_CORE_H

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sperr_hip.h"
#include "engine_internal.h"
#include "host_container.hpp"
#include "speck_dec.h"
#include "dequant.h"
#include "speck_enc.h"
#include "speck_tree_host.hpp"
#include "outlier.h"
#include "poison_env.h"
#include "view.h"
#include "xform.h"

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// profiling
// ------------------------------------------------------------------------------------------
struct ProfEntry {
  double ms = 0.0;     // sum of the launch durations
  double busy = 0.0;   // time during which at least one launch of the kernel was running (launches
                       // of sub-batches on different streams overlap)
  int launches = 0;
};

struct Profiler {
  bool on = false;
  std::string only;   // when not empty: only launches of this kernel are bracketed
  std::mutex mu;      // sub-batches are enqueued from several host threads
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t ref = nullptr;   // origin of the time axis of one collect() period
  struct Open {
    const char* name;
    hipEvent_t a, b;
  };
  std::vector<Open> open;
  std::map<std::string, ProfEntry> acc;

  hipEvent_t get()   // (mu held)
  {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess)
        return nullptr;
      pool.push_back(e);
    }
    return pool[used++];
  }
  void collect()
  {
    std::lock_guard<std::mutex> lock(mu);
    std::map<std::string, std::vector<std::pair<float, float>>> spans;
    for (auto& o : open) {
      float ms = 0.f, t0 = 0.f;
      if (o.a && o.b && hipEventElapsedTime(&ms, o.a, o.b) == hipSuccess) {
        auto& e = acc[o.name];
        e.ms += ms;
        e.launches++;
        if (ref && hipEventElapsedTime(&t0, ref, o.a) == hipSuccess)
          spans[o.name].push_back({t0, t0 + ms});
        else
          e.busy += ms;
      }
    }
    for (auto& kv : spans) {
      auto& v = kv.second;
      std::sort(v.begin(), v.end());
      double busy = 0.0;
      float lo = v[0].first, hi = v[0].second;
      for (size_t i = 1; i < v.size(); i++) {
        if (v[i].first > hi) {
          busy += hi - lo;
          lo = v[i].first;
          hi = v[i].second;
        }
        else
          hi = std::max(hi, v[i].second);
      }
      acc[kv.first].busy += busy + (hi - lo);
    }
    open.clear();
    used = 0;
    ref = nullptr;
  }
};

// ---- the file-scope state of the host side, defined in engine.hip ----
// global switches (sperrhip_profile_enable / _only); the accumulators live in the engines
extern bool g_prof_on;
extern std::string g_prof_only;
extern std::mutex g_prof_cfg_mu;
extern thread_local Profiler* t_prof;   // the profiler of the engine this thread drives (Lease; prof_begin, engine.hip)
extern std::atomic<unsigned long long> g_dbg_counter[5];   // sperrhip_debug_counter (0..2, [3] as counter 7, [4] as counter 8)
extern bool g_lis_stamps_on;                               // sperrhip_debug_lis_stamps
extern std::vector<uint64_t> g_lis_stamps_host;            //   chunk 0 of the last decoded batch
// (t_shared_device: engine_internal.h; g_pool: below, after its type)

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------
// The workspace poison (poison_env.h).  The stream of the call this thread makes, set by its Lease:
// what a call allocates on the way is filled there.  A sub-batch's own host thread has none: stream 0
extern thread_local hipStream_t t_call_stream;

// `n` bytes at `p` that were allocated just now, filled before their first use, whichever stream that is on: the host
// waits for the fill.  Nothing is queued with the switch off
inline int poison_fresh(void* p, size_t n)
{
  const int v = poison_env();
  if (v < 0 || !p || !n)
    return 0;
  HIP_CHECK(hipMemsetAsync(p, v, n, t_call_stream));
  HIP_CHECK(hipStreamSynchronize(t_call_stream));
  return 0;
}

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  void drop()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // workspace: the buffer is a call's working memory, which the poison switch fills (not a plan's tables, which are
  // uploaded whole and once)
  int ensure(size_t bytes, bool workspace = true)
  {
    if (bytes <= n)
      return 0;
    if (p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
    // (a quarter more than asked for, for the small buffers whose size follows the data -- outlier
    //  streams, slots --: a hipFree waits for every stream of the device, the other workers' included,
    //  and a buffer that fits exactly is too small for the next call's slightly longer streams)
    size_t want = bytes < (size_t(256) << 20) ? bytes + bytes / 4 + 4096 : bytes;
    // (callers size their requests against the free memory they saw: when the slack is what does not fit,
    //  the exact size still may)
    if (want != bytes && hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      want = bytes;
    }
    if (!p)
      HIP_CHECK(hipMalloc(&p, want));
    n = want;
    return workspace ? poison_fresh(p, n) : 0;
  }
};

struct Arena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  template <typename T>
  T* take(size_t count)
  {
    // sizes may come from an untrusted header: nothing here may wrap
    if (used > cap || count > (cap - used) / sizeof(T))
      return nullptr;
    const size_t bytes = (count * sizeof(T) + 255) / 256 * 256;
    if (bytes > cap - used)
      return nullptr;
    T* r = reinterpret_cast<T*>(base + used);
    used += bytes;
    return r;
  }
};

// bytes that hold `bits` bits; bit counts read from a container may be anything up to 2^64 - 1
inline uint64_t bytes_of_bits(uint64_t bits)
{
  return bits / 8 + (bits % 8 != 0);
}

inline size_t round_up(size_t v, size_t m)
{
  return (v + m - 1) / m * m;
}

using hostc::Dims;
using hostc::chunk_count;
using hostc::box_chunks;
using hostc::chunk_volume;
using hostc::ContainerInfo;
using hostc::parse_container_host;
using hostc::keep_portion;

// ------------------------------------------------------------------------------------------
// per-shape plan: tree tables on the device, tile maps, DWT pass list
// ------------------------------------------------------------------------------------------
struct LiftPass {
  int axis;
  uint32_t region[3];
};

// How a chunk shape's transform runs.  Decided once, when the plan is made (plan_schedule, engine.hip): the encoder's
// launches (float_stages, pwe_stage_begin) and the decoder's memory layout and launches (compact_box, decode_group,
// enqueue_inverse) read it, and nothing else asks the pass list these questions.
struct LiftSchedule {
  enum Head { kNoHead, kHeadXY, kHeadXYZ };
  Head head = kNoHead;     // the finest level's full-size passes that one kernel runs, straight from / into the volume
  bool fusable = false;    // the passes can collect the largest coefficient / dequantise on the way (plan_fusable)
  bool brick = false;      // x-y-z head, fusable, at least three passes: the coarser levels can work in a compact box
  bool level2 = false;     // passes 3 to 5 -- the second level -- run as one launch each way (plan_level2)
  uint32_t coarseBox[3] = {1, 1, 1};   // the box the coarser levels work in: the largest region of the passes k >= 3
  struct Pass {   // what pass_fuse_rule says of a pass: -1, 0 or 1, and the box of the later passes
    int fuse;
    uint32_t inner[3];
  };
  std::vector<Pass> pass;
  // The passes, counted from the finest, that fused launches run instead of the per-axis kernel: the forward walk's
  // per-axis loop starts there and the inverse walk's stops there
  static size_t fused_passes(Head head, bool level2) { return level2 ? 6 : head == kHeadXYZ ? 3 : head == kHeadXY ? 2 : 0; }
};

struct ShapePlan {
  uint32_t dims[3];
  uint32_t N = 0;
  spk::HostTree ht;
  spk::Tree dtree{};
  DevBuf tables;
  const uint64_t* d_initLIS = nullptr;
  const uint32_t* d_initLen = nullptr;
  const uint32_t* d_levelOff = nullptr;
  const uint16_t* d_tileLevel = nullptr;
  const uint32_t* d_tileStart = nullptr;
  const uint32_t* d_levelFirstTile = nullptr;
  const uint32_t* d_levelNumTiles = nullptr;
  const uint32_t* d_depthBlocks = nullptr;
  const uint8_t* d_levelSlot = nullptr;
  const uint64_t* d_iRoots = nullptr;   // (2D forest)
  const uint8_t* d_slotLevel = nullptr;
  const spk::LevelClass* d_levelClass = nullptr;
  const uint32_t* d_wordLeaf = nullptr;   // nullptr: no raster word lies over leaf-word grids
  const FusedRoot* d_fusedRoots = nullptr;   // non-null: the encoder's 32-bit pass can take k_head_fused (fused_head_roots)
  const uint8_t* d_mxSlot = nullptr;      // k_lis_mx: column of every shape class
  const uint8_t* d_mxLevelGroup = nullptr;
  int l0Level = -1;                       // LIS level of 2x2x2 leaf sets that k_lis_l0 can decode
  int l1Level = -1;                       // LIS level of 4x4x4 sets that k_lis_l1 can decode
  int l2Level = -1;                       // LIS level of 8x8x8 sets that k_lis_l2 can decode
  int maxK = 0;
  std::vector<uint32_t> depthBlockOff;
  uint32_t nListTiles = 0, nSlots = 0, nPixTiles = 0, nstrides = 0;
  uint64_t maxPhaseBits = 0;
  size_t lisEntries = 0;
  std::vector<LiftPass> fwd;
  LiftSchedule schedule;   // which kernels run the passes (plan_schedule)
  DecPlanHost dec{};       // the list kernels the shape's decoder takes (plan_list_kernels); per-call fields at their defaults
};

// The plan of a dx x dy x dz chunk, its kernel choices decided by the rules of engine.hip (fuse_xy ... plan_list_kernels);
// twoD: the plan of a slice's DECODER, with the forest of the 2D coder (spk::kTree2D).  0 ok
int build_plan(ShapePlan& P, size_t dx, size_t dy, size_t dz, bool twoD = false);

// ------------------------------------------------------------------------------------------
// engines: one per (device, concurrent caller)
// ------------------------------------------------------------------------------------------
// The reference's classes are re-entrant (one compressor object per OpenMP thread,
// src/SPERR3D_OMP_C.cpp:61-92).  Here an engine owns everything a call needs on ONE device (streams,
// per-shape plans, workspaces); a call leases an idle engine of the device that is current on the
// calling thread and a new one is made when all of them are busy (up to
// SPERR_HIP_ENGINES_PER_DEVICE, default 4; then callers wait).  The chunk farm (farm.hip) runs
// several workers per device this way.
constexpr uint32_t kSubStreams = 8;

struct Engine {
  int dev = -1;
  bool busy = false;
  bool ready = false;
  Profiler prof;
  hipStream_t sub[kSubStreams] = {};
  hipEvent_t evFork = nullptr, evJoin[kSubStreams] = {};
  hipStream_t outl = nullptr;               // the 1D decoder of outlier streams runs here, beside the chunk decoders
  hipStream_t outlQ[kSubStreams] = {};      //   (one per sub-batch; outlQ[0] == outl; a priority of their own: init_handles)
  hipStream_t sideQ[kSubStreams] = {};      // the encoder's census beside a part's pyramid (normal priority)
  hipEvent_t evOutl[kSubStreams] = {}, evOutlFork[kSubStreams] = {};   // (per sub-batch)
  hipEvent_t evPweFork = nullptr;          // encoder, point-wise error mode: the outlier stage's first half starts beside the 3D coder
  hipEvent_t evPweJoin = nullptr;          //   ... and its end is waited for by the batch's stream, not by the host (round 6)
  std::map<Dims, std::unique_ptr<ShapePlan>> plans;
  std::vector<Dims> planOrder;             // least recently used first
  DevBuf arena, slots, misc;
  DevBuf outlFixed, outlVar, outlStream;   // point-wise error mode: workspace of the outlier coder
  DevBuf pweBox;                           //   ... and the coarser levels' box of its reconstruction (pwe_stage_begin)
  hipStream_t pweLastStream = nullptr;     //   stream the last batch's outlier stage ended on without a wait (round 6): the
                                           //   next batch of the SAME call may run its stage on another one and reuses the buffers
  DevBuf outlDec[kSubStreams];             //   (decoder: one per sub-batch of a call)
  DevBuf decBox[kSubStreams];              //   ... and the coarser levels' box of a sub-batch with outlier streams
  uint32_t* liveHost[kSubStreams] = {};    // pinned: answers to "do any chunks still decode" (DecPlanHost)
  void* pweHost = nullptr;                 // pinned: the outlier stage's first read-back (a copy into pageable memory
  size_t pweHostBytes = 0;                 //   would hold the host until the stream gets there: compress_impl)
  hipEvent_t liveEv[kSubStreams][kLiveSlots] = {};
  DevBuf wideScratch;                       // 64-bit retry of a batch whose coder arrays lay over the chunk buffer
  DevBuf fieldsStage, fieldsStage2;         // interleaved fields (fields.h): the stacked volumes the batch code works on,
                                            //   and the quality call's other side
  DevBuf boxesStage;                        // boxes of a batch (boxes.h): the staging array of the staged form
  DevBuf maskStage, maskStage2;             // missing values (mask.h): the in-filled volume the encoder reads; the
                                            //   compacted arrays of the quality call
  DevBuf maskWork;                          //   ... and the bit array, the tile counts and the partials of mask.hip
  DevBuf maskPyramid;                       //   ... and the levels of a smooth in-fill (mask_fill.h) in global memory
  DevBuf relStage;                          // relative error (rel.h): the double volume or box y that the coder sees
  DevBuf relWork;                           //   ... and the sign bits' workspace with the read-back record of rel.hip
  DevBuf sizeWork;                          // size mode (budget.h): the survey's table of the volume and the dealt budgets
  DevBuf seriesStage;                       // time series (series.h): the fp64 bands between the butterflies and the coder
  DevBuf seriesTab;                         //   ... and the kernels' tables of step, band and output pointers
  std::vector<std::unique_ptr<DevBuf>> pweBufs;   // outlier streams of the batches of one call
  size_t freeMemAtInit = 0;

  // an engine whose initialisation fails is never handed out (EnginePool::acquire): what it made
  // up to the failure goes back at once
  int init()
  {
    if (ready)
      return 0;
    const int rc = init_handles();
    if (rc)
      destroy_handles();
    return rc;
  }
  void destroy_handles()
  {
    auto ds = [](hipStream_t& s) { if (s) (void)hipStreamDestroy(s); s = nullptr; };
    auto de = [](hipEvent_t& e) { if (e) (void)hipEventDestroy(e); e = nullptr; };
    for (uint32_t q = 0; q < kSubStreams; q++) {
      ds(sub[q]);
      de(evJoin[q]);
      if (q > 0)
        ds(outlQ[q]);
      ds(sideQ[q]);
      de(evOutl[q]);
      de(evOutlFork[q]);
      if (q == 0) {
        de(evPweFork);
        de(evPweJoin);
      }
      if (liveHost[q])
        (void)hipHostFree(liveHost[q]);
      liveHost[q] = nullptr;
      if (q == 0 && pweHost) {
        (void)hipHostFree(pweHost);
        pweHost = nullptr;
        pweHostBytes = 0;
      }
      for (int k = 0; k < kLiveSlots; k++)
        de(liveEv[q][k]);
    }
    de(evFork);
    ds(outl);
    outlQ[0] = nullptr;
    ready = false;
  }
  int init_handles()
  {
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    freeMemAtInit = fr;
    for (uint32_t q = 0; q < kSubStreams; q++) {
      HIP_CHECK(hipStreamCreateWithFlags(&sub[q], hipStreamNonBlocking));
      HIP_CHECK(hipEventCreateWithFlags(&evJoin[q], hipEventDisableTiming));
    }
    HIP_CHECK(hipEventCreateWithFlags(&evFork, hipEventDisableTiming));
    // The streams of the 1D decoder (outlier lists, beside a sub-batch's chunk decoders) get a priority of
    // their own.  The runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues PER PRIORITY, and a side
    // stream that shares a hardware queue with the stream it is meant to run beside runs behind it instead
    // (round 4: with eight sub-streams and eight side streams on eight queues, eight point-wise-error chunks
    // at a tolerance of 1e-4 decoded in 44.8 ms -- the 30 ms of the 1D decoder and then the rest -- where 16
    // queues, or this, give 31; 16 queues cost the fixed-rate compression 2 %).  Not the encoder's census
    // streams: with a priority of their own 8 chunks compress at 63 instead of 75 GB/s.
    int prLeast = 0, prGreatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest) != hipSuccess) {
      (void)hipGetLastError();
      prLeast = prGreatest = 0;
    }
    static const int sidePrio = getenv("SPERR_HIP_SIDE_PRIORITY") ? atoi(getenv("SPERR_HIP_SIDE_PRIORITY")) : 1;
    const int prSide = sidePrio > 0 ? prGreatest : sidePrio < 0 ? prLeast : 0;   // (0: like every other stream)
    HIP_CHECK(hipStreamCreateWithPriority(&outl, hipStreamNonBlocking, prSide));
    outlQ[0] = outl;
    for (uint32_t q = 1; q < kSubStreams; q++)
      HIP_CHECK(hipStreamCreateWithPriority(&outlQ[q], hipStreamNonBlocking, prSide));
    for (uint32_t q = 0; q < kSubStreams; q++)
      HIP_CHECK(hipStreamCreateWithFlags(&sideQ[q], hipStreamNonBlocking));
    for (uint32_t q = 0; q < kSubStreams; q++) {
      HIP_CHECK(hipEventCreateWithFlags(&evOutl[q], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&evOutlFork[q], hipEventDisableTiming));
    }
    HIP_CHECK(hipEventCreateWithFlags(&evPweFork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&evPweJoin, hipEventDisableTiming));
    for (uint32_t q = 0; q < kSubStreams; q++) {
      HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&liveHost[q]), kLiveSlots * sizeof(uint32_t), hipHostMallocDefault));
      for (int k = 0; k < kLiveSlots; k++)
        HIP_CHECK(hipEventCreateWithFlags(&liveEv[q][k], hipEventDisableTiming));
    }
    ready = true;
    return 0;
  }

  // the device tables of at most kMaxPlans chunk shapes are kept (a ragged volume has 8 shapes)
  static constexpr size_t kMaxPlans = 64;
  // (dz = 0: the decoder's plan of a dx x dy slice, with the 2D coder's forest)
  ShapePlan* plan(size_t dx, size_t dy, size_t dz)
  {
    const Dims key{dx, dy, dz};
    auto it = plans.find(key);
    if (it != plans.end()) {
      auto pos = std::find(planOrder.begin(), planOrder.end(), key);
      if (pos != planOrder.end())
        planOrder.erase(pos);
      planOrder.push_back(key);
      return it->second.get();
    }
    auto p = std::make_unique<ShapePlan>();
    if (dz == 0 ? build_plan(*p, dx, dy, 1, true) : build_plan(*p, dx, dy, dz))
      return nullptr;
    ShapePlan* raw = p.get();
    plans[key] = std::move(p);
    planOrder.push_back(key);
    return raw;
  }
  // sperrhip_release(): everything an idle engine holds in HBM goes back (streams and events
  // stay; the next call sizes the workspaces again).  The engine's device is current.
  // THE list of the engine's workspace buffers: the arena, the containers' slots, and what point-wise error mode adds
  // (the outlier coder's arrays, the boxes of the coarser levels, the outlier streams) and the staging buffers of the
  // fields, boxes, mask and relative error calls.  drop_memory, device_bytes and the poison fill walk it, so a buffer
  // added here is dropped, counted and poisoned alike.  (Not the plans' tables: constant data, uploaded once)
  template <typename Self, typename F>
  static void walk_buffers(Self& e, F&& f)
  {
    for (auto* b : {&e.arena, &e.slots, &e.misc, &e.outlFixed, &e.outlVar, &e.outlStream, &e.pweBox, &e.wideScratch,
                    &e.fieldsStage, &e.fieldsStage2, &e.boxesStage, &e.maskStage, &e.maskStage2, &e.maskWork,
                    &e.maskPyramid, &e.relStage, &e.relWork, &e.sizeWork, &e.seriesStage, &e.seriesTab})
      f(*b);
    for (auto& b : e.outlDec)
      f(b);
    for (auto& b : e.decBox)
      f(b);
    for (auto& b : e.pweBufs)
      if (b)
        f(*b);
  }
  void drop_memory()
  {
    for (auto& kv : plans)
      kv.second->tables.drop();
    plans.clear();
    planOrder.clear();
    walk_buffers(*this, [](DevBuf& b) { b.drop(); });
    pweBufs.clear();
  }
  // every workspace buffer of the engine -- sperrhip_debug_counter(6)
  size_t device_bytes() const
  {
    size_t n = 0;
    walk_buffers(*this, [&n](const DevBuf& b) { n += b.n; });
    return n;
  }
  // ---- the workspace poison (SPERR_HIP_POISON, poison_env.h) ----
  // A call has leased the engine and has queued nothing yet: every buffer the engine holds is filled on the call's
  // stream, and every stream of the engine waits for the fill, so that it stands in front of the call's first kernel
  // wherever the call forks to.  (Nothing of the engine is in flight: a call ends in a wait of the host.)  With the
  // switch off nothing is queued; *filled says whether anything was
  int poison_fill(hipStream_t st, bool* filled)
  {
    *filled = false;
    const int v = poison_env();
    if (v < 0)
      return 0;
    int rc = 0;
    walk_buffers(*this, [&](DevBuf& b) {
      if (rc == 0 && b.p && hipMemsetAsync(b.p, v, b.n, st) != hipSuccess)
        rc = -1;
    });
    if (rc) {
      fprintf(stderr, "[sperr_hip] the poison fill failed: %s\n", hipGetErrorString(hipGetLastError()));
      return -1;
    }
    *filled = true;
    HIP_CHECK(hipEventRecord(evFork, st));
    for (uint32_t q = 0; q < kSubStreams; q++) {
      HIP_CHECK(hipStreamWaitEvent(sub[q], evFork, 0));
      HIP_CHECK(hipStreamWaitEvent(outlQ[q], evFork, 0));
      HIP_CHECK(hipStreamWaitEvent(sideQ[q], evFork, 0));
    }
    return 0;
  }
  // A call carves the arena again for a further batch of workspace (a cap on the arena, more than 256 chunks of a
  // shape, a second shape group): `ss` is the stream that uses the arena first, and the earlier batch has been waited
  // for by the host.  *filled as above
  int poison_arena(hipStream_t ss, bool* filled = nullptr)
  {
    const int v = poison_env();
    if (filled)
      *filled = v >= 0 && arena.p;
    if (v >= 0 && arena.p)
      HIP_CHECK(hipMemsetAsync(arena.p, v, arena.n, ss));
    return 0;
  }
  // called between calls only (no kernel of this engine is in flight)
  void trim_plans()
  {
    while (planOrder.size() > kMaxPlans) {
      auto it = plans.find(planOrder.front());
      if (it != plans.end()) {
        if (it->second->tables.p)
          (void)hipFree(it->second->tables.p);
        plans.erase(it);
      }
      planOrder.erase(planOrder.begin());
    }
  }
};

struct EnginePool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::unique_ptr<Engine>> all;

  // an idle engine of the device current on this thread; nullptr: no device / initialisation failed
  Engine* acquire()
  {
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      fprintf(stderr, "[sperr_hip] no HIP device available; this library has no CPU fallback\n");
      return nullptr;
    }
    if (hipGetDevice(&dev) != hipSuccess)
      return nullptr;
    static const size_t perDev = getenv("SPERR_HIP_ENGINES_PER_DEVICE")
                                     ? (size_t)std::max(1, atoi(getenv("SPERR_HIP_ENGINES_PER_DEVICE")))
                                     : 4;
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      size_t have = 0;
      for (auto& e : all)
        if (e->dev == dev) {
          have++;
          if (!e->busy) {
            e->busy = true;
            return e.get();
          }
        }
      if (have < perDev) {
        auto e = std::make_unique<Engine>();
        e->dev = dev;
        e->busy = true;
        Engine* raw = e.get();
        all.push_back(std::move(e));
        lock.unlock();
        if (raw->init()) {
          lock.lock();
          raw->busy = false;
          raw->dev = -1;   // never handed out again
          cv.notify_all();
          return nullptr;
        }
        return raw;
      }
      cv.wait(lock);
    }
  }
  void release(Engine* e)
  {
    {
      std::lock_guard<std::mutex> lock(mu);
      e->busy = false;
    }
    cv.notify_all();
  }
  // engines of a device that are on a call right now (the caller's own included)
  size_t busy_on(int dev)
  {
    std::lock_guard<std::mutex> lock(mu);
    size_t n = 0;
    for (auto& e : all)
      n += (e->dev == dev && e->busy) ? 1 : 0;
    return n;
  }
};

extern EnginePool g_pool;   // (engine.hip)

// a call's hold on an engine; also makes the engine's profiler the calling thread's
// `st` is the call's stream: under the poison switch the engine's buffers are filled on it before the call does anything
// (Engine::poison_fill; a fill that fails gives the engine back: e is null)
struct Lease {
  Engine* e;
  hipStream_t st;
  bool poisoned = false;
  explicit Lease(hipStream_t stream) : e(g_pool.acquire()), st(stream)
  {
    if (e) {
      {
        std::lock_guard<std::mutex> lock(g_prof_cfg_mu);
        e->prof.on = g_prof_on;
        e->prof.only = g_prof_only;
        t_prof = &e->prof;
      }
      t_call_stream = st;
      if (e->poison_fill(st, &poisoned)) {
        (void)hipStreamSynchronize(st);
        t_prof = nullptr;
        t_call_stream = nullptr;
        g_pool.release(e);
        e = nullptr;
      }
    }
  }
  ~Lease()
  {
    if (e) {
      // (a call whose kernels use nothing of the engine's may end without a wait, abi_mask.hip: the fill it queued must
      //  not run into the engine's next call on another stream)
      if (poisoned)
        (void)hipStreamSynchronize(st);
      t_call_stream = nullptr;
      t_prof = nullptr;
      e->trim_plans();
      g_pool.release(e);
    }
  }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
};

// a call that did not end well waits for the caller's stream and the engine's before its host buffers go (engine.hip)
void drain_after_error(Engine& E, hipStream_t st);

// How the kernels see a valid view (view.h) of a volume of dimz slices: their address is (z * rows + y) * pitch + x,
// so the first two entries are pitches rather than extents; nothing on the device reads the third
inline VolDesc view_desc(const ViewPitch& p, size_t dimz) { return VolDesc{{p.y, p.z / p.y, dimz}}; }

// ------------------------------------------------------------------------------------------
// the encoder's front (encode.hip); the decoder's is decode_request.h
// ------------------------------------------------------------------------------------------
// what a compression call makes: a 3D container, or one 2D slice without / with the 10-byte header
enum class Coded { Container, Slice, SliceWithHeader };

// The volume `vol` at d_src (floats or doubles, x fastest; with srcView the first element of a valid strided view of
// it) into d_dst, which holds dst_cap bytes, in chunks of chunkPref where the volume allows.  mode 1: fixed rate,
// `quality` bits per value; mode 2: fixed PSNR; mode 3: fixed point-wise error.  0 ok, *dst_len the bytes written
int compress_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, int mode,
                double quality, uint8_t* d_dst, size_t dst_cap, size_t* dst_len, hipStream_t st,
                Coded what = Coded::Container, const ViewPitch* srcView = nullptr);
// nvol volumes of dims `vol` back to back into nvol containers (slices: streams) back to back: container v at
// [offsets[v], offsets[v + 1])
int compress_batch_to(Engine& E, const void* d_src, int is_float, size_t nvol, const Dims& vol, const Dims& chunkPref,
                      int mode, double quality, uint8_t* d_dst, size_t dst_cap, size_t* offsets, hipStream_t st,
                      Coded what = Coded::Container);

// chunks the container of a volume has (the reference's rule, hostc::chunk_segments; SIZE_MAX: too many to count)
inline size_t container_chunk_count(const Dims& vol, const Dims& chunkPref)
{
  Dims cdim;
  for (int a = 0; a < 3; a++) {
    if (vol[a] == 0)
      return 0;
    cdim[a] = std::min(std::max<size_t>(1, chunkPref[a]), vol[a]);
  }
  return chunk_count(vol, cdim);
}

// The size mode (budget.h).  The survey: per chunk of the volume, in container order, the fixed-rate
// step q, the plane count, the plane table's row of 32 (the stream's bits at the end of plane p under an unlimited budget)
// and whether the chunk is constant -- host arrays; no stream is written
int size_survey_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, double* q, int32_t* nbp,
                   uint64_t* end, uint8_t* is_const, hipStream_t st);
// ... and a container of at most target_bytes bytes, every chunk's budget dealt by budget_deal on the survey; budgets_out
// (host, may be null): the budgets in bits.  -1, with nothing of d_dst written, when the target does not hold the headers
// and a payload byte per chunk that is not constant
int compress_size_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, size_t target_bytes,
                     uint8_t* d_dst, size_t dst_cap, size_t* dst_len, uint64_t* budgets_out, hipStream_t st);

// PSNR of the whole volume (psnr_vol.h).  The smallest and largest sample of a volume (with srcView:
// of a valid strided view) -- psnr_vol.hip; -1 when a sample is a NaN.  One wait of the host
int range_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const ViewPitch* srcView, double* vmin,
             double* vmax, hipStream_t st);
// ... and the container whose chunks all take their q from the ladder of one target: range 0 means the volume's own.
// Everything behind the q is mode 2's flow.  -1, with *dst_len and d_dst untouched, for a volume whose own range is not
// finite and when a chunk is refused by k_mse_ladder_pick
int compress_psnr_to(Engine& E, const void* d_src, int is_float, const Dims& vol, const Dims& chunkPref, double psnr,
                     double range, uint8_t* d_dst, size_t dst_cap, size_t* dst_len, hipStream_t st,
                     const ViewPitch* srcView);

// ---- stage access for the parity tests (abi_stages.hip): one stage of a chunk of the plan's shape on the caller's data
// (the encoder's stages are encode.hip's, speck3d_decode_stage is decode.hip's)
// the integer coder on coefficients of 4 or 8 bytes (wide) and their sign words: {u8 planes, u64 total_bits, payload}
int speck3d_encode_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_coef, bool wide,
                         const uint64_t* d_sign, uint64_t raw_budget, uint8_t* d_dst, size_t dst_cap, size_t* dst_len);
// the plane table of such coefficients (32-bit; 3D forests): end[p], p < 64, the stream's bits at the end of plane p under an
// unlimited budget, zeros from the plane count *nbp on (launch_speck_plane_table) -- host memory
int speck3d_plane_bits_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_coef, const uint64_t* d_sign,
                             uint64_t* end, int* nbp);
// ... and back: such a stream into coefficients and sign words; *width_out the coefficients' bytes
int speck3d_decode_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_stream, size_t stream_len,
                         void* d_coef, uint64_t* d_sign, int* width_out);
// the outlier stage of point-wise error mode on a reconstruction of the caller's: nb chunks cut along z
int outlier_encode_stage(Engine& E, hipStream_t st, const ShapePlan& P, const void* d_orig, int is_float,
                         const double* d_recon, uint32_t nb, double tol, uint8_t* d_dst, size_t dst_cap, size_t* lens);

// ------------------------------------------------------------------------------------------
// the C boundary
// ------------------------------------------------------------------------------------------
// nothing thrown by the host side (std::bad_alloc of a vector, std::system_error of a thread)
// may cross the C boundary
template <typename F>
int guarded(const char* what, F&& body) noexcept
{
  try {
    return body();
  }
  catch (const std::bad_alloc&) {
    fprintf(stderr, "[sperr_hip] %s: out of host memory\n", what);
  }
  catch (const std::exception& e) {
    fprintf(stderr, "[sperr_hip] %s: %s\n", what, e.what());
  }
  catch (...) {
    fprintf(stderr, "[sperr_hip] %s: unknown exception\n", what);
  }
  return -1;
}

}  // namespace sperrhip

#endif
