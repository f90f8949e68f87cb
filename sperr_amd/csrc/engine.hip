// engine.hip -- host side of the HIP engine: chunk grid, per-shape plans, batched workspaces,
// container assembly / parsing.  The C ABI declared in include/sperr_hip.h is abi.hip and abi_stages.hip, which see
// this unit through engine_core.h (types, globals, the encoder's front) and decode_request.h (the decoder's front).
//
// Host logic restated from the reference (file:line under /root/reference):
//   src/sperr_helper.cpp:542-592            chunk_volume (x fastest, short remainders merged)
//   src/SPERR3D_OMP_C.cpp:23-30,61-141      chunk loop  -> batches of equally shaped chunks
//   src/SPERR3D_OMP_C.cpp:145-234           container header + concatenated chunk streams
//   src/SPERR3D_Stream_Tools.cpp:46-105     container header parsing
//   src/SPERR3D_OMP_D.cpp:23-135            decompress driver
//   src/SPECK_FLT.cpp:401-541               per-chunk pipeline order and the fixed-rate retry
#include <chrono>
#include <deque>
#include <numeric>
#include <thread>

#include "decode_request.h"

// The decoder runs the shape groups of a volume side by side on up to eight streams; the ROCm
// runtime maps streams onto four hardware queues unless told otherwise, and reads the variable at
// the process's first HIP call: a host that loads this library before that gets eight.
__attribute__((constructor)) static void sperrhip_ask_for_hw_queues()
{
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
}

namespace sperrhip {

// ------------------------------------------------------------------------------------------
// profiling
// ------------------------------------------------------------------------------------------
// the file-scope state other units see (extern in engine_core.h)
// global switches (sperrhip_profile_enable / _only); the accumulators live in the engines
bool g_prof_on = false;
std::string g_prof_only;
std::mutex g_prof_cfg_mu;
thread_local Profiler* t_prof = nullptr;       // the profiler of the engine this thread drives
static thread_local const char* t_prof_cur = nullptr;
static thread_local hipEvent_t t_prof_a = nullptr;
std::atomic<unsigned long long> g_dbg_counter[4];   // sperrhip_debug_counter (0..2, and [3] as counter 7)
bool g_lis_stamps_on = false;
std::vector<uint64_t> g_lis_stamps_host;   // chunk 0 of the last decoded batch
EnginePool g_pool;

void prof_begin(const char* name, hipStream_t stream)
{
  Profiler* P = t_prof;
  if (!P || !P->on || (!P->only.empty() && P->only != name))
    return;
  std::lock_guard<std::mutex> lock(P->mu);
  if (!P->ref) {
    P->ref = P->get();
    if (P->ref)
      hipEventRecord(P->ref, stream);
  }
  t_prof_cur = name;
  t_prof_a = P->get();
  if (t_prof_a)
    hipEventRecord(t_prof_a, stream);
}

void prof_end(hipStream_t stream)
{
  Profiler* P = t_prof;
  if (!P || !P->on || !t_prof_cur)
    return;
  std::lock_guard<std::mutex> lock(P->mu);
  hipEvent_t b = P->get();
  if (b)
    hipEventRecord(b, stream);
  P->open.push_back({t_prof_cur, t_prof_a, b});
  t_prof_cur = nullptr;
}

thread_local bool t_shared_device = false;   // (engine_internal.h)

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------
namespace {

// src/Conditioner.cpp:137-163
uint32_t condi_num_strides(size_t len)
{
  const size_t dflt = 2048;
  if (len % dflt == 0)
    return (uint32_t)dflt;
  for (size_t n = dflt; n <= 32768; n++)
    if (len % n == 0)
      return (uint32_t)n;
  size_t n = dflt;
  while (len % n != 0)
    n--;
  return (uint32_t)n;
}

// ------------------------------------------------------------------------------------------
// per-shape plan: tree tables on the device, tile maps, DWT pass list
// ------------------------------------------------------------------------------------------
// The encoder's fused head (k_head_fused, speck_enc.hip) wants workgroups that own whole pixel tiles AND whole leaf sets:
// an all-octree forest (cubic power-of-two roots) whose every deepest grid is one pyramid_leaf4 takes (leaf4_block) with
// even y and z origins, rows that are a power of two with at least two of them in a pixel tile, slices that are whole
// tiles and come in pairs.  Returns the kernel's root table, empty when the shape does not qualify (256^3, 128^3 and
// 64^3 chunks do; a chunk with an axis that is no power of two, or under 64 samples a side, does not).
std::vector<FusedRoot> fused_head_roots(const spk::HostTree& h)
{
  std::vector<FusedRoot> out;
  const uint32_t dx = h.dims[0], dy = h.dims[1], dz = h.dims[2];
  if (!(h.flags & spk::kTreeAllOct) || (h.flags & spk::kTree2D) || h.roots.empty() || h.roots.size() > (size_t)spk::kMaxRoots)
    return out;
  if ((dx & (dx - 1)) != 0 || dx < 8 || dx > (uint32_t)kPixTile / 2 || ((size_t)dx * dy) % kPixTile != 0 || dz % 2 != 0)
    return out;
  uint64_t covered = 0;
  for (const spk::Root& r : h.roots) {
    const spk::Grid& g = h.grids[r.gridFirst + r.Dmax - 1];
    const uint32_t side = r.len[0];
    if (!(g.kind & spk::kGridOct) || g.e[0] < 2 || g.e[1] != g.e[0] || g.e[2] != g.e[0] || r.org[0] % 8 != 0 ||
        r.org[1] % 2 != 0 || r.org[2] % 2 != 0 || r.len[1] != side || r.len[2] != side || side != (2u << g.e[0]))
      return std::vector<FusedRoot>();
    out.push_back(FusedRoot{(uint32_t)r.org[0] | ((uint32_t)r.org[1] << 16), (uint32_t)r.org[2] | (side << 16), g.nodeOff, g.e[0]});
    covered += (uint64_t)side * side * side;
  }
  if (covered != (uint64_t)dx * dy * dz)   // (the roots are disjoint boxes: every sample has a leaf parent)
    return std::vector<FusedRoot>();
  return out;
}

struct Blob {  // host-side staging of all tables of a plan, uploaded in one copy
  std::vector<char> bytes;
  template <typename T>
  size_t add(const std::vector<T>& v)
  {
    const size_t off = round_up(bytes.size(), 256);
    bytes.resize(off + std::max<size_t>(v.size(), 1) * sizeof(T), 0);
    if (!v.empty())
      memcpy(bytes.data() + off, v.data(), v.size() * sizeof(T));
    return off;
  }
};

// ---- the rules of a shape's kernel choices: build_plan asks them once and keeps the answers (ShapePlan::schedule, ::dec) ----
// the transform starts with the full-size x pass followed by the full-size y pass (every dyadic
// shape; wavelet-packet shapes start along z), and the rows fit the fused kernel's LDS tile
static bool fuse_xy(const ShapePlan& P)
{
  if (P.fwd.size() < 2 || P.fwd[0].axis != 0 || P.fwd[1].axis != 1)
    return false;
  for (int a = 0; a < 3; a++)
    if (P.fwd[0].region[a] != P.dims[a] || P.fwd[1].region[a] != P.dims[a])
      return false;
  return lift_xy_applicable(P.dims);
}

// ... and the full-size z pass follows (every dyadic shape): all three in one kernel
static bool fuse_xyz(const ShapePlan& P)
{
  if (!fuse_xy(P) || P.fwd.size() < 3 || P.fwd[2].axis != 2)
    return false;
  for (int a = 0; a < 3; a++)
    if (P.fwd[2].region[a] != P.dims[a])
      return false;
  return lift_xyz_applicable(P.dims);
}

// LiftFuse of pass k (xform.h): the samples of its region that no LATER pass of the forward order
// touches.  The later passes' regions are boxes at the origin; when one of them contains all the
// others (dyadic plans: the next pass; wavelet-packet plans: the full-size x pass for every z pass)
// the samples are those outside it.  Returns 0 when there are none, 1 when there are (inner = that
// box), -1 when the later regions are not nested (no plan of build_plan is like that).
static int pass_fuse_rule(const ShapePlan& P, size_t k, uint32_t inner[3])
{
  const LiftPass& ps = P.fwd[k];
  inner[0] = inner[1] = inner[2] = 0;
  for (size_t j = k + 1; j < P.fwd.size(); j++)
    for (int a = 0; a < 3; a++)
      inner[a] = std::max(inner[a], P.fwd[j].region[a]);
  bool nested = k + 1 >= P.fwd.size();
  for (size_t j = k + 1; j < P.fwd.size(); j++)
    nested = nested || (P.fwd[j].region[0] == inner[0] && P.fwd[j].region[1] == inner[1] &&
                        P.fwd[j].region[2] == inner[2]);
  if (!nested)
    return -1;
  bool covers = true;
  for (int a = 0; a < 3; a++)
    covers = covers && inner[a] >= ps.region[a];
  return covers ? 0 : 1;
}
// ... as the plan keeps it (LiftSchedule::pass)
int pass_fuse(const ShapePlan& P, size_t k, uint32_t inner[3])
{
  std::copy_n(P.schedule.pass[k].inner, 3, inner);
  return P.schedule.pass[k].fuse;
}

// Can the lifting passes collect the largest coefficient / dequantise on the way?  Not when the
// fused x-y kernel of the finest level would have to (slices: their next pass is a coarser level).
static bool plan_fusable(const ShapePlan& P)
{
  if (P.fwd.empty())
    return false;
  for (const LiftSchedule::Pass& ps : P.schedule.pass)
    if (ps.fuse < 0)
      return false;
  if (P.schedule.head != LiftSchedule::kNoHead && (P.schedule.pass[0].fuse != 0 || P.schedule.pass[1].fuse != 0))
    return false;
  return true;
}

// Can the SECOND level of this shape run as one launch each way (k_lift2_fwd / k_lift2_inv, xform.h) instead of three
// per-axis passes?  Passes 3, 4 and 5 have to be x, y and z of one region -- the low halves the fused finest-level kernel
// leaves --, the region has to fit the sliding-window kernels with rows of at most 128 samples, and the passes have to
// nest (plan_fusable: the kernels tell the box's samples from the others by LiftFuse::inner).
static bool level2_fits(const ShapePlan& P)
{
  if (!P.schedule.brick || P.fwd.size() < 6)
    return false;
  for (int k = 3; k < 6; k++) {
    if (P.fwd[k].axis != k - 3)
      return false;
    for (int a = 0; a < 3; a++)
      if (P.fwd[k].region[a] != P.dims[a] - P.dims[a] / 2)
        return false;
  }
  const LiftSchedule::Pass& z = P.schedule.pass[2];
  if (z.fuse <= 0 || z.inner[0] != P.fwd[3].region[0] || z.inner[1] != P.fwd[3].region[1] ||
      z.inner[2] != P.fwd[3].region[2])
    return false;
  return lift2_applicable(P.fwd[3].region);
}
// Does it?  Decided once, when the plan is made: the encoder's launches (float_stages) and the decoder's memory layout
// and launches (decode_group, enqueue_inverse) follow it.  By default only where the region has at least kLevel2Floor
// samples along every axis, in both directions alike, because that is where it was measured to gain
// (profiles/level2_fused_ab.txt): at 128^3 (256^3 chunks) decompression gains 1.8 % run against run; at 64^3, 32^3 and
// 16^3 (128^3, 64^3, 32^3 chunks, 64 and 512 of them) compress and decompress times with and without it lie inside
// each other's spread -- the launch is no slower there, the march through the slices costs what the three launches
// cost -- with one exception, 512 chunks of 32^3, which decode 3 to 4 % faster with it.  A gain that cannot be told
// from the spread is not taken: the small shapes keep the launches they had, which tests/test_gpu_level.py pins launch
// by launch for 32^3 chunks (with the launch on, those tables would have to change: 12 k_lift_axis<false, 0> become 4
// k_lift2_inv<true>; the 32^3 decode gain above is what that would buy).  Nothing between 64 and 128 was measured; the
// floor sits midway.
// SPERR_HIP_XYZ_LEVEL2=0: the three passes everywhere, for A/B runs and tests; =2: the launch wherever it fits, for the
// same (the tests put every shape the kernels can go wrong at through them this way).  Read whenever a plan is made:
// sperrhip_release() drops the plans.
constexpr uint32_t kLevel2Floor = 96;
static bool plan_level2(const ShapePlan& P)
{
  const char* env = getenv("SPERR_HIP_XYZ_LEVEL2");
  const int sw = env ? atoi(env) : 1;
  if (sw == 0 || !level2_fits(P))
    return false;
  const uint32_t* r = P.fwd[3].region;
  return sw == 2 || std::min(r[0], std::min(r[1], r[2])) >= kLevel2Floor;
}

// The schedule of the pass list P.fwd, each answer from the ones before it
static void plan_schedule(ShapePlan& P)
{
  LiftSchedule& S = P.schedule;
  S = LiftSchedule{};
  S.pass.resize(P.fwd.size());
  for (size_t k = 0; k < P.fwd.size(); k++)
    S.pass[k].fuse = pass_fuse_rule(P, k, S.pass[k].inner);
  S.head = fuse_xyz(P) ? LiftSchedule::kHeadXYZ : fuse_xy(P) ? LiftSchedule::kHeadXY : LiftSchedule::kNoHead;
  S.fusable = plan_fusable(P);
  S.brick = S.head == LiftSchedule::kHeadXYZ && S.fusable && P.fwd.size() >= 3;
  for (size_t k = 3; k < P.fwd.size(); k++)   // (a chunk with one level of transform has no coarser pass: 1 x 1 x 1)
    for (int a = 0; a < 3; a++)
      S.coarseBox[a] = std::max(S.coarseBox[a], P.fwd[k].region[a]);
  S.level2 = plan_level2(P);
}

// the lists of the larger sets GPU-wide (k_lis_hi); SPERR_HIP_LIS_HI=0 and regular trees whose geometry
// tables do not fit the kernel's LDS go to k_lis_mx, which takes any shape (k_lis_tables, one workgroup
// per chunk, was the table kernel of rounds 1-3: removed in round 4)
constexpr int kHiMaxK = 9;   // longest class chain k_lis_hi takes (chunk dims up to 1024)
static bool use_lis_hi(const ShapePlan& P, bool tables)
{
  static const bool hiEnv = !(getenv("SPERR_HIP_LIS_HI") && atoi(getenv("SPERR_HIP_LIS_HI")) == 0);
  return hiEnv && tables && P.ht.grids.size() <= 288 && P.ht.roots.size() <= 48 &&
         P.maxK >= 1 && P.maxK <= kHiMaxK;
}
// every LIS level is regular and the table kernels (k_lis_l0 / _l1 / _hi) can take the shape
static bool use_tables(const ShapePlan& P)
{
  if (!P.ht.allRegular || P.maxK < 1)
    return false;
  return use_lis_hi(P, true);
}
// lists that mix set shapes (any chunk extent that is not a power of two, every slice): k_lis_mx (speck_mx.hip:
// rows keyed by shape class, several workgroups per chunk, only the walk serial).  SPERR_HIP_LIS_MIXED=0, and trees
// the class machinery does not take (more than 254 classes, 48 roots, 352 grids): k_lis_walk, the serial walk.
// The switch does not apply to the 2D coder's forest: only k_lis_mx has the type-I phase a slice needs, and every
// slice's forest fits it (tests/test_slice_forest_host.py).
// (k_lis_mixed, the one-workgroup-per-chunk kernel of rounds 2-3 whose formulation k_lis_mx took over, was removed
// at the end of round 4.)
static bool use_mixed(const ShapePlan& P, bool tables)
{
  static const bool mixEnv = !(getenv("SPERR_HIP_LIS_MIXED") && atoi(getenv("SPERR_HIP_LIS_MIXED")) == 0);
  const bool twoD = (P.ht.flags & spk::kTree2D) != 0;
  if ((!twoD && !mixEnv) || tables || P.ht.cls.empty() || P.ht.roots.size() > 48 || P.ht.grids.size() > 352 ||
      P.ht.mxSlot.size() != P.ht.cls.size())
    return false;
  return 2 * kMxS + 256 <= kMxRing && ((kMxS + kMxM) >> 6) + 5 <= 64 && kMxM >= 192 &&
         mx_smem_bytes(kMxS, kMxM, kMxQ) <= 138u * 1024u;   // (k_lis_mx has 21 KB of static LDS)
}
// The decoder's sweep from a plane's refinement to the next plane's census as one launch, and the plane's end with the
// next scan as another (k_pix_turn, k_dec_turn, speck_dec.hip: 14 launches a plane instead of 16, a mask word's second
// sigOld load and the read-modify-write of its plane word gone)?  Decided once, when the plan is made; the launcher
// takes it where the refinement goes through bit planes (32-bit coefficients).  By default only for chunks of at least
// kPixTurnFloor decoder tiles (256 mask words = 16384 samples each: 64 tiles = 1 Mi samples), which is where it was
// measured (profiles/pix_turn_ab.txt, 256^3 chunks: 1024 tiles).  Below that a plane's sweeps are a handful of workgroups,
// and tests/test_gpu_level.py and tests/test_gpu_lift_schedule.py pin the decoder's launches one by one for chunks of 32^3,
// 16^3, 2 x 23 x 20, 512 x 20 x 20 and for slices: at most 13 tiles.  Nothing between 13 and 64 tiles is pinned or measured.
// SPERR_HIP_PIX_TURN=0: the four kernels everywhere, for A/B runs and tests; =2: the sweep wherever it fits, for the same.
// Read whenever a plan is made: sperrhip_release() drops the plans.
constexpr uint32_t kPixTurnFloor = 64;
static bool plan_pix_turn(const ShapePlan& P)
{
  const char* env = getenv("SPERR_HIP_PIX_TURN");
  const int sw = env ? atoi(env) : 1;
  if (sw == 0)
    return false;
  const size_t decTiles = (round_up((size_t)P.N, 512) / 64 + kThreads - 1) / kThreads;   // DecBuffers::nPixTiles
  return sw == 2 || decTiles >= kPixTurnFloor;
}

// the list kernels a chunk shape takes, once its tree, its tables and its list levels are there
static DecPlanHost plan_list_kernels(const ShapePlan& P, bool tables)
{
  DecPlanHost ph{P.d_initLIS, P.d_initLen, tables, P.l0Level >= 0 && P.ht.grids.size() <= 288,
                 P.l1Level >= 0 && P.ht.grids.size() <= 288, P.maxK};
  ph.l2 = ph.l1 && P.l2Level >= 0;
  ph.hi = use_lis_hi(P, ph.tables);   // the lists of the larger sets GPU-wide
  ph.mixed = use_mixed(P, tables);
  ph.pixTurn = plan_pix_turn(P);
  return ph;
}

}  // namespace

// twoD: the plan of a slice's DECODER, with the forest of the 2D coder (spk::kTree2D)
int build_plan(ShapePlan& P, size_t dx, size_t dy, size_t dz, bool twoD)
{
  // set coordinates are packed 16 bits per axis (speck_tree.h pack_node), sample indices are 32 bits
  const unsigned __int128 samples = (unsigned __int128)dx * dy * dz;
  if (dx == 0 || dy == 0 || dz == 0 || dx > 0xffff || dy > 0xffff || dz > 0xffff || samples > (1ull << 31)) {
    fprintf(stderr, "[sperr_hip] chunk of %zu x %zu x %zu not supported (at most 65535 per axis, 2^31 samples)\n",
            dx, dy, dz);
    return -1;
  }
  P.dims[0] = (uint32_t)dx;
  P.dims[1] = (uint32_t)dy;
  P.dims[2] = (uint32_t)dz;
  P.N = (uint32_t)(dx * dy * dz);
  // (the columns of k_lis_mx only for the trees that can end up there: they cost as much as the rest of the tree)
  P.ht = spk::build_tree(dx, dy, dz, twoD, false);
  P.maxK = 0;
  for (const auto& lc : P.ht.levelClass)
    P.maxK = std::max<int>(P.maxK, lc.K);
  const bool tables = use_tables(P);
  if (!tables)
    spk::build_mx_columns(P.ht);
  const spk::HostTree& h = P.ht;
  const uint32_t nlev = h.nlevels;

  // LIS storage: level l owns [levelOff[l], levelOff[l+1]); keep room for the roots
  std::vector<uint32_t> cap(nlev), levelOff(nlev + 1, 0), initLen(nlev);
  for (uint32_t l = 0; l < nlev; l++) {
    cap[l] = std::max<uint32_t>(h.levelCap[l], (uint32_t)h.initLIS[l].size());
    levelOff[l + 1] = levelOff[l] + cap[l];
    initLen[l] = (uint32_t)h.initLIS[l].size();
  }
  P.lisEntries = levelOff[nlev] + 8;
  std::vector<uint64_t> initLIS(levelOff[nlev] ? levelOff[nlev] : 1, 0);
  for (uint32_t l = 0; l < nlev; l++)
    for (size_t k = 0; k < h.initLIS[l].size(); k++)
      initLIS[levelOff[l] + k] = h.initLIS[l][k];

  // list tiles in traversal order: deepest level first
  std::vector<uint16_t> tileLevel;
  std::vector<uint32_t> tileStart, levelFirstTile(nlev, 0), levelNumTiles(nlev, 0);
  for (uint32_t l = nlev; l-- > 0;) {
    levelFirstTile[l] = (uint32_t)tileLevel.size();
    const uint32_t nt = (cap[l] + kListTile - 1) / kListTile;
    levelNumTiles[l] = nt;
    for (uint32_t t = 0; t < nt; t++) {
      tileLevel.push_back((uint16_t)l);
      tileStart.push_back(t * kListTile);
    }
  }
  P.nListTiles = (uint32_t)tileLevel.size();

  // node blocks grouped by depth
  std::vector<uint32_t> depthBlocks;
  P.depthBlockOff.assign(h.maxDepth + 1, 0);
  for (uint32_t d = 0; d < h.maxDepth; d++) {
    P.depthBlockOff[d] = (uint32_t)depthBlocks.size();
    for (uint32_t b = 0; b < h.blockGrid.size(); b++)
      if (h.grids[h.blockGrid[b]].depth == d)
        depthBlocks.push_back(b);
  }
  P.depthBlockOff[h.maxDepth] = (uint32_t)depthBlocks.size();

  // birth-mask slots: every level that can hold sets
  std::vector<uint8_t> levelSlot(nlev, 0xff), slotLevel;
  for (uint32_t l = 0; l < nlev; l++)
    if (cap[l]) {
      levelSlot[l] = (uint8_t)slotLevel.size();
      slotLevel.push_back((uint8_t)l);
    }
  P.nSlots = (uint32_t)slotLevel.size();
  P.maxPhaseBits = (uint64_t)h.nsets + 2ull * P.N + 64;
  P.nPixTiles = (P.N + kPixTile - 1) / kPixTile;
  P.nstrides = condi_num_strides(P.N);

  // raster mask words that lie over one row of 32 leaf sets (spk::kGridLeafWord)
  std::vector<uint32_t> wordLeaf;
  for (const spk::Root& r : h.roots) {
    const spk::Grid& g = h.grids[r.gridFirst + r.Dmax - 1];
    if (!(g.kind & spk::kGridLeafWord))
      continue;
    if (wordLeaf.empty())
      wordLeaf.assign((P.N + 63) / 64, 0xffffffffu);
    for (uint32_t z = 0; z < r.len[2]; z++)
      for (uint32_t y = 0; y < r.len[1]; y++)
        for (uint32_t x = 0; x < r.len[0]; x += 64) {
          const size_t idx = ((size_t)(r.org[2] + z) * dy + r.org[1] + y) * dx + r.org[0] + x;
          const uint32_t fid = g.nodeOff + ((((z / 2) << g.e[1]) + y / 2) << g.e[0]) + x / 2;
          wordLeaf[idx / 64] = fid | (y & 1u) | ((z & 1u) << 1);
        }
  }

  // upload
  Blob blob;
  const size_t oRoots = blob.add(h.roots), oGrids = blob.add(h.grids), oTab = blob.add(h.tab),
               oBG = blob.add(h.blockGrid), oInit = blob.add(initLIS), oInitLen = blob.add(initLen),
               oLevOff = blob.add(levelOff), oTL = blob.add(tileLevel), oTS = blob.add(tileStart),
               oLFT = blob.add(levelFirstTile), oLNT = blob.add(levelNumTiles),
               oDB = blob.add(depthBlocks), oLS = blob.add(levelSlot), oSL = blob.add(slotLevel),
               oLC = blob.add(h.levelClass), oWL = blob.add(wordLeaf), oCls = blob.add(h.cls),
               oGC = blob.add(h.gridCls), oIR = blob.add(h.iRoots),
               oMS = blob.add(h.mxSlot), oMG = blob.add(h.mxLevelGroup);
  const std::vector<FusedRoot> fusedRoots = twoD ? std::vector<FusedRoot>() : fused_head_roots(h);
  const size_t oFR = blob.add(fusedRoots);
  P.l0Level = -1;   // the first non-empty list the sorting pass visits, when it holds 2x2x2 sets
  for (uint32_t l = nlev; l-- > 0;) {
    if (cap[l] == 0)
      continue;
    if (h.allRegular && h.levelClass[l].regular && h.levelClass[l].K == 1 &&
        h.levelClass[l].arity[0] == 8)
      P.l0Level = (int)l;
    break;
  }
  P.l1Level = -1;   // the next non-empty list, when it holds 4x4x4 sets made of those leaf sets
  if (P.l0Level >= 0)
    for (uint32_t l = (uint32_t)P.l0Level; l-- > 0;) {
      if (cap[l] == 0)
        continue;
      const spk::LevelClass& lc = h.levelClass[l];
      if (lc.regular && lc.K == 2 && lc.arity[0] == 8 && lc.arity[1] == 8 &&
          lc.lev[0] == (uint8_t)P.l0Level)
        P.l1Level = (int)l;
      break;
    }
  P.l2Level = -1;   // and the one after it, when it holds 8x8x8 sets made of those (SPERR_HIP_LIS_L2=0: k_lis_hi takes it)
  static const bool l2Env = !(getenv("SPERR_HIP_LIS_L2") && atoi(getenv("SPERR_HIP_LIS_L2")) == 0);
  if (P.l1Level >= 0 && l2Env)
    for (uint32_t l = (uint32_t)P.l1Level; l-- > 0;) {
      if (cap[l] == 0)
        continue;
      const spk::LevelClass& lc = h.levelClass[l];
      if (lc.regular && lc.K == 3 && lc.arity[0] == 8 && lc.arity[1] == 8 && lc.arity[2] == 8 &&
          lc.lev[0] == (uint8_t)P.l0Level && lc.lev[1] == (uint8_t)P.l1Level)
        P.l2Level = (int)l;
      break;
    }
  if (P.tables.ensure(blob.bytes.size()))
    return -1;
  HIP_CHECK(hipMemcpy(P.tables.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice));
  char* base = static_cast<char*>(P.tables.p);
  P.dtree = h.view();
  P.dtree.roots = reinterpret_cast<const spk::Root*>(base + oRoots);
  P.dtree.grids = reinterpret_cast<const spk::Grid*>(base + oGrids);
  P.dtree.tab = reinterpret_cast<const uint16_t*>(base + oTab);
  P.dtree.blockGrid = reinterpret_cast<const uint16_t*>(base + oBG);
  P.dtree.cls = reinterpret_cast<const spk::ShapeCls*>(base + oCls);
  P.dtree.gridCls = reinterpret_cast<const uint8_t*>(base + oGC);
  P.d_mxSlot = reinterpret_cast<const uint8_t*>(base + oMS);
  P.d_mxLevelGroup = reinterpret_cast<const uint8_t*>(base + oMG);
  P.d_iRoots = h.iRoots.empty() ? nullptr : reinterpret_cast<const uint64_t*>(base + oIR);
  P.d_initLIS = reinterpret_cast<const uint64_t*>(base + oInit);
  P.d_initLen = reinterpret_cast<const uint32_t*>(base + oInitLen);
  P.d_levelOff = reinterpret_cast<const uint32_t*>(base + oLevOff);
  P.d_tileLevel = reinterpret_cast<const uint16_t*>(base + oTL);
  P.d_tileStart = reinterpret_cast<const uint32_t*>(base + oTS);
  P.d_levelFirstTile = reinterpret_cast<const uint32_t*>(base + oLFT);
  P.d_levelNumTiles = reinterpret_cast<const uint32_t*>(base + oLNT);
  P.d_depthBlocks = reinterpret_cast<const uint32_t*>(base + oDB);
  P.d_levelSlot = reinterpret_cast<const uint8_t*>(base + oLS);
  P.d_slotLevel = reinterpret_cast<const uint8_t*>(base + oSL);
  P.d_levelClass = reinterpret_cast<const spk::LevelClass*>(base + oLC);
  P.d_wordLeaf = wordLeaf.empty() ? nullptr : reinterpret_cast<const uint32_t*>(base + oWL);
  P.d_fusedRoots = fusedRoots.empty() ? nullptr : reinterpret_cast<const FusedRoot*>(base + oFR);

  // DWT pass list (src/CDF97.cpp:132-139,170-225,284-292,387-429); the inverse runs it backwards
  P.fwd.clear();
  size_t levels = 0;
  auto approx = [](size_t len, size_t lev) { return (uint32_t)spk::approx_detail_len(len, lev)[0]; };
  if (spk::can_use_dyadic({dx, dy, dz}, levels)) {
    for (size_t lev = 0; lev < levels; lev++) {
      LiftPass ps{0, {approx(dx, lev), approx(dy, lev), approx(dz, lev)}};
      for (int a = 0; a < 3; a++) {
        ps.axis = a;
        P.fwd.push_back(ps);
      }
    }
  }
  else {
    const size_t nz = spk::num_of_xforms(dz), nxy = spk::num_of_xforms(std::min(dx, dy));
    for (size_t lev = 0; lev < nz; lev++)
      P.fwd.push_back({2, {(uint32_t)dx, (uint32_t)dy, approx(dz, lev)}});
    for (size_t lev = 0; lev < nxy; lev++) {
      P.fwd.push_back({0, {approx(dx, lev), approx(dy, lev), (uint32_t)dz}});
      P.fwd.push_back({1, {approx(dx, lev), approx(dy, lev), (uint32_t)dz}});
    }
  }
  plan_schedule(P);
  P.dec = plan_list_kernels(P, tables);
  return 0;
}

namespace {

// How much workspace a call may use: 80 % of what is free plus what the engine already holds --
// or SPERR_HIP_ARENA_MAX_MB when that is less (a soft cap: it bounds how many chunks of a batch
// are in flight together, one chunk is always allowed; for hosts that share the device, and for
// tests that want a volume NOT to fit).
size_t arena_cap_env()
{
  const char* v = getenv("SPERR_HIP_ARENA_MAX_MB");   // read per call: a test changes it
  return v ? (size_t)std::max(1ll, atoll(v)) << 20 : ~size_t(0);
}
// SPERR_HIP_ARENA_DEBUG=1: every array of a batch's workspace with its size, on stderr
bool arena_debug()
{
  static const bool on = getenv("SPERR_HIP_ARENA_DEBUG") && atoi(getenv("SPERR_HIP_ARENA_DEBUG")) != 0;
  return on;
}
size_t arena_room(size_t have, size_t freeNow)
{
  return std::min((size_t)((freeNow + have) * 0.80), arena_cap_env());
}
size_t arena_budget(size_t have, size_t freeNow)
{
  return std::min(std::max(have, (size_t)((freeNow + have) * 0.80)), arena_cap_env());
}

// bytes of workspace one chunk of this shape needs
struct EncSizes {
  size_t streamWords, maskWords, perChunk;
};

uint64_t rounded_budget(uint64_t raw)
{
  if (raw == 0)
    return ~0ull;
  while (raw % 8)
    raw++;
  return raw;
}

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
// compression
// ------------------------------------------------------------------------------------------
struct ChunkRef {
  uint32_t gid;
  uint32_t org[3];
};

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

// list storage of the 1D coder: level l holds at most 2^l runs, and never more than `most`
void speck1d_level_offsets(OutlierBufs& ob, uint32_t N, uint64_t most)
{
  ob.nlists = (uint32_t)spk::num_of_partitions(N) + 1;
  uint64_t off = 0;
  for (uint32_t l = 0; l <= (uint32_t)kO1MaxLevels; l++) {
    ob.levelOff[l] = (uint32_t)std::min<uint64_t>(off, 0xffffffffull);
    if (l < ob.nlists)
      off += l < 40 ? std::min<uint64_t>(1ull << l, most) : most;
  }
  ob.runStride = round_up((size_t)off + 64, 64);
}

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
// The brick inverse: what a decoder reconstructs of a batch, in the conditioned domain, as doubles in the chunk buffer
// -- for the encoder's point-wise error stage and for the decoder's outlier correctors, which both need the values
// before the mean is added.  By the decoder's own fused kernels: the coarser levels (passes k >= 3) in a compact
// buffer of their box, dequantising as they load (LiftFuse mode 2), the finest level by k_lift_xyz_inv writing doubles
// into the chunk buffer as if it were a volume of bricks (a chunk's offset rides in org[0], hence the 32-bit guard; no
// mean added) -- instead of an inverse quantiser pass and fifteen per-axis passes over the whole chunk (14.9 of the
// 56 ms a 1024^3 volume took to compress in PWE mode; 12.7 ms for 64 chunks of 256^3 with correctors to decode).
// Never the second level as one launch: the box is one buffer, and k_lift2_inv cannot work in place.
// A caller adds its own conditions to brick_inverse_fits: no chunk of the batch may have 64-bit coefficients.
bool brick_inverse_fits(const ShapePlan& P, uint32_t nb, size_t valsStride)
{
  return P.schedule.brick && (uint64_t)nb * valsStride <= 0xffffffffull;
}
// box: the engine's buffer for the coarser levels' box and the bricks; bricks: the host copy of the latter, which has
// to live until the stream has taken it
int enqueue_brick_inverse(hipStream_t st, const ShapePlan& P, DevBuf& box, std::vector<ChunkGeom>& bricks, uint32_t nb,
                          double* vals, size_t valsStride, CoderState* cst, const ChunkGeom* geom, const DequantSrc& src)
{
  const uint32_t* cd = P.dims;
  const uint32_t* cbox = P.schedule.coarseBox;
  const size_t boxStride = round_up((size_t)cbox[0] * cbox[1] * cbox[2], 64);
  const size_t geomOff = round_up((size_t)nb * boxStride * 8, 256);
  if (box.ensure(geomOff + (size_t)nb * sizeof(ChunkGeom) + 256))
    return -1;
  double* boxVals = static_cast<double*>(box.p);
  ChunkGeom* d_bricks = reinterpret_cast<ChunkGeom*>(static_cast<char*>(box.p) + geomOff);
  bricks.assign(nb, ChunkGeom{});
  for (uint32_t i = 0; i < nb; i++)
    bricks[i].org[0] = (uint32_t)((size_t)i * valsStride);
  HIP_CHECK(hipMemcpyAsync(d_bricks, bricks.data(), nb * sizeof(ChunkGeom), hipMemcpyHostToDevice, st));
  auto fuse = [&](size_t k, LiftFuse& lf) {
    if (pass_fuse(P, k, lf.inner) > 0) {
      lf.mode = 2;
      lf.src = src;
    }
    lf.bufx = cbox[0];
    lf.bufy = cbox[1];
  };
  for (size_t k = P.fwd.size(); k-- > 3;) {
    const LiftPass& ps = P.fwd[k];
    LiftFuse lf;
    fuse(k, lf);
    if (launch_lift(st, false, boxVals, boxStride, nb, cd, ps.axis, ps.region, cst, 0, nullptr, VolDesc{}, geom, &lf))
      return -1;
  }
  LiftFuse lf;
  fuse(2, lf);
  lf.noMean = 1;
  const VolDesc brickVol{{cd[0], cd[1], cd[2]}};   // (rows of cx samples, slices of cx * cy: a brick)
  return launch_lift_xyz(st, false, boxVals, boxStride, nb, cd, cst, 2, vals, brickVol, d_bricks, &lf);
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

}  // namespace

// Work queued by a call that fails must not outlive the call: the caller's buffers and the engine's arena are
// reused as soon as it returns.  A call (EncodeCall, DecodeCall) that did not end well waits for the caller's stream
// and the engine's in its destructor, before its members -- the host buffers queued copies read and write -- go.
void drain_after_error(Engine& E, hipStream_t st)
{
  (void)hipStreamSynchronize(st);
  for (uint32_t q = 0; q < kSubStreams; q++)
    for (hipStream_t s : {E.sub[q], E.outlQ[q], E.sideQ[q]})
      if (s)
        (void)hipStreamSynchronize(s);
  (void)hipGetLastError();
  E.pweLastStream = nullptr;
}

namespace {

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
      const uint32_t parts = (mode == 1 && !slice && n >= partsMin && n <= 512) ? std::min<uint32_t>(std::min<uint32_t>(partsEnv, n / 4), kSubStreams) : 1u;
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
      const uint64_t raw = (uint64_t)(bpp * (double)P->N);
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
    sideBySide = mode == 1 && !slice && groups.size() > 1;
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
    const uint64_t raw_budget = (uint64_t)(bpp * (double)P->N);  // SPECK_FLT.cpp:491
    // (point-wise error mode: the coder's arrays get memory of their own -- 127 MB more per 256^3 chunk --, so that the
    //  outlier stage's reconstruction can be written into the chunk buffer while the coder runs, see below)
    const bool encAlias = mode != 3;
    const size_t per = enc_bytes_per_chunk(*P, raw_budget, encAlias);
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const size_t budgetBytes = arena_budget(E.arena.n, fr);
    uint32_t B = (uint32_t)std::min<size_t>(refs.size(), std::max<size_t>(1, budgetBytes / per));
    B = std::min<uint32_t>(B, 256);
    if (sideBySide)
      B = (uint32_t)refs.size();
    else if (E.arena.ensure(std::max((size_t)B * per, enc_bytes_for(*P, B, raw_budget, encAlias)) + 4096))
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
    b.hc.resize(nb);
    HIP_CHECK(hipMemcpyAsync(b.hc.data(), b.bb.eb.cst, nb * sizeof(CoderState), hipMemcpyDeviceToHost, b.ss));
    HIP_CHECK(hipStreamSynchronize(b.ss));
    bool retry = false;
    for (auto& c : b.hc)
      retry |= (c.need_retry != 0);
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
    if (float_stages<T>(b.ss, *b.P, bb, nb, b.P->dims, d_src, vd, b.orgAligned, mode == 2))
      return -1;
    if (launch_maxabs_q(b.ss, bb.vals, bb.valsStride, nb, b.P->N, e.cst, b.P->schedule.fusable))
      return -1;
    if (mode == 2 && psnr_q_search(b.ss, *b.P, bb, nb, quality, hcKeep.emplace_back(), hcKeep.emplace_back()))
      return -1;
    if (mode == 3 && pwe_q_setup(b.ss, bb, nb, quality, hcKeep.emplace_back(), pweWide))
      return -1;
    if (bb.fusedHead) {
      // quantiser, leaf level of the pyramid and census in one kernel: the fills first (M, E and leafDesc, which the
      // kernel writes, have memory of their own; what else lies over the chunk buffer is written after it)
      if (reset_enc_pass(b.ss, bb, nb, true))
        return -1;
      const EncPlanHost ph{b.P->d_initLIS, b.P->d_initLen, b.P->d_depthBlocks, b.P->depthBlockOff, b.P->ht.nsets};
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
    if (bb.aliased && wide_retry_prepare<T>(b.ss, E, *b.P, bb, b.nb, b.P->dims, d_src, vd, b.orgAligned, mode == 2))
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

// dynamic LDS above 64 KB has to be allowed per kernel and per device
std::vector<std::array<size_t, 6>> host_chunk_volume(const Dims3& vol, const Dims3& chunk)
{
  return chunk_volume(vol, chunk);
}

int host_parse_container(const uint8_t* p, size_t len, HostContainer& out)
{
  if (len < 18)
    return -1;
  ContainerInfo ci;
  size_t need = 0;
  if (parse_container_host(p, len, len, ci, &need) != 0)
    return -1;
  out.vol = ci.vol;
  out.chunk = ci.chunk;
  out.nvals = ci.nvals;
  out.is_float = ci.is_float;
  out.multi = ci.multi;
  out.portion = (p[1] & 0x80) != 0;
  out.off = std::move(ci.off);
  out.len = std::move(ci.len);
  return 0;
}

size_t host_chunk_stream_bound(size_t nvals, int mode, double quality)
{
  const double n = (double)nvals;
  const uint64_t raw = mode == 1 ? (uint64_t)(quality * n) : 0;
  // without a budget every plane is coded: at most 66 bits per sample and 64 tests per set, and
  // a chunk has fewer sets than samples (the bound of max_payload_bits, engine-side)
  const uint64_t unlimited = (uint64_t)(130.0 * n) + 64;
  const uint64_t bits = raw ? std::min(rounded_budget(raw), unlimited) : unlimited;
  size_t total = 26 + (size_t)((bits + 7) / 8) + 8;
  if (mode == 3)   // the outlier stream: the same bound for the 1D coder over n values
    total += 9 + (size_t)((unlimited + 7) / 8);
  return total;
}

int set_max_dyn_lds(const void* fn, int bytes)
{
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> done;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find({dev, fn});
  if (it != done.end() && it->second >= bytes)
    return 0;
  HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done[{dev, fn}] = bytes;
  return 0;
}

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

// f(float{}) or f(double{}): the element type an entry point's is_float / output_float names
template <typename F>
int with_elem(int is_float, F&& f)
{
  return is_float ? f(float{}) : f(double{});
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
