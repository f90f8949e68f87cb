// engine.hip -- host side of the HIP engine, the part both directions share: per-shape plans and their kernel choices,
// the file-scope state, the workspace budget, the brick inverse.  The encode call is encode.hip and the decode call
// decode.hip, which see this unit through engine_parts.h; the C ABI declared in include/sperr_hip.h is abi.hip and
// abi_stages.hip, which see all three through engine_core.h (types, globals, the encoder's front) and decode_request.h
// (the decoder's front).
//
// Host logic restated from the reference (file:line under /root/reference):
//   src/sperr_helper.cpp:542-592            chunk_volume (x fastest, short remainders merged)
//   src/SPERR3D_Stream_Tools.cpp:46-105     container header parsing
#include "engine_parts.h"

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
thread_local hipStream_t t_call_stream = nullptr;   // ... and the stream of its call (Lease; the poison fills)
static thread_local const char* t_prof_cur = nullptr;
static thread_local hipEvent_t t_prof_a = nullptr;
std::atomic<unsigned long long> g_dbg_counter[5];   // sperrhip_debug_counter (0..2, [3] as counter 7, [4] as counter 8)
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

}  // namespace

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
  if (P.tables.ensure(blob.bytes.size(), false))   // (constant data: not a workspace, never poisoned)
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

// ------------------------------------------------------------------------------------------
// what the encode and the decode call share (engine_parts.h)
// ------------------------------------------------------------------------------------------
// How much workspace a call may use: 80 % of what is free plus what the engine already holds --
// or SPERR_HIP_ARENA_MAX_MB when that is less (a soft cap: it bounds how many chunks of a batch
// are in flight together, one chunk is always allowed; for hosts that share the device, and for
// tests that want a volume NOT to fit).
static size_t arena_cap_env()
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

uint64_t rounded_budget(uint64_t raw)
{
  if (raw == 0)
    return ~0ull;
  while (raw % 8)
    raw++;
  return raw;
}

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

// the brick inverse (engine_parts.h says what it is and who takes it)
bool brick_inverse_fits(const ShapePlan& P, uint32_t nb, size_t valsStride)
{
  return P.schedule.brick && (uint64_t)nb * valsStride <= 0xffffffffull;
}
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
  // a chunk has fewer sets than samples (the bound of max_payload_bits, encode.hip)
  const uint64_t unlimited = (uint64_t)(130.0 * n) + 64;
  const uint64_t bits = raw ? std::min(rounded_budget(raw), unlimited) : unlimited;
  size_t total = 26 + (size_t)((bits + 7) / 8) + 8;
  if (mode == 3)   // the outlier stream: the same bound for the 1D coder over n values
    total += 9 + (size_t)((unlimited + 7) / 8);
  return total;
}

// dynamic LDS above 64 KB has to be allowed per kernel and per device
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

}  // namespace sperrhip
