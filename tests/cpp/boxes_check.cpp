// Host check of sperr_amd/csrc/boxes.h, the one statement of what a boxes call decodes and writes: for a few hundred
// seeded plans -- volumes with merged remainders, chunk dims that do not divide, containers with different chunk
// dims, a level of a dyadic container -- that the pairs' windows tile every entry's box exactly once, that every
// window lies inside its slot's extent, that the slots are distinct and in the stated order, that `shared` holds
// exactly when some slot has two pairs, that the staging z offsets are disjoint and in order, that the geometry of
// either form puts every sample where it belongs (the crop writers' address rule and k_boxes_copy's, walked on the
// host), and that the direct geometry of a single entry is what Window::place + crop_geom give for that box.  Then the
// refusals, the INT32_MAX and 2^32 ones among them.  tests/test_boxes_host.py builds it under the address and
// undefined sanitizers and runs it; it prints "boxes_check ok" and returns 0 when everything holds.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "boxes.h"

using namespace sperrhip;

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      failures++;                                                  \
    }                                                              \
  } while (0)

// what sample (x, y, z) of the grid of container c is called in this check
static uint64_t name_of(size_t c, size_t x, size_t y, size_t z)
{
  return ((uint64_t)(c + 1) << 48) | ((uint64_t)z << 32) | ((uint64_t)y << 16) | (uint64_t)x;
}

// one plan: every property, and both ways of filling the output walked sample by sample
static void check_plan(size_t ncont, const Dims& full, const std::vector<Dims>& cell, const std::vector<uint32_t>& which,
                       const std::vector<size_t>& lo, const Dims& box)
{
  const size_t nbox = lo.size() / 3;
  BoxesPlan P;
  const bool ok = boxes_plan(ncont, full, cell.data(), which.empty() ? nullptr : which.data(), lo.data(), nbox, box, P);
  CHECK(ok);
  if (!ok)
    return;
  auto cont_of = [&](size_t e) { return which.empty() ? e : (size_t)which[e]; };
  CHECK(P.nbox == nbox && P.box == box && P.outVals == box[0] * box[1] * box[2] * nbox);
  CHECK((P.outDims == Dims{box[0], box[1], box[2] * nbox}));
  CHECK(P.geom.size() == P.slots.size());
  // slots: distinct, ascending by (container, id), each the cell chunk_volume lists under that id
  for (size_t k = 0; k < P.slots.size(); k++) {
    const BoxesSlot& s = P.slots[k];
    if (k)
      CHECK(P.slots[k - 1].cont < s.cont || (P.slots[k - 1].cont == s.cont && P.slots[k - 1].id < s.id));
    const auto cv = hostc::chunk_volume(full, cell[s.cont]);
    CHECK(s.id < cv.size());
    if (s.id < cv.size())
      for (int a = 0; a < 3; a++)
        CHECK(s.org[a] == cv[s.id][2 * a] && s.ext[a] == cv[s.id][2 * a + 1]);
  }
  // pairs: in entry order, inside their slot, of the entry's container; shared exactly when a slot has two
  std::vector<size_t> uses(P.slots.size(), 0);
  std::vector<uint32_t> seen(P.outVals, 0);
  for (size_t i = 0; i < P.pairs.size(); i++) {
    const BoxesPair& p = P.pairs[i];
    CHECK(p.entry < nbox && p.slot < P.slots.size());
    if (i)
      CHECK(P.pairs[i - 1].entry <= p.entry);
    const BoxesSlot& s = P.slots[p.slot];
    CHECK(s.cont == cont_of(p.entry));
    uses[p.slot]++;
    for (int a = 0; a < 3; a++) {
      CHECK(p.lo[a] < p.hi[a] && p.hi[a] <= s.ext[a]);
      CHECK(p.at[a] + (p.hi[a] - p.lo[a]) <= box[a]);
      CHECK(s.org[a] + p.lo[a] == lo[3 * p.entry + a] + p.at[a]);   // the window is the same samples on both sides
    }
    for (size_t z = 0; z < p.hi[2] - p.lo[2]; z++)
      for (size_t y = 0; y < p.hi[1] - p.lo[1]; y++)
        for (size_t x = 0; x < p.hi[0] - p.lo[0]; x++)
          seen[((p.entry * box[2] + p.at[2] + z) * box[1] + p.at[1] + y) * box[0] + p.at[0] + x]++;
  }
  bool tiled = true, anyTwo = false;
  for (uint32_t n : seen)
    tiled = tiled && n == 1;
  CHECK(tiled);   // the windows tile every entry's box exactly once
  for (size_t n : uses) {
    CHECK(n >= 1);
    anyTwo = anyTwo || n > 1;
  }
  CHECK(P.shared == anyTwo);
  CHECK(P.shared == (P.slots.size() < P.pairs.size()));
  // what the output has to hold
  std::vector<uint64_t> want(P.outVals), out(P.outVals, 0);
  for (size_t e = 0; e < nbox; e++)
    for (size_t z = 0; z < box[2]; z++)
      for (size_t y = 0; y < box[1]; y++)
        for (size_t x = 0; x < box[0]; x++)
          want[((e * box[2] + z) * box[1] + y) * box[0] + x] =
              name_of(cont_of(e), lo[3 * e] + x, lo[3 * e + 1] + y, lo[3 * e + 2] + z);
  // the crop writers' rule (crop_has / crop_addr, lift_dev.h): sample (x, y, z) of a chunk inside [lo, hi) goes to
  // ((rel[2] + z) * dims[1] + rel[1] + y) * dims[0] + rel[0] + x of an array of dims `dims`
  auto write_slots = [&](const Dims& dims, std::vector<uint64_t>& arr, std::vector<uint32_t>& hits) {
    for (size_t k = 0; k < P.slots.size(); k++) {
      const BoxesSlot& s = P.slots[k];
      const BoxCrop& g = P.geom[k];
      for (uint32_t z = g.lo[2]; z < g.hi[2]; z++)
        for (uint32_t y = g.lo[1]; y < g.hi[1]; y++)
          for (uint32_t x = g.lo[0]; x < g.hi[0]; x++) {
            const int64_t ox = (int64_t)g.rel[0] + x, oy = (int64_t)g.rel[1] + y, oz = (int64_t)g.rel[2] + z;
            const bool in = ox >= 0 && oy >= 0 && oz >= 0 && (size_t)ox < dims[0] && (size_t)oy < dims[1] &&
                            (size_t)oz < dims[2];
            CHECK(in);
            if (!in)
              return;
            const size_t at = ((size_t)oz * dims[1] + (size_t)oy) * dims[0] + (size_t)ox;
            arr[at] = name_of(s.cont, s.org[0] + x, s.org[1] + y, s.org[2] + z);
            hits[at]++;
          }
    }
  };
  if (!P.shared) {
    std::vector<uint32_t> hits(P.outVals, 0);
    write_slots(P.outDims, out, hits);
    bool once = true;
    for (uint32_t n : hits)
      once = once && n == 1;
    CHECK(once);
    CHECK(out == want);
    CHECK(P.stageVals == 0);
    return;
  }
  // staged: slot k whole at (0, 0, z_k), the z ranges disjoint and in order; then the copy as k_boxes_copy walks it
  size_t z = 0, mx = 0, my = 0;
  for (const BoxesSlot& s : P.slots) {
    CHECK(s.stageZ == z);
    z += s.ext[2];
    mx = std::max(mx, s.ext[0]);
    my = std::max(my, s.ext[1]);
  }
  CHECK((P.stageDims == Dims{mx, my, z}) && P.stageVals == mx * my * z);
  std::vector<uint64_t> stage(P.stageVals, 0);
  std::vector<uint32_t> hits(P.stageVals, 0);
  write_slots(P.stageDims, stage, hits);
  bool atMostOnce = true;
  for (uint32_t n : hits)
    atMostOnce = atMostOnce && n <= 1;
  CHECK(atMostOnce);
  std::vector<BoxesCopyPair> cp;
  std::vector<uint64_t> first;
  BoxesCopyGeom g;
  boxes_copy_args(P, cp, first, g);
  CHECK(g.total == P.outVals && g.npairs == P.pairs.size() && first.size() == cp.size() + 1);
  std::vector<uint32_t> wrote(P.outVals, 0);
  for (size_t p = 0; p < cp.size(); p++)
    for (uint64_t i = first[p]; i < first[p + 1]; i++) {
      const BoxesCopyPair& c = cp[p];
      const uint64_t r = i - first[p], x = r % c.w[0], row = r / c.w[0], y = row % c.w[1], zz = row / c.w[1];
      const uint64_t s = c.src + zz * g.srcSlice + y * g.srcRow + x, d = c.dst + zz * g.dstSlice + y * g.dstRow + x;
      const bool in = zz < c.w[2] && s < stage.size() && d < out.size();
      CHECK(in);
      if (!in)
        return;
      out[d] = stage[s];
      wrote[d]++;
    }
  bool once = true;
  for (uint32_t n : wrote)
    once = once && n == 1;
  CHECK(once);
  CHECK(out == want);
  // the 16-byte form is chosen only where every row of every window allows it
  for (size_t esz : {size_t(4), size_t(8)}) {
    const size_t pack = kBoxesPackBytes / esz;
    bool all = g.srcRow % pack == 0 && g.srcSlice % pack == 0 && g.dstRow % pack == 0 && g.dstSlice % pack == 0;
    for (const BoxesCopyPair& c : cp)
      all = all && c.src % pack == 0 && c.dst % pack == 0 && c.w[0] % pack == 0;
    CHECK(boxes_vec_ok(0x1000, 0x2000, cp, g, esz) == all);
    CHECK(!boxes_vec_ok(0x1004, 0x2000, cp, g, esz) && !boxes_vec_ok(0x1000, 0x2008, cp, g, esz));
  }
}

// The rule of a single box as the decoder has had it (Window::place + crop_geom, decode_request.h), written out again: a
// chunk at origin o of extent ext and the box [lo, lo + dims) give rel = o - lo, lo = max(lo - o, 0) and
// hi = min(lo + dims - o, ext)
static void check_single_entry(const Dims& full, const Dims& cell, const Dims& lo, const Dims& box)
{
  BoxesPlan P;
  const bool ok = boxes_plan(1, full, &cell, nullptr, lo.data(), 1, box, P);
  CHECK(ok);
  if (!ok)
    return;
  std::vector<uint32_t> ids;
  CHECK(hostc::box_chunks(full, cell, lo, box, ids));
  CHECK(!P.shared && P.slots.size() == ids.size() && P.pairs.size() == ids.size());
  const auto cv = hostc::chunk_volume(full, cell);
  for (size_t k = 0; k < P.slots.size() && k < ids.size(); k++) {
    CHECK(P.slots[k].id == ids[k] && P.slots[k].cont == 0);   // (box_chunks lists ids in ascending order)
    const auto& c = cv[ids[k]];
    for (int a = 0; a < 3; a++) {
      const size_t o = c[2 * a], ext = c[2 * a + 1], hi = lo[a] + box[a];
      CHECK(P.geom[k].rel[a] == (int32_t)((int64_t)o - (int64_t)lo[a]));
      CHECK(P.geom[k].lo[a] == (uint32_t)(lo[a] > o ? lo[a] - o : 0));
      CHECK(P.geom[k].hi[a] == (uint32_t)std::min<size_t>(hi - o, ext));
    }
  }
}

static void check_seeded()
{
  std::mt19937_64 rng(20261020);
  auto pick = [&](size_t lo, size_t hi) { return lo + (size_t)(rng() % (hi - lo + 1)); };
  int plans = 0;
  for (int t = 0; t < 360; t++) {
    Dims full{pick(1, 40), pick(1, 40), pick(1, 40)};
    const size_t ncont = pick(1, 4);
    std::vector<Dims> cell(ncont);
    const int kind = t % 3;   // 0: chunk dims that differ and do not divide; 1: one chunk dims; 2: a level's grid
    if (kind == 2) {          // a level of a dyadic container: the cells divide the level's dims
      const Dims cr{pick(1, 8), pick(1, 8), pick(1, 8)};
      full = Dims{cr[0] * pick(1, 5), cr[1] * pick(1, 5), cr[2] * pick(1, 5)};
      cell.assign(ncont, cr);
    }
    else
      for (size_t c = 0; c < ncont; c++)
        cell[c] = (kind == 1 && c) ? cell[0] : Dims{pick(1, 17), pick(1, 17), pick(1, 17)};
    const Dims box{pick(1, full[0]), pick(1, full[1]), pick(1, full[2])};
    std::vector<uint32_t> which;
    size_t nbox = ncont;
    if (t % 4) {   // entries with repeating containers: shared chunks are likely
      nbox = pick(1, 7);
      for (size_t e = 0; e < nbox; e++)
        which.push_back((uint32_t)pick(0, ncont - 1));
    }
    std::vector<size_t> lo;
    for (size_t e = 0; e < nbox; e++)
      for (int a = 0; a < 3; a++)
        lo.push_back(t % 5 == 0 && e ? lo[a] : pick(0, full[a] - box[a]));   // (every fifth: one origin for all)
    check_plan(ncont, full, cell, which, lo, box);
    check_single_entry(full, cell[0], Dims{lo[0], lo[1], lo[2]}, box);
    plans++;
  }
  CHECK(plans >= 300);
  // the shapes the GPU tests use: merged remainders of 40 x 48 x 56 in 32^3, and crops that share chunks of 64^3
  const Dims v1{56, 48, 40}, c32{32, 32, 32};
  check_plan(2, v1, {c32, c32}, {}, {0, 0, 0, 0, 0, 0}, v1);
  check_plan(2, v1, {c32, c32}, {}, {33, 30, 31, 33, 30, 31}, Dims{9, 17, 8});
  check_plan(3, Dims{64, 64, 64}, {c32, c32, c32}, {0, 1, 0, 2}, {3, 9, 20, 0, 0, 0, 3, 9, 20, 40, 44, 47},
             Dims{24, 20, 17});
}

static void check_refusals()
{
  const Dims full{64, 64, 64}, c32{32, 32, 32}, box{8, 8, 8};
  const Dims cells[2] = {c32, c32};
  const size_t lo2[6] = {0, 0, 0, 8, 8, 8};
  const uint32_t w01[2] = {0, 1}, w02[2] = {0, 2};
  BoxesPlan P;
  CHECK(boxes_plan(2, full, cells, nullptr, lo2, 2, box, P));
  CHECK(boxes_plan(2, full, cells, w01, lo2, 2, box, P));
  CHECK(!boxes_plan(0, full, cells, nullptr, lo2, 0, box, P));                 // no containers
  CHECK(!boxes_plan(2, full, cells, w01, lo2, 0, box, P));                     // no entries
  CHECK(!boxes_plan(2, full, cells, nullptr, lo2, 1, box, P));                 // which == NULL and nbox != ncont
  CHECK(!boxes_plan(2, full, cells, w02, lo2, 2, box, P));                     // an index out of range
  CHECK(!boxes_plan(2, full, cells, nullptr, lo2, 2, Dims{8, 0, 8}, P));       // an extent of 0
  CHECK(!boxes_plan(2, full, cells, nullptr, lo2, 2, Dims{8, 8, 57}, P));      // entry 1 leaves the volume
  CHECK(boxes_plan(2, full, cells, nullptr, lo2, 2, Dims{8, 8, 56}, P));
  const size_t far[6] = {0, 0, 0, 64, 0, 0};
  CHECK(!boxes_plan(2, full, cells, nullptr, far, 2, Dims{1, 1, 1}, P));       // an origin outside
  const Dims zero[2] = {c32, Dims{32, 0, 32}};
  CHECK(!boxes_plan(2, full, zero, nullptr, lo2, 2, box, P));                  // a cell extent of 0
  CHECK(!boxes_plan(2, full, nullptr, nullptr, lo2, 2, box, P) && !boxes_plan(2, full, cells, nullptr, nullptr, 2, box, P));
  // nbox * bz beyond INT32_MAX: three boxes of 2^30 slices of one sample (one cell: nothing large is listed)
  {
    const Dims tall{1, 1, size_t(1) << 30}, cell1[1] = {tall};
    const uint32_t w3[3] = {0, 0, 0};
    const size_t lo3[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(!boxes_plan(1, tall, cell1, w3, lo3, 3, tall, P));
    const uint32_t w1[1] = {0};
    CHECK(boxes_plan(1, tall, cell1, w1, lo3, 1, tall, P) && !P.shared && P.outVals == (size_t(1) << 30));
    const Dims wide{(size_t(1) << 31), 1, 1}, cellw[1] = {wide};
    CHECK(!boxes_plan(1, wide, cellw, w1, lo3, 1, wide, P));                   // a box dim beyond INT32_MAX
  }
  // the staging array's z extent beyond INT32_MAX: 2^16 cells of 65535 slices each, met by two entries
  {
    const Dims vol{size_t(1) << 16, 1, 65535}, cell1[1] = {Dims{1, 1, 65535}};
    const uint32_t w2[2] = {0, 0}, w1[1] = {0};
    const size_t lo[6] = {0, 0, 0, 0, 0, 0};
    CHECK(!boxes_plan(1, vol, cell1, w2, lo, 2, vol, P));
    CHECK(boxes_plan(1, vol, cell1, w1, lo, 1, vol, P) && !P.shared && P.slots.size() == (size_t(1) << 16));
  }
  // more than 2^32 - 1 pairs: three entries that each meet 2^31 cells -- refused before a pair is listed
  {
    const Dims vol{2048, 2048, 512}, cell1[1] = {Dims{1, 1, 1}};
    const uint32_t w3[3] = {0, 0, 0};
    const size_t lo[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(!boxes_plan(1, vol, cell1, w3, lo, 3, vol, P));
    CHECK(!boxes_plan(size_t(1) << 32 | 1, vol, cell1, w3, lo, 3, vol, P));    // more containers than 32 bits index
  }
}

int main()
{
  check_seeded();
  check_refusals();
  if (failures) {
    std::fprintf(stderr, "boxes_check: %d failures\n", failures);
    return 1;
  }
  std::printf("boxes_check ok\n");
  return 0;
}
