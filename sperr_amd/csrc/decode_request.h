// decode_request.h -- the decoder's front (decode.hip), as the C ABI (abi.hip) calls it: what a container's header says,
// which levels and windows a container has, what one decompression call decodes and writes (DecodeRequest), and the
// calls themselves.  Internal, like engine_core.h.
#ifndef SPERR_AMD_DECODE_REQUEST_H
#define SPERR_AMD_DECODE_REQUEST_H

#include <numeric>

#include "engine_core.h"

namespace sperrhip {

// multi-resolution decoding (SPERR3D_OMP_D::decompress(p, true), src/SPERR3D_OMP_D.cpp:50-150):
// the volume at every coarsened resolution of the chunks (src/sperr_helper.cpp:70-123), coarsest
// first.  Only for dyadic chunks that tile the volume.
struct MultiRes {
  size_t nlev = 0;
  std::array<uint32_t, 3> cres[16];   // chunk resolution of level h
  std::array<uint32_t, 3> grid;       // chunks per axis
  double* d_level[16];
};

// the levels of a volume cut into chunks of cdim: m.nlev = 0 when there are none.  Returns 0
int multires_levels(const Dims& vol, const Dims& cdim, MultiRes& m);
// a slice: one level per level of dwt2d (src/sperr_helper.cpp:86-95, src/CDF97.cpp:114-130)
void multires_levels_2d(size_t dx, size_t dy, MultiRes& m);

// A window of a call's output, [lo, lo + dims), and the chunks it meets (box_chunks, chunk_volume order).  Either a
// box of the volume at full resolution (sperrhip_decompress_box_dev), or -- `level` -- a box of level h of the
// hierarchy alone, coarsest first, in the level's coordinates (sperrhip_decompress_level_dev).  The level is the grid
// of the chunks' corners of resolution cres[h], so the chunks its box meets are box_chunks of the level's dims with
// cres[h] as the chunk size.  Or, with slotGeom, the output of a boxes call (boxes.h): many boxes of either kind, the
// chunks of many containers
struct Window {
  Dims lo, dims;
  std::vector<uint32_t> ids;
  bool crop = false;    // the window is not all of what it is a window of (window_select)
  bool level = false;   // of level h of m; otherwise of the volume
  size_t h = 0;
  MultiRes m;
  // Boxes of a batch (boxes.h, sperrhip_decompress_boxes_dev): the window is the call's whole output -- nbox boxes back
  // to back, or the staging array -- and every slot brings its own geometry, BoxesPlan::geom; lo is unused and `dims`
  // the output's.  Empty: the one box [lo, lo + dims), each chunk placed by place() + crop_geom()
  std::vector<CropGeom> slotGeom;
  // what the chunk of slot `slot`, at `org` with dims `cd`, writes of the window, and where
  CropGeom geom_of(uint32_t slot, const uint32_t org[3], const uint32_t cd[3]) const
  {
    if (!slotGeom.empty())
      return slotGeom[slot];
    size_t o[3], ext[3];
    place(org, cd, o, ext);
    return crop_geom(o, ext);
  }
  // the chunk at `org` of dims `cd`, in the coordinates the window is given in: its origin and extent
  void place(const uint32_t org[3], const uint32_t cd[3], size_t o[3], size_t ext[3]) const
  {
    for (int a = 0; a < 3; a++) {
      ext[a] = level ? m.cres[h][a] : cd[a];
      o[a] = level ? org[a] / cd[a] * ext[a] : org[a];
    }
  }
  // what a chunk at `o` of extent `ext` (both as place() gives them) writes of the window, and where
  CropGeom crop_geom(const size_t o[3], const size_t ext[3]) const
  {
    CropGeom g;
    for (int a = 0; a < 3; a++) {
      const size_t hi = lo[a] + dims[a];
      g.rel[a] = (int32_t)((int64_t)o[a] - (int64_t)lo[a]);
      g.lo[a] = (uint32_t)(lo[a] > o[a] ? lo[a] - o[a] : 0);
      g.hi[a] = (uint32_t)std::min<size_t>(hi - o[a], ext[a]);
    }
    return g;
  }
};

// The box [lo, lo + dims) of a container's volume and the chunks it meets; -1 when window_select refuses it
int box_select(const ContainerInfo& ci, const size_t lo[3], const size_t dims[3], Window& w);
// Level `level` of the container `ci` describes, whole (lo and dims null) or the box [lo, lo + dims) of it, and the
// chunks it meets; -1 when the container has no such level or window_select refuses the box
int level_select(const ContainerInfo& ci, size_t level, const size_t* lo, const size_t* dims, Window& w);

// What one decompression call decodes, and what it writes: everything DecodeCall needs to know beside the container
// `ci` and the buffers.  The two halves are independent but for the pairs valid() excludes
struct DecodeRequest {
  using ChunkList = std::vector<std::array<size_t, 6>>;
  // ---- the source: where the chunks come from
  // a batch (sperrhip_decompress_batch_dev): the chunks of every container, z origins shifted into the stacked view
  // that `ci` describes -- the volume (x, y, nvol z) and every chunk's absolute offset and length (null: the chunks
  // of the one container, chunk_volume)
  const ChunkList* stacked = nullptr;
  // the chunks are slices, decoded on the 2D coder's forest: `ci` describes one chunk of dims (x, y, 1) whose stream
  // starts at d_src, or with `stacked` a batch of them, chunk s of dims (x, y, 1) at (0, 0, s)
  bool slices = false;
  // a batch of slices whose streams carry the 10-byte header (sperrhip_decompress_2d_batch_dev): ci.off points behind
  // each header; {dimx, dimy} that every header has to name (null: no headers)
  const uint32_t* sliceHdr = nullptr;
  // ---- the output: what d_dst receives
  // null: the whole volume.  A box of it: only the chunks the box meets are read and decoded, and d_dst is the box.
  // One level alone or a box of it: the same, the inverse passes stop at the level and no outlier stream is looked at
  const Window* window = nullptr;
  // beside the volume, every level of the hierarchy into levels->d_level (sperrhip_decompress_multires_dev)
  const MultiRes* levels = nullptr;
  // d_dst is the first element of a strided view (view.h; valid for the output's dims) of a larger array: the volume
  // or the box goes there, and nothing outside the view is written (sperrhip_decompress_view_dev).  null: dense
  const ViewPitch* outView = nullptr;

  // (a box that is the whole volume is no window: such a call is the whole-volume decode)
  void set_window(const Window& w) { window = (w.level || w.crop) ? &w : nullptr; }

  // every combination of source and output the decoder refuses
  bool valid() const
  {
    if (window && slices)   // a window is cut along a container's chunk grid; a slice is one chunk
      return false;
    if (window && levels)   // the side outputs are whole levels: a box reads only some chunks, a level stops before the rest
      return false;
    if (stacked && levels)   // the stacked view is no volume with a hierarchy: each container has its own
      return false;
    if (level() && stacked && window->slotGeom.empty())   // a level's grid of chunk corners is one container's: only the
      return false;                                        //   boxes call, whose slots bring their geometry, has many
    if (window && !window->slotGeom.empty() && (!stacked || window->slotGeom.size() != window->ids.size()))
      return false;   // per-slot geometry is the boxes call's, one record per chunk of its list
    if (level() && level()->h >= level()->m.nlev)   // the container has no such level
      return false;
    if (outView && (stacked || slices || levels || level()))   // a view holds one volume or a box of it at full resolution
      return false;
    return true;
  }

  // the level the inverse stops at (null: it runs to full resolution)
  const Window* level() const { return window && window->level ? window : nullptr; }
  // the chunks' windows travel to the device (DecBatchBufs::crop, the kCrop writers)
  bool cropped() const { return window && window->crop; }
  // (a level is taken before the outlier correctors are added, src/SPECK_FLT.cpp:568-603: no stream of them is read)
  bool reads_outliers() const { return !level(); }
  ChunkList chunks(const ContainerInfo& ci) const { return stacked ? *stacked : chunk_volume(ci.vol, ci.chunk); }
  // The chunks of the call, slot by slot: slot i is chunk sel[i] of chunks() (all of them in order, or the window's)
  std::vector<uint32_t> slots(size_t nchunks) const
  {
    if (window)
      return window->ids;
    std::vector<uint32_t> sel(nchunks);
    std::iota(sel.begin(), sel.end(), 0u);
    return sel;
  }
  // the output: the volume, or the window (its chunks write their pieces of it)
  // (the non-crop writers place a chunk by its origin in the volume, the crop writers by its origin relative to the
  //  box: with a view only the pitches differ)
  VolDesc out_desc(const ContainerInfo& ci) const
  {
    const Dims& d = window ? window->dims : ci.vol;
    return outView ? view_desc(*outView, d[2]) : VolDesc{{d[0], d[1], d[2]}};
  }
  // values d_dst has to hold: the output's, or with a view its extent (0: the view is not valid for the output)
  size_t out_vals(const ContainerInfo& ci) const
  {
    if (outView) {
      const Dims& d = window ? window->dims : ci.vol;
      size_t e = 0;
      return view_extent(d[0], d[1], d[2], *outView, &e) ? e : 0;
    }
    return window ? window->dims[0] * window->dims[1] * window->dims[2] : ci.nvals;
  }
};

// ---- containers on the device: their headers ...
// the header of the container of src_len bytes at d_src (SPERR3D_Stream_Tools.cpp:46-105).  0 ok
int read_container_info(const uint8_t* d_src, size_t src_len, ContainerInfo& ci, hipStream_t st);
// The headers of containers that lie anywhere: container v is the len[v] bytes at d_src + off[v], parsed into ci[v]
// (offsets relative to the container).  heads: 32 bytes per container, its first 26 (or fewer) and zeros
int read_headers_at(Engine& E, const uint8_t* d_src, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len,
                    std::vector<ContainerInfo>& ci, std::vector<uint8_t>& heads, hipStream_t st);
// The containers of a batch, container v at [offs[v], offs[v + 1]) of d_src, as the stacked view a batch decode takes
// (DecodeRequest::stacked): `all` describes the volume (x, y, nvol z), `list` its chunks
int read_batch_info(Engine& E, const uint8_t* d_src, const size_t* offs, size_t nvol, ContainerInfo& all,
                    std::vector<std::array<size_t, 6>>& list, hipStream_t st);
// ... and their truncation (sperrhip_trunc_dev / _batch_dev): each container keeps `pct` percent of every chunk stream,
// back to back into d_dst.  outOffs: nvol + 1 entries.  0 ok, 1 when d_dst is null or too small (outOffs still filled)
int trunc_impl(Engine& E, const uint8_t* d_src, const size_t* offs, size_t nvol, unsigned pct, uint8_t* d_dst,
               size_t dst_cap, size_t* outOffs, hipStream_t st);

// ---- the decode calls: d_dst takes floats or doubles as output_float says
// `req` of the container at d_src (described by `ci`) into d_dst (x fastest), which holds dst_cap_bytes
int decode_to(Engine& E, const void* d_src, int output_float, void* d_dst, size_t dst_cap_bytes,
              const ContainerInfo& ci, hipStream_t st, const DecodeRequest& req);
// the window `w` of it, once d_dst is seen to hold the window
int decode_window(Engine& E, const void* d_src, int output_float, void* d_dst, size_t dst_cap_bytes,
                  const ContainerInfo& ci, hipStream_t st, const Window& w, const ViewPitch* outView = nullptr);

// sperrhip_decompress_boxes_dev (boxes.h) on an engine the caller holds, its arguments seen to be no NULL pointers, no
// zero counts, no index of `which` beyond ncont and no zero box extent.  vol (may be null): the dims every container
// has to name
int decode_boxes_to(Engine& E, const void* const* d_srcs, const size_t* src_lens, size_t ncont, const uint32_t* which,
                    const size_t* box_lo, size_t nbox, const size_t box_dims[3], const size_t* level, unsigned pct,
                    int output_float, void* d_dst, size_t dst_cap_bytes, hipStream_t st, const Dims* vol);

}  // namespace sperrhip

#endif
