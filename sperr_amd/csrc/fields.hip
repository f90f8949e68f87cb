// fields.hip -- the two kernels that move interleaved fields of a device array (fields.h: the layout, the constants
// and the LDS slot map) to and from stacked volumes, which is what the batch calls take and return.
//
//   k_fields_gather<T, kVec>    interleaved -> stacked
//   k_fields_scatter<T, kVec>   stacked -> interleaved; writes nothing but selected fields of samples inside the dims
//
// A workgroup of kFieldsTileX threads takes kFieldsTileX x positions of one (y, z) row: on the interleaved side a
// contiguous span of at most kFieldsTileX * stride_x elements, on the stacked side kFieldsTileX consecutive values
// of every selected field.  Both sides are read and written with consecutive lanes on consecutive addresses; the
// transposition happens in LDS, whose image of the span is skewed by fields_lds_slot().  Blocks are (tile, y) along
// x of the grid and walk z along y of the grid.
//
// kVec moves 16-byte packs on both sides; the host chooses it once per call (fields_vec_ok, and for the scatter
// nfields == stride_x as well: a pack stored into a subset would write a neighbour's bytes).  The other form moves
// element by element, needs the alignment of T only, and is also the one that takes records wider than
// kFieldsMaxLdsStride: its lanes then move the selected pieces directly, without LDS.
// Inside a tile every index is 32-bit (a span has at most kFieldsTileX * kFieldsMaxLdsStride elements); only the row
// bases are 64-bit.
#include "common.h"
#include "fields.h"

namespace sperrhip {

namespace {

struct FieldsGeom {
  uint64_t pitch_y, pitch_z;   // of the interleaved array, elements
  uint64_t vol;                // elements of one stacked volume
  uint32_t stride_x, nfields, dimx, dimy, dimz, tilesX;
};

template <typename T>
struct FieldsPack;
template <>
struct FieldsPack<float> {
  typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct FieldsPack<double> {
  typedef double type __attribute__((ext_vector_type(2)));
};

// where a block stands: its tile's first x, the x positions it holds, and the two row bases
struct FieldsTile {
  uint32_t y, x0, nx;
};

__device__ inline FieldsTile fields_tile(const FieldsGeom& g)
{
  const uint32_t y = blockIdx.x / g.tilesX, t = blockIdx.x - y * g.tilesX;
  const uint32_t x0 = t * kFieldsTileX;
  return FieldsTile{y, x0, min(kFieldsTileX, g.dimx - x0)};
}

// pack p of the stacked side of a tile: the field it belongs to and its index in the field's run of nxq packs
__device__ inline void fields_pack_of(uint32_t p, uint32_t nx, uint32_t nxq, uint32_t fullq, uint32_t& f, uint32_t& xq)
{
  if (nx == kFieldsTileX) {   // (fullq: a power of two)
    f = p / fullq;
    xq = p % fullq;
  }
  else {
    f = p / nxq;
    xq = p - f * nxq;
  }
}

template <typename T, bool kVec>
__global__ __launch_bounds__(256) void k_fields_gather(const T* __restrict__ src, T* __restrict__ dst, FieldsGeom g)
{
  extern __shared__ __align__(16) unsigned char fields_lds[];
  T* lds = reinterpret_cast<T*>(fields_lds);
  using Pack = typename FieldsPack<T>::type;
  constexpr uint32_t P = kFieldsPackBytes / sizeof(T);
  const uint32_t tid = threadIdx.x, stride = g.stride_x, nf = g.nfields;
  const FieldsTile t = fields_tile(g);
  // elements of the span that belong to the array: behind the last record's selected fields it may end
  const uint32_t span = (t.nx - 1) * stride + nf;
  for (uint32_t z = blockIdx.y; z < g.dimz; z += gridDim.y) {
    const T* s = src + ((uint64_t)z * g.pitch_z + (uint64_t)t.y * g.pitch_y + (uint64_t)t.x0 * stride);
    T* d = dst + (((uint64_t)z * g.dimy + t.y) * g.dimx + t.x0);
    if (!kVec && stride > kFieldsMaxLdsStride) {   // wide records: the selected pieces alone, no LDS
      if (tid < t.nx)
        for (uint32_t f = 0; f < nf; f++)
          d[f * g.vol + tid] = s[(uint64_t)tid * stride + f];
      continue;
    }
    if (kVec) {
      const uint32_t npk = t.nx * stride / P;   // (nx is a whole number of packs)
      for (uint32_t p = tid; p < npk; p += kFieldsTileX) {
        const uint32_t i = p * P;
        if (i + P <= span) {
          const Pack v = *reinterpret_cast<const Pack*>(s + i);
#pragma unroll
          for (uint32_t j = 0; j < P; j++)
            lds[fields_lds_slot(i + j)] = v[j];
        }
        else {
          for (uint32_t j = 0; i + j < span; j++)
            lds[fields_lds_slot(i + j)] = s[i + j];
        }
      }
      __syncthreads();
      const uint32_t nxq = t.nx / P;
      for (uint32_t p = tid; p < nxq * nf; p += kFieldsTileX) {
        uint32_t f, xq;
        fields_pack_of(p, t.nx, nxq, kFieldsTileX / P, f, xq);
        Pack v;
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          v[j] = lds[fields_lds_slot((xq * P + j) * stride + f)];
        *reinterpret_cast<Pack*>(d + f * g.vol + xq * P) = v;
      }
    }
    else {
      for (uint32_t i = tid; i < span; i += kFieldsTileX)
        lds[fields_lds_slot(i)] = s[i];
      __syncthreads();
      if (tid < t.nx)
        for (uint32_t f = 0; f < nf; f++)
          d[f * g.vol + tid] = lds[fields_lds_slot(tid * stride + f)];
    }
    __syncthreads();   // (the next slice's span goes into the same image)
  }
}

template <typename T, bool kVec>
__global__ __launch_bounds__(256) void k_fields_scatter(const T* __restrict__ src, T* __restrict__ dst, FieldsGeom g)
{
  extern __shared__ __align__(16) unsigned char fields_lds[];
  T* lds = reinterpret_cast<T*>(fields_lds);
  using Pack = typename FieldsPack<T>::type;
  constexpr uint32_t P = kFieldsPackBytes / sizeof(T);
  const uint32_t tid = threadIdx.x, stride = g.stride_x, nf = g.nfields;
  const FieldsTile t = fields_tile(g);
  const uint32_t span = (t.nx - 1) * stride + nf;
  for (uint32_t z = blockIdx.y; z < g.dimz; z += gridDim.y) {
    const T* s = src + (((uint64_t)z * g.dimy + t.y) * g.dimx + t.x0);
    T* d = dst + ((uint64_t)z * g.pitch_z + (uint64_t)t.y * g.pitch_y + (uint64_t)t.x0 * stride);
    if (!kVec && stride > kFieldsMaxLdsStride) {
      if (tid < t.nx)
        for (uint32_t f = 0; f < nf; f++)
          d[(uint64_t)tid * stride + f] = s[f * g.vol + tid];
      continue;
    }
    if (kVec) {   // (nfields == stride_x: every element of the span is a selected field)
      const uint32_t nxq = t.nx / P;
      for (uint32_t p = tid; p < nxq * nf; p += kFieldsTileX) {
        uint32_t f, xq;
        fields_pack_of(p, t.nx, nxq, kFieldsTileX / P, f, xq);
        const Pack v = *reinterpret_cast<const Pack*>(s + f * g.vol + xq * P);
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          lds[fields_lds_slot((xq * P + j) * stride + f)] = v[j];
      }
      __syncthreads();
      const uint32_t npk = t.nx * stride / P;
      for (uint32_t p = tid; p < npk; p += kFieldsTileX) {
        const uint32_t i = p * P;
        Pack v;
#pragma unroll
        for (uint32_t j = 0; j < P; j++)
          v[j] = lds[fields_lds_slot(i + j)];
        *reinterpret_cast<Pack*>(d + i) = v;
      }
    }
    else {
      if (tid < t.nx)
        for (uint32_t f = 0; f < nf; f++)
          lds[fields_lds_slot(tid * stride + f)] = s[f * g.vol + tid];
      __syncthreads();
      if (nf == stride) {
        for (uint32_t i = tid; i < span; i += kFieldsTileX)
          d[i] = lds[fields_lds_slot(i)];
      }
      else {
        // element i of the span is field i % stride_x of its record: only the selected ones are stored, each with a
        // store of its own width, and the image's other slots are never read
        uint32_t f = tid % stride;
        const uint32_t step = kFieldsTileX % stride;
        for (uint32_t i = tid; i < span; i += kFieldsTileX) {
          if (f < nf)
            d[i] = lds[fields_lds_slot(i)];
          f += step;
          if (f >= stride)
            f -= stride;
        }
      }
    }
    __syncthreads();
  }
}

// the geometry of a call, or false: a layout that is not valid, sizes that overflow, or dims the grid cannot hold
bool fields_geom(size_t nfields, size_t dimx, size_t dimy, size_t dimz, FieldsLayout l, FieldsGeom& g, dim3& grid)
{
  size_t count = 0;
  if (!fields_valid(nfields, dimx, dimy, dimz, l) || !fields_stacked(nfields, dimx, dimy, dimz, &count))
    return false;
  if (dimx >= kViewCursorMaxDim || dimy >= kViewCursorMaxDim || l.stride_x >= kViewCursorMaxDim)
    return false;
  const size_t tilesX = (dimx + kFieldsTileX - 1) / kFieldsTileX;
  if (tilesX * dimy >= kViewCursorMaxDim)   // (blocks along x of the grid)
    return false;
  g = FieldsGeom{(uint64_t)l.pitch_y, (uint64_t)l.pitch_z, (uint64_t)(count / nfields), (uint32_t)l.stride_x,
                 (uint32_t)nfields,   (uint32_t)dimx,      (uint32_t)dimy,             (uint32_t)dimz,
                 (uint32_t)tilesX};
  grid = dim3((uint32_t)(tilesX * dimy), (uint32_t)std::min<size_t>(dimz, 65535));
  return true;
}

size_t fields_lds_bytes(size_t stride_x, size_t elem_size)
{
  return stride_x > kFieldsMaxLdsStride ? 0 : (size_t)fields_lds_slots((uint32_t)stride_x) * elem_size;
}

template <typename T>
int gather_launch(const T* d_inter, T* d_stacked, const FieldsGeom& g, dim3 grid, FieldsLayout l, hipStream_t st)
{
  const size_t lds = fields_lds_bytes(g.stride_x, sizeof(T));
  const bool vec = g.stride_x <= kFieldsMaxLdsStride &&
                   fields_vec_ok((uintptr_t)d_inter, (uintptr_t)d_stacked, g.dimx, l, sizeof(T));
  if (vec)
    LAUNCH_K((k_fields_gather<T, true>), grid, dim3(kFieldsTileX), lds, st, d_inter, d_stacked, g);
  else
    LAUNCH_K((k_fields_gather<T, false>), grid, dim3(kFieldsTileX), lds, st, d_inter, d_stacked, g);
  HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int scatter_launch(const T* d_stacked, T* d_inter, const FieldsGeom& g, dim3 grid, FieldsLayout l, hipStream_t st)
{
  const size_t lds = fields_lds_bytes(g.stride_x, sizeof(T));
  const bool vec = g.stride_x <= kFieldsMaxLdsStride && g.nfields == g.stride_x &&
                   fields_vec_ok((uintptr_t)d_inter, (uintptr_t)d_stacked, g.dimx, l, sizeof(T));
  if (vec)
    LAUNCH_K((k_fields_scatter<T, true>), grid, dim3(kFieldsTileX), lds, st, d_stacked, d_inter, g);
  else
    LAUNCH_K((k_fields_scatter<T, false>), grid, dim3(kFieldsTileX), lds, st, d_stacked, d_inter, g);
  HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int fields_gather_run(const void* d_inter, FieldsLayout l, size_t nfields, int is_float, size_t dimx, size_t dimy,
                      size_t dimz, void* d_stacked, void* hip_stream)
{
  FieldsGeom g;
  dim3 grid;
  if (!d_inter || !d_stacked || !fields_geom(nfields, dimx, dimy, dimz, l, g, grid))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  return is_float ? gather_launch(static_cast<const float*>(d_inter), static_cast<float*>(d_stacked), g, grid, l, st)
                  : gather_launch(static_cast<const double*>(d_inter), static_cast<double*>(d_stacked), g, grid, l, st);
}

int fields_scatter_run(const void* d_stacked, size_t nfields, int is_float, size_t dimx, size_t dimy, size_t dimz,
                       void* d_inter, FieldsLayout l, void* hip_stream)
{
  FieldsGeom g;
  dim3 grid;
  if (!d_inter || !d_stacked || !fields_geom(nfields, dimx, dimy, dimz, l, g, grid))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  return is_float ? scatter_launch(static_cast<const float*>(d_stacked), static_cast<float*>(d_inter), g, grid, l, st)
                  : scatter_launch(static_cast<const double*>(d_stacked), static_cast<double*>(d_inter), g, grid, l, st);
}

}  // namespace sperrhip
