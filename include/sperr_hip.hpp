// sperr_hip.hpp -- header-only C++ mirrors of the reference's driver classes on top of the C ABI
// of libsperr_hip.so (include/sperr_hip.h).  Same names, methods, argument meaning and return
// codes as the reference, so code written against
//
//     /root/reference/include/SPERR3D_OMP_C.h:14-35   (sperr::SPERR3D_OMP_C)
//     /root/reference/include/SPERR3D_OMP_D.h:15-32   (sperr::SPERR3D_OMP_D)
//     /root/reference/include/SPECK_FLT.h:17-65       (sperr::SPECK3D_FLT, the per-chunk pipeline;
//                                                      sperr::SPECK2D_FLT, one slice)
//     /root/reference/include/SPERR3D_Stream_Tools.h:11-66 (SPERR3D_Header, SPERR3D_Stream_Tools)
//     /root/reference/include/sperr_helper.h:35,54-64 (dims_type, vec8_type, vecd_type, RTNType)
//
// compiles unchanged when it includes this header instead and links -lsperr_hip.  The chunk
// pipeline itself runs on the GPU; set_num_threads() is accepted and ignored.  The fixed-rate
// (set_bitrate), fixed-PSNR (set_psnr) and fixed point-wise error (set_tolerance) modes all run
// on the GPU path.
#ifndef SPERR_HIP_HPP
#define SPERR_HIP_HPP

#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sperr_hip.h"

namespace sperr {

using dims_type = std::array<size_t, 3>;
using vec8_type = std::vector<uint8_t>;
using vecd_type = std::vector<double>;
using vecf_type = std::vector<float>;

enum class RTNType {  // include/sperr_helper.h:54-64
  Good = 0,
  WrongLength,
  IOError,
  BitBudgetMet,
  VersionMismatch,
  SliceVolumeMismatch,
  CompModeUnknown,
  FE_Invalid,
  Error
};

enum class CompMode : unsigned char { PSNR, PWE, Rate, Unknown };

namespace detail {
// Width in bytes of the integer coefficients of a chunk stream (SPECK_FLT::integer_len,
// /root/reference/src/SPECK_FLT.cpp:193-213).  The reference picks it from the largest quantised
// coefficient when it encodes (:324-337: <= 255, <= 65535, <= 2^32 - 1) and from the number of
// bit planes in the SPECK header when it decodes (:64-72: <= 8, <= 16, <= 32) -- one and the same
// rule, so the stream's header byte answers for both.  A stream without coefficients (constant
// field) leaves the default, uint64 (include/SPECK_FLT.h:68).
inline size_t integer_len_of(const vec8_type& stream)
{
  if (stream.size() < 18 || (stream[0] & 0x01))
    return sizeof(uint64_t);
  const unsigned nbp = stream[17];
  return nbp <= 8 ? 1 : nbp <= 16 ? 2 : nbp <= 32 ? 4 : 8;
}
}  // namespace detail

// ---- src/SPERR3D_OMP_C.cpp:12-161 --------------------------------------------------------------
class SPERR3D_OMP_C {
 public:
  void set_num_threads(size_t) {}
  void set_dims_and_chunks(dims_type vol_dims, dims_type chunk_dims)
  {
    m_dims = vol_dims;
    for (size_t i = 0; i < 3; i++) {  // clamp to [1, vol] (SPERR3D_OMP_C.cpp:23-30)
      size_t c = chunk_dims[i] < 1 ? 1 : chunk_dims[i];
      m_chunk_dims[i] = c > vol_dims[i] ? vol_dims[i] : c;
    }
  }
  void set_psnr(double v) { m_mode = CompMode::PSNR; m_quality = v; }
  void set_tolerance(double v) { m_mode = CompMode::PWE; m_quality = v; }
  void set_bitrate(double v) { m_mode = CompMode::Rate; m_quality = v; }

  template <typename T>
  auto compress(const T* buf, size_t buf_len) -> RTNType
  {
    static_assert(std::is_floating_point<T>::value, "!! Only floating point values are supported !!");
    if (m_mode == CompMode::Unknown)
      return RTNType::CompModeUnknown;
    if (buf_len != m_dims[0] * m_dims[1] * m_dims[2])
      return RTNType::WrongLength;
    const int mode = m_mode == CompMode::Rate ? 1 : m_mode == CompMode::PSNR ? 2 : 3;
    void* dst = nullptr;
    size_t len = 0;
    const int rtn = sperr_comp_3d(buf, std::is_same<T, float>::value ? 1 : 0, m_dims[0], m_dims[1],
                                  m_dims[2], m_chunk_dims[0], m_chunk_dims[1], m_chunk_dims[2], mode,
                                  m_quality, 0, &dst, &len);
    if (rtn != 0)
      return RTNType::Error;
    m_stream.assign(static_cast<uint8_t*>(dst), static_cast<uint8_t*>(dst) + len);
    std::free(dst);
    return RTNType::Good;
  }
  auto get_encoded_bitstream() const -> vec8_type { return m_stream; }

 private:
  CompMode m_mode = CompMode::Unknown;
  double m_quality = 0.0;
  dims_type m_dims = {0, 0, 0}, m_chunk_dims = {0, 0, 0};
  vec8_type m_stream;
};

// ---- src/SPERR3D_OMP_D.cpp:13-165 --------------------------------------------------------------
class SPERR3D_OMP_D {
 public:
  void set_num_threads(size_t) {}
  auto use_bitstream(const void* p, size_t total_len) -> RTNType
  {
    const auto* u8 = static_cast<const uint8_t*>(p);
    if (total_len < 18)
      return RTNType::WrongLength;
    if (u8[0] != 0)
      return RTNType::VersionMismatch;
    if (!(u8[1] & 0x40))
      return RTNType::SliceVolumeMismatch;
    size_t dx, dy, dz;
    int is_float;
    sperr_parse_header(p, &dx, &dy, &dz, &is_float);
    m_dims = {dx, dy, dz};
    m_chunk_dims = m_dims;
    if (u8[1] & 0x10) {
      uint16_t c3[3];
      std::memcpy(c3, u8 + 14, 6);
      m_chunk_dims = {c3[0], c3[1], c3[2]};
    }
    m_ptr = u8;
    m_len = total_len;
    return RTNType::Good;
  }
  // the pointer MUST be the one given to use_bitstream (SPERR3D_OMP_D.cpp:53-56)
  auto decompress(const void* bitstream, bool multi_res = false) -> RTNType
  {
    if (bitstream == nullptr || m_ptr == nullptr || bitstream != m_ptr)
      return RTNType::Error;
    void* dst = nullptr;
    size_t dx, dy, dz;
    m_hierarchy.clear();
    if (multi_res) {   // SPERR3D_OMP_D.cpp:68-84,121-130: the volume at every coarsened resolution
      size_t nlev = 0, ldims[48];
      double* levels[16] = {};
      if (sperrhip_decomp_3d_multires(m_ptr, m_len, 0, &dx, &dy, &dz, &dst, &nlev, ldims, levels) != 0)
        return RTNType::Error;
      for (size_t h = 0; h < nlev; h++) {
        const size_t n = ldims[3 * h] * ldims[3 * h + 1] * ldims[3 * h + 2];
        m_hierarchy.emplace_back(levels[h], levels[h] + n);
        std::free(levels[h]);
      }
    }
    else if (sperr_decomp_3d(m_ptr, m_len, 0, 0, &dx, &dy, &dz, &dst) != 0)
      return RTNType::Error;
    const auto* d = static_cast<const double*>(dst);
    m_vol.assign(d, d + dx * dy * dz);
    std::free(dst);
    return RTNType::Good;
  }
  // (this library's addition) only the box [lo, lo + dims) of the volume, decoded from the chunks it
  // meets (sperrhip_decomp_3d_box); view_decoded_data() then holds the box, x fastest.  pct (here and below): decode
  // the first pct percent of every chunk stream only, what decoding progressive_truncate(.., pct) gives (0: all)
  auto decompress_box(const void* bitstream, dims_type lo, dims_type dims, unsigned pct = 0) -> RTNType
  {
    return window_impl(bitstream, pct, nullptr, lo.data(), dims.data());
  }
  // (this library's addition) one level of the hierarchy alone, coarsest first as view_hierarchy() orders them, whole
  // or the box [lo, lo + dims) of it in the level's coordinates (sperrhip_decomp_3d_level): only the chunks it meets
  // are read and only the level's part of the inverse transform runs; view_decoded_data() then holds it, x fastest
  auto decompress_level(const void* bitstream, size_t level, unsigned pct = 0) -> RTNType
  {
    return window_impl(bitstream, pct, &level, nullptr, nullptr);
  }
  auto decompress_level(const void* bitstream, size_t level, dims_type lo, dims_type dims, unsigned pct = 0) -> RTNType
  {
    return window_impl(bitstream, pct, &level, lo.data(), dims.data());
  }
  // (this library's addition) the volume from the first pct percent of every chunk stream
  // (sperrhip_decomp_3d_portion): only those bytes travel to the device
  auto decompress_portion(const void* bitstream, unsigned pct) -> RTNType
  {
    return window_impl(bitstream, pct, nullptr, nullptr, nullptr, true);
  }
  auto view_decoded_data() const -> const vecd_type& { return m_vol; }
  auto release_decoded_data() -> vecd_type&& { return std::move(m_vol); }
  auto view_hierarchy() const -> const std::vector<vecd_type>& { return m_hierarchy; }
  auto release_hierarchy() -> std::vector<vecd_type>&& { return std::move(m_hierarchy); }
  auto get_dims() const -> dims_type { return m_dims; }
  auto get_chunk_dims() const -> dims_type { return m_chunk_dims; }

 private:
  // a box (level null), a level or a box of one; `portion`: through sperrhip_decomp_3d_portion whatever pct is
  auto window_impl(const void* bitstream, unsigned pct, const size_t* level, const size_t* lo, const size_t* dims,
                   bool portion = false) -> RTNType
  {
    if (bitstream == nullptr || m_ptr == nullptr || bitstream != m_ptr)
      return RTNType::Error;
    void* dst = nullptr;
    size_t od[3] = {0, 0, 0};
    m_hierarchy.clear();
    int rtn;
    if (portion || pct != 0)
      rtn = sperrhip_decomp_3d_portion(m_ptr, m_len, pct, 0, level, lo, dims, od, &dst);
    else if (level)
      rtn = sperrhip_decomp_3d_level(m_ptr, m_len, 0, *level, lo, dims, od, &dst);
    else {
      rtn = sperrhip_decomp_3d_box(m_ptr, m_len, 0, lo, dims, &dst);
      for (int a = 0; a < 3; a++)
        od[a] = dims[a];
    }
    if (rtn != 0)
      return RTNType::Error;
    const auto* d = static_cast<const double*>(dst);
    m_vol.assign(d, d + od[0] * od[1] * od[2]);
    std::free(dst);
    return RTNType::Good;
  }
  dims_type m_dims = {0, 0, 0}, m_chunk_dims = {0, 0, 0};
  const uint8_t* m_ptr = nullptr;
  size_t m_len = 0;
  vecd_type m_vol;
  std::vector<vecd_type> m_hierarchy;   // multi-resolution decoding, coarsest first
};

// ---- src/SPECK_FLT.cpp:11-606 + src/SPECK3D_FLT.cpp: one chunk ---------------------------------
// A chunk stream is the single-chunk container minus its 18-byte header
// (src/SPERR3D_OMP_C.cpp:163-234: 14 bytes + one 4-byte length).
class SPECK3D_FLT {
 public:
  template <typename T>
  void copy_data(const T* p, size_t len) { m_vals.assign(p, p + len); }
  void take_data(vecd_type&& buf) { m_vals = std::move(buf); }
  void set_dims(dims_type d) { m_dims = d; }
  void set_bitrate(double bpp) { m_mode = CompMode::Rate; m_quality = bpp; }
  void set_psnr(double v) { m_mode = CompMode::PSNR; m_quality = v; }
  void set_tolerance(double v) { m_mode = CompMode::PWE; m_quality = v; }
  auto integer_len() const -> size_t { return detail::integer_len_of(m_stream); }

  auto compress() -> RTNType
  {
    if (m_vals.empty() || m_vals.size() != m_dims[0] * m_dims[1] * m_dims[2])
      return RTNType::Error;
    if (m_mode == CompMode::Unknown)
      return RTNType::CompModeUnknown;
    const int mode = m_mode == CompMode::Rate ? 1 : m_mode == CompMode::PSNR ? 2 : 3;
    void* dst = nullptr;
    size_t len = 0;
    if (sperr_comp_3d(m_vals.data(), 0, m_dims[0], m_dims[1], m_dims[2], m_dims[0], m_dims[1],
                      m_dims[2], mode, m_quality, 0, &dst, &len) != 0)
      return RTNType::Error;
    const auto* u8 = static_cast<const uint8_t*>(dst);
    m_stream.assign(u8 + 18, u8 + len);
    std::free(dst);
    return RTNType::Good;
  }
  void append_encoded_bitstream(vec8_type& buf) const
  {
    buf.insert(buf.end(), m_stream.begin(), m_stream.end());
  }
  auto use_bitstream(const void* p, size_t len) -> RTNType
  {
    if (len < 17)
      return RTNType::WrongLength;
    const auto* u8 = static_cast<const uint8_t*>(p);
    m_stream.assign(u8, u8 + len);
    return RTNType::Good;
  }
  auto decompress(bool multi_res = false) -> RTNType
  {
    if (m_stream.empty())
      return RTNType::Error;
    // wrap the chunk stream into a single-chunk container (double output)
    vec8_type c(18 + m_stream.size());
    c[0] = 0;
    c[1] = 0x40;
    const uint32_t v3[3] = {(uint32_t)m_dims[0], (uint32_t)m_dims[1], (uint32_t)m_dims[2]};
    std::memcpy(c.data() + 2, v3, 12);
    const uint32_t l = (uint32_t)m_stream.size();
    std::memcpy(c.data() + 14, &l, 4);
    std::memcpy(c.data() + 18, m_stream.data(), m_stream.size());
    void* dst = nullptr;
    size_t dx, dy, dz;
    m_hierarchy.clear();
    if (multi_res) {   // a chunk that is not dyadic has no hierarchy (src/CDF97.cpp:150-168)
      size_t nlev = 0, ld[48];
      double* lv[16] = {};
      if (sperrhip_decomp_3d_multires(c.data(), c.size(), 0, &dx, &dy, &dz, &dst, &nlev, ld, lv) != 0)
        return RTNType::Error;
      for (size_t h = 0; h < nlev; h++) {
        m_hierarchy.emplace_back(lv[h], lv[h] + ld[3 * h] * ld[3 * h + 1] * ld[3 * h + 2]);
        std::free(lv[h]);
      }
    }
    else if (sperr_decomp_3d(c.data(), c.size(), 0, 0, &dx, &dy, &dz, &dst) != 0)
      return RTNType::Error;
    const auto* d = static_cast<const double*>(dst);
    m_vals.assign(d, d + dx * dy * dz);
    std::free(dst);
    return RTNType::Good;
  }
  auto view_hierarchy() const -> const std::vector<vecd_type>& { return m_hierarchy; }
  auto release_hierarchy() -> std::vector<vecd_type>&& { return std::move(m_hierarchy); }
  auto view_decoded_data() const -> const vecd_type& { return m_vals; }
  auto release_decoded_data() -> vecd_type&& { return std::move(m_vals); }

 private:
  CompMode m_mode = CompMode::Unknown;
  double m_quality = 0.0;
  dims_type m_dims = {0, 0, 0};
  vecd_type m_vals;
  vec8_type m_stream;
  std::vector<vecd_type> m_hierarchy;
};

// ---- src/SPECK_FLT.cpp + src/SPECK2D_FLT.cpp: one slice, dims = {x, y, 1} ------------------------
// The stream is the one sperr_comp_2d produces without its 10-byte header (src/SPERR_C_API.cpp:7-83).
class SPECK2D_FLT {
 public:
  template <typename T>
  void copy_data(const T* p, size_t len) { m_vals.assign(p, p + len); }
  void take_data(vecd_type&& buf) { m_vals = std::move(buf); }
  void set_dims(dims_type d) { m_dims = d; }
  void set_bitrate(double bpp) { m_mode = CompMode::Rate; m_quality = bpp; }
  void set_psnr(double v) { m_mode = CompMode::PSNR; m_quality = v; }
  void set_tolerance(double v) { m_mode = CompMode::PWE; m_quality = v; }
  auto integer_len() const -> size_t { return detail::integer_len_of(m_stream); }

  auto compress() -> RTNType
  {
    if (m_dims[2] != 1 || m_vals.empty() || m_vals.size() != m_dims[0] * m_dims[1])
      return RTNType::Error;
    if (m_mode == CompMode::Unknown)
      return RTNType::CompModeUnknown;
    const int mode = m_mode == CompMode::Rate ? 1 : m_mode == CompMode::PSNR ? 2 : 3;
    void* dst = nullptr;
    size_t len = 0;
    if (sperr_comp_2d(m_vals.data(), 0, m_dims[0], m_dims[1], mode, m_quality, 0, &dst, &len) != 0)
      return RTNType::Error;
    const auto* u8 = static_cast<const uint8_t*>(dst);
    m_stream.assign(u8, u8 + len);
    std::free(dst);
    return RTNType::Good;
  }
  void append_encoded_bitstream(vec8_type& buf) const
  {
    buf.insert(buf.end(), m_stream.begin(), m_stream.end());
  }
  auto use_bitstream(const void* p, size_t len) -> RTNType
  {
    if (len < 17)
      return RTNType::WrongLength;
    const auto* u8 = static_cast<const uint8_t*>(p);
    m_stream.assign(u8, u8 + len);
    return RTNType::Good;
  }
  auto decompress(bool multi_res = false) -> RTNType
  {
    if (m_stream.empty() || m_dims[2] != 1)
      return RTNType::Error;
    void* dst = nullptr;
    m_hierarchy.clear();
    if (multi_res) {
      size_t nlev = 0, ld[32];
      double* lv[16] = {};
      if (sperrhip_decomp_2d_multires(m_stream.data(), m_stream.size(), 0, m_dims[0], m_dims[1], &dst, &nlev,
                                      ld, lv) != 0)
        return RTNType::Error;
      for (size_t h = 0; h < nlev; h++) {
        m_hierarchy.emplace_back(lv[h], lv[h] + ld[2 * h] * ld[2 * h + 1]);
        std::free(lv[h]);
      }
    }
    else if (sperr_decomp_2d(m_stream.data(), m_stream.size(), 0, m_dims[0], m_dims[1], &dst) != 0)
      return RTNType::Error;
    const auto* d = static_cast<const double*>(dst);
    m_vals.assign(d, d + m_dims[0] * m_dims[1]);
    std::free(dst);
    return RTNType::Good;
  }
  auto view_decoded_data() const -> const vecd_type& { return m_vals; }
  auto release_decoded_data() -> vecd_type&& { return std::move(m_vals); }
  auto view_hierarchy() const -> const std::vector<vecd_type>& { return m_hierarchy; }
  auto release_hierarchy() -> std::vector<vecd_type>&& { return std::move(m_hierarchy); }

 private:
  CompMode m_mode = CompMode::Unknown;
  double m_quality = 0.0;
  dims_type m_dims = {0, 0, 0};
  vecd_type m_vals;
  vec8_type m_stream;
  std::vector<vecd_type> m_hierarchy;
};

// ---- include/SPERR3D_Stream_Tools.h:11-66, src/SPERR3D_Stream_Tools.cpp ---------------------------
struct SPERR3D_Header {
  uint8_t major_version = 0;
  bool is_portion = false;
  bool is_3D = false;
  bool is_float = false;
  bool multi_chunk = false;
  dims_type vol_dims = {0, 0, 0};
  dims_type chunk_dims = {0, 0, 0};
  size_t header_len = 0;
  size_t stream_len = 0;
  std::vector<size_t> chunk_offsets;   // (offset, length) of every chunk
};

class SPERR3D_Stream_Tools {
 public:
  auto get_header_len(std::array<uint8_t, 20> magic) const -> size_t
  {
    const bool multi = (magic[1] & 0x10) != 0;
    dims_type v, c;
    m_dims_of(magic.data(), multi, v, c);
    return (multi ? 20 : 14) + 4 * m_num_chunks(v, c);
  }
  auto get_stream_header(const void* p) const -> SPERR3D_Header
  {
    SPERR3D_Header h;
    const auto* u8 = static_cast<const uint8_t*>(p);
    h.major_version = u8[0];
    h.is_portion = (u8[1] & 0x80) != 0;   // pack_8_booleans: bool i at bit 7 - i
    h.is_3D = (u8[1] & 0x40) != 0;
    h.is_float = (u8[1] & 0x20) != 0;
    h.multi_chunk = (u8[1] & 0x10) != 0;
    m_dims_of(u8, h.multi_chunk, h.vol_dims, h.chunk_dims);
    const size_t n = m_num_chunks(h.vol_dims, h.chunk_dims), at = h.multi_chunk ? 20 : 14;
    h.header_len = at + 4 * n;
    h.chunk_offsets.resize(2 * n);
    size_t off = h.header_len;
    for (size_t i = 0; i < n; i++) {
      uint32_t l;
      std::memcpy(&l, u8 + at + 4 * i, 4);
      h.chunk_offsets[2 * i] = off;
      h.chunk_offsets[2 * i + 1] = l;
      off += l;
    }
    h.stream_len = off;
    return h;
  }
  // keep `pct` percent of every chunk (at least 64 bytes of each); an empty vector on failure
  auto progressive_truncate(const void* stream, size_t stream_len, unsigned pct) const -> vec8_type
  {
    vec8_type out;
    void* dst = nullptr;
    size_t len = 0;
    if (sperr_trunc_3d(stream, stream_len, pct, &dst, &len) == 0) {
      const auto* u8 = static_cast<const uint8_t*>(dst);
      out.assign(u8, u8 + len);
      std::free(dst);
    }
    return out;
  }
  // (this library's addition) the same on a container in device memory, into device memory (sperrhip_trunc_dev):
  // the bytes written to d_out, which holds `cap` (stream_len always suffices); 0 on failure
  auto progressive_truncate_dev(const void* d_stream, size_t stream_len, unsigned pct, void* d_out, size_t cap) const
      -> size_t
  {
    size_t len = 0;
    return sperrhip_trunc_dev(d_stream, stream_len, pct, d_out, cap, &len, nullptr) == 0 ? len : 0;
  }
  auto progressive_read(const std::string& filename, unsigned pct) const -> vec8_type
  {
    vec8_type whole;
    if (std::FILE* f = std::fopen(filename.c_str(), "rb")) {
      uint8_t buf[1 << 16];
      for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;)
        whole.insert(whole.end(), buf, buf + got);
      std::fclose(f);
    }
    return whole.size() < 18 ? vec8_type() : progressive_truncate(whole.data(), whole.size(), pct);
  }

 private:
  static void m_dims_of(const uint8_t* u8, bool multi, dims_type& v, dims_type& c)
  {
    uint32_t v3[3];
    std::memcpy(v3, u8 + 2, 12);
    v = {v3[0], v3[1], v3[2]};
    c = v;
    if (multi) {
      uint16_t c3[3];
      std::memcpy(c3, u8 + 14, 6);
      c = {c3[0], c3[1], c3[2]};
    }
  }
  // src/sperr_helper.cpp:542-592: a remainder longer than half a chunk becomes a chunk of its own
  static auto m_num_chunks(const dims_type& v, const dims_type& c) -> size_t
  {
    size_t n = 1;
    for (int a = 0; a < 3; a++) {
      size_t seg = c[a] ? v[a] / c[a] : 0;
      if (c[a] && v[a] % c[a] > c[a] / 2)
        seg++;
      n *= seg ? seg : 1;
    }
    return n;
  }
};

// (this library's addition) calc_stats<T> then calc_mean_var<T> of two arrays of n values in device memory
// (sperrhip_quality_dev): {rmse, linfty, psnr, min, max, mean, var, mse}, each a T widened to double.
// RTNType::Good, or RTNType::Error (out untouched) for n == 0, a null pointer or no device.
template <typename T>
inline auto quality_dev(const T* d_orig, const T* d_recon, size_t n, std::array<double, 8>& out,
                        void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int rtn = sperrhip_quality_dev(d_orig, d_recon, sizeof(T) == 4, n, out.data(), hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// (this library's addition) Strided views of device arrays (sperrhip_view: the interior of an array with ghost cells,
// a slice of a larger one): a volume of `dims`, x fastest with unit x stride, rows pitch_y and slices pitch_z elements
// apart from its first element.  The calls below are the device-pointer calls with such a view in place of a packed
// array; no packed copy is made.  RTNType::Error (nothing written) for a view that is not valid, a null pointer, or an
// output that does not hold the view.
using view_type = sperrhip_view;

// the dense view of a volume
inline auto dense_view(dims_type dims) -> view_type { return view_type{dims[0], dims[0] * dims[1]}; }

// quality_dev of two arrays of `dims` read through views; a null view means dense (sperrhip_quality_view_dev)
template <typename T>
inline auto quality_view_dev(const T* d_orig, const view_type* view_orig, const T* d_recon,
                             const view_type* view_recon, dims_type dims, std::array<double, 8>& out,
                             void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int rtn = sperrhip_quality_view_dev(d_orig, view_orig, d_recon, view_recon, sizeof(T) == 4, dims[0], dims[1],
                                            dims[2], out.data(), hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// A view of a device volume into a container in device memory of `cap` bytes (sperrhip_compress_view_dev); `len`
// receives the container's length.  `mode` and `quality` as SPERR3D_OMP_C's setters name them.
template <typename T>
inline auto compress_view_dev(const T* d_src, const view_type& view, dims_type dims, dims_type chunks, CompMode mode,
                              double quality, void* d_out, size_t cap, size_t& len, void* hip_stream = nullptr)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int m = mode == CompMode::Rate ? 1 : mode == CompMode::PSNR ? 2 : mode == CompMode::PWE ? 3 : 0;
  if (m == 0)
    return RTNType::CompModeUnknown;
  const int rtn = sperrhip_compress_view_dev(d_src, &view, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0],
                                             chunks[1], chunks[2], m, quality, d_out, cap, &len, hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// The volume of a device container, or with `box_lo` / `box_dims` (both or neither) a box of it, from the first `pct`
// percent of every chunk stream (0: all), into a view of `cap_bytes` of device memory at d_out
// (sperrhip_decompress_view_dev).  Nothing outside the view is written.
template <typename T>
inline auto decompress_view_dev(const void* d_stream, size_t stream_len, T* d_out, const view_type& view,
                                size_t cap_bytes, const dims_type* box_lo = nullptr,
                                const dims_type* box_dims = nullptr, unsigned pct = 0, void* hip_stream = nullptr)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int rtn = sperrhip_decompress_view_dev(d_stream, stream_len, pct, sizeof(T) == 4,
                                               box_lo ? box_lo->data() : nullptr, box_dims ? box_dims->data() : nullptr,
                                               d_out, &view, cap_bytes, hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// (this library's addition) Interleaved fields of a device array (sperrhip_fields: a solver's (z, y, x, nvar), a
// channels-last tensor): `nfields` consecutive fields from the data pointer, the first selected field at (0, 0, 0);
// samples stride_x, rows pitch_y and slices pitch_z elements apart.  A null layout means the dense interleave of
// nfields.  One container per field, each what the device-pointer calls make of the packed copy of that field.
// RTNType::Error (nothing written) for a layout that is not valid, a null pointer, or an output that does not hold it.
using fields_type = sperrhip_fields;

// the dense interleave of nfields fields of a volume
inline auto dense_fields(size_t nfields, dims_type dims) -> fields_type
{
  return fields_type{nfields, dims[0] * nfields, dims[0] * dims[1] * nfields};
}

// nfields containers back to back into `cap` bytes of device memory at d_out (sperrhip_compress_fields_dev);
// `offsets` receives nfields + 1 entries, container f at [offsets[f], offsets[f + 1])
template <typename T>
inline auto compress_fields_dev(const T* d_src, const fields_type* layout, size_t nfields, dims_type dims,
                                dims_type chunks, CompMode mode, double quality, void* d_out, size_t cap,
                                std::vector<size_t>& offsets, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int m = mode == CompMode::Rate ? 1 : mode == CompMode::PSNR ? 2 : mode == CompMode::PWE ? 3 : 0;
  if (m == 0)
    return RTNType::CompModeUnknown;
  offsets.assign(nfields + 1, 0);
  const int rtn = sperrhip_compress_fields_dev(d_src, layout, nfields, sizeof(T) == 4, dims[0], dims[1], dims[2],
                                               chunks[0], chunks[1], chunks[2], m, quality, d_out, cap, offsets.data(),
                                               hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// The containers at [offsets[f], offsets[f + 1]) of d_streams, each a volume of `dims`, into the fields of d_out that
// `layout` names, within `cap_bytes` from d_out (sperrhip_decompress_fields_dev).  Nothing but those fields is written.
template <typename T>
inline auto decompress_fields_dev(const void* d_streams, const std::vector<size_t>& offsets, dims_type dims, T* d_out,
                                  const fields_type* layout, size_t cap_bytes, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  if (offsets.size() < 2)
    return RTNType::Error;
  const int rtn = sperrhip_decompress_fields_dev(d_streams, offsets.data(), offsets.size() - 1, sizeof(T) == 4, dims[0],
                                                 dims[1], dims[2], d_out, layout, cap_bytes, hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// (this library's addition) A box per entry out of a batch of device containers, in one call
// (sperrhip_decompress_boxes_dev): entry e is the box [box_lo[e], box_lo[e] + box_dims) of container which[e] -- of
// container e when `which` is empty -- or, with `level`, of that level of its hierarchy in the level's coordinates;
// from the first `pct` percent of every chunk stream (0: all).  d_streams[c] is container c, stream_lens[c] bytes of
// device memory anywhere.  d_out receives box_lo.size() boxes back to back within `cap_bytes`.  RTNType::Error, with
// nothing written, for what the C call refuses.
template <typename T>
inline auto decompress_boxes_dev(const std::vector<const void*>& d_streams, const std::vector<size_t>& stream_lens,
                                 const std::vector<uint32_t>& which, const std::vector<dims_type>& box_lo,
                                 dims_type box_dims, T* d_out, size_t cap_bytes, const size_t* level = nullptr,
                                 unsigned pct = 0, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  if (d_streams.size() != stream_lens.size() || (!which.empty() && which.size() != box_lo.size()))
    return RTNType::Error;
  std::vector<size_t> lo;
  for (const auto& o : box_lo)
    lo.insert(lo.end(), o.begin(), o.end());
  const int rtn = sperrhip_decompress_boxes_dev(d_streams.data(), stream_lens.data(), d_streams.size(),
                                                which.empty() ? nullptr : which.data(), lo.data(), box_lo.size(),
                                                box_dims.data(), level, pct, sizeof(T) == 4, d_out, cap_bytes,
                                                hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// quality_dev of every field of two interleaved arrays; `out` receives eight figures per field
// (sperrhip_quality_fields_dev)
template <typename T>
inline auto quality_fields_dev(const T* d_orig, const fields_type* layout_orig, const T* d_recon,
                               const fields_type* layout_recon, size_t nfields, dims_type dims,
                               std::vector<std::array<double, 8>>& out, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  out.assign(nfields, std::array<double, 8>{});
  const int rtn = sperrhip_quality_fields_dev(d_orig, layout_orig, d_recon, layout_recon, nfields, sizeof(T) == 4,
                                              dims[0], dims[1], dims[2], nfields ? out[0].data() : nullptr, hip_stream);
  return rtn == 0 ? RTNType::Good : RTNType::Error;
}

// (this library's addition) Missing values (include/sperr_hip.h, "masked volumes"): a container of the in-filled
// volume and a mask stream.  MissingRule::NaN takes no threshold; AbsGE takes one, finite and > 0.
// RTNType::WrongLength: the mask's (or the container's) buffer is too small, mask_len then names the size needed.
enum class MissingRule : int { NaN = SPERRHIP_MISSING_NAN, AbsGE = SPERRHIP_MISSING_ABS_GE };

namespace detail {
inline auto mask_rtn(int rtn) -> RTNType
{
  return rtn == 0 ? RTNType::Good : rtn == 1 ? RTNType::WrongLength : rtn == 2 ? RTNType::CompModeUnknown : RTNType::Error;
}
}  // namespace detail

// the stream of n samples into d_mask, the in-filled samples into d_filled (null: none; may be d_src)
template <typename T>
inline auto mask_make_dev(const T* d_src, size_t n, MissingRule rule, double threshold, T* d_filled, void* d_mask,
                          size_t mask_cap, size_t& mask_len, size_t& nmissing, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_mask_make_dev(d_src, sizeof(T) == 4, n, static_cast<int>(rule), threshold, d_filled,
                                                 d_mask, mask_cap, &mask_len, &nmissing, hip_stream));
}

// What stands at the missing samples of the in-filled volume (include/sperr_hip.h, SPERRHIP_FILL_*): the midrange of
// the valid samples, a value of the caller's, or the smooth pull-push fill
enum class FillKind : int { Midrange = SPERRHIP_FILL_MIDRANGE, Value = SPERRHIP_FILL_VALUE, Smooth = SPERRHIP_FILL_SMOOTH };

// ... of a volume of dims (x, y, z) with a fill; fill_value is read by FillKind::Value alone
template <typename T>
inline auto mask_make_dev(const T* d_src, dims_type dims, MissingRule rule, double threshold, FillKind fill,
                          double fill_value, T* d_filled, void* d_mask, size_t mask_cap, size_t& mask_len,
                          size_t& nmissing, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_mask_make_vol_dev(d_src, sizeof(T) == 4, dims[0], dims[1], dims[2],
                                                     static_cast<int>(rule), threshold, static_cast<int>(fill),
                                                     fill_value, d_filled, d_mask, mask_cap, &mask_len, &nmissing,
                                                     hip_stream));
}

// `value` at the missing samples of the box of a volume that d_vol holds (null box: the whole volume); nothing else
template <typename T>
inline auto mask_apply_dev(T* d_vol, dims_type vol_dims, const dims_type* box_lo, const dims_type* box_dims,
                           const void* d_mask, size_t mask_len, double value, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_mask_apply_dev(d_vol, sizeof(T) == 4, vol_dims.data(),
                                                  box_lo ? box_lo->data() : nullptr,
                                                  box_dims ? box_dims->data() : nullptr, d_mask, mask_len, value,
                                                  hip_stream));
}

template <typename T>
inline auto compress_masked_dev(const T* d_src, dims_type dims, dims_type chunks, CompMode mode, double quality,
                                MissingRule rule, double threshold, void* d_out, size_t cap, size_t& out_len,
                                void* d_mask, size_t mask_cap, size_t& mask_len, size_t& nmissing,
                                void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int m = mode == CompMode::Rate ? 1 : mode == CompMode::PSNR ? 2 : mode == CompMode::PWE ? 3 : 0;
  if (m == 0)
    return RTNType::CompModeUnknown;
  return detail::mask_rtn(sperrhip_compress_masked_dev(d_src, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0],
                                                       chunks[1], chunks[2], m, quality, static_cast<int>(rule),
                                                       threshold, d_out, cap, &out_len, d_mask, mask_cap, &mask_len,
                                                       &nmissing, hip_stream));
}

// ... with a fill
template <typename T>
inline auto compress_masked_dev(const T* d_src, dims_type dims, dims_type chunks, CompMode mode, double quality,
                                MissingRule rule, double threshold, FillKind fill, double fill_value, void* d_out,
                                size_t cap, size_t& out_len, void* d_mask, size_t mask_cap, size_t& mask_len,
                                size_t& nmissing, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const int m = mode == CompMode::Rate ? 1 : mode == CompMode::PSNR ? 2 : mode == CompMode::PWE ? 3 : 0;
  if (m == 0)
    return RTNType::CompModeUnknown;
  return detail::mask_rtn(sperrhip_compress_masked_fill_dev(d_src, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0],
                                                            chunks[1], chunks[2], m, quality, static_cast<int>(rule),
                                                            threshold, static_cast<int>(fill), fill_value, d_out, cap,
                                                            &out_len, d_mask, mask_cap, &mask_len, &nmissing,
                                                            hip_stream));
}

// the volume (null box) or a box of it, from the first pct percent of every chunk stream (0: all), `value` at the
// missing samples
template <typename T>
inline auto decompress_masked_dev(const void* d_stream, size_t stream_len, const void* d_mask, size_t mask_len,
                                  double value, T* d_out, size_t cap_bytes, const dims_type* box_lo = nullptr,
                                  const dims_type* box_dims = nullptr, unsigned pct = 0, void* hip_stream = nullptr)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_decompress_masked_dev(d_stream, stream_len, pct, sizeof(T) == 4,
                                                         box_lo ? box_lo->data() : nullptr,
                                                         box_dims ? box_dims->data() : nullptr, d_mask, mask_len, value,
                                                         d_out, cap_bytes, hip_stream));
}

// quality_dev of the valid samples of two arrays
template <typename T>
inline auto quality_masked_dev(const T* d_orig, const T* d_recon, size_t n, const void* d_mask, size_t mask_len,
                               std::array<double, 8>& out, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_quality_masked_dev(d_orig, d_recon, sizeof(T) == 4, n, d_mask, mask_len, out.data(),
                                                      hip_stream));
}

// (this library's addition) Point-wise relative error (include/sperr_hip.h, "relative error"): |x' - x| <= eps |x|, zeros
// and signs exact; a container of the double volume y and a side stream.  RTNType::WrongLength: the side buffer (or the
// container's) is too small, side_len then names the size needed.
// The map kind: y is the piecewise linear interpolant of log2|x| (the default) or log2|x| itself, which gives the smaller
// container.  A decode takes it from the side stream.
enum class RelMap : int { linear = SPERRHIP_REL_LINEAR, log = SPERRHIP_REL_LOG };

// t of eps for fp32 (T = float) or fp64 data; Error: eps is refused
template <typename T>
inline auto rel_tolerance(double eps, double& t, RelMap map = RelMap::linear) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_rel_tolerance_kind(eps, sizeof(T) == 4, static_cast<int>(map), &t));
}

// y of n samples into d_y and their side stream (which states no bound) into d_side
template <typename T>
inline auto rel_forward_dev(const T* d_src, size_t n, double* d_y, void* d_side, size_t side_cap, size_t& side_len,
                            size_t& nzero, size_t& nneg, void* hip_stream = nullptr, RelMap map = RelMap::linear)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_rel_forward_kind_dev(d_src, sizeof(T) == 4, n, static_cast<int>(map), d_y, d_side,
                                                        side_cap, &side_len, &nzero, &nneg, hip_stream));
}

// x' of y' of the box of a volume that d_y holds (null box: the whole volume); d_out may be d_y when T is double
template <typename T>
inline auto rel_inverse_dev(const double* d_y, dims_type vol_dims, const dims_type* box_lo, const dims_type* box_dims,
                            const void* d_side, size_t side_len, T* d_out, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_rel_inverse_dev(d_y, vol_dims.data(), box_lo ? box_lo->data() : nullptr,
                                                   box_dims ? box_dims->data() : nullptr, d_side, side_len,
                                                   sizeof(T) == 4, d_out, hip_stream));
}

// fill_value (y's domain) is read by FillKind::Value alone
template <typename T>
inline auto compress_rel_dev(const T* d_src, dims_type dims, dims_type chunks, double eps, FillKind fill,
                             double fill_value, void* d_out, size_t cap, size_t& out_len, void* d_side, size_t side_cap,
                             size_t& side_len, void* hip_stream = nullptr, RelMap map = RelMap::linear) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_compress_rel_kind_dev(d_src, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0],
                                                         chunks[1], chunks[2], eps, static_cast<int>(map),
                                                         static_cast<int>(fill), fill_value, d_out, cap, &out_len,
                                                         d_side, side_cap, &side_len, hip_stream));
}

// the volume (null box) or a box of it, from the first pct percent of every chunk stream (0: all; a portion carries no
// bound)
template <typename T>
inline auto decompress_rel_dev(const void* d_stream, size_t stream_len, const void* d_side, size_t side_len, T* d_out,
                               size_t cap_bytes, const dims_type* box_lo = nullptr, const dims_type* box_dims = nullptr,
                               unsigned pct = 0, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_decompress_rel_dev(d_stream, stream_len, pct, sizeof(T) == 4,
                                                      box_lo ? box_lo->data() : nullptr,
                                                      box_dims ? box_dims->data() : nullptr, d_side, side_len, d_out,
                                                      cap_bytes, hip_stream));
}

// out: the largest |x' - x| / |x|, the samples beyond eps, the samples that differ in zero class or sign, the samples
// whose original is no zero
template <typename T>
inline auto rel_check_dev(const T* d_orig, const T* d_recon, size_t n, double eps, std::array<double, 4>& out,
                          void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_rel_check_dev(d_orig, d_recon, sizeof(T) == 4, n, eps, out.data(), hip_stream));
}

// ---- compression to a byte target (the size mode, sperr_hip.h) ----
// A volume's survey: what every threshold would cost.  The vectors get one entry per chunk in container order, `end`
// 32 per chunk (end[c * 32 + p]: the payload bits of chunk c's stream at the end of bit plane p)
struct SizeSurvey {
  std::vector<double> q;
  std::vector<int32_t> nbp;
  std::vector<uint64_t> end;
  std::vector<uint8_t> is_const;
};

template <typename T>
inline auto size_survey_dev(const T* d_src, dims_type dims, dims_type chunks, SizeSurvey& out, void* hip_stream = nullptr)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  const size_t n = sperrhip_chunk_count(dims[0], dims[1], dims[2], chunks[0], chunks[1], chunks[2]);
  out.q.assign(n, 0.0);
  out.nbp.assign(n, 0);
  out.end.assign(n * 32, 0);
  out.is_const.assign(n, 0);
  return detail::mask_rtn(sperrhip_size_survey_dev(d_src, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0], chunks[1],
                                                   chunks[2], n, out.q.data(), out.nbp.data(), out.end.data(),
                                                   out.is_const.data(), hip_stream));
}

// A container of at most target_bytes bytes whose chunks all stop at (nearly) the same absolute threshold; budgets (may
// be null): every chunk's budget in bits.  Error, with nothing written to d_out, when the target does not hold the
// headers and a payload byte per chunk
template <typename T>
inline auto compress_size_dev(const T* d_src, dims_type dims, dims_type chunks, size_t target_bytes, void* d_out, size_t cap,
                              size_t& out_len, std::vector<uint64_t>* budgets = nullptr, void* hip_stream = nullptr)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  if (budgets)
    budgets->assign(sperrhip_chunk_count(dims[0], dims[1], dims[2], chunks[0], chunks[1], chunks[2]), 0);
  return detail::mask_rtn(sperrhip_compress_size_dev(d_src, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0], chunks[1],
                                                     chunks[2], target_bytes, d_out, cap, &out_len,
                                                     budgets ? budgets->data() : nullptr, budgets ? budgets->size() : 0,
                                                     hip_stream));
}

// ---- compression to a PSNR of the whole volume (sperr_hip.h) ----
// The smallest and the largest sample of a device volume, dense (view null) or a view.  Error when a sample is a NaN
template <typename T>
inline auto range_dev(const T* d_src, dims_type dims, double& vmin, double& vmax, const view_type* view = nullptr,
                      void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_range_dev(d_src, view, sizeof(T) == 4, dims[0], dims[1], dims[2], &vmin, &vmax, hip_stream));
}

// A container whose chunks are all coded to `psnr` dB of one range: the volume's own (range 0) or the caller's.  cap as
// sperrhip_max_compressed_size(..., 2, psnr) says.  Error, with nothing written, for a volume with a NaN or an infinity
template <typename T>
inline auto compress_psnr_dev(const T* d_src, dims_type dims, dims_type chunks, double psnr, void* d_out, size_t cap,
                              size_t& out_len, double range = 0.0, const view_type* view = nullptr,
                              void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_compress_psnr_dev(d_src, view, sizeof(T) == 4, dims[0], dims[1], dims[2], chunks[0], chunks[1],
                                                     chunks[2], psnr, range, d_out, cap, &out_len, hip_stream));
}

// ---- time series: a Haar transform across the steps (sperr_hip.h) ----
enum class SeriesKind : int { tol = SPERRHIP_SERIES_TOL, psnr = SPERRHIP_SERIES_PSNR };
using series_info_type = std::array<uint8_t, SPERRHIP_SERIES_INFO_BYTES>;

// the groups of a series: {first step, levels} each.  Host only; empty for arguments the library refuses
inline auto series_plan(size_t nsteps, unsigned levels) -> std::vector<std::pair<size_t, unsigned>>
{
  size_t ng = 0;
  if (sperrhip_series_plan(nsteps, levels, &ng, nullptr, nullptr, 0) != 0)
    return {};
  std::vector<size_t> starts(ng);
  std::vector<unsigned> lv(ng);
  std::vector<std::pair<size_t, unsigned>> out;
  if (sperrhip_series_plan(nsteps, levels, &ng, starts.data(), lv.data(), ng) == 0)
    for (size_t i = 0; i < ng; i++)
      out.emplace_back(starts[i], lv[i]);
  return out;
}

// the bands (= containers) a decode of the steps [t0, t0 + nt) needs, in order.  Host only; empty when refused
inline auto series_needs(size_t nsteps, unsigned levels, size_t t0, size_t nt) -> std::vector<size_t>
{
  std::vector<unsigned char> need(nsteps);
  std::vector<size_t> out;
  if (nsteps != 0 && sperrhip_series_needs(nsteps, levels, t0, nt, need.data(), nullptr) == 0)
    for (size_t b = 0; b < nsteps; b++)
      if (need[b])
        out.push_back(b);
  return out;
}

// rho and tau[0 .. levels] of a tolerance and the series' largest |sample|.  Host only
inline auto series_tolerance(double tol, double maxabs, unsigned levels, double& rho, std::vector<double>& tau) -> RTNType
{
  tau.assign(5, 0.0);
  const int rtn = sperrhip_series_tolerance(tol, maxabs, levels, &rho, tau.data());
  tau.resize(rtn == 0 ? levels + 1 : 0);
  return detail::mask_rtn(rtn);
}

// Stage access: the steps (device pointers, one per step, n samples each) into nsteps dense bands of n doubles at d_bands
template <typename T>
inline auto series_forward_dev(const std::vector<const T*>& d_steps, unsigned levels, size_t n, double* d_bands,
                               void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_series_forward_dev(reinterpret_cast<const void* const*>(d_steps.data()), sizeof(T) == 4,
                                                      d_steps.size(), levels, n, d_bands, hip_stream));
}

// ... and the steps [t0, t0 + d_outs.size()) of the bands back
template <typename T>
inline auto series_inverse_dev(const double* d_bands, size_t nsteps, unsigned levels, size_t n, size_t t0,
                               const std::vector<T*>& d_outs, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_series_inverse_dev(d_bands, nsteps, levels, n, t0, d_outs.size(), sizeof(T) == 4,
                                                      reinterpret_cast<void* const*>(d_outs.data()), hip_stream));
}

// A series of d_steps.size() steps into as many containers back to back at d_out: container b at [offsets[b],
// offsets[b + 1]).  quality: the tolerance, or the PSNR in dB of `range` (0: the series' own).  cap as
// sperrhip_max_compressed_size_batch(steps, ..., 3 or 2, quality) says
template <typename T>
inline auto compress_series_dev(const std::vector<const T*>& d_steps, dims_type dims, dims_type chunks, unsigned levels,
                                SeriesKind kind, double quality, void* d_out, size_t cap, std::vector<size_t>& offsets,
                                series_info_type& info, double range = 0.0, void* hip_stream = nullptr) -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  offsets.assign(d_steps.size() + 1, 0);
  return detail::mask_rtn(sperrhip_compress_series_dev(reinterpret_cast<const void* const*>(d_steps.data()), sizeof(T) == 4,
                                                       d_steps.size(), dims[0], dims[1], dims[2], chunks[0], chunks[1],
                                                       chunks[2], levels, static_cast<int>(kind), quality, range, d_out, cap,
                                                       offsets.data(), info.data(), hip_stream));
}

// The steps [t0, t0 + d_outs.size()) of a series, whole or a box of every step (both null: whole), from the first pct
// percent of every chunk stream.  The outputs are untouched when the call fails
template <typename T>
inline auto decompress_series_dev(const series_info_type& info, const void* d_streams, const std::vector<size_t>& offsets,
                                  size_t t0, const std::vector<T*>& d_outs, const dims_type* box_lo = nullptr,
                                  const dims_type* box_dims = nullptr, unsigned pct = 0, void* hip_stream = nullptr)
    -> RTNType
{
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
  return detail::mask_rtn(sperrhip_decompress_series_dev(info.data(), d_streams, offsets.data(), t0, d_outs.size(),
                                                         box_lo ? box_lo->data() : nullptr,
                                                         box_dims ? box_dims->data() : nullptr, pct, sizeof(T) == 4,
                                                         reinterpret_cast<void* const*>(d_outs.data()), hip_stream));
}

}  // namespace sperr

#endif
