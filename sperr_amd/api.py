"""Python binding of libsperr_hip.so (ctypes) -- plumbing for tests and bench.py.

torch is used only for device memory, streams and (in bench.py) torch.distributed; the compute
path is the C-ABI library declared in include/sperr_hip.h.  There is no CPU fallback: importing
works anywhere, but every call needs a GPU and raises if the library is missing or a call fails.
"""
import ctypes as C
import math
import os

import numpy as np

# the decoder runs the shape groups of a volume side by side on up to 8 streams: ask the ROCm runtime
# for as many hardware queues (default 4; only read at the process's first HIP call)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SPERR_HIP_LIB: another build of the same library, e.g. one with diagnostic switches compiled in)
LIB_PATH = os.environ.get("SPERR_HIP_LIB") or os.path.join(_HERE, "libsperr_hip.so")
_sz, _vp = C.c_size_t, C.c_void_p
builtins_range = range   # (compress_to_psnr and compress_series have a parameter of that name)

# every symbol include/sperr_hip.h declares
EXPORTS = [
    "sperr_comp_3d", "sperr_decomp_3d", "sperr_parse_header", "sperr_trunc_3d",
    "sperrhip_max_compressed_size", "sperrhip_compress_dev", "sperrhip_decompress_dev",
    "sperrhip_parse_header_dev", "sperrhip_parse_header_stream_dev", "sperrhip_dwt3d_dev", "sperrhip_speck3d_encode_dev",
    "sperrhip_speck3d_decode_dev", "sperrhip_outlier_encode_dev", "sperrhip_profile_enable", "sperrhip_profile_reset",
    "sperrhip_profile_get", "sperrhip_profile_get2", "sperrhip_profile_only",
    "sperrhip_multires_levels", "sperrhip_decompress_multires_dev", "sperrhip_decomp_3d_multires",
    "sperr_comp_2d", "sperr_decomp_2d", "sperrhip_max_compressed_size_2d", "sperrhip_compress_2d_dev",
    "sperrhip_decompress_2d_dev", "sperrhip_version", "sperrhip_debug_lis_stamps",
    "sperrhip_multires_levels_2d", "sperrhip_decompress_2d_multires_dev", "sperrhip_decomp_2d_multires",
    "sperrhip_comp_3d_farm", "sperrhip_decomp_3d_farm", "sperrhip_decomp_3d_into",
    "sperrhip_farm_selftest", "sperrhip_release", "sperrhip_debug_counter",
    "sperrhip_numa_probe", "sperrhip_numa_bind_self", "sperrhip_farm_device_place",
    "sperrhip_host_cpus", "sperrhip_host_throttle", "sperrhip_farm_threads",
    "sperrhip_box_chunks", "sperrhip_decompress_box_dev", "sperrhip_decomp_3d_box",
    "sperrhip_max_compressed_size_batch", "sperrhip_compress_batch_dev", "sperrhip_decompress_batch_dev",
    "sperrhip_max_compressed_size_2d_batch", "sperrhip_compress_2d_batch_dev", "sperrhip_decompress_2d_batch_dev",
    "sperrhip_decompress_level_dev", "sperrhip_decomp_3d_level",
    "sperrhip_portion_len", "sperrhip_decompress_portion_dev", "sperrhip_decomp_3d_portion",
    "sperrhip_trunc_dev", "sperrhip_trunc_batch_dev",
    "sperrhip_quality_dev", "sperrhip_quality_batch_dev",
    "sperrhip_compress_view_dev", "sperrhip_decompress_view_dev", "sperrhip_quality_view_dev",
    "sperrhip_compress_fields_dev", "sperrhip_decompress_fields_dev", "sperrhip_quality_fields_dev",
    "sperrhip_fields_gather_dev", "sperrhip_fields_scatter_dev",
    "sperrhip_boxes_plan", "sperrhip_decompress_boxes_dev",
    "sperrhip_mask_max_size", "sperrhip_mask_make_dev", "sperrhip_mask_parse_dev", "sperrhip_mask_parse_stream_dev",
    "sperrhip_mask_apply_dev",
    "sperrhip_mask_expand_dev", "sperrhip_compress_masked_dev", "sperrhip_decompress_masked_dev",
    "sperrhip_quality_masked_dev", "sperrhip_mask_make_vol_dev", "sperrhip_compress_masked_fill_dev",
    "sperrhip_rel_tolerance", "sperrhip_rel_max_size", "sperrhip_rel_forward_dev", "sperrhip_rel_inverse_dev",
    "sperrhip_compress_rel_dev", "sperrhip_decompress_rel_dev", "sperrhip_rel_parse_stream_dev",
    "sperrhip_rel_check_dev",
    "sperrhip_rel_tolerance_kind", "sperrhip_rel_forward_kind_dev", "sperrhip_compress_rel_kind_dev",
    "sperrhip_rel_parse_stream_kind_dev",
    "sperrhip_speck3d_plane_bits_dev", "sperrhip_chunk_count", "sperrhip_size_survey_dev", "sperrhip_compress_size_dev",
    "sperrhip_psnr_ladder", "sperrhip_range_dev", "sperrhip_compress_psnr_dev",
    "sperrhip_series_plan", "sperrhip_series_needs", "sperrhip_series_tolerance", "sperrhip_series_parse",
    "sperrhip_series_forward_dev", "sperrhip_series_inverse_dev", "sperrhip_compress_series_dev",
    "sperrhip_decompress_series_dev",
]


class SperrHipError(RuntimeError):
    pass


class View(C.Structure):
    """sperrhip_view: the pitches of a strided view in elements (include/sperr_hip.h)"""
    _fields_ = [("pitch_y", _sz), ("pitch_z", _sz)]


class Fields(C.Structure):
    """sperrhip_fields: the layout of an interleaved array in elements (include/sperr_hip.h)"""
    _fields_ = [("stride_x", _sz), ("pitch_y", _sz), ("pitch_z", _sz)]


class Quality:
    """The figures of one reconstruction against its original (SperrHip.quality): rmse, linfty, psnr, mse, and
    the original's min, max, mean, var and sigma = sqrt(var); with the compressed size known also bitrate and
    accuracy_gain (None otherwise).  Values of the arrays' type widened to float."""
    __slots__ = ("rmse", "linfty", "psnr", "min", "max", "mean", "var", "mse", "sigma", "bitrate", "accuracy_gain")

    def __init__(self, figs, n, nbytes=None):
        self.rmse, self.linfty, self.psnr, self.min, self.max, self.mean, self.var, self.mse = figs
        self.sigma = math.sqrt(self.var)
        self.bitrate = self.accuracy_gain = None
        if nbytes is not None:
            # as the reference's tool prints them (utilities/sperr3d.cpp:380-382), in double
            self.bitrate = 8.0 * nbytes / n
            with np.errstate(divide="ignore"):
                self.accuracy_gain = float(np.log2(np.float64(self.sigma) / np.float64(self.rmse))) - self.bitrate

    def __repr__(self):
        return "Quality(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


def host_cpus(lib):
    """CPUs this process may use, as the library's farm sees them (sperr_amd/csrc/host_cpus.hpp): the machine's
    count, the affinity mask, the cgroup's CFS quota in CPUs (0.0: none) and the smallest of them."""
    vis, aff, use = _sz(0), _sz(0), _sz(0)
    quota = C.c_double(0.0)
    lib.sperrhip_host_cpus.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_double),
                                       C.POINTER(_sz)]
    rc = lib.sperrhip_host_cpus(None, None, C.byref(vis), C.byref(aff), C.byref(quota), C.byref(use))
    if rc != 0:
        raise SperrHipError(f"sperrhip_host_cpus returned {rc}")
    return {"cores_visible": vis.value, "affinity": aff.value, "cpu_quota": quota.value or None, "usable": use.value}


def box_chunks(lib, vol_xyz, chunks_xyz, box_lo_xyz, box_dims_xyz):
    """ids (chunk_volume order) of the chunks that the box [lo, lo + dims) of a volume meets; host only.
    Raises SperrHipError for an empty box or one that leaves the volume."""
    lo, dims, count = (_sz * 3)(*box_lo_xyz), (_sz * 3)(*box_dims_xyz), _sz(0)
    rc = lib.sperrhip_box_chunks(*vol_xyz, *chunks_xyz, lo, dims, None, 0, C.byref(count))
    if rc == 1:
        ids = (C.c_uint32 * max(count.value, 1))()
        rc = lib.sperrhip_box_chunks(*vol_xyz, *chunks_xyz, lo, dims, ids, count.value, C.byref(count))
    if rc != 0:
        raise SperrHipError(f"sperrhip_box_chunks returned {rc}")
    return list(ids[:count.value])


def host_throttle(lib):
    """(nr_throttled, throttled_usec) of the process's cgroup so far, or None when there is no cpu.stat"""
    nr, us = C.c_ulonglong(0), C.c_ulonglong(0)
    lib.sperrhip_host_throttle.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    if lib.sperrhip_host_throttle(None, None, C.byref(nr), C.byref(us)) != 0:
        return None
    return nr.value, us.value


def load_library():
    if not os.path.exists(LIB_PATH):
        raise SperrHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch brings a HIP runtime of its own: when the library is loaded first it binds to the system's,
    # and a process with two runtimes does not see the GPU through the second one.  Callers here move
    # their data with torch anyway, so its runtime is loaded first and serves both.
    try:
        import torch  # noqa: F401
    except Exception:   # noqa: BLE001  (the loader itself does not need it)
        pass
    lib = C.CDLL(LIB_PATH)
    lib.sperr_comp_3d.restype = C.c_int
    lib.sperr_comp_3d.argtypes = [_vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int, C.c_double,
                                  _sz, C.POINTER(_vp), C.POINTER(_sz)]
    lib.sperr_decomp_3d.restype = C.c_int
    lib.sperr_decomp_3d.argtypes = [_vp, _sz, C.c_int, _sz, C.POINTER(_sz), C.POINTER(_sz),
                                    C.POINTER(_sz), C.POINTER(_vp)]
    lib.sperr_parse_header.restype = None
    lib.sperr_parse_header.argtypes = [_vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz),
                                       C.POINTER(C.c_int)]
    lib.sperr_trunc_3d.restype = C.c_int
    lib.sperr_trunc_3d.argtypes = [_vp, _sz, C.c_uint, C.POINTER(_vp), C.POINTER(_sz)]
    lib.sperrhip_max_compressed_size.restype = _sz
    lib.sperrhip_max_compressed_size.argtypes = [_sz] * 6 + [C.c_int, C.c_double]
    lib.sperrhip_compress_dev.restype = C.c_int
    lib.sperrhip_compress_dev.argtypes = [_vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int,
                                          C.c_double, _vp, _sz, C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_dev.restype = C.c_int
    lib.sperrhip_decompress_dev.argtypes = [_vp, _sz, C.c_int, _vp, _sz, C.POINTER(_sz),
                                            C.POINTER(_sz), C.POINTER(_sz), _vp]
    lib.sperrhip_max_compressed_size_batch.restype = _sz
    lib.sperrhip_max_compressed_size_batch.argtypes = [_sz] * 7 + [C.c_int, C.c_double]
    lib.sperrhip_compress_batch_dev.restype = C.c_int
    lib.sperrhip_compress_batch_dev.argtypes = [_vp, C.c_int] + [_sz] * 7 + [C.c_int, C.c_double, _vp, _sz,
                                                                             C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_batch_dev.restype = C.c_int
    lib.sperrhip_decompress_batch_dev.argtypes = [_vp, C.POINTER(_sz), _sz, C.c_int, _vp, _sz] + \
        [C.POINTER(_sz)] * 3 + [_vp]
    lib.sperrhip_max_compressed_size_2d_batch.restype = _sz
    lib.sperrhip_max_compressed_size_2d_batch.argtypes = [_sz, _sz, _sz, C.c_int, C.c_double]
    lib.sperrhip_compress_2d_batch_dev.restype = C.c_int
    lib.sperrhip_compress_2d_batch_dev.argtypes = [_vp, C.c_int, _sz, _sz, _sz, C.c_int, C.c_double, C.c_int, _vp, _sz,
                                                   C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_2d_batch_dev.restype = C.c_int
    lib.sperrhip_decompress_2d_batch_dev.argtypes = [_vp, C.POINTER(_sz), _sz, C.c_int, C.c_int, _sz, _sz, _vp, _sz,
                                                     _vp]
    lib.sperrhip_box_chunks.restype = C.c_int
    lib.sperrhip_box_chunks.argtypes = [_sz] * 6 + [C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_uint32), _sz,
                                                    C.POINTER(_sz)]
    lib.sperrhip_decompress_box_dev.restype = C.c_int
    lib.sperrhip_decompress_box_dev.argtypes = [_vp, _sz, C.c_int, C.POINTER(_sz), C.POINTER(_sz), _vp, _sz, _vp]
    lib.sperrhip_decomp_3d_box.restype = C.c_int
    lib.sperrhip_decomp_3d_box.argtypes = [_vp, _sz, C.c_int, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_vp)]
    lib.sperrhip_decompress_level_dev.restype = C.c_int
    lib.sperrhip_decompress_level_dev.argtypes = [_vp, _sz, C.c_int, _sz, C.POINTER(_sz), C.POINTER(_sz), _vp, _sz, _vp]
    lib.sperrhip_decomp_3d_level.restype = C.c_int
    lib.sperrhip_decomp_3d_level.argtypes = [_vp, _sz, C.c_int, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz),
                                             C.POINTER(_vp)]
    lib.sperrhip_portion_len.restype = _sz
    lib.sperrhip_portion_len.argtypes = [_sz, C.c_uint]
    lib.sperrhip_decompress_portion_dev.restype = C.c_int
    lib.sperrhip_decompress_portion_dev.argtypes = [_vp, _sz, C.c_uint, C.c_int, C.POINTER(_sz), C.POINTER(_sz),
                                                    C.POINTER(_sz), _vp, _sz, _vp]
    lib.sperrhip_decomp_3d_portion.restype = C.c_int
    lib.sperrhip_decomp_3d_portion.argtypes = [_vp, _sz, C.c_uint, C.c_int, C.POINTER(_sz), C.POINTER(_sz),
                                               C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_vp)]
    lib.sperrhip_trunc_dev.restype = C.c_int
    lib.sperrhip_trunc_dev.argtypes = [_vp, _sz, C.c_uint, _vp, _sz, C.POINTER(_sz), _vp]
    lib.sperrhip_trunc_batch_dev.restype = C.c_int
    lib.sperrhip_trunc_batch_dev.argtypes = [_vp, C.POINTER(_sz), _sz, C.c_uint, _vp, _sz, C.POINTER(_sz), _vp]
    lib.sperrhip_quality_dev.restype = C.c_int
    lib.sperrhip_quality_dev.argtypes = [_vp, _vp, C.c_int, _sz, C.POINTER(C.c_double), _vp]
    lib.sperrhip_quality_batch_dev.restype = C.c_int
    lib.sperrhip_quality_batch_dev.argtypes = [_vp, _vp, C.c_int, _sz, _sz, C.POINTER(C.c_double), _vp]
    lib.sperrhip_compress_view_dev.restype = C.c_int
    lib.sperrhip_compress_view_dev.argtypes = [_vp, C.POINTER(View), C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int,
                                               C.c_double, _vp, _sz, C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_view_dev.restype = C.c_int
    lib.sperrhip_decompress_view_dev.argtypes = [_vp, _sz, C.c_uint, C.c_int, C.POINTER(_sz), C.POINTER(_sz), _vp,
                                                 C.POINTER(View), _sz, _vp]
    lib.sperrhip_quality_view_dev.restype = C.c_int
    lib.sperrhip_quality_view_dev.argtypes = [_vp, C.POINTER(View), _vp, C.POINTER(View), C.c_int, _sz, _sz, _sz,
                                              C.POINTER(C.c_double), _vp]
    lib.sperrhip_compress_fields_dev.restype = C.c_int
    lib.sperrhip_compress_fields_dev.argtypes = [_vp, C.POINTER(Fields), _sz, C.c_int] + [_sz] * 6 + \
        [C.c_int, C.c_double, _vp, _sz, C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_fields_dev.restype = C.c_int
    lib.sperrhip_decompress_fields_dev.argtypes = [_vp, C.POINTER(_sz), _sz, C.c_int, _sz, _sz, _sz, _vp,
                                                   C.POINTER(Fields), _sz, _vp]
    lib.sperrhip_quality_fields_dev.restype = C.c_int
    lib.sperrhip_quality_fields_dev.argtypes = [_vp, C.POINTER(Fields), _vp, C.POINTER(Fields), _sz, C.c_int, _sz, _sz,
                                                _sz, C.POINTER(C.c_double), _vp]
    lib.sperrhip_fields_gather_dev.restype = C.c_int
    lib.sperrhip_fields_gather_dev.argtypes = [_vp, C.POINTER(Fields), _sz, C.c_int, _sz, _sz, _sz, _vp, _sz, _vp]
    lib.sperrhip_fields_scatter_dev.restype = C.c_int
    lib.sperrhip_fields_scatter_dev.argtypes = [_vp, _sz, C.c_int, _sz, _sz, _sz, _vp, C.POINTER(Fields), _sz, _vp]
    lib.sperrhip_boxes_plan.restype = C.c_int
    lib.sperrhip_boxes_plan.argtypes = [_sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_uint32), C.POINTER(_sz), _sz,
                                        C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]
    lib.sperrhip_decompress_boxes_dev.restype = C.c_int
    lib.sperrhip_decompress_boxes_dev.argtypes = [C.POINTER(_vp), C.POINTER(_sz), _sz, C.POINTER(C.c_uint32),
                                                  C.POINTER(_sz), _sz, C.POINTER(_sz), C.POINTER(_sz), C.c_uint,
                                                  C.c_int, _vp, _sz, _vp]
    lib.sperrhip_mask_max_size.restype = _sz
    lib.sperrhip_mask_max_size.argtypes = [_sz]
    lib.sperrhip_mask_make_dev.restype = C.c_int
    lib.sperrhip_mask_make_dev.argtypes = [_vp, C.c_int, _sz, C.c_int, C.c_double, _vp, _vp, _sz, C.POINTER(_sz),
                                           C.POINTER(_sz), _vp]
    lib.sperrhip_mask_make_vol_dev.restype = C.c_int
    lib.sperrhip_mask_make_vol_dev.argtypes = [_vp, C.c_int, _sz, _sz, _sz, C.c_int, C.c_double, C.c_int, C.c_double,
                                               _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz), _vp]
    lib.sperrhip_compress_masked_fill_dev.restype = C.c_int
    lib.sperrhip_compress_masked_fill_dev.argtypes = [_vp, C.c_int] + [_sz] * 6 + \
        [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, _vp, _sz, C.POINTER(_sz), _vp, _sz,
         C.POINTER(_sz), C.POINTER(_sz), _vp]
    lib.sperrhip_mask_parse_dev.restype = C.c_int
    lib.sperrhip_mask_parse_dev.argtypes = [_vp, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_int)]
    lib.sperrhip_mask_parse_stream_dev.restype = C.c_int
    lib.sperrhip_mask_parse_stream_dev.argtypes = [_vp, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_int), _vp]
    lib.sperrhip_mask_apply_dev.restype = C.c_int
    lib.sperrhip_mask_apply_dev.argtypes = [_vp, C.c_int, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _vp, _sz,
                                            C.c_double, _vp]
    lib.sperrhip_mask_expand_dev.restype = C.c_int
    lib.sperrhip_mask_expand_dev.argtypes = [_vp, _sz, _vp, _sz, _vp]
    lib.sperrhip_compress_masked_dev.restype = C.c_int
    lib.sperrhip_compress_masked_dev.argtypes = [_vp, C.c_int] + [_sz] * 6 + [C.c_int, C.c_double, C.c_int, C.c_double,
                                                                             _vp, _sz, C.POINTER(_sz), _vp, _sz,
                                                                             C.POINTER(_sz), C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_masked_dev.restype = C.c_int
    lib.sperrhip_decompress_masked_dev.argtypes = [_vp, _sz, C.c_uint, C.c_int, C.POINTER(_sz), C.POINTER(_sz), _vp,
                                                   _sz, C.c_double, _vp, _sz, _vp]
    lib.sperrhip_quality_masked_dev.restype = C.c_int
    lib.sperrhip_quality_masked_dev.argtypes = [_vp, _vp, C.c_int, _sz, _vp, _sz, C.POINTER(C.c_double), _vp]
    lib.sperrhip_rel_tolerance.restype = C.c_int
    lib.sperrhip_rel_tolerance.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_double)]
    lib.sperrhip_rel_max_size.restype = _sz
    lib.sperrhip_rel_max_size.argtypes = [_sz]
    lib.sperrhip_rel_forward_dev.restype = C.c_int
    lib.sperrhip_rel_forward_dev.argtypes = [_vp, C.c_int, _sz, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz),
                                             C.POINTER(_sz), _vp]
    lib.sperrhip_rel_inverse_dev.restype = C.c_int
    lib.sperrhip_rel_inverse_dev.argtypes = [_vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _vp, _sz, C.c_int,
                                             _vp, _vp]
    lib.sperrhip_compress_rel_dev.restype = C.c_int
    lib.sperrhip_compress_rel_dev.argtypes = [_vp, C.c_int] + [_sz] * 6 + [C.c_double, C.c_int, C.c_double, _vp, _sz,
                                                                          C.POINTER(_sz), _vp, _sz, C.POINTER(_sz), _vp]
    lib.sperrhip_decompress_rel_dev.restype = C.c_int
    lib.sperrhip_decompress_rel_dev.argtypes = [_vp, _sz, C.c_uint, C.c_int, C.POINTER(_sz), C.POINTER(_sz), _vp, _sz,
                                                _vp, _sz, _vp]
    lib.sperrhip_rel_parse_stream_dev.restype = C.c_int
    lib.sperrhip_rel_parse_stream_dev.argtypes = [_vp, _sz, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(_sz),
                                                  C.POINTER(_sz), C.POINTER(_sz), _vp]
    lib.sperrhip_rel_tolerance_kind.restype = C.c_int
    lib.sperrhip_rel_tolerance_kind.argtypes = [C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.sperrhip_rel_forward_kind_dev.restype = C.c_int
    lib.sperrhip_rel_forward_kind_dev.argtypes = [_vp, C.c_int, _sz, C.c_int, _vp, _vp, _sz, C.POINTER(_sz),
                                                  C.POINTER(_sz), C.POINTER(_sz), _vp]
    lib.sperrhip_compress_rel_kind_dev.restype = C.c_int
    lib.sperrhip_compress_rel_kind_dev.argtypes = [_vp, C.c_int] + [_sz] * 6 + [C.c_double, C.c_int, C.c_int, C.c_double,
                                                                               _vp, _sz, C.POINTER(_sz), _vp, _sz,
                                                                               C.POINTER(_sz), _vp]
    lib.sperrhip_rel_parse_stream_kind_dev.restype = C.c_int
    lib.sperrhip_rel_parse_stream_kind_dev.argtypes = [_vp, _sz, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                       C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz),
                                                       C.POINTER(C.c_int), _vp]
    lib.sperrhip_rel_check_dev.restype = C.c_int
    lib.sperrhip_rel_check_dev.argtypes = [_vp, _vp, C.c_int, _sz, C.c_double, C.POINTER(C.c_double), _vp]
    lib.sperrhip_parse_header_dev.restype = C.c_int
    lib.sperrhip_parse_header_dev.argtypes = [_vp, _sz] + [C.POINTER(_sz)] * 3 + \
        [C.POINTER(C.c_int)] + [C.POINTER(_sz)] * 3
    lib.sperrhip_parse_header_stream_dev.restype = C.c_int
    lib.sperrhip_parse_header_stream_dev.argtypes = lib.sperrhip_parse_header_dev.argtypes + [_vp]
    lib.sperrhip_dwt3d_dev.restype = C.c_int
    lib.sperrhip_dwt3d_dev.argtypes = [_vp, _sz, _sz, _sz, C.c_int, _vp]
    lib.sperrhip_speck3d_plane_bits_dev.restype = C.c_int
    lib.sperrhip_speck3d_plane_bits_dev.argtypes = [_vp, C.c_int, _vp, _sz, _sz, _sz, _vp, C.POINTER(C.c_int), _vp]
    lib.sperrhip_size_survey_dev.restype = C.c_int
    lib.sperrhip_chunk_count.restype = _sz
    lib.sperrhip_chunk_count.argtypes = [_sz] * 6
    lib.sperrhip_size_survey_dev.argtypes = [_vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _vp]
    lib.sperrhip_compress_size_dev.restype = C.c_int
    lib.sperrhip_compress_size_dev.argtypes = [_vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, _sz, _vp, _sz,
                                               C.POINTER(_sz), _vp, _sz, _vp]
    lib.sperrhip_psnr_ladder.restype = C.c_int
    lib.sperrhip_psnr_ladder.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double), _vp]
    lib.sperrhip_range_dev.restype = C.c_int
    lib.sperrhip_range_dev.argtypes = [_vp, _vp, C.c_int, _sz, _sz, _sz, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp]
    lib.sperrhip_compress_psnr_dev.restype = C.c_int
    lib.sperrhip_compress_psnr_dev.argtypes = [_vp, _vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, C.c_double, C.c_double,
                                               _vp, _sz, C.POINTER(_sz), _vp]
    _dp = C.POINTER(C.c_double)
    lib.sperrhip_series_plan.restype = C.c_int
    lib.sperrhip_series_plan.argtypes = [_sz, C.c_uint, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(C.c_uint), _sz]
    lib.sperrhip_series_needs.restype = C.c_int
    lib.sperrhip_series_needs.argtypes = [_sz, C.c_uint, _sz, _sz, C.POINTER(C.c_ubyte), C.POINTER(_sz)]
    lib.sperrhip_series_tolerance.restype = C.c_int
    lib.sperrhip_series_tolerance.argtypes = [C.c_double, C.c_double, C.c_uint, _dp, _dp]
    lib.sperrhip_series_parse.restype = C.c_int
    lib.sperrhip_series_parse.argtypes = [C.c_char_p, C.POINTER(_sz), C.POINTER(C.c_uint), C.POINTER(_sz),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp, _dp, _dp]
    lib.sperrhip_series_forward_dev.restype = C.c_int
    lib.sperrhip_series_forward_dev.argtypes = [C.POINTER(_vp), C.c_int, _sz, C.c_uint, _sz, _vp, _vp]
    lib.sperrhip_series_inverse_dev.restype = C.c_int
    lib.sperrhip_series_inverse_dev.argtypes = [_vp, _sz, C.c_uint, _sz, _sz, _sz, C.c_int, C.POINTER(_vp), _vp]
    lib.sperrhip_compress_series_dev.restype = C.c_int
    lib.sperrhip_compress_series_dev.argtypes = [C.POINTER(_vp), C.c_int] + [_sz] * 7 + \
        [C.c_uint, C.c_int, C.c_double, C.c_double, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_ubyte), _vp]
    lib.sperrhip_decompress_series_dev.restype = C.c_int
    lib.sperrhip_decompress_series_dev.argtypes = [C.c_char_p, _vp, C.POINTER(_sz), _sz, _sz, C.POINTER(_sz),
                                                   C.POINTER(_sz), C.c_uint, C.c_int, C.POINTER(_vp), _vp]
    lib.sperrhip_speck3d_encode_dev.restype = C.c_int
    lib.sperrhip_speck3d_encode_dev.argtypes = [_vp, C.c_int, _vp, _sz, _sz, _sz, _sz, _vp, _sz,
                                                C.POINTER(_sz), _vp]
    lib.sperrhip_speck3d_decode_dev.restype = C.c_int
    lib.sperrhip_speck3d_decode_dev.argtypes = [_vp, _sz, _sz, _sz, _sz, _vp, _vp,
                                                C.POINTER(C.c_int), _vp]
    lib.sperrhip_outlier_encode_dev.restype = C.c_int
    lib.sperrhip_outlier_encode_dev.argtypes = [_vp, C.c_int, _vp, _sz, _sz, _sz, _sz, C.c_double, _vp, _sz,
                                                C.POINTER(_sz), _vp]
    lib.sperrhip_profile_enable.argtypes = [C.c_int]
    lib.sperrhip_profile_only.argtypes = [C.c_char_p]
    lib.sperrhip_profile_get2.restype = C.c_int
    lib.sperrhip_profile_get2.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
    lib.sperrhip_profile_get.restype = C.c_int
    lib.sperrhip_profile_get.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int), C.c_int]
    lib.sperrhip_version.restype = C.c_char_p
    lib.sperrhip_comp_3d_farm.restype = C.c_int
    lib.sperrhip_comp_3d_farm.argtypes = [_vp, C.c_int, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int, C.c_double,
                                          _sz, _vp, _sz, C.POINTER(_vp), C.POINTER(_sz)]
    lib.sperrhip_decomp_3d_farm.restype = C.c_int
    lib.sperrhip_decomp_3d_farm.argtypes = [_vp, _sz, C.c_int, _sz, _vp, _sz, C.POINTER(_sz),
                                            C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_vp)]
    lib.sperrhip_decomp_3d_into.restype = C.c_int
    lib.sperrhip_decomp_3d_into.argtypes = [_vp, _sz, C.c_int, _sz, _vp, _sz, _vp, _sz, C.POINTER(_sz),
                                            C.POINTER(_sz), C.POINTER(_sz)]
    return lib


class SperrHip:
    """Device-resident SPERR 3D compressor / decompressor (fixed-rate mode)."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise SperrHipError("no GPU visible: libsperr_hip has no CPU fallback")
        self._libc = C.CDLL(None)
        self._libc.free.argtypes = [_vp]

    def _stream(self):
        return _vp(self.torch.cuda.current_stream().cuda_stream)

    # ---- strided views ---------------------------------------------------------------------
    @staticmethod
    def view_of(t):
        """The sperrhip_view of a 3-D cuda tensor (z, y, x) that is a strided view of a larger one -- the interior
        of an array with ghost cells, one member of a stacked buffer: unit x stride, rows stride(1) and slices
        stride(0) elements apart, the slice pitch a multiple of the row pitch.  data_ptr() is its first element.
        Raises SperrHipError for anything else (an x stride other than 1, a negative or overlapping stride, a slice
        pitch that is no multiple of the row pitch): nothing is ever copied silently."""
        if t.dim() != 3:
            raise SperrHipError(f"a view is a 3-D tensor (z, y, x), not {t.dim()}-D")
        dz, dy, dx = (int(d) for d in t.shape)
        sz, sy, sx = (int(v) for v in t.stride())
        if min(dz, dy, dx) < 1:
            raise SperrHipError("a view has no empty dimension")
        if dx > 1 and sx != 1:
            raise SperrHipError(f"a view has unit x stride, this tensor has {sx}")
        # (the stride of a dimension of size 1 says nothing: take the tightest pitch that fits)
        if dy == 1:
            sy = sz if dz > 1 and sz >= dx else dx
        if dz == 1:
            sz = sy * dy
        if sy < dx or sz < sy * dy or sz % sy != 0:
            raise SperrHipError(f"strides {tuple(t.stride())} of shape {tuple(t.shape)} are no view: the row pitch must "
                                "be at least x, the slice pitch at least y rows and a multiple of the row pitch")
        return View(sy, sz)

    @staticmethod
    def _no_view(t, what):
        if not t.is_contiguous():
            raise SperrHipError(f"{what} takes contiguous tensors only, no strided views")

    @staticmethod
    def _room_bytes(t):
        """bytes from the tensor's first element to the end of its storage"""
        return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()

    def _decompress_view(self, container, pct, output_float, lo, dims, out):
        rtn = self.lib.sperrhip_decompress_view_dev(container.data_ptr(), container.numel(), int(pct),
                                                    int(output_float), lo, dims, out.data_ptr(),
                                                    C.byref(self.view_of(out)), self._room_bytes(out), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_view_dev returned {rtn}")
        return out

    # ---- device-resident API -------------------------------------------------------------
    def max_compressed_size(self, shape_zyx, chunks_xyz, quality, mode=1):
        dz, dy, dx = shape_zyx
        return self.lib.sperrhip_max_compressed_size(dx, dy, dz, *chunks_xyz, mode, quality)

    def compress(self, vol, chunks_xyz, bpp, out=None, mode=1):
        """vol: cuda tensor float32/float64 shaped (z, y, x), contiguous or a strided view (view_of) of a larger
        tensor, which is read where it lies.  Returns a cuda uint8 tensor view of
        the container (a slice of `out` when given).  mode 1: `bpp` is the bit rate; mode 2: it is
        the target PSNR in dB; mode 3: the point-wise error tolerance (the reference's modes,
        include/SPERR_C_API.h:95-99)."""
        torch = self.torch
        assert vol.is_cuda and vol.dim() == 3
        assert vol.dtype in (torch.float32, torch.float64)
        view = None if vol.is_contiguous() else self.view_of(vol)
        dz, dy, dx = vol.shape
        cap = self.max_compressed_size(vol.shape, chunks_xyz, bpp, mode)
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=vol.device)
        n = _sz(0)
        if view is not None:
            rtn = self.lib.sperrhip_compress_view_dev(vol.data_ptr(), C.byref(view), int(vol.dtype == torch.float32),
                                                      dx, dy, dz, *chunks_xyz, mode, float(bpp), out.data_ptr(),
                                                      out.numel(), C.byref(n), self._stream())
            if rtn != 0:
                raise SperrHipError(f"sperrhip_compress_view_dev returned {rtn}")
            return out[:n.value]
        rtn = self.lib.sperrhip_compress_dev(vol.data_ptr(), int(vol.dtype == torch.float32), dx,
                                             dy, dz, *chunks_xyz, mode, float(bpp), out.data_ptr(),
                                             out.numel(), C.byref(n), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_dev returned {rtn}")
        return out[:n.value]

    # ---- compression to a PSNR of the whole volume (psnr_vol.h) -----------------------------
    def _psnr_args(self, vol, what):
        torch = self.torch
        if not (vol.is_cuda and vol.dim() == 3 and vol.dtype in (torch.float32, torch.float64)):
            raise SperrHipError(f"{what} takes a 3-D cuda tensor of float32 or float64")
        return None if vol.is_contiguous() else C.byref(self.view_of(vol))

    def psnr_ladder(self, range, psnr):
        """(t, q): the target mean squared error of a range and a PSNR in dB, and the five quantisation steps a chunk
        can end on (a numpy float64 array) -- sperrhip_psnr_ladder, host only"""
        t, q = C.c_double(0.0), np.zeros(5, dtype=np.float64)
        if self.lib.sperrhip_psnr_ladder(float(range), float(psnr), C.byref(t), q.ctypes.data) != 0:
            raise SperrHipError(f"a range of {range} at {psnr} dB gives no quantisation step")
        return t.value, q

    def value_range(self, vol):
        """(min, max) of a cuda tensor (z, y, x) of float32 or float64, contiguous or a strided view (view_of), as
        Python floats: one streaming read on the device.  Raises SperrHipError when a sample is a NaN."""
        view = self._psnr_args(vol, "value_range")
        dz, dy, dx = vol.shape
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        rtn = self.lib.sperrhip_range_dev(vol.data_ptr(), view, int(vol.dtype == self.torch.float32), dx, dy, dz,
                                          C.byref(lo), C.byref(hi), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_range_dev returned {rtn}")
        return lo.value, hi.value

    def compress_to_psnr(self, vol, chunks_xyz, psnr, range=None, out=None):
        """A container coded to `psnr` dB of the WHOLE volume's range (mode 2 codes every chunk to `psnr` dB of its
        own): every chunk takes the same target error t = range^2 10^(-psnr/10) and the reference's own search for
        its quantisation step.  range None: the volume's own, max - min; a positive number is taken as it is (a time
        series' common range).  vol as compress() takes it, contiguous or a view.  An ordinary container: decompress,
        decompress_box and the rest open it.  Raises SperrHipError for a volume with a NaN or an infinity and for a
        target so fine that a coefficient would be 2^63 steps or more."""
        torch = self.torch
        view = self._psnr_args(vol, "compress_to_psnr")
        dz, dy, dx = vol.shape
        rng = 0.0 if range is None else float(range)
        if range is not None and not rng > 0.0:
            raise SperrHipError("a range is a positive number (None: the volume's own)")
        cap = self.max_compressed_size(vol.shape, chunks_xyz, float(psnr), 2)
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=vol.device)
        n = _sz(0)
        rtn = self.lib.sperrhip_compress_psnr_dev(vol.data_ptr(), view, int(vol.dtype == torch.float32), dx, dy, dz,
                                                  *chunks_xyz, float(psnr), rng, out.data_ptr(), out.numel(),
                                                  C.byref(n), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_psnr_dev returned {rtn}")
        return out[:n.value]

    # ---- compression to a byte target (the size mode) ---------------------------------------
    def _chunk_count(self, shape_zyx, chunks_xyz):
        dz, dy, dx = (int(d) for d in shape_zyx)
        return int(self.lib.sperrhip_chunk_count(dx, dy, dz, *(int(c) for c in chunks_xyz)))

    def _size_args(self, vol, what):
        torch = self.torch
        if not (vol.is_cuda and vol.dim() == 3 and vol.dtype in (torch.float32, torch.float64)):
            raise SperrHipError(f"{what} takes a 3-D cuda tensor of float32 or float64")
        self._no_view(vol, what)

    def size_survey(self, vol, chunks_xyz):
        """What any absolute threshold would cost, without compressing.  vol as compress() takes it (contiguous).
        Returns a dict of numpy arrays, one entry per chunk in container order: "q" the fixed-rate quantisation
        step, "nbp" the number of bit planes, "end" (nchunks, 32) uint64 -- end[c, p] the payload bits of chunk c's
        stream at the end of plane p under an unlimited budget, zeros from nbp[c] on --, "is_const" bool.  Coding
        chunk c down to plane p leaves an error of the order of q[c] * 2**p and takes 26 + end[c, p] / 8 bytes."""
        self._size_args(vol, "size_survey")
        dz, dy, dx = vol.shape
        n = self._chunk_count(vol.shape, chunks_xyz)
        q, nbp = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32)
        end, ic = np.zeros((n, 32), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        rtn = self.lib.sperrhip_size_survey_dev(vol.data_ptr(), int(vol.dtype == self.torch.float32), dx, dy, dz,
                                                *chunks_xyz, n, q.ctypes.data, nbp.ctypes.data, end.ctypes.data,
                                                ic.ctypes.data, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_size_survey_dev returned {rtn}")
        return {"q": q, "nbp": nbp, "end": end, "is_const": ic.astype(bool)}

    def compress_to_size(self, vol, chunks_xyz, nbytes, out=None, return_plan=False):
        """A container of at most `nbytes` bytes: an ordinary fixed-rate container whose chunks each got a budget of
        their own, dealt so that all of them stop at (nearly) the same absolute threshold (budget.h).  vol as
        compress() takes it (contiguous); `out`, when given and at least nbytes long, receives the container and is
        not written when the call is refused (SperrHipError: the target does not hold the headers and a payload
        byte per chunk).  Returns the container (a cuda uint8 view), with return_plan the pair (container, budgets):
        every chunk's budget in bits as a numpy uint64 array, 0 for a constant chunk."""
        self._size_args(vol, "compress_to_size")
        torch = self.torch
        dz, dy, dx = vol.shape
        nbytes = int(nbytes)
        if nbytes < 0:
            raise SperrHipError("a byte target is not negative")
        n = self._chunk_count(vol.shape, chunks_xyz)
        if out is None or out.numel() < nbytes:
            out = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=vol.device)
        budgets = np.zeros(n, dtype=np.uint64)
        ln = _sz(0)
        rtn = self.lib.sperrhip_compress_size_dev(vol.data_ptr(), int(vol.dtype == torch.float32), dx, dy, dz,
                                                  *chunks_xyz, nbytes, out.data_ptr(), out.numel(), C.byref(ln),
                                                  budgets.ctypes.data, n, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_size_dev returned {rtn}")
        return (out[:ln.value], budgets) if return_plan else out[:ln.value]

    def parse_header(self, container):
        """((z, y, x), is_float, chunks (x, y, z)) of a device container's header, read on the current stream: behind
        whatever is still writing the container there"""
        d = [_sz(0) for _ in range(6)]
        isf = C.c_int(0)
        rtn = self.lib.sperrhip_parse_header_stream_dev(container.data_ptr(), container.numel(),
                                                        C.byref(d[0]), C.byref(d[1]), C.byref(d[2]),
                                                        C.byref(isf), C.byref(d[3]), C.byref(d[4]),
                                                        C.byref(d[5]), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_parse_header_stream_dev returned {rtn}")
        return (d[2].value, d[1].value, d[0].value), bool(isf.value), \
               (d[3].value, d[4].value, d[5].value)

    def _portion_dev(self, container, pct, output_float, level, lo, dims, out):
        """sperrhip_decompress_portion_dev into `out`: the decode `level` / `lo` / `dims` name, of the first `pct`
        percent of every chunk stream"""
        rtn = self.lib.sperrhip_decompress_portion_dev(container.data_ptr(), container.numel(), int(pct),
                                                       int(output_float), None if level is None else C.byref(_sz(level)),
                                                       lo, dims, out.data_ptr(), out.numel() * out.element_size(),
                                                       self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_portion_dev returned {rtn}")
        return out

    def decompress(self, container, output_float=True, out=None, shape_zyx=None, pct=0):
        """The volume of a device container, a cuda tensor shaped (z, y, x) -- `out` when given, which may be a
        strided view (view_of) of a larger tensor: the volume is written into it and nothing around it.  pct (here and in
        decompress_box / decompress_level): decode the first pct percent of every chunk stream only, bit for bit the
        decode of truncate(container, pct) without making it; 0: everything."""
        torch = self.torch
        assert container.is_cuda and container.dtype == torch.uint8 and container.is_contiguous()
        if shape_zyx is None:
            shape_zyx, _, _ = self.parse_header(container)
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty(shape_zyx, dtype=dt, device=container.device)
        if not out.is_contiguous():
            assert out.dtype == dt and out.is_cuda
            if tuple(out.shape) != tuple(shape_zyx):
                raise SperrHipError(f"the view is {tuple(out.shape)}, the volume {tuple(shape_zyx)}")
            return self._decompress_view(container, pct, output_float, None, None, out)
        assert out.dtype == dt and out.is_contiguous()
        if pct:
            return self._portion_dev(container, pct, output_float, None, None, None, out)
        dx, dy, dz = _sz(0), _sz(0), _sz(0)
        rtn = self.lib.sperrhip_decompress_dev(container.data_ptr(), container.numel(),
                                               int(output_float), out.data_ptr(),
                                               out.numel() * out.element_size(), C.byref(dx),
                                               C.byref(dy), C.byref(dz), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_dev returned {rtn}")
        return out

    def decompress_box(self, container, box_lo_xyz, box_dims_xyz, output_float=True, out=None, pct=0):
        """The box [lo, lo + dims) (x, y, z order) of a device container's volume, decoded from the chunks it
        meets only; a cuda tensor shaped (dims z, dims y, dims x) -- `out` when given, which may be a strided view
        (view_of) of a larger tensor."""
        torch = self.torch
        assert container.is_cuda and container.dtype == torch.uint8 and container.is_contiguous()
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty(tuple(int(d) for d in reversed(box_dims_xyz)), dtype=dt, device=container.device)
        if not out.is_contiguous():
            assert out.dtype == dt and out.is_cuda
            if tuple(out.shape) != tuple(int(d) for d in reversed(box_dims_xyz)):
                raise SperrHipError(f"the view is {tuple(out.shape)}, the box (x, y, z) {tuple(box_dims_xyz)}")
            return self._decompress_view(container, pct, output_float, (_sz * 3)(*box_lo_xyz),
                                         (_sz * 3)(*box_dims_xyz), out)
        assert out.dtype == dt and out.is_contiguous() and out.is_cuda
        if pct:
            return self._portion_dev(container, pct, output_float, None, (_sz * 3)(*box_lo_xyz),
                                     (_sz * 3)(*box_dims_xyz), out)
        rtn = self.lib.sperrhip_decompress_box_dev(container.data_ptr(), container.numel(), int(output_float),
                                                   (_sz * 3)(*box_lo_xyz), (_sz * 3)(*box_dims_xyz), out.data_ptr(),
                                                   out.numel() * out.element_size(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_box_dev returned {rtn}")
        return out

    @staticmethod
    def _box_args(box_lo_xyz, box_dims_xyz):
        if (box_lo_xyz is None) != (box_dims_xyz is None):
            raise ValueError("give both box_lo_xyz and box_dims_xyz, or neither")
        if box_lo_xyz is None:
            return None, None
        return (_sz * 3)(*box_lo_xyz), (_sz * 3)(*box_dims_xyz)

    def decompress_level(self, container, level, box_lo_xyz=None, box_dims_xyz=None, output_float=False, out=None,
                         pct=0):
        """Level `level` of a device container's hierarchy (coarsest first, as multires_levels orders them), whole or
        the box [lo, lo + dims) of it (x, y, z order, the level's coordinates): only the chunks it meets are read and
        only the level's part of the inverse transform runs.  A cuda tensor shaped (z, y, x) -- `out` when given."""
        torch = self.torch
        assert container.is_cuda and container.dtype == torch.uint8 and container.is_contiguous()
        if out is not None:
            self._no_view(out, "decompress_level")
        dt = torch.float32 if output_float else torch.float64
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        if out is None:
            if dims is None:
                shape, _, chunks = self.parse_header(container)
                lv = self.multires_levels(shape, chunks)
                if not 0 <= level < len(lv):
                    raise SperrHipError(f"the container has {len(lv)} levels, level {level} was asked for")
                zyx = lv[level]
            else:
                zyx = tuple(int(d) for d in reversed(box_dims_xyz))
            out = torch.empty(zyx, dtype=dt, device=container.device)
        assert out.dtype == dt and out.is_contiguous() and out.is_cuda
        if pct:
            return self._portion_dev(container, pct, output_float, level, lo, dims, out)
        rtn = self.lib.sperrhip_decompress_level_dev(container.data_ptr(), container.numel(), int(output_float),
                                                     level, lo, dims, out.data_ptr(),
                                                     out.numel() * out.element_size(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_level_dev returned {rtn}")
        return out

    def truncate(self, container, pct, out=None):
        """sperr_trunc_3d of a device container on the device: a cuda uint8 view (of `out` when it is large enough) of
        the container that keeps the first pct percent of every chunk stream."""
        torch = self.torch
        assert container.is_cuda and container.dtype == torch.uint8 and container.is_contiguous()
        if out is None or out.numel() < container.numel():
            out = torch.empty(container.numel(), dtype=torch.uint8, device=container.device)
        n = _sz(0)
        rtn = self.lib.sperrhip_trunc_dev(container.data_ptr(), container.numel(), int(pct), out.data_ptr(),
                                          out.numel(), C.byref(n), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_trunc_dev returned {rtn}")
        return out[:n.value]

    def truncate_batch(self, containers, pct, out=None):
        """truncate() of every container of a list in one call and one kernel launch: cuda uint8 views into one
        buffer (`out` when it is large enough), in order.  The containers are concatenated first unless they already
        lie back to back in one buffer."""
        torch = self.torch
        assert len(containers) > 0
        for c in containers:
            assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 1 and c.is_contiguous()
        nvol = len(containers)
        packed = all(b.data_ptr() == a.data_ptr() + a.numel() and
                     b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
                     for a, b in zip(containers, containers[1:]))
        src = containers[0] if packed else torch.cat(list(containers))
        offs, outs = (_sz * (nvol + 1))(), (_sz * (nvol + 1))()
        for v, c in enumerate(containers):
            offs[v + 1] = offs[v] + c.numel()
        if out is None or out.numel() < offs[nvol]:
            out = torch.empty(offs[nvol], dtype=torch.uint8, device=src.device)
        rtn = self.lib.sperrhip_trunc_batch_dev(src.data_ptr(), offs, nvol, int(pct), out.data_ptr(), out.numel(),
                                                outs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_trunc_batch_dev returned {rtn}")
        return [out[outs[v]:outs[v + 1]] for v in range(nvol)]

    def max_compressed_size_batch(self, nvol, shape_zyx, chunks_xyz, quality, mode=1):
        dz, dy, dx = shape_zyx
        return self.lib.sperrhip_max_compressed_size_batch(nvol, dx, dy, dz, *chunks_xyz, mode, quality)

    def compress_batch(self, vols, chunks_xyz, quality, mode=1, out=None):
        """vols: contiguous cuda tensor float32/float64 shaped (N, z, y, x).  Returns N cuda uint8 tensors, views into
        one buffer (`out` when it is large enough) in order: container v is what compress() makes of vols[v]."""
        torch = self.torch
        self._no_view(vols, "compress_batch")
        assert vols.is_cuda and vols.is_contiguous() and vols.dim() == 4
        assert vols.dtype in (torch.float32, torch.float64)
        nvol, dz, dy, dx = vols.shape
        cap = self.max_compressed_size_batch(nvol, vols.shape[1:], chunks_xyz, quality, mode)
        if cap == 0:
            raise SperrHipError("sperrhip_max_compressed_size_batch overflows")
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=vols.device)
        offs = (_sz * (nvol + 1))()
        rtn = self.lib.sperrhip_compress_batch_dev(vols.data_ptr(), int(vols.dtype == torch.float32), nvol, dx, dy,
                                                   dz, *chunks_xyz, mode, float(quality), out.data_ptr(),
                                                   out.numel(), offs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_batch_dev returned {rtn}")
        return [out[offs[v]:offs[v + 1]] for v in range(nvol)]

    def decompress_batch(self, containers, output_float=True, out=None):
        """containers: a list of cuda uint8 tensors (compress_batch's views, or any), each a container of a volume of
        the same dims.  They are concatenated first unless they already lie back to back in one buffer.  Returns a
        cuda tensor shaped (N, z, y, x) -- `out` when given."""
        torch = self.torch
        assert len(containers) > 0
        for c in containers:
            assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 1 and c.is_contiguous()
        nvol = len(containers)
        packed = all(b.data_ptr() == a.data_ptr() + a.numel() and
                     b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
                     for a, b in zip(containers, containers[1:]))
        src = containers[0] if packed else torch.cat(list(containers))
        offs = (_sz * (nvol + 1))()
        for v, c in enumerate(containers):
            offs[v + 1] = offs[v] + c.numel()
        shape_zyx, _, _ = self.parse_header(src[:offs[1]])
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty((nvol,) + tuple(shape_zyx), dtype=dt, device=src.device)
        assert out.dtype == dt and out.is_contiguous() and out.is_cuda
        dx, dy, dz = _sz(0), _sz(0), _sz(0)
        rtn = self.lib.sperrhip_decompress_batch_dev(src.data_ptr(), offs, nvol, int(output_float), out.data_ptr(),
                                                     out.numel() * out.element_size(), C.byref(dx), C.byref(dy),
                                                     C.byref(dz), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_batch_dev returned {rtn}")
        return out

    # ---- a box per entry out of a batch of containers --------------------------------------------
    @staticmethod
    def _boxes_args(ncont, box_lo_xyz, box_dims_xyz, which, level):
        """(which, lo, nbox, dims, level) as the boxes calls take them.  box_lo_xyz: one origin for all entries, or
        one per entry; the entries are `which`'s, or one per container"""
        nbox = len(which) if which is not None else ncont
        los = [box_lo_xyz] * nbox if np.ndim(box_lo_xyz) == 1 else list(box_lo_xyz)
        if len(los) != nbox:
            raise SperrHipError(f"{len(los)} box origins for {nbox} entries")
        lo = (_sz * (3 * max(nbox, 1)))(*[int(v) for o in los for v in o])
        wh = None if which is None else (C.c_uint32 * max(nbox, 1))(*[int(v) for v in which])
        return wh, lo, nbox, (_sz * 3)(*[int(d) for d in box_dims_xyz]), None if level is None else C.byref(_sz(level))

    def boxes_plan(self, shape_zyx, chunks_xyz, box_lo_xyz, box_dims_xyz, which=None, level=None):
        """What decompress_boxes would do with containers of volume `shape_zyx`; host only.  chunks_xyz: the chunk
        shape of every container, one (x, y, z) each.  A dict of slots (chunks decoded), pairs (pieces written),
        staged, staging_values and output_values; raises SperrHipError for what the call would refuse."""
        cds = [tuple(c) for c in chunks_xyz]
        n = len(cds)
        wh, lo, nbox, dims, lv = self._boxes_args(n, box_lo_xyz, box_dims_xyz, which, level)
        dz, dy, dx = (int(d) for d in shape_zyx)
        out = (_sz * 5)()
        rtn = self.lib.sperrhip_boxes_plan(n, (_sz * 3)(dx, dy, dz), (_sz * (3 * n))(*[int(v) for c in cds for v in c]),
                                           wh, lo, nbox, dims, lv, out)
        if rtn != 0:
            raise SperrHipError(f"sperrhip_boxes_plan returned {rtn}")
        return {"slots": out[0], "pairs": out[1], "staged": bool(out[2]), "staging_values": out[3],
                "output_values": out[4]}

    def decompress_boxes(self, containers, box_lo_xyz, box_dims_xyz, which=None, level=None, pct=0, output_float=True,
                         out=None):
        """A box per entry out of a list of device containers, in one call: entry e is the box [lo_e, lo_e + dims)
        (x, y, z order) of containers[which[e]] (which None: of containers[e]), or with `level` of that level of its
        hierarchy, in the level's coordinates; box_lo_xyz is one origin for all entries or one per entry.  The
        containers are cuda uint8 tensors wherever they lie -- they are never concatenated -- of volumes of the same
        dims.  Only the chunks some box meets are read, and one that several entries meet is decoded once.  A cuda
        tensor shaped (entries, dims z, dims y, dims x) -- `out` when given; entry e is bit for bit decompress_box /
        decompress_level of its container with the same box and pct."""
        torch = self.torch
        for c in containers:
            assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 1 and c.is_contiguous()
        ncont = len(containers)
        wh, lo, nbox, dims, lv = self._boxes_args(ncont, box_lo_xyz, box_dims_xyz, which, level)
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            if ncont == 0 or nbox == 0:
                raise SperrHipError("decompress_boxes: no containers or no entries")
            out = torch.empty((nbox,) + tuple(int(d) for d in reversed(box_dims_xyz)), dtype=dt,
                              device=containers[0].device)
        self._no_view(out, "decompress_boxes")
        assert out.dtype == dt and out.is_cuda
        ptrs = (_vp * max(ncont, 1))(*[c.data_ptr() for c in containers])
        lens = (_sz * max(ncont, 1))(*[c.numel() for c in containers])
        rtn = self.lib.sperrhip_decompress_boxes_dev(ptrs, lens, ncont, wh, lo, nbox, dims, lv, int(pct),
                                                     int(output_float), out.data_ptr(),
                                                     out.numel() * out.element_size(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_boxes_dev returned {rtn}")
        return out

    # ---- time series: a Haar transform across the steps ------------------------------------------
    def series_plan(self, nsteps, levels=3):
        """The groups of a series, host only: a list of (first step, levels of the group)."""
        ng = _sz(0)
        if self.lib.sperrhip_series_plan(int(nsteps), int(levels), C.byref(ng), None, None, 0) != 0:
            raise SperrHipError("sperrhip_series_plan refuses these arguments")
        starts, lv = (_sz * ng.value)(), (C.c_uint * ng.value)()
        rtn = self.lib.sperrhip_series_plan(int(nsteps), int(levels), C.byref(ng), starts, lv, ng.value)
        if rtn != 0:
            raise SperrHipError(f"sperrhip_series_plan returned {rtn}")
        return [(int(starts[i]), int(lv[i])) for i in range(ng.value)]

    def series_needs(self, nsteps, levels, t0=0, nt=None):
        """The bands (= containers) a decode of the steps [t0, t0 + nt) needs, host only: a sorted list."""
        nt = int(nsteps) - int(t0) if nt is None else int(nt)
        if nsteps <= 0 or t0 < 0 or nt < 0:
            raise SperrHipError("sperrhip_series_needs refuses these arguments")
        need = (C.c_ubyte * int(nsteps))()
        if self.lib.sperrhip_series_needs(int(nsteps), int(levels), int(t0), nt, need, None) != 0:
            raise SperrHipError("sperrhip_series_needs refuses these arguments")
        return [b for b in range(int(nsteps)) if need[b]]

    def series_tolerance(self, tol, maxabs, levels=3):
        """(rho, [tau_0 .. tau_levels]) of a tolerance and the series' largest |sample|, host only."""
        rho, tau = C.c_double(0.0), (C.c_double * 5)()
        if self.lib.sperrhip_series_tolerance(float(tol), float(maxabs), int(levels), C.byref(rho), tau) != 0:
            raise SperrHipError(f"sperrhip_series_tolerance refuses tol {tol} at a largest sample of {maxabs}")
        return rho.value, [tau[l] for l in range(int(levels) + 1)]

    def series_parse(self, info):
        """The fields of an info record (64 bytes), host only."""
        rec = bytes(info)
        n, lv, dims, isf, kind = _sz(0), C.c_uint(0), (_sz * 3)(), C.c_int(0), C.c_int(0)
        q, rng, M, rho = C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
        if len(rec) != 64 or self.lib.sperrhip_series_parse(rec, C.byref(n), C.byref(lv), dims, C.byref(isf),
                                                            C.byref(kind), C.byref(q), C.byref(rng), C.byref(M),
                                                            C.byref(rho)) != 0:
            raise SperrHipError("not a series info record")
        return {"nsteps": n.value, "levels": lv.value, "shape_zyx": (dims[2], dims[1], dims[0]),
                "is_float": bool(isf.value), "kind": "tol" if kind.value == 0 else "psnr", "quality": q.value,
                "range": rng.value, "maxabs": M.value, "rho": rho.value}

    def _series_steps(self, vols, what):
        """the steps of a series as a list of dense cuda tensors of one shape and dtype"""
        torch = self.torch
        steps = list(vols) if isinstance(vols, (list, tuple)) else [vols[t] for t in range(vols.shape[0])]
        if not steps:
            raise SperrHipError(f"{what}: a series has at least one step")
        for s in steps:
            assert s.is_cuda and s.dtype in (torch.float32, torch.float64)
            if s.dtype != steps[0].dtype or s.shape != steps[0].shape:
                raise SperrHipError(f"{what}: the steps of a series share shape and dtype")
            self._no_view(s, what)
        return steps

    def series_forward(self, vols, levels=3, out=None):
        """Stage access, k_series_fwd alone: the N steps (a list of dense cuda tensors of one shape, anywhere in
        memory, or a tensor whose steps are dense) into the N fp64 bands, a cuda tensor shaped (N,) + step shape."""
        torch = self.torch
        steps = self._series_steps(vols, "series_forward")
        n = steps[0].numel()
        if out is None:
            out = torch.empty((len(steps),) + tuple(steps[0].shape), dtype=torch.float64, device=steps[0].device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == len(steps) * n
        ptrs = (_vp * len(steps))(*[s.data_ptr() for s in steps])
        rtn = self.lib.sperrhip_series_forward_dev(ptrs, int(steps[0].dtype == torch.float32), len(steps), int(levels),
                                                   n, out.data_ptr(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_series_forward_dev returned {rtn}")
        return out

    def series_inverse(self, bands, levels=3, t0=0, nt=None, output_float=True, out=None):
        """Stage access, k_series_inv alone: the steps [t0, t0 + nt) of the fp64 bands (N, ...), of which only the
        needed ones are read.  out: a list of nt dense cuda tensors, or a tensor shaped (nt, ...); made when None."""
        torch = self.torch
        assert bands.is_cuda and bands.dtype == torch.float64 and bands.is_contiguous() and bands.dim() >= 2
        nsteps = bands.shape[0]
        nt = nsteps - t0 if nt is None else nt
        n = bands[0].numel()
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty((max(nt, 0),) + tuple(bands.shape[1:]), dtype=dt, device=bands.device)
        outs = list(out) if isinstance(out, (list, tuple)) else [out[t] for t in range(out.shape[0])]
        if len(outs) != nt or nt <= 0 or t0 < 0:
            raise SperrHipError(f"series_inverse: {len(outs)} outputs for the steps [{t0}, {t0 + nt})")
        for o in outs:
            assert o.is_cuda and o.dtype == dt and o.numel() == n
            self._no_view(o, "series_inverse")
        ptrs = (_vp * nt)(*[o.data_ptr() for o in outs])
        rtn = self.lib.sperrhip_series_inverse_dev(bands.data_ptr(), nsteps, int(levels), n, int(t0), int(nt),
                                                   int(output_float), ptrs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_series_inverse_dev returned {rtn}")
        return out

    def compress_series(self, vols, chunks_xyz, tol=None, psnr=None, levels=3, range=None, out=None):
        """N time steps of one field -- a list of dense cuda tensors (z, y, x) of one shape and dtype, anywhere in
        memory, or a (t, z, y, x) tensor whose steps are dense -- into N containers, one per band of a Haar transform
        across the steps, and the 64-byte info record.  Exactly one of `tol` (every sample of every step within tol)
        and `psnr` (dB of `range`, default the series' own) is given.  Returns (containers, info): N cuda uint8
        views into one buffer, and bytes."""
        torch = self.torch
        steps = self._series_steps(vols, "compress_series")
        if (tol is None) == (psnr is None):
            raise SperrHipError("compress_series takes exactly one of tol and psnr")
        if steps[0].dim() != 3:
            raise SperrHipError("compress_series takes steps shaped (z, y, x)")
        kind, quality = (0, float(tol)) if psnr is None else (1, float(psnr))
        nsteps = len(steps)
        dz, dy, dx = steps[0].shape
        cap = self.max_compressed_size_batch(nsteps, steps[0].shape, chunks_xyz, quality, 3 if kind == 0 else 2)
        if cap == 0:
            raise SperrHipError("sperrhip_max_compressed_size_batch overflows")
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=steps[0].device)
        offs = (_sz * (nsteps + 1))()
        info = (C.c_ubyte * 64)()
        ptrs = (_vp * nsteps)(*[s.data_ptr() for s in steps])
        rtn = self.lib.sperrhip_compress_series_dev(ptrs, int(steps[0].dtype == torch.float32), nsteps, dx, dy, dz,
                                                    *chunks_xyz, int(levels), kind, quality,
                                                    0.0 if range is None else float(range), out.data_ptr(),
                                                    out.numel(), offs, info, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_series_dev returned {rtn}")
        return [out[offs[b]:offs[b + 1]] for b in builtins_range(nsteps)], bytes(info)

    def decompress_series(self, containers, info, t0=0, nt=None, box_lo_xyz=None, box_dims_xyz=None, pct=0,
                          output_float=True, out=None):
        """The steps [t0, t0 + nt) of a series (nt None: to its end), whole or a box of every step, from the first pct
        percent of every chunk stream.  containers: compress_series' list; only those the range needs (series_needs)
        are decoded, and unless the list lies back to back in one buffer only those are concatenated first.  out: a list of nt dense cuda tensors or a
        tensor shaped (nt, z, y, x) of the volume's or the box's shape; made when None.  It is untouched when the
        call fails."""
        torch = self.torch
        rec = bytes(info)
        if len(rec) != 64:
            raise SperrHipError("not a series info record")
        h = self.series_parse(rec)
        nsteps = h["nsteps"]
        if len(containers) != nsteps:
            raise SperrHipError(f"{len(containers)} containers for a series of {nsteps} steps")
        for c in containers:
            assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 1 and c.is_contiguous()
        nt = nsteps - t0 if nt is None else nt
        packed = all(b.data_ptr() == a.data_ptr() + a.numel() and
                     b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
                     for a, b in zip(containers, containers[1:]))
        # (containers that do not lie back to back are concatenated, but only those the range needs: the others get
        #  an empty byte range, which the call never looks at)
        need = range(nsteps) if packed else self.series_needs(nsteps, h["levels"], t0, nt)
        src = containers[0] if packed else torch.cat([containers[b] for b in need])
        offs = (_sz * (nsteps + 1))()
        for v, c in enumerate(containers):
            offs[v + 1] = offs[v] + (c.numel() if v in need else 0)
        if (box_lo_xyz is None) != (box_dims_xyz is None):
            raise SperrHipError("decompress_series takes a box's origin and dims together")
        lo, dims = (None, None) if box_lo_xyz is None else self._box_args(box_lo_xyz, box_dims_xyz)
        shape = h["shape_zyx"] if box_dims_xyz is None else tuple(int(d) for d in reversed(box_dims_xyz))
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty((max(nt, 0),) + tuple(shape), dtype=dt, device=src.device)
        outs = list(out) if isinstance(out, (list, tuple)) else [out[t] for t in builtins_range(out.shape[0])]
        if len(outs) != nt:
            raise SperrHipError(f"decompress_series: {len(outs)} outputs for {nt} steps")
        n = int(np.prod(shape))
        for o in outs:
            assert o.is_cuda and o.dtype == dt and o.numel() == n
            self._no_view(o, "decompress_series")
        ptrs = (_vp * max(nt, 1))(*[o.data_ptr() for o in outs])
        rtn = self.lib.sperrhip_decompress_series_dev(rec, src.data_ptr(), offs, int(t0), int(nt), lo, dims, int(pct),
                                                      int(output_float), ptrs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_series_dev returned {rtn}")
        return out

    # ---- quality figures of a reconstruction ---------------------------------------------------
    def _quality_args(self, orig, recon):
        torch = self.torch
        assert orig.is_cuda and recon.is_cuda and orig.is_contiguous() and recon.is_contiguous()
        assert orig.dtype == recon.dtype and orig.dtype in (torch.float32, torch.float64)
        assert orig.numel() == recon.numel() and orig.numel() > 0

    def quality(self, orig, recon, nbytes=None):
        """The reference's figures (calc_stats, calc_mean_var) of `recon` against `orig`, computed where they are:
        contiguous cuda tensors of one dtype (float32 / float64) and numel, any shape -- or, when either is a strided
        view (view_of), two 3-D tensors of one shape (z, y, x), each contiguous or a view, with the figures of their
        packed copies.  A Quality record; `nbytes` (the compressed size) adds bitrate and accuracy_gain."""
        if not (orig.is_contiguous() and recon.is_contiguous()):
            return self._quality_view(orig, recon, nbytes)
        self._quality_args(orig, recon)
        out = (C.c_double * 8)()
        rtn = self.lib.sperrhip_quality_dev(orig.data_ptr(), recon.data_ptr(), int(orig.dtype == self.torch.float32),
                                            orig.numel(), out, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_quality_dev returned {rtn}")
        return Quality(out[:8], orig.numel(), nbytes)

    def _quality_view(self, orig, recon, nbytes):
        torch = self.torch
        assert orig.is_cuda and recon.is_cuda
        assert orig.dtype == recon.dtype and orig.dtype in (torch.float32, torch.float64)
        if orig.dim() != 3 or tuple(orig.shape) != tuple(recon.shape):
            raise SperrHipError(f"with a view, both tensors are (z, y, x) of one shape: {tuple(orig.shape)} and "
                                f"{tuple(recon.shape)}")
        vo = None if orig.is_contiguous() else C.byref(self.view_of(orig))
        vr = None if recon.is_contiguous() else C.byref(self.view_of(recon))
        dz, dy, dx = orig.shape
        out = (C.c_double * 8)()
        rtn = self.lib.sperrhip_quality_view_dev(orig.data_ptr(), vo, recon.data_ptr(), vr,
                                                 int(orig.dtype == torch.float32), dx, dy, dz, out, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_quality_view_dev returned {rtn}")
        return Quality(out[:8], orig.numel(), nbytes)

    def quality_batch(self, origs, recons):
        """quality() of every pair of a batch in one call: stacked tensors (N, ...), as compress_batch takes and
        decompress_batch returns them.  A list of N Quality records."""
        self._quality_args(origs, recons)
        assert origs.dim() >= 2 and origs.shape[0] == recons.shape[0]
        nvol = origs.shape[0]
        n = origs.numel() // nvol
        out = (C.c_double * (8 * nvol))()
        rtn = self.lib.sperrhip_quality_batch_dev(origs.data_ptr(), recons.data_ptr(),
                                                  int(origs.dtype == self.torch.float32), nvol, n, out, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_quality_batch_dev returned {rtn}")
        return [Quality(out[8 * v:8 * v + 8], n) for v in range(nvol)]

    # ---- interleaved fields ------------------------------------------------------------------
    @staticmethod
    def fields_of(t, field_dim=-1):
        """(Fields, nfields, (z, y, x)) of a 4-D cuda tensor whose dimension `field_dim` is the field axis: that axis
        has stride 1, the other three are read as (z, y, x) and their strides are the layout's pitch_z, pitch_y and
        stride_x, which must obey the rule of include/sperr_hip.h (a record at least nfields wide, rows and slices
        that do not overlap).  A contiguous (z, y, x, c) tensor, its slices t[..., a:b], its halo interiors, and with
        field_dim=0 the (c, z, y, x) view of a channels-last tensor all are.  data_ptr() is the first selected field.
        Raises SperrHipError for anything else: nothing is ever copied silently."""
        if t.dim() != 4:
            raise SperrHipError(f"interleaved fields are a 4-D tensor, not {t.dim()}-D")
        fd = field_dim % 4
        nf, sf = int(t.shape[fd]), int(t.stride(fd))
        (dz, dy, dx) = (int(t.shape[a]) for a in range(4) if a != fd)
        (sz, sy, sx) = (int(t.stride(a)) for a in range(4) if a != fd)
        if min(nf, dz, dy, dx) < 1:
            raise SperrHipError("interleaved fields have no empty dimension")
        if nf > 1 and sf != 1:
            raise SperrHipError(f"the field axis has stride 1, dimension {field_dim} of this tensor has {sf}")
        # (the stride of a dimension of size 1 says nothing: take the tightest that fits)
        if dx == 1:
            sx = nf
        if dy == 1:
            sy = sz if dz > 1 and sz >= dx * sx else dx * sx
        if dz == 1:
            sz = sy * dy
        if sx < nf or sy < dx * sx or sz < sy * dy:
            raise SperrHipError(f"strides {tuple(t.stride())} of shape {tuple(t.shape)} are no interleaved layout: the "
                                "record must be at least the fields wide, the row pitch at least x records and the "
                                "slice pitch at least y rows")
        return Fields(sx, sy, sz), nf, (dz, dy, dx)

    def _fields_args(self, t, field_dim):
        torch = self.torch
        assert t.is_cuda and t.dtype in (torch.float32, torch.float64)
        return self.fields_of(t, field_dim)

    def compress_fields(self, t, chunks_xyz, quality, mode=1, field_dim=-1, out=None):
        """The fields of an interleaved cuda tensor (fields_of), one container each: a list of cuda uint8 views into
        one buffer (`out` when it is large enough) in order; container f is what compress() makes of the packed copy
        of field f.  The tensor is read where it lies."""
        torch = self.torch
        lay, nf, (dz, dy, dx) = self._fields_args(t, field_dim)
        cap = self.max_compressed_size_batch(nf, (dz, dy, dx), chunks_xyz, quality, mode)
        if cap == 0:
            raise SperrHipError("sperrhip_max_compressed_size_batch overflows")
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=t.device)
        offs = (_sz * (nf + 1))()
        rtn = self.lib.sperrhip_compress_fields_dev(t.data_ptr(), C.byref(lay), nf, int(t.dtype == torch.float32), dx,
                                                    dy, dz, *chunks_xyz, mode, float(quality), out.data_ptr(),
                                                    out.numel(), offs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_fields_dev returned {rtn}")
        return [out[offs[f]:offs[f + 1]] for f in range(nf)]

    def decompress_fields(self, containers, out=None, field_dim=-1, output_float=True):
        """containers: a list of cuda uint8 tensors, container f the volume of field f, all of the same dims (they are
        concatenated first unless they already lie back to back in one buffer).  They are decoded into the fields of
        `out`, an interleaved cuda tensor (fields_of) with as many fields as containers -- a slice t[..., a:b] of a
        wider one, a halo interior --, and nothing else of it is written; out=None makes a contiguous (z, y, x, c)
        tensor.  Returns `out`."""
        torch = self.torch
        assert len(containers) > 0
        for c in containers:
            assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 1 and c.is_contiguous()
        nf = len(containers)
        packed = all(b.data_ptr() == a.data_ptr() + a.numel() and
                     b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
                     for a, b in zip(containers, containers[1:]))
        src = containers[0] if packed else torch.cat(list(containers))
        offs = (_sz * (nf + 1))()
        for f, c in enumerate(containers):
            offs[f + 1] = offs[f] + c.numel()
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            shape_zyx, _, _ = self.parse_header(src[:offs[1]])
            out = torch.empty(tuple(shape_zyx) + (nf,), dtype=dt, device=src.device)
            field_dim = -1
        assert out.dtype == dt and out.is_cuda
        lay, nfo, (dz, dy, dx) = self.fields_of(out, field_dim)
        if nfo != nf:
            raise SperrHipError(f"{nf} containers for {nfo} fields")
        rtn = self.lib.sperrhip_decompress_fields_dev(src.data_ptr(), offs, nf, int(output_float), dx, dy, dz,
                                                      out.data_ptr(), C.byref(lay), self._room_bytes(out),
                                                      self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_fields_dev returned {rtn}")
        return out

    def quality_fields(self, orig, recon, field_dim=-1):
        """quality() of every field of two interleaved cuda tensors (fields_of) of one shape and dtype, whose layouts
        may differ: a list of Quality records, each the figures of the two packed copies of that field."""
        lo, nf, zyx = self._fields_args(orig, field_dim)
        lr, nfr, zyxr = self._fields_args(recon, field_dim)
        if orig.dtype != recon.dtype or nf != nfr or zyx != zyxr:
            raise SperrHipError(f"the two tensors differ in dtype or shape: {tuple(orig.shape)} and {tuple(recon.shape)}")
        dz, dy, dx = zyx
        out = (C.c_double * (8 * nf))()
        rtn = self.lib.sperrhip_quality_fields_dev(orig.data_ptr(), C.byref(lo), recon.data_ptr(), C.byref(lr), nf,
                                                   int(orig.dtype == self.torch.float32), dx, dy, dz, out,
                                                   self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_quality_fields_dev returned {rtn}")
        return [Quality(out[8 * f:8 * f + 8], dz * dy * dx) for f in range(nf)]

    def fields_gather(self, t, field_dim=-1, out=None):
        """Stage access: the fields of an interleaved cuda tensor (fields_of) as stacked volumes (c, z, y, x), what
        compress_batch takes -- `out` when given (contiguous)."""
        torch = self.torch
        lay, nf, (dz, dy, dx) = self._fields_args(t, field_dim)
        if out is None:
            out = torch.empty((nf, dz, dy, dx), dtype=t.dtype, device=t.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == t.dtype
        rtn = self.lib.sperrhip_fields_gather_dev(t.data_ptr(), C.byref(lay), nf, int(t.dtype == torch.float32), dx, dy,
                                                  dz, out.data_ptr(), out.numel() * out.element_size(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_fields_gather_dev returned {rtn}")
        return out

    def fields_scatter(self, stacked, out, field_dim=-1):
        """Stage access: stacked volumes (c, z, y, x), contiguous, into the fields of the interleaved cuda tensor `out`
        (fields_of); nothing else of `out` is written."""
        torch = self.torch
        assert stacked.is_cuda and stacked.is_contiguous() and stacked.dim() == 4 and stacked.dtype == out.dtype
        lay, nf, (dz, dy, dx) = self._fields_args(out, field_dim)
        if tuple(stacked.shape) != (nf, dz, dy, dx):
            raise SperrHipError(f"stacked volumes {tuple(stacked.shape)} for fields {(nf, dz, dy, dx)}")
        rtn = self.lib.sperrhip_fields_scatter_dev(stacked.data_ptr(), nf, int(out.dtype == torch.float32), dx, dy, dz,
                                                   out.data_ptr(), C.byref(lay), self._room_bytes(out), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_fields_scatter_dev returned {rtn}")
        return out

    # ---- missing values ----------------------------------------------------------------------
    @staticmethod
    def _missing_rule(missing):
        """(rule, threshold) of include/sperr_hip.h: "nan", or the threshold of the absolute-value rule"""
        if isinstance(missing, str):
            if missing != "nan":
                raise ValueError(f'missing is "nan" or a threshold, not {missing!r}')
            return 1, 0.0
        return 2, float(missing)

    def _mask_arg(self, mask):
        torch = self.torch
        assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous()
        if mask.data_ptr() % 8:
            raise SperrHipError("a mask stream starts on an 8-byte boundary")

    def mask_max_size(self, n):
        return self.lib.sperrhip_mask_max_size(n)

    @staticmethod
    def _fill_kind(fill):
        """(kind, value) of include/sperr_hip.h, SPERRHIP_FILL_*: "midrange", "smooth", or the caller's number"""
        if isinstance(fill, str):
            if fill not in ("midrange", "smooth"):
                raise ValueError(f'fill is "midrange", "smooth" or a number, not {fill!r}')
            return (0 if fill == "midrange" else 2), 0.0
        return 1, float(fill)

    def mask_make(self, vol, missing="nan", filled_out=None, fill="midrange"):
        """The mask stream of a contiguous cuda tensor (float32 / float64, any shape): which samples are missing --
        NaNs, or with a number those whose absolute value is not below it -- as (cuda uint8 tensor, nmissing).
        filled_out (same dtype and numel; may be `vol` itself) receives the in-filled samples: the missing ones hold
        the midrange of the valid ones, the number given as `fill`, or with "smooth" a pull-push extension of the valid
        samples into the missing region, for which the tensor's shape is (z, y, x) -- fewer dimensions lead with 1s,
        more than three are refused."""
        torch = self.torch
        assert vol.is_cuda and vol.is_contiguous() and vol.dtype in (torch.float32, torch.float64)
        if filled_out is not None:
            assert filled_out.is_cuda and filled_out.is_contiguous() and filled_out.dtype == vol.dtype
            assert filled_out.numel() == vol.numel()
        rule, thr = self._missing_rule(missing)
        kind, value = self._fill_kind(fill)
        n = vol.numel()
        mask = torch.empty(self.mask_max_size(n), dtype=torch.uint8, device=vol.device)
        mlen, nmiss = _sz(0), _sz(0)
        filled = None if filled_out is None else filled_out.data_ptr()
        if kind == 0:
            rtn = self.lib.sperrhip_mask_make_dev(vol.data_ptr(), int(vol.dtype == torch.float32), n, rule, thr,
                                                  filled, mask.data_ptr(), mask.numel(), C.byref(mlen),
                                                  C.byref(nmiss), self._stream())
            if rtn != 0:
                raise SperrHipError(f"sperrhip_mask_make_dev returned {rtn}")
            return mask[:mlen.value], nmiss.value
        dx, dy, dz = n, 1, 1
        if kind == 2:
            if vol.dim() > 3:
                raise SperrHipError(f"a smooth fill takes a shape (z, y, x): {vol.dim()} dimensions are refused")
            dz, dy, dx = (1,) * (3 - vol.dim()) + tuple(vol.shape)
        rtn = self.lib.sperrhip_mask_make_vol_dev(vol.data_ptr(), int(vol.dtype == torch.float32), dx, dy, dz, rule,
                                                  thr, kind, value, filled, mask.data_ptr(), mask.numel(),
                                                  C.byref(mlen), C.byref(nmiss), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_mask_make_vol_dev returned {rtn}")
        return mask[:mlen.value], nmiss.value

    def mask_parse(self, mask):
        """(n, nmissing, kind) of a mask stream's header, read on the current stream"""
        self._mask_arg(mask)
        n, nmiss, kind = _sz(0), _sz(0), C.c_int(0)
        rtn = self.lib.sperrhip_mask_parse_stream_dev(mask.data_ptr(), mask.numel(), C.byref(n), C.byref(nmiss),
                                                      C.byref(kind), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_mask_parse_stream_dev returned {rtn}")
        return n.value, nmiss.value, kind.value

    def mask_apply(self, vol, mask, value, box_lo_xyz=None, box_dims_xyz=None, vol_shape_zyx=None):
        """`value` into the missing samples of `vol`, a contiguous cuda tensor, in place; nothing else is written.
        With a box, `vol` is the box [lo, lo + dims) (x, y, z order) of a volume of vol_shape_zyx."""
        torch = self.torch
        assert vol.is_cuda and vol.is_contiguous() and vol.dtype in (torch.float32, torch.float64)
        self._mask_arg(mask)
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        if dims is None:   # (the whole volume is one run of samples: only their number matters)
            vd = (_sz * 3)(vol.numel(), 1, 1)
        else:
            if vol_shape_zyx is None:
                raise ValueError("a box needs vol_shape_zyx")
            if vol.numel() != math.prod(box_dims_xyz):
                raise SperrHipError(f"a tensor of {vol.numel()} samples for a box (x, y, z) {tuple(box_dims_xyz)}")
            vd = (_sz * 3)(*(int(d) for d in reversed(vol_shape_zyx)))
        rtn = self.lib.sperrhip_mask_apply_dev(vol.data_ptr(), int(vol.dtype == torch.float32), vd, lo, dims,
                                               mask.data_ptr(), mask.numel(), float(value), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_mask_apply_dev returned {rtn}")
        return vol

    def mask_bits(self, mask):
        """The mask as a flat cuda torch.bool tensor of n entries, True where a sample is missing"""
        torch = self.torch
        n, _, _ = self.mask_parse(mask)
        out = torch.empty(n, dtype=torch.uint8, device=mask.device)
        rtn = self.lib.sperrhip_mask_expand_dev(mask.data_ptr(), mask.numel(), out.data_ptr(), n, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_mask_expand_dev returned {rtn}")
        return out.view(torch.bool)

    def compress_masked(self, vol, chunks_xyz, quality, mode=1, missing="nan", fill="midrange"):
        """A contiguous cuda tensor (z, y, x) with missing samples (mask_make) as (container, mask): the container is
        compress() of the in-filled volume, which any SPERR reader decodes; the mask says which samples were missing.
        `fill` as in mask_make: "smooth" gives the smaller container, the decode is the same for every fill."""
        torch = self.torch
        assert vol.is_cuda and vol.dim() == 3 and vol.dtype in (torch.float32, torch.float64)
        self._no_view(vol, "compress_masked")
        rule, thr = self._missing_rule(missing)
        kind, value = self._fill_kind(fill)
        dz, dy, dx = vol.shape
        out = torch.empty(self.max_compressed_size(vol.shape, chunks_xyz, quality, mode), dtype=torch.uint8,
                          device=vol.device)
        mask = torch.empty(self.mask_max_size(vol.numel()), dtype=torch.uint8, device=vol.device)
        n, mlen, nmiss = _sz(0), _sz(0), _sz(0)
        if kind == 0:
            name = "sperrhip_compress_masked_dev"
            rtn = self.lib.sperrhip_compress_masked_dev(vol.data_ptr(), int(vol.dtype == torch.float32), dx, dy, dz,
                                                        *chunks_xyz, mode, float(quality), rule, thr, out.data_ptr(),
                                                        out.numel(), C.byref(n), mask.data_ptr(), mask.numel(),
                                                        C.byref(mlen), C.byref(nmiss), self._stream())
        else:
            name = "sperrhip_compress_masked_fill_dev"
            rtn = self.lib.sperrhip_compress_masked_fill_dev(vol.data_ptr(), int(vol.dtype == torch.float32), dx, dy,
                                                             dz, *chunks_xyz, mode, float(quality), rule, thr, kind,
                                                             value, out.data_ptr(), out.numel(), C.byref(n),
                                                             mask.data_ptr(), mask.numel(), C.byref(mlen),
                                                             C.byref(nmiss), self._stream())
        if rtn != 0:
            raise SperrHipError(f"{name} returned {rtn}")
        return out[:n.value], mask[:mlen.value]

    def decompress_masked(self, container, mask, value=float("nan"), box_lo_xyz=None, box_dims_xyz=None, pct=0,
                          output_float=True, out=None, level=None):
        """decompress() or, with a box, decompress_box() of a container, with `value` at the samples `mask` names.
        A level is refused, here alone: the C call has no level argument, because a mask has no coarser level."""
        torch = self.torch
        assert container.is_cuda and container.dtype == torch.uint8 and container.is_contiguous()
        self._mask_arg(mask)
        if level is not None:
            raise SperrHipError("decompress_masked decodes no level: a mask has no coarser level")
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            zyx = self.parse_header(container)[0] if dims is None else tuple(int(d) for d in reversed(box_dims_xyz))
            out = torch.empty(zyx, dtype=dt, device=container.device)
        assert out.dtype == dt and out.is_cuda
        self._no_view(out, "decompress_masked")
        rtn = self.lib.sperrhip_decompress_masked_dev(container.data_ptr(), container.numel(), int(pct),
                                                      int(output_float), lo, dims, mask.data_ptr(), mask.numel(),
                                                      float(value), out.data_ptr(), out.numel() * out.element_size(),
                                                      self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_masked_dev returned {rtn}")
        return out

    def quality_masked(self, orig, recon, mask):
        """quality() of the valid samples of two contiguous cuda tensors: the figures of the arrays compacted to the
        samples `mask` does not name, in linear order."""
        self._quality_args(orig, recon)
        self._mask_arg(mask)
        out = (C.c_double * 8)()
        rtn = self.lib.sperrhip_quality_masked_dev(orig.data_ptr(), recon.data_ptr(),
                                                   int(orig.dtype == self.torch.float32), orig.numel(),
                                                   mask.data_ptr(), mask.numel(), out, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_quality_masked_dev returned {rtn}")
        n, nmiss, _ = self.mask_parse(mask)
        return Quality(out[:8], n - nmiss)

    # ---- relative error ----------------------------------------------------------------------
    REL_MAPS = {"linear": 0, "log": 1}   # the map kinds of include/sperr_hip.h: SPERRHIP_REL_LINEAR, SPERRHIP_REL_LOG

    def _rel_map(self, map):
        if map not in self.REL_MAPS:
            raise ValueError(f"map is 'linear' or 'log', not {map!r}")
        return self.REL_MAPS[map]

    def rel_tolerance(self, eps, is_float=True, map="linear"):
        """t of eps (include/sperr_hip.h, "relative error"): the point-wise tolerance of the y volume under the map
        kind `map`, "linear" (y the piecewise linear interpolant of log2|x|) or "log" (y = log2|x|).  A refused eps
        raises."""
        t = C.c_double(0.0)
        if self.lib.sperrhip_rel_tolerance_kind(float(eps), int(bool(is_float)), self._rel_map(map), C.byref(t)) != 0:
            raise SperrHipError(f"a relative bound of {eps!r} is refused")
        return t.value

    def rel_max_size(self, n):
        return self.lib.sperrhip_rel_max_size(n)

    def _side_arg(self, side):
        torch = self.torch
        assert side.is_cuda and side.dtype == torch.uint8 and side.is_contiguous()
        if side.data_ptr() % 8:
            raise SperrHipError("a side stream starts on an 8-byte boundary")

    def rel_forward(self, vol, map="linear"):
        """(y, side, nzero, nneg) of a contiguous cuda tensor (float32 / float64, any shape): y as a float64 tensor of
        the same shape, NaN in the zero class, and the side stream with the zero and sign bits (its eps is 0.0: a
        forward call states no bound).  `map` as in rel_tolerance; the side stream names it."""
        torch = self.torch
        assert vol.is_cuda and vol.is_contiguous() and vol.dtype in (torch.float32, torch.float64)
        n = vol.numel()
        y = torch.empty(vol.shape, dtype=torch.float64, device=vol.device)
        side = torch.empty(self.rel_max_size(n), dtype=torch.uint8, device=vol.device)
        slen, nzero, nneg = _sz(0), _sz(0), _sz(0)
        kind = self._rel_map(map)
        rtn = self.lib.sperrhip_rel_forward_kind_dev(vol.data_ptr(), int(vol.dtype == torch.float32), n, kind,
                                                     y.data_ptr(), side.data_ptr(), side.numel(), C.byref(slen),
                                                     C.byref(nzero), C.byref(nneg), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_rel_forward_kind_dev returned {rtn}")
        return y, side[:slen.value], nzero.value, nneg.value

    def rel_inverse(self, y, side, box_lo_xyz=None, box_dims_xyz=None, vol_shape_zyx=None, output_float=True,
                    out=None):
        """x' of y', a contiguous cuda float64 tensor: the whole volume, or with a box the box [lo, lo + dims)
        (x, y, z order) of a volume of vol_shape_zyx.  out=y works in place when output_float is False.  The map kind
        is the side stream's."""
        torch = self.torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == torch.float64
        self._side_arg(side)
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        if dims is None:   # (the whole volume is one run of samples: only their number matters)
            vd = (_sz * 3)(y.numel(), 1, 1)
        else:
            if vol_shape_zyx is None:
                raise ValueError("a box needs vol_shape_zyx")
            if y.numel() != math.prod(box_dims_xyz):
                raise SperrHipError(f"a tensor of {y.numel()} samples for a box (x, y, z) {tuple(box_dims_xyz)}")
            vd = (_sz * 3)(*(int(d) for d in reversed(vol_shape_zyx)))
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty(y.shape, dtype=dt, device=y.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == dt and out.numel() == y.numel()
        rtn = self.lib.sperrhip_rel_inverse_dev(y.data_ptr(), vd, lo, dims, side.data_ptr(), side.numel(),
                                                int(output_float), out.data_ptr(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_rel_inverse_dev returned {rtn}")
        return out

    def compress_rel(self, vol, chunks_xyz, eps, fill="smooth", map="linear"):
        """A contiguous cuda tensor (z, y, x) of finite samples as (container, side) under the point-wise relative
        bound |x' - x| <= eps |x|, zeros and signs exact: the container is compress_masked() of the double volume y in
        point-wise error mode at rel_tolerance(eps), which any SPERR reader decodes; the side stream holds the zero
        and sign bits.  `fill` as in mask_make, in y's domain: what stands where a sample is zero.  `map` as in
        rel_tolerance: "log" gives the smaller container; decompress_rel reads the kind off the side stream."""
        torch = self.torch
        assert vol.is_cuda and vol.dim() == 3 and vol.dtype in (torch.float32, torch.float64)
        self._no_view(vol, "compress_rel")
        is_float = vol.dtype == torch.float32
        t = self.rel_tolerance(eps, is_float, map)
        kind, value = self._fill_kind(fill)
        dz, dy, dx = vol.shape
        out = torch.empty(self.max_compressed_size(vol.shape, chunks_xyz, t, 3), dtype=torch.uint8, device=vol.device)
        side = torch.empty(self.rel_max_size(vol.numel()), dtype=torch.uint8, device=vol.device)
        n, slen = _sz(0), _sz(0)
        rtn = self.lib.sperrhip_compress_rel_kind_dev(vol.data_ptr(), int(is_float), dx, dy, dz, *chunks_xyz,
                                                      float(eps), self._rel_map(map), kind, value, out.data_ptr(),
                                                      out.numel(), C.byref(n), side.data_ptr(), side.numel(),
                                                      C.byref(slen), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_rel_kind_dev returned {rtn}")
        return out[:n.value], side[:slen.value]

    def decompress_rel(self, container, side, box_lo_xyz=None, box_dims_xyz=None, pct=0, output_float=True, out=None):
        """x' of a container and side stream of compress_rel: the whole volume or, with a box, the box.  A portion
        (pct other than 0 or 100) carries no bound: finite values, zeros and signs exact."""
        torch = self.torch
        assert container.is_cuda and container.dtype == torch.uint8 and container.is_contiguous()
        self._side_arg(side)
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            zyx = self.parse_header(container)[0] if dims is None else tuple(int(d) for d in reversed(box_dims_xyz))
            out = torch.empty(zyx, dtype=dt, device=container.device)
        assert out.dtype == dt and out.is_cuda
        self._no_view(out, "decompress_rel")
        rtn = self.lib.sperrhip_decompress_rel_dev(container.data_ptr(), container.numel(), int(pct),
                                                   int(output_float), lo, dims, side.data_ptr(), side.numel(),
                                                   out.data_ptr(), out.numel() * out.element_size(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_rel_dev returned {rtn}")
        return out

    def _rel_parse(self, side):
        self._side_arg(side)
        isf, eps, n, nzero, nneg, kind = C.c_int(0), C.c_double(0.0), _sz(0), _sz(0), _sz(0), C.c_int(0)
        rtn = self.lib.sperrhip_rel_parse_stream_kind_dev(side.data_ptr(), side.numel(), C.byref(isf), C.byref(eps),
                                                          C.byref(n), C.byref(nzero), C.byref(nneg), C.byref(kind),
                                                          self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_rel_parse_stream_kind_dev returned {rtn}")
        return (bool(isf.value), eps.value, n.value, nzero.value, nneg.value), kind.value

    def rel_parse(self, side):
        """(is_float, eps, n, nzero, nneg) of a side stream's headers, read on the current stream"""
        return self._rel_parse(side)[0]

    def rel_kind(self, side):
        """"linear" or "log": the map kind a side stream names"""
        kind = self._rel_parse(side)[1]
        return next(name for name, k in self.REL_MAPS.items() if k == kind)

    def rel_check(self, orig, recon, eps):
        """(worst, violations, mismatches, counted) of two contiguous cuda tensors of one dtype: over the samples
        whose original is no zero the largest |x' - x| / |x| and how many exceed eps, how many samples differ in zero
        class or sign, and how many originals are no zeros."""
        self._quality_args(orig, recon)
        out = (C.c_double * 4)()
        rtn = self.lib.sperrhip_rel_check_dev(orig.data_ptr(), recon.data_ptr(),
                                              int(orig.dtype == self.torch.float32), orig.numel(), float(eps), out,
                                              self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_rel_check_dev returned {rtn}")
        return out[0], int(out[1]), int(out[2]), int(out[3])

    # ---- stage access ----------------------------------------------------------------------
    def dwt3d(self, vals, inverse=False):
        """In-place on a contiguous cuda float64 tensor shaped (z, y, x)."""
        torch = self.torch
        assert vals.is_cuda and vals.dtype == torch.float64 and vals.is_contiguous()
        dz, dy, dx = vals.shape
        rtn = self.lib.sperrhip_dwt3d_dev(vals.data_ptr(), dx, dy, dz, int(inverse), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_dwt3d_dev returned {rtn}")
        return vals

    def speck3d_encode(self, coef, sign, budget_bits=0, _slice=False):
        """coef: cuda int32 (uint32 bits) or int64 (uint64 bits) tensor (z, y, x); sign: cuda int64
        tensor of (n+63)//64 words. Returns the stream as bytes."""
        torch = self.torch
        assert coef.is_cuda and coef.is_contiguous() and sign.is_cuda
        width = coef.element_size()
        if _slice:   # dimz = 0 asks the entry for the plan of a dx x dy slice
            dz, (dy, dx) = 0, coef.shape
        else:
            dz, dy, dx = coef.shape
        n = coef.numel()
        cap = 9 + (budget_bits + 7) // 8 + 64 if budget_bits else 9 + 70 * n // 8 + 4096
        out = torch.empty(cap, dtype=torch.uint8, device=coef.device)
        ln = _sz(0)
        rtn = self.lib.sperrhip_speck3d_encode_dev(coef.data_ptr(), width, sign.data_ptr(), dx, dy,
                                                   dz, budget_bits, out.data_ptr(), cap,
                                                   C.byref(ln), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_speck3d_encode_dev returned {rtn}")
        return bytes(out[:ln.value].cpu().numpy())

    def speck3d_plane_bits(self, coef, sign):
        """The plane table of one chunk's quantised coefficients (cuda int32 holding uint32 bits, (z, y, x); sign as in
        speck3d_encode): (end, nbp) -- end[p], a numpy uint64 array of 64, the stream's bits at the end of plane p
        under an unlimited budget, zeros from the plane count nbp on.  Counted, not coded: no stream is written."""
        assert coef.is_cuda and coef.is_contiguous() and sign.is_cuda and coef.dim() == 3
        dz, dy, dx = coef.shape
        end = np.zeros(64, dtype=np.uint64)
        nbp = C.c_int(0)
        rtn = self.lib.sperrhip_speck3d_plane_bits_dev(coef.data_ptr(), coef.element_size(), sign.data_ptr(), dx, dy, dz,
                                                       end.ctypes.data, C.byref(nbp), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_speck3d_plane_bits_dev returned {rtn}")
        return end, nbp.value

    def speck2d_encode(self, coef, sign, budget_bits=0):
        """The 2D coder (the quadtree forest and the type-I set of a slice) on its own.  coef: cuda int32 (uint32
        bits) or int64 (uint64 bits) tensor (y, x); sign as in speck3d_encode.  Returns the stream as bytes."""
        assert coef.dim() == 2
        return self.speck3d_encode(coef, sign, budget_bits, _slice=True)

    def speck2d_decode(self, stream, shape_yx):
        """Returns (coef uint64 numpy (y, x), sign uint64 numpy words) of a 2D coder's stream."""
        dy, dx = shape_yx
        c, s = self.speck3d_decode(stream, (1, dy, dx), _slice=True)
        return c.reshape(dy, dx), s

    def speck3d_decode(self, stream, shape_zyx, _slice=False):
        """Returns (coef uint64 numpy (z,y,x), sign uint64 numpy words)."""
        torch = self.torch
        dz, dy, dx = shape_zyx
        n = dz * dy * dx
        if _slice:   # dimz = 0 asks the entry for the plan of a dx x dy slice
            assert dz == 1
            dz = 0
        s = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
        coef = torch.zeros(n, dtype=torch.int64, device="cuda")
        sign = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        w = C.c_int(0)
        rtn = self.lib.sperrhip_speck3d_decode_dev(s.data_ptr(), s.numel(), dx, dy, dz,
                                                   coef.data_ptr(), sign.data_ptr(), C.byref(w),
                                                   self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_speck3d_decode_dev returned {rtn}")
        raw = coef.cpu().numpy()
        if w.value == 4:
            c = raw.view(np.uint32)[:n].astype(np.uint64)
        else:
            c = raw.view(np.uint64)
        return c.reshape(shape_zyx), sign.cpu().numpy().view(np.uint64)

    def outlier_encode(self, orig, recon, chunk_shape_zyx, tol):
        """orig: cuda float32 / float64 tensor, recon: cuda float64 tensor, both nchunks chunks of chunk_shape_zyx
        stacked along z.  Returns the chunks' outlier streams as a list of bytes (b"": no sample beyond tol)."""
        torch = self.torch
        assert orig.is_cuda and recon.is_cuda and orig.is_contiguous() and recon.is_contiguous()
        assert orig.dtype in (torch.float32, torch.float64) and recon.dtype == torch.float64
        dz, dy, dx = chunk_shape_zyx
        n = dz * dy * dx
        assert orig.numel() == recon.numel() and orig.numel() % n == 0 and orig.numel() > 0
        nch = orig.numel() // n
        cap = nch * (9 + 33 * n + 64)   # (at most 4 * 64 + 1 bits a sample: pwe_stage_finish's dense bound)
        out = torch.empty(cap, dtype=torch.uint8, device=orig.device)
        lens = (_sz * nch)()
        rtn = self.lib.sperrhip_outlier_encode_dev(orig.data_ptr(), int(orig.dtype == torch.float32), recon.data_ptr(),
                                                   dx, dy, dz, nch, float(tol), out.data_ptr(), cap, lens,
                                                   self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_outlier_encode_dev returned {rtn}")
        host = out[:sum(lens)].cpu().numpy().tobytes()
        offs = np.concatenate([[0], np.cumsum(list(lens))]).astype(np.int64)
        return [host[offs[c]:offs[c + 1]] for c in range(nch)]

    # ---- reference-compatible host API (include/sperr_hip.h) ------------------------------
    def comp_3d(self, vol, chunks_xyz, mode, quality, nthreads=0):
        vol = np.ascontiguousarray(vol)
        dz, dy, dx = vol.shape
        dst, n = _vp(None), _sz(0)
        rtn = self.lib.sperr_comp_3d(vol.ctypes.data, int(vol.dtype == np.float32), dx, dy, dz,
                                     *chunks_xyz, mode, quality, nthreads, C.byref(dst),
                                     C.byref(n))
        if rtn != 0:
            raise SperrHipError(f"sperr_comp_3d returned {rtn}")
        out = C.string_at(dst.value, n.value)
        self._libc.free(dst)
        return out

    def trunc_3d(self, stream, pct):
        buf = np.frombuffer(stream, dtype=np.uint8)
        dst, n = _vp(None), _sz(0)
        rtn = self.lib.sperr_trunc_3d(buf.ctypes.data, buf.size, pct, C.byref(dst), C.byref(n))
        if rtn != 0:
            raise SperrHipError(f"sperr_trunc_3d returned {rtn}")
        out = C.string_at(dst.value, n.value)
        self._libc.free(dst)
        return out

    def decomp_3d(self, stream, output_float=True, nthreads=0):
        buf = np.frombuffer(stream, dtype=np.uint8)
        dst = _vp(None)
        dx, dy, dz = _sz(0), _sz(0), _sz(0)
        rtn = self.lib.sperr_decomp_3d(buf.ctypes.data, buf.size, int(output_float), nthreads,
                                       C.byref(dx), C.byref(dy), C.byref(dz), C.byref(dst))
        if rtn != 0:
            raise SperrHipError(f"sperr_decomp_3d returned {rtn}")
        n = dx.value * dy.value * dz.value
        dt = np.float32 if output_float else np.float64
        out = np.frombuffer(C.string_at(dst.value, n * np.dtype(dt).itemsize), dtype=dt).copy()
        self._libc.free(dst)
        return out.reshape(dz.value, dy.value, dx.value)

    def decomp_3d_box(self, stream, box_lo_xyz, box_dims_xyz, output_float=True):
        """The box [lo, lo + dims) (x, y, z order) of a host container (bytes or a uint8 array, pageable or
        pinned) as a numpy array shaped (dims z, dims y, dims x); one device decodes it."""
        buf = stream if isinstance(stream, np.ndarray) else np.frombuffer(stream, dtype=np.uint8)
        dst = _vp(None)
        rtn = self.lib.sperrhip_decomp_3d_box(buf.ctypes.data, buf.size, int(output_float), (_sz * 3)(*box_lo_xyz),
                                              (_sz * 3)(*box_dims_xyz), C.byref(dst))
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decomp_3d_box returned {rtn}")
        dx, dy, dz = (int(d) for d in box_dims_xyz)
        dt = np.float32 if output_float else np.float64
        out = np.frombuffer(C.string_at(dst.value, dx * dy * dz * np.dtype(dt).itemsize), dtype=dt).copy()
        self._libc.free(dst)
        return out.reshape(dz, dy, dx)

    def decomp_3d_level(self, stream, level, box_lo_xyz=None, box_dims_xyz=None, output_float=False):
        """Level `level` of a host container's hierarchy (bytes or a uint8 array, pageable or pinned), whole or the
        box [lo, lo + dims) of it in the level's coordinates, as a numpy array shaped (z, y, x)."""
        buf = stream if isinstance(stream, np.ndarray) else np.frombuffer(stream, dtype=np.uint8)
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        dst = _vp(None)
        od = (_sz * 3)()
        rtn = self.lib.sperrhip_decomp_3d_level(buf.ctypes.data, buf.size, int(output_float), level, lo, dims, od,
                                                C.byref(dst))
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decomp_3d_level returned {rtn}")
        dx, dy, dz = int(od[0]), int(od[1]), int(od[2])
        dt = np.float32 if output_float else np.float64
        out = np.frombuffer(C.string_at(dst.value, dx * dy * dz * np.dtype(dt).itemsize), dtype=dt).copy()
        self._libc.free(dst)
        return out.reshape(dz, dy, dx)

    def decomp_3d_portion(self, stream, pct, level=None, box_lo_xyz=None, box_dims_xyz=None, output_float=True):
        """The volume (no level, no box), a box of it, a level of the hierarchy or a box of one, of a host container
        (bytes or a uint8 array), decoded from the first pct percent of every chunk stream: only those bytes of the
        chosen chunks travel to the device.  A numpy array shaped (z, y, x)."""
        buf = stream if isinstance(stream, np.ndarray) else np.frombuffer(stream, dtype=np.uint8)
        lo, dims = self._box_args(box_lo_xyz, box_dims_xyz)
        dst = _vp(None)
        od = (_sz * 3)()
        rtn = self.lib.sperrhip_decomp_3d_portion(buf.ctypes.data, buf.size, int(pct), int(output_float),
                                                  None if level is None else C.byref(_sz(level)), lo, dims, od,
                                                  C.byref(dst))
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decomp_3d_portion returned {rtn}")
        dx, dy, dz = int(od[0]), int(od[1]), int(od[2])
        dt = np.float32 if output_float else np.float64
        out = np.frombuffer(C.string_at(dst.value, dx * dy * dz * np.dtype(dt).itemsize), dtype=dt).copy()
        self._libc.free(dst)
        return out.reshape(dz, dy, dx)

    # ---- chunk farm on an explicit device list (include/sperr_hip.h) -------------------------
    @staticmethod
    def _devs(devices):
        if not devices:
            return None, 0
        arr = (C.c_int * len(devices))(*devices)
        return arr, len(devices)

    def comp_3d_farm(self, vol, chunks_xyz, mode, quality, devices=None, nthreads=0):
        """vol: numpy (z, y, x) or a pinned torch CPU tensor; -> container bytes."""
        ptr, shape, is_float = self._host_array(vol)
        dz, dy, dx = shape
        dst, n = _vp(None), _sz(0)
        arr, nd = self._devs(devices)
        rtn = self.lib.sperrhip_comp_3d_farm(ptr, is_float, dx, dy, dz, *chunks_xyz, mode, quality,
                                             nthreads, arr, nd, C.byref(dst), C.byref(n))
        if rtn != 0:
            raise SperrHipError(f"sperrhip_comp_3d_farm returned {rtn}")
        out = C.string_at(dst.value, n.value)
        self._libc.free(dst)
        return out

    def _host_array(self, vol, writable=False):
        """(pointer, shape, is_float) of a host volume.  float32 or float64 only -- anything else would
        be read with the wrong element size; an output buffer must be C-contiguous (a copy made here
        would take the values and the caller's array would stay empty)."""
        if isinstance(vol, np.ndarray):
            if vol.dtype not in (np.float32, np.float64):
                raise SperrHipError(f"host volumes are float32 or float64, not {vol.dtype}")
            if writable and not (vol.flags.c_contiguous and vol.flags.writeable):
                raise SperrHipError("the output array must be C-contiguous and writable")
            vol = np.ascontiguousarray(vol)
            self._keep = vol
            return vol.ctypes.data, vol.shape, int(vol.dtype == np.float32)
        if vol.is_cuda or not vol.is_contiguous():
            raise SperrHipError("a torch host volume must be a contiguous CPU tensor")
        if vol.dtype not in (self.torch.float32, self.torch.float64):
            raise SperrHipError(f"host volumes are float32 or float64, not {vol.dtype}")
        return vol.data_ptr(), tuple(vol.shape), int(vol.dtype == self.torch.float32)

    def release(self):
        """sperrhip_release: idle engines and farm workers give their memory back."""
        self.lib.sperrhip_release.restype = None
        self.lib.sperrhip_release.argtypes = []
        self.lib.sperrhip_release()

    def decomp_3d_farm(self, stream, output_float=True, devices=None, nthreads=0):
        buf = np.frombuffer(stream, dtype=np.uint8)
        dst = _vp(None)
        dx, dy, dz = _sz(0), _sz(0), _sz(0)
        arr, nd = self._devs(devices)
        rtn = self.lib.sperrhip_decomp_3d_farm(buf.ctypes.data, buf.size, int(output_float), nthreads,
                                               arr, nd, C.byref(dx), C.byref(dy), C.byref(dz),
                                               C.byref(dst))
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decomp_3d_farm returned {rtn}")
        n = dx.value * dy.value * dz.value
        dt = np.float32 if output_float else np.float64
        out = np.frombuffer(C.string_at(dst.value, n * np.dtype(dt).itemsize), dtype=dt).copy()
        self._libc.free(dst)
        return out.reshape(dz.value, dy.value, dx.value)

    def decomp_3d_into(self, stream, out, devices=None, nthreads=0):
        """out: numpy array or (pinned) torch CPU tensor shaped (z, y, x), float32 or float64."""
        buf = np.frombuffer(stream, dtype=np.uint8) if isinstance(stream, (bytes, bytearray)) else stream
        sptr = buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr()
        slen = buf.size if isinstance(buf, np.ndarray) else buf.numel()
        ptr, shape, is_float = self._host_array(out, writable=True)
        nbytes = int(np.prod(shape)) * (4 if is_float else 8)
        dx, dy, dz = _sz(0), _sz(0), _sz(0)
        arr, nd = self._devs(devices)
        rtn = self.lib.sperrhip_decomp_3d_into(sptr, slen, is_float, nthreads, arr, nd, ptr, nbytes,
                                               C.byref(dx), C.byref(dy), C.byref(dz))
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decomp_3d_into returned {rtn}")
        assert (dz.value, dy.value, dx.value) == tuple(shape)
        return out

    # ---- 2D slices --------------------------------------------------------------------------
    def compress_2d(self, img, quality, mode=1, header=False):
        """img: cuda tensor float32/float64 (y, x). Returns a cuda uint8 tensor (sperr_comp_2d)."""
        torch = self.torch
        self._no_view(img, "compress_2d")
        assert img.is_cuda and img.is_contiguous() and img.dim() == 2
        dy, dx = img.shape
        self.lib.sperrhip_max_compressed_size_2d.restype = _sz
        self.lib.sperrhip_max_compressed_size_2d.argtypes = [_sz, _sz, C.c_int, C.c_double]
        cap = self.lib.sperrhip_max_compressed_size_2d(dx, dy, mode, float(quality))
        out = torch.empty(cap, dtype=torch.uint8, device=img.device)
        n = _sz(0)
        self.lib.sperrhip_compress_2d_dev.argtypes = [C.c_void_p, C.c_int, _sz, _sz, C.c_int, C.c_double,
                                                      C.c_int, C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p]
        rtn = self.lib.sperrhip_compress_2d_dev(img.data_ptr(), int(img.dtype == torch.float32), dx, dy,
                                                mode, float(quality), int(header), out.data_ptr(),
                                                out.numel(), C.byref(n), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_2d_dev returned {rtn}")
        return out[:n.value]

    def decompress_2d(self, stream, shape_yx, output_float=True):
        """stream: cuda uint8 tensor WITHOUT the optional 10-byte header (sperr_decomp_2d)."""
        torch = self.torch
        dy, dx = shape_yx
        stream = stream.contiguous()
        out = torch.empty((dy, dx), dtype=torch.float32 if output_float else torch.float64,
                          device=stream.device)
        self.lib.sperrhip_decompress_2d_dev.argtypes = [C.c_void_p, _sz, C.c_int, _sz, _sz, C.c_void_p,
                                                        _sz, C.c_void_p]
        rtn = self.lib.sperrhip_decompress_2d_dev(stream.data_ptr(), stream.numel(), int(output_float),
                                                  dx, dy, out.data_ptr(),
                                                  out.numel() * out.element_size(), self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_2d_dev returned {rtn}")
        return out

    # ---- a batch of same-shape slices --------------------------------------------------------
    def max_compressed_size_2d_batch(self, nslice, shape_yx, quality, mode=1):
        dy, dx = shape_yx
        return self.lib.sperrhip_max_compressed_size_2d_batch(nslice, dx, dy, mode, float(quality))

    def compress_2d_batch(self, imgs, quality, mode=1, header=False, out=None):
        """imgs: contiguous cuda tensor float32/float64 shaped (N, y, x) -- N slices, or a (z, y, x) volume coded
        plane by plane.  Returns N cuda uint8 tensors, views into one buffer (`out` when it is large enough) in order:
        stream s is what compress_2d() makes of imgs[s]."""
        torch = self.torch
        assert imgs.is_cuda and imgs.is_contiguous() and imgs.dim() == 3
        assert imgs.dtype in (torch.float32, torch.float64)
        n, dy, dx = imgs.shape
        cap = self.max_compressed_size_2d_batch(n, (dy, dx), quality, mode)
        if cap == 0:
            raise SperrHipError("sperrhip_max_compressed_size_2d_batch: no slices, or the bound overflows")
        if out is None or out.numel() < cap:
            out = torch.empty(cap, dtype=torch.uint8, device=imgs.device)
        offs = (_sz * (n + 1))()
        rtn = self.lib.sperrhip_compress_2d_batch_dev(imgs.data_ptr(), int(imgs.dtype == torch.float32), n, dx, dy,
                                                      mode, float(quality), int(header), out.data_ptr(), out.numel(),
                                                      offs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_compress_2d_batch_dev returned {rtn}")
        return [out[offs[s]:offs[s + 1]] for s in range(n)]

    def decompress_2d_batch(self, streams, shape_yx, output_float=True, header=False, out=None):
        """streams: a list of cuda uint8 tensors (compress_2d_batch's views, or any), each the stream of a slice of
        shape_yx -- with the 10-byte header in front when `header`.  They are concatenated first unless they already
        lie back to back in one buffer.  Returns a cuda tensor shaped (N, y, x) -- `out` when given."""
        torch = self.torch
        assert len(streams) > 0
        for c in streams:
            assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 1 and c.is_contiguous()
        n = len(streams)
        dy, dx = shape_yx
        packed = all(b.data_ptr() == a.data_ptr() + a.numel() and
                     b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
                     for a, b in zip(streams, streams[1:]))
        src = streams[0] if packed else torch.cat(list(streams))
        offs = (_sz * (n + 1))()
        for s, c in enumerate(streams):
            offs[s + 1] = offs[s] + c.numel()
        dt = torch.float32 if output_float else torch.float64
        if out is None:
            out = torch.empty((n, dy, dx), dtype=dt, device=src.device)
        assert out.dtype == dt and out.is_contiguous() and out.is_cuda
        rtn = self.lib.sperrhip_decompress_2d_batch_dev(src.data_ptr(), offs, n, int(header), int(output_float), dx,
                                                        dy, out.data_ptr(), out.numel() * out.element_size(),
                                                        self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_2d_batch_dev returned {rtn}")
        return out

    # ---- multi-resolution decoding ----------------------------------------------------------
    def multires_levels(self, shape_zyx, chunks_xyz):
        """[(z, y, x) of every coarsened level], coarsest first (empty: no hierarchy exists)."""
        dz, dy, dx = shape_zyx
        nlev = _sz(0)
        dims = (_sz * 48)()
        self.lib.sperrhip_multires_levels.argtypes = [_sz] * 6 + [C.POINTER(_sz), C.POINTER(_sz)]
        if self.lib.sperrhip_multires_levels(dx, dy, dz, *chunks_xyz, C.byref(nlev), dims) != 0:
            raise SperrHipError("sperrhip_multires_levels failed")
        return [(dims[3 * h + 2], dims[3 * h + 1], dims[3 * h]) for h in range(nlev.value)]

    def decompress_multires(self, stream, output_float=True):
        """-> (volume, [float64 level volumes, coarsest first]); SPERR3D_OMP_D::decompress(p, true)."""
        torch = self.torch
        shape, _, chunks = self.parse_header(stream)   # (z, y, x), is_float, (x, y, z)
        lv = self.multires_levels(shape, chunks)
        out = torch.empty(shape, dtype=torch.float32 if output_float else torch.float64,
                          device=stream.device)
        levels = [torch.empty(s, dtype=torch.float64, device=stream.device) for s in lv]
        ptrs = (C.c_void_p * max(1, len(lv)))(*[t.data_ptr() for t in levels])
        self.lib.sperrhip_decompress_multires_dev.argtypes = [C.c_void_p, _sz, C.c_int, C.c_void_p,
                                                              _sz, _sz, C.c_void_p, C.c_void_p]
        rtn = self.lib.sperrhip_decompress_multires_dev(stream.data_ptr(), stream.numel(),
                                                        int(output_float), out.data_ptr(),
                                                        out.numel() * out.element_size(), len(lv),
                                                        ptrs, self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_multires_dev returned {rtn}")
        return out, levels

    def multires_levels_2d(self, shape_yx):
        """[(y, x) of every coarsened level of a slice], coarsest first."""
        dy, dx = shape_yx
        nlev = _sz(0)
        dims = (_sz * 32)()
        self.lib.sperrhip_multires_levels_2d.argtypes = [_sz, _sz, C.POINTER(_sz), C.POINTER(_sz)]
        if self.lib.sperrhip_multires_levels_2d(dx, dy, C.byref(nlev), dims) != 0:
            raise SperrHipError("sperrhip_multires_levels_2d failed")
        return [(dims[2 * h + 1], dims[2 * h]) for h in range(nlev.value)]

    def decompress_2d_multires(self, stream, shape_yx, output_float=True):
        """-> (slice, [float64 level slices, coarsest first]); SPECK2D_FLT::decompress(true)."""
        torch = self.torch
        dy, dx = shape_yx
        stream = stream.contiguous()
        lv = self.multires_levels_2d(shape_yx)
        out = torch.empty((dy, dx), dtype=torch.float32 if output_float else torch.float64,
                          device=stream.device)
        levels = [torch.empty(s, dtype=torch.float64, device=stream.device) for s in lv]
        ptrs = (C.c_void_p * max(1, len(lv)))(*[t.data_ptr() for t in levels])
        self.lib.sperrhip_decompress_2d_multires_dev.argtypes = [C.c_void_p, _sz, C.c_int, _sz, _sz, C.c_void_p,
                                                                 _sz, _sz, C.c_void_p, C.c_void_p]
        rtn = self.lib.sperrhip_decompress_2d_multires_dev(stream.data_ptr(), stream.numel(), int(output_float),
                                                           dx, dy, out.data_ptr(),
                                                           out.numel() * out.element_size(), len(lv), ptrs,
                                                           self._stream())
        if rtn != 0:
            raise SperrHipError(f"sperrhip_decompress_2d_multires_dev returned {rtn}")
        return out, levels

    # ---- profiling ------------------------------------------------------------------------
    def profile(self, on=True, only=None):
        """Bracket kernel launches with HIP events; `only`: just that kernel (cheap)."""
        self.lib.sperrhip_profile_only(only.encode() if only else None)
        self.lib.sperrhip_profile_enable(int(on))
        if on:
            self.lib.sperrhip_profile_reset()

    def profile_report(self, with_sum=False):
        """{kernel: (ms during which it was running, launches)}; with_sum: (busy ms, launches, sum
        of the launch durations) -- launches of sub-batches on different streams overlap."""
        cap = 128
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        sm = (C.c_double * cap)()
        cnt = (C.c_int * cap)()
        n = self.lib.sperrhip_profile_get2(names, ms, sm, cnt, cap)
        if with_sum:
            return {names[i].decode(): (ms[i], cnt[i], sm[i]) for i in range(min(n, cap))}
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(n, cap))}
