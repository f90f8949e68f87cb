"""GPU: the launches of the transform's two walks (float_stages, encode.hip, and enqueue_inverse, decode.hip) and of the brick
inverse (enqueue_brick_inverse, engine.hip: the encoder's point-wise-error reconstruction and the decoder's, with outlier correctors),
call by call.

A chunk shape's schedule (ShapePlan::schedule) says which kernels run its transform; the launch tables of
test_gpu_level.py pin what the decoder makes of it for fixed-rate containers of 32^3 chunks.  This file pins the
rest: the encoder, the two brick paths, the unfused fallbacks beside them and the second level as one launch.  Every
case compresses a volume and decodes the container as fp32 with the kernel profile on; the container has to equal
the CPU oracle's byte for byte, the decoded volume the oracle's bit for bit, and the launches -- kernel names with
their template arguments, and counts -- the tables below, exactly.

Cases (fp32 volumes of at most 64^3 samples):
  cubes            64^3 in 32^3 chunks at a fixed rate, a PSNR target and a PWE tolerance: two levels, x-y-z head
  cubes_level2     the same with SPERR_HIP_XYZ_LEVEL2=2: the level-2 region is 16^3, so both walks take the level-2
                   launch; the PWE reconstructions do not (the brick inverse never takes k_lift2_inv)
  one_level        32^3 in 16^3 chunks, PWE: one level, so the brick inverse has no coarse pass and its box is 1 x 1 x 1
  packet           a chunk of 2 x 23 x 20: a wavelet-packet transform (z passes only), PWE: the unfused fallbacks
  long_rows        a chunk of 512 x 20 x 20: dyadic, rows too long for the fused head, PWE: the unfused fallbacks
  wide             two chunks of 32^3, one constant, the other with more than 32 bit planes (the field of
                   test_gpu_level.py::test_level_parity_psnr_wide_coefficients, as fp32), at a PWE tolerance and at a
                   PSNR target: 64-bit coefficients, so neither side takes the brick inverse
The PWE tolerances were chosen with the oracle on the CPU so that chunks carry outlier streams -- without one the
decoder's brick path is skipped -- and every PWE case asserts that they do."""
import os

import numpy as np
import pytest

from fields import smooth_field
from sperr_amd.synth import turbulence
from test_gpu_level import outlier_start

pytestmark = pytest.mark.gpu
SWITCH = "SPERR_HIP_XYZ_LEVEL2"


def wide_field():
    v = smooth_field((32, 32, 64), dtype=np.float32)
    v[:, :, :32] = 0.75
    return v


# name -> (volume, chunk dims (x, y, z), the level-2 switch or None, [(label, mode, quality)])
CASES = {
    "cubes": (lambda: turbulence((64, 64, 64)), (32, 32, 32), None, [("rate", 1, 2.0), ("psnr", 2, 80.0), ("pwe", 3, 1e-3)]),
    "cubes_level2": (lambda: turbulence((64, 64, 64)), (32, 32, 32), "2", [("rate", 1, 2.0), ("psnr", 2, 80.0), ("pwe", 3, 1e-3)]),
    "one_level": (lambda: turbulence((32, 32, 32)), (16, 16, 16), None, [("pwe", 3, 1e-3)]),
    "packet": (lambda: turbulence((20, 23, 2)), (2, 23, 20), None, [("pwe", 3, 1e-3)]),
    "long_rows": (lambda: turbulence((20, 20, 512)), (512, 20, 20), None, [("pwe", 3, 1e-3)]),
    "wide": (wide_field, (32, 32, 32), None, [("pwe", 3, 1e-10), ("psnr", 2, 230.0)]),
}


def chunk_streams(container):
    """the chunks' streams (a container of one chunk has the short header, without chunk dims)"""
    multi = bool(container[1] & 0x10)
    pos = 20 if multi else 14
    vol = np.frombuffer(container, dtype=np.uint32, count=3, offset=2)
    ch = np.frombuffer(container, dtype=np.uint16, count=3, offset=14) if multi else vol
    nch = int(np.prod([(int(v) + int(c) - 1) // int(c) for v, c in zip(vol, ch)]))
    lens = np.frombuffer(container, dtype=np.uint32, count=nch, offset=pos)
    offs = pos + 4 * nch + np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])
    return [container[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from sperr_amd.api import SperrHip
    e = SperrHip()
    before = os.environ.get(SWITCH)
    yield e
    if before is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = before
    e.release()


def launched(eng, fn):
    """(what fn returns, {kernel name: launches}), as test_gpu_level.profile_names counts them"""
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: n for k, (_, n) in eng.profile_report().items() if n > 0}
    finally:
        eng.profile(False)


def collect(eng, oracle, name):
    """{"<label>/compress" | "<label>/decompress": launches} of a case, everything checked against the oracle"""
    import torch
    make, ch, sw, settings = CASES[name]
    v = make()
    assert v.dtype == np.float32 and v.size <= 64 ** 3
    before = os.environ.get(SWITCH)
    if sw is not None:
        os.environ[SWITCH] = sw
    eng.release()   # (the plans go: the next call makes them again and reads the switch)
    try:
        dv = torch.from_numpy(v).cuda()
        got = {}
        for label, mode, q in settings:
            want = oracle.comp_3d(v, ch, mode, q)
            streams = chunk_streams(want)
            if mode == 3:
                assert any(outlier_start(s) is not None for s in streams), (name, label, "no chunk has an outlier stream")
            if name == "wide":
                assert any(len(s) >= 26 and not (s[0] & 1) and s[17] > 32 for s in streams), (name, label, "no 64-bit chunk")
            c, got[label + "/compress"] = launched(eng, lambda: bytes(eng.compress(dv, ch, q, mode=mode).cpu().numpy()))
            assert c == want, (name, label, "container differs from the oracle's")
            dev = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()
            back, got[label + "/decompress"] = launched(eng, lambda: eng.decompress(dev, output_float=True).cpu().numpy())
            ref = oracle.decomp_3d(want, True)
            assert back.shape == ref.shape and back.dtype == ref.dtype, (name, label)
            assert np.array_equal(back.view(np.uint32), ref.view(np.uint32)), (name, label, "decoded volume differs")
        return got
    finally:
        if sw is not None:
            if before is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = before
            eng.release()


# Launches (kernel name -> count) of every call above, measured by collect() with the library built from the parent
# commit 53554cb ("Fuse the second transform level into one launch, forward and inverse"), before the schedule moved
# into the plan and the two brick inverses became one.
PARENT_LAUNCHES = {
    "cubes": {
        "rate/compress": {
            "(k_lift_axis<true, 0>)": 3, "(k_lift_xyz_fwd<1>)": 1, "k_born_place": 14, "k_bucket_scan": 1,
            "k_census": 1, "k_census_scan": 1, "k_chain": 4, "k_container_header": 1, "k_copy_slots": 1,
            "k_emit_pixels<uint32_t>": 1, "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1,
            "k_enc_state_init": 1, "k_list_apply": 14, "k_list_count": 14, "k_list_scan": 14, "k_make_q_rate": 1,
            "k_mask_scan": 14, "k_mean_finalize<T>": 1, "k_plane_turn": 16, "k_pyramid<false>": 4,
            "k_quantize4": 1, "k_split_emit<false>": 14, "k_stride_sums<T>": 1, "k_write_slot": 1,
        },
        "rate/decompress": {
            "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<1, true>)": 4, "k_dec_count": 72, "k_dec_header": 4,
            "k_dec_live": 8, "k_dec_load_words": 4, "k_dec_plane_end": 72, "k_dec_scan": 72, "k_gather_heads": 1,
            "k_leaf_apply": 72, "k_lip_apply<uint32_t>": 72, "k_lip_deposit": 72, "k_lip_scan": 72,
            "k_lip_words": 72, "k_lis_compact": 72, "k_lis_hi<uint32_t>": 72, "k_lis_l0": 72, "k_lis_l1": 72,
            "k_lis_l2": 72, "k_place_scan": 72, "k_place_scatter": 72, "k_ref_assemble": 4, "k_ref_deposit": 72,
        },
        "psnr/compress": {
            "(k_lift_axis<true, 0>)": 3, "(k_lift_xyz_fwd<1>)": 1, "k_born_place": 14, "k_bucket_scan": 1,
            "k_census": 1, "k_census_scan": 1, "k_chain": 4, "k_container_header": 1, "k_copy_slots": 1,
            "k_emit_pixels<uint32_t>": 1, "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1,
            "k_enc_state_init": 1, "k_list_apply": 14, "k_list_count": 14, "k_list_scan": 14, "k_make_q_rate": 1,
            "k_mask_scan": 14, "k_mean_finalize<T>": 1, "k_mse_final": 1, "k_mse_strides": 1, "k_plane_turn": 16,
            "k_pyramid<false>": 4, "k_quantize4": 1, "k_split_emit<false>": 14, "k_stride_sums<T>": 1,
            "k_write_slot": 1,
        },
        "psnr/decompress": {
            "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<1, true>)": 4, "k_dec_count": 56, "k_dec_header": 4,
            "k_dec_load_words": 4, "k_dec_plane_end": 56, "k_dec_scan": 56, "k_gather_heads": 1,
            "k_leaf_apply": 56, "k_lip_apply<uint32_t>": 56, "k_lip_deposit": 56, "k_lip_scan": 56,
            "k_lip_words": 56, "k_lis_compact": 56, "k_lis_hi<uint32_t>": 56, "k_lis_l0": 56, "k_lis_l1": 56,
            "k_lis_l2": 56, "k_place_scan": 56, "k_place_scatter": 56, "k_ref_assemble": 4, "k_ref_deposit": 56,
        },
        "pwe/compress": {
            "(k_lift_axis<false, 0>)": 3, "(k_lift_axis<true, 0>)": 3, "(k_lift_xyz_fwd<1>)": 1,
            "(k_lift_xyz_inv<2, false>)": 1, "(k_outlier_scan<T, 0>)": 1, "(k_outlier_scan<T, 1>)": 1,
            "(k_outlier_scan<T, 2>)": 1, "k_born_place": 14, "k_bucket_scan": 1, "k_census": 1, "k_census_scan": 1,
            "k_chain": 4, "k_container_header": 1, "k_copy_slots": 1, "k_copy_slots2": 1,
            "k_emit_pixels<uint32_t>": 1, "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1,
            "k_enc_state_init": 1, "k_list_apply": 14, "k_list_count": 14, "k_list_scan": 14, "k_make_q_rate": 1,
            "k_mask_scan": 14, "k_mean_finalize<T>": 1, "k_outlier_prefix": 1, "k_outlier_stream_out": 1,
            "k_plane_turn": 16, "k_pyramid<false>": 4, "k_quantize4": 1, "k_speck1d<true>": 1,
            "k_split_emit<false>": 14, "k_stride_sums<T>": 1, "k_write_slot": 1,
        },
        "pwe/decompress": {
            "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<2, true>)": 4, "k_dec_count": 55, "k_dec_header": 4,
            "k_dec_load_words": 4, "k_dec_plane_end": 55, "k_dec_scan": 55, "k_gather_heads": 2,
            "k_leaf_apply": 55, "k_lip_apply<uint32_t>": 55, "k_lip_deposit": 55, "k_lip_scan": 55,
            "k_lip_words": 55, "k_lis_compact": 55, "k_lis_hi<uint32_t>": 55, "k_lis_l0": 55, "k_lis_l1": 55,
            "k_lis_l2": 55, "k_outlier_apply": 4, "k_outlier_stream_in": 4, "k_place_scan": 55,
            "k_place_scatter": 55, "k_ref_assemble": 4, "k_ref_deposit": 55, "k_scatter_uncondition<T>": 4,
            "k_speck1d<false>": 4,
        },
    },
    "cubes_level2": {
        "rate/compress": {
            "(k_lift_xyz_fwd<1>)": 1, "k_born_place": 14, "k_bucket_scan": 1, "k_census": 1, "k_census_scan": 1,
            "k_chain": 4, "k_container_header": 1, "k_copy_slots": 1, "k_emit_pixels<uint32_t>": 1,
            "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1, "k_enc_state_init": 1,
            "k_lift2_fwd": 1, "k_list_apply": 14, "k_list_count": 14, "k_list_scan": 14, "k_make_q_rate": 1,
            "k_mask_scan": 14, "k_mean_finalize<T>": 1, "k_plane_turn": 16, "k_pyramid<false>": 4,
            "k_quantize4": 1, "k_split_emit<false>": 14, "k_stride_sums<T>": 1, "k_write_slot": 1,
        },
        "rate/decompress": {
            "(k_lift2_inv<true>)": 4, "(k_lift_xyz_inv<1, true>)": 4, "k_dec_count": 72, "k_dec_header": 4,
            "k_dec_live": 8, "k_dec_load_words": 4, "k_dec_plane_end": 72, "k_dec_scan": 72, "k_gather_heads": 1,
            "k_leaf_apply": 72, "k_lip_apply<uint32_t>": 72, "k_lip_deposit": 72, "k_lip_scan": 72,
            "k_lip_words": 72, "k_lis_compact": 72, "k_lis_hi<uint32_t>": 72, "k_lis_l0": 72, "k_lis_l1": 72,
            "k_lis_l2": 72, "k_place_scan": 72, "k_place_scatter": 72, "k_ref_assemble": 4, "k_ref_deposit": 72,
        },
        "psnr/compress": {
            "(k_lift_xyz_fwd<1>)": 1, "k_born_place": 14, "k_bucket_scan": 1, "k_census": 1, "k_census_scan": 1,
            "k_chain": 4, "k_container_header": 1, "k_copy_slots": 1, "k_emit_pixels<uint32_t>": 1,
            "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1, "k_enc_state_init": 1,
            "k_lift2_fwd": 1, "k_list_apply": 14, "k_list_count": 14, "k_list_scan": 14, "k_make_q_rate": 1,
            "k_mask_scan": 14, "k_mean_finalize<T>": 1, "k_mse_final": 1, "k_mse_strides": 1, "k_plane_turn": 16,
            "k_pyramid<false>": 4, "k_quantize4": 1, "k_split_emit<false>": 14, "k_stride_sums<T>": 1,
            "k_write_slot": 1,
        },
        "psnr/decompress": {
            "(k_lift2_inv<true>)": 4, "(k_lift_xyz_inv<1, true>)": 4, "k_dec_count": 56, "k_dec_header": 4,
            "k_dec_load_words": 4, "k_dec_plane_end": 56, "k_dec_scan": 56, "k_gather_heads": 1,
            "k_leaf_apply": 56, "k_lip_apply<uint32_t>": 56, "k_lip_deposit": 56, "k_lip_scan": 56,
            "k_lip_words": 56, "k_lis_compact": 56, "k_lis_hi<uint32_t>": 56, "k_lis_l0": 56, "k_lis_l1": 56,
            "k_lis_l2": 56, "k_place_scan": 56, "k_place_scatter": 56, "k_ref_assemble": 4, "k_ref_deposit": 56,
        },
        "pwe/compress": {
            "(k_lift_axis<false, 0>)": 3, "(k_lift_xyz_fwd<1>)": 1, "(k_lift_xyz_inv<2, false>)": 1,
            "(k_outlier_scan<T, 0>)": 1, "(k_outlier_scan<T, 1>)": 1, "(k_outlier_scan<T, 2>)": 1,
            "k_born_place": 14, "k_bucket_scan": 1, "k_census": 1, "k_census_scan": 1, "k_chain": 4,
            "k_container_header": 1, "k_copy_slots": 1, "k_copy_slots2": 1, "k_emit_pixels<uint32_t>": 1,
            "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1, "k_enc_state_init": 1,
            "k_lift2_fwd": 1, "k_list_apply": 14, "k_list_count": 14, "k_list_scan": 14, "k_make_q_rate": 1,
            "k_mask_scan": 14, "k_mean_finalize<T>": 1, "k_outlier_prefix": 1, "k_outlier_stream_out": 1,
            "k_plane_turn": 16, "k_pyramid<false>": 4, "k_quantize4": 1, "k_speck1d<true>": 1,
            "k_split_emit<false>": 14, "k_stride_sums<T>": 1, "k_write_slot": 1,
        },
        "pwe/decompress": {
            "(k_lift_axis<false, 0>)": 12, "(k_lift_xyz_inv<2, true>)": 4, "k_dec_count": 55, "k_dec_header": 4,
            "k_dec_load_words": 4, "k_dec_plane_end": 55, "k_dec_scan": 55, "k_gather_heads": 2,
            "k_leaf_apply": 55, "k_lip_apply<uint32_t>": 55, "k_lip_deposit": 55, "k_lip_scan": 55,
            "k_lip_words": 55, "k_lis_compact": 55, "k_lis_hi<uint32_t>": 55, "k_lis_l0": 55, "k_lis_l1": 55,
            "k_lis_l2": 55, "k_outlier_apply": 4, "k_outlier_stream_in": 4, "k_place_scan": 55,
            "k_place_scatter": 55, "k_ref_assemble": 4, "k_ref_deposit": 55, "k_scatter_uncondition<T>": 4,
            "k_speck1d<false>": 4,
        },
    },
    "one_level": {
        "pwe/compress": {
            "(k_lift_xyz_fwd<1>)": 1, "(k_lift_xyz_inv<2, false>)": 1, "(k_outlier_scan<T, 0>)": 1,
            "(k_outlier_scan<T, 1>)": 1, "(k_outlier_scan<T, 2>)": 1, "k_born_place": 12, "k_bucket_scan": 1,
            "k_census": 1, "k_census_scan": 1, "k_chain": 3, "k_container_header": 1, "k_copy_slots": 1,
            "k_copy_slots2": 1, "k_emit_pixels<uint32_t>": 1, "k_enc_bound": 1, "k_enc_finalize": 1,
            "k_enc_planes_setup": 1, "k_enc_state_init": 1, "k_list_apply": 12, "k_list_count": 12,
            "k_list_scan": 12, "k_make_q_rate": 1, "k_mask_scan": 12, "k_mean_finalize<T>": 1,
            "k_outlier_prefix": 1, "k_outlier_stream_out": 1, "k_plane_turn": 14, "k_pyramid<false>": 3,
            "k_quantize4": 1, "k_speck1d<true>": 1, "k_split_emit<false>": 12, "k_stride_sums<T>": 1,
            "k_write_slot": 1,
        },
        "pwe/decompress": {
            "(k_lift_xyz_inv<2, true>)": 4, "k_dec_count": 48, "k_dec_header": 4, "k_dec_load_words": 4,
            "k_dec_plane_end": 48, "k_dec_scan": 48, "k_gather_heads": 2, "k_leaf_apply": 48,
            "k_lip_apply<uint32_t>": 48, "k_lip_deposit": 48, "k_lip_scan": 48, "k_lip_words": 48,
            "k_lis_compact": 48, "k_lis_hi<uint32_t>": 48, "k_lis_l0": 48, "k_lis_l1": 48, "k_lis_l2": 48,
            "k_outlier_apply": 4, "k_outlier_stream_in": 4, "k_place_scan": 48, "k_place_scatter": 48,
            "k_ref_assemble": 4, "k_ref_deposit": 48, "k_scatter_uncondition<T>": 4, "k_speck1d<false>": 4,
        },
    },
    "packet": {
        "pwe/compress": {
            "(k_lift_axis<false, 0>)": 2, "(k_lift_axis<true, 0>)": 1, "(k_lift_axis<true, 1>)": 1,
            "(k_outlier_scan<T, 0>)": 1, "(k_outlier_scan<T, 1>)": 1, "(k_outlier_scan<T, 2>)": 1,
            "k_born_place": 11, "k_bucket_scan": 1, "k_census": 1, "k_census_scan": 1, "k_chain": 5,
            "k_container_header": 1, "k_copy_slots": 1, "k_copy_slots2": 1, "k_emit_pixels<uint32_t>": 1,
            "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1, "k_enc_state_init": 1,
            "k_inv_quantize<uint32_t>": 1, "k_inv_quantize<uint64_t>": 1, "k_list_apply": 11, "k_list_count": 11,
            "k_list_scan": 11, "k_make_q_rate": 1, "k_mask_scan": 11, "k_mean_finalize<T>": 1,
            "k_outlier_prefix": 1, "k_outlier_stream_out": 1, "k_plane_turn": 13, "k_pyramid<true>": 5,
            "k_quantize<uint32_t>": 1, "k_speck1d<true>": 1, "k_split_emit<true>": 11, "k_stride_sums<T>": 1,
            "k_write_slot": 1,
        },
        "pwe/decompress": {
            "(k_lift_axis<false, 0>)": 2, "k_dec_count": 11, "k_dec_header": 1, "k_dec_load_words": 1,
            "k_dec_plane_end": 11, "k_dec_scan": 11, "k_gather_heads": 2, "k_leaf_apply": 11,
            "k_lip_apply<uint32_t>": 11, "k_lip_deposit": 11, "k_lip_scan": 11, "k_lip_words": 11,
            "k_lis_compact": 11, "k_lis_mx<false>": 11, "k_outlier_apply": 1, "k_outlier_stream_in": 1,
            "k_place_scan": 11, "k_place_scatter": 11, "k_ref_assemble": 1, "k_ref_deposit": 11,
            "k_scatter_uncondition<T>": 1, "k_speck1d<false>": 1,
        },
    },
    "long_rows": {
        "pwe/compress": {
            "(k_lift_axis<false, 0>)": 6, "(k_lift_axis<true, 0>)": 4, "(k_lift_xy<true, 1>)": 1,
            "(k_outlier_scan<T, 0>)": 1, "(k_outlier_scan<T, 1>)": 1, "(k_outlier_scan<T, 2>)": 1,
            "k_born_place": 14, "k_bucket_scan": 1, "k_census": 1, "k_census_scan": 1, "k_chain": 8,
            "k_container_header": 1, "k_copy_slots": 1, "k_copy_slots2": 1, "k_emit_pixels<uint32_t>": 1,
            "k_enc_bound": 1, "k_enc_finalize": 1, "k_enc_planes_setup": 1, "k_enc_state_init": 1,
            "k_inv_quantize<uint32_t>": 1, "k_inv_quantize<uint64_t>": 1, "k_list_apply": 14, "k_list_count": 14,
            "k_list_scan": 14, "k_make_q_rate": 1, "k_mask_scan": 14, "k_mean_finalize<T>": 1,
            "k_outlier_prefix": 1, "k_outlier_stream_out": 1, "k_plane_turn": 16, "k_pyramid<true>": 8,
            "k_quantize4": 1, "k_speck1d<true>": 1, "k_split_emit<true>": 14, "k_stride_sums<T>": 1,
            "k_write_slot": 1,
        },
        "pwe/decompress": {
            "(k_lift_axis<false, 0>)": 6, "k_dec_count": 14, "k_dec_header": 1, "k_dec_load_words": 1,
            "k_dec_plane_end": 14, "k_dec_scan": 14, "k_gather_heads": 2, "k_leaf_apply": 14,
            "k_lip_apply<uint32_t>": 14, "k_lip_deposit": 14, "k_lip_scan": 14, "k_lip_words": 14,
            "k_lis_compact": 14, "k_lis_mx<false>": 14, "k_outlier_apply": 1, "k_outlier_stream_in": 1,
            "k_place_scan": 14, "k_place_scatter": 14, "k_ref_assemble": 1, "k_ref_deposit": 14,
            "k_scatter_uncondition<T>": 1, "k_speck1d<false>": 1,
        },
    },
    "wide": {
        "psnr/compress": {
            "(k_lift_axis<true, 0>)": 6, "(k_lift_xyz_fwd<1>)": 2, "k_born_place": 40, "k_bucket_scan": 2,
            "k_census": 2, "k_census_scan": 2, "k_chain": 8, "k_container_header": 1, "k_copy_slots": 1,
            "k_emit_pixels<uint32_t>": 1, "k_emit_pixels<uint64_t>": 1, "k_enc_bound": 2, "k_enc_finalize": 2,
            "k_enc_planes_setup": 2, "k_enc_state_init": 2, "k_list_apply": 40, "k_list_count": 40,
            "k_list_scan": 40, "k_make_q_rate": 1, "k_mark_wide": 1, "k_mask_scan": 40, "k_mean_finalize<T>": 2,
            "k_mse_final": 1, "k_mse_strides": 1, "k_plane_turn": 44, "k_pyramid<false>": 8, "k_quantize4": 1,
            "k_quantize<uint64_t>": 1, "k_split_emit<false>": 40, "k_stride_sums<T>": 2, "k_write_slot": 2,
        },
        "psnr/decompress": {
            "(k_lift_axis<false, 0>)": 3, "(k_lift_xyz_inv<1, false>)": 1, "k_dec_count": 39, "k_dec_header": 2,
            "k_dec_live": 12, "k_dec_load_words": 2, "k_dec_plane_end": 39, "k_dec_scan": 39, "k_gather_heads": 1,
            "k_inv_quantize<uint64_t>": 1, "k_leaf_apply": 39, "k_lip_apply<uint64_t>": 39, "k_lip_deposit": 39,
            "k_lip_scan": 39, "k_lip_words": 39, "k_lis_compact": 39, "k_lis_hi<uint64_t>": 39, "k_lis_l0": 39,
            "k_lis_l1": 39, "k_lis_l2": 39, "k_place_scan": 39, "k_place_scatter": 39,
            "k_ref_apply2<uint64_t>": 39,
        },
        "pwe/compress": {
            "(k_lift_axis<false, 0>)": 6, "(k_lift_axis<true, 0>)": 3, "(k_lift_xyz_fwd<1>)": 1,
            "(k_outlier_scan<T, 0>)": 1, "(k_outlier_scan<T, 1>)": 1, "(k_outlier_scan<T, 2>)": 1,
            "k_born_place": 47, "k_bucket_scan": 2, "k_census": 2, "k_census_scan": 2, "k_chain": 8,
            "k_container_header": 1, "k_copy_slots": 1, "k_copy_slots2": 1, "k_emit_pixels<uint32_t>": 1,
            "k_emit_pixels<uint64_t>": 1, "k_enc_bound": 2, "k_enc_finalize": 2, "k_enc_planes_setup": 2,
            "k_enc_state_init": 2, "k_inv_quantize<uint32_t>": 1, "k_inv_quantize<uint64_t>": 1,
            "k_list_apply": 47, "k_list_count": 47, "k_list_scan": 47, "k_make_q_rate": 1, "k_mark_wide": 1,
            "k_mask_scan": 47, "k_mean_finalize<T>": 1, "k_outlier_prefix": 1, "k_outlier_stream_out": 1,
            "k_plane_turn": 51, "k_pyramid<false>": 8, "k_quantize4": 1, "k_quantize<uint64_t>": 1,
            "k_speck1d<true>": 1, "k_split_emit<false>": 47, "k_stride_sums<T>": 1, "k_write_slot": 2,
        },
        "pwe/decompress": {
            "(k_lift_axis<false, 0>)": 6, "k_dec_count": 46, "k_dec_header": 2, "k_dec_live": 15,
            "k_dec_load_words": 2, "k_dec_plane_end": 46, "k_dec_scan": 46, "k_gather_heads": 2,
            "k_inv_quantize<uint64_t>": 1, "k_leaf_apply": 46, "k_lip_apply<uint64_t>": 46, "k_lip_deposit": 46,
            "k_lip_scan": 46, "k_lip_words": 46, "k_lis_compact": 46, "k_lis_hi<uint64_t>": 46, "k_lis_l0": 46,
            "k_lis_l1": 46, "k_lis_l2": 46, "k_outlier_apply": 1, "k_outlier_stream_in": 1, "k_place_scan": 46,
            "k_place_scatter": 46, "k_ref_apply2<uint64_t>": 46, "k_scatter_uncondition<T>": 1,
            "k_speck1d<false>": 1,
        },
    },
}


@pytest.mark.parametrize("name", list(CASES))
def test_calls_launch_what_the_parent_launched(eng, oracle, name):
    got = collect(eng, oracle, name)
    for call, rep in got.items():
        print(name, call, sum(rep.values()), rep)
    assert got == PARENT_LAUNCHES[name]
    if name == "cubes_level2":   # the walks take the level-2 launch, the brick inverses never do
        assert got["pwe/compress"].get("k_lift2_fwd", 0) > 0 and not any("k_lift2_inv" in k for k in got["pwe/compress"])
        assert not any("k_lift2_inv" in k for k in got["pwe/decompress"])
        assert any("k_lift2_inv" in k for k in got["rate/decompress"])
