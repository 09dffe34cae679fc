"""waifu2x-converter-cpp_amd -- host-side mirror of the reference's hot-path interface over the
C ABI of lib/libw2xc_hip.so (include/w2xc_hip.h).

The directory name is not a Python identifier; load it with ``__graft_entry__.load_package()``
(registers it as module ``w2xc_amd``).

Names follow /root/reference/src/modelHandler.hpp and convertRoutine.hpp:

    models = []
    modelUtility.generateModelFromJSON("models/scale2.0x_model.json", models)   # modelHandler.cpp:170
    modelUtility.getInstance().setNumberOfJobs(4)                               # :199
    out = Mat()
    ok = convertWithModels(Mat(y_plane), out, models)                           # convertRoutine.cpp:21
    ok = models[0].filter(inputPlanes, outputPlanes)                            # modelHandler.cpp:26

``Mat`` is a minimal stand-in for a CV_32FC1 ``cv::Mat`` (a float32 numpy view, may be a strided
ROI).  All arithmetic happens in the HIP library; there is no CPU fallback -- if the shared
library is missing the import fails, and without a GPU every compute call returns ``False`` /
raises ``W2xcError``.  PyTorch is only used by callers for device memory and streams.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libw2xc_hip.so")

OK, ERR_IO, ERR_JSON, ERR_ARG, ERR_PLANES, ERR_HIP, ERR_UNSUPPORTED, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6, -7
PRECISION_FP32, PRECISION_BF16, PRECISION_BF16X2, PRECISION_BF16X3, PRECISION_FP16X2 = 0, 1, 2, 3, 4
KERNEL_AUTO, KERNEL_DIRECT, KERNEL_MFMA, KERNEL_WINOGRAD, KERNEL_WINOGRAD32, KERNEL_WINOGRAD4 = 0, 1, 2, 3, 4, 5
FUSION_AUTO, FUSION_OFF, FUSION_ON, FUSION_FIRST, FUSION_LAST, FUSION_GATHER_LAUNCH, FUSION_PROG = 0, 1, 2, 3, 4, 5, 6
YUV_420, YUV_422, YUV_444, YUV_400 = 0, 1, 2, 3
# chroma siting ("Chroma siting", include/w2xc_hip.h): flags or-ed onto a layout -- along x / y a chroma sample sits ON luma column / row 2k
CHROMA_COSITED_X, CHROMA_COSITED_Y = 0x10, 0x20
YUV_420_LEFT, YUV_420_TOPLEFT, YUV_422_LEFT = YUV_420 | CHROMA_COSITED_X, YUV_420 | CHROMA_COSITED_X | CHROMA_COSITED_Y, YUV_422 | CHROMA_COSITED_X
RANGE_FULL, RANGE_LIMITED = 0, 1
MATRIX_BT601, MATRIX_BT709, MATRIX_BT2020 = 0, 1, 2
PACK_LOW, PACK_HIGH = 0, 1
# "Sized YUV frames": iterations = the smallest k with (w << k) >= out_w and (h << k) >= out_h (W2XC_ITERATIONS_AUTO)
ITERATIONS_AUTO = -1


class W2xcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("w2xc error %d: %s" % (code, msg))
        self.code = code


class Opts(C.Structure):
    """struct w2xc_opts (include/w2xc_hip.h)."""
    _fields_ = [("struct_size", C.c_int), ("precision", C.c_int), ("kernel", C.c_int), ("device", C.c_int),
                ("device_mask", C.c_uint), ("band_rows", C.c_int), ("workspace_mb", C.c_int),
                ("profile", C.c_int), ("verbose", C.c_int), ("filter_resident", C.c_int), ("fusion", C.c_int),
                ("host_units", C.c_int), ("host_chunk_kb", C.c_int), ("host_numa", C.c_int)]


class RowPlan(C.Structure):
    """struct w2xc_row_plan (include/w2xc_hip.h): the band geometry of one row-range conversion."""
    _fields_ = [("struct_size", C.c_int), ("n_layers", C.c_int), ("halo_rows_per_layer", C.c_int), ("band_rows", C.c_int),
                ("n_bands", C.c_int), ("fused_first", C.c_int), ("fused_last", C.c_int), ("workspace_bytes", C.c_ulonglong * 2)]


class YuvPlanes(C.Structure):
    """struct w2xc_yuv_planes (include/w2xc_hip.h): one side of a YUV frame call -- n frames, pointers as integers, strides in bytes; c_px = 1: planar
    chroma, 2: two interleaved planes (NV12: v = u + 1)."""
    _fields_ = [("y", C.c_void_p), ("y_stride", C.c_size_t), ("y_frame_stride", C.c_size_t), ("u", C.c_void_p), ("v", C.c_void_p),
                ("c_stride", C.c_size_t), ("c_frame_stride", C.c_size_t), ("c_px", C.c_int)]


class Yuv16Planes(C.Structure):
    """struct w2xc_yuv16_planes (include/w2xc_hip.h): one side of a 16-bit YUV frame call -- YuvPlanes with pointers to 16-bit words (even), strides in bytes
    (even), c_px in samples (2: P010, v = u + 2 bytes) and the packing of a value in its word (PACK_LOW / PACK_HIGH)."""
    _fields_ = YuvPlanes._fields_ + [("pack", C.c_int)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("HIP extension %s is missing -- build it with __graft_entry__.build() "
                          "(make -C waifu2x-converter-cpp_amd/csrc). There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  Callers use torch for device memory and
    # streams, so let torch's copy load first: libw2xc_hip.so then binds to the same (single) HIP runtime
    # and device pointers / streams can be shared.  Without torch the system ROCm runtime is used.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:   # torch is plumbing, not a requirement
            pass
    lib = C.CDLL(LIB_PATH)
    vp, ci, cs, fp = C.c_void_p, C.c_int, C.c_size_t, C.c_void_p
    sig = {
        "w2xc_opts_init": (None, [C.POINTER(Opts)]),
        "w2xc_opts_init_sized": (None, [C.POINTER(Opts), cs]),
        "w2xc_set_default_opts": (ci, [C.POINTER(Opts)]),
        "w2xc_plan_rows": (ci, [vp, ci, ci, ci, ci, ci, ci, C.POINTER(Opts), C.POINTER(RowPlan)]),
        "w2xc_plan_region": (ci, [C.POINTER(RowPlan), ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]),
        "w2xc_model_load_json": (ci, [C.c_char_p, C.POINTER(vp)]),
        "w2xc_model_from_arrays": (ci, [ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "w2xc_model_add_upconv_head": (ci, [vp, ci, fp, fp]),
        "w2xc_model_has_head": (ci, [vp]),
        "w2xc_model_free": (None, [vp]),
        "w2xc_model_trim": (ci, [vp]),
        "w2xc_model_layers": (ci, [vp]),
        "w2xc_model_nin": (ci, [vp, ci]),
        "w2xc_model_nout": (ci, [vp, ci]),
        "w2xc_model_get_layer": (ci, [vp, ci, fp, fp]),
        "w2xc_set_jobs": (ci, [ci]),
        "w2xc_get_jobs": (ci, []),
        "w2xc_set_block_size": (ci, [ci, ci]),
        "w2xc_set_block_size_exp2": (ci, [ci]),
        "w2xc_get_block_size": (None, [C.POINTER(ci), C.POINTER(ci)]),
        "w2xc_convert_plane": (ci, [vp, fp, cs, ci, ci, fp, cs, ci, C.POINTER(Opts)]),
        "w2xc_convert_plane_device": (ci, [vp, fp, cs, ci, ci, fp, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_planes_device": (ci, [vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_process_image_u8_ex_device": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, vp, C.POINTER(Opts)]),
        "w2xc_process_image_u8_ex": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, C.POINTER(Opts)]),
        "w2xc_process_image_u8_batch_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, vp, C.POINTER(Opts)]),
        "w2xc_process_image_u8_batch": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, C.POINTER(Opts)]),
        "w2xc_process_image_rgb_u8_ex_device": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, vp, C.POINTER(Opts)]),
        "w2xc_process_image_rgb_u8_ex": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, C.POINTER(Opts)]),
        "w2xc_process_image_rgb_u8_batch_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, vp, C.POINTER(Opts)]),
        "w2xc_process_image_rgb_u8_batch": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, C.POINTER(Opts)]),
        "w2xc_process_image_rgba_u8_ex_device": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, ci, vp, C.POINTER(Opts)]),
        "w2xc_process_image_rgba_u8_ex": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, ci, C.POINTER(Opts)]),
        "w2xc_process_image_rgba_u8_batch_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, ci, vp, C.POINTER(Opts)]),
        "w2xc_process_image_rgba_u8_batch": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, ci, C.POINTER(Opts)]),
        "w2xc_process_image_u8_tta_device": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_u8_tta": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, C.POINTER(Opts), ci]),
        "w2xc_process_image_u8_batch_tta_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_u8_batch_tta": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgb_u8_tta_device": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgb_u8_tta": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.c_double, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgb_u8_batch_tta_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgb_u8_batch_tta": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, C.POINTER(Opts), ci]),
        "w2xc_convert_batch_tta_device": (ci, [vp, ci, ci, fp, cs, cs, ci, ci, fp, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_planes_tta_device": (ci, [vp, ci, ci, fp, cs, cs, ci, ci, fp, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_tta_spread_device": (ci, [fp, ci, cs, cs, ci, ci, fp, fp, cs, vp]),
        "w2xc_tta_gather_device": (ci, [fp, fp, cs, ci, ci, ci, fp, cs, cs, vp]),
        "w2xc_bleed_rgba_u8_device": (ci, [fp, cs, ci, ci, ci, fp, cs, vp]),
        "w2xc_bleed_rgba_u8_trim": (ci, []),
        "w2xc_convert_planes_nn2x_device": (ci, [vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_planes_up2x_device": (ci, [vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_planes_up2x_batch_device": (ci, [vp, ci, ci, fp, cs, cs, cs, ci, ci, fp, cs, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_process_image_rgb_u8_up2x_batch_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgb_u8_up2x_batch": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgba_u8_up2x_batch_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, ci, vp, C.POINTER(Opts)]),
        "w2xc_process_image_rgba_u8_up2x_batch": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, ci, C.POINTER(Opts)]),
        "w2xc_process_image_rgba_u8_batch_tta_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, ci, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgba_u8_batch_tta": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, ci, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgba_u8_up2x_batch_tta_device": (ci, [vp, vp, ci, fp, cs, cs, ci, ci, fp, cs, cs, ci, C.c_double, ci, vp, C.POINTER(Opts), ci]),
        "w2xc_process_image_rgba_u8_up2x_batch_tta": (ci, [vp, vp, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, ci, C.c_double, ci, C.POINTER(Opts), ci]),
        "w2xc_tta_spread_u8_device": (ci, [fp, ci, cs, cs, ci, ci, ci, ci, ci, fp, fp, cs, vp]),
        "w2xc_tta_gather_u8_device": (ci, [fp, fp, cs, ci, ci, ci, ci, ci, ci, fp, cs, cs, ci, ci, vp]),
        "w2xc_process_frames_yuv_u8_device": (ci, [vp, vp, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), C.POINTER(YuvPlanes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), C.POINTER(YuvPlanes), ci, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u8_rgb_device": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), C.POINTER(YuvPlanes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u8_rgb": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), C.POINTER(YuvPlanes), ci, C.POINTER(Opts)]),
        "w2xc_yuv8_to_rgb_device": (ci, [C.POINTER(YuvPlanes), ci, ci, ci, ci, ci, ci, fp, cs, cs, vp]),
        "w2xc_rgb_to_yuv8_device": (ci, [fp, cs, cs, ci, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), vp]),
        "w2xc_process_frames_yuv_u16_device": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), C.POINTER(Yuv16Planes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), C.POINTER(Yuv16Planes), ci, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16_rgb_device": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), C.POINTER(Yuv16Planes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16_rgb": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), C.POINTER(Yuv16Planes), ci, C.POINTER(Opts)]),
        "w2xc_yuv16_to_rgb_device": (ci, [C.POINTER(Yuv16Planes), ci, ci, ci, ci, ci, ci, ci, fp, cs, cs, vp]),
        "w2xc_rgb_to_yuv16_device": (ci, [fp, cs, cs, ci, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), vp]),
        "w2xc_y16_to_plane_device": (ci, [fp, ci, cs, cs, ci, ci, ci, ci, ci, fp, cs, vp]),
        "w2xc_plane_to_y16_device": (ci, [fp, ci, cs, ci, ci, ci, ci, ci, fp, cs, cs, vp]),
        "w2xc_chroma2x_u16_device": (ci, [fp, ci, cs, cs, ci, ci, ci, ci, ci, fp, cs, cs, ci, ci, ci, ci, vp]),
        "w2xc_chroma2x_u16_sited_device": (ci, [fp, ci, cs, cs, ci, ci, ci, ci, ci, fp, cs, cs, ci, ci, ci, ci, ci, vp]),
        "w2xc_y8_to_plane_device": (ci, [fp, ci, cs, cs, ci, ci, ci, fp, cs, vp]),
        "w2xc_plane_to_y8_device": (ci, [fp, ci, cs, ci, ci, ci, fp, cs, cs, vp]),
        "w2xc_chroma2x_u8_device": (ci, [fp, ci, cs, cs, ci, ci, ci, fp, cs, cs, ci, ci, ci, vp]),
        "w2xc_chroma2x_u8_sited_device": (ci, [fp, ci, cs, cs, ci, ci, ci, fp, cs, cs, ci, ci, ci, ci, vp]),
        "w2xc_process_frames_yuv_u8_sized_device": (ci, [vp, vp, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), ci, ci, C.POINTER(YuvPlanes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u8_sized": (ci, [vp, vp, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), ci, ci, C.POINTER(YuvPlanes), ci, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u8_rgb_sized_device": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), ci, ci, C.POINTER(YuvPlanes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u8_rgb_sized": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(YuvPlanes), ci, ci, C.POINTER(YuvPlanes), ci, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16_sized_device": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), ci, ci, C.POINTER(Yuv16Planes), ci, vp, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16_sized": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), ci, ci, C.POINTER(Yuv16Planes), ci, C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16_rgb_sized_device": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), ci, ci, C.POINTER(Yuv16Planes), ci, vp,
                                                              C.POINTER(Opts)]),
        "w2xc_process_frames_yuv_u16_rgb_sized": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, C.POINTER(Yuv16Planes), ci, ci, C.POINTER(Yuv16Planes), ci, C.POINTER(Opts)]),
        "w2xc_chroma_resize_u8_device": (ci, [fp, ci, cs, cs, ci, ci, ci, fp, cs, cs, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]),
        "w2xc_chroma_resize_u16_device": (ci, [fp, ci, cs, cs, ci, ci, ci, ci, ci, fp, cs, cs, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]),
        "w2xc_u8_to_rgb_device": (ci, [fp, cs, ci, ci, fp, fp, fp, vp]),
        "w2xc_rgb_to_u8_device": (ci, [fp, fp, fp, ci, ci, fp, cs, vp]),
        "w2xc_process_image_u8_device": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, vp, C.POINTER(Opts)]),
        "w2xc_process_image_u8": (ci, [vp, vp, fp, cs, ci, ci, fp, cs, ci, C.POINTER(Opts)]),
        "w2xc_scale2x_image_u8_device": (ci, [vp, fp, cs, ci, ci, fp, cs, ci, vp, C.POINTER(Opts)]),
        "w2xc_scale2x_image_u8": (ci, [vp, fp, cs, ci, ci, fp, cs, ci, C.POINTER(Opts)]),
        "w2xc_resize2x_cubic_device": (ci, [fp, ci, ci, fp, vp]),
        "w2xc_resize_linear_device": (ci, [fp, ci, ci, fp, ci, ci, vp]),
        "w2xc_u8_to_yuv_device": (ci, [fp, cs, ci, ci, fp, fp, fp, vp]),
        "w2xc_yuv_to_u8_device": (ci, [fp, fp, fp, ci, ci, fp, cs, vp]),
        "w2xc_convert_plane_nn2x": (ci, [vp, fp, cs, ci, ci, fp, cs, C.POINTER(Opts)]),
        "w2xc_convert_plane_nn2x_device": (ci, [vp, fp, cs, ci, ci, fp, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_plane_rows": (ci, [vp, fp, cs, ci, ci, ci, ci, ci, ci, ci, fp, cs, C.POINTER(Opts)]),
        "w2xc_layer_filter_device": (ci, [vp, ci, ci, fp, C.c_longlong, C.c_longlong, C.c_longlong, ci, ci, fp, C.c_longlong,
                                          C.c_longlong, C.c_longlong, vp, C.POINTER(Opts)]),
        "w2xc_convert_rows_device": (ci, [vp, fp, cs, ci, ci, ci, ci, ci, ci, fp, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_batch_device": (ci, [vp, ci, ci, fp, cs, cs, ci, ci, fp, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_convert_planes_batch_device": (ci, [vp, ci, ci, ci, fp, cs, cs, cs, ci, ci, fp, cs, cs, cs, vp, C.POINTER(Opts)]),
        "w2xc_batch_plan": (ci, [vp, ci, ci, ci, ci, C.POINTER(Opts), C.POINTER(ci), C.POINTER(ci)]),
        "w2xc_convert_batch": (ci, [vp, ci, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, C.POINTER(Opts)]),
        "w2xc_layer_filter": (ci, [vp, ci, ci, C.POINTER(fp), cs, ci, ci, C.POINTER(fp), cs, C.POINTER(Opts)]),
        "w2xc_profile_read": (ci, [vp, ci, C.POINTER(C.c_float), C.POINTER(ci), ci]),
        "w2xc_profile_reset": (None, [vp, ci]),
        "w2xc_debug_fill_scratch": (ci, [vp, ci, C.c_uint, C.POINTER(C.c_ulonglong)]),
        "w2xc_debug_fail_nth": (C.c_longlong, [ci, C.c_longlong]),
        "w2xc_layer_kernel_name": (C.c_char_p, [vp, ci, C.POINTER(Opts)]),
        "w2xc_device_count": (ci, []),
        "w2xc_last_error": (C.c_char_p, []),
        "w2xc_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)   # AttributeError if the ABI lost a symbol
        f.restype = res
        f.argtypes = args
    return lib, tuple(sig)


_lib, ABI_SYMBOLS = _load()


def lib():
    return _lib


def last_error():
    return (_lib.w2xc_last_error() or b"").decode(errors="replace")


def device_count():
    return _lib.w2xc_device_count()


DEBUG_FAIL_ALLOC, DEBUG_FAIL_COPY, DEBUG_FAIL_LAUNCH = 1, 2, 3


def debug_fail_nth(kind, nth):
    """Test aid (w2xc_debug_fail_nth): the nth event of `kind` (DEBUG_FAIL_*) from now on fails once, on the host, in place of the runtime call; nth = 0
    disarms.  -> the events of that kind since the previous call with that kind; -1 for an unknown kind or a negative nth (nothing is armed)."""
    return int(_lib.w2xc_debug_fail_nth(int(kind), int(nth)))


def make_opts(**kw):
    o = Opts()
    _lib.w2xc_opts_init(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown w2xc_opts field %r" % k)
        setattr(o, k, v)
    return o


# ---------------------------------------------------------------------------------------------
class Mat:
    """Stand-in for a CV_32FC1 cv::Mat: wraps a 2-D float32 array whose rows are contiguous
    (row stride arbitrary, like a cv::Mat ROI with its ``step``)."""

    def __init__(self, array=None):
        self.array = None
        if array is not None:
            a = np.asarray(array)
            if a.dtype != np.float32 or a.ndim != 2:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.ndim != 2:
                    raise ValueError("Mat wants a 2-D plane")
            if a.strides[1] != 4:
                a = np.ascontiguousarray(a)
            self.array = a

    @property
    def rows(self):
        return 0 if self.array is None else self.array.shape[0]

    @property
    def cols(self):
        return 0 if self.array is None else self.array.shape[1]

    @property
    def step(self):
        return 0 if self.array is None else self.array.strides[0]

    def size(self):
        return (self.cols, self.rows)   # cv::Size(width, height)

    def create(self, rows, cols):
        if self.array is None or self.array.shape != (rows, cols):
            self.array = np.empty((rows, cols), np.float32)

    def copyTo(self, other):
        other.create(self.rows, self.cols)
        other.array[...] = self.array


class _ModelSet:
    """Owns one w2xc_model* (== the reference's std::vector<std::unique_ptr<Model>>)."""

    def __init__(self, handle):
        self.handle = C.c_void_p(handle)

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h and _lib is not None:
            _lib.w2xc_model_free(h)

    @classmethod
    def from_json(cls, path):
        h = C.c_void_p()
        rc = _lib.w2xc_model_load_json(os.fsencode(path), C.byref(h))
        if rc != OK:
            raise W2xcError(rc, last_error())
        return cls(h.value)

    @classmethod
    def from_layers(cls, layers, head=None):
        """layers: [(nin, nout, W[o,i,3,3] float32, bias[o] float64)]; head = (W[c,o,4,4] float32, bias[o] float64 or None): the 4x4 stride-2
        transposed-convolution head of an upconv model behind them (w2xc_model_add_upconv_head)"""
        n = len(layers)
        nin = (C.c_int * n)(*[l[0] for l in layers])
        nout = (C.c_int * n)(*[l[1] for l in layers])
        ws = [np.ascontiguousarray(l[2], dtype=np.float32) for l in layers]
        bs = [np.ascontiguousarray(l[3], dtype=np.float64) for l in layers]
        for (ni, no, _, _), w, b in zip(layers, ws, bs):
            if w.shape != (no, ni, 3, 3) or b.shape != (no,):
                raise ValueError("layer arrays have the wrong shape")
        wp = (C.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        h = C.c_void_p()
        rc = _lib.w2xc_model_from_arrays(n, nin, nout, wp, bp, C.byref(h))
        if rc != OK:
            raise W2xcError(rc, last_error())
        ms = cls(h.value)
        if head is not None:
            ms.add_upconv_head(*head)
        return ms

    def add_upconv_head(self, weight, bias=None):
        """append the head: weight [nin, nout, 4, 4] (nin = the last layer's output planes), bias [nout] or None = zeros"""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        # (a model that has its head already: the library refuses before it reads the weights)
        if not self.has_head and (w.ndim != 4 or w.shape[0] != self.planes(self.n_layers - 1)[1] or w.shape[2:] != (4, 4)):
            raise ValueError("head weight must be [nin, nout, 4, 4]")
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
        if b is not None and b.shape != (w.shape[1],):
            raise ValueError("head bias must be [nout]")
        rc = _lib.w2xc_model_add_upconv_head(self.handle, int(w.shape[1]), w.ctypes.data, None if b is None else b.ctypes.data)
        if rc != OK:
            raise W2xcError(rc, last_error())

    @property
    def has_head(self):
        return bool(_lib.w2xc_model_has_head(self.handle))

    def trim(self):
        """release the buffers that grew with the largest plane so far (w2xc_model_trim); weights stay resident"""
        rc = _lib.w2xc_model_trim(self.handle)
        if rc != OK:
            raise W2xcError(rc, last_error())

    @property
    def n_layers(self):
        return _lib.w2xc_model_layers(self.handle)

    def planes(self, l):
        return _lib.w2xc_model_nin(self.handle, l), _lib.w2xc_model_nout(self.handle, l)

    def layer_arrays(self, l):
        nin, nout = self.planes(l)
        head = self.has_head and l == self.n_layers - 1   # (the head's weight is [nin, nout, 4, 4])
        w = np.empty((nin, nout, 4, 4) if head else (nout, nin, 3, 3), np.float32)
        b = np.empty((nout,), np.float64)
        rc = _lib.w2xc_model_get_layer(self.handle, l, w.ctypes.data, b.ctypes.data)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return nin, nout, w, b

    # -- functional forms used by tests / bench ------------------------------------------------
    def convert(self, plane, block_splitting=True, opts=None):
        """convertWithModels on a host float32 plane -> new float32 plane (raises on failure)."""
        src = Mat(plane)
        out = np.empty((src.rows, src.cols), np.float32)
        rc = _lib.w2xc_convert_plane(self.handle, src.array.ctypes.data, src.step, src.cols, src.rows,
                                     out.ctypes.data, out.strides[0], int(block_splitting),
                                     C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return out

    def convert_planes_device(self, n_in, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                              out_plane_stride_bytes, out_stride_bytes, stream=0, opts=None):
        """Multi-plane wrapper (pad n / all layers / crop) on planar device planes; writes every plane of the
        last layer (w2xc_convert_planes_device)."""
        rc = _lib.w2xc_convert_planes_device(self.handle, n_in, C.c_void_p(d_in), in_plane_stride_bytes, in_stride_bytes, w, h,
                                             C.c_void_p(d_out), out_plane_stride_bytes, out_stride_bytes, C.c_void_p(stream),
                                             C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_planes_nn2x_device(self, n_in, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                                   out_plane_stride_bytes, out_stride_bytes, stream=0, opts=None):
        """convert_planes_device with the nearest-neighbour 2x folded into layer 1 (w2xc_convert_planes_nn2x_device): (w, h) is the
        source size, the output planes are 2w x 2h."""
        rc = _lib.w2xc_convert_planes_nn2x_device(self.handle, n_in, C.c_void_p(d_in), in_plane_stride_bytes, in_stride_bytes, w, h,
                                                  C.c_void_p(d_out), out_plane_stride_bytes, out_stride_bytes, C.c_void_p(stream),
                                                  C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_planes_up2x_device(self, n_in, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                                   out_plane_stride_bytes, out_stride_bytes, stream=0, opts=None):
        """an upconv head model on planar device planes (w2xc_convert_planes_up2x_device): (w, h) is the source size, every plane of the
        head comes out at 2w x 2h, unclipped"""
        rc = _lib.w2xc_convert_planes_up2x_device(self.handle, n_in, C.c_void_p(d_in), in_plane_stride_bytes, in_stride_bytes, w, h,
                                                  C.c_void_p(d_out), out_plane_stride_bytes, out_stride_bytes, C.c_void_p(stream),
                                                  C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def scale2x_image_u8(self, img, iterations=1, opts=None):
        """The CLI's scale phase on an h x w x 3 uint8 image (main.cpp:74-76,126-156,171-172) -> (h<<it) x (w<<it) x 3."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, ch = img.shape
        if ch != 3:
            raise ValueError("want h x w x 3 uint8")
        out = np.empty((h << iterations, w << iterations, 3), np.uint8)
        rc = _lib.w2xc_scale2x_image_u8(self.handle, img.ctypes.data, img.strides[0], w, h, out.ctypes.data, out.strides[0],
                                        iterations, C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return out

    def scale2x_image_u8_device(self, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations=1, stream=0, opts=None):
        rc = _lib.w2xc_scale2x_image_u8_device(self.handle, C.c_void_p(d_in), in_stride_bytes, w, h, C.c_void_p(d_out),
                                               out_stride_bytes, iterations, C.c_void_p(stream),
                                               C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_nn2x(self, plane, opts=None):
        """cv::resize(INTER_NEAREST, 2x) + convertWithModels (main.cpp:132-148) in one call: h x w -> 2h x 2w."""
        src = Mat(plane)
        out = np.empty((2 * src.rows, 2 * src.cols), np.float32)
        rc = _lib.w2xc_convert_plane_nn2x(self.handle, src.array.ctypes.data, src.step, src.cols, src.rows,
                                          out.ctypes.data, out.strides[0], C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return out

    def convert_nn2x_device(self, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, stream=0, opts=None):
        rc = _lib.w2xc_convert_plane_nn2x_device(self.handle, C.c_void_p(d_in), in_stride_bytes, w, h, C.c_void_p(d_out),
                                                 out_stride_bytes, C.c_void_p(stream), C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_device(self, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, stream=0, opts=None):
        """Device-pointer form (ints: hipDeviceptr / hipStream_t).  Asynchronous on `stream`."""
        rc = _lib.w2xc_convert_plane_device(self.handle, C.c_void_p(d_in), in_stride_bytes, w, h,
                                            C.c_void_p(d_out), out_stride_bytes, C.c_void_p(stream),
                                            C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_batch(self, planes, nn2x=False, opts=None, out=None):
        """n host planes of one size in one call (w2xc_convert_batch): `planes` is a list of h x w float32 planes or an (n, h, w) array; returns
        an (n, h << nn2x, w << nn2x) float32 array (or fills `out`, such an array).  Plane i is bit-identical to convert[_nn2x](planes[i])."""
        up = 1 if nn2x else 0
        if isinstance(planes, np.ndarray):
            if planes.ndim != 3:
                raise ValueError("convert_batch wants an (n, h, w) array or a list of h x w planes")
            planes = [planes[i] for i in range(planes.shape[0])]
        srcs = [Mat(p).array for p in planes]
        if not srcs:
            raise ValueError("convert_batch wants at least one plane")
        h, w = srcs[0].shape
        if any(a.shape != (h, w) for a in srcs):
            raise ValueError("convert_batch: every plane must have the same size (group planes by size)")
        if len({a.strides[0] for a in srcs}) != 1:
            srcs = [np.ascontiguousarray(a) for a in srcs]
        n = len(srcs)
        if out is None:
            out = np.empty((n, h << up, w << up), np.float32)
        elif out.shape != (n, h << up, w << up) or out.dtype != np.float32 or out.strides[2] != 4:
            raise ValueError("convert_batch: `out` must be a float32 (n, h', w') array with contiguous rows")
        ip = (C.c_void_p * n)(*[a.ctypes.data for a in srcs])
        op = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        rc = _lib.w2xc_convert_batch(self.handle, n, up, ip, srcs[0].strides[0], w, h, op, out.strides[1],
                                     C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return out

    def convert_batch_device(self, n, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes,
                             out_stride_bytes, nn2x=False, stream=0, opts=None):
        """Device-pointer batch (w2xc_convert_batch_device): n planes of w x h at d_in + i * in_plane_stride_bytes, outputs
        (w << nn2x) x (h << nn2x) at d_out + i * out_plane_stride_bytes.  Asynchronous on `stream`."""
        rc = _lib.w2xc_convert_batch_device(self.handle, n, 1 if nn2x else 0, C.c_void_p(d_in), in_plane_stride_bytes, in_stride_bytes, w, h,
                                            C.c_void_p(d_out), out_plane_stride_bytes, out_stride_bytes, C.c_void_p(stream),
                                            C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_planes_batch_device(self, n, n_in, d_in, in_image_stride_bytes, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                                    out_image_stride_bytes, out_plane_stride_bytes, out_stride_bytes, nn2x=False, stream=0, opts=None):
        """Device-pointer batch of multi-plane images (w2xc_convert_planes_batch_device): n images of n_in planes of w x h, image i at d_in +
        i * in_image_stride_bytes, all planes of the last layer out, (w << nn2x) x (h << nn2x).  Each image has the bits of
        convert_planes[_nn2x]_device.  Asynchronous on `stream`."""
        rc = _lib.w2xc_convert_planes_batch_device(self.handle, n, 1 if nn2x else 0, n_in, C.c_void_p(d_in), in_image_stride_bytes, in_plane_stride_bytes,
                                                   in_stride_bytes, w, h, C.c_void_p(d_out), out_image_stride_bytes, out_plane_stride_bytes,
                                                   out_stride_bytes, C.c_void_p(stream), C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_planes_up2x_batch_device(self, n, n_in, d_in, in_image_stride_bytes, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                                         out_image_stride_bytes, out_plane_stride_bytes, out_stride_bytes, stream=0, opts=None):
        """Device-pointer batch for an upconv head model (w2xc_convert_planes_up2x_batch_device): n images of n_in planes of w x h, image i at d_in +
        i * in_image_stride_bytes, every plane of the head out at 2w x 2h.  Each image has the bits of convert_planes_up2x_device.  Asynchronous
        on `stream`."""
        rc = _lib.w2xc_convert_planes_up2x_batch_device(self.handle, n, n_in, C.c_void_p(d_in), in_image_stride_bytes, in_plane_stride_bytes,
                                                        in_stride_bytes, w, h, C.c_void_p(d_out), out_image_stride_bytes, out_plane_stride_bytes,
                                                        out_stride_bytes, C.c_void_p(stream), C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def batch_plan(self, n_in, w, h, nn2x=False, opts=None, up2x=False):
        """(batched, sub_batch) of w2xc_batch_plan: does a batch of w x h images of n_in planes run one launch per layer with these options, and how
        many images one sub-batch takes.  up2x: the plan of convert_planes_up2x_batch_device (an upconv head model; nn2x does not apply).  Host
        arithmetic only."""
        batched, sub = C.c_int(0), C.c_int(0)
        rc = _lib.w2xc_batch_plan(self.handle, n_in, w, h, 2 if up2x else 1 if nn2x else 0, C.byref(opts) if opts is not None else None, C.byref(batched), C.byref(sub))
        if rc != OK:
            raise W2xcError(rc, last_error())
        return batched.value, sub.value

    def convert_batch_tta_device(self, n, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes,
                                 out_stride_bytes, nn2x=False, stream=0, opts=None):
        """One test-time-augmentation pass on each of n planes (w2xc_convert_batch_tta_device; arguments as convert_batch_device): the model on
        the 8 flips / transposes of a plane, each result transformed back, their fp32 mean (the order of the sum: include/w2xc_hip.h)."""
        rc = _lib.w2xc_convert_batch_tta_device(self.handle, n, 1 if nn2x else 0, C.c_void_p(d_in), in_plane_stride_bytes, in_stride_bytes, w, h,
                                                C.c_void_p(d_out), out_plane_stride_bytes, out_stride_bytes, C.c_void_p(stream),
                                                C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_planes_tta_device(self, n_in, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes,
                                  out_stride_bytes, nn2x=False, stream=0, opts=None):
        """One test-time-augmentation pass of a multi-plane model (w2xc_convert_planes_tta_device; arguments as convert_planes_device, or -- nn2x
        -- as convert_planes_nn2x_device)."""
        rc = _lib.w2xc_convert_planes_tta_device(self.handle, n_in, 1 if nn2x else 0, C.c_void_p(d_in), in_plane_stride_bytes, in_stride_bytes, w, h,
                                                 C.c_void_p(d_out), out_plane_stride_bytes, out_stride_bytes, C.c_void_p(stream),
                                                 C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_rows_device(self, d_view, view_stride_bytes, view_h, view_y0, w, plane_h, row_begin, row_end,
                            d_out, out_stride_bytes, stream=0, opts=None):
        """Row-band form (one shard of a plane): see w2xc_convert_rows_device in include/w2xc_hip.h."""
        rc = _lib.w2xc_convert_rows_device(self.handle, C.c_void_p(d_view), view_stride_bytes, view_h, view_y0, w,
                                           plane_h, row_begin, row_end, C.c_void_p(d_out), out_stride_bytes,
                                           C.c_void_p(stream), C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def convert_rows(self, view, view_y0, plane_h, row_begin, row_end, nn2x=0, opts=None, out=None):
        """One unit of the tile farm from HOST memory (w2xc_convert_plane_rows): `view` holds source rows
        [view_y0, view_y0 + len(view)) of a plane_h-row source plane; returns output rows [row_begin, row_end) (in
        output coordinates: of the 2x plane when nn2x = 1)."""
        src = Mat(view)
        w = src.cols
        if out is None:
            out = np.empty((row_end - row_begin, w << nn2x), np.float32)
        rc = _lib.w2xc_convert_plane_rows(self.handle, src.array.ctypes.data, src.step, view_y0, src.rows, w, plane_h, nn2x,
                                          row_begin, row_end, out.ctypes.data, out.strides[0],
                                          C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return out

    def filter_device(self, layer, n_in, d_in, in_strides, w, h, d_out, out_strides, stream=0, opts=None):
        """Model::filter on device data; *_strides = (plane, row, pixel) element strides in floats (w2xc_layer_filter_device)."""
        rc = _lib.w2xc_layer_filter_device(self.handle, layer, n_in, C.c_void_p(d_in), in_strides[0], in_strides[1], in_strides[2], w, h,
                                           C.c_void_p(d_out), out_strides[0], out_strides[1], out_strides[2], C.c_void_p(stream),
                                           C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())

    def filter(self, layer, planes, opts=None):
        """Model::filter: [nin,h,w] -> [nout,h,w]; raises W2xcError(ERR_PLANES) on a plane-count mismatch."""
        planes = [Mat(p).array for p in planes]
        nout = self.planes(layer)[1]
        h, w = planes[0].shape
        strides = {p.strides[0] for p in planes}
        if len(strides) != 1:
            planes = [np.ascontiguousarray(p) for p in planes]
        out = np.empty((nout, h, w), np.float32)
        ip = (C.c_void_p * len(planes))(*[p.ctypes.data for p in planes])
        op = (C.c_void_p * nout)(*[out[o].ctypes.data for o in range(nout)])
        rc = _lib.w2xc_layer_filter(self.handle, layer, len(planes), ip, planes[0].strides[0], w, h, op,
                                    out.strides[1], C.byref(opts) if opts is not None else None)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return out

    def plan_rows(self, w, plane_h, row_begin=0, row_end=None, view_y0=0, view_h=None, opts=None):
        """The band geometry a row-range conversion would run with (w2xc_plan_rows): no device needed."""
        row_end = plane_h if row_end is None else row_end
        view_h = plane_h - view_y0 if view_h is None else view_h
        p = RowPlan()
        p.struct_size = C.sizeof(RowPlan)
        rc = _lib.w2xc_plan_rows(self.handle, w, view_y0, view_h, plane_h, row_begin, row_end,
                                 C.byref(opts) if opts is not None else None, C.byref(p))
        if rc != OK:
            raise W2xcError(rc, last_error())
        return p

    @staticmethod
    def plan_region(plan, plane_h, layer, y0, y1):
        """plane rows [top, bottom) layer `layer` (1-based) computes for the band [y0, y1) under `plan` (w2xc_plan_region)"""
        t, b = C.c_int(), C.c_int()
        rc = _lib.w2xc_plan_region(C.byref(plan), plane_h, layer, y0, y1, C.byref(t), C.byref(b))
        if rc != OK:
            raise W2xcError(rc, last_error())
        return t.value, b.value

    def kernel_name(self, layer, opts=None):
        return _lib.w2xc_layer_kernel_name(self.handle, layer, C.byref(opts) if opts is not None else None).decode()

    def profile_read(self, device=-1):
        n = self.n_layers
        ms = (C.c_float * n)()
        cnt = (C.c_int * n)()
        rc = _lib.w2xc_profile_read(self.handle, device, ms, cnt, n)
        if rc != OK:
            raise W2xcError(rc, last_error())
        return list(ms), list(cnt)

    def profile_reset(self, device=-1):
        _lib.w2xc_profile_reset(self.handle, device)

    def fill_scratch(self, word, device=-1):
        """Test aid (w2xc_debug_fill_scratch): fill every grow-only scratch buffer of this model's context on `device` with the
        32-bit `word`; returns the number of bytes filled (0: no context yet)."""
        n = C.c_ulonglong(0)
        rc = _lib.w2xc_debug_fill_scratch(self.handle, device, word & 0xFFFFFFFF, C.byref(n))
        if rc != OK:
            raise W2xcError(rc, last_error())
        return n.value


class Model:
    """w2xc::Model -- ONE conv layer (modelHandler.hpp:24-90)."""

    def __init__(self, model_set, index):
        self._set, self._index = model_set, index

    def getNInputPlanes(self):
        return self._set.planes(self._index)[0]

    def getNOutputPlanes(self):
        return self._set.planes(self._index)[1]

    def filter(self, inputPlanes, outputPlanes):
        """bool filter(std::vector<cv::Mat>& in, std::vector<cv::Mat>& out) -- modelHandler.cpp:26-72."""
        try:
            out = self._set.filter(self._index, [m.array if isinstance(m, Mat) else m for m in inputPlanes])
        except W2xcError as e:
            sys.stderr.write(str(e) + "\n")
            return False
        del outputPlanes[:]
        outputPlanes.extend(Mat(out[o]) for o in range(out.shape[0]))
        return True

    def printWeightMatrix(self):   # modelHandler.cpp:229-235
        _, _, w, _ = self._set.layer_arrays(self._index)
        for k in w.reshape(-1, 3, 3):
            print(k)

    def printBiases(self):         # modelHandler.cpp:237-242
        for b in self._set.layer_arrays(self._index)[3]:
            print(b)


class modelUtility:
    """w2xc::modelUtility (modelHandler.hpp:92-113): JSON loader + nJob / block-size singleton."""
    _instance = None

    @staticmethod
    def generateModelFromJSON(fileName, models):
        try:
            s = _ModelSet.from_json(fileName)
        except W2xcError as e:
            sys.stderr.write(str(e) + "\n")
            return False
        models.extend(Model(s, i) for i in range(s.n_layers))
        return True

    @staticmethod
    def getInstance():
        if modelUtility._instance is None:
            modelUtility._instance = modelUtility()
        return modelUtility._instance

    def setNumberOfJobs(self, n):
        return _lib.w2xc_set_jobs(int(n)) == OK

    def getNumberOfJobs(self):
        return _lib.w2xc_get_jobs()

    def setBlockSize(self, size):
        return _lib.w2xc_set_block_size(int(size[0]), int(size[1])) == OK

    def setBlockSizeExp2Square(self, exp):
        return _lib.w2xc_set_block_size_exp2(int(exp)) == OK

    def getBlockSize(self):
        w, h = C.c_int(), C.c_int()
        _lib.w2xc_get_block_size(C.byref(w), C.byref(h))
        return (w.value, h.value)


def _set_of(models):
    """The w2xc_model* behind a list of Model layers.  A list that is exactly one loaded file in
    order reuses its handle (weights stay resident on the GPUs); any other selection / order of
    layers gets its own container, as the reference allows any vector of Models."""
    if not models:
        raise W2xcError(ERR_ARG, "empty model list")
    s = models[0]._set
    if all(m._set is s for m in models) and [m._index for m in models] == list(range(s.n_layers)):
        return s
    return _ModelSet.from_layers([m._set.layer_arrays(m._index) for m in models])


def convertWithModels(inputPlane, outputPlane, models, blockSplitting=True, opts=None):
    """bool w2xc::convertWithModels(cv::Mat& in, cv::Mat& out, std::vector<std::unique_ptr<Model>>&,
    bool blockSplitting = true) -- convertRoutine.cpp:21-51.  `outputPlane` (a Mat) is
    (re)allocated to the input size like cv::Mat::copyTo does (:46)."""
    try:
        s = _set_of(models)
        src = inputPlane if isinstance(inputPlane, Mat) else Mat(inputPlane)
        res = s.convert(src.array, blockSplitting, opts)
    except W2xcError as e:
        sys.stderr.write(str(e) + "\n")
        return False
    Mat(res).copyTo(outputPlane)
    return True


# ---- sharding one plane into independent row bands (multi-GPU: no exchange, host-side gather) ----
def shard_rows(plane_h, n_parts, part):
    """Output rows [begin, end) of shard `part` of `n_parts` (contiguous, sizes differ by <= 1 row).
    Same split as the in-process multi-device path of w2xc_convert_plane (csrc/w2xc_host_pipeline.cpp)."""
    return (plane_h * part) // n_parts, (plane_h * (part + 1)) // n_parts


def shard_view(plane_h, row_begin, row_end, n_layers):
    """Input rows [y0, y1) a shard needs: its rows plus an n_layers halo, clipped to the plane
    (the 2*nModel overlap of the reference's block split, convertRoutine.cpp:100-131).  This is the MINIMUM the row entry points accept;
    a shard that is to stitch BIT-identically with the whole-plane call passes the wide halo -- shard_view(h, ra, rb, 4 * n_layers) -- which the
    default F(4x4) mid-layer kernel needs for its banding-invariant geometry (on the minimum view W2XC_KERNEL_AUTO is refused with
    ERR_ARG; name a kernel -- KERNEL_WINOGRAD32 is banding-invariant there -- to use it)."""
    return max(0, row_begin - n_layers), min(plane_h, row_end + n_layers)


def _check(rc):
    if rc != OK:
        raise W2xcError(rc, last_error())


def _handles(noise, scale):
    return noise.handle if noise else None, scale.handle if scale else None


def _final_size(w, h, iterations, shrink_ratio):
    fw, fh = w << iterations, h << iterations
    if shrink_ratio:
        fw, fh = int(float(fw * shrink_ratio)), int(float(fh * shrink_ratio))
    return fw, fh


def _tta_entry(name, tta):
    """the entry point of an image call and its arguments behind opts: `name` itself without test-time augmentation, its *_tta form (int tta last) with"""
    if not tta:
        return getattr(_lib, name), ()
    return getattr(_lib, name.replace("_ex", "").replace("_device", "") + "_tta" + ("_device" if name.endswith("_device") else "")), (int(tta),)


def _image_host(entry, who, img, channels, noise, scale, iterations, opts, shrink_ratio, extra=(), lenient=False, tail=()):
    """the single-image host calls: an h x w x channels uint8 image in, the H x W x channels result out; `extra` = the entry's arguments between
    shrink_ratio and opts, `tail` those behind opts.  lenient (process_image_u8): whatever numpy casts to a contiguous uint8 array, unchecked"""
    if lenient:
        img = np.ascontiguousarray(img, dtype=np.uint8)
    else:
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise ValueError("%s wants a uint8 image (got %s)" % (who, img.dtype))
        if img.ndim != 3 or img.shape[2] != channels:
            raise ValueError("%s wants an h x w x %d image (got shape %r)" % (who, channels, img.shape))
        if img.strides[1:] != (channels, 1):
            img = np.ascontiguousarray(img)
    h, w, _ = img.shape
    fw, fh = _final_size(w, h, iterations, shrink_ratio)
    out = np.empty((max(fh, 0), max(fw, 0), channels), np.uint8)
    _check(entry(*_handles(noise, scale), img.ctypes.data, img.strides[0], w, h, out.ctypes.data, out.strides[0], iterations, float(shrink_ratio),
                 *extra, C.byref(opts) if opts is not None else None, *tail))
    return out


def _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts, batch=None, extra=(), tail=()):
    """the device-pointer image calls: one image, or -- batch = (n, in_image_stride_bytes, out_image_stride_bytes) -- n of them; `extra` = the entry's
    arguments between shrink_ratio and the stream (bleed_passes), `tail` those behind opts (tta)"""
    n, in_img, out_img = ((), (), ()) if batch is None else ((batch[0],), (batch[1],), (batch[2],))
    _check(entry(*_handles(noise, scale), *n, C.c_void_p(d_in), *in_img, in_stride_bytes, w, h, C.c_void_p(d_out), *out_img, out_stride_bytes, iterations,
                 float(shrink_ratio), *extra, C.c_void_p(stream), C.byref(opts) if opts is not None else None, *tail))


def process_image_u8(img, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, tta=False):
    """The CLI's processing modes on an h x w x 3 uint8 image (main.cpp -m noise | scale | noise_scale):
    `noise` / `scale` are _ModelSet objects (either may be None); shrink_ratio = the final INTER_LINEAR shrink
    of main.cpp:158-167 (0 = none).  tta: test-time augmentation -- every model pass on the 8 flips / transposes of Y, averaged
    (w2xc_process_image_u8_tta; 8x the CNN work)."""
    entry, tail = _tta_entry("w2xc_process_image_u8_ex", tta)
    return _image_host(entry, "process_image_u8", img, 3, noise, scale, iterations, opts, shrink_ratio, lenient=True, tail=tail)


def process_image_u8_device(d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, noise=None, scale=None, iterations=0, shrink_ratio=0.0,
                            stream=0, opts=None, tta=False):
    """Device-pointer form (w2xc_process_image_u8_ex_device / _tta_device): w x h x 3 uint8 at d_in, the result at d_out.  Asynchronous on `stream`."""
    entry, tail = _tta_entry("w2xc_process_image_u8_ex_device", tta)
    _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts, tail=tail)


def process_image_u8_batch(imgs, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, out=None, tta=False):
    """n uint8 images of one size in one call (w2xc_process_image_u8_batch): `imgs` is an (n, h, w, 3) uint8 array or a sequence of equal-shape
    (h, w, 3) uint8 arrays (ROI views with padded rows are passed as they are, page-locked arrays are DMA'd in place); returns an (n, H, W, 3)
    uint8 array (or fills `out`, such an array).  Image i is byte-identical to process_image_u8(imgs[i], ...) with the same arguments."""
    entry, tail = _tta_entry("w2xc_process_image_u8_batch", tta)
    return _image_batch(entry, "process_image_u8_batch", imgs, noise, scale, iterations, opts, shrink_ratio, out, tail)


def _image_batch(entry, who, imgs, noise, scale, iterations, opts, shrink_ratio, out, tail=(), channels=3, extra=()):
    """the host image batch of Y models (process_image_u8_batch), of RGB models (process_image_rgb_u8_batch) and of RGBA images (process_image_rgba_u8_batch,
    channels = 4): same arguments, same checks; `extra` = the entry's arguments between shrink_ratio and opts, `tail` those behind opts"""
    ch = channels
    if isinstance(imgs, np.ndarray):
        if imgs.ndim != 4:
            raise ValueError("%s wants an (n, h, w, %d) array or a sequence of h x w x %d images" % (who, ch, ch))
        imgs = [imgs[i] for i in range(imgs.shape[0])]
    srcs = [np.asarray(a) for a in imgs]
    if not srcs:
        raise ValueError("%s wants at least one image" % who)
    for a in srcs:
        if a.dtype != np.uint8:
            raise ValueError("%s wants uint8 images (got %s)" % (who, a.dtype))
        if a.ndim != 3 or a.shape[2] != ch:
            raise ValueError("%s wants h x w x %d images (got shape %r)" % (who, ch, a.shape))
    h, w, _ = srcs[0].shape
    if any(a.shape != (h, w, ch) for a in srcs):
        raise ValueError("%s: every image must have the same size (group images by size)" % who)
    if any(a.strides[1:] != (ch, 1) for a in srcs) or len({a.strides[0] for a in srcs}) != 1:
        srcs = [np.ascontiguousarray(a) for a in srcs]
    n = len(srcs)
    fw, fh = _final_size(w, h, iterations, shrink_ratio)
    if out is None:
        out = np.empty((n, max(fh, 0), max(fw, 0), ch), np.uint8)
    elif not isinstance(out, np.ndarray) or out.shape != (n, fh, fw, ch) or out.dtype != np.uint8 or out.strides[2:] != (ch, 1):
        raise ValueError("%s: `out` must be a uint8 (n, H, W, %d) array with contiguous rows" % (who, ch))
    ip = (C.c_void_p * n)(*[a.ctypes.data for a in srcs])
    op = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
    _check(entry(*_handles(noise, scale), n, ip, srcs[0].strides[0], w, h,
                 op, out.strides[1], iterations, float(shrink_ratio), *extra, C.byref(opts) if opts is not None else None, *tail))
    return out


def process_image_u8_batch_device(n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes,
                                  noise=None, scale=None, iterations=0, shrink_ratio=0.0, stream=0, opts=None, tta=False):
    """Device-pointer image batch (w2xc_process_image_u8_batch_device): n images of w x h x 3 uint8 at d_in + i * in_image_stride_bytes, the
    outputs at d_out + i * out_image_stride_bytes.  Asynchronous on `stream`."""
    entry, tail = _tta_entry("w2xc_process_image_u8_batch_device", tta)
    _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts,
                  batch=(n, in_image_stride_bytes, out_image_stride_bytes), tail=tail)


# ---- RGB models (3 planes in, 3 out): the image calls above for the form most published waifu2x weights have ----
def process_image_rgb_u8(img, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, tta=False):
    """An h x w x 3 uint8 image through RGB models (w2xc_process_image_rgb_u8_ex): x = u8 / 255 on the channels as given, an optional noise
    pass, `iterations` 2x passes (nearest 2x + CNN on all three planes), the optional INTER_LINEAR shrink, saturate(rint(255 x)).
    `noise` / `scale` are _ModelSet objects whose first layer takes 3 planes and whose last gives 3 (either may be None).  tta: test-time
    augmentation -- every pass on the 8 flips / transposes of the three planes, averaged before the rounding (w2xc_process_image_rgb_u8_tta)."""
    entry, tail = _tta_entry("w2xc_process_image_rgb_u8_ex", tta)
    return _image_host(entry, "process_image_rgb_u8", img, 3, noise, scale, iterations, opts, shrink_ratio, tail=tail)


def process_image_rgb_u8_device(d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, noise=None, scale=None, iterations=0, shrink_ratio=0.0,
                                stream=0, opts=None, tta=False):
    """Device-pointer form (w2xc_process_image_rgb_u8_ex_device): w x h x 3 uint8 at d_in, the result at d_out.  Asynchronous on `stream`."""
    entry, tail = _tta_entry("w2xc_process_image_rgb_u8_ex_device", tta)
    _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts, tail=tail)


def process_image_rgb_u8_batch(imgs, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, out=None, tta=False):
    """n uint8 images of one size through RGB models in one call (w2xc_process_image_rgb_u8_batch); arguments and checks as
    process_image_u8_batch.  Image i is byte-identical to process_image_rgb_u8(imgs[i], ...) with the same arguments."""
    entry, tail = _tta_entry("w2xc_process_image_rgb_u8_batch", tta)
    return _image_batch(entry, "process_image_rgb_u8_batch", imgs, noise, scale, iterations, opts, shrink_ratio, out, tail)


def process_image_rgb_u8_batch_device(n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes,
                                      noise=None, scale=None, iterations=0, shrink_ratio=0.0, stream=0, opts=None, tta=False):
    """Device-pointer image batch for RGB models (w2xc_process_image_rgb_u8_batch_device); arguments as process_image_u8_batch_device."""
    entry, tail = _tta_entry("w2xc_process_image_rgb_u8_batch_device", tta)
    _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts,
                  batch=(n, in_image_stride_bytes, out_image_stride_bytes), tail=tail)


def process_image_rgb_u8_up2x_batch(imgs, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, out=None, tta=False):
    """n uint8 images of one size with an upconv head model as `scale` (w2xc_process_image_rgb_u8_up2x_batch); arguments and checks as
    process_image_rgb_u8_batch.  Image i is byte-identical to process_image_rgb_u8(imgs[i], ...); tta: every pass on the 8 flips / transposes, the
    variants as the images of a head batch (n = 1 is the single-image TTA form)."""
    return _image_batch(_lib.w2xc_process_image_rgb_u8_up2x_batch, "process_image_rgb_u8_up2x_batch", imgs, noise, scale, iterations, opts, shrink_ratio, out,
                        (1 if tta else 0,))


def process_image_rgb_u8_up2x_batch_device(n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes,
                                           noise=None, scale=None, iterations=0, shrink_ratio=0.0, stream=0, opts=None, tta=False):
    """Device-pointer form (w2xc_process_image_rgb_u8_up2x_batch_device); arguments as process_image_rgb_u8_batch_device."""
    _image_device(_lib.w2xc_process_image_rgb_u8_up2x_batch_device, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio,
                  stream, opts, batch=(n, in_image_stride_bytes, out_image_stride_bytes), tail=(1 if tta else 0,))


def u8_to_rgb_device(d_in, in_stride_bytes, w, h, d_planes, stream=0):
    """uint8 / 255 of a w x h x 3 image into three contiguous w x h float planes at d_planes (w2xc_u8_to_rgb_device)."""
    ps = w * h * 4
    _check(_lib.w2xc_u8_to_rgb_device(C.c_void_p(d_in), in_stride_bytes, w, h, C.c_void_p(d_planes), C.c_void_p(d_planes + ps),
                                      C.c_void_p(d_planes + 2 * ps), C.c_void_p(stream)))


def rgb_to_u8_device(d_planes, w, h, d_out, out_stride_bytes, stream=0):
    """saturate(rint(255 x)) of three contiguous w x h float planes at d_planes into a w x h x 3 uint8 image (w2xc_rgb_to_u8_device)."""
    ps = w * h * 4
    _check(_lib.w2xc_rgb_to_u8_device(C.c_void_p(d_planes), C.c_void_p(d_planes + ps), C.c_void_p(d_planes + 2 * ps), w, h, C.c_void_p(d_out),
                                      out_stride_bytes, C.c_void_p(stream)))


def resize_linear_device(d_src, sw, sh, d_dst, dw, dh, stream=0):
    """cv::resize(Size(dw, dh), INTER_LINEAR) of the contiguous sw x sh float plane at d_src into the contiguous dw x dh plane at d_dst
    (w2xc_resize_linear_device): the resize of the image calls' shrink, at any pair of sizes."""
    _check(_lib.w2xc_resize_linear_device(C.c_void_p(d_src), sw, sh, C.c_void_p(d_dst), dw, dh, C.c_void_p(stream)))


# ---- test-time augmentation's building blocks (the image and plane calls take tta=True / are _ModelSet.convert_*_tta_device) ----
def tta_spread_device(d_src, n, src_plane_stride_bytes, src_stride_bytes, w, h, d_up, d_tr, variant_plane_stride_bytes, stream=0):
    """n float planes of w x h at d_src -> their 8 n flips / transposes (w2xc_tta_spread_device): T_k of plane i at d_up + (k n + i) variant strides
    for k = 0..3 (h x w), at d_tr + ((k - 4) n + i) strides for k = 4..7 (w x h); T_k = hflip if k & 1, then vflip if k & 2, then transpose if k & 4."""
    _check(_lib.w2xc_tta_spread_device(C.c_void_p(d_src), n, src_plane_stride_bytes, src_stride_bytes, w, h, C.c_void_p(d_up), C.c_void_p(d_tr),
                                       variant_plane_stride_bytes, C.c_void_p(stream)))


def tta_gather_device(d_up, d_tr, variant_plane_stride_bytes, n, w, h, d_dst, dst_plane_stride_bytes, dst_stride_bytes, stream=0):
    """8 n result planes in tta_spread_device's layout (the upright ones w x h) -> n planes of w x h at d_dst: each variant transformed back, their
    fp32 sum in the order k = 0..7, times 0.125 (w2xc_tta_gather_device)."""
    _check(_lib.w2xc_tta_gather_device(C.c_void_p(d_up), C.c_void_p(d_tr), variant_plane_stride_bytes, n, w, h, C.c_void_p(d_dst),
                                       dst_plane_stride_bytes, dst_stride_bytes, C.c_void_p(stream)))


def tta_spread_u8_device(d_src, n, image_stride_bytes, stride_bytes, px_bytes, ch0, ch_step, w, h, d_up, d_tr, variant_plane_stride_bytes, stream=0):
    """n interleaved uint8 images of w x h (pixels px_bytes apart) -> the 8 variants of their 3 n planes, plane 3 i + c = byte ch0 + c * ch_step of each
    pixel / 255: the floats and the layout of u8_to_rgb_device + tta_spread_device on 3 n planes (w2xc_tta_spread_u8_device)."""
    _check(_lib.w2xc_tta_spread_u8_device(C.c_void_p(d_src), n, image_stride_bytes, stride_bytes, px_bytes, ch0, ch_step, w, h, C.c_void_p(d_up),
                                          C.c_void_p(d_tr), variant_plane_stride_bytes, C.c_void_p(stream)))


def tta_gather_u8_device(d_up, d_tr, variant_plane_stride_bytes, n, planes_per_image, first_plane, n_ch, w, h, d_dst, image_stride_bytes, stride_bytes,
                         px_bytes, byte0, stream=0):
    """8 planes_per_image n result planes in tta_spread_device's layout -> bytes byte0 .. byte0 + n_ch - 1 of the px_bytes-wide pixels of n images at d_dst:
    saturate(rint(255 x)) of tta_gather_device's sum for planes first_plane .. of each image; no other byte is written (w2xc_tta_gather_u8_device)."""
    _check(_lib.w2xc_tta_gather_u8_device(C.c_void_p(d_up), C.c_void_p(d_tr), variant_plane_stride_bytes, n, planes_per_image, first_plane, n_ch, w, h,
                                          C.c_void_p(d_dst), image_stride_bytes, stride_bytes, px_bytes, byte0, C.c_void_p(stream)))


# ---- RGBA images: alpha through the scale model, the colour bled under the transparent pixels ----
def process_image_rgba_u8(img, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, bleed_passes=-1, tta=False):
    """An h x w x 4 uint8 image (three colour channels in the order the 3-channel call of the route expects, alpha last) through Y models or RGB models
    -- the models choose the route (w2xc_process_image_rgba_u8_ex): the colour bytes are those of process_image_u8 / process_image_rgb_u8 on the image
    after `bleed_passes` passes of the colour bleed (< 0: the layer counts of the models given; 0: none), alpha goes through the scale model.
    tta: test-time augmentation -- the n = 1 form of w2xc_process_image_rgba_u8_batch_tta."""
    if tta:
        return process_image_rgba_u8_batch([img], noise, scale, iterations, opts, shrink_ratio, bleed_passes, tta=tta)[0]
    return _image_host(_lib.w2xc_process_image_rgba_u8_ex, "process_image_rgba_u8", img, 4, noise, scale, iterations, opts, shrink_ratio,
                       extra=(int(bleed_passes),))


def process_image_rgba_u8_device(d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, noise=None, scale=None, iterations=0, shrink_ratio=0.0,
                                 bleed_passes=-1, stream=0, opts=None, tta=False):
    """Device-pointer form (w2xc_process_image_rgba_u8_ex_device): w x h x 4 uint8 at d_in, the result at d_out.  Asynchronous on `stream`.
    tta: the n = 1 form of w2xc_process_image_rgba_u8_batch_tta_device."""
    if tta:
        return process_image_rgba_u8_batch_device(1, d_in, 0, in_stride_bytes, w, h, d_out, 0, out_stride_bytes, noise, scale, iterations, shrink_ratio,
                                                  bleed_passes, stream, opts, tta=tta)
    _image_device(_lib.w2xc_process_image_rgba_u8_ex_device, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream,
                  opts, extra=(int(bleed_passes),))


def process_image_rgba_u8_batch(imgs, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, bleed_passes=-1, out=None, tta=False):
    """n RGBA images of one size in one call (w2xc_process_image_rgba_u8_batch): `imgs` is an (n, h, w, 4) uint8 array or a sequence of equal-shape
    (h, w, 4) uint8 arrays; returns an (n, H, W, 4) uint8 array (or fills `out`, such an array).  Image i is byte-identical to
    process_image_rgba_u8(imgs[i], ...) with the same arguments.  tta: every CNN pass of colour and alpha is its TTA pass
    (w2xc_process_image_rgba_u8_batch_tta)."""
    entry, tail = _tta_entry("w2xc_process_image_rgba_u8_batch", tta)
    return _image_batch(entry, "process_image_rgba_u8_batch", imgs, noise, scale, iterations, opts, shrink_ratio, out, tail, channels=4,
                        extra=(int(bleed_passes),))


def process_image_rgba_u8_batch_device(n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes,
                                       noise=None, scale=None, iterations=0, shrink_ratio=0.0, bleed_passes=-1, stream=0, opts=None, tta=False):
    """Device-pointer batch of RGBA images (w2xc_process_image_rgba_u8_batch_device / _batch_tta_device): n images of w x h x 4 uint8 at
    d_in + i * in_image_stride_bytes, the outputs at d_out + i * out_image_stride_bytes.  Asynchronous on `stream`."""
    entry, tail = _tta_entry("w2xc_process_image_rgba_u8_batch_device", tta)
    _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts,
                  batch=(n, in_image_stride_bytes, out_image_stride_bytes), extra=(int(bleed_passes),), tail=tail)


def process_image_rgba_u8_up2x_batch(imgs, noise=None, scale=None, iterations=0, opts=None, shrink_ratio=0.0, bleed_passes=-1, out=None, tta=False):
    """n >= 1 RGBA images of one size with an upconv head model as `scale` (w2xc_process_image_rgba_u8_up2x_batch); arguments and checks as
    process_image_rgba_u8_batch.  The colour bytes of image i are those of process_image_rgb_u8 on the bled image, alpha is channel 1 of the scale-only
    call on (A, A, A); one image is the single-image form.  tta: w2xc_process_image_rgba_u8_up2x_batch_tta."""
    entry, tail = _tta_entry("w2xc_process_image_rgba_u8_up2x_batch", tta)
    return _image_batch(entry, "process_image_rgba_u8_up2x_batch", imgs, noise, scale, iterations, opts, shrink_ratio, out, tail, channels=4,
                        extra=(int(bleed_passes),))


def process_image_rgba_u8_up2x_batch_device(n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes,
                                            noise=None, scale=None, iterations=0, shrink_ratio=0.0, bleed_passes=-1, stream=0, opts=None, tta=False):
    """Device-pointer form (w2xc_process_image_rgba_u8_up2x_batch_device / _batch_tta_device); arguments as process_image_rgba_u8_batch_device."""
    entry, tail = _tta_entry("w2xc_process_image_rgba_u8_up2x_batch_device", tta)
    _image_device(entry, noise, scale, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, stream, opts,
                  batch=(n, in_image_stride_bytes, out_image_stride_bytes), extra=(int(bleed_passes),), tail=tail)


def bleed_rgba_u8_device(d_in, in_stride_bytes, w, h, passes, d_out_rgb, out_stride_bytes, stream=0):
    """`passes` passes of the colour bleed on the w x h x 4 uint8 image at d_in -> the packed w x h x 3 image at d_out_rgb (w2xc_bleed_rgba_u8_device)."""
    _check(_lib.w2xc_bleed_rgba_u8_device(C.c_void_p(d_in), in_stride_bytes, w, h, int(passes), C.c_void_p(d_out_rgb), out_stride_bytes, C.c_void_p(stream)))


def bleed_rgba_u8_trim():
    """release the scratch bleed_rgba_u8_device keeps per device (w2xc_bleed_rgba_u8_trim); waits for those devices first"""
    _check(_lib.w2xc_bleed_rgba_u8_trim())


# ---- YUV frames: luma through Y models, chroma 2x on bytes (include/w2xc_hip.h, "YUV frames") ----
def yuv_chroma_size(w, h, chroma):
    """(cw, ch) of the chroma planes of a w x h frame; (0, 0) for YUV_400.  The siting flags (CHROMA_COSITED_*) do not change a size: they are masked off"""
    if isinstance(chroma, int) and chroma >= 0:
        chroma &= 0xF
    if chroma == YUV_400:
        return 0, 0
    if chroma not in (YUV_420, YUV_422, YUV_444):
        raise ValueError("unknown chroma layout %r" % (chroma,))
    return ((w + 1) // 2 if chroma != YUV_444 else w), ((h + 1) // 2 if chroma == YUV_420 else h)


def process_frames_yuv_u8_device(n, w, h, chroma, d_in, d_out, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, stream=0, opts=None):
    """Device-pointer form (w2xc_process_frames_yuv_u8_device): n frames of w x h described by the YuvPlanes d_in, the (w << iterations) x (h << iterations)
    frames by d_out.  Asynchronous on `stream`."""
    _check(_lib.w2xc_process_frames_yuv_u8_device(*_handles(noise, scale), n, w, h, chroma, range, C.byref(d_in), C.byref(d_out), iterations,
                                                  C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def _yuv_side(y, u, v, uv, pack=None):
    """the YuvPlanes of host arrays: y (n, h, w); u and v (n, ch, cw) planar, or uv (n, ch, cw, 2) interleaved (NV12); neither: no chroma.  pack: the
    Yuv16Planes of uint16 arrays with that packing"""
    s = YuvPlanes() if pack is None else Yuv16Planes()
    if pack is not None:
        s.pack = pack
    s.y, s.y_stride, s.y_frame_stride = y.ctypes.data, y.strides[1], y.strides[0]
    s.c_px = 1
    if uv is not None:
        s.u, s.v, s.c_stride, s.c_frame_stride, s.c_px = uv.ctypes.data, uv.ctypes.data + uv.itemsize, uv.strides[1], uv.strides[0], 2
    elif u is not None:
        s.u, s.v, s.c_stride, s.c_frame_stride = u.ctypes.data, v.ctypes.data, u.strides[1], u.strides[0]
    return s


def process_frames_yuv_u8(y, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, opts=None, out_nv12=None):
    """n YUV frames in one call (w2xc_process_frames_yuv_u8): y is an (n, h, w) uint8 array; chroma either planar -- u and v, (n, ch, cw) uint8 -- or
    interleaved -- uv, (n, ch, cw, 2) uint8, NV12 --, none with YUV_400.  Luma goes through `noise` and, `iterations` (0 or 1) times, through `scale`;
    chroma is enlarged on bytes.  Returns (Y, U, V), or (Y, UV) where the output is interleaved (out_nv12; default: as the input), or (Y,) for YUV_400."""
    return _frames_yuv_host(None, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12)


def process_frames_yuv_u8_rgb(y, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, matrix=MATRIX_BT709,
                              opts=None, out_nv12=None):
    """n YUV frames through RGB models -- three planes to three planes -- or an upconv head model as `scale`, by the colour matrix `matrix` (MATRIX_BT601 /
    _BT709 / _BT2020; w2xc_process_frames_yuv_u8_rgb).  Arrays and result as process_frames_yuv_u8; YUV_400 is refused: a grey frame belongs to that call."""
    return _frames_yuv_host(matrix, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12)


def sized_iterations(w, h, out_w, out_h):
    """what ITERATIONS_AUTO resolves to: the smallest k with (w << k) >= out_w and (h << k) >= out_h (5 where four steps do not reach: the call refuses it)"""
    k = 0
    while k < 5 and ((w << k) < out_w or (h << k) < out_h):
        k += 1
    return k


def _frames_yuv_host(matrix, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, wide=None, size=None):
    """the host frame calls: matrix = None: w2xc_process_frames_yuv_u8, else w2xc_process_frames_yuv_u8_rgb with that matrix; wide = (depth, pack, out_pack):
    their forms on uint16 arrays, w2xc_process_frames_yuv_u16[_rgb]; size = (out_w, out_h): their _sized forms"""
    dt, name = (np.uint8, "process_frames_yuv_u8") if wide is None else (np.uint16, "process_frames_yuv_u16")

    def u8(a, nd, what):
        a = np.asarray(a)
        if a.dtype != dt or a.ndim != nd:
            raise ValueError("%s wants %s as a %d-D %s array (got %s, shape %r)" % (name, what, nd, np.dtype(dt).name, a.dtype, a.shape))
        return np.ascontiguousarray(a)
    y = u8(y, 3, "y")
    n, h, w = y.shape
    cw, ch = yuv_chroma_size(w, h, chroma)
    if chroma == YUV_400:
        u = v = uv = None
    elif uv is not None:
        uv = u8(uv, 4, "uv")
        if uv.shape != (n, ch, cw, 2):
            raise ValueError("%s: uv must be (n, %d, %d, 2), got %r" % (name, ch, cw, uv.shape))
    else:
        if u is None or v is None:
            raise ValueError("%s wants u and v, or uv, unless chroma is YUV_400" % name)
        u, v = u8(u, 3, "u"), u8(v, 3, "v")
        if u.shape != (n, ch, cw) or v.shape != (n, ch, cw):
            raise ValueError("%s: u and v must be (n, %d, %d), got %r and %r" % (name, ch, cw, u.shape, v.shape))
    W, H = (w << iterations, h << iterations) if size is None else size
    ocw, och = yuv_chroma_size(max(W, 0), max(H, 0), chroma)
    nv12 = (uv is not None) if out_nv12 is None else bool(out_nv12)
    oy = np.empty((n, max(H, 0), max(W, 0)), dt)
    ou = ov = ouv = None
    if chroma != YUV_400:
        if nv12:
            ouv = np.empty((n, och, ocw, 2), dt)
        else:
            ou, ov = np.empty((n, och, ocw), dt), np.empty((n, och, ocw), dt)
    po = C.byref(opts) if opts is not None else None
    if wide is not None:
        depth, pack, out_pack = wide
        si, so = _yuv_side(y, u, v, uv, pack), _yuv_side(oy, ou, ov, ouv, pack if out_pack is None else out_pack)
        if size is not None and matrix is None:
            _check(_lib.w2xc_process_frames_yuv_u16_sized(*_handles(noise, scale), n, w, h, chroma, range, depth, C.byref(si), W, H, C.byref(so), iterations, po))
        elif size is not None:
            _check(_lib.w2xc_process_frames_yuv_u16_rgb_sized(*_handles(noise, scale), n, w, h, chroma, range, depth, matrix, C.byref(si), W, H, C.byref(so),
                                                              iterations, po))
        elif matrix is None:
            _check(_lib.w2xc_process_frames_yuv_u16(*_handles(noise, scale), n, w, h, chroma, range, depth, C.byref(si), C.byref(so), iterations, po))
        else:
            _check(_lib.w2xc_process_frames_yuv_u16_rgb(*_handles(noise, scale), n, w, h, chroma, range, depth, matrix, C.byref(si), C.byref(so), iterations, po))
        return (oy,) if chroma == YUV_400 else (oy, ouv) if nv12 else (oy, ou, ov)
    si, so = _yuv_side(y, u, v, uv), _yuv_side(oy, ou, ov, ouv)
    if size is not None and matrix is None:
        _check(_lib.w2xc_process_frames_yuv_u8_sized(*_handles(noise, scale), n, w, h, chroma, range, C.byref(si), W, H, C.byref(so), iterations, po))
    elif size is not None:
        _check(_lib.w2xc_process_frames_yuv_u8_rgb_sized(*_handles(noise, scale), n, w, h, chroma, range, matrix, C.byref(si), W, H, C.byref(so), iterations, po))
    elif matrix is None:
        _check(_lib.w2xc_process_frames_yuv_u8(*_handles(noise, scale), n, w, h, chroma, range, C.byref(si), C.byref(so), iterations, po))
    else:
        _check(_lib.w2xc_process_frames_yuv_u8_rgb(*_handles(noise, scale), n, w, h, chroma, range, matrix, C.byref(si), C.byref(so), iterations, po))
    return (oy,) if chroma == YUV_400 else (oy, ouv) if nv12 else (oy, ou, ov)


def process_frames_yuv_u8_rgb_device(n, w, h, chroma, d_in, d_out, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, matrix=MATRIX_BT709, stream=0,
                                     opts=None):
    """Device-pointer form (w2xc_process_frames_yuv_u8_rgb_device): n frames of w x h described by the YuvPlanes d_in through RGB models or an upconv head
    model, the (w << iterations) x (h << iterations) frames by d_out.  Asynchronous on `stream`."""
    _check(_lib.w2xc_process_frames_yuv_u8_rgb_device(*_handles(noise, scale), n, w, h, chroma, range, matrix, C.byref(d_in), C.byref(d_out), iterations,
                                                      C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def yuv8_to_rgb_device(d_src, n, w, h, chroma, range, matrix, d_rgb, image_stride_bytes, plane_stride_bytes, stream=0):
    """n frames (the YuvPlanes d_src) -> their 3 n float planes R, G, B in [0, 1] with contiguous rows, frame i's at d_rgb + i * image_stride_bytes +
    {0, 1, 2} * plane_stride_bytes (w2xc_yuv8_to_rgb_device)."""
    _check(_lib.w2xc_yuv8_to_rgb_device(C.byref(d_src), n, w, h, chroma, range, matrix, C.c_void_p(d_rgb), image_stride_bytes, plane_stride_bytes, C.c_void_p(stream)))


def rgb_to_yuv8_device(d_rgb, image_stride_bytes, plane_stride_bytes, n, w, h, chroma, range, matrix, d_dst, stream=0):
    """3 n float planes of w x h -> the bytes of n frames (the YuvPlanes d_dst), chroma the box mean over its luma block (w2xc_rgb_to_yuv8_device)."""
    _check(_lib.w2xc_rgb_to_yuv8_device(C.c_void_p(d_rgb), image_stride_bytes, plane_stride_bytes, n, w, h, chroma, range, matrix, C.byref(d_dst), C.c_void_p(stream)))


def y8_to_plane_device(d_src, n, frame_stride_bytes, stride_bytes, w, h, range, d_dst, plane_stride_bytes, stream=0):
    """n luma byte planes of w x h -> n float planes with contiguous rows: y = byte / 255 (RANGE_FULL) or (byte - 16) / 219 (RANGE_LIMITED)
    (w2xc_y8_to_plane_device)."""
    _check(_lib.w2xc_y8_to_plane_device(C.c_void_p(d_src), n, frame_stride_bytes, stride_bytes, w, h, range, C.c_void_p(d_dst), plane_stride_bytes, C.c_void_p(stream)))


def plane_to_y8_device(d_src, n, plane_stride_bytes, w, h, range, d_dst, frame_stride_bytes, stride_bytes, stream=0):
    """n float planes with contiguous rows -> n luma byte planes: saturate(rint(255 y)) or saturate(rint(219 y + 16)) (w2xc_plane_to_y8_device)."""
    _check(_lib.w2xc_plane_to_y8_device(C.c_void_p(d_src), n, plane_stride_bytes, w, h, range, C.c_void_p(d_dst), frame_stride_bytes, stride_bytes, C.c_void_p(stream)))


def chroma2x_u8_device(d_src, n, src_frame_stride_bytes, src_stride_bytes, src_px, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px, ow, oh, stream=0):
    """the bicubic 2x of n chroma byte planes of cw x ch samples (src_px bytes apart), bytes to bytes: the leading ow x oh samples of each enlargement, dst_px
    bytes apart (w2xc_chroma2x_u8_device)."""
    _check(_lib.w2xc_chroma2x_u8_device(C.c_void_p(d_src), n, src_frame_stride_bytes, src_stride_bytes, src_px, cw, ch, C.c_void_p(d_dst), dst_frame_stride_bytes,
                                        dst_stride_bytes, dst_px, ow, oh, C.c_void_p(stream)))


def chroma2x_u8_sited_device(d_src, n, src_frame_stride_bytes, src_stride_bytes, src_px, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px, ow, oh,
                             cosited, stream=0):
    """chroma2x_u8_device for chroma co-sited with luma: cosited = CHROMA_COSITED_X | CHROMA_COSITED_Y, any combination; 0 is chroma2x_u8_device, byte for byte
    (w2xc_chroma2x_u8_sited_device)."""
    _check(_lib.w2xc_chroma2x_u8_sited_device(C.c_void_p(d_src), n, src_frame_stride_bytes, src_stride_bytes, src_px, cw, ch, C.c_void_p(d_dst),
                                              dst_frame_stride_bytes, dst_stride_bytes, dst_px, ow, oh, cosited, C.c_void_p(stream)))


# ---- 16-bit YUV frames: values of 8 .. 16 bits in uint16 words (include/w2xc_hip.h, "16-bit YUV frames") ----
def process_frames_yuv_u16(y, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, opts=None, out_nv12=None,
                           depth=10, pack=PACK_LOW, out_pack=None):
    """process_frames_yuv_u8 on uint16 arrays (w2xc_process_frames_yuv_u16): every word holds a value of `depth` bits (8 .. 16) in its low bits (PACK_LOW:
    yuv420p10le, y4m C420p10) or its high bits (PACK_HIGH: P010 with uv); out_pack: the packing of the result (default: that of the input).  uv / out_nv12:
    interleaved chroma, (n, ch, cw, 2), as P010 has it."""
    return _frames_yuv_host(None, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, wide=(depth, pack, out_pack))


def process_frames_yuv_u16_rgb(y, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, matrix=MATRIX_BT709,
                               opts=None, out_nv12=None, depth=10, pack=PACK_LOW, out_pack=None):
    """process_frames_yuv_u8_rgb on uint16 arrays (w2xc_process_frames_yuv_u16_rgb); depth, pack and out_pack as process_frames_yuv_u16."""
    return _frames_yuv_host(matrix, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, wide=(depth, pack, out_pack))


def process_frames_yuv_u16_device(n, w, h, chroma, d_in, d_out, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, stream=0, opts=None, depth=10):
    """Device-pointer form (w2xc_process_frames_yuv_u16_device): n frames of w x h described by the Yuv16Planes d_in -- its `pack` included --, the
    (w << iterations) x (h << iterations) frames by d_out.  Asynchronous on `stream`."""
    _check(_lib.w2xc_process_frames_yuv_u16_device(*_handles(noise, scale), n, w, h, chroma, range, depth, C.byref(d_in), C.byref(d_out), iterations,
                                                   C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def process_frames_yuv_u16_rgb_device(n, w, h, chroma, d_in, d_out, noise=None, scale=None, iterations=0, range=RANGE_LIMITED, matrix=MATRIX_BT709, stream=0,
                                      opts=None, depth=10):
    """Device-pointer form (w2xc_process_frames_yuv_u16_rgb_device); arguments as process_frames_yuv_u16_device, and the colour matrix."""
    _check(_lib.w2xc_process_frames_yuv_u16_rgb_device(*_handles(noise, scale), n, w, h, chroma, range, depth, matrix, C.byref(d_in), C.byref(d_out), iterations,
                                                       C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def yuv16_to_rgb_device(d_src, n, w, h, chroma, range, depth, matrix, d_rgb, image_stride_bytes, plane_stride_bytes, stream=0):
    """n frames (the Yuv16Planes d_src) -> their 3 n float planes R, G, B in [0, 1] (w2xc_yuv16_to_rgb_device); planes as yuv8_to_rgb_device."""
    _check(_lib.w2xc_yuv16_to_rgb_device(C.byref(d_src), n, w, h, chroma, range, depth, matrix, C.c_void_p(d_rgb), image_stride_bytes, plane_stride_bytes,
                                         C.c_void_p(stream)))


def rgb_to_yuv16_device(d_rgb, image_stride_bytes, plane_stride_bytes, n, w, h, chroma, range, depth, matrix, d_dst, stream=0):
    """3 n float planes of w x h -> the words of n frames (the Yuv16Planes d_dst) (w2xc_rgb_to_yuv16_device)."""
    _check(_lib.w2xc_rgb_to_yuv16_device(C.c_void_p(d_rgb), image_stride_bytes, plane_stride_bytes, n, w, h, chroma, range, depth, matrix, C.byref(d_dst),
                                         C.c_void_p(stream)))


def y16_to_plane_device(d_src, n, frame_stride_bytes, stride_bytes, w, h, range, depth, pack, d_dst, plane_stride_bytes, stream=0):
    """n luma planes of 16-bit words -> n float planes with contiguous rows (w2xc_y16_to_plane_device); strides in bytes"""
    _check(_lib.w2xc_y16_to_plane_device(C.c_void_p(d_src), n, frame_stride_bytes, stride_bytes, w, h, range, depth, pack, C.c_void_p(d_dst), plane_stride_bytes,
                                         C.c_void_p(stream)))


def plane_to_y16_device(d_src, n, plane_stride_bytes, w, h, range, depth, pack, d_dst, frame_stride_bytes, stride_bytes, stream=0):
    """n float planes with contiguous rows -> n luma planes of 16-bit words (w2xc_plane_to_y16_device); strides in bytes"""
    _check(_lib.w2xc_plane_to_y16_device(C.c_void_p(d_src), n, plane_stride_bytes, w, h, range, depth, pack, C.c_void_p(d_dst), frame_stride_bytes, stride_bytes,
                                         C.c_void_p(stream)))


def chroma2x_u16_device(d_src, n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, depth, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px,
                        dst_pack, ow, oh, stream=0):
    """the bicubic 2x of n chroma planes of cw x ch 16-bit samples (src_px samples apart), words to words: the leading ow x oh samples of each enlargement,
    dst_px samples apart (w2xc_chroma2x_u16_device); strides in bytes"""
    _check(_lib.w2xc_chroma2x_u16_device(C.c_void_p(d_src), n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, depth, C.c_void_p(d_dst),
                                         dst_frame_stride_bytes, dst_stride_bytes, dst_px, dst_pack, ow, oh, C.c_void_p(stream)))


def chroma2x_u16_sited_device(d_src, n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, depth, d_dst, dst_frame_stride_bytes, dst_stride_bytes,
                              dst_px, dst_pack, ow, oh, cosited, stream=0):
    """chroma2x_u16_device for chroma co-sited with luma: cosited = CHROMA_COSITED_X | CHROMA_COSITED_Y, any combination; 0 is chroma2x_u16_device, word for word
    (w2xc_chroma2x_u16_sited_device)."""
    _check(_lib.w2xc_chroma2x_u16_sited_device(C.c_void_p(d_src), n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, depth, C.c_void_p(d_dst),
                                               dst_frame_stride_bytes, dst_stride_bytes, dst_px, dst_pack, ow, oh, cosited, C.c_void_p(stream)))


# ---- Sized YUV frames: an output size, up to four 2x steps, ITERATIONS_AUTO (include/w2xc_hip.h, "Sized YUV frames") ----
def process_frames_yuv_u8_sized(y, out_w, out_h, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED,
                                opts=None, out_nv12=None):
    """process_frames_yuv_u8 with the output frame out_w x out_h: iterations 0 .. 4 or ITERATIONS_AUTO, w <= out_w <= w << iterations and the same in y; the last
    level is shrunk linearly, chroma resized in one step (w2xc_process_frames_yuv_u8_sized)."""
    return _frames_yuv_host(None, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, size=(out_w, out_h))


def process_frames_yuv_u8_rgb_sized(y, out_w, out_h, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED,
                                    matrix=MATRIX_BT709, opts=None, out_nv12=None):
    """process_frames_yuv_u8_rgb with the output frame out_w x out_h (w2xc_process_frames_yuv_u8_rgb_sized)."""
    return _frames_yuv_host(matrix, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, size=(out_w, out_h))


def process_frames_yuv_u16_sized(y, out_w, out_h, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED,
                                 opts=None, out_nv12=None, depth=10, pack=PACK_LOW, out_pack=None):
    """process_frames_yuv_u16 with the output frame out_w x out_h (w2xc_process_frames_yuv_u16_sized)."""
    return _frames_yuv_host(None, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, wide=(depth, pack, out_pack), size=(out_w, out_h))


def process_frames_yuv_u16_rgb_sized(y, out_w, out_h, u=None, v=None, uv=None, chroma=YUV_420, noise=None, scale=None, iterations=ITERATIONS_AUTO,
                                     range=RANGE_LIMITED, matrix=MATRIX_BT709, opts=None, out_nv12=None, depth=10, pack=PACK_LOW, out_pack=None):
    """process_frames_yuv_u16_rgb with the output frame out_w x out_h (w2xc_process_frames_yuv_u16_rgb_sized)."""
    return _frames_yuv_host(matrix, y, u, v, uv, chroma, noise, scale, iterations, range, opts, out_nv12, wide=(depth, pack, out_pack), size=(out_w, out_h))


def process_frames_yuv_u8_sized_device(n, w, h, chroma, d_in, out_w, out_h, d_out, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED, stream=0,
                                       opts=None):
    """Device-pointer form (w2xc_process_frames_yuv_u8_sized_device): n frames of w x h described by the YuvPlanes d_in, the out_w x out_h frames by d_out.
    Asynchronous on `stream`."""
    _check(_lib.w2xc_process_frames_yuv_u8_sized_device(*_handles(noise, scale), n, w, h, chroma, range, C.byref(d_in), out_w, out_h, C.byref(d_out), iterations,
                                                        C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def process_frames_yuv_u8_rgb_sized_device(n, w, h, chroma, d_in, out_w, out_h, d_out, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED,
                                           matrix=MATRIX_BT709, stream=0, opts=None):
    """Device-pointer form (w2xc_process_frames_yuv_u8_rgb_sized_device); arguments as process_frames_yuv_u8_sized_device, and the colour matrix."""
    _check(_lib.w2xc_process_frames_yuv_u8_rgb_sized_device(*_handles(noise, scale), n, w, h, chroma, range, matrix, C.byref(d_in), out_w, out_h, C.byref(d_out),
                                                            iterations, C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def process_frames_yuv_u16_sized_device(n, w, h, chroma, d_in, out_w, out_h, d_out, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED, stream=0,
                                        opts=None, depth=10):
    """Device-pointer form (w2xc_process_frames_yuv_u16_sized_device): Yuv16Planes on both sides, their `pack` included."""
    _check(_lib.w2xc_process_frames_yuv_u16_sized_device(*_handles(noise, scale), n, w, h, chroma, range, depth, C.byref(d_in), out_w, out_h, C.byref(d_out),
                                                         iterations, C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def process_frames_yuv_u16_rgb_sized_device(n, w, h, chroma, d_in, out_w, out_h, d_out, noise=None, scale=None, iterations=ITERATIONS_AUTO, range=RANGE_LIMITED,
                                            matrix=MATRIX_BT709, stream=0, opts=None, depth=10):
    """Device-pointer form (w2xc_process_frames_yuv_u16_rgb_sized_device); arguments as process_frames_yuv_u16_sized_device, and the colour matrix."""
    _check(_lib.w2xc_process_frames_yuv_u16_rgb_sized_device(*_handles(noise, scale), n, w, h, chroma, range, depth, matrix, C.byref(d_in), out_w, out_h,
                                                             C.byref(d_out), iterations, C.c_void_p(stream), C.byref(opts) if opts is not None else None))


def chroma_resize_u8_device(d_src, n, src_frame_stride_bytes, src_stride_bytes, src_px, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px, ow, oh,
                            w, h, out_w, out_h, sub_x, sub_y, cosited=0, stream=0):
    """the bicubic of chroma2x_u8_sited_device at any ratio: n chroma byte planes of cw x ch -> ow x oh, positions by the LUMA sizes w x h -> out_w x out_h
    (out_w >= w, out_h >= h), the layout's subsampling flags sub_x / sub_y (0 or 1) and `cosited` (w2xc_chroma_resize_u8_device)."""
    _check(_lib.w2xc_chroma_resize_u8_device(C.c_void_p(d_src), n, src_frame_stride_bytes, src_stride_bytes, src_px, cw, ch, C.c_void_p(d_dst), dst_frame_stride_bytes,
                                             dst_stride_bytes, dst_px, ow, oh, w, h, out_w, out_h, sub_x, sub_y, cosited, C.c_void_p(stream)))


def chroma_resize_u16_device(d_src, n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, depth, d_dst, dst_frame_stride_bytes, dst_stride_bytes,
                             dst_px, dst_pack, ow, oh, w, h, out_w, out_h, sub_x, sub_y, cosited=0, stream=0):
    """chroma_resize_u8_device on 16-bit words of `depth` bits, either packing on either side (w2xc_chroma_resize_u16_device); strides in bytes"""
    _check(_lib.w2xc_chroma_resize_u16_device(C.c_void_p(d_src), n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, depth, C.c_void_p(d_dst),
                                              dst_frame_stride_bytes, dst_stride_bytes, dst_px, dst_pack, ow, oh, w, h, out_w, out_h, sub_x, sub_y, cosited,
                                              C.c_void_p(stream)))
