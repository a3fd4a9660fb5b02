"""ctypes loader for the two in-tree native libraries.

There is no Python or CPU fallback: if the libraries are missing (not built) this raises, and on a
machine without a HIP device every compute entry point returns an error code that the wrappers turn
into an exception.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# SI_HIP_LIB: a differently built kernel library (development: diagnostic / variant builds under build_variants/)
LIB_HIP_PATH = os.environ.get("SI_HIP_LIB") or os.path.join(PKG, "libsi_hip.so")
# SI_HOST_LIB: a differently built host library (tools/asan_host.sh points it at the ASan + UBSan build)
LIB_HOST_PATH = os.environ.get("SI_HOST_LIB") or os.path.join(PKG, "libsimpleinfer_amd.so")

_hip = None
_host = None


class NativeLibraryMissing(ImportError):
    pass


def _load(path):
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            "%s is not built: run `python -m simpleinfer_amd.build` (or __graft_entry__.build()); "
            "simpleinfer_amd has no non-HIP fallback" % path)
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


class SiConvPlan(C.Structure):
    """include/si_hip.h SiConvPlan: kernel-form choices of one call (every form of a family produces the same bits)"""
    _fields_ = [(k, C.c_int) for k in ("f32_tile", "wino23_form", "wino23_ocg", "f16_tile", "f16_detect_tile", "f16_s2c32", "f16_slab",
                                       "f16_slab_w2", "f16_pw_patch", "split3_bm")]
    DEFAULTS = dict(f32_tile=-1, wino23_form=0, wino23_ocg=0, f16_tile=-1, f16_detect_tile=-1, f16_s2c32=-1, f16_slab=-1, f16_slab_w2=-1,
                    f16_pw_patch=-1, split3_bm=0)

    def __init__(self, **kw):
        super().__init__()
        vals = dict(self.DEFAULTS)
        for k, v in kw.items():
            if k not in vals:
                raise TypeError("SiConvPlan has no field %r" % k)
            vals[k] = int(v)
        for k, v in vals.items():
            setattr(self, k, v)


class SiConv2dDesc(C.Structure):
    # (fewer positional initialisers than fields leave the trailing ones -- plan, range_flag -- NULL: the defaults)
    _fields_ = [(k, C.c_int) for k in
                ("n", "ih", "iw", "ic", "in_ld", "oh", "ow", "oc", "out_ld", "kh", "kw", "sh", "sw", "dh", "dw",
                 "pt", "pl", "groups", "has_bias", "act1", "has_residual", "res_ld", "act2")] + [
                     ("act_param", C.c_float), ("plan", C.POINTER(SiConvPlan)), ("range_flag", C.c_void_p)]


class SiConvTranspose2dDesc(C.Structure):
    _fields_ = [(k, C.c_int) for k in
                ("n", "ih", "iw", "ic", "in_ld", "oh", "ow", "oc", "out_ld", "kh", "kw", "sh", "sw", "ph", "pw", "oph", "opw", "dh", "dw",
                 "groups", "has_bias", "act")] + [("act_param", C.c_float)]


class SiUpsampleDesc(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n", "ih", "iw", "c", "in_ld", "oh", "ow", "out_ld", "align_corners")] + [
        ("step_h", C.c_float), ("step_w", C.c_float)]


class SiGroupNormDesc(C.Structure):
    """include/si_norm.h"""
    _fields_ = [(k, C.c_int) for k in ("n", "h", "w", "c", "groups", "in_ld", "out_ld")] + [
        ("eps", C.c_float), ("affine", C.c_int), ("act", C.c_int), ("act_param", C.c_float)]


class SiPad2dDesc(C.Structure):
    """include/si_pad.h"""
    _fields_ = [(k, C.c_int) for k in ("n", "ih", "iw", "c", "in_ld", "oh", "ow", "out_ld", "pad_l", "pad_r", "pad_t", "pad_b", "mode")] + [
        ("value", C.c_float)]


class SiAvgPool2dDesc(C.Structure):
    """include/si_pool.h"""
    _fields_ = [(k, C.c_int) for k in ("n", "ih", "iw", "c", "in_ld", "oh", "ow", "out_ld", "kh", "kw", "sh", "sw", "pt", "pl", "adaptive",
                                       "count_include_pad", "divisor_override")]


class SiSoftmaxDesc(C.Structure):
    """include/si_softmax.h"""
    _fields_ = [(k, C.c_int) for k in ("n", "h", "w", "c", "in_ld", "out_ld", "axis", "log")]


class SiReduceDesc(C.Structure):
    """include/si_reduce.h; axes: bit mask of the NHWC axes reduced over (1 n, 2 h, 4 w, 8 c)"""
    _fields_ = [(k, C.c_int) for k in ("n", "h", "w", "c", "in_ld", "out_ld", "axes", "op")]


class SiParamActDesc(C.Structure):
    """include/si_act.h; op: 0 clamp (p0 lo, p1 hi), 1 softplus (p0 beta, p1 threshold), 2 mish"""
    _fields_ = [("op", C.c_int), ("p0", C.c_float), ("p1", C.c_float), ("pixels", C.c_size_t), ("c", C.c_int), ("in_ld", C.c_int),
                ("out_ld", C.c_int)]


class SiLpNormDesc(C.Structure):
    """include/si_lpnorm.h; axes: bit mask of the NHWC axes reduced over (1 n, 2 h, 4 w, 8 c); p: 0 one, 1 two, 2 inf"""
    _fields_ = [(k, C.c_int) for k in ("n", "h", "w", "c", "in_ld", "out_ld", "axes", "p", "normalize")] + [("eps", C.c_float)]


class SiPixelShuffleDesc(C.Structure):
    """include/si_superres.h"""
    _fields_ = [(k, C.c_int) for k in ("n", "ih", "iw", "ic", "in_ld", "oh", "ow", "oc", "out_ld", "r", "inverse")]


class SiSliceDesc(C.Structure):
    """include/si_slice.h; start / step in NHWC order"""
    _fields_ = [(k, C.c_int) for k in ("n", "ih", "iw", "ic", "in_ld")] + [("start", C.c_int * 4), ("step", C.c_int * 4)] + [
        (k, C.c_int) for k in ("on", "oh", "ow", "oc", "out_ld")]


class SiPermuteDesc(C.Structure):
    """include/si_permute.h; the output loop nest, outermost first, with the input stride of every loop dimension"""
    _fields_ = [("rank", C.c_int), ("dims", C.c_int * 4), ("in_stride", C.c_longlong * 4), ("out_ld", C.c_int), ("form", C.c_int)]


class SiAttentionDesc(C.Structure):
    """include/si_attention.h; sb / ss: element strides of the batch index and of the sequence index"""
    _fields_ = [(k, C.c_int) for k in ("batch", "heads", "lq", "lk", "d")] + [
        (k, C.c_longlong) for k in ("q_sb", "q_ss", "k_sb", "k_ss", "v_sb", "v_ss", "o_sb", "o_ss")] + [("scale", C.c_float)]


class SiDeformConv2dDesc(C.Structure):
    """include/si_deform.h; in_ld / off_ld / mask_ld / out_ld: the pixel strides of x, offset, mask and out"""
    _fields_ = [(k, C.c_int) for k in
                ("n", "ih", "iw", "ic", "in_ld", "oh", "ow", "oc", "out_ld", "off_ld", "mask_ld", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw",
                 "groups", "offset_groups", "has_mask", "has_bias", "act")] + [("act_param", C.c_float)]


class SiGridSampleDesc(C.Structure):
    """include/si_grid.h; in_ld / out_ld: pixel strides of x and out (0: dense); gs_*: the element strides of the grid (grid_source 0), which
    are not looked at when the pointer is theta (grid_source 1)"""
    _fields_ = [(k, C.c_int) for k in ("n", "c", "h", "w", "ho", "wo", "in_ld", "out_ld", "mode", "padding_mode", "align_corners", "grid_source",
                                       "spatial_dims")] + [(k, C.c_longlong) for k in ("gs_n", "gs_h", "gs_w", "gs_k")]


class SiAffineGridDesc(C.Structure):
    """include/si_grid.h; out_ld: row stride of the stored [n][w][2][h] image (0: dense)"""
    _fields_ = [(k, C.c_int) for k in ("n", "h", "w", "out_ld", "align_corners")]


class SiRoiAlignDesc(C.Structure):
    """include/si_roi.h; in_ld / out_ld: pixel strides of x and out, rois_ld: row stride of the fp32 boxes (0: dense)"""
    _fields_ = [(k, C.c_int) for k in ("n", "c", "h", "w", "k", "ph", "pw", "in_ld", "out_ld", "rois_ld", "sampling_ratio", "aligned")] + [
        ("spatial_scale", C.c_float)]


class SiRnnDesc(C.Structure):
    """include/si_rnn.h; st / sb: element strides of the time index and of the batch index of x, the gate workspace and y"""
    _fields_ = [(k, C.c_int) for k in ("cell", "t", "batch", "input", "hidden", "dirs")] + [
        (k, C.c_longlong) for k in ("x_st", "x_sb", "g_st", "g_sb", "y_st", "y_sb")] + [("step0", C.c_int)]


class SiConv1dDesc(C.Structure):
    """include/si_conv1d.h; sn / sc: element strides of the batch index and of the channel row of x and y"""
    _fields_ = [(k, C.c_int) for k in ("n", "c", "l", "oc", "lo", "k", "stride", "dilation", "pad_left", "groups")] + [
        (k, C.c_longlong) for k in ("x_sn", "x_sc", "y_sn", "y_sc")] + [("act", C.c_int), ("act_param", C.c_float)]


class SiXcorrDesc(C.Structure):
    """include/si_xcorr.h; NHWC views: sn / sh / sp the element strides of the image (w: the filter; depthwise: the image), the row and the pixel,
    w_sc that of the filter's channel"""
    _fields_ = [(k, C.c_int) for k in ("n", "h", "w", "c", "oc", "ho", "wo", "kh", "kw", "stride_h", "stride_w", "dilation_h", "dilation_w",
                                       "pad_top", "pad_left", "groups")] + [
        (k, C.c_longlong) for k in ("x_sn", "x_sh", "x_sp", "w_sn", "w_sh", "w_sp", "w_sc", "y_sn", "y_sh", "y_sp")] + [
        ("per_sample", C.c_int), ("act", C.c_int), ("act_param", C.c_float)]


class SiDetectPostDesc(C.Structure):
    """include/si_detect.h; ne = 4 + objectness + classes + extra, ld / image_ld the element strides of a row (ROWS) or a channel (CHANNELS) and
    of an image"""
    _fields_ = [(k, C.c_int) for k in ("n", "rows", "classes", "objectness", "extra", "layout", "ld")] + [("image_ld", C.c_longlong),
                ("box_format", C.c_int), ("prob_threshold", C.c_float), ("nms_threshold", C.c_float), ("agnostic", C.c_int), ("max_det", C.c_int)]


class SiDetectPostOut(C.Structure):
    """include/si_detect.h; device pointers: dets and counts, and the three optional outputs (NULL: not wanted)"""
    _fields_ = [(k, C.c_void_p) for k in ("dets", "counts", "src_rows", "net_boxes", "extras")]


class SiDetectMaskDesc(C.Structure):
    """include/si_detect.h; prototypes [n][mh][mw][nm] with pixels proto_ld apart, the coefficients at extras[b][d][coef_off .. coef_off + nm)"""
    _fields_ = [(k, C.c_int) for k in ("n", "mh", "mw", "nm", "proto_ld", "max_det", "extra", "coef_off")] + [
        ("ratio_w", C.c_float), ("ratio_h", C.c_float)]


class SiBinaryDesc(C.Structure):
    """include/si_binary.h; d: extents of x / out in storage order, c0_stride / c1_stride: element strides of the constants (0: broadcast)"""
    _fields_ = [("d", C.c_int * 4), ("x_ld", C.c_int), ("out_ld", C.c_int), ("stages", C.c_int), ("op", C.c_int * 2), ("c0_stride", C.c_int * 4),
                ("c1_stride", C.c_int * 4), ("grid_cap", C.c_int)]


class SiLayoutNest(C.Structure):
    """include/si_layout.h; what si_layout_plan returns: view != 0, or the loop nest of the copy"""
    _fields_ = [("view", C.c_int), ("rank", C.c_int), ("dims", C.c_int * 8), ("in_stride", C.c_longlong * 8)]


class SiConv2dUpsampledSource(C.Structure):
    _fields_ = [("src", C.c_void_p), ("ih", C.c_int), ("iw", C.c_int), ("c", C.c_int), ("ld", C.c_int), ("c0", C.c_int),
                ("inv_scale_h", C.c_float), ("inv_scale_w", C.c_float)]


class SiYoloLevel(C.Structure):
    _fields_ = [("na", C.c_int), ("ne", C.c_int), ("rows_total", C.c_int), ("row_off", C.c_int), ("stride", C.c_float)]


class SiPool2dDesc(C.Structure):
    _fields_ = [(k, C.c_int) for k in
                ("n", "ih", "iw", "c", "in_ld", "oh", "ow", "out_ld", "kh", "kw", "sh", "sw", "dh", "dw", "pt", "pl")]


def hip():
    """libsi_hip.so with argtypes/restypes set (include/si_hip.h)."""
    global _hip
    if _hip is not None:
        return _hip
    L = _load(LIB_HIP_PATH)
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    ip = C.POINTER(C.c_int)
    sig = {
        "si_hip_version": (C.c_char_p, []),
        "si_hip_error_string": (C.c_char_p, [i]),
        "si_hip_device_count": (i, [ip]),
        "si_hip_set_device": (i, [i]),
        "si_hip_get_device": (i, [ip]),
        "si_hip_device_info": (i, [i, C.c_char_p, ip, C.POINTER(sz), ip]),
        "si_hip_malloc": (i, [C.POINTER(vp), sz]),
        "si_hip_free": (i, [vp]),
        "si_hip_host_alloc": (i, [C.POINTER(vp), sz]),
        "si_hip_host_free": (i, [vp]),
        "si_hip_host_register": (i, [vp, sz]),
        "si_hip_host_unregister": (i, [vp]),
        "si_hip_memset_async": (i, [vp, i, sz, vp]),
        "si_hip_memcpy_h2d": (i, [vp, vp, sz, vp]),
        "si_hip_memcpy_d2h": (i, [vp, vp, sz, vp]),
        "si_hip_memcpy_d2d": (i, [vp, vp, sz, vp]),
        "si_hip_stream_create": (i, [C.POINTER(vp)]),
        "si_hip_stream_create_priority": (i, [C.POINTER(vp), i]),
        "si_hip_stream_destroy": (i, [vp]),
        "si_hip_stream_sync": (i, [vp]),
        "si_hip_device_sync": (i, []),
        "si_hip_event_create": (i, [C.POINTER(vp)]),
        "si_hip_event_destroy": (i, [vp]),
        "si_hip_event_record": (i, [vp, vp]),
        "si_hip_event_sync": (i, [vp]),
        "si_hip_event_elapsed_ms": (i, [vp, vp, C.POINTER(f)]),
        "si_hip_stream_wait_event": (i, [vp, vp]),
        "si_hip_ipc_get_mem_handle": (i, [vp, vp]),
        "si_hip_ipc_open_mem_handle": (i, [vp, C.POINTER(vp)]),
        "si_hip_ipc_close_mem_handle": (i, [vp]),
        "si_hip_enable_peer_access": (i, [i]),
        "si_hip_device_pci_bus_id": (i, [i, C.c_char_p, i]),
        "si_hip_device_by_pci_bus_id": (i, [C.c_char_p]),
        "si_hip_graph_begin_capture": (i, [vp]),
        "si_hip_graph_end_capture": (i, [vp, C.POINTER(vp)]),
        "si_hip_graph_launch": (i, [vp, vp]),
        "si_hip_graph_destroy": (i, [vp]),
        "si_hip_conv2d_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_split3_supported": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_split3_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_split3_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_split3_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_split3_split_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_split3_upcat_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dUpsampledSource)]),
        "si_hip_conv2d_split3_upcat_f32": (i, [C.POINTER(SiConv2dDesc), vp, C.POINTER(SiConv2dUpsampledSource), vp, vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_wino23_split_supported": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino23_split_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino23_split_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_wino23_split_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_wino23_eligible": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino23_preferred": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino23_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino23_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_wino23_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_wino43_eligible": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino43_preferred": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino43_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_wino43_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_wino43_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_split_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_upcat_f32": (i, [C.POINTER(SiConv2dDesc), vp, C.POINTER(SiConv2dUpsampledSource), vp, vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_yolo_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, C.POINTER(SiYoloLevel), vp, vp, vp, vp]),
        "si_hip_conv2d_split3_yolo_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, C.POINTER(SiYoloLevel), vp, vp, vp, vp]),
        "si_hip_conv2d_upcat_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dUpsampledSource)]),
        "si_hip_conv2d_kernel_name": (C.c_char_p, [C.POINTER(SiConv2dDesc), vp]),
        "si_hip_conv2d_kernel_name_form": (C.c_char_p, [C.POINTER(SiConv2dDesc), vp, i]),
        "si_hip_conv_transpose2d_weight_elems": (sz, [C.POINTER(SiConvTranspose2dDesc)]),
        "si_hip_conv_transpose2d_pack_weight_host": (i, [C.POINTER(SiConvTranspose2dDesc), vp, vp]),
        "si_hip_conv_transpose2d_f32": (i, [C.POINTER(SiConvTranspose2dDesc), vp, vp, vp, vp, vp]),
        "si_hip_conv_transpose2d_kernel_name": (C.c_char_p, [C.POINTER(SiConvTranspose2dDesc)]),
        "si_hip_linear_f32": (i, [vp, i, i, vp, vp, i, vp, vp]),
        "si_hip_maxpool2d_f32": (i, [C.POINTER(SiPool2dDesc), vp, vp, vp]),
        "si_hip_adaptive_avgpool2d_f32": (i, [vp, i, i, i, i, i, vp, i, i, i, vp]),
        "si_hip_upsample_nearest_f32": (i, [vp, i, i, i, i, i, f, f, vp, i, i, i, vp]),
        "si_hip_upsample_nearest_steps_f32": (i, [vp, i, i, i, i, i, f, f, vp, i, i, i, vp]),
        "si_upsample_step": (i, [i, i, i, i, C.c_double, C.POINTER(C.c_float)]),
        "si_upsample_out_size": (i, [i, C.c_double]),
        "si_hip_upsample_bilinear_f32": (i, [C.POINTER(SiUpsampleDesc), vp, vp, vp]),
        "si_hip_upsample_bilinear_f16": (i, [C.POINTER(SiUpsampleDesc), vp, vp, vp]),
        "si_hip_upsample_bilinear_kernel_name": (C.c_char_p, [C.POINTER(SiUpsampleDesc), vp, vp, i]),
        "si_hip_segment_labels_f32": (i, [C.POINTER(SiUpsampleDesc), vp, vp, vp]),
        "si_hip_segment_labels_f16": (i, [C.POINTER(SiUpsampleDesc), vp, vp, vp]),
        "si_hip_copy_channels_f32": (i, [vp, sz, i, i, vp, i, vp]),
        "si_hip_cat_axis_f32": (i, [vp, ip, vp, ip, i, i, vp]),
        "si_hip_nhwc_to_nchw_f32": (i, [vp, i, i, i, i, i, vp, vp]),
        "si_hip_activation_f32": (i, [i, f, vp, sz, i, i, vp, i, vp]),
        "si_hip_binary_f32": (i, [i, vp, ip, i, vp, ip, i, vp, ip, i, vp]),
        "si_hip_binary_scalar_f32": (i, [i, vp, sz, i, i, f, vp, i, vp]),
        "si_hip_unary_f32": (i, [i, vp, sz, i, i, vp, i, vp]),
        "si_hip_batchnorm2d_f32": (i, [vp, sz, i, i, vp, vp, vp, vp, f, vp, i, vp]),
        "si_hip_yolo_decode_f32": (i, [vp, i, i, i, i, i, vp, vp, f, vp, i, i, vp]),
        "si_hip_f32_to_f16_host": (i, [vp, vp, sz]),
        "si_hip_f16_to_f32_host": (i, [vp, vp, sz]),
        "si_hip_conv2d_f16_supported": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_upcat_f16": (i, [C.POINTER(SiConv2dDesc), vp, C.POINTER(SiConv2dUpsampledSource), vp, vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_upcat_f16_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dUpsampledSource)]),
        "si_hip_conv2d_f16_tile_variant": (i, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_f16_kernel_name": (C.c_char_p, [C.POINTER(SiConv2dDesc), i]),
        "si_hip_conv2d_f16_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_f16_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_f16": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, i, vp]),
        "si_hip_conv2d_depthwise_f16": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_stem_f16": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp]),
        "si_hip_conv2d_stem_f16_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_stem_split3_f32": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp]),
        "si_hip_conv2d_stem_split3_weight_elems": (sz, [C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_stem_split3_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_stem_f16_pack_weight_host": (i, [C.POINTER(SiConv2dDesc), vp, vp]),
        "si_hip_conv2d_split_f16": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_yolo_f16": (i, [C.POINTER(SiConv2dDesc), vp, vp, vp, C.POINTER(SiYoloLevel), vp, vp, vp, vp]),
        "si_hip_conv2d_pw_slab_f16_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_pw_slab_f16": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_pw_cv3_f16_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_pw_cv3_f16": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp, vp, i, vp, vp,
                                         vp, vp]),
        "si_hip_conv2d_stem_s2c32_f16_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc)]),
        "si_hip_conv2d_stem_s2c32_f16": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp, vp]),
        "si_hip_conv2d_stem_s2c32_pw_f16_supported": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), i]),
        "si_hip_conv2d_stem_s2c32_pw_f16": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), C.POINTER(SiConv2dDesc), vp, vp, vp, vp, vp, vp,
                                                vp, vp, i, vp, i, vp]),
        "si_hip_conv2d_yolo_f16_tile": (i, [C.POINTER(SiConv2dDesc), C.POINTER(SiYoloLevel)]),
        "si_hip_activation_f16": (i, [i, f, vp, sz, i, i, vp, i, vp]),
        "si_hip_unary_f16": (i, [i, vp, sz, i, i, vp, i, vp]),
        "si_hip_binary_same_f16": (i, [i, vp, i, vp, i, vp, i, sz, i, vp]),
        "si_hip_binary_bcast_f16": (i, [i, vp, i, vp, i, vp, i, i, sz, i, vp]),
        "si_hip_maxpool2d_f16": (i, [C.POINTER(SiPool2dDesc), vp, vp, vp]),
        "si_hip_maxpool5_chain3_f32": (i, [vp, i, i, i, i, i, vp, i, vp, i, vp, i, vp]),
        "si_hip_maxpool5_chain3_f16": (i, [vp, i, i, i, i, i, vp, i, vp, i, vp, i, vp]),
        "si_hip_adaptive_avgpool2d_f16": (i, [vp, i, i, i, i, i, vp, i, i, i, vp]),
        "si_hip_convert_f32_f16": (i, [vp, sz, i, i, vp, i, vp]),
        "si_hip_convert_f16_f32": (i, [vp, sz, i, i, vp, i, vp]),
        "si_letterbox_geometry": (None, [i, i, i, i, ip, ip, C.POINTER(f), ip, ip]),
        "si_hip_letterbox_u8_f32": (i, [vp, i, i, vp, i, i, i, i, vp]),
        "si_hip_letterbox_batch_u8_f32": (i, [vp, i, sz, i, i, vp, i, i, i, i, vp]),
        "si_hip_resize_bilinear_u8c3": (i, [vp, i, sz, i, i, vp, sz, i, i, vp]),
        "si_hip_resize_letterbox_batch_u8_f32": (i, [vp, i, sz, i, i, vp, i, i, vp]),
        "si_hip_yolo_postprocess_workspace_bytes": (sz, [i, i, i]),
        "si_hip_yolo_postprocess_f32": (i, [vp, i, i, i, f, f, i, vp, vp, vp, i, vp, sz, vp]),
    }
    # include/si_norm.h: nn.GroupNorm / nn.InstanceNorm2d (a header and a table of their own, as si_shard.h has)
    norm = {
        "si_hip_groupnorm_workspace_bytes": (sz, [C.POINTER(SiGroupNormDesc)]),
        "si_hip_groupnorm_f32": (i, [C.POINTER(SiGroupNormDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_groupnorm_f16": (i, [C.POINTER(SiGroupNormDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_groupnorm_kernel_name": (C.c_char_p, [C.POINTER(SiGroupNormDesc), vp, vp, i]),
    }
    # include/si_pad.h: the explicit 2-D pads (again a header and a table of their own)
    pad = {
        "si_hip_pad2d_f32": (i, [C.POINTER(SiPad2dDesc), vp, vp, vp]),
        "si_hip_pad2d_f16": (i, [C.POINTER(SiPad2dDesc), vp, vp, vp]),
        "si_hip_pad2d_kernel_name": (C.c_char_p, [C.POINTER(SiPad2dDesc), vp, vp, i]),
    }
    # include/si_pool.h: nn.AvgPool2d and the general nn.AdaptiveAvgPool2d
    pool = {
        "si_hip_avgpool2d_f32": (i, [C.POINTER(SiAvgPool2dDesc), vp, vp, vp]),
        "si_hip_avgpool2d_f16": (i, [C.POINTER(SiAvgPool2dDesc), vp, vp, vp]),
        "si_hip_avgpool2d_kernel_name": (C.c_char_p, [C.POINTER(SiAvgPool2dDesc), vp, vp, i]),
    }
    # include/si_softmax.h: nn.Softmax / nn.LogSoftmax / nn.Softmax2d and the functional spellings
    softmax = {
        "si_hip_softmax_f32": (i, [C.POINTER(SiSoftmaxDesc), vp, vp, vp]),
        "si_hip_softmax_f16": (i, [C.POINTER(SiSoftmaxDesc), vp, vp, vp]),
        "si_hip_softmax_kernel_name": (C.c_char_p, [C.POINTER(SiSoftmaxDesc), vp, vp, i]),
    }
    # include/si_superres.h: nn.PixelShuffle / nn.PixelUnshuffle and nn.PReLU
    superres = {
        "si_hip_pixel_shuffle_f32": (i, [C.POINTER(SiPixelShuffleDesc), vp, vp, vp]),
        "si_hip_pixel_shuffle_f16": (i, [C.POINTER(SiPixelShuffleDesc), vp, vp, vp]),
        "si_hip_pixel_shuffle_kernel_name": (C.c_char_p, [C.POINTER(SiPixelShuffleDesc), vp, vp, i]),
        "si_hip_prelu_f32": (i, [vp, sz, i, i, vp, i, vp, i, vp]),
        "si_hip_prelu_f16": (i, [vp, sz, i, i, vp, i, vp, i, vp]),
        "si_hip_prelu_kernel_name": (C.c_char_p, [vp, sz, i, i, i, vp, i, i]),
    }
    # include/si_slice.h: torch.chunk / torch.split / Tensor.slice
    split_args = [vp, sz, i, i, i, ip, ip, C.POINTER(vp), ip]
    slice_ = {
        "si_hip_slice_f32": (i, [C.POINTER(SiSliceDesc), vp, vp, vp]),
        "si_hip_slice_f16": (i, [C.POINTER(SiSliceDesc), vp, vp, vp]),
        "si_hip_slice_kernel_name": (C.c_char_p, [C.POINTER(SiSliceDesc), vp, vp, i]),
        "si_hip_split_channels_f32": (i, split_args + [vp]),
        "si_hip_split_channels_f16": (i, split_args + [vp]),
        "si_hip_split_channels_kernel_name": (C.c_char_p, split_args + [i]),
    }
    # include/si_reduce.h: torch.sum / torch.mean / torch.amax / torch.amin
    reduce_ = {
        "si_hip_reduce_f32": (i, [C.POINTER(SiReduceDesc), vp, vp, vp]),
        "si_hip_reduce_f16": (i, [C.POINTER(SiReduceDesc), vp, vp, vp]),
        "si_hip_reduce_kernel_name": (C.c_char_p, [C.POINTER(SiReduceDesc), vp, vp, i]),
    }
    # include/si_act.h: clamp (nn.ReLU6 / nn.Hardtanh / torch.clamp), nn.Softplus, nn.Mish
    act = {
        "si_hip_param_act_f32": (i, [C.POINTER(SiParamActDesc), vp, vp, vp]),
        "si_hip_param_act_f16": (i, [C.POINTER(SiParamActDesc), vp, vp, vp]),
        "si_hip_param_act_kernel_name": (C.c_char_p, [C.POINTER(SiParamActDesc), vp, vp, i]),
    }
    # include/si_permute.h: the strided-gather copy behind Tensor.permute / reshape / view / torch.transpose
    permute_ = {
        "si_hip_permute_f32": (i, [C.POINTER(SiPermuteDesc), vp, vp, vp]),
        "si_hip_permute_f16": (i, [C.POINTER(SiPermuteDesc), vp, vp, vp]),
        "si_hip_permute_kernel_name": (C.c_char_p, [C.POINTER(SiPermuteDesc), vp, vp, i]),
    }
    # include/si_attention.h: fused scaled dot-product attention, the kernel of nn.MultiheadAttention
    attention_ = {
        "si_hip_attention_f32": (i, [C.POINTER(SiAttentionDesc), vp, vp, vp, vp, vp]),
        "si_hip_attention_f16": (i, [C.POINTER(SiAttentionDesc), vp, vp, vp, vp, vp]),
        "si_hip_attention_kernel_name": (C.c_char_p, [C.POINTER(SiAttentionDesc), vp, vp, vp, vp, i]),
    }
    # include/si_deform.h: deformable convolution, the kernel of torchvision.ops.DeformConv2d
    deform_ = {
        "si_hip_deform_conv2d_weight_elems": (sz, [C.POINTER(SiDeformConv2dDesc)]),
        "si_hip_deform_conv2d_pack_weight_host": (i, [C.POINTER(SiDeformConv2dDesc), vp, vp]),
        "si_hip_deform_conv2d_f32": (i, [C.POINTER(SiDeformConv2dDesc), vp, vp, vp, vp, vp, vp, vp]),
        "si_hip_deform_conv2d_kernel_name": (C.c_char_p, [C.POINTER(SiDeformConv2dDesc), vp, vp, vp, vp]),
    }
    # include/si_grid.h: F.grid_sample and F.affine_grid
    grid_ = {
        "si_hip_grid_sample_f32": (i, [C.POINTER(SiGridSampleDesc), vp, vp, vp, vp]),
        "si_hip_grid_sample_f16": (i, [C.POINTER(SiGridSampleDesc), vp, vp, vp, vp]),
        "si_hip_grid_sample_kernel_name": (C.c_char_p, [C.POINTER(SiGridSampleDesc), vp, vp, vp, i]),
        "si_hip_affine_grid_f32": (i, [C.POINTER(SiAffineGridDesc), vp, vp, vp]),
        "si_hip_affine_grid_f16": (i, [C.POINTER(SiAffineGridDesc), vp, vp, vp]),
        "si_hip_affine_grid_kernel_name": (C.c_char_p, [C.POINTER(SiAffineGridDesc), vp, vp, i]),
    }
    # include/si_roi.h: torchvision.ops.RoIAlign / roi_align (the boxes are fp32 for both entries)
    roi_ = {
        "si_hip_roi_align_f32": (i, [C.POINTER(SiRoiAlignDesc), vp, vp, vp, vp]),
        "si_hip_roi_align_f16": (i, [C.POINTER(SiRoiAlignDesc), vp, vp, vp, vp]),
        "si_hip_roi_align_kernel_name": (C.c_char_p, [C.POINTER(SiRoiAlignDesc), vp, vp, vp, i]),
    }
    # include/si_rnn.h: the recurrent step kernel of nn.LSTM / nn.GRU
    rnn_ = {
        "si_hip_rnn_layer_f32": (i, [C.POINTER(SiRnnDesc), vp, vp, vp, vp, vp, vp, vp, vp]),
        "si_hip_rnn_layer_f16": (i, [C.POINTER(SiRnnDesc), vp, vp, vp, vp, vp, vp, vp, vp]),
        "si_hip_rnn_workspace_bytes": (sz, [C.POINTER(SiRnnDesc), i, i]),
        "si_hip_rnn_pack_whh_f32": (i, [C.POINTER(SiRnnDesc), vp, vp]),
        "si_hip_rnn_pack_whh_f16": (i, [C.POINTER(SiRnnDesc), vp, vp]),
        "si_hip_rnn_kernel_name": (C.c_char_p, [C.POINTER(SiRnnDesc), vp, vp, i]),
    }
    # include/si_binary.h: arithmetic of an activation against one or two graph constants (pnnx.Attribute operands)
    binary_ = {
        "si_hip_binary_const_f32": (i, [C.POINTER(SiBinaryDesc), vp, vp, vp, vp, vp]),
        "si_hip_binary_const_f16": (i, [C.POINTER(SiBinaryDesc), vp, vp, vp, vp, vp]),
        "si_hip_binary_const_kernel_name": (C.c_char_p, [C.POINTER(SiBinaryDesc), vp, vp, vp, vp, i]),
    }
    # include/si_conv1d.h: the temporal convolution kernels of nn.Conv1d
    conv1d_ = {
        "si_hip_conv1d_f32": (i, [C.POINTER(SiConv1dDesc), vp, vp, vp, vp, vp]),
        "si_hip_conv1d_f16": (i, [C.POINTER(SiConv1dDesc), vp, vp, vp, vp, vp]),
        "si_hip_conv1d_weight_bytes": (sz, [C.POINTER(SiConv1dDesc), i]),
        "si_hip_conv1d_pack_weights_f32": (i, [C.POINTER(SiConv1dDesc), vp, vp]),
        "si_hip_conv1d_pack_weights_f16": (i, [C.POINTER(SiConv1dDesc), vp, vp]),
        "si_hip_conv1d_kernel_name": (C.c_char_p, [C.POINTER(SiConv1dDesc), vp, vp, i]),
    }
    # include/si_xcorr.h: the cross-correlation kernels of F.conv2d with a tensor filter
    xcorr_ = {
        "si_hip_xcorr_f32": (i, [C.POINTER(SiXcorrDesc), vp, vp, vp, vp, vp]),
        "si_hip_xcorr_f16": (i, [C.POINTER(SiXcorrDesc), vp, vp, vp, vp, vp]),
        "si_hip_xcorr_kernel_name": (C.c_char_p, [C.POINTER(SiXcorrDesc), vp, vp, vp, i]),
    }
    # include/si_detect.h: detection post-processing for anchor-free heads, payloads and instance masks
    detect_ = {
        "si_hip_detect_postprocess_workspace_bytes": (sz, [C.POINTER(SiDetectPostDesc)]),
        "si_hip_detect_postprocess_f32": (i, [C.POINTER(SiDetectPostDesc), vp, vp, C.POINTER(SiDetectPostOut), vp, sz, vp]),
        "si_hip_detect_filter_kernel_name": (C.c_char_p, [C.POINTER(SiDetectPostDesc), vp]),
        "si_hip_detect_masks_f32": (i, [C.POINTER(SiDetectMaskDesc), vp, vp, vp, vp, vp, vp]),
        "si_hip_detect_masks_kernel_name": (C.c_char_p, [C.POINTER(SiDetectMaskDesc), vp]),
    }
    # include/si_lpnorm.h: torch.norm / F.normalize
    lpnorm_ = {
        "si_hip_lpnorm_f32": (i, [C.POINTER(SiLpNormDesc), vp, vp, vp]),
        "si_hip_lpnorm_f16": (i, [C.POINTER(SiLpNormDesc), vp, vp, vp]),
        "si_hip_lpnorm_kernel_name": (C.c_char_p, [C.POINTER(SiLpNormDesc), vp, vp, i]),
    }
    for name, (res, args) in (list(sig.items()) + list(norm.items()) + list(pad.items()) + list(pool.items()) + list(softmax.items()) +
                              list(superres.items()) + list(slice_.items()) + list(reduce_.items()) + list(act.items()) + list(permute_.items()) +
                              list(attention_.items()) + list(deform_.items()) + list(grid_.items()) + list(roi_.items()) + list(rnn_.items()) +
                              list(binary_.items()) + list(conv1d_.items()) + list(xcorr_.items()) + list(detect_.items()) + list(lpnorm_.items())):
        fn = getattr(L, name)  # AttributeError here = header/library mismatch, which tests check
        fn.restype = res
        fn.argtypes = args
    L._si_signatures = sig
    L._si_norm_signatures = norm
    L._si_pad_signatures = pad
    L._si_pool_signatures = pool
    L._si_softmax_signatures = softmax
    L._si_superres_signatures = superres
    L._si_slice_signatures = slice_
    L._si_reduce_signatures = reduce_
    L._si_act_signatures = act
    L._si_permute_signatures = permute_
    L._si_attention_signatures = attention_
    L._si_deform_signatures = deform_
    L._si_grid_signatures = grid_
    L._si_roi_signatures = roi_
    L._si_rnn_signatures = rnn_
    L._si_binary_signatures = binary_
    L._si_conv1d_signatures = conv1d_
    L._si_xcorr_signatures = xcorr_
    L._si_detect_signatures = detect_
    L._si_lpnorm_signatures = lpnorm_
    _hip = L
    return L


class SiGatherStats(C.Structure):
    """include/si_shard.h"""
    _fields_ = [("wait_copies_ms_total", C.c_double), ("wait_barrier_ms_total", C.c_double), ("copy_ms_total", C.c_double),
                ("copy_ms_max", C.c_double), ("completes", C.c_longlong), ("copies", C.c_longlong), ("landed_ms_total", C.c_double)]


def host():
    """libsimpleinfer_amd.so with argtypes/restypes set (include/si_engine.h)."""
    global _host
    if _host is not None:
        return _host
    hip()  # dependency, loaded RTLD_GLOBAL first
    L = _load(LIB_HOST_PATH)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    cp = C.c_char_p
    sig = {
        "si_engine_create": (i, [C.POINTER(vp)]),
        "si_engine_destroy": (i, [vp]),
        "si_engine_set_option": (i, [vp, cp, i]),
        "si_engine_load_model": (i, [vp, cp, cp]),
        "si_engine_release": (i, [vp]),
        "si_engine_num_inputs": (i, [vp]),
        "si_engine_num_outputs": (i, [vp]),
        "si_engine_input_name": (cp, [vp, i]),
        "si_engine_output_name": (cp, [vp, i]),
        "si_engine_operand_shape": (i, [vp, cp, C.POINTER(i), C.POINTER(i)]),
        "si_engine_input": (i, [vp, cp, vp, i]),
        "si_engine_bind_output": (i, [vp, cp, vp]),
        "si_engine_forward": (i, [vp]),
        "si_engine_forward_async": (i, [vp]),
        "si_engine_sync": (i, [vp]),
        "si_engine_extract": (i, [vp, cp, C.POINTER(vp), C.POINTER(i)]),
        "si_engine_stream": (vp, [vp]),
        "si_engine_last_forward_ms": (C.c_float, [vp]),
        "si_engine_profile": (i, [vp]),
        "si_engine_profile_entry": (i, [vp, i, C.POINTER(cp), C.POINTER(cp), C.POINTER(cp), C.POINTER(C.c_float),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "si_engine_schedule": (i, [vp, cp, sz]),
        "si_pnnx_dump": (i, [cp, cp, i, cp]),
        "si_pnnx_save": (i, [cp, cp, i, i, cp, cp]),
        "si_registry_types": (i, [cp, sz]),
    }
    # include/si_shard.h: node-local rank group + direct output all-gather
    shard = {
        "si_group_create": (i, [cp, i, i, C.c_double, C.POINTER(vp)]),
        "si_group_destroy": (i, [vp]),
        "si_group_rank": (i, [vp]),
        "si_group_world": (i, [vp]),
        "si_group_barrier": (i, [vp]),
        "si_group_allgather": (i, [vp, vp, sz, vp]),
        "si_gather_create": (i, [vp, i, sz, i, C.POINTER(vp)]),
        "si_gather_create_mode": (i, [vp, i, sz, i, i, C.POINTER(vp)]),
        "si_gather_mode": (i, [vp]),
        "si_rccl_available": (i, []),
        "si_rccl_init": (i, [vp, i, C.POINTER(vp)]),
        "si_rccl_allgather": (i, [vp, vp, vp, sz, vp]),
        "si_rccl_destroy": (i, [vp]),
        "si_gather_destroy": (i, [vp]),
        "si_gather_slots": (i, [vp]),
        "si_gather_slab_bytes": (sz, [vp]),
        "si_gather_buffer": (vp, [vp, i]),
        "si_gather_slab": (vp, [vp, i]),
        "si_gather_push": (i, [vp, i, vp]),
        "si_gather_complete": (i, [vp, i]),
        "si_gather_stats": (i, [vp, C.POINTER(SiGatherStats), i]),
    }
    # include/si_layout.h: the layout algebra (pure host code: no device is touched)
    ip = C.POINTER(C.c_int)
    layout = {
        "si_layout_plan": (i, [i, ip, i, i, ip, ip, ip, i, ip, C.POINTER(SiLayoutNest)]),
    }
    for name, (res, args) in list(sig.items()) + list(shard.items()) + list(layout.items()):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    L._si_signatures = sig
    L._si_shard_signatures = shard
    L._si_layout_signatures = layout
    _host = L
    return L
