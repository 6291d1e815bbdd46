"""ctypes binding of librelax_hip.so (include/relax_hip.h).  No fallback: if the
HIP library is missing or fails to load, importing the engine raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RELAX_HIP_LIB") or os.path.join(_HERE, "csrc", "librelax_hip.so")   # override: another build of it

c_u8p = C.POINTER(C.c_uint8)
c_i32p = C.POINTER(C.c_int32)
c_u32p = C.POINTER(C.c_uint32)
c_f32p = C.POINTER(C.c_float)
c_vp = C.c_void_p

# name -> (restype, argtypes); mirrors include/relax_hip.h one to one
PROTOTYPES = {
    "relax_abi_version": (C.c_int, []),
    "relax_create": (C.c_int, [C.c_int, C.POINTER(c_vp)]),
    "relax_destroy": (C.c_int, [c_vp]),
    "relax_last_error": (C.c_char_p, [c_vp]),
    "relax_reserve": (C.c_int, [c_vp, C.c_int]),
    "relax_set_option": (C.c_int, [c_vp, C.c_char_p, C.c_int]),
    "relax_get_option": (C.c_int, [c_vp, C.c_char_p, C.POINTER(C.c_int)]),
    "relax_load_resnet50": (C.c_int, [c_vp, C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int]),
    "relax_load_vit": (C.c_int, [c_vp, C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int,
                                 C.c_int, C.c_int, C.c_int]),
    "relax_load_vit_ex": (C.c_int, [c_vp, C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int]),
    "relax_vit_geometry": (C.c_int, [c_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "relax_load_vgg16": (C.c_int, [c_vp, C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int]),
    "relax_fragment_pairs": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                       c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "relax_fragment_image": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                       c_vp, c_vp, c_vp, c_vp, c_vp]),
    "relax_gather_patches": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_fragment_pairs_ex": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "relax_fragment_image_ex": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          c_vp, c_vp, c_vp, c_vp, c_vp]),
    "relax_gather_patches_ex": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_merge_fragments": (C.c_int, [c_vp, c_vp, c_vp, c_vp, C.c_int64, c_vp]),
    "relax_attention_overlay": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "relax_attention_overlay_ex": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp,
                                             c_vp, c_vp]),
    "relax_optical_flow": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "relax_optical_flow_ex": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_double, C.c_int, c_vp, c_vp, c_vp]),
    "relax_flow_plan": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), c_vp, c_vp]),
    "relax_optical_flow_flags": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_double, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_flow_gauss_window": (C.c_int, [C.c_int, c_vp]),
    "relax_flow_area_table": (C.c_int, [C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "relax_flow_initial_level": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, c_vp, c_vp]),
    "relax_flow_to_rgb":(C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "relax_resize_frames": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "relax_resize_residual": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_resize_output_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "relax_resize_table": (C.c_int, [C.c_int, C.c_int, C.c_int, c_vp, c_vp, C.POINTER(C.c_int)]),
    "relax_resize_frames_ex": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "relax_resize_residual_ex": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_resnet50_features": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, C.POINTER(c_vp), c_vp]),
    "relax_resnet50_clip_features": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "relax_resnet50_canvas_geometry": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "relax_resnet50_set_canvas": (C.c_int, [c_vp, C.c_int, C.c_int]),
    "relax_resnet50_get_canvas": (C.c_int, [c_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "relax_resnet50_canvas_geometry_ex": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "relax_resnet50_set_canvas_ex": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_int]),
    "relax_vgg16_features": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, C.POINTER(c_vp), c_vp]),
    "relax_vit_features": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp]),
    "relax_vit_features_ex": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_vit_features_canvas": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_vit_intermediate_layers": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_vit_pos_embed": (C.c_int, [c_vp, C.c_int, C.c_int, c_vp, c_vp]),
    "relax_vit_canvas_geometry": (C.c_int, [c_vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "relax_load_mlp_head": (C.c_int, [c_vp, C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int,
                                      c_vp, c_vp, c_vp, C.c_int]),
    "relax_mlp_head": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp]),
    "relax_head_fit_scaler": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "relax_head_train_transform": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp]),
    "relax_head_train_init": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_int]),
    "relax_head_train_init_ex": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "relax_head_train_arch": (C.c_int, [c_vp, C.POINTER(C.c_int)]),
    "relax_head_train_import": (C.c_int, [c_vp, C.c_int, C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int,
                                          C.c_int64, C.c_int64]),
    "relax_head_train_export_numel": (C.c_int64, [c_vp]),
    "relax_head_train_export": (C.c_int, [c_vp, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "relax_head_train_copy": (C.c_int, [c_vp, C.c_int, C.c_int, c_vp]),
    "relax_head_criterion": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_float, C.c_float, c_vp, c_vp, c_vp]),
    "relax_head_train_step": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, c_vp, C.c_int] + [C.c_float] * 6 + [C.c_uint64, C.c_uint64,
                                        c_vp, c_vp, c_vp]),
    "relax_head_train_eval": (C.c_int, [c_vp, C.c_int, c_vp, c_vp, C.c_int, c_vp, C.c_int, C.c_float, C.c_float, c_vp, c_vp]),
    "relax_head_train_bn_pass": (C.c_int, [c_vp, C.c_int, C.c_int, c_vp, C.c_int, c_vp, C.c_int, c_vp]),
    "relax_head_train_swa_update": (C.c_int, [c_vp, c_vp]),
    "relax_head_train_loss_read": (C.c_int, [c_vp, C.c_int, C.c_int, c_vp, c_vp]),
    "relax_head_train_pad_abs_sum": (C.c_int, [c_vp, c_vp, c_vp]),
    "relax_head_train_dw1": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, c_vp]),
    "relax_head_train_step_adam": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, c_vp, C.c_int] + [C.c_double] * 5 + [C.c_int] + [C.c_float] * 3 +
                                             [C.c_uint64, C.c_uint64, c_vp, c_vp, c_vp]),
    "relax_head_train_export_optimizer": (C.c_int, [c_vp, C.c_int, c_vp, c_vp, c_vp]),
    "relax_head_train_import_optimizer": (C.c_int, [c_vp, C.POINTER(c_vp), C.POINTER(c_vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                                    C.c_int, C.c_int64]),
    "relax_head_train_pad_abs_sum_adam": (C.c_int, [c_vp, c_vp, c_vp]),
    "relax_head_train_dw1_adam": (C.c_int, [c_vp, C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_int, c_vp]),
    "relax_metrics_correlation": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp]),
    "relax_metrics_kendall": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, c_vp, c_vp]),
    "relax_metrics_pair_counts": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, c_vp, c_vp]),
    "relax_op_gemm": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_vp]),
    "relax_op_conv2d_nhwc": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp] + [C.c_int] * 10 + [c_vp]),
    "relax_op_conv2d_nhwc_ex": (C.c_int, [c_vp] * 12 + [C.c_int] * 3 + [c_vp, c_vp] + [C.c_int] * 11 + [c_vp]),
    "relax_op_layernorm": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_float, c_vp]),
    "relax_op_attention": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_int, c_vp]),
    "relax_op_attention_ex": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp]),
    "relax_op_bn_relu_maxpool": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_vp]),
    "relax_op_bn_relu_maxpool_amax": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_vp]),
    "relax_op_gap": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int64, c_vp]),
    "relax_op_pool_stats": (C.c_int, [c_vp, c_vp, C.c_int64, c_vp, C.c_int64, C.c_int, C.c_int, c_vp]),
    "relax_op_token_stats": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp]),
    "relax_op_vit_norm_token_stats": (C.c_int, [c_vp, c_vp, c_vp, c_vp, C.c_float, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp]),
    "relax_copy_bytes": (C.c_int, [c_vp, c_vp, c_vp, C.c_int64, c_vp]),
    "relax_segment_mean": (C.c_int, [c_vp, c_vp, C.c_int64, C.c_int, C.c_int, c_vp, C.c_int, c_vp, C.c_int64, C.c_int, c_vp]),
    "relax_png_decode": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, c_vp, C.c_int64, c_vp, C.c_int64, c_vp, c_vp]),
    "relax_png_encode_bound": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "relax_png_encode": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, c_vp, C.c_int64, c_vp, C.c_int64, c_vp, c_vp, c_vp]),
    "relax_png_encode_passes": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, c_vp, C.c_int64, c_vp, C.c_int64, c_vp, c_vp, C.c_int, c_vp]),
    "relax_yuv_frame_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "relax_yuv_coefficients": (C.c_int, [C.c_int, C.c_int, c_i32p]),
    "relax_yuv_to_bgr": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, C.c_int64, c_vp, c_vp]),
    "relax_yuv_frame_bytes_ex": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "relax_yuv_format_info": (C.c_int, [C.c_int, c_i32p]),
    "relax_yuv_to_bgr_ex": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, C.c_int64, c_vp, c_vp]),
    "relax_yuv_greyscale_scan_ex": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "relax_greyscale_scan": (C.c_int, [c_vp, C.c_int64, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "relax_yuv_greyscale_scan": (C.c_int, [c_vp, C.c_int64, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "relax_profile_enable": (C.c_int, [c_vp, C.c_int]),
    "relax_profile_read": (C.c_int, [c_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int64)]),
}

_lib = None


def load():
    """dlopen librelax_hip.so and attach prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C relax-vqa_amd/csrc).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.relax_abi_version() != 1:
        raise RuntimeError(f"librelax_hip.so ABI {lib.relax_abi_version()} != 1")
    _lib = lib
    return lib
