"""Host side of the MI355X feature-extraction engine.

PyTorch-ROCm is plumbing only (device memory allocation, streams, torch.distributed, tiny host-to-device copies of
index vectors); all compute of the clip paths (clip_vectors / full_clip_vectors: fragments, backbones, per-clip means) goes
through the C-ABI of librelax_hip.so (include/relax_hip.h) - the fragments are written straight into the batch buffer the
backbones read and the per-clip means straight into the result matrix, so no aten kernel runs in between.
Array-in / array-out counterparts of the reference's path-based functions:

  fragment_pairs      <- cv2.absdiff + process_patches('frame_diff') + get_original_frame_patches
                         (src/main_fragment_layerstack.py:302-310)
  fragment_image      <- process_patches('optical_flow', flow_rgb) (src/main_fragment_layerstack.py:319)
  merge_fragments     <- merge_fragments (src/main_fragment_layerstack.py:242-245)
  resnet50_features   <- get_deep_feature('resnet50', .., 'layer_stack'|'pool') + process_video_feature
                         (src/main_fragment_layerstack.py:83-99,124-160)
  vit_features        <- get_deep_feature('vit', ..) + process_video_feature (src/main_fragment_pool.py:114-143)
  vit_attention       <- get_last_selfattention + visualize_attention (src/extractor/visualise_vit.py:241-250,353-369)
  attention_overlay   <- map_attention_to_original (src/demo_visual.py:12-25)
  attention_overlays  <- the __main__ of src/demo_visual.py (:86-128) for a whole clip
  residual_resize     <- cv2.absdiff + the extractors' resize of the whole residual image (src/main_residual.py:223-231)
  whole_residual_*    <- the per-pair loop body of src/main_residual.py:221-254 (fragment-free ablation rows)
  whole_frame_pool_features <- the per-frame loop body of src/main_layer.py:189-196
  extract_clip        <- the per-video loop body of src/main_fragment_layerstack.py:293-344 plus the ViT
                         branch of src/demo_test.py:137-161 (config 3 of BASELINE.json)
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, colormap
from .fragment_geometry import backbone_geometry, fragment_geometry, overlay_slot_rule

LAYER_STACK_DIM = 13120
RN50_POOL_DIM = 2051
TOP_N = 196
TARGET = 224
RN_CANVAS_ANY = 1            # RELAX_RN_CANVAS_ANY (include/relax_hip.h): ResNet-50 canvases of any size in [64, 1024]
VGG16_LAYER_STACK_DIM = 4224
VGG16_POOL_DIM = 4099
VGG16_FEATURE_INDEX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]   # features[i] of the 13 convolutions (tap order)
VGG16_TAP_SHAPES = [(64, 224)] * 2 + [(128, 112)] * 2 + [(256, 56)] * 3 + [(512, 28)] * 3 + [(512, 14)] * 3
RN50_TAP_SHAPES = [(64, 112)] + [(256, 56)] * 3 + [(512, 28)] * 4 + [(1024, 14)] * 4 + [(2048, 7)] * 3
VIT_CONFIGS = {"vit_tiny": (192, 12, 3), "vit_small": (384, 12, 6), "vit_base": (768, 12, 12)}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class RelaxEngine:
    """One engine per (process, device).  Not thread-safe (mirrors the C handle)."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("RelaxEngine needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)  # make sure the HIP context exists before the library touches it
        h = C.c_void_p()
        rc = self.lib.relax_create(self.device.index, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"relax_create failed ({rc}): {self.lib.relax_last_error(None).decode()}")
        self.h = h
        self.vit_dim = None
        # opt-in, default off: (directory, video_name[, numbers]) makes full_clip_vector - the demo driver's pass,
        # demo_test.evaluate_video_quality - also write every pair's PNG files (visualisation.write_example_set)
        self.demo_write_png = None
        self.vit_patch = self.vit_ntok = self.vit_npatch = None   # geometry of the loaded ViT (load_vit)

    def close(self):
        if getattr(self, "h", None):
            self.lib.relax_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.relax_last_error(self.h).decode()}")

    # ---- frame decode ---------------------------------------------------------------------------
    def decode_png(self, sources, out=None, statuses=None, stats=None):
        """PNG files (paths or bytes) -> uint8 BGR [N,H,W,3] on this engine's device, as sampling.read_frame_bgr /
        cv2.imread (src/main_fragment_layerstack.py:295-296) give them, decoded by relax_png_decode (one workgroup per
        image); a list of [H,W,3] tensors if the sizes differ.  out: a uint8 [N,H,W,3] view to fill (strided slots allowed,
        e.g. clip.view(-1,H,W,3) of a [T,2,H,W,3] clip).  statuses / stats: see pngdecode.PngDecoder.decode.  The decode runs
        on this thread's own stream (pngdecode.decoder_for) and has finished when this returns; the result is recorded on
        the current stream.  16-bit, palette, gray + alpha and interlaced files are decoded on the host (counted in
        stats['fallback'])."""
        from . import pngdecode
        return pngdecode.decoder_for(self.device).decode(sources, out=out, statuses=statuses, stats=stats)

    def encode_png(self, images, filter=None, stats=None):
        """uint8 device images -> list of bytes, one PNG file each, as cv2.imwrite (src/main_fragment_layerstack.py:310,325)
        writes them: BGR as RGB, [H,W] as gray; equal to OpenCV's files on the decoded pixels.  images: [N,H,W,3] or [N,H,W],
        or a list of [H,W,3] / [H,W] tensors of differing sizes; items may sit in strided slots with packed rows (a view of a
        [T,2,H,W,3] clip, attention_overlay's frames).  filter: None = per row the filter with the smallest sum of absolute
        values, or 0..4 for every row.  All images go through one relax_png_encode call on this thread's own stream
        (pngencode.encoder_for), which has finished when this returns.  Channels other than 1 or 3 and rows over 16 KiB are
        written by Pillow (counted in stats['fallback'])."""
        from . import pngencode
        return pngencode.encoder_for(self.device).encode(images, filter=filter, stats=stats)

    def write_png(self, paths, images, filter=None, stats=None):
        """encode_png, each file written to its path."""
        from . import pngencode
        pngencode.encoder_for(self.device).write(paths, images, filter=filter, stats=stats)

    def yuv_to_bgr(self, planes_u8_device, H, W, pixfmt, matrix="bt601", out=None):
        """Raw 8-bit YUV frames already on the device -> uint8 BGR [N,H,W,3] (relax_yuv_to_bgr; the arithmetic and the chroma
        replication are stated in include/relax_hip.h and as numpy in sampling.yuv_frame_bgr).  planes_u8_device: uint8, N whole
        frames back to back (any shape with N * frame_bytes elements; a host array is uploaded first).  pixfmt: yuv420p, yuvj420p,
        yuv422p, yuvj422p, yuv444p, yuvj444p or nv12 (sampling.yuv_layout; others raise).  matrix: 'bt601' (what ffmpeg assumes
        for untagged raw input) or 'bt709'.  out: a uint8 [N,H,W,3] view to fill (strided slots with packed rows allowed, e.g.
        clip.view(-1,H,W,3)).  Runs on the current stream.  The kernel moves 16 bytes per access when W is a multiple of 16 and
        frame and slot start at 16-byte-aligned addresses, else bytewise, per frame."""
        return self._yuv_to_bgr(planes_u8_device, H, W, pixfmt, matrix, out, False)

    def yuv_to_bgr_ex(self, planes_u8_device, H, W, pixfmt, matrix="bt601", out=None):
        """yuv_to_bgr for every pixfmt of sampling.yuv_format (relax_yuv_to_bgr_ex): 10 / 12-bit planar, p010le, yuyv422, uyvy422,
        yuv411p, yuv410p and nv21 beside the 8-bit names, which give yuv_to_bgr's bytes.  The same arguments and the same checks;
        the numpy statement is sampling.yuv_frame_bgr_ex on sampling.yuv_samples."""
        return self._yuv_to_bgr(planes_u8_device, H, W, pixfmt, matrix, out, True)

    def _yuv_to_bgr(self, planes_u8_device, H, W, pixfmt, matrix, out, extended):
        from . import sampling
        layout, full_range, frame_bytes, _ = sampling._yuv_source(pixfmt, extended)
        convert, name = (self.lib.relax_yuv_to_bgr_ex, "relax_yuv_to_bgr_ex") if extended else (self.lib.relax_yuv_to_bgr, "relax_yuv_to_bgr")
        if matrix not in sampling.YUV_MATRICES:
            raise ValueError(f"matrix {matrix!r} is not one of {', '.join(sampling.YUV_MATRICES)}")
        H, W = int(H), int(W)
        fb = frame_bytes(H, W)
        src = self._dev_u8(planes_u8_device).view(-1)
        if src.numel() % fb:
            raise ValueError(f"{src.numel()} bytes is not a whole number of {W}x{H} {pixfmt} frames of {fb} bytes")
        N = src.numel() // fb
        slot = H * W * 3
        if out is None:
            out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=self.device)
        else:
            if out.dtype != torch.uint8 or out.device != self.device or tuple(out.shape) != (N, H, W, 3):
                raise ValueError(f"out must be uint8 [{N},{H},{W},3] on {self.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
            if out.stride()[1:] != (W * 3, 3, 1) or (N > 1 and out.stride(0) < slot):
                raise ValueError(f"out must hold each frame as contiguous rows in its own slot, strides {out.stride()}")
        if N == 0:
            return out
        stride = out.stride(0) if N > 1 else slot
        # built on the device, on the current stream: a host tensor copied over would wait for the stream (tests/test_gpu_stream_contract.py)
        n_idx = torch.arange(N, dtype=torch.int64, device=self.device)
        items = torch.stack([n_idx * fb, n_idx * stride], dim=1).contiguous()
        status = torch.empty(N, dtype=torch.int32, device=self.device)
        rc = convert(_ptr(src), src.numel(), _ptr(items), N, layout, H, W, sampling.YUV_MATRICES[matrix],
                     int(full_range), _ptr(out), (N - 1) * stride + slot, _ptr(status), _stream())
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc}): {self.lib.relax_last_error(None).decode()}")
        return out

    # ---- greyscale screen (data_processing/check_greyscale.py, csrc/greyscale.hip) -------------------------------
    def greyscale_scan(self, frames):
        """The reference's is_greyscale_image (src/data_processing/check_greyscale.py:25-35) for many frames at once
        (relax_greyscale_scan): frames uint8 [N,H,W,3], [T,2,H,W,3], a strided view of either, or [N,H,W] (greyscale by the
        reference's first branch, nothing launched); a host array is uploaded first.  -> a dict of device tensors - 'records' int32
        [N,8], 'wrapped' [N,3] (maxima of (b-g, b-r, g-r) mod 256: the reference's rule), 'abs' [N,3] (maxima of the absolute
        differences), 'status' [N] - with is_greyscale(threshold=3, mode='reference') -> bool [N]."""
        from .data_processing import check_greyscale
        if isinstance(frames, np.ndarray):
            frames = self._dev_u8(frames)
        return check_greyscale.scan_frames(frames)

    def yuv_greyscale_scan(self, planes, H, W, pixfmt, matrix="bt601"):
        """greyscale_scan(yuv_to_bgr(planes, H, W, pixfmt, matrix)) in one pass that writes no BGR (relax_yuv_greyscale_scan):
        each pixel is converted in registers and goes straight into the maxima.  Arguments as yuv_to_bgr's."""
        from .data_processing import check_greyscale
        return check_greyscale.scan_yuv_frames(self._dev_u8(planes), H, W, pixfmt, matrix)

    def yuv_greyscale_scan_ex(self, planes, H, W, pixfmt, matrix="bt601"):
        """greyscale_scan(yuv_to_bgr_ex(planes, H, W, pixfmt, matrix)) in one pass that writes no BGR
        (relax_yuv_greyscale_scan_ex), for every pixfmt of sampling.yuv_format.  Arguments and checks as yuv_greyscale_scan's."""
        from .data_processing import check_greyscale
        return check_greyscale.scan_yuv_frames(self._dev_u8(planes), H, W, pixfmt, matrix, extended=True)

    # ---- weights ------------------------------------------------------------------------------
    def _marshal_state_dict(self, sd):
        names, arrays = [], []
        for k, v in sd.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            v = np.asarray(v)
            if v.dtype.kind != "f":
                continue  # num_batches_tracked etc.
            names.append(k.encode())
            arrays.append(np.ascontiguousarray(v, dtype=np.float32))
        n = len(names)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
        cnames = (C.c_char_p * n)(*names)
        numels = (C.c_int64 * n)(*[a.size for a in arrays])
        return ptrs, cnames, numels, n, arrays

    def load_resnet50(self, state_dict):
        """state_dict: torchvision resnet50 key names -> fp32 arrays/tensors."""
        ptrs, names, numels, n, keep = self._marshal_state_dict(state_dict)
        self._check(self.lib.relax_load_resnet50(self.h, ptrs, names, numels, n), "relax_load_resnet50")
        del keep

    def load_vgg16(self, state_dict):
        """state_dict: torchvision vgg16 key names -> fp32 arrays/tensors (classifier.6 is ignored)."""
        ptrs, names, numels, n, keep = self._marshal_state_dict(state_dict)
        self._check(self.lib.relax_load_vgg16(self.h, ptrs, names, numels, n), "relax_load_vgg16")
        del keep

    def load_vit(self, state_dict, name_model="vit_base", patch_size=None):
        """state_dict: DINO ViT key names -> fp32 arrays/tensors.  patch_size 8 or 16 (VitGenerator's second argument,
        src/extractor/visualise_vit_layer.py:263-329); None reads it from patch_embed.proj.weight's shape [dim,3,p,p].
        Sets vit_patch, vit_ntok ((224/p)^2 + 1: 197 / 785) and vit_npatch: the geometry of a 224 x 224 call.  A ViT call sizes its
        outputs by the canvas it is given (vit_canvas_geometry)."""
        dim, depth, heads = VIT_CONFIGS[name_model]
        if patch_size is None:
            w = state_dict.get("patch_embed.proj.weight")
            if w is None or len(w.shape) != 4 or w.shape[2] != w.shape[3]:
                raise ValueError("load_vit: patch_size=None needs patch_embed.proj.weight of shape [dim,3,p,p] to read p from")
            patch_size = int(w.shape[2])
        if patch_size not in (8, 16):
            raise ValueError(f"load_vit: patch_size {patch_size} is not built (8 or 16)")
        ptrs, names, numels, n, keep = self._marshal_state_dict(state_dict)
        self._check(self.lib.relax_load_vit_ex(self.h, ptrs, names, numels, n, dim, depth, heads, int(patch_size)), "relax_load_vit_ex")
        self.vit_dim = dim
        self.vit_patch, self.vit_ntok, _, _ = self.vit_geometry()
        self.vit_npatch = self.vit_ntok - 1
        del keep

    def vit_canvas_geometry(self, Hc, Wc):
        """(gh, gw, ntok) of an [Hc, Wc] canvas under the loaded ViT: gh = Hc // patch, gw = Wc // patch (the trailing pixels are ignored, as the
        reference's stride-p convolution ignores them, src/extractor/visualise_vit_layer.py:132-149), ntok = gh * gw + 1.  A side below the patch
        size or more than 4096 patches is refused (RuntimeError naming the value)."""
        if self.vit_dim is None:
            raise RuntimeError("load_vit first")
        v = [C.c_int(0) for _ in range(3)]
        self._check(self.lib.relax_vit_canvas_geometry(self.h, int(Hc), int(Wc), *[C.byref(x) for x in v]), "relax_vit_canvas_geometry")
        return tuple(int(x.value) for x in v)

    def vit_pos_embed(self, gh, gw):
        """interpolate_pos_encoding (src/extractor/visualise_vit_layer.py:197-219) for a gh x gw patch grid -> fp32 [1 + gh*gw, dim]: the class
        row, then the loaded table resampled bicubically as torch does it in fp32; the loaded table itself on the 224 x 224 grid."""
        if self.vit_dim is None:
            raise RuntimeError("load_vit first")
        gh, gw = int(gh), int(gw)
        if gh < 1 or gw < 1:
            raise ValueError(f"vit_pos_embed: grid {gh} x {gw}")
        out = torch.empty((1 + gh * gw, self.vit_dim), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_vit_pos_embed(self.h, gh, gw, _ptr(out), _stream()), "relax_vit_pos_embed")
        return out

    def vit_geometry(self):
        """(patch, ntok, dim, heads) of the loaded ViT at 224 x 224, read back from the library (relax_vit_geometry)."""
        v = [C.c_int(0) for _ in range(4)]
        self._check(self.lib.relax_vit_geometry(self.h, *[C.byref(x) for x in v]), "relax_vit_geometry")
        return tuple(int(x.value) for x in v)

    def load_mlp_head(self, state_dict, scaler_scale, scaler_min, imputer_statistics=None):
        """state_dict: the reference Mlp's keys (src/model_regression.py:37-58; without any bn1 key: the plain Mlp of
        src/model_regression_simple.py, loaded unfolded); scaler_* / imputer_statistics: the
        MinMaxScaler.scale_/.min_ and SimpleImputer.statistics_ arrays of the reference's model/scaler/*.pkl."""
        ptrs, names, numels, n, keep = self._marshal_state_dict(state_dict)
        sc = np.ascontiguousarray(scaler_scale, dtype=np.float64)
        mn = np.ascontiguousarray(scaler_min, dtype=np.float64)
        st = None if imputer_statistics is None else np.ascontiguousarray(imputer_statistics, dtype=np.float64)
        rc = self.lib.relax_load_mlp_head(self.h, ptrs, names, numels, n, C.c_void_p(st.ctypes.data) if st is not None else None,
                                          C.c_void_p(sc.ctypes.data), C.c_void_p(mn.ctypes.data), int(sc.size))
        self._check(rc, "relax_load_mlp_head")
        del keep

    def mlp_head(self, features):
        """features fp32 [n, F] on the device -> predicted scores fp32 [n] (src/demo_test.py:177-208)."""
        features = features.to(self.device, torch.float32).contiguous()
        out = torch.empty((features.shape[0],), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_mlp_head(self.h, _ptr(features), features.shape[0], _ptr(out), _stream()), "relax_mlp_head")
        return out

    # ---- training the quality head (head_train.py, csrc/head_train.hip) -------------------------------------------
    def fit_scaler(self, features, want_range=False):
        """preprocess_data's fit (src/model_regression.py:122-135) on a device fp32 [n, F] matrix, NaN / +-inf counted as 0:
        {'imputer_statistics', 'scale', 'min'} as host float64 [F] - what load_mlp_head takes (+ 'data_min' / 'data_max')."""
        features = features.to(self.device, torch.float32).contiguous()
        n, F = features.shape
        out = torch.empty((5, F), dtype=torch.float64, device=self.device)
        rc = self.lib.relax_head_fit_scaler(self.h, _ptr(features), n, F, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                            _ptr(out[3]) if want_range else None, _ptr(out[4]) if want_range else None, _stream())
        self._check(rc, "relax_head_fit_scaler")
        host = out.cpu().numpy()
        res = {"imputer_statistics": host[0].copy(), "scale": host[1].copy(), "min": host[2].copy()}
        if want_range:
            res.update(data_min=host[3].copy(), data_max=host[4].copy())
        return res

    def head_train_transform(self, features, scale, min_):
        """The training transform: NaN / +-inf -> 0, x * scale + min_ in float64, to fp32 [n, Fpad] (columns padded to a
        multiple of 32 with zeros) - the matrix the training steps read.  scale / min_: host arrays (uploaded, which waits for the current
        stream) or float64 device tensors, which are read where they are: the call then only enqueues."""
        features = features.to(self.device, torch.float32).contiguous()
        n, F = features.shape

        def f64(v):
            if isinstance(v, torch.Tensor) and v.is_cuda:
                return v.to(self.device, torch.float64).contiguous()
            return torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(self.device)
        sc, mn = f64(scale), f64(min_)
        xp = torch.empty((n, (F + 31) // 32 * 32), dtype=torch.float32, device=self.device)
        rc = self.lib.relax_head_train_transform(self.h, _ptr(features), n, F, _ptr(sc), _ptr(mn), _ptr(xp), _stream())
        self._check(rc, "relax_head_train_transform")
        return xp

    def fit_head(self, features, mos, config=None):
        """Trains the quality head as the reference's train_and_evaluate does; see head_train.fit_head."""
        from . import head_train
        return head_train.fit_head(self, features, mos, config)

    def fit_head_simple(self, features, mos, config=None):
        """Trains the plain head (no BatchNorm) on one 80/20 validation split, as the reference's model_regression_simple.py does;
        see head_train.fit_head_simple."""
        from . import head_train
        return head_train.fit_head_simple(self, features, mos, config)

    def fine_tune_head(self, state_dict, features, mos, config=None):
        """Fine-tunes a trained head as the reference's fine_tune_model does (a state dict without bn1 keys: the plain head); see
        head_train.fine_tune_head."""
        from . import head_train
        return head_train.fine_tune_head(self, state_dict, features, mos, config)

    # ---- scoring a head (metrics.py, csrc/metrics.hip) -----------------------------------------------------------
    def correlation_metrics(self, y_true, y_pred, return_fitted=False):
        """compute_correlation_metrics (src/model_regression.py:149-161) on the device: {'plcc', 'rmse', 'srcc', 'krcc', 'popt',
        'beta', 'converged', 'iterations', ...}; see metrics.correlation_metrics."""
        from . import metrics
        return metrics.correlation_metrics(self, y_true, y_pred, return_fitted)

    def kendall(self, x, y):
        """Kendall's tau-b and Spearman's rho from one pair pass on the device; see metrics.kendall."""
        from . import metrics
        return metrics.kendall(self, x, y)

    def evaluate_head(self, features_train, mos_train, features_test, mos_test, config=None):
        """One train / test split as the reference's main() runs it; see metrics.evaluate_head."""
        from . import metrics
        return metrics.evaluate_head(self, features_train, mos_train, features_test, mos_test, config)

    def holdout_protocol(self, features, mos, config=None, n_repeats=21, test_size=0.2, groups=None, drop_indices=None):
        """The repeated 80/20 hold-out with medians and the median model; drop_indices: the rows of a greyscale report, dropped
        first (metrics.drop_rows).  See metrics.holdout_protocol."""
        from . import metrics
        return metrics.holdout_protocol(self, features, mos, config, n_repeats, test_size, groups, drop_indices)

    def load_fitted_head(self, result):
        """load_mlp_head on what fit_head / fit_head_simple / fine_tune_head returned (either variant of the head)."""
        state_dict, scaler = result[0], result[1]
        self.load_mlp_head(state_dict, scaler["scale"], scaler["min"], scaler["imputer_statistics"])

    PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16x6": 2, "f16x2": 3}

    def set_precision(self, mode):
        """'fp32': exact fp32 products on the fp32 MFMA.  'bf16x6' (fp32-grade): each fp32 operand is held as three bf16
        values (hi + mid + lo, exact) and a*b = the six partial products of weight >= 2^-16 on the bf16 MFMA with fp32
        accumulation - as close to the exact result as the fp32 FMA chain at 6/16 of its matrix cycles.  'f16x2' (fp32-grade): each
        fp32 operand as two fp16 values of a power-of-two multiple of itself (22 bits; scales from bounds that hold for every input,
        csrc/h2.h), three partial products (four below K = 256) on the fp16 MFMA - the whole ViT-B (GEMMs and attention), ResNet-50's
        stem, 3x3 convolutions and layer3 / layer4; the launches without an f16x2 kernel run bf16x6 under it.  'bf16x3' (opt-in, lower precision): two bf16 values, three products, ~1e-5 norm-relative
        (the parity bar is 1e-3)."""
        self.set_option("gemm_precision", self.PRECISIONS[mode])

    def precision(self):
        """The arithmetic the engine's contraction kernel is in right now, read back from the library."""
        return {v: k for k, v in self.PRECISIONS.items()}[self.get_option("gemm_precision")]

    def set_option(self, key, value):
        self._check(self.lib.relax_set_option(self.h, key.encode(), int(value)), "relax_set_option")

    def get_option(self, key):
        v = C.c_int()
        self._check(self.lib.relax_get_option(self.h, key.encode(), C.byref(v)), "relax_get_option")
        return v.value

    def reserve(self, max_images):
        """Size the activation arena for batches of max_images fragments, for the models loaded NOW (load first, then reserve): the
        ViT's share follows its geometry - ViT-B/8 (785 tokens) takes 33.5 MB per image, 3.7 times ViT-B/16's 9.1 MB."""
        self._check(self.lib.relax_reserve(self.h, int(max_images)), "relax_reserve")

    # ---- stage A ------------------------------------------------------------------------------
    def _dev_u8(self, a):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        a = a.to(self.device, non_blocking=True)
        if a.dtype != torch.uint8:
            raise TypeError(f"expected uint8, got {a.dtype}")
        return a.contiguous()

    def fragment_pairs(self, frames, top_n=TOP_N, want_scores=False, out_ori=None, out_diff=None, patch_size=16, target_size=TARGET):
        """frames: uint8 [T,2,H,W,3] BGR (frames[t,0] = sampled frame, frames[t,1] = the next one).
        -> dict(positions int32 [T,196,2], counts int32 [T], ori_frag, diff_frag uint8 [T,224,224,3][, scores])
        out_ori / out_diff: optional preallocated [T,224,224,3] uint8 views (slices of a batch buffer) to write into.
        patch_size 8 / 16 / 32, target_size a multiple of it up to 448 (fragment_geometry.py): slots = (target_size / patch_size)^2,
        positions [T,slots,2], canvases [T,target_size,target_size,3], scores [T,H//patch_size,W//patch_size]; top_n=None = all slots."""
        geo = fragment_geometry(patch_size, target_size)      # (top_n out of range: refused by the library, a RuntimeError)
        top_n = geo.slots if top_n is None else int(top_n)
        frames = self._dev_u8(frames)
        if frames.dim() != 5 or frames.shape[1] != 2 or frames.shape[4] != 3:
            raise ValueError(f"frames must be [T,2,H,W,3], got {tuple(frames.shape)}")
        T, _, H, W, _ = frames.shape
        dev = self.device
        P, tgt = geo.patch_size, geo.target_size
        positions = torch.empty((T, geo.slots, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((T,), dtype=torch.int32, device=dev)
        ori = out_ori if out_ori is not None else torch.empty((T, tgt, tgt, 3), dtype=torch.uint8, device=dev)
        diff = out_diff if out_diff is not None else torch.empty((T, tgt, tgt, 3), dtype=torch.uint8, device=dev)
        for o in (ori, diff):
            if o.dtype != torch.uint8 or tuple(o.shape) != (T, tgt, tgt, 3) or not o.is_contiguous():
                raise ValueError(f"fragment_pairs: output buffers must be contiguous uint8 [T,{tgt},{tgt},3]")
        scores = torch.empty((T, (H // P) * (W // P)), dtype=torch.int32, device=dev) if want_scores else None
        frame_bytes = H * W * 3
        base = frames.data_ptr()
        rc = self.lib.relax_fragment_pairs_ex(self.h, C.c_void_p(base), C.c_void_p(base + frame_bytes), 2 * frame_bytes,
                                              T, H, W, P, tgt, top_n, _ptr(positions), _ptr(counts), _ptr(ori), _ptr(diff),
                                              _ptr(scores), _stream())
        self._check(rc, "relax_fragment_pairs")
        out = dict(positions=positions, counts=counts, ori_frag=ori, diff_frag=diff)
        if want_scores:
            out["scores"] = scores.view(T, H // P, W // P)
        return out

    def fragment_image(self, images, top_n=TOP_N, want_scores=False, out=None, patch_size=16, target_size=TARGET):
        """images: uint8 [T,H,W,3] residual images (e.g. flow_to_rgb output). -> dict(positions, counts, frag[, scores]);
        patch_size / target_size / top_n=None as in fragment_pairs."""
        geo = fragment_geometry(patch_size, target_size)      # (top_n out of range: refused by the library, a RuntimeError)
        top_n = geo.slots if top_n is None else int(top_n)
        images = self._dev_u8(images)
        if images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"images must be [T,H,W,3], got {tuple(images.shape)}")
        T, H, W, _ = images.shape
        dev = self.device
        P, tgt = geo.patch_size, geo.target_size
        positions = torch.empty((T, geo.slots, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((T,), dtype=torch.int32, device=dev)
        frag = out if out is not None else torch.empty((T, tgt, tgt, 3), dtype=torch.uint8, device=dev)
        if frag.dtype != torch.uint8 or tuple(frag.shape) != (T, tgt, tgt, 3) or not frag.is_contiguous():
            raise ValueError(f"fragment_image: the output buffer must be contiguous uint8 [T,{tgt},{tgt},3]")
        scores = torch.empty((T, (H // P) * (W // P)), dtype=torch.int32, device=dev) if want_scores else None
        rc = self.lib.relax_fragment_image_ex(self.h, _ptr(images), H * W * 3, T, H, W, P, tgt, top_n, _ptr(positions),
                                              _ptr(counts), _ptr(frag), _ptr(scores), _stream())
        self._check(rc, "relax_fragment_image")
        out = dict(positions=positions, counts=counts, frag=frag)
        if want_scores:
            out["scores"] = scores.view(T, H // P, W // P)
        return out

    def gather_patches(self, images, positions, counts, patch_size=16, target_size=TARGET):
        """get_original_frame_patches with given positions: int32 [T,slots,2] (slots of the geometry), counts int32 [T]
        -> uint8 [T,target_size,target_size,3]; a position outside the patch grid gives a zero tile."""
        geo = fragment_geometry(patch_size, target_size)
        images = self._dev_u8(images)
        T, H, W, _ = images.shape
        positions = positions.to(self.device, torch.int32).contiguous()
        counts = counts.to(self.device, torch.int32).contiguous()
        if tuple(positions.shape) != (T, geo.slots, 2) or tuple(counts.shape) != (T,):
            raise ValueError(f"gather_patches: positions [T,{geo.slots},2] and counts [T] expected for T={T}, got "
                             f"{tuple(positions.shape)}, {tuple(counts.shape)}")
        frag = torch.empty((T, geo.target_size, geo.target_size, 3), dtype=torch.uint8, device=self.device)
        rc = self.lib.relax_gather_patches_ex(self.h, _ptr(images), H * W * 3, T, H, W, geo.patch_size, geo.target_size, _ptr(positions),
                                              _ptr(counts), _ptr(frag), _stream())
        self._check(rc, "relax_gather_patches")
        return frag

    def merge_fragments(self, a, b, out=None):
        a, b = self._dev_u8(a), self._dev_u8(b)
        if a.shape != b.shape:
            raise ValueError("merge_fragments: shape mismatch")
        if out is None:
            out = torch.empty_like(a)
        self._check(self.lib.relax_merge_fragments(self.h, _ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()),
                    "relax_merge_fragments")
        return out

    FLOW_DEFAULTS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)

    def optical_flow(self, frames, want_flow=False, want_image=True, *, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5,
                     poly_sigma=1.2, flags=0, initial_flow=None, extended=False):
        """frames uint8 [T,2,H,W,3] BGR -> (flow fp32 [T,H,W,2] | None, flow image uint8 [T,H,W,3] | None): Farneback flow
        and the reference's flow_to_rgb visualisation (src/main_fragment_layerstack.py:313-316).  The keywords are
        cv2.calcOpticalFlowFarneback's parameters; their defaults are the reference's literals, and with all of them at the default the
        call is relax_optical_flow as ever.  Anything else goes through relax_optical_flow_ex (include/relax_hip.h has the limits:
        pyr_scale 0.5..0.95, levels 0..8 down to scale 1/32, odd winsize 3..63, iterations 1..10, poly_n 5 or 7, flags 0); the literals
        passed explicitly through it give the same bits.
        extended=True (the opt-in): the call goes through relax_optical_flow_flags, which also takes flags 256 (OPTFLOW_FARNEBACK_GAUSSIAN:
        the Gaussian window), 4 (OPTFLOW_USE_INITIAL_FLOW, with initial_flow fp32 [T,H,W,2]) and 260.  Both modes are pinned to the formulas
        stated in include/relax_hip.h and to their float64 restatement (tests/flow_flag_ref.py), not to an OpenCV build.  Without it
        nothing changes: flags 4 and 256 are refused as before."""
        given = dict(pyr_scale=pyr_scale, levels=levels, winsize=winsize, iterations=iterations, poly_n=poly_n, poly_sigma=poly_sigma,
                     flags=flags)
        if extended:
            return self._optical_flow_flags(frames, want_flow, want_image, given, initial_flow)
        if initial_flow is not None:
            raise ValueError("optical_flow: initial_flow needs extended=True (and flags with bit 4)")
        return self._optical_flow(frames, want_flow, want_image, None if given == self.FLOW_DEFAULTS else given)

    def optical_flow_flags(self, frames, want_flow=False, want_image=True, **params):
        """optical_flow through relax_optical_flow_flags whatever the parameters are (missing ones: the literals; initial_flow: the field
        flags bit 4 starts from) - the direct form of optical_flow(..., extended=True)."""
        initial_flow = params.pop("initial_flow", None)
        unknown = set(params) - set(self.FLOW_DEFAULTS)
        if unknown:
            raise TypeError(f"optical_flow_flags: unknown parameters {sorted(unknown)}")
        return self._optical_flow_flags(frames, want_flow, want_image, {**self.FLOW_DEFAULTS, **params}, initial_flow)

    def clip_flow_images(self, frames, flow_params=None):
        """The flow images of a clip's pairs for the clip methods' flow_params keyword: a dict of optical_flow's keywords (None: the literals),
        'extended' among them - {'flags': 256, 'extended': True} is the Gaussian window.  'initial_flow' is refused: the pairs of a clip are
        computed as one batch of independent pairs, and chaining pair t - 1's flow into pair t is not what these methods do."""
        flow_params = dict(flow_params or {})
        if "initial_flow" in flow_params:
            raise ValueError("flow_params: initial_flow is not accepted by the clip methods (a clip's pairs are independent); "
                             "call optical_flow(..., initial_flow=..., extended=True) and pass flow_images")
        return self.optical_flow(frames, **flow_params)[1]

    def _optical_flow_flags(self, frames, want_flow, want_image, params, initial_flow):
        frames = self._dev_u8(frames)
        if frames.dim() != 5 or frames.shape[1] != 2 or frames.shape[4] != 3:
            raise ValueError(f"frames must be [T,2,H,W,3], got {tuple(frames.shape)}")
        T, _, H, W, _ = frames.shape
        init = None
        if initial_flow is not None:
            init = initial_flow
            if not (isinstance(init, torch.Tensor) and init.device == frames.device and init.dtype == torch.float32 and init.is_contiguous()):
                init = torch.as_tensor(init).to(self.device, torch.float32).contiguous()
            if tuple(init.shape) != (T, H, W, 2):
                raise ValueError(f"initial_flow must be [T,H,W,2] = {(T, H, W, 2)}, got {tuple(init.shape)}")
        fl = torch.empty((T, H, W, 2), dtype=torch.float32, device=self.device) if want_flow else None
        im = torch.empty((T, H, W, 3), dtype=torch.uint8, device=self.device) if want_image else None
        fb = H * W * 3
        base = frames.data_ptr()
        rc = self.lib.relax_optical_flow_flags(self.h, C.c_void_p(base), C.c_void_p(base + fb), 2 * fb, T, H, W, float(params["pyr_scale"]),
                                               int(params["levels"]), int(params["winsize"]), int(params["iterations"]), int(params["poly_n"]),
                                               float(params["poly_sigma"]), int(params["flags"]), _ptr(init), _ptr(fl), _ptr(im), _stream())
        self._check(rc, "relax_optical_flow_flags")
        return fl, im

    def optical_flow_in_place(self, frames, flow, want_image=False, **params):
        """OpenCV's in/out use: `flow` fp32 [T,H,W,2] on the device is the initial field (flags must have bit 4) and receives the result
        (relax_optical_flow_flags with init_flow == flow) -> (flow, flow image | None)."""
        frames = self._dev_u8(frames)
        T, _, H, W, _ = frames.shape
        if not (isinstance(flow, torch.Tensor) and flow.is_cuda and flow.dtype == torch.float32 and flow.is_contiguous()
                and tuple(flow.shape) == (T, H, W, 2)):
            raise ValueError(f"optical_flow_in_place: flow must be a contiguous fp32 device tensor {(T, H, W, 2)}")
        unknown = set(params) - set(self.FLOW_DEFAULTS)
        if unknown:
            raise TypeError(f"optical_flow_in_place: unknown parameters {sorted(unknown)}")
        p = {**self.FLOW_DEFAULTS, **params}
        im = torch.empty((T, H, W, 3), dtype=torch.uint8, device=self.device) if want_image else None
        fb = H * W * 3
        base = frames.data_ptr()
        rc = self.lib.relax_optical_flow_flags(self.h, C.c_void_p(base), C.c_void_p(base + fb), 2 * fb, T, H, W, float(p["pyr_scale"]),
                                               int(p["levels"]), int(p["winsize"]), int(p["iterations"]), int(p["poly_n"]), float(p["poly_sigma"]),
                                               int(p["flags"]), _ptr(flow), _ptr(flow), _ptr(im), _stream())
        self._check(rc, "relax_optical_flow_flags")
        return flow, im

    def flow_initial_level(self, initial_flow, pyr_scale=0.5, levels=3):
        """initial_flow fp32 [T,H,W,2] -> fp32 [T,h_c,w_c,2]: the field relax_optical_flow_flags' coarsest level starts from under flags bit 4
        (relax_flow_initial_level: cv::resize(INTER_AREA)'s table, times (float)scale; (h_c, w_c) = flow_plan(H, W, pyr_scale, levels)[0])."""
        init = torch.as_tensor(initial_flow).to(self.device, torch.float32).contiguous()
        if init.dim() != 4 or init.shape[3] != 2:
            raise ValueError(f"initial_flow must be [T,H,W,2], got {tuple(init.shape)}")
        T, H, W, _ = init.shape
        top = self.flow_plan(H, W, pyr_scale, levels)[0]
        out = torch.empty((T, top["h"], top["w"], 2), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_flow_initial_level(self.h, _ptr(init), T, H, W, float(pyr_scale), int(levels), _ptr(out), _stream()),
                    "relax_flow_initial_level")
        return out

    def flow_gauss_window(self, winsize):
        """The half window of flags 256 (relax_flow_gauss_window; no GPU work) -> numpy float32 [winsize // 2 + 1], centre first."""
        k = np.zeros(max(int(winsize) // 2 + 1, 1), dtype=np.float32)
        if self.lib.relax_flow_gauss_window(int(winsize), k.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(f"relax_flow_gauss_window failed: {self.lib.relax_last_error(None).decode()}")
        return k

    def flow_area_table(self, src, dst):
        """cv::resize(INTER_AREA)'s table for one axis (relax_flow_area_table; no GPU work) -> (first int32 [dst], count int32 [dst],
        weights float64 [dst, src // dst + 2]): cell d is sum_j weights[d, j] * source[first[d] + j], j < count[d]."""
        src, dst = int(src), int(dst)
        n = max(dst, 1)
        first, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
        weights = np.zeros((n, src // n + 2), np.float64)
        if self.lib.relax_flow_area_table(src, dst, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                          weights.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(f"relax_flow_area_table failed: {self.lib.relax_last_error(None).decode()}")
        return first, count, weights

    def optical_flow_ex(self, frames, want_flow=False, want_image=True, **params):
        """optical_flow through relax_optical_flow_ex whatever the parameters are (missing ones: the literals) - what a test of the
        literal route calls."""
        unknown = set(params) - set(self.FLOW_DEFAULTS)
        if unknown:
            raise TypeError(f"optical_flow_ex: unknown parameters {sorted(unknown)}")
        return self._optical_flow(frames, want_flow, want_image, {**self.FLOW_DEFAULTS, **params})

    def flow_plan(self, H, W, pyr_scale=0.5, levels=3):
        """The pyramid calcOpticalFlowFarneback builds for H x W frames (relax_flow_plan; no GPU work) -> list of dict(h, w, ksize,
        sigma), coarsest level first, the full-size level last: len - 1 is the number of levels used below it (OpenCV stops before a
        side falls under 32 pixels)."""
        n = C.c_int(0)
        hwk = (C.c_int32 * (3 * 9))()
        sig = (C.c_double * 9)()
        rc = self.lib.relax_flow_plan(int(H), int(W), float(pyr_scale), int(levels), C.byref(n), C.cast(hwk, C.c_void_p), C.cast(sig, C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"relax_flow_plan failed ({rc}): {self.lib.relax_last_error(None).decode()}")
        return [dict(h=hwk[3 * i], w=hwk[3 * i + 1], ksize=hwk[3 * i + 2], sigma=sig[i]) for i in range(n.value + 1)]

    def _optical_flow(self, frames, want_flow, want_image, params):
        frames = self._dev_u8(frames)
        if frames.dim() != 5 or frames.shape[1] != 2 or frames.shape[4] != 3:
            raise ValueError(f"frames must be [T,2,H,W,3], got {tuple(frames.shape)}")
        T, _, H, W, _ = frames.shape
        fl = torch.empty((T, H, W, 2), dtype=torch.float32, device=self.device) if want_flow else None
        im = torch.empty((T, H, W, 3), dtype=torch.uint8, device=self.device) if want_image else None
        fb = H * W * 3
        base = frames.data_ptr()
        if params is None:
            rc = self.lib.relax_optical_flow(self.h, C.c_void_p(base), C.c_void_p(base + fb), 2 * fb, T, H, W, _ptr(fl), _ptr(im),
                                             _stream())
            self._check(rc, "relax_optical_flow")
            return fl, im
        rc = self.lib.relax_optical_flow_ex(self.h, C.c_void_p(base), C.c_void_p(base + fb), 2 * fb, T, H, W, float(params["pyr_scale"]),
                                            int(params["levels"]), int(params["winsize"]), int(params["iterations"]), int(params["poly_n"]),
                                            float(params["poly_sigma"]), int(params["flags"]), _ptr(fl), _ptr(im), _stream())
        self._check(rc, "relax_optical_flow_ex")
        return fl, im

    def flow_to_rgb(self, flow):
        """flow fp32 [T,H,W,2] -> uint8 [T,H,W,3] (src/main_fragment_layerstack.py:162-175)."""
        flow = flow.to(self.device, torch.float32).contiguous()
        T, H, W, _ = flow.shape
        out = torch.empty((T, H, W, 3), dtype=torch.uint8, device=self.device)
        self._check(self.lib.relax_flow_to_rgb(self.h, _ptr(flow), T, H, W, _ptr(out), _stream()), "relax_flow_to_rgb")
        return out

    def resize_frames(self, frames, bilinear=True, lanczos=True, out_bilinear=None, out_lanczos=None):
        """frames uint8 [N,H,W,3] -> (bilinear, lanczos) uint8 [N,224,224,3] each (None if not requested), bit-identical
        to PIL's Image.resize((224,224), BILINEAR / LANCZOS) (the reference's whole-frame inputs; relax_resize_frames)."""
        return self._resize_frames("resize_frames", frames, None, bilinear, lanczos, out_bilinear, out_lanczos)

    def resize_output_size(self, H, W, size):
        """(out_h, out_w) that transforms.Resize(size), size an int, gives a PIL image of H x W: the shorter side becomes size, the
        longer int(size * long / short) (torchvision's _compute_resized_output_size; relax_resize_output_size)."""
        oh, ow = C.c_int(0), C.c_int(0)
        rc = self.lib.relax_resize_output_size(int(H), int(W), int(size), C.byref(oh), C.byref(ow))
        if rc != 0:
            raise RuntimeError(f"relax_resize_output_size failed ({rc}): {self.lib.relax_last_error(None).decode()}")
        return oh.value, ow.value

    def _resize_target(self, H, W, size):
        """size: an int (the shorter-side rule of resize_output_size) or an (h, w) pair -> (out_h, out_w)"""
        if isinstance(size, (int, np.integer)):
            return self.resize_output_size(H, W, size)
        oh, ow = size
        return int(oh), int(ow)

    def _resize_outputs(self, what, n, oh, ow, bilinear, lanczos, out_bilinear, out_lanczos):
        outs = []
        for want, given in ((bilinear, out_bilinear), (lanczos, out_lanczos)):
            o = (given if given is not None else torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=self.device)) if want else None
            if o is not None and (o.dtype != torch.uint8 or tuple(o.shape) != (n, oh, ow, 3) or not o.is_contiguous() or not o.is_cuda):
                raise ValueError(f"{what}: output buffers must be contiguous device uint8 [{n},{oh},{ow},3]")
            outs.append(o)
        return outs

    def resize_frames_to(self, frames, size, bilinear=True, lanczos=True, out_bilinear=None, out_lanczos=None):
        """frames uint8 [N,H,W,3] -> (bilinear, lanczos) uint8 [N,out_h,out_w,3] each (None if not requested), bit-identical to
        PIL's Image.resize((out_w,out_h), BILINEAR / LANCZOS), down, up or mixed (relax_resize_frames_ex).  size: an int - the
        shorter side becomes size, as transforms.Resize(size) does it (resize_output_size) - or an (h, w) pair.  Items may be
        strided as in resize_frames."""
        return self._resize_frames("resize_frames_to", frames, size, bilinear, lanczos, out_bilinear, out_lanczos)

    def _resize_frames(self, what, frames, size, bilinear, lanczos, out_bilinear, out_lanczos):
        """size None: 224 x 224 through relax_resize_frames (its width limit and message), otherwise relax_resize_frames_ex"""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        frames = frames.to(self.device, non_blocking=True)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"frames must be uint8 [N,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
        N, H, W, _ = frames.shape
        oh, ow = (TARGET, TARGET) if size is None else self._resize_target(H, W, size)
        if frames.stride()[1:] != (W * 3, 3, 1):      # items may be strided (e.g. clip[:, 0]); pixels must be packed
            frames = frames.contiguous()
        item_stride = frames.stride(0) if N > 1 else H * W * 3
        ob, ol = self._resize_outputs(what, N, oh, ow, bilinear, lanczos, out_bilinear, out_lanczos)
        src, outs = (self.h, _ptr(frames), item_stride, N, H, W), (_ptr(ob), _ptr(ol), _stream())
        if size is None:
            self._check(self.lib.relax_resize_frames(*src, *outs), "relax_resize_frames")
        else:
            self._check(self.lib.relax_resize_frames_ex(*src, oh, ow, *outs), "relax_resize_frames_ex")
        return ob, ol

    def residual_resize(self, frames, bilinear=True, lanczos=True, want_residual=False, out_bilinear=None, out_lanczos=None, size=None):
        """frames uint8 [T,2,H,W,3] as fragment_pairs takes them -> (bilinear, lanczos, residual): the two uint8 [T,224,224,3]
        resizes of the WHOLE frame difference cv2.absdiff(next, orig) (src/main_residual.py:223-231), bit-identical to
        resize_frames on that image, and the uint8 [T,H,W,3] difference image itself; None for any output not requested.
        One launch reads each pair once (relax_resize_residual); without want_residual the difference never reaches memory.
        size (None: 224 x 224 through relax_resize_residual, its width limit and message): an int or an (h, w) pair as
        resize_frames_to takes it -> outputs [T,out_h,out_w,3] through relax_resize_residual_ex."""
        frames = self._dev_u8(frames)
        if frames.dim() != 5 or frames.shape[1] != 2 or frames.shape[4] != 3:
            raise ValueError(f"frames must be [T,2,H,W,3], got {tuple(frames.shape)}")
        T, _, H, W, _ = frames.shape
        oh, ow = (TARGET, TARGET) if size is None else self._resize_target(H, W, size)
        ob, ol = self._resize_outputs("residual_resize", T, oh, ow, bilinear, lanczos, out_bilinear, out_lanczos)
        res = torch.empty((T, H, W, 3), dtype=torch.uint8, device=self.device) if want_residual else None
        fb = H * W * 3
        base = frames.data_ptr()
        src, outs = (self.h, C.c_void_p(base), C.c_void_p(base + fb), 2 * fb, T, H, W), (_ptr(ob), _ptr(ol), _ptr(res), _stream())
        if size is None:
            self._check(self.lib.relax_resize_residual(*src, *outs), "relax_resize_residual")
        else:
            self._check(self.lib.relax_resize_residual_ex(*src, oh, ow, *outs), "relax_resize_residual_ex")
        return ob, ol, res

    # ---- stage B ------------------------------------------------------------------------------
    def _frags(self, frags):
        frags = self._dev_u8(frags)
        if frags.dim() == 3:
            frags = frags.unsqueeze(0)
        if tuple(frags.shape[1:]) != (TARGET, TARGET, 3):
            raise ValueError(f"fragments must be [N,224,224,3], got {tuple(frags.shape)}")
        return frags

    def resnet50_features(self, frags, layer_stack=True, pool=True, taps=None):
        """frags uint8 [N,224,224,3] BGR -> (layer_stack fp32 [N,13120] | None, pool fp32 [N,2051] | None[, taps]).
        taps: optional iterable of tap indices (0..14) whose full activations [N,C,H,W] are returned too."""
        frags = self._frags(frags)
        N = frags.shape[0]
        dev = self.device
        ls = torch.empty((N, LAYER_STACK_DIM), dtype=torch.float32, device=dev) if layer_stack else None
        pl = torch.empty((N, RN50_POOL_DIM), dtype=torch.float32, device=dev) if pool else None
        tap_out, tap_ptrs = {}, None
        if taps is not None:
            arr = (C.c_void_p * 15)()
            for t in taps:
                c, s = RN50_TAP_SHAPES[t]
                tap_out[t] = torch.empty((N, c, s, s), dtype=torch.float32, device=dev)
                arr[t] = tap_out[t].data_ptr()
            tap_ptrs = arr
        rc = self.lib.relax_resnet50_features(self.h, _ptr(frags), N, _ptr(ls), _ptr(pl), tap_ptrs, _stream())
        self._check(rc, "relax_resnet50_features")
        return (ls, pl, tap_out) if taps is not None else (ls, pl)

    def vgg16_features(self, frags, layer_stack=True, pool=True, taps=None):
        """frags uint8 [N,224,224,3] BGR -> (layer_stack fp32 [N,4224] | None, pool fp32 [N,4099] | None[, taps]).
        taps: optional iterable of tap indices, 0..12 the convolutions (features[VGG16_FEATURE_INDEX[i]], [N,C,H,W]), 13 fc1 and
        14 fc2 ([N,4096]); every tap is post-ReLU, as the reference's hooks read it."""
        frags = self._frags(frags)
        N = frags.shape[0]
        dev = self.device
        ls = torch.empty((N, VGG16_LAYER_STACK_DIM), dtype=torch.float32, device=dev) if layer_stack else None
        pl = torch.empty((N, VGG16_POOL_DIM), dtype=torch.float32, device=dev) if pool else None
        tap_out, tap_ptrs = {}, None
        if taps is not None:
            arr = (C.c_void_p * 15)()
            for t in taps:
                if t < 13:
                    c, s = VGG16_TAP_SHAPES[t]
                    tap_out[t] = torch.empty((N, c, s, s), dtype=torch.float32, device=dev)
                else:
                    tap_out[t] = torch.empty((N, 4096), dtype=torch.float32, device=dev)
                arr[t] = tap_out[t].data_ptr()
            tap_ptrs = arr
        rc = self.lib.relax_vgg16_features(self.h, _ptr(frags), N, _ptr(ls), _ptr(pl), tap_ptrs, _stream())
        self._check(rc, "relax_vgg16_features")
        return (ls, pl, tap_out) if taps is not None else (ls, pl)

    def resnet50_clip_features(self, frags, n_layer_stack):
        """frags uint8 [N,224,224,3]: the first n_layer_stack images are original fragments (-> layer stack fp32
        [n_layer_stack,13120]), the others residual fragments (-> pool fp32 [N - n_layer_stack, 2051]); ONE forward
        (src/main_fragment_layerstack.py:327-328).  Same values as resnet50_features on the respective images."""
        frags = self._frags(frags)
        N = frags.shape[0]
        n_ls = int(n_layer_stack)
        if not 0 <= n_ls <= N:
            raise ValueError(f"n_layer_stack={n_ls} outside [0, {N}]")
        ls = torch.empty((n_ls, LAYER_STACK_DIM), dtype=torch.float32, device=self.device)
        pl = torch.empty((N - n_ls, RN50_POOL_DIM), dtype=torch.float32, device=self.device)
        rc = self.lib.relax_resnet50_clip_features(self.h, _ptr(frags), N, n_ls, _ptr(ls) if n_ls else None, _ptr(pl) if N > n_ls else None,
                                                   _stream())
        self._check(rc, "relax_resnet50_clip_features")
        return ls, pl

    # ---- ResNet-50 on any canvas ---------------------------------------------------------------
    def resnet50_canvas_geometry(self, Hc, Wc, any_size=False):
        """-> ([(h, w)] * 15: the map of every tap on an [Hc, Wc] canvas, arena bytes per image).  Accepted: Hc and Wc multiples of 32 in
        [64, 1024] (every stage map even down to layer4, the stem's output whole 256-pixel tiles); anything else is a ValueError that names
        the offending value.  any_size=True (RELAX_RN_CANVAS_ANY): every Hc, Wc in [64, 1024], the maps by torch's floor rule (65 x 67: 33 x 34,
        17 x 17, 9 x 9, 5 x 5, 3 x 3).  Host arithmetic: no model needs to be loaded."""
        taps = (C.c_int * 30)()
        arena = C.c_int64(0)
        if any_size:
            rc = self.lib.relax_resnet50_canvas_geometry_ex(int(Hc), int(Wc), RN_CANVAS_ANY, taps, C.byref(arena))
        else:
            rc = self.lib.relax_resnet50_canvas_geometry(int(Hc), int(Wc), taps, C.byref(arena))
        if rc != 0:
            raise ValueError(self.lib.relax_last_error(None).decode())
        return [(taps[2 * t], taps[2 * t + 1]) for t in range(15)], int(arena.value)

    def resnet50_canvas(self):
        """(Hc, Wc) the ResNet-50 entries run at: 224 x 224 unless a *_canvas method is under way."""
        hc, wc = C.c_int(0), C.c_int(0)
        self._check(self.lib.relax_resnet50_get_canvas(self.h, C.byref(hc), C.byref(wc)), "relax_resnet50_get_canvas")
        return hc.value, wc.value

    def _rn_set_canvas(self, Hc, Wc, any_size):
        if any_size:
            self._check(self.lib.relax_resnet50_set_canvas_ex(self.h, Hc, Wc, RN_CANVAS_ANY), "relax_resnet50_set_canvas_ex")
        else:
            self._check(self.lib.relax_resnet50_set_canvas(self.h, Hc, Wc), "relax_resnet50_set_canvas")

    def _rn_canvas_images(self, images):
        images = self._dev_u8(images)
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if images.dim() != 4 or images.shape[3] != 3 or images.shape[0] < 1:
            raise ValueError(f"images must be [N,Hc,Wc,3], got {tuple(images.shape)}")
        return images

    def resnet50_features_canvas(self, images, layer_stack=True, pool=True, taps=None, any_size=False):
        """images uint8 [N,Hc,Wc,3] BGR on any accepted canvas (resnet50_canvas_geometry) -> what resnet50_features returns: (layer_stack fp32
        [N,13120] | None, pool fp32 [N,2051] | None[, taps]), the exported taps [N,C,h_t,w_t] of that canvas.  torchvision's ResNet-50 takes
        any size; both rows are spatial means and keep their widths.  At 224 x 224 this is resnet50_features, launch for launch.  The canvas is
        set on the handle for this call and 224 x 224 (with the default rule) put back when it returns or raises, so every other method keeps
        finding the default.  any_size=True: every canvas in [64, 1024] (resnet50_canvas_geometry); on a canvas the default rule takes, the
        same launches and bits as without it."""
        images = self._rn_canvas_images(images)
        N, Hc, Wc = (int(v) for v in images.shape[:3])
        shapes = self.resnet50_canvas_geometry(Hc, Wc, any_size)[0]       # (a refused canvas: ValueError naming the value, the handle untouched)
        try:
            self._rn_set_canvas(Hc, Wc, any_size)
            dev = self.device
            ls = torch.empty((N, LAYER_STACK_DIM), dtype=torch.float32, device=dev) if layer_stack else None
            pl = torch.empty((N, RN50_POOL_DIM), dtype=torch.float32, device=dev) if pool else None
            tap_out, tap_ptrs = {}, None
            if taps is not None:
                arr = (C.c_void_p * 15)()
                for t in taps:
                    c, (th, tw) = RN50_TAP_SHAPES[t][0], shapes[t]
                    tap_out[t] = torch.empty((N, c, th, tw), dtype=torch.float32, device=dev)
                    arr[t] = tap_out[t].data_ptr()
                tap_ptrs = arr
            rc = self.lib.relax_resnet50_features(self.h, _ptr(images), N, _ptr(ls), _ptr(pl), tap_ptrs, _stream())
            self._check(rc, "relax_resnet50_features")
        finally:
            self.lib.relax_resnet50_set_canvas(self.h, TARGET, TARGET)
        return (ls, pl, tap_out) if taps is not None else (ls, pl)

    def resnet50_clip_features_canvas(self, images, n_layer_stack, any_size=False):
        """resnet50_clip_features on any accepted canvas: images uint8 [N,Hc,Wc,3], the first n_layer_stack -> layer stack fp32
        [n_layer_stack,13120], the others -> pool fp32 [N - n_layer_stack,2051]; ONE forward.  224 x 224 is put back as in
        resnet50_features_canvas."""
        images = self._rn_canvas_images(images)
        N, Hc, Wc = (int(v) for v in images.shape[:3])
        n_ls = int(n_layer_stack)
        if not 0 <= n_ls <= N:
            raise ValueError(f"n_layer_stack={n_ls} outside [0, {N}]")
        self.resnet50_canvas_geometry(Hc, Wc, any_size)
        try:
            self._rn_set_canvas(Hc, Wc, any_size)
            ls = torch.empty((n_ls, LAYER_STACK_DIM), dtype=torch.float32, device=self.device)
            pl = torch.empty((N - n_ls, RN50_POOL_DIM), dtype=torch.float32, device=self.device)
            rc = self.lib.relax_resnet50_clip_features(self.h, _ptr(images), N, n_ls, _ptr(ls) if n_ls else None, _ptr(pl) if N > n_ls else None,
                                                       _stream())
            self._check(rc, "relax_resnet50_clip_features")
        finally:
            self.lib.relax_resnet50_set_canvas(self.h, TARGET, TARGET)
        return ls, pl

    def _canvas(self, images):
        """-> (uint8 [N,Hc,Wc,3] on the device, ntok of that canvas under the loaded ViT)"""
        if self.vit_dim is None:
            raise RuntimeError("load_vit first")
        images = self._dev_u8(images)
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if images.dim() != 4 or images.shape[3] != 3 or images.shape[0] < 1:
            raise ValueError(f"images must be [N,Hc,Wc,3], got {tuple(images.shape)}")
        if tuple(images.shape[1:3]) == (TARGET, TARGET):
            return images, self.vit_ntok
        return images, self.vit_canvas_geometry(images.shape[1], images.shape[2])[2]

    def vit_features(self, frags, tokens=False, pooled=True, attention=False):
        """frags uint8 [N,Hc,Wc,3] BGR, any canvas (vit_canvas_geometry: gh x gw = npatch patches, the position table resampled onto that grid
        as the reference's prepare_tokens does, src/extractor/visualise_vit_layer.py:197-232) -> (tokens fp32 [N,npatch,dim] | None, pooled fp32
        [N,3*dim] | None); at 224 x 224 npatch = 196, or 784 with a patch-8 model.  attention=True adds a third element: the last block's CLS
        attention to the patches, fp32 [N,heads,npatch] (src/extractor/visualise_vit.py:241-250,353-369: attn[:, :, 0, 1:]); tokens and
        pooled are unchanged by it."""
        frags, ntok = self._canvas(frags)
        N, Hc, Wc, _ = frags.shape
        dev = self.device
        tk = torch.empty((N, ntok - 1, self.vit_dim), dtype=torch.float32, device=dev) if tokens else None
        pl = torch.empty((N, 3 * self.vit_dim), dtype=torch.float32, device=dev) if pooled else None
        at = torch.empty((N, self.vit_dim // 64, ntok), dtype=torch.float32, device=dev) if attention else None
        if tk is None and pl is None and at is None:
            raise ValueError("vit_features: no output requested")
        self._check(self.lib.relax_vit_features_canvas(self.h, _ptr(frags), N, Hc, Wc, _ptr(tk), _ptr(pl), _ptr(at), _stream()),
                    "relax_vit_features_canvas")
        return (tk, pl, at[:, :, 1:]) if attention else (tk, pl)

    def vit_attention(self, frags, with_cls=False):
        """frags uint8 [N,Hc,Wc,3] BGR (any canvas, as vit_features) -> fp32 [N,heads,npatch]: get_last_selfattention's CLS row without the
        CLS column (src/extractor/visualise_vit.py:241-250,353-369).  The forward stops after the last block's qkv GEMM.
        with_cls=True returns the whole row [N,heads,ntok] (column 0 = the CLS key; each row sums to 1).  At 224 x 224 npatch / ntok =
        196 / 197, or 784 / 785 with a patch-8 model."""
        frags, ntok = self._canvas(frags)
        N, Hc, Wc, _ = frags.shape
        at = torch.empty((N, self.vit_dim // 64, ntok), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_vit_features_canvas(self.h, _ptr(frags), N, Hc, Wc, None, None, _ptr(at), _stream()),
                    "relax_vit_features_canvas")
        return at if with_cls else at[:, :, 1:]

    def vit_intermediate_layers(self, frags, n=1, tokens=False, cls=True, pooled=True):
        """VisionTransformer.get_intermediate_layers(x, n) (src/extractor/visualise_vit_layer.py:252-260): the final norm of the output of
        each of the last n blocks, from ONE forward.  frags uint8 [N,Hc,Wc,3] BGR, any canvas (as vit_features) -> dict of the requested
        'tokens' fp32 [n,N,ntok,dim] (row 0 the CLS token), 'cls' fp32 [n,N,dim], 'pooled' fp32 [n,N,3*dim] (mean | max | std over the
        patch tokens); tap k is block depth - n + k, so the last one is vit_features' norm (tokens[-1][:, 1:] and pooled[-1] are its bits).
        n outside [1, depth] is refused by the library (RuntimeError naming n)."""
        frags, ntok = self._canvas(frags)
        N, Hc, Wc, _ = frags.shape
        n = int(n)
        if not (tokens or cls or pooled):
            raise ValueError("vit_intermediate_layers: no output requested")
        rows = max(n, 0)   # (the library names a bad n; nothing is allocated for it)
        dev, dim = self.device, self.vit_dim
        out = {}
        if tokens:
            out["tokens"] = torch.empty((rows, N, ntok, dim), dtype=torch.float32, device=dev)
        if cls:
            out["cls"] = torch.empty((rows, N, dim), dtype=torch.float32, device=dev)
        if pooled:
            out["pooled"] = torch.empty((rows, N, 3 * dim), dtype=torch.float32, device=dev)
        self._check(self.lib.relax_vit_intermediate_layers(self.h, _ptr(frags), N, Hc, Wc, n, _ptr(out.get("tokens")), _ptr(out.get("cls")),
                                                           _ptr(out.get("pooled")), _stream()), "relax_vit_intermediate_layers")
        return out

    def attention_overlay(self, frames, positions, counts, patch_values, lut=None, patch_size=16):
        """map_attention_to_original (src/demo_visual.py:12-25) on the GPU.
        frames uint8 [T,H,W,3] BGR (items may be strided, pixels packed); positions int32 [T,slots,2] / counts int32 [T] as
        fragment_pairs returns them at this patch_size (8 / 16 / 32; the slot count is read from positions: 196 at 16 / 224);
        patch_values fp32 [T,slots] in slot order; lut uint8 [256,3] BGR (None: colormap.jet_lut_bgr(),
        see there for passing cv2's own table) -> uint8 [T,H,W,3] = 0.6 frame + 0.4 lut[level] (csrc/vit_attention_map.hip).
        With a ViT loaded, patch_size has to agree with it by fragment_geometry.overlay_slot_rule (one slot per token: a patch-8 model
        takes patch_size=8, 784 slots; a 16 x 16 fragment under it raises ValueError; 32 goes with either model)."""
        self._overlay_tokens_per_slot("attention_overlay", patch_size)
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        frames = frames.to(self.device, non_blocking=True)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"frames must be uint8 [T,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
        T, H, W, _ = frames.shape
        if frames.stride()[1:] != (W * 3, 3, 1):
            frames = frames.contiguous()
        positions = torch.as_tensor(positions).to(self.device, torch.int32).contiguous()
        counts = torch.as_tensor(counts).to(self.device, torch.int32).contiguous()
        values = torch.as_tensor(patch_values).to(self.device, torch.float32).contiguous()
        slots = int(positions.shape[1]) if positions.dim() == 3 else -1
        if slots < 1 or tuple(positions.shape) != (T, slots, 2) or tuple(counts.shape) != (T,) or tuple(values.shape) != (T, slots):
            raise ValueError(f"attention_overlay: positions [T,slots,2], counts [T], patch_values [T,slots] expected for T={T}, got "
                             f"{tuple(positions.shape)}, {tuple(counts.shape)}, {tuple(values.shape)}")
        if lut is None:
            if getattr(self, "_jet_lut", None) is None:
                self._jet_lut = torch.from_numpy(colormap.jet_lut_bgr()).to(self.device)
            lut = self._jet_lut
        else:
            lut = torch.as_tensor(np.asarray(lut) if not torch.is_tensor(lut) else lut).to(self.device).contiguous()
            if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
                raise ValueError(f"lut must be uint8 [256,3] BGR, got {lut.dtype} {tuple(lut.shape)}")
        out = torch.empty((T, H, W, 3), dtype=torch.uint8, device=self.device)
        stride = frames.stride(0) if T > 1 else H * W * 3
        rc = self.lib.relax_attention_overlay_ex(self.h, _ptr(frames), stride, T, H, W, int(patch_size), slots, _ptr(positions), _ptr(counts),
                                                 _ptr(values), _ptr(lut), _ptr(out), _stream())
        self._check(rc, "relax_attention_overlay")
        return out

    def _overlay_tokens_per_slot(self, what, patch_size):
        """fragment_geometry.overlay_slot_rule against the loaded ViT (no model loaded: nothing to disagree with)."""
        fragment_geometry(patch_size, patch_size)
        if self.vit_patch is None:
            return 1
        try:
            return overlay_slot_rule(int(patch_size), self.vit_patch)
        except ValueError as e:
            raise ValueError(f"{what}: {e} ({self.vit_npatch} patch tokens)") from None

    OVERLAY_FRAGMENTS = ("residual_imp", "residual_of_imp", "ori_frag", "residual_merged_frag")

    def attention_overlays(self, frames, fragment="ori_frag", flow_images=None, lut=None, patch_size=16, top_n=None, target_size=None,
                           flow_params=None):
        """The __main__ of src/demo_visual.py (:86-128) for a whole clip: frames uint8 [T,2,H,W,3] as fragment_pairs takes them;
        fragment one of OVERLAY_FRAGMENTS:
          residual_imp          the frame-difference fragment, frame-difference positions
          ori_frag              the original fragment, frame-difference positions
          residual_merged_frag  merge_fragments(difference fragment, flow fragment), frame-difference positions
          residual_of_imp       the flow fragment, flow positions (flow_images, or Farneback on the GPU when None; flow_params: a dict
                                of optical_flow's keywords for it, None = the reference's literals)
        patch_size / top_n: the fragment's geometry on the 224 x 224 canvas (slots = (224 / patch_size)^2: 784 / 196 / 49; top_n=None
        = all).  patch_size must go with the loaded ViT (fragment_geometry.overlay_slot_rule): equal to its patch size - a patch-8
        model with patch_size=8 paints its 784 tokens one to one -, or 32, where a slot takes the mean of the head-mean attention
        of the tokens it covers (get_activation_png's reshape-and-mean, src/demo_visual.py:41-60).
        -> dict(overlay uint8 [T,H,W,3] over frames[:, 0], patch_means fp32 [T,slots] (head mean, slot order),
                attention fp32 [T,heads,npatch], positions, counts)."""
        if fragment not in self.OVERLAY_FRAGMENTS:
            raise ValueError(f"fragment must be one of {self.OVERLAY_FRAGMENTS}, got {fragment!r}")
        geo = backbone_geometry(patch_size, top_n, target_size)
        if self.vit_dim is None:
            raise RuntimeError("load_vit first")
        per = self._overlay_tokens_per_slot("attention_overlays", geo.patch_size)
        kw = dict(patch_size=geo.patch_size, top_n=geo.top_n)
        frames = self._dev_u8(frames)
        fr = self.fragment_pairs(frames, **kw)
        positions, counts = fr["positions"], fr["counts"]
        if fragment in ("residual_of_imp", "residual_merged_frag"):
            if flow_images is None:
                flow_images = self.clip_flow_images(frames, flow_params)
            fl = self.fragment_image(flow_images, **kw)
        if fragment == "residual_imp":
            image = fr["diff_frag"]
        elif fragment == "ori_frag":
            image = fr["ori_frag"]
        elif fragment == "residual_merged_frag":
            image = self.merge_fragments(fr["diff_frag"], fl["frag"])
        else:
            image, positions, counts = fl["frag"], fl["positions"], fl["counts"]
        attention = self.vit_attention(image)
        patch_means = attention.mean(dim=1)
        if per > 1:      # a slot of per x per tokens: the mean of the block (file-free visualisation path: aten)
            side = geo.tiles_per_row
            patch_means = patch_means.view(-1, side, per, side, per).mean(dim=(2, 4)).reshape(-1, geo.slots)
        overlay = self.attention_overlay(frames[:, 0], positions, counts, patch_means, lut=lut, patch_size=geo.patch_size)
        return dict(overlay=overlay, patch_means=patch_means, attention=attention, positions=positions, counts=counts)

    # ---- whole clip ---------------------------------------------------------------------------
    def extract_clip(self, frames, resnet=True, vit=True, flow_images=None, flow=False, patch_size=16, top_n=None, target_size=None,
                     flow_params=None):
        """frames uint8 [T,2,H,W,3] on the device -> per-frame features (all fp32, on the device):
             resnet: [T,15171] = layer-stack of the original fragment | pool of the residual fragment
             vit:    [T,4608]  = pool of the original fragment | pool of the residual fragment
        The residual fragment is the frame-difference fragment, merged 50/50 with the optical-flow
        fragment when flow_images (uint8 [T,H,W,3]) are supplied (src/main_fragment_layerstack.py:313-325).
        patch_size / top_n: the fragments' geometry on the 224 x 224 canvas (8 / 16 / 32; top_n=None = all (224 / patch_size)^2 slots;
        positions come back as [T,slots,2]); target_size is refused: the clip paths cut 224 x 224 (fragment_geometry.backbone_geometry; other
        canvases: fragment_resnet_vectors / fragment_vit_vectors / fragment_canvas_vectors).
        flow_params: a dict of optical_flow's keywords for the flow computed here (flow=True without flow_images); None = the literals."""
        kw = self._clip_geometry(patch_size, top_n, target_size)
        fr = self.fragment_pairs(frames, **kw)
        resid = fr["diff_frag"]
        if flow and flow_images is None:
            flow_images = self.clip_flow_images(frames, flow_params)     # full ReLaX: Farneback + flow_to_rgb on the GPU
        if flow_images is not None:
            fl = self.fragment_image(flow_images, **kw)
            resid = self.merge_fragments(resid, fl["frag"])
        T = resid.shape[0]
        both = torch.cat([fr["ori_frag"], resid], dim=0)
        out = {"positions": fr["positions"], "counts": fr["counts"]}
        if resnet:
            ls, pool = self.resnet50_clip_features(both, T)
            out["resnet"] = torch.cat([ls, pool], dim=1)
        if vit:
            _, pooled = self.vit_features(both, tokens=False, pooled=True)
            out["vit"] = torch.cat([pooled[:T], pooled[T:]], dim=1)
        return out

    def fragment_vit_vectors(self, frames, patch_size=16, target_size=TARGET, top_n=None):
        """frames uint8 [T,2,H,W,3] -> fp32 [T, 6*dim]: the ViT pool of the original fragment | the pool of the frame-difference fragment, both
        cut by fragment_pairs at patch_size on a target_size x target_size canvas (any multiple of patch_size up to 448) and run through the ViT
        at that canvas - the row of extract_clip's 'vit' block, which is this at target_size 224."""
        fr = self.fragment_pairs(frames, top_n=top_n, patch_size=patch_size, target_size=target_size)
        T = fr["ori_frag"].shape[0]
        _, pooled = self.vit_features(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), tokens=False, pooled=True)
        return torch.cat([pooled[:T], pooled[T:]], dim=1)

    def fragment_resnet_vectors(self, frames, patch_size=16, target_size=TARGET, top_n=None, any_size=False):
        """frames uint8 [T,2,H,W,3] -> fp32 [T, 13120 + 2051]: the ResNet-50 layer stack of the original fragment | the pool of the
        frame-difference fragment, both cut by fragment_pairs at patch_size on a target_size x target_size canvas and run through ResNet-50 at
        that canvas in ONE forward - the row of extract_clip's 'resnet' block, which is this at target_size 224.  target_size: a multiple of
        patch_size (fragment_pairs) and of 32 (resnet50_canvas_geometry) up to 448; e.g. 232 at patch 8 is a fragment canvas but not a
        ResNet-50 one and is refused naming the value, before anything is cut - unless any_size=True, under which every fragment canvas in
        [64, 448] is a ResNet-50 one too."""
        self.resnet50_canvas_geometry(target_size, target_size, any_size)
        fr = self.fragment_pairs(frames, top_n=top_n, patch_size=patch_size, target_size=target_size)
        return self._fragment_resnet_row(fr, any_size)

    def _fragment_resnet_row(self, fr, any_size=False):
        T = fr["ori_frag"].shape[0]
        ls, pool = self.resnet50_clip_features_canvas(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), T, any_size=any_size)
        return torch.cat([ls, pool], dim=1)

    def fragment_canvas_vectors(self, frames, target_size, patch_size=16, top_n=None, any_size=False):
        """frames uint8 [T,2,H,W,3] -> fp32 [T, 15171 + 6*dim]: fragment_resnet_vectors | fragment_vit_vectors of the same fragments (ONE
        fragment_pairs call) - extract_clip's 'resnet' | 'vit' row on a canvas of the caller's choosing (a multiple of 32 and of patch_size, up
        to 448; any_size=True: a multiple of patch_size in [64, 448], e.g. 232 at patch 8)."""
        self.resnet50_canvas_geometry(target_size, target_size, any_size)
        fr = self.fragment_pairs(frames, top_n=top_n, patch_size=patch_size, target_size=target_size)
        T = fr["ori_frag"].shape[0]
        _, pooled = self.vit_features(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), tokens=False, pooled=True)
        return torch.cat([self._fragment_resnet_row(fr, any_size), pooled[:T], pooled[T:]], dim=1)

    def fragment_vit_layer_stack(self, frames, n=4, cls=False, patch_size=16, target_size=TARGET, top_n=None):
        """frames uint8 [T,2,H,W,3] -> fp32 [T, 2*n*3*dim] (+ 2*n*dim columns with cls=True): fragment_vit_vectors with the last n blocks'
        taps (vit_intermediate_layers) in place of the last block's pool.  Per fragment - the original, then the frame difference - the taps in
        block order, each tap its pooled row, or its CLS row | its pooled row with cls=True (DINO's linear-probe features).  n=1, cls=False is
        fragment_vit_vectors' row, bit for bit."""
        fr = self.fragment_pairs(frames, top_n=top_n, patch_size=patch_size, target_size=target_size)
        T = fr["ori_frag"].shape[0]
        out = self.vit_intermediate_layers(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), n=n, tokens=False, cls=cls, pooled=True)
        taps = torch.cat([out["cls"], out["pooled"]], dim=2) if cls else out["pooled"]       # [n, 2T, F]
        rows = taps.permute(1, 0, 2).reshape(2 * T, -1)                                        # a fragment's taps side by side
        return torch.cat([rows[:T], rows[T:]], dim=1)

    @staticmethod
    def _clip_geometry(patch_size, top_n, target_size):
        """The fragment keywords of a clip path (224 x 224 canvases for the backbones), checked."""
        geo = backbone_geometry(patch_size, top_n, target_size)
        return dict(patch_size=geo.patch_size, top_n=geo.top_n)

    def _segment_means(self, out, blocks, counts):
        """out [len(counts), F] <- per-clip means; blocks: list of (src [rows, cols] fp32, first row, dst column)."""
        offs = np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]), dtype=np.int32)   # host array, passed by value
        for src, row0, col0 in blocks:
            rc = self.lib.relax_segment_mean(self.h, _ptr(src), src.stride(0), src.shape[1], row0, C.c_void_p(offs.ctypes.data), len(counts),
                                             _ptr(out), out.stride(0), col0, _stream())
            self._check(rc, "relax_segment_mean")
        return out

    def clip_vectors(self, clips, resnet=True, vit=True, per_frame=False, patch_size=16, top_n=None, target_size=None):
        """Several clips (list of uint8 [T,2,H,W,3] device tensors, any mix of resolutions) in ONE batched pass of
        both backbones -> fp32 [len(clips), F] per-clip mean vectors.  Bigger batches fill the 256 CUs better
        (more tiles per launch, fewer partial rounds).  A clip's row equals the row it gets alone to fp32 rounding; it is
        bit-identical across batch compositions (and therefore across ranks of a sharded run) only with
        set_option("gemm_split_k", 0): the default tail split cuts the last tiles of a GEMM along K by the batch size.
        per_frame=True: -> (matrix, [fp32 [T_i, F] per clip]) - the per-frame rows the reference saves per video
        (src/main_fragment_layerstack.py:345-354) next to their means.  patch_size / top_n / target_size as in extract_clip."""
        kw = self._clip_geometry(patch_size, top_n, target_size)
        counts = [int(c.shape[0]) for c in clips]
        n = sum(counts)
        both = torch.empty((2 * n, TARGET, TARGET, 3), dtype=torch.uint8, device=self.device)   # [originals | residuals]
        at = 0
        for c, t in zip(clips, counts):
            self.fragment_pairs(c, out_ori=both[at:at + t], out_diff=both[n + at:n + at + t], **kw)
            at += t
        F = (LAYER_STACK_DIM + RN50_POOL_DIM if resnet else 0) + (6 * self.vit_dim if vit else 0)
        out = torch.empty((len(clips), F), dtype=torch.float32, device=self.device)
        blocks, col = [], 0
        if resnet:
            ls, pool = self.resnet50_clip_features(both, n)        # layer stack of the originals, pool of the residuals
            blocks += [(ls, 0, 0), (pool, 0, LAYER_STACK_DIM)]
            col = LAYER_STACK_DIM + RN50_POOL_DIM
        if vit:
            _, pooled = self.vit_features(both, tokens=False, pooled=True)
            blocks += [(pooled, 0, col), (pooled, n, col + 3 * self.vit_dim)]
        self._segment_means(out, blocks, counts)
        if not per_frame:
            return out
        return out, self._per_frame_rows(blocks, counts)

    def rows_mean(self, rows):
        """fp32 [T, F] device tensor of per-frame rows -> their mean [F], by the same kernel (relax_segment_mean: the rows of a
        column added in order, one division) that reduces freshly computed rows: the dataset driver's resume path uses it so that
        a row rebuilt from the per-frame files is bit-identical to the one the first run returned."""
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((1, rows.shape[1]), dtype=torch.float32, device=self.device)
        return self._segment_means(out, [(rows, 0, 0)], [int(rows.shape[0])])[0]

    @staticmethod
    def _per_frame_rows(blocks, counts):
        """blocks as for _segment_means -> per clip the [T, F] matrix of its frames (file output only: aten copies)."""
        rows, at = [], 0
        order = sorted(blocks, key=lambda b: b[2])
        for t in counts:
            rows.append(torch.cat([src[row0 + at:row0 + at + t] for src, row0, _ in order], dim=1))
            at += t
        return rows

    def whole_frame_features(self, frames):
        """frames uint8 [N,H,W,3] BGR (whole sampled frames) -> (ResNet-50 layer-stack fp32 [N,13120], ViT pooled
        fp32 [N,2304]): the per-frame features of src/main_layer_stack.py:81-151 / src/demo_test.py:81-87, with the
        Pillow-exact resizes done on the GPU."""
        bil, lan = self.resize_frames(frames)
        ls, _ = self.resnet50_features(bil, layer_stack=True, pool=False)
        _, vp = self.vit_features(lan, tokens=False, pooled=True)
        return ls, vp

    def whole_frame_vit_canvas(self, frames, size, tokens=False, pooled=True, attention=False):
        """frames uint8 [N,H,W,3] BGR -> vit_features of the frames LANCZOS-resized to the canvas `size` (an int: the shorter side, as
        transforms.Resize(size); or an (h, w) pair) on the GPU: the reference's whole-frame ViT input (img.resize(..., LANCZOS),
        src/extractor/visualise_vit_layer.py:466-473) at a size of the caller's choosing, e.g. 1080 x 1920 -> 270 x 480 = 481 tokens.
        size=(224, 224) is whole_frame_features' ViT half, through the same 224 kernels."""
        if not isinstance(size, (int, np.integer)) and tuple(int(v) for v in size) == (TARGET, TARGET):
            lan = self.resize_frames(frames, bilinear=False, lanczos=True)[1]
        else:
            lan = self.resize_frames_to(frames, size, bilinear=False, lanczos=True)[1]
        return self.vit_features(lan, tokens=tokens, pooled=pooled, attention=attention)

    def whole_frame_resnet_canvas(self, frames, size, layer_stack=True, pool=True, any_size=False):
        """frames uint8 [N,H,W,3] BGR -> resnet50_features_canvas of the frames BILINEAR-resized to the canvas `size` (an int: the shorter side,
        as transforms.Resize(size); or an (h, w) pair) on the GPU, Pillow-exact: the reference's whole-frame ResNet input (transforms.Resize,
        src/extractor/visualise_resnet.py:40-50) without squashing the frame to a square - for 16:9 frames (288, 512) keeps the aspect
        ratio on an accepted canvas.  A size whose result is not an accepted canvas (e.g. the int 288 on 1080 x 1920 -> 288 x 512 is, (270,
        480) is not) is refused naming the value, before anything is resized - unless any_size=True, under which every size in [64, 1024]
        is a canvas (1080 x 1920 -> (270, 480)).  size=(224, 224) is whole_frame_features' ResNet half."""
        if len(frames.shape) != 4 or frames.shape[3] != 3:
            raise ValueError(f"frames must be uint8 [N,H,W,3], got {tuple(frames.shape)}")
        oh, ow = self._resize_target(int(frames.shape[1]), int(frames.shape[2]), size)
        self.resnet50_canvas_geometry(oh, ow, any_size)
        bil = self.resize_frames_to(frames, (oh, ow), bilinear=True, lanczos=False)[0]
        return self.resnet50_features_canvas(bil, layer_stack=layer_stack, pool=pool, any_size=any_size)

    def whole_frame_canvas_vectors(self, frames, size):
        """frames uint8 [N,H,W,3] BGR -> fp32 [N, 13120 + 2051 + 3*dim]: both backbones on the SAME canvas `size` (an int: the shorter side; or an
        (h, w) pair; anything in [64, 1024] both ways) - whole_frame_resnet_canvas(any_size=True)'s layer stack | pool beside
        whole_frame_vit_canvas' pooled row, from ONE resize call that reads each frame once for both filters (ResNet-50 sees the BILINEAR canvas, the
        ViT the LANCZOS one, as the reference's whole-frame inputs).  E.g. 1080 x 1920 -> (270, 480); a 540 x 960 frame at its own size is not
        resized at all."""
        if self.vit_dim is None:
            raise RuntimeError("load_vit first")
        if len(frames.shape) != 4 or frames.shape[3] != 3:
            raise ValueError(f"frames must be uint8 [N,H,W,3], got {tuple(frames.shape)}")
        oh, ow = self._resize_target(int(frames.shape[1]), int(frames.shape[2]), size)
        self.resnet50_canvas_geometry(oh, ow, True)              # (refused before anything is resized)
        if (oh, ow) == (int(frames.shape[1]), int(frames.shape[2])):
            bil = lan = self._dev_u8(frames)
        else:
            bil, lan = self.resize_frames_to(frames, (oh, ow), bilinear=True, lanczos=True)
        ls, pool = self.resnet50_features_canvas(bil, any_size=True)
        _, pooled = self.vit_features(lan, tokens=False, pooled=True)
        return torch.cat([ls, pool, pooled], dim=1)

    # ---- fragment-free ablation rows (src/main_residual.py, src/main_layer.py) ---------------------------------
    RESIDUAL_NAMES = ("frame_diff", "optical_flow")

    def _whole_residual_inputs(self, frames, residual_name, bilinear, lanczos, flow_images=None, out_bilinear=None, out_lanczos=None,
                               flow_params=None):
        """The two backbone inputs of one clip's whole residual images: the frame difference through the fused
        difference + resize, the flow image (given, or Farneback on the GPU) through resize_frames."""
        if residual_name == "frame_diff":
            return self.residual_resize(frames, bilinear=bilinear, lanczos=lanczos, out_bilinear=out_bilinear,
                                        out_lanczos=out_lanczos)[:2]
        if flow_images is None:
            flow_images = self.clip_flow_images(frames, flow_params)
        return self.resize_frames(flow_images, bilinear=bilinear, lanczos=lanczos, out_bilinear=out_bilinear, out_lanczos=out_lanczos)

    def _check_residual_name(self, residual_name):
        if residual_name not in self.RESIDUAL_NAMES:
            raise ValueError(f"residual_name must be one of {self.RESIDUAL_NAMES}, got {residual_name!r}")

    @staticmethod
    def _check_backbones(resnet, vit, vgg16):
        if not (resnet or vit or vgg16):
            raise ValueError("no backbone requested")

    def _pool_blocks(self, bil, lan, resnet, vit, vgg16):
        """-> [(name, per-image pool rows)] in the column order resnet | vit | vgg16 of those requested."""
        blocks = []
        if resnet:
            blocks.append(("resnet", self.resnet50_features(bil, layer_stack=False, pool=True)[1]))
        if vit:
            blocks.append(("vit", self.vit_features(lan, tokens=False, pooled=True)[1]))
        if vgg16:
            blocks.append(("vgg16", self.vgg16_features(bil, layer_stack=False, pool=True)[1]))
        return blocks

    def whole_residual_features(self, frames, residual_name="frame_diff", resnet=True, vit=True, vgg16=False, flow_images=None, vit_size=None,
                                flow_params=None):
        """frames uint8 [T,2,H,W,3] -> dict of per-frame fp32 device tensors, the rows src/main_residual.py:221-254 saves per
        video: the WHOLE residual image (residual_name 'frame_diff': cv2.absdiff(next, orig); 'optical_flow': the flow image,
        flow_images uint8 [T,H,W,3] or Farneback on the GPU) resized to 224 x 224 and pooled:
          'resnet' [T,2051] avgpool | mean, max, std      'vgg16' [T,4099] fc2 | mean, max, std      (BILINEAR bytes)
          'vit'    [T,3*dim] token mean | max | std                                                  (LANCZOS bytes)
        vit_size (None: 224 x 224, the calls above unchanged): the ViT's canvas, an int or an (h, w) pair as resize_frames_to takes it.
        flow_params: a dict of optical_flow's keywords for the flow computed here ('optical_flow' without flow_images); None = the literals."""
        self._check_residual_name(residual_name)
        self._check_backbones(resnet, vit, vgg16)
        if vit_size is None or not vit:
            bil, lan = self._whole_residual_inputs(frames, residual_name, resnet or vgg16, vit, flow_images, flow_params=flow_params)
            return dict(self._pool_blocks(bil, lan, resnet, vit, vgg16))
        # the ViT's input on its own canvas (a second pass over the pairs); the BILINEAR 224 x 224 bytes of the other backbones as before
        if residual_name == "optical_flow" and flow_images is None:
            flow_images = self.clip_flow_images(frames, flow_params)
        bil = self._whole_residual_inputs(frames, residual_name, True, False, flow_images)[0] if resnet or vgg16 else None
        if residual_name == "frame_diff":
            lan = self.residual_resize(frames, bilinear=False, lanczos=True, size=vit_size)[1]
        else:
            lan = self.resize_frames_to(flow_images, vit_size, bilinear=False, lanczos=True)[1]
        return dict(self._pool_blocks(bil, lan, resnet, vit, vgg16))

    def whole_residual_vectors(self, clips, residual_name="frame_diff", resnet=True, vit=True, vgg16=False, flow_images=None,
                               per_frame=False, flow_params=None):
        """Several clips (list of uint8 [T_i,2,H_i,W_i,3], any mix of resolutions; flow_images: optional list of uint8
        [T_i,H_i,W_i,3]) in ONE batched pass per backbone -> fp32 [len(clips), F] per-clip means of the whole_residual_features
        rows, columns resnet | vit | vgg16 of those requested.  per_frame=True as in clip_vectors; flow_params as in whole_residual_features."""
        self._check_residual_name(residual_name)
        self._check_backbones(resnet, vit, vgg16)
        counts = [int(c.shape[0]) for c in clips]
        n = sum(counts)
        bil = torch.empty((n, TARGET, TARGET, 3), dtype=torch.uint8, device=self.device) if resnet or vgg16 else None
        lan = torch.empty((n, TARGET, TARGET, 3), dtype=torch.uint8, device=self.device) if vit else None
        at = 0
        for i, (c, t) in enumerate(zip(clips, counts)):
            self._whole_residual_inputs(c, residual_name, bil is not None, lan is not None,
                                        None if flow_images is None else flow_images[i],
                                        None if bil is None else bil[at:at + t], None if lan is None else lan[at:at + t], flow_params=flow_params)
            at += t
        blocks, col = [], 0
        for _, rows in self._pool_blocks(bil, lan, resnet, vit, vgg16):
            blocks.append((rows, 0, col))
            col += rows.shape[1]
        out = torch.empty((len(clips), col), dtype=torch.float32, device=self.device)
        self._segment_means(out, blocks, counts)
        if not per_frame:
            return out
        return out, self._per_frame_rows(blocks, counts)

    def whole_frame_pool_features(self, frames, resnet=True, vit=True, vgg16=False):
        """frames uint8 [N,H,W,3] BGR (whole sampled frames) -> dict of per-frame fp32 device tensors, the rows of
        src/main_layer.py:189-196: 'resnet' [N,2048] the avgpool vector WITHOUT the three statistics (:135-137), 'vgg16'
        [N,4096] fc2, 'vit' [N,3*dim] token mean | max | std - views of the backbones' pool outputs."""
        self._check_backbones(resnet, vit, vgg16)
        bil, lan = self.resize_frames(frames, bilinear=resnet or vgg16, lanczos=vit)
        out = dict(self._pool_blocks(bil, lan, resnet, vit, vgg16))
        if resnet:
            out["resnet"] = out["resnet"][:, :RN50_POOL_DIM - 3]
        if vgg16:
            out["vgg16"] = out["vgg16"][:, :VGG16_POOL_DIM - 3]
        return out

    def full_clip_vector(self, frames, flow_images=None, flow=False, whole_frames=None, patch_size=16, top_n=None, target_size=None,
                         flow_params=None):
        """frames uint8 [T,2,H,W,3] -> fp32 [35203]: the vector src/demo_test.py:171-175 assembles
        (whole-frame ResNet-50 LS | whole-frame ViT | fragment ResNet-50 LS+pool | fragment ViT x2), each part averaged
        over the sampled frames.  Without flow_images the residual fragment is the frame-difference fragment alone.
        whole_frames uint8 [Ts,H,W,3]: all sampled frames when the last one has no pair (see full_clip_vectors).
        With self.demo_write_png set, the pairs' files are written too (src/demo_test.py:120,135; at the reference's 16 / 196
        geometry whatever patch_size says); the vector is the same.  patch_size / top_n / target_size / flow_params as in extract_clip."""
        if self.demo_write_png is not None:
            from . import visualisation
            visualisation.write_for_driver(self, frames, self.demo_write_png, flow=flow or flow_images is not None)
        return self.full_clip_vectors([frames], flow=flow, flow_images=None if flow_images is None else [flow_images],
                                      whole_frames=None if whole_frames is None else [whole_frames], patch_size=patch_size, top_n=top_n,
                                      target_size=target_size, flow_params=flow_params)[0]

    def full_clip_vectors(self, clips, flow=True, flow_images=None, whole_frames=None, patch_size=16, top_n=None, target_size=None,
                          flow_params=None):
        """Several clips -> fp32 [len(clips), 35203] in ONE batched pass of each backbone (3*T fragments / frames per
        clip: original fragment, residual fragment, whole frame).  Same layout as full_clip_vector.  Batch-invariant to
        fp32 rounding; bit for bit only with set_option("gemm_split_k", 0) (see clip_vectors).
        whole_frames: optional list of uint8 [Ts,H,W,3] per clip - ALL sampled frames (src/demo_test.py:76-87 averages the
        whole-frame features over every sampled frame, including a last one that has no `next` partner and therefore no
        pair); default: the first frame of every pair.
        = full_features(full_prepare(...)): full_prepare is the byte / HBM work (fragments, Farneback flow, resizes), full_features
        the contractions.  Running the two halves of consecutive batches on two streams was measured at 1.01 x
        (tools/flow_overlap_try.py) and is not done in the product; the split stays because the dataset driver stages on it.
        patch_size / top_n / target_size / flow_params as in extract_clip."""
        return self.full_features(self.full_prepare(clips, flow=flow, flow_images=flow_images, whole_frames=whole_frames,
                                                    patch_size=patch_size, top_n=top_n, target_size=target_size, flow_params=flow_params))

    def full_prepare(self, clips, flow=True, flow_images=None, whole_frames=None, patch_size=16, top_n=None, target_size=None,
                     flow_params=None):
        """The input half of full_clip_vectors: fragments (difference + flow, merged), whole-frame resizes -> the two backbone
        input batches.  Everything is enqueued on the current stream."""
        kw = self._clip_geometry(patch_size, top_n, target_size)
        counts = [int(c.shape[0]) for c in clips]
        wf = [c[:, 0] for c in clips] if whole_frames is None else list(whole_frames)
        wcounts = [int(w.shape[0]) for w in wf]
        n, nw = sum(counts), sum(wcounts)
        # ResNet batch: the layer-stack images first [ori | bilinear whole frames], then the pool images [residual]
        rn_in = torch.empty((2 * n + nw, TARGET, TARGET, 3), dtype=torch.uint8, device=self.device)
        vit_in = torch.empty((2 * n + nw, TARGET, TARGET, 3), dtype=torch.uint8, device=self.device)  # [ori | residual | lanczos]
        frag_bytes = TARGET * TARGET * 3
        at = aw = 0
        for i, (c, t) in enumerate(zip(clips, counts)):
            res = vit_in[n + at:n + at + t]
            self.fragment_pairs(c, out_ori=vit_in[at:at + t], out_diff=res, **kw)
            fimg = None if flow_images is None else flow_images[i]
            if flow and fimg is None:
                fimg = self.clip_flow_images(c, flow_params)
            if fimg is not None:
                self.merge_fragments(res, self.fragment_image(fimg, **kw)["frag"], out=res)
            tw = wcounts[i]
            self.resize_frames(wf[i], out_bilinear=rn_in[n + aw:n + aw + tw], out_lanczos=vit_in[2 * n + aw:2 * n + aw + tw])
            at += t
            aw += tw
        # the fragments are the same for both backbones
        self._check(self.lib.relax_copy_bytes(self.h, _ptr(vit_in), _ptr(rn_in), n * frag_bytes, _stream()), "relax_copy_bytes")
        self._check(self.lib.relax_copy_bytes(self.h, _ptr(vit_in[n:]), _ptr(rn_in[n + nw:]), n * frag_bytes, _stream()), "relax_copy_bytes")
        return dict(rn_in=rn_in, vit_in=vit_in, counts=counts, wcounts=wcounts, n=n, nw=nw)

    def full_features(self, prep):
        """The backbone half of full_clip_vectors: prep from full_prepare (of this or another engine on the same device) ->
        fp32 [clips, 35203]."""
        rn_in, vit_in, counts, wcounts, n, nw = (prep[k] for k in ("rn_in", "vit_in", "counts", "wcounts", "n", "nw"))
        ls, pool = self.resnet50_clip_features(rn_in, n + nw)
        _, vp = self.vit_features(vit_in, tokens=False, pooled=True)
        d = self.vit_dim
        out = torch.empty((len(counts), LAYER_STACK_DIM + 3 * d + LAYER_STACK_DIM + RN50_POOL_DIM + 6 * d), dtype=torch.float32,
                          device=self.device)
        c0 = LAYER_STACK_DIM + 3 * d
        self._segment_means(out, [(ls, n, 0), (vp, 2 * n, LAYER_STACK_DIM)], wcounts)
        return self._segment_means(out, [(ls, 0, c0), (pool, 0, c0 + LAYER_STACK_DIM),
                                         (vp, 0, c0 + LAYER_STACK_DIM + RN50_POOL_DIM),
                                         (vp, n, c0 + LAYER_STACK_DIM + RN50_POOL_DIM + 3 * d)], counts)

    def clip_vector(self, frames, **kw):
        """Per-clip mean over frames of the concatenated features (src/demo_test.py:171-175)."""
        f = self.extract_clip(frames, **kw)
        parts = [f[k] for k in ("resnet", "vit") if k in f]
        out = torch.empty((1, sum(p.shape[1] for p in parts)), dtype=torch.float32, device=self.device)
        blocks, col = [], 0
        for p in parts:
            blocks.append((p, 0, col))
            col += p.shape[1]
        return self._segment_means(out, blocks, [int(parts[0].shape[0])])[0]

    # ---- operator level (tests / benches) -------------------------------------------------------
    def op_gemm(self, A, W, bias=None, residual=None, act=0, out=None):
        M, K = A.shape
        N = W.shape[0]
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_op_gemm(self.h, _ptr(A), _ptr(W), _ptr(bias), _ptr(residual), _ptr(out), M, N, K,
                                           act, _stream()), "relax_op_gemm")
        return out

    def op_conv2d_nhwc(self, x, w_packed, bias, residual, Cout, KH, KW, stride, pad, act):
        Nimg, H, W, Cin = x.shape
        Ho = (H + 2 * pad - KH) // stride + 1
        Wo = (W + 2 * pad - KW) // stride + 1
        out = torch.empty((Nimg, Ho, Wo, Cout), dtype=torch.float32, device=self.device)
        rc = self.lib.relax_op_conv2d_nhwc(self.h, _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(out),
                                           Nimg, H, W, Cin, Cout, KH, KW, stride, pad, act, _stream())
        self._check(rc, "relax_op_conv2d_nhwc")
        return out

    def op_conv2d_nhwc_ex(self, x, w_packed, bias, Cout, KH, KW, stride, pad, act=1, residual=None, residual_h2=None, img_res_inv=None,
                          out=True, out_h2=False, img_out_scale=None, amax=False, gap=False, gap_rows=0, out_rows=0, no_split=False,
                          w3=None, bias3=None):
        """relax_op_conv2d_nhwc_ex: the f16x2 convolution with the model drivers' epilogue outputs.  out / gap: True allocates, a
        tensor is filled in place (a test pre-fills it with a sentinel), False / None leaves the output out; out_h2: True allocates
        the planes as uint16 [M, 2 * Cn] (per 16 values: 16 x hi, 16 x lo), which needs img_out_scale [Nimg]; amax: the per-image
        maxima as int32 bits [Nimg]; w3 [Cout3, Cout] with bias3: the back-to-back form, every output then has Cn = Cout3 columns.
        Returns a dict: out [Nimg, Ho, Wo, Cn], out_h2, amax, gap [M / gap_group, Cn], gap_group."""
        Nimg, H, W, Cin = x.shape
        Ho = (H + 2 * pad - KH) // stride + 1
        Wo = (W + 2 * pad - KW) // stride + 1
        M = Nimg * Ho * Wo
        Cn = w3.shape[0] if w3 is not None else Cout
        wide = Cout % 256 == 0
        group = 4 if wide or (Ho * Wo) % 16 else 16
        if out is True:
            out = torch.empty((Nimg, Ho, Wo, Cn), dtype=torch.float32, device=self.device)
        elif out is False:
            out = None
        if gap is True:
            gap = torch.empty((M // group, Cn), dtype=torch.float32, device=self.device)
        elif gap is False:
            gap = None
        planes = torch.empty((M, 2 * Cn), dtype=torch.int16, device=self.device) if out_h2 else None
        mx = torch.empty(Nimg, dtype=torch.int32, device=self.device) if amax else None
        for t, shape in ((out, (Nimg, Ho, Wo, Cn)), (gap, (M // group, Cn)), (residual, (Nimg, Ho, Wo, Cn)), (residual_h2, (M, 2 * Cn)),
                         (img_out_scale, (Nimg,)), (img_res_inv, (Nimg,)), (bias, (Cout,)), (bias3, (Cn,)), (w3, (Cn, Cout)),
                         (w_packed, (Cout, KH * KW * Cin))):
            if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"op_conv2d_nhwc_ex: an operand of shape {tuple(t.shape)} where contiguous {shape} on {self.device} is expected")
        rc = self.lib.relax_op_conv2d_nhwc_ex(self.h, _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(residual_h2),
                                              _ptr(img_res_inv), _ptr(out), _ptr(planes), _ptr(img_out_scale), _ptr(mx), _ptr(gap),
                                              gap_rows, out_rows, int(bool(no_split)), _ptr(w3), _ptr(bias3), Cn if w3 is not None else 0,
                                              Nimg, H, W, Cin, Cout, KH, KW, stride, pad, act, _stream())
        self._check(rc, "relax_op_conv2d_nhwc_ex")
        return {"out": out, "out_h2": planes, "amax": mx, "gap": gap, "gap_group": group}

    def op_layernorm(self, x, g, b, eps):
        rows, dim = x.shape
        y = torch.empty_like(x)
        self._check(self.lib.relax_op_layernorm(self.h, _ptr(x), _ptr(g), _ptr(b), _ptr(y), rows, dim, eps, _stream()),
                    "relax_op_layernorm")
        return y

    def op_vit_norm_token_stats(self, x, g, b, eps, cls=True, pooled=True):
        """x fp32 [Nimg,ntok,dim] -> (the normed row 0 [Nimg,dim] | None, mean | max | std over the normed rows 1.. [Nimg,3*dim] | None): one
        tap of vit_intermediate_layers, the bits of op_layernorm followed by op_token_stats"""
        Nimg, ntok, dim = x.shape
        c = torch.empty((Nimg, dim), dtype=torch.float32, device=self.device) if cls else None
        p = torch.empty((Nimg, 3 * dim), dtype=torch.float32, device=self.device) if pooled else None
        self._check(self.lib.relax_op_vit_norm_token_stats(self.h, _ptr(x), _ptr(g), _ptr(b), eps, _ptr(c), _ptr(p), Nimg, ntok, dim, _stream()),
                    "relax_op_vit_norm_token_stats")
        return c, p

    def op_attention(self, qkv, n_img, heads):
        out = torch.empty((qkv.shape[0], heads * 64), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_op_attention(self.h, _ptr(qkv), _ptr(out), n_img, heads, _stream()),
                    "relax_op_attention")
        return out

    def op_attention_ex(self, qkv, n_img, ntok, heads):
        """The streaming attention kernel (csrc/attention_stream.hip) at any token count: qkv fp32 [n_img*ntok, 3*heads*64] ->
        fp32 [n_img*ntok, heads*64]; exact fp32 under "gemm_precision" 0 / 1, bf16x6 under 2, and under 3 the f16x2 streaming kernel
        (csrc/attention_stream_h2.hip) with the options "att_h2" and "att_h2_stream" on, bf16x6 otherwise (relax_op_attention_ex)."""
        if qkv.dim() != 2 or tuple(qkv.shape) != (n_img * ntok, 3 * heads * 64) or qkv.dtype != torch.float32:
            raise ValueError(f"op_attention_ex: qkv must be fp32 [{n_img * ntok}, {3 * heads * 64}], got {qkv.dtype} {tuple(qkv.shape)}")
        qkv = qkv.to(self.device).contiguous()
        out = torch.empty((qkv.shape[0], heads * 64), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_op_attention_ex(self.h, _ptr(qkv), _ptr(out), n_img, ntok, heads, _stream()),
                    "relax_op_attention_ex")
        return out

    def op_bn_relu_maxpool(self, x, scale, shift, amax_out=None):
        """amax_out: an int32 [Nimg] tensor that receives the bits of each image's largest output (relax_op_bn_relu_maxpool_amax)."""
        Nimg, H, W, Cc = x.shape
        y = torch.empty((Nimg, H // 2, W // 2, Cc), dtype=torch.float32, device=self.device)
        if amax_out is not None:
            if tuple(amax_out.shape) != (Nimg,) or amax_out.dtype != torch.int32 or amax_out.device != self.device:
                raise ValueError("op_bn_relu_maxpool: amax_out must be int32 [Nimg] on the engine's device")
            self._check(self.lib.relax_op_bn_relu_maxpool_amax(self.h, _ptr(x), _ptr(scale), _ptr(shift), _ptr(y), _ptr(amax_out), Nimg,
                                                           H, W, Cc, _stream()), "relax_op_bn_relu_maxpool_amax")
            return y
        self._check(self.lib.relax_op_bn_relu_maxpool(self.h, _ptr(x), _ptr(scale), _ptr(shift), _ptr(y), Nimg, H, W,
                                                      Cc, _stream()), "relax_op_bn_relu_maxpool")
        return y

    def op_gap(self, x, out=None):
        """x fp32 [Nimg,HW,C] -> the spatial means [Nimg,C]; out: a contiguous fp32 [Nimg, stride >= C] tensor whose rows receive them in
        their first C columns (the rest of each row is left as it is)"""
        Nimg, HW, Cc = x.shape
        if out is None:
            out = torch.empty((Nimg, Cc), dtype=torch.float32, device=self.device)
        elif (out.dim() != 2 or out.shape[0] != Nimg or out.shape[1] < Cc or out.dtype != torch.float32 or not out.is_contiguous()
              or out.device != self.device):
            raise ValueError(f"op_gap: out must be contiguous fp32 [{Nimg}, >= {Cc}] on {self.device}")
        self._check(self.lib.relax_op_gap(self.h, _ptr(x), _ptr(out), Nimg, HW, Cc, out.shape[1], _stream()), "relax_op_gap")
        return out

    def op_pool_stats(self, v, dim, out=None):
        """The tail of the pool vectors (relax_op_pool_stats): v contiguous fp32 [n, v_stride >= dim] -> out [n, out_stride >= dim + 3] with
        out[:, :dim] = v[:, :dim], then mean, max and population std of those dim values; dim 2048 or 4096.  Columns past dim + 2 of a
        given `out` are left as they are."""
        if v.dim() != 2 or v.dtype != torch.float32 or not v.is_contiguous() or v.device != self.device or v.shape[1] < dim:
            raise ValueError(f"op_pool_stats: v must be contiguous fp32 [n, >= {dim}] on {self.device}")
        n = v.shape[0]
        if out is None:
            out = torch.empty((n, dim + 3), dtype=torch.float32, device=self.device)
        elif (out.dim() != 2 or out.shape[0] != n or out.shape[1] < dim + 3 or out.dtype != torch.float32 or not out.is_contiguous()
              or out.device != self.device):
            raise ValueError(f"op_pool_stats: out must be contiguous fp32 [{n}, >= {dim + 3}] on {self.device}")
        self._check(self.lib.relax_op_pool_stats(self.h, _ptr(v), v.shape[1], _ptr(out), out.shape[1], n, dim, _stream()),
                    "relax_op_pool_stats")
        return out

    def op_token_stats(self, x):
        Nimg, T, dim = x.shape
        out = torch.empty((Nimg, 3 * dim), dtype=torch.float32, device=self.device)
        self._check(self.lib.relax_op_token_stats(self.h, _ptr(x), _ptr(out), Nimg, T, dim, _stream()),
                    "relax_op_token_stats")
        return out

    # ---- measurement ----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.relax_profile_enable(self.h, int(bool(on))), "relax_profile_enable")

    def profile_read(self, kind):
        ms, work, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.relax_profile_read(self.h, kind, C.byref(ms), C.byref(work), C.byref(n)),
                    "relax_profile_read")
        return ms.value, work.value, n.value


def pack_conv_weight(w_oihw, cin_pad=None):
    """OIHW fp32 -> [Cout, Kpad] with k = (dy*KW+dx)*Cin_pad + c, zero padded to a multiple of 32
    (the layout relax_op_conv2d_nhwc expects; the model loader does the same on the host in C++)."""
    w = np.asarray(w_oihw, dtype=np.float32)
    co, ci, kh, kw = w.shape
    cp = cin_pad or ci
    k = kh * kw * cp
    kpad = -(-k // 32) * 32
    out = np.zeros((co, kpad), dtype=np.float32)
    t = np.zeros((co, kh, kw, cp), dtype=np.float32)
    t[..., :ci] = w.transpose(0, 2, 3, 1)
    out[:, :k] = t.reshape(co, k)
    return out
