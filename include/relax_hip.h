/*
 * relax_hip.h — C-ABI of librelax_hip.so, the MI355X (gfx950) engine for the
 * ReLaX-VQA feature-extraction hot path.
 *
 * The reference (xinyiW915/ReLaX-VQA) has no FFI: its de-facto operator API for
 * this path is a set of module-level Python functions that pass PNG paths and
 * numpy arrays.  Each entry point below names the reference interface it
 * replaces (file:line relative to the reference repo).  The Python host layer
 * (relax-vqa_amd/) keeps those function names and binds this header through
 * ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative relax_status otherwise;
 *     relax_last_error() gives the message (Python raises RuntimeError).
 *   - caller allocates: every in/out buffer is a DEVICE pointer (e.g.
 *     torch.Tensor.data_ptr() under PyTorch-ROCm) unless the name says host.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  All work
 *     is enqueued on it; no hidden synchronisation.
 *   - a handle owns only weights + workspace; it is NOT thread-safe; one handle
 *     per (process, device).  The workspace is reused from call to call, so calls on
 *     one handle must be ordered: issue them on ONE stream (or order the streams with
 *     events); two backbone calls running concurrently on different streams would race.
 *   - images are uint8 HWC **BGR** exactly as cv2.imread holds them
 *     (src/main_fragment_layerstack.py:295-296); fragments are 224x224x3 (the
 *     *_ex fragment entry points cut target_size x target_size x 3 canvases; the
 *     backbones take 224 only).
 */
#ifndef RELAX_HIP_H
#define RELAX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RELAX_ABI_VERSION 1

/* the reference's literals: the geometry of the entry points without a patch_size / target_size argument, and the only canvas
 * the backbones take.  The *_ex fragment entry points take patch_size 8 / 16 / 32 and any canvas up to RELAX_MAX_TARGET. */
#define RELAX_PATCH 16           /* patch_size  (main_fragment_layerstack.py:298) */
#define RELAX_TARGET 224         /* target_size (main_fragment_layerstack.py:297) */
#define RELAX_TOP_N 196          /* top_n = (224/16)^2 (main_fragment_layerstack.py:299) */
#define RELAX_FRAG_BYTES (224 * 224 * 3)
#define RELAX_MAX_PATCH 32       /* 32*32*3*255 = 783360 < 2^20, the range of the selection's two 10-bit radix levels */
#define RELAX_MAX_TARGET 448     /* (448/8)^2 = 3136 slots at most */
#define RELAX_RN50_LAYER_STACK_DIM 13120 /* 64+3*256+4*512+4*1024+3*2048 */
#define RELAX_RN50_POOL_DIM 2051         /* 2048 + mean,max,std */
#define RELAX_RN50_NUM_TAPS 15
#define RELAX_VGG16_LAYER_STACK_DIM 4224 /* 64+64+128+128+3*256+3*512+3*512 */
#define RELAX_VGG16_POOL_DIM 4099        /* fc2 4096 + mean,max,std */
#define RELAX_VGG16_NUM_TAPS 15          /* 13 convolutions, fc1, fc2 */

typedef enum relax_status {
    RELAX_OK = 0,
    RELAX_ERR_INVALID = -1,   /* bad argument */
    RELAX_ERR_HIP = -2,       /* a HIP runtime call failed */
    RELAX_ERR_STATE = -3,     /* weights not loaded / workspace too small */
    RELAX_ERR_NOMEM = -4
} relax_status;

typedef struct relax_handle relax_handle;
typedef void* relax_stream;

/* ---- lifetime ------------------------------------------------------------------------------ */
int relax_abi_version(void);
int relax_create(int device, relax_handle** out);
int relax_destroy(relax_handle* h);
/* message of the last failing call on this handle (h may be NULL: last create error) */
const char* relax_last_error(const relax_handle* h);

/* Size the activation workspace for batches of up to max_images fragments
 * (ResNet-50 and ViT share one arena).  Called implicitly (growing) by the
 * backbone entry points; call it up front to keep allocation out of timed code. */
int relax_reserve(relax_handle* h, int max_images);

/* Integer options.  "gemm_precision": 3 (default) = "f16x2" (fp32-grade): every fp32 operand is held as two fp16 numbers of a
 * power-of-two multiple of itself, x * s = hi + lo (22 bits), and a*b = ah*bh + ah*bl + al*bh on v_mfma_f32_16x16x32_f16 with fp32
 * accumulation (al*bl, 2^-22 of the product, is added for K < 256 only); every scale comes from a bound, never from the data of a
 * batch - weights per output row, ViT activations one static power of two per tensor, ResNet-50 activations one per image from
 * Hoelder's inequality on the measured per-image maxima of the producer's inputs - so nothing can overflow and no row depends on its
 * batch (csrc/gemm_h2.hip, csrc/h2.h, tests/test_gpu_h2.py).  Accuracy: against fp64, each output's error measured against its sum of
 * magnitudes is no larger than the exact-fp32 path's, within two bounds of the format (tests/fp32_grade.py): at short K it may
 * exceed the chain's by 2^-23 / sqrt(K) (22-bit operands against one fp32 rounding per product), and a value below 2^-17 of its row's maximum keeps an absolute error of 2^-39 of that
 * maximum instead of 22 bits of itself.  It covers the plain GEMMs with N % 256 == 0 (the whole ViT-B/16;
 * relax_op_gemm), the convolutions of ResNet-50's layer3 / layer4 (relax_op_conv2d_nhwc with Cin % 32 == 0, Cout % 256 == 0) and the
 * 3x3 convolutions of its layer1 / layer2 (K x K filters onto 64 / 128 channels, K >= 256: v_mfma_f32_32x32x16_f16 on the four-wave
 * tiles of csrc/gemm_x6.hip, the two small products in an accumulator of their own), its stem (csrc/conv1_x6.hip) and the ViT's attention (csrc/attention_h2.hip;
 * relax_op_attention); everything else runs as under 2.  0 = exact fp32 products (v_mfma_f32_32x32x2_f32); 2 = "bf16x6" (fp32-grade):
 * every fp32 operand is held as three bf16 numbers hi + mid + lo (exact) and a*b = the six partial products of weight
 * >= 2^-16 on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16, two products per instruction; 32x32x16 on the 64 / 128-column
 * tiles) with fp32 accumulation - as close to the exact sum as the fp32 FMA chain
 * (csrc/gemm_x6.hip, tests/test_gpu_x6.py); used by the ViT / ResNet drivers and by relax_op_gemm; 1 = "bf16x3":
 * every fp32 operand is split on the fly into bf16 hi + lo and a*b = hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation (about 2^-16 relative error per product; measured features within ~1e-5 of the fp32 path).
 * "gemm_split_k" (default 1): cut the tail tiles of a contraction along K so the last round fills
 * the chip; results stay deterministic for a given batch, but the K-summation order of tail tiles then depends on the
 * batch size - set 0 when features must be bit-identical across batch compositions (e.g. comparing sharded runs).
 * "gemm_variant", "gemm_variant_n64" (exact-fp32 kernel only), "gemm_group_m": tuning knobs (tile variants are listed in
 * csrc/gemm.hip; none of them changes results beyond fp32 rounding).  "flow_max_pairs": cap on the pairs one optical-flow launch takes
 * (0 = by workspace size).  "x6_fp32_rows" (default 1): bf16x6 contractions onto 64 / 128 output columns read fp32 activation rows and
 * split them in the K loop, and the ResNet-50 block outputs inside layer1 / layer2 travel as fp32 (4 bytes per value instead of 6);
 * 0 = split planes everywhere: the same bits, more bytes (kept as the A/B switch of tests/test_gpu_x6.py).
 * "h2_form" (default 1): 1 = the f16x2 loop with 32-deep K steps and three products for K >= 256; 0 = 16-deep steps, four products
 * ("h2_stages" = 3 or 4 LDS stages, same bits); 2 = 32-deep steps, four products at every K.  "rn_h2" (default 1): under
 * "gemm_precision" 3 ResNet-50's layer3 / layer4 run f16x2; 0 = the whole network on bf16x6 (the A/B switch of tests/test_gpu_h2.py).
 * "rn_h2_early" (default 1): with "rn_h2", the stem and the 3x3 convolutions of layer1 / layer2 run f16x2 as well; 0 = bf16x6 there.
 * "att_h2" (default 1): under "gemm_precision" 3 the ViT's attention runs on fp16 planes too (csrc/attention_h2.hip: the qkv GEMM writes planes,
 * three partial products, K / V by LDS-DMA into the fragment images); 0 = the bf16x6 attention kernel on an fp32 qkv output (A/B switch).
 * "att_h2_stream" (default 1): with "att_h2", a token count other than 197 (a patch-8 model's 785, any other canvas) runs attention on
 * fp16 planes too (csrc/attention_stream_h2.hip: attention_h2's arithmetic with an online softmax over key tiles of 64; the qkv GEMM
 * writes planes); 0 = that GEMM writes fp32 and the streaming bf16x6 kernel (csrc/attention_stream.hip) writes the fp16 planes the
 * projection reads.  197 tokens run csrc/attention_h2.hip either way.  The option also picks relax_op_attention_ex's kernel under 3.
 * "rn_fuse" (default 1): with "rn_h2_early", the layer1 / layer2 blocks without a downsample branch run their 3x3 and their conv3 back to back in ONE
 * launch (csrc/gemm_x6.hip, B2B: the 3x3's output tile stays in registers as the A operand of the 1x1, conv3 on f16x2 with one scale
 * per pixel row); 0 = two launches, conv3 on bf16x6 (A/B switch).  "b2b_rows" (256 or 128): rows per tile of layer1's such launches, same bits.
 * "rn_c1_h2" (default 1): layer2's conv1 (1x1, fp32 rows in) on f16x2 - the rows are split into two fp16 planes in the K loop with the image's scale -;
 * 0 = bf16x6 (A/B switch).
 * "debug_poison" (test mode, default 0): every workspace request fills the buffer with 0xFF bytes
 * first (synchronously), so a read of workspace that was not written in the same call shows up in the results. */
int relax_set_option(relax_handle* h, const char* key, int value);
/* Reads an option back (bench.py reports the arithmetic the ENGINE is in, not the one its command line asked for).  Two read-only
 * counters for leak checks of long passes (tests/test_gpu_soak.py): "profile_events" = HIP events the handle owns (pooled + in open spans),
 * "workspace_mib" = MiB of its device workspaces (they grow to the largest batch seen and stay). */
int relax_get_option(relax_handle* h, const char* key, int* value);

/* ---- weights ------------------------------------------------------------------------------- */
/* Replaces `models.resnet50(pretrained=True)` (src/extractor/visualise_resnet.py:21,
 * visualise_resnet_layer.py:20).  names[i] are torchvision state-dict keys
 * ("conv1.weight", "layer1.0.bn1.running_var", ...); tensors[i] are HOST fp32
 * pointers in PyTorch layout (OIHW for convs); numels[i] their element counts.
 * BatchNorm (eps 1e-5, eval) is folded into the following conv's weights/bias,
 * except bn1 which is applied after the raw `conv1` tap. "fc.*" is ignored. */
int relax_load_resnet50(relax_handle* h, const float* const* tensors, const char* const* names,
                        const int64_t* numels, int n);

/* Replaces VitGenerator(name_model, patch_size=16, ...) + load_state_dict
 * (src/extractor/visualise_vit_layer.py:263-329).  DINO state-dict keys
 * ("cls_token", "blocks.0.attn.qkv.weight", ...).  dim/depth/heads: 768/12/12
 * for vit_base (:287-289); head_dim must be 64.  The checkpoint's pos_embed is the 224x224 table (197 tokens); the canvas of a call
 * is an argument of relax_vit_features_canvas.  = relax_load_vit_ex with patch_size 16. */
int relax_load_vit(relax_handle* h, const float* const* tensors, const char* const* names,
                   const int64_t* numels, int n, int dim, int depth, int heads);
/* VitGenerator(name_model, patch_size, ...) for patch_size 8 or 16 (:263-329 builds both): 224 / p patches per side, (224 / p)^2 + 1
 * tokens (785 / 197), patch-embed K = 3 p^2.  patch_embed.proj.weight must hold dim * 3 p^2 values and pos_embed ntok * dim: a
 * checkpoint of the other patch size is refused with both counts in the message, before the loaded model is touched.  Every later
 * call sizes itself by the loaded geometry (relax_vit_features: tokens [N, ntok - 1, dim], cls_attention [N, heads, ntok];
 * relax_reserve: ViT-B/8 takes 33.5 MB of arena per image, 3.7 times ViT-B/16).  197 tokens run the single-tile attention
 * kernels, 785 the streaming ones (csrc/attention_stream.hip). */
int relax_load_vit_ex(relax_handle* h, const float* const* tensors, const char* const* names,
                      const int64_t* numels, int n, int dim, int depth, int heads, int patch_size);
/* the geometry of the loaded ViT at 224x224 (any pointer may be NULL); refused before relax_load_vit */
int relax_vit_geometry(relax_handle* h, int* patch, int* ntok, int* dim, int* heads);
/* The patch grid of an [Hc, Wc] canvas under the loaded ViT: gh = Hc / p, gw = Wc / p (floors: PatchEmbed's stride-p convolution ignores
 * the trailing rows and columns of pixels, src/extractor/visualise_vit_layer.py:132-149), ntok = gh * gw + 1 (any pointer may be NULL).
 * Refused with the value in the message: Hc or Wc below the patch size, more than 4096 patches (4097 tokens: 1024^2 px at patch 16). */
int relax_vit_canvas_geometry(relax_handle* h, int Hc, int Wc, int* gh, int* gw, int* ntok);
/* interpolate_pos_encoding (src/extractor/visualise_vit_layer.py:197-219) for a gh x gw patch grid: out = device fp32 [1 + gh*gw, dim],
 * row 0 the class row, the others the loaded [side, side] table resampled by F.interpolate(scale_factor=((gh + .1) / side,
 * (gw + .1) / side), mode='bicubic') as torch evaluates it in fp32 (align_corners=False, A = -0.75, border taps clamped).  gh = gw = side
 * returns the loaded table (:200-201).  The tables of the last four grids stay on the handle; a ViT load drops them.  A grid that is not
 * among them is built inside the call: device memory is allocated (and the least recently used table freed, which waits for the device), the
 * kernel runs on `stream` and the call waits for `stream`.  Such a call cannot be captured into a graph, and a workload that cycles through
 * more than four grids pays a device-wide wait per call; a call on a cached grid, or on the loaded one, does neither.  The same holds for
 * relax_vit_features_canvas, which gets its table here. */
int relax_vit_pos_embed(relax_handle* h, int gh, int gw, float* out, relax_stream stream);

/* Replaces models.vgg16(pretrained=True) (src/extractor/visualise_vgg.py:21, visualise_vgg_layer.py:19; torchvision
 * configuration D, no BatchNorm).  torchvision keys: features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias} and
 * classifier.{0,3}.{weight,bias}; "classifier.6.*" is ignored.  A missing key or a wrong size is refused with a message naming
 * the key.  classifier.0's columns are permuted once here from the NCHW flatten of pool5 to the NHWC one. */
int relax_load_vgg16(relax_handle* h, const float* const* tensors, const char* const* names,
                     const int64_t* numels, int n);

/* ---- stage A: residual -> patch score -> top-n -> fragments (bit-exact integer path) -------- */
/* Replaces, per (frame, next) pair: cv2.absdiff (main_fragment_layerstack.py:302),
 * process_patches('frame_diff') = get_patch_diff + extract_important_patches (:232-240,
 * :177-210) and get_original_frame_patches (:212-230).
 *   orig, next : uint8 [H,W,3] per pair; pair t starts at orig + t*pair_stride (bytes)
 *   positions  : int32 [T,196,2] (y,x) patch coordinates in raster order, (-1,-1) past counts[t]
 *   counts     : int32 [T]  = min(top_n, (H/16)*(W/16))
 *   ori_frag   : uint8 [T,224,224,3] patches of `orig`   (may be NULL)
 *   diff_frag  : uint8 [T,224,224,3] patches of |next-orig| (may be NULL)
 *   scores     : uint32 [T,(H/16)*(W/16)] patch sums (may be NULL -> internal scratch)
 * Tie rule: higher score first, then lower flat patch index. */
int relax_fragment_pairs(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride,
                         int T, int H, int W, int top_n, int32_t* positions, int32_t* counts,
                         uint8_t* ori_frag, uint8_t* diff_frag, uint32_t* scores, relax_stream stream);

/* The same with the reference's patch_size / target_size arguments (get_patch_diff :177, extract_important_patches :191,
 * get_original_frame_patches :212, process_patches :232 all take them; main_residual_fragment.py:173-214 likewise).
 * relax_fragment_pairs = this at (RELAX_PATCH, RELAX_TARGET), byte for byte.
 *   patch_size  : 8, 16 or 32.  A score sums patch_size^2 * 3 bytes; the selection's two 10-bit radix levels hold 2^20 and
 *                 32*32*3*255 = 783360 is the largest that fits, so anything above 32 is refused, as is any other value
 *   target_size : a positive multiple of patch_size, at most RELAX_MAX_TARGET; slots = (target_size / patch_size)^2
 *   top_n       : in [0, slots]
 *   positions   : int32 [T,slots,2], (-1,-1) past counts[t];  counts : int32 [T] = min(top_n, (H/patch_size)*(W/patch_size))
 *   ori_frag, diff_frag : uint8 [T,target_size,target_size,3], patch k at tile (k / (target/patch), k % (target/patch)), zero
 *                 tiles past counts[t] (may be NULL)
 *   scores      : uint32 [T,(H/patch_size)*(W/patch_size)] (may be NULL)
 * A rejected geometry returns RELAX_ERR_INVALID with the offending value in the message and launches nothing.
 * Rows are read 16 bytes per lane when W*3, pair_stride and both pointers are multiples of 16 (at patch_size 8 every third
 * chunk is split between two patches; columns past the last whole patch are not read), byte by byte otherwise; same results. */
int relax_fragment_pairs_ex(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride,
                            int T, int H, int W, int patch_size, int target_size, int top_n, int32_t* positions,
                            int32_t* counts, uint8_t* ori_frag, uint8_t* diff_frag, uint32_t* scores, relax_stream stream);

/* Same selection on an already-computed residual image (the optical-flow image of
 * process_patches('optical_flow'), main_fragment_layerstack.py:319; main_residual_fragment.py:206-214).
 *   image: uint8 [H,W,3] per item, item t at image + t*item_stride. */
int relax_fragment_image(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W,
                         int top_n, int32_t* positions, int32_t* counts, uint8_t* frag, uint32_t* scores,
                         relax_stream stream);

/* process_patches(.., patch_size, target_size, top_n) on a residual image (main_fragment_layerstack.py:232-240,
 * main_residual_fragment.py:206-214): relax_fragment_image with the geometry arguments of relax_fragment_pairs_ex. */
int relax_fragment_image_ex(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W,
                            int patch_size, int target_size, int top_n, int32_t* positions, int32_t* counts, uint8_t* frag,
                            uint32_t* scores, relax_stream stream);

/* get_original_frame_patches (main_fragment_layerstack.py:212-230) with given positions. */
int relax_gather_patches(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W,
                         const int32_t* positions, const int32_t* counts, uint8_t* frag, relax_stream stream);
/* get_original_frame_patches(original_frame, positions, patch_size, target_size) (main_fragment_layerstack.py:212-230):
 * positions int32 [T,slots,2], frag uint8 [T,target_size,target_size,3], geometry as in relax_fragment_pairs_ex.  The
 * positions are the caller's: a slot outside the (H/patch_size) x (W/patch_size) grid, negative ones included, gives a zero tile. */
int relax_gather_patches_ex(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W,
                            int patch_size, int target_size, const int32_t* positions, const int32_t* counts, uint8_t* frag,
                            relax_stream stream);

/* merge_fragments = cv2.addWeighted(a,.5,b,.5,0) (main_fragment_layerstack.py:242-245):
 * round-half-to-even(0.5a+0.5b) on uint8. n_bytes elements. */
int relax_merge_fragments(relax_handle* h, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n_bytes,
                          relax_stream stream);

/* map_attention_to_original (src/demo_visual.py:12-25): per-patch values painted back onto the frames they were cut from,
 * scaled to levels and blended with a colour table.
 *   frames       : uint8 [H,W,3] BGR per frame; frame t at frames + t*frame_stride (bytes)
 *   positions    : int32 [T,196,2], counts int32 [T]: relax_fragment_pairs' format (patch units, slot order).  Slot k < counts[t]
 *                  paints the patch at positions[t,k] with patch_values[t,k]; a later slot on the same patch wins; out-of-range
 *                  positions paint nothing (relax_gather_patches gives them a zero tile); every other pixel is 0.
 *   patch_values : fp32 [T,196]
 *   lut_bgr      : uint8 [256,3] BGR colour table (cv2.applyColorMap's role)
 *   out          : uint8 [T,H,W,3] contiguous
 * level = trunc((double)v / (double)max * 255) with max over the whole frame, zeros included (numpy on the reference's float64
 * array); max <= 0 (undefined in the reference) gives level 0 everywhere, as do negative and NaN values.
 * out = (6 frame + 4 lut[level] + 5) / 10 per byte = cv2.addWeighted(frame, 0.6, heat, 0.4, 0) on uint8. */
int relax_attention_overlay(relax_handle* h, const uint8_t* frames, int64_t frame_stride, int T, int H, int W,
                            const int32_t* positions, const int32_t* counts, const float* patch_values,
                            const uint8_t* lut_bgr, uint8_t* out, relax_stream stream);
/* map_attention_to_original(original_frame, attention_map, positions, patch_size) (src/demo_visual.py:12-25) with its patch_size
 * argument: positions int32 [T,slots,2] in units of patch_size x patch_size patches, patch_values fp32 [T,slots]; patch_size 8, 16
 * or 32, slots in [1, 3136].  Same semantics: a later slot on the same patch wins, out-of-range positions paint nothing, max over
 * the whole frame with zeros included, level 0 for max <= 0, negative and NaN values.  relax_attention_overlay = this at
 * (RELAX_PATCH, RELAX_TOP_N), byte for byte. */
int relax_attention_overlay_ex(relax_handle* h, const uint8_t* frames, int64_t frame_stride, int T, int H, int W,
                               int patch_size, int slots, const int32_t* positions, const int32_t* counts,
                               const float* patch_values, const uint8_t* lut_bgr, uint8_t* out, relax_stream stream);

/* ---- optical flow --------------------------------------------------------------- */
/* Replaces cv2.calcOpticalFlowFarneback(gray(orig), gray(next), None, 0.5, 3, 15, 3, 5, 1.2, 0) and flow_to_rgb
 * (src/main_fragment_layerstack.py:313-316, 162-175; src/main_residual_fragment.py:283-287).  Parameters are the
 * reference's literals.  orig/next as in relax_fragment_pairs.
 *   flow     : fp32 [T,H,W,2] (dx,dy)                       (may be NULL)
 *   flow_bgr : uint8 [T,H,W,3] the visualisation image that process_patches('optical_flow', ...) consumes (may be NULL)
 * OpenCV's algorithm restated (not ported); parity is by tolerance against the reference's example flow PNGs. */
int relax_optical_flow(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                       float* flow, uint8_t* flow_bgr, relax_stream stream);
/* cv2.calcOpticalFlowFarneback(gray(orig), gray(next), None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
 * + flow_to_rgb: relax_optical_flow with OpenCV's parameters as arguments.  Buffers, chunking, workspace and visualisation as there.
 * Formula source: OpenCV's optflowgf.cpp as restated by oracle/flow_ref.py (farneback(prev, next, pyr_scale, levels, winsize,
 * iterations, poly_n, poly_sigma)): the pyramid of relax_flow_plan below, FarnebackPrepareGaussian(poly_n, poly_sigma), the box
 * window winsize, `iterations` updates per level, the coarser flow resized and multiplied by (float)(1 / pyr_scale).
 * With the reference's literals (0.5, 3, 15, 3, 5, 1.2, 0) it runs relax_optical_flow's launches: the same bits at the same speed.
 * Accepted: */
#define RELAX_FLOW_PYR_SCALE_MIN 0.5
#define RELAX_FLOW_PYR_SCALE_MAX 0.95
#define RELAX_FLOW_MAX_LEVELS 8        /* levels 0..8, as long as the coarsest level USED (relax_flow_plan) has scale >= 1/32 */
#define RELAX_FLOW_MIN_SCALE (1.0 / 32) /* 79 smoothing taps */
#define RELAX_FLOW_MIN_WINSIZE 3
#define RELAX_FLOW_MAX_WINSIZE 63      /* odd values only */
#define RELAX_FLOW_MAX_ITERATIONS 10   /* 1..10 */
/* poly_n 5 or 7; poly_sigma finite and > 0; flags 0.
 * Refused (RELAX_ERR_INVALID, the offending value named in relax_last_error, before anything is launched - and before the handle is
 * looked at: with h NULL the refusal is in relax_last_error(NULL), so the rules can be asked on a machine without a GPU):
 *   - anything outside the limits above;
 *   - an even winsize: OpenCV's box pass sums 2 * (winsize / 2) + 1 rows and columns but scales by 1 / winsize^2, the oracle sums
 *     exactly winsize; without OpenCV at hand nothing pins which of the two an even window means;
 *   - flags with OPTFLOW_FARNEBACK_GAUSSIAN (256) or OPTFLOW_USE_INITIAL_FLOW (4), each by name: the oracle restates neither. */
int relax_optical_flow_ex(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                          double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags,
                          float* flow, uint8_t* flow_bgr, relax_stream stream);
/* The pyramid calcOpticalFlowFarneback builds for H x W frames (H, W >= 16), OpenCV's own loop: scale = pyr_scale multiplied k
 * times in double; level k and every coarser one is dropped when W * scale < 32 or H * scale < 32; sigma = (1 / scale - 1) / 2,
 * smoothing kernel max(cvRound(5 sigma) | 1, 3) taps, level size cvRound(side * scale) (round half to even).
 *   n_levels       : the levels used below the full-size one (0..levels)
 *   level_hw_ksize : int32 [n_levels + 1][3] = (h, w, smoothing taps) per level, COARSEST FIRST, the full-size level last
 *                    (room for levels + 1 rows; may be NULL)
 *   level_sigma    : double [n_levels + 1], the smoothing sigma per level (may be NULL)
 * pyr_scale and levels within the limits above; refused too: a coarsest used scale under RELAX_FLOW_MIN_SCALE.
 * No handle, no GPU: host arithmetic; errors through relax_last_error(NULL). */
int relax_flow_plan(int H, int W, double pyr_scale, int levels, int* n_levels, int32_t* level_hw_ksize, double* level_sigma);
/* relax_optical_flow_ex with the two flag bits it refuses: flags in {0, 4, 256, 260}.  The six parameters: relax_optical_flow_ex's rules and
 * wording (the rules answer with h == NULL through relax_last_error(NULL) here too); any other flags bit is refused with the value named.
 * With flags 0 (init_flow NULL) it makes relax_optical_flow_ex's launches: the same bits.
 * BOTH MODES ARE PINNED TO THE FORMULAS STATED HERE, restated in float64 by tests/flow_flag_ref.py, AND NOT TO AN OPENCV BUILD: nothing here can
 * run OpenCV, and its output on these modes has not been compared.
 * RELAX_FLOW_GAUSSIAN (OPTFLOW_FARNEBACK_GAUSSIAN, 256): the box window of the flow update becomes a separable Gaussian window of the same
 *   2 m + 1 taps, m = winsize / 2, sigma = 0.3 m: k[0] = 1, k[i] = (float)exp(-i^2 / (2 sigma^2)), s = 1 / (1 + 2 sum k[1..m]) in double,
 *   k[i] = (float)(k[i] s).  Over each of the five planes of the matrix image M, rows then columns, replicated borders:
 *   v = M[y] k[0] + sum_i (M[min(y + i, h - 1)] + M[max(y - i, 0)]) k[i], the same along x on v.  All 2 m + 1 taps are used (the outermost is
 *   3.9e-3 of the centre).  The 2 x 2 solve is the box window's, in double, regulariser 1e-3, without a 1 / winsize^2 (the taps sum to 1).
 *   It takes update_matrices_k + gauss_solve_any at every window, 15 included; results do not depend on batch, chunk or "flow_seg_rows".
 * RELAX_FLOW_USE_INITIAL (OPTFLOW_USE_INITIAL_FLOW, 4): at the coarsest level USED (relax_flow_plan's first row, h_c x w_c at scale_c) the zero
 *   field becomes resize_area(init_flow, h_c, w_c) * (float)scale_c; finer levels are unchanged.  resize_area is cv::resize(INTER_AREA)'s
 *   separable table (relax_flow_area_table below), accumulated in double.
 *   init_flow : fp32 [T,H,W,2]; required with bit 4 and NULL without it - both mistakes are refused by name.  init_flow == flow is allowed
 *               (OpenCV's in/out use: a chunk of pairs reads its initial field before it writes its flow); any other overlap is refused.
 *               The call waits for the stream once per chunk (the host tables of the resize). */
#define RELAX_FLOW_USE_INITIAL 4
#define RELAX_FLOW_GAUSSIAN 256
int relax_optical_flow_flags(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                             double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags,
                             const float* init_flow, float* flow, uint8_t* flow_bgr, relax_stream stream);
/* The Gaussian window above, one half of it: half_taps[0 .. winsize / 2] (room for winsize / 2 + 1 floats), odd winsize in
 * RELAX_FLOW_MIN_WINSIZE .. RELAX_FLOW_MAX_WINSIZE.  No handle, no GPU; errors through relax_last_error(NULL). */
int relax_flow_gauss_window(int winsize, float* half_taps);
/* cv::resize(INTER_AREA)'s table for one axis, src >= dst >= 1.  S = src / dst in double; cell d covers [d S, d S + S), cw = min(S, src - d S):
 *   - full source pixels s1 = ceil(d S) up to but not including s2 = min(floor(d S + S), src - 1), with s1 = min(s1, s2), at 1 / cw each;
 *   - the left partial pixel s1 - 1 at (s1 - d S) / cw if that overlap exceeds 1e-3;
 *   - the right partial pixel s2 at min(d S + S - s2, 1, cw) / cw if that overlap exceeds 1e-3
 *     (an overlap of at most 1e-3 pixel is dropped, as in OpenCV: such a row sums to a little under 1; it takes dst / gcd(src, dst) >= 1000).
 *   first, count : int32 [dst] - source pixels first[d] .. first[d] + count[d] - 1
 *   weights      : double [dst][RELAX_FLOW_AREA_TAPS(src, dst)], count[d] of each row written, in source order
 * With dst == src it is a copy.  No handle, no GPU; errors through relax_last_error(NULL). */
#define RELAX_FLOW_AREA_TAPS(src, dst) ((src) / (dst) + 2)
int relax_flow_area_table(int src, int dst, int32_t* first, int32_t* count, double* weights);
/* The starting field of relax_optical_flow_flags' coarsest level alone: out fp32 [T,h_c,w_c,2] = resize_area(init_flow [T,H,W,2]) *
 * (float)scale_c with (h_c, w_c) relax_flow_plan(H, W, pyr_scale, levels)'s first row; levels 0: a copy, bit for bit.  Waits for the stream. */
int relax_flow_initial_level(relax_handle* h, const float* init_flow, int T, int H, int W, double pyr_scale, int levels, float* out,
                             relax_stream stream);
/* flow_to_rgb alone: fp32 [T,H,W,2] -> uint8 [T,H,W,3] (BGR, despite the reference's name). */
int relax_flow_to_rgb(relax_handle* h, const float* flow, int T, int H, int W, uint8_t* flow_bgr, relax_stream stream);

/* ---- whole-frame front-end ------------------------------------------------------ */
/* H x W -> 224 x 224, bit-identical to Pillow's 8-bit resample:
 *   out_bilinear : what transforms.Resize((224,224)) gives a PIL image (src/extractor/visualise_resnet.py:40-47)
 *   out_lanczos  : img.resize((224,224), Image.Resampling.LANCZOS)     (src/extractor/visualise_vit_layer.py:466-469)
 * frames uint8 [H,W,3] per item (item n at frames + n*item_stride; channel order is irrelevant), outputs
 * uint8 [N,224,224,3]; either output may be NULL.  One read of each frame serves both filters.
 * This is relax_resize_frames_ex (below) at out_h = out_w = 224, on the same kernels, with these consequences:
 *   - a pass whose dimension is already 224 is skipped and the bytes are copied, as Pillow does it (the 224 -> 224 table is one
 *     coefficient 2^22 per sample for both filters, so an identity pass would give the same bytes);
 *   - W above RELAX_RESIZE_224_MAX_IN_W (5461) is refused, as it always was on this entry, although the kernels stage rows up to
 *     RELAX_RESIZE_MAX_IN_W; W = 5457..5461 stage 4 * 16384 + 32 bytes of LDS, more than 64 KiB, and take the dynamic-LDS opt-in;
 *   - N above 65535 (the launch grid; once a failed launch) and H above RELAX_RESIZE_MAX_IN_H (once computed: the table builder
 *     itself has no limit) are refused with RELAX_ERR_INVALID and the value named;
 *   - the tables come from the handle's cache of 16 (least recently used replaced; a call needs at most four), and a table with
 *     a coefficient outside 24 bits would be refused - for out = 224 none is (the largest over the input sizes tested is 5 386 769);
 *   - a table that is not in the cache is built inside the call: device memory is allocated (and the least recently used table freed,
 *     which waits for the device) and the table is uploaded with a blocking copy.  Such a call cannot be captured into a graph; a call
 *     whose tables are all cached only enqueues on `stream`.  The same holds for the three other resize entries below. */
int relax_resize_frames(relax_handle* h, const uint8_t* frames, int64_t item_stride, int N, int H, int W,
                        uint8_t* out_bilinear, uint8_t* out_lanczos, relax_stream stream);

/* The same resize of the frame difference of T pairs: the whole residual image of src/main_residual.py:223-231
 * (cv2.absdiff(img_next, img_original), resized by the extractors: src/extractor/visualise_resnet_layer.py:39-43 BILINEAR,
 * src/extractor/visualise_vit_layer.py:466-469 LANCZOS).  orig / next / pair_stride as in relax_fragment_pairs.
 *   out_bilinear, out_lanczos : uint8 [T,224,224,3], what relax_resize_frames returns for the image |next - orig|
 *   residual                  : uint8 [T,H,W,3] contiguous, the difference image itself (the reference's _residual.png)
 * Any of the three may be NULL, not all.  The difference is taken while the rows are staged on the chip: a pair is read
 * once, and the residual image is written only when asked for.
 * `residual` must not overlap `orig` or `next` (the kernel treats the three as distinct memory).
 * Rows move 16 bytes per lane only when W*3, pair_stride and all of orig, next and a non-NULL residual are multiples of
 * 16; any one of them off (an odd residual pointer alone included) puts the whole call on the much slower bytewise path.
 * This is relax_resize_residual_ex at out_h = out_w = 224: the limits and consequences listed at relax_resize_frames hold here
 * too (T in the place of N).  With W == 224 and H != 224 the difference image goes through the handle's workspace once and serves
 * both filters. */
int relax_resize_residual(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                          uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual, relax_stream stream);

/* ---- whole-frame front-end at ANY output size (the canvases relax_vit_features_canvas takes) --------- */
/* The reference's resize size is an argument: transforms.Resize(img_size) (src/extractor/visualise_vit_layer.py:339-342, the
 * reduced-size form left commented at :473; visualise_vit.py:339-342; demo_visual.py:27-28) and img.resize(..., LANCZOS) - in
 * both cases Pillow's 8-bit resample.  The limits of the resize entries: */
#define RELAX_RESIZE_BILINEAR 0
#define RELAX_RESIZE_LANCZOS 1
#define RELAX_RESIZE_MAX_OUT 2048     /* out_h, out_w: 1..2048 (a 4096-patch ViT canvas reaches 2048 pixels on a side: 2048 x 512 at patch 16) */
#define RELAX_RESIZE_MAX_IN_W 8192    /* W: four input rows are staged in LDS (8192 * 3 * 4 B = 96 KiB; above 64 KiB by opt-in) */
#define RELAX_RESIZE_MAX_IN_H 16384   /* H, and in_size of relax_resize_table */
#define RELAX_RESIZE_224_MAX_IN_W 5461   /* W of relax_resize_frames / relax_resize_residual: four rows of it are the 64 KiB their first kernels staged */
/* Everything outside them is refused (RELAX_ERR_INVALID) with the offending value named in relax_last_error. */

/* The size transforms.Resize(size), size an int, gives a PIL image of H x W (torchvision's _compute_resized_output_size): the
 * shorter side becomes `size`, the longer int(size * long / short); when W <= H - W == H included - W is the shorter side.
 * Integer arithmetic: size * long < 2^26 inside the limits (H, W 1..RELAX_RESIZE_MAX_IN_H, size 1..RELAX_RESIZE_MAX_OUT), and
 * Python's correctly rounded double quotient can reach the next integer from a fractional value only with quotient * short near
 * 2^53, so floor division is int() of Python's expression.  A longer side above RELAX_RESIZE_MAX_OUT is refused.
 * No handle, no GPU: host arithmetic; errors through relax_last_error(NULL). */
int relax_resize_output_size(int H, int W, int size, int* out_h, int* out_w);

/* The table of one resample pass, in_size -> out_size, filt RELAX_RESIZE_BILINEAR / _LANCZOS - Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc for the box (0, in_size), the table every resize kernel of this library reads:
 *   bounds : int32 [out_size][2]  first tap, tap count
 *   coeffs : int32 [out_size][*ksize]  the taps as 22-bit fixed point, zero behind the count
 * bounds == NULL: only *ksize is written (the query before the buffers are made).  Host only, errors as above. */
int relax_resize_table(int in_size, int out_size, int filt, int32_t* bounds, int32_t* coeffs, int* ksize);

/* relax_resize_frames at a runtime output size: outputs uint8 [N,out_h,out_w,3], bit-identical to
 * Image.resize((out_w,out_h), BILINEAR / LANCZOS) for downscaling, upscaling and mixed; either may be NULL, not both.
 * Pillow's order and skips are kept (the uint8 intermediate makes them visible): the horizontal pass first, its result stored
 * as uint8 [N,H,out_w,3] in the handle's workspace, then the vertical pass; a pass whose dimension already matches is skipped and
 * the bytes are copied.  One read of each frame serves both filters.  Rows are staged 16 bytes per lane when W*3, item_stride and
 * frames are multiples of 16, bytewise otherwise (decided per call).  The tables are cached on the handle per (input size, output
 * size, filter), the least recently used of 16 replaced; a table that is not cached is built inside the call, which then waits for the
 * device (see relax_resize_frames).  relax_resize_frames is this entry at 224 x 224 with its own width limit. */
int relax_resize_frames_ex(relax_handle* h, const uint8_t* frames, int64_t item_stride, int N, int H, int W, int out_h, int out_w,
                           uint8_t* out_bilinear, uint8_t* out_lanczos, relax_stream stream);

/* relax_resize_residual at a runtime output size: out_bilinear / out_lanczos uint8 [T,out_h,out_w,3] = what
 * relax_resize_frames_ex returns for the image |next - orig|, residual uint8 [T,H,W,3] contiguous.  Any of the three may be NULL,
 * not all.  relax_resize_residual's contract holds unchanged: `residual` must not overlap `orig` or `next`, and rows move 16 bytes
 * per lane only when W*3, pair_stride and all of orig, next and a non-NULL residual are multiples of 16 (an odd residual pointer
 * alone puts the whole call on the bytewise path). */
int relax_resize_residual_ex(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                             int out_h, int out_w, uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual,
                             relax_stream stream);

/* ---- stage B: backbones ---------------------------------------------------------------------- */
/* ResNet-50 on N fragments (uint8 [N,224,224,3] BGR).  One forward per image yields everything
 * the reference gets from 15 hooked forwards + 1 avgpool forward:
 *   layer_stack : fp32 [N,13120] = get_deep_feature(..,'layer_stack') + process_video_feature(..,'layer_stack')
 *                 (main_fragment_layerstack.py:91-96,134-140; extractor/visualise_resnet.py:62-109)   (may be NULL)
 *   pool        : fp32 [N,2051]  = get_deep_feature(..,'pool') + process_video_feature(..,'pool')
 *                 (main_fragment_layerstack.py:97-99,141-149; extractor/visualise_resnet_layer.py:62-102) (may be NULL)
 *   taps_nchw   : NULL, or RELAX_RN50_NUM_TAPS device pointers (each NULL or fp32 [N,C,H,W]) receiving the
 *                 hooked activations themselves (visualise_resnet.process_video_frame's dict values).
 * 224 x 224 is the canvas of a freshly loaded model.  After relax_resnet50_set_canvas(h, Hc, Wc) the images are read as uint8 [N,Hc,Wc,3]
 * and the taps are written as [N,C,h_t,w_t] of that canvas (relax_resnet50_canvas_geometry's tap_hw); layer_stack and pool keep their
 * widths, the model ends in spatial means.  The canvas is read when the call is made: a captured graph keeps the canvas it was captured
 * with. */
int relax_resnet50_features(relax_handle* h, const uint8_t* frags, int N, float* layer_stack, float* pool,
                            float* const* taps_nchw, relax_stream stream);

/* The clip path asks different things of the two groups of its batch: the layer stack of the ORIGINAL fragments and the pool
 * vector of the RESIDUAL fragments (src/main_fragment_layerstack.py:327-328: get_deep_feature(.., original_frag_path, ..,
 * 'layer_stack') and get_deep_feature(.., merged_frag_path, .., 'pool'); :340-341).  ONE forward over all N images:
 *   images [0, n_layer_stack)  -> layer_stack fp32 [n_layer_stack, 13120]
 *   images [n_layer_stack, N)  -> pool        fp32 [N - n_layer_stack, 2051]
 * Same values as relax_resnet50_features on the respective images; the taps of the second group are neither reduced nor written
 * as fp32, the pool statistics of the first group are not formed.  Either group may be empty (its pointer may then be NULL).
 * The images are read at the handle's canvas, as relax_resnet50_features reads them. */
int relax_resnet50_clip_features(relax_handle* h, const uint8_t* frags, int N, int n_layer_stack, float* layer_stack, float* pool,
                                 relax_stream stream);

/* ResNet-50 on any canvas.  torchvision's ResNet-50 takes any input size (convolutions, one 3x3 / 2 max-pool, an adaptive average pool:
 * src/extractor/visualise_resnet.py:21), and the layer-stack row (13120 channel means) and the pool row (2051) have the same width on
 * every canvas.  The kernels take the canvases on which every stage map is even down to layer4 and the stem's output is whole 256-pixel
 * tiles per image: Hc and Wc multiples of 32 in [64, 1024].  The canvas is a property of the loaded model, set by a host-only call as
 * relax_load_vit_ex fixes a patch size; relax_resnet50_features and relax_resnet50_clip_features run at it.  (A one-call
 * relax_resnet50_features_canvas entry with the canvas as an argument, like relax_vit_features_canvas, is left for a change that is free to
 * extend the stream-contract table of the tests.)
 *
 * relax_resnet50_canvas_geometry: host arithmetic, no handle, no GPU.  tap_hw (may be NULL) receives [RELAX_RN50_NUM_TAPS][2] ints, the
 * {height, width} of every tap's map: {Hc / 2, Wc / 2} for tap 0, then Hc / 4 (3 taps), / 8 (4), / 16 (4), / 32 (3) - at 224 x 224: 112, 56,
 * 28, 14, 7.  arena_bytes_per_image (may be NULL): what one image of that canvas takes of the forward's workspace (relax_reserve).
 * RELAX_ERR_INVALID for anything but an accepted canvas; relax_last_error(NULL) then names the offending value, as relax_resnet50_set_canvas'
 * message does. */
int relax_resnet50_canvas_geometry(int Hc, int Wc, int* tap_hw, int64_t* arena_bytes_per_image);
/* Sets the canvas of the loaded ResNet-50 for the calls that follow on this handle: validation and two integers - no launch, no allocation,
 * no synchronisation; the workspace grows in the next forward as it does for a larger batch (relax_reserve sizes it for the canvas set at
 * that moment).  A refused canvas (RELAX_ERR_INVALID) leaves the previous one, and relax_last_error names the offending value ("resnet50:
 * canvas height 230 is not a multiple of 32 in [64, 1024] (canvas 230 x 224)").  relax_load_resnet50 puts 224 x 224 back.  At 224 x 224
 * a forward launches the kernels it always launched, with the same bits; at any other canvas the stem runs its 16 x 16-tile form
 * (csrc/conv1_x6.hip) and every bottleneck the first launch form whose kernel takes its maps (csrc/host_logic.h: rn_maps_*). */
int relax_resnet50_set_canvas(relax_handle* h, int Hc, int Wc);
/* the canvas the next forward runs at (either pointer may be NULL) */
int relax_resnet50_get_canvas(relax_handle* h, int* Hc, int* Wc);

/* ResNet-50 on EVERY canvas size, opt-in.  flags = 0: the two entries above, with their rule and their messages.  RELAX_RN_CANVAS_ANY: Hc and
 * Wc are any integers in [64, 1024]; every stage follows torch's floor rule floor((n + 2 p - k) / s) + 1, so maps may be odd (65 x 67:
 * 33 x 34, 17 x 17, 9 x 9, 5 x 5, 3 x 3).  On such a canvas the stem runs its partial-tile form (image rows at any byte alignment), the max-pool
 * its any-map form (the 3 x 3 window clipped at all four edges, per-image maxima on any map), and every bottleneck the first launch form whose
 * kernel takes its maps.  On a canvas the default rule accepts the flag changes nothing: the same launches, the same bits.  Any other flag bit
 * is refused by name; a value outside [64, 1024] is refused naming the value and the canvas ("resnet50: canvas height 63 is not in [64, 1024]
 * (canvas 63 x 64)").  A refused call leaves the outputs / the previous canvas untouched.  relax_resnet50_get_canvas reports the canvas as
 * before; relax_load_resnet50 puts 224 x 224 and the default rule back.  Host-only, as the entries above: the forward goes through
 * relax_resnet50_features / relax_resnet50_clip_features at the handle's canvas. */
#define RELAX_RN_CANVAS_ANY 1
int relax_resnet50_canvas_geometry_ex(int Hc, int Wc, int flags, int* tap_hw, int64_t* arena_bytes_per_image);
int relax_resnet50_set_canvas_ex(relax_handle* h, int Hc, int Wc, int flags);

/* VGG-16 on N fragments (uint8 [N,224,224,3] BGR; images are processed in chunks of at most 32).  Every tap is read POST-ReLU:
 * torchvision's ReLU(inplace=True) behind each hooked module rectifies the hooked tensor before the reference copies it.
 *   layer_stack : fp32 [N,4224] = get_deep_feature('vgg16',..,'layer_stack') + process_video_feature(..,'layer_stack'):
 *                 spatial means of features[0,2,5,...,28] (main_fragment_layerstack.py:101-105,134-140;
 *                 extractor/visualise_vgg.py:38-58)   (may be NULL)
 *   pool        : fp32 [N,4099]  = get_deep_feature('vgg16',..,'pool') + process_video_feature(..,'pool'): fc2 =
 *                 classifier[3] + mean,max,std (main_fragment_layerstack.py:106-108,141-149; extractor/visualise_vgg_layer.py:51-58)
 *                 (may be NULL)
 *   taps_nchw   : NULL, or RELAX_VGG16_NUM_TAPS device pointers (each NULL or fp32): 0..12 the convolutions [N,C,H,W],
 *                 13 fc1 [N,4096], 14 fc2 [N,4096]. */
int relax_vgg16_features(relax_handle* h, const uint8_t* frags, int N, float* layer_stack, float* pool,
                         float* const* taps_nchw, relax_stream stream);

/* ViT on N fragments.  tokens: fp32 [N,196,dim] final-norm patch tokens
 * (visualise_vit_layer.process_video_frame, :447-500; [N,784,dim] with a patch-8 model) (may be NULL);
 * pooled: fp32 [N,3*dim] mean|max|std over tokens (main_fragment_pool.py:124-133) (may be NULL). */
int relax_vit_features(relax_handle* h, const uint8_t* frags, int N, float* tokens, float* pooled,
                       relax_stream stream);
/* relax_vit_features plus the attention of the LAST block's CLS query (src/extractor/visualise_vit.py:241-250
 * get_last_selfattention, :123-127 Block.forward(return_attention=True), :353-369 visualize_attention):
 *   cls_attention : fp32 [N,heads,ntok] = softmax(q_0 . k_j / 8) over all ntok keys (197; 785 at patch 8), per (image, head) (may be NULL).
 *                   Column 0 is the CLS key; the reference keeps columns 1..196 (attn[0, :, 0, 1:]).
 * Tokens and pooled are the same bits as relax_vit_features gives.  With cls_attention alone the forward stops after the
 * last block's qkv GEMM (the last block's attention core, proj, MLP and the final norm are skipped).  All three NULL: refused. */
int relax_vit_features_ex(relax_handle* h, const uint8_t* frags, int N, float* tokens, float* pooled, float* cls_attention,
                          relax_stream stream);
/* relax_vit_features_ex on images of any size: VisionTransformer.forward / get_last_selfattention with prepare_tokens'
 * interpolate_pos_encoding (src/extractor/visualise_vit_layer.py:197-232, 234-250; src/extractor/visualise_vit.py:353-370 runs an
 * image cropped to patch multiples at its own size).  images uint8 [N,Hc,Wc,3] BGR; the grid is relax_vit_canvas_geometry's
 * (gh = Hc / p, gw = Wc / p, trailing pixels ignored), npatch = gh * gw, ntok = npatch + 1:
 *   tokens [N,npatch,dim], pooled [N,3*dim], cls_attention [N,heads,ntok]   (each may be NULL, not all three).
 * The position table is relax_vit_pos_embed(gh, gw).  197 tokens run the single-tile attention kernels, any other count the
 * streaming ones.  Hc = Wc = 224 is relax_vit_features_ex: the same launches, the same bits. */
int relax_vit_features_canvas(relax_handle* h, const uint8_t* images, int N, int Hc, int Wc, float* tokens, float* pooled,
                              float* cls_attention, relax_stream stream);
/* VisionTransformer.get_intermediate_layers(x, n) (src/extractor/visualise_vit_layer.py:252-260): the final norm (:234-239, eps 1e-6)
 * applied to the output of each of the last n_last blocks, in ONE forward on any canvas (images, Hc, Wc as relax_vit_features_canvas).
 * Tap k = 0 .. n_last - 1 is block depth - n_last + k, the reference's order; the last tap is forward's own norm:
 *   tokens [n_last,N,ntok,dim]   the normed rows, row 0 the CLS token (forward's x[:, 0]), rows 1.. the patch tokens
 *   cls    [n_last,N,dim]        the normed CLS row alone: the same bits as tokens[k][:, 0]
 *   pooled [n_last,N,3*dim]      mean | max | population std over the normed patch tokens: the same bits as relax_op_token_stats of
 *                                tokens[k][:, 1:], and for the last tap as relax_vit_features' pooled
 * (each may be NULL, not all three).  cls and pooled come from one launch per tap that reads the residual stream and writes no normed
 * tokens (csrc/vit_layers.hip).  n_last outside [1, depth] is refused. */
int relax_vit_intermediate_layers(relax_handle* h, const uint8_t* images, int N, int Hc, int Wc, int n_last, float* tokens, float* cls,
                                  float* pooled, relax_stream stream);

/* ---- quality head at inference --------------------------------------------------- */
/* Replaces imputer.transform + scaler.transform + Mlp.forward (src/demo_test.py:177-208, src/model_regression.py:37-58).
 * State-dict keys of the reference's Mlp (fc1/bn1/fc2/fc3; a 'module.' prefix is stripped and 'n_averaged' ignored as
 * fix_state_dict does, demo_test.py:25-35); HOST pointers.  imputer_statistics = SimpleImputer.statistics_ (may be
 * NULL), scaler_scale / scaler_min = MinMaxScaler.scale_ / .min_, all HOST float64 [input_features].
 * A state dict with no bn1.* key at all is the plain Mlp of src/model_regression_simple.py:37-58: fc1.weight is padded and fc1.bias
 * copied as they are, nothing is folded; some but not all of the four bn1 tensors is refused. */
int relax_load_mlp_head(relax_handle* h, const float* const* tensors, const char* const* names, const int64_t* numels,
                        int n, const double* imputer_statistics, const double* scaler_scale, const double* scaler_min,
                        int input_features);
/* features: device fp32 [n, input_features] (the all-gathered per-clip vectors) -> scores: device fp32 [n]. */
int relax_mlp_head(relax_handle* h, const float* features, int n, float* scores, relax_stream stream);

/* ---- quality head, training ----------------------------------------------------------- */
/* Replaces preprocess_data's fit (src/model_regression.py:122-135): NaN and +-inf of x (device fp32 [n,F]) count as 0;
 * imputer_statistics = column means (SimpleImputer.statistics_), scaler_scale = 1 / (max - min) (1 where the range is below
 * 10 eps(float64), sklearn's _handle_zeros_in_scale), scaler_min = -data_min * scale (MinMaxScaler.scale_ / .min_): DEVICE
 * float64 [F] each, the vectors relax_load_mlp_head takes from the host.  data_min / data_max: DEVICE float64 [F], may be NULL.
 * One pass over the matrix.  Enqueued on `stream`. */
int relax_head_fit_scaler(relax_handle* h, const float* x, int n, int F, double* imputer_statistics, double* scaler_scale,
                          double* scaler_min, double* data_min, double* data_max, relax_stream stream);
/* Replaces X[isnan] = 0; X[isinf] = 0; scaler.transform(X); torch.FloatTensor(X) (model_regression.py:123-130, :392):
 * x device fp32 [n,F] -> xp device fp32 [n, Fpad], Fpad = F rounded up to a multiple of 32, padding columns zero.
 * (The reference scores with NaN -> column mean, demo_test.py:177-181, but trains on NaN -> 0: relax_mlp_head keeps the former.) */
int relax_head_train_transform(relax_handle* h, const float* x, int n, int F, const double* scaler_scale, const double* scaler_min,
                               float* xp, relax_stream stream);
/* Allocates the training state of an Mlp(input_features, hidden_features) (model_regression.py:37-58; hidden_features a multiple of
 * 128): three parameter sets with their BatchNorm buffers - 0 the live model with its SGD momentum buffers, 1 the SWA average
 * (AveragedModel, :388), 2 a snapshot (copy.deepcopy(model), :445) - all zero until relax_head_train_import, Adam's second-moment block, and the workspace
 * of batches of up to max_batch rows (2..1024).  Waits for the device. */
int relax_head_train_init(relax_handle* h, int input_features, int hidden_features, int max_batch);
/* relax_head_train_init with the head's variant.  batchnorm = 1: relax_head_train_init itself, bit for bit.  batchnorm = 0: the plain
 * Mlp of src/model_regression_simple.py:37-58 (fc1 -> GELU -> dropout -> fc2 -> GELU -> dropout -> fc3, bn1 commented out) - the head
 * behind the reference's KoNViD-1k / YouTube-UGC / LIVE-VQC / CVD2014 numbers.  Its three sets hold fc1.weight [H1,Fpad], fc1.bias,
 * fc2.weight, fc2.bias, fc3.weight, fc3.bias and no bn1 block; the optimizer blocks follow.  Any other value is refused.  The variant
 * is a property of the state: every relax_head_train_* entry below acts on whichever variant the state has.  On a plain state
 *   - a step computes a1 = dropout(GELU(z1)) under the same mask key as the BatchNorm step (one (seed, step): the same masks),
 *     dz1 = (dz2 W2) * mask / (1 - rate) * GELU'(z1), and fc1.bias has a real gradient, db1 = sum_b dz1, summed in a fixed order;
 *   - import / import_optimizer refuse any bn1.* key by name; export / export_optimizer write the six tensors in the order above and
 *     relax_head_train_export_numel reports that count; counters[0] (num_batches_tracked) stays 0;
 *   - relax_head_train_bn_pass checks its arguments and returns RELAX_OK without a launch, as torch.optim.swa_utils.update_bn returns
 *     at once for a model without BatchNorm.  Waits for the device. */
int relax_head_train_init_ex(relax_handle* h, int input_features, int hidden_features, int max_batch, int batchnorm);
/* *batchnorm = 1 for a state with bn1, 0 for a plain one; RELAX_ERR_INVALID without a state. */
int relax_head_train_arch(relax_handle* h, int* batchnorm);
/* Loads a state dict (the keys relax_load_mlp_head takes; HOST pointers) into a set: the initial model, or the checkpoint
 * fine_tune.py:130-136 starts from.  Into set 0 it also zeroes the momentum buffers, Adam's second moments and its step count (a new optimizer).  Waits for the device. */
int relax_head_train_import(relax_handle* h, int set, const float* const* tensors, const char* const* names, const int64_t* numels, int n,
                            int64_t num_batches_tracked, int64_t n_averaged);
/* Floats of a set as relax_head_train_export writes them (-1 without a state). */
int64_t relax_head_train_export_numel(relax_handle* h);
/* model.state_dict() (or, with momentum != 0, the momentum_buffer of each parameter; set 0 only): HOST fp32, in the order
 * fc1.weight [H1,F], fc1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, fc2.weight [H2,H1], fc2.bias,
 * fc3.weight [1,H2], fc3.bias; counters[2] = bn1.num_batches_tracked, n_averaged.  Waits for `stream`. */
int relax_head_train_export(relax_handle* h, int set, int momentum, float* out, int64_t* counters, relax_stream stream);
/* dst_set <- src_set, parameters, buffers and counters (copy.deepcopy(model); AveragedModel(model) at its creation). */
int relax_head_train_copy(relax_handle* h, int dst_set, int src_set, relax_stream stream);
/* MAEAndRankLoss.forward (model_regression.py:69-89, use_margin off) and its gradient: pred / target device fp32 [B];
 * loss device fp32 [1]; grad device fp32 [B] (may be NULL).  One B x B kernel. */
int relax_head_criterion(relax_handle* h, const float* pred, const float* target, int B, float l1_w, float rank_w, float* loss,
                         float* grad, relax_stream stream);
/* One iteration of train_one_epoch (model_regression.py:296-304) on the live set: zero_grad, forward in train mode, criterion,
 * backward, optim.SGD(momentum, weight_decay).step().  xp: device [n, Fpad] from relax_head_train_transform; target: device
 * fp32 [n]; index: device int32 [B], the batch's rows; 2 <= B <= max_batch.  Dropout masks come from a counter-based generator
 * keyed by (seed, step, layer, element) - not torch's stream; mask1 [B,H1] / mask2 [B,H2] (device uint8, may be NULL) receive
 * the masks used.  The batch loss is added into a device accumulator (relax_head_train_loss_read).  Enqueued on `stream`;
 * never waits for the device (relax_head_train_init sizes the contraction's split-K workspace).  fc1 / fc2 run on the exact-fp32
 * contraction whatever "gemm_precision" is set.  `index` is not validated: a row outside [0, n) is clamped into the matrix. */
int relax_head_train_step(relax_handle* h, const float* xp, const float* target, int n, const int32_t* index, int B, float lr,
                          float momentum, float weight_decay, float l1_w, float rank_w, float drop_rate, uint64_t seed, uint64_t step,
                          uint8_t* mask1, uint8_t* mask2, relax_stream stream);
/* One iteration of evaluate (model_regression.py:308-322): eval-mode forward of a set over the rows `index`, predictions to
 * pred (device fp32 [B]); with target != NULL the batch's criterion goes into the evaluation accumulator.  1 <= B <= max_batch. */
int relax_head_train_eval(relax_handle* h, int set, const float* xp, const float* target, int n, const int32_t* index, int B, float l1_w,
                          float rank_w, float* pred, relax_stream stream);
/* torch.optim.swa_utils.update_bn (model_regression.py:459), one batch per call: with reset != 0 first running_mean = 0,
 * running_var = 1, num_batches_tracked = 0; then (B > 0) a train-mode forward through bn1 whose momentum is
 * 1 / num_batches_tracked.  B = 0 only resets.  On a plain state (relax_head_train_init_ex, batchnorm 0) the arguments are checked
 * and RELAX_OK returned with no launch: update_bn likewise returns at once for a model without BatchNorm. */
int relax_head_train_bn_pass(relax_handle* h, int set, int reset, const float* xp, int n, const int32_t* index, int B, relax_stream stream);
/* swa_model.update_parameters(model) (model_regression.py:410): set 1 <- running average of set 0's parameters (buffers are
 * not averaged: AveragedModel's use_buffers=False), n_averaged += 1.  One launch over all parameters. */
int relax_head_train_swa_update(relax_handle* h, relax_stream stream);
/* The loss accumulators (which: 0 training steps, 1 evaluation): out[3] HOST = sum of batch losses, sum of batch loss x batch
 * rows (the loss.item() * inputs.size(0) of :304 / :320), batches; reset != 0 zeroes them.  Waits for `stream`: the one read of
 * an epoch. */
int relax_head_train_loss_read(relax_handle* h, int which, int reset, double* out, relax_stream stream);
/* out[2] HOST = sum |fc1.weight[:, F:Fpad]|, sum |its momentum buffer[:, F:Fpad]| of the live set: the zero padding of K, which a step
 * must leave exactly zero.  Waits for `stream`. */
int relax_head_train_pad_abs_sum(relax_handle* h, double* out, relax_stream stream);
/* The last stage of a step alone, on the batch and dz1 the last relax_head_train_step left (a measurement, tools/head_train_bench.py):
 * fused != 0 the step's own kernel (dW1 = dz1^T X_b with the SGD update in its epilogue); fused == 0 the same tiles writing dW1 to
 * memory, then a separate update pass.  Both change fc1.weight and its momentum. */
int relax_head_train_dw1(relax_handle* h, int fused, int B, float lr, float momentum, float weight_decay, relax_stream stream);
/* The same iteration under optim.Adam (src/model_regression.py:381-386, src/model_regression_simple.py:377-382; decoupled == 0:
 * g = grad + weight_decay w) or optim.AdamW (src/fine_tune.py:151-155; decoupled != 0: w *= 1 - lr weight_decay, g = grad), torch's
 * single-tensor arithmetic without amsgrad: m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g g,
 * w -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  The live set keeps exp_avg where SGD keeps its momentum buffers,
 * exp_avg_sq in a second block, and ONE step count t on the host (torch's per-parameter `step` values are all equal): this call
 * increments it and computes the two bias corrections from it in double, so nothing waits for the device.  The optimizer's scalars are
 * doubles, as torch holds them.  Everything else as relax_head_train_step, whose launches it shares.  Do not alternate the two step
 * entries on one state without an import in between: they read the first block differently. */
int relax_head_train_step_adam(relax_handle* h, const float* xp, const float* target, int n, const int32_t* index, int B, double lr,
                               double beta1, double beta2, double eps, double weight_decay, int decoupled, float l1_w, float rank_w,
                               float drop_rate, uint64_t seed, uint64_t step, uint8_t* mask1, uint8_t* mask2, relax_stream stream);
/* optimizer.state_dict()['state'] of the Adam / AdamW above: which = 0 exp_avg, 1 exp_avg_sq of every parameter, HOST fp32 in the
 * flat order of relax_head_train_export (zeros under the two buffer keys); *t_out = the step count.  Waits for `stream`. */
int relax_head_train_export_optimizer(relax_handle* h, int which, float* out, int64_t* t_out, relax_stream stream);
/* optimizer.load_state_dict(): both moments of every parameter (HOST pointers under the parameters' state-dict keys, marshalled as
 * for relax_head_train_import: exp_avg[i] and exp_avg_sq[i] belong to names[i]) and the step count, to resume a run.
 * relax_head_train_import into set 0 resets all three (a new optimizer), so call this after it.  Waits for the device. */
int relax_head_train_import_optimizer(relax_handle* h, const float* const* exp_avg, const float* const* exp_avg_sq, const char* const* names,
                                      const int64_t* numels, int n, int64_t t);
/* relax_head_train_pad_abs_sum with exp_avg_sq as a third sum: out[3] HOST = sum | . [:, F:Fpad]| of fc1.weight, exp_avg, exp_avg_sq.
 * Waits for `stream`, as relax_head_train_pad_abs_sum does. */
int relax_head_train_pad_abs_sum_adam(relax_handle* h, double* out, relax_stream stream);
/* relax_head_train_dw1 under Adam / AdamW (a measurement, tools/head_train_bench.py): fused != 0 the Adam step's own kernel, fused == 0
 * the same tiles writing dW1, then a separate update pass.  Both change fc1.weight and both moments; the step count stays. */
int relax_head_train_dw1_adam(relax_handle* h, int fused, int B, double lr, double beta1, double beta2, double eps, double weight_decay,
                              int decoupled, relax_stream stream);

/* ---- correlation metrics of a head's predictions (csrc/metrics.hip, csrc/metrics_core.h) ----- */
/* compute_correlation_metrics (src/model_regression.py:149-161) with fit_logistic_regression / logistic_func (:138-147) on the
 * device: y_true / y_pred DEVICE fp64 [n], 2 <= n <= 131072 (beyond that n^3 leaves the exact range of the rank sums;
 * RELAX_ERR_INVALID).  out: 17 doubles, DEVICE or HOST memory -
 *   [0] plcc   pearson(y_true, fitted)            [1] rmse   sqrt(mean((y_true - fitted)^2))
 *   [2] srcc   Spearman's rho of the average ranks [3] krcc   Kendall's tau-b
 *   [4..7] popt = b1..b4 of  b2 + (b1 - b2) / (1 + exp(-(x - b3) / |b4|))  fitted to (x = y_pred, y = y_true)
 *   [8] iterations (trial points of the Levenberg-Marquardt loop)   [9] converged (1: the stopping rule was met; 0: the
 *   iteration cap or the damping limit ended the loop)   [10] cost at p0   [11] final cost (sums of squared residuals)
 *   [12] count of non-finite inputs   [13..16] p0 = max(y_true), min(y_true), mean(y_pred), 0.5 (the reference's beta)
 * y_pred_logistic: DEVICE fp64 [n] or NULL, the fitted scores.  The fit replaces scipy.optimize.curve_fit's MINPACK run (analytic
 * Jacobian; ftol = xtol = 1.49e-8 as curve_fit sets them) in ONE persistent launch, bit-reproducible from run to run.  Any
 * non-finite input makes [0..7], [10], [11], [13..16] and the fitted scores NaN and [12] its count; that is not an error status.
 * With `out` in device memory the call only enqueues on `stream`; with `out` in host memory it copies the results and waits for
 * `stream`.  Uses a workspace the handle owns (20 bytes per element). */
int relax_metrics_correlation(relax_handle* h, const double* y_true, const double* y_pred, int n, double* out, double* y_pred_logistic,
                              relax_stream stream);
/* The pair pass alone: scipy.stats.kendalltau / spearmanr of model_regression.py:154-157 (the per-epoch selection metric of
 * :425-429).  x / y DEVICE fp64 [n], n as above; out: 8 doubles, DEVICE or HOST (as above) -
 *   [0] krcc = S / sqrt((n0 - n1) (n0 - n2))   [1] srcc   [2] S = concordant - discordant pairs   [3] n1, [4] n2 = pairs tied in
 *   x, in y   [5] n0 = n (n - 1) / 2   [6] count of non-finite inputs (then [0], [1] are NaN)   [7] 0
 * All counting is in integers, so the result does not depend on the launch geometry; krcc / srcc are NaN for a constant input. */
int relax_metrics_kendall(relax_handle* h, const double* x, const double* y, int n, double* out, relax_stream stream);
/* The per-element counters the pair pass leaves (a test / inspection path): counts DEVICE int32 [5][n] = values below x[i],
 * values equal to x[i] (itself included), the same two for y, and the sum over j of sign(x[i] - x[j]) sign(y[i] - y[j]).
 * The average rank of x[i] is below + (equal + 1) / 2.  Enqueued on `stream`. */
int relax_metrics_pair_counts(relax_handle* h, const double* x, const double* y, int n, int32_t* counts, relax_stream stream);

/* ---- operator level (what the backbones are built from; parity-tested one by one) ------------ */
/* out[M,N] = act(A[M,K] * W[N,K]^T + bias[N] + residual[M,N]);  act: 0 none, 1 relu, 2 gelu(erf).
 * fp32 in, fp32 MFMA accumulate.  K % 32 == 0 (bf16x6: K % 16 == 0), N % 64 == 0.  bias/residual may be NULL; every pointer
 * 16-byte aligned.  These operator-level entry points are test / bench paths: under "gemm_precision" 3 (default; N % 256 == 0)
 * both operands are converted to fp16 planes on every call, each row with the power-of-two scale of its own maximum; under 2 (and under
 * 3 for the other shapes) the operands are converted to split planes on every call (two extra kernels, (M+N)*K*6 bytes; the model drivers keep weights
 * and activations in that format instead; where N % 256 != 0 only W is converted: the 64 / 128-column form of the kernel
 * splits the fp32 rows of A in its K loop, as ResNet-50's layer1 / layer2 do), into a workspace the handle owns - like every entry point they must not run
 * concurrently on two streams of one handle.  Finite operands up to 3.38e38 (csrc/sp3.h); beyond: "gemm_precision" 0. */
int relax_op_gemm(relax_handle* h, const float* A, const float* W, const float* bias, const float* residual,
                  float* out, int M, int N, int K, int act, relax_stream stream);
/* NHWC conv as implicit GEMM: in [Nimg,H,W,Cin], w [Cout, KH*KW*Cin (padded to %32)] (k = (dy*KW+dx)*Cin+c),
 * out [Nimg,Ho,Wo,Cout].  Cin a power of two >= 4 when KH*KW > 1.  Under "gemm_precision" 2 the bf16x6 kernel takes
 * geometries with Cin % 16 == 0, KH*KW <= 32 and Cout % 64 == 0; every other one runs on the exact-fp32 kernel. */
int relax_op_conv2d_nhwc(relax_handle* h, const float* in, const float* w, const float* bias,
                         const float* residual, float* out, int Nimg, int H, int W, int Cin, int Cout,
                         int KH, int KW, int stride, int pad, int act, relax_stream stream);
/* relax_op_conv2d_nhwc under "gemm_precision" 3 with the outputs of the epilogue that only the model drivers use (a test / bench
 * path like its neighbours; every other precision is refused).  Conversions, geometry rules and dispatch are those of
 * relax_op_conv2d_nhwc under f16x2: the wide form (Cin % 32 == 0, Cout % 256 == 0) runs gemm_h3, the narrow form (a KxK filter,
 * Cin % 16 == 0, K = KH*KW*Cin a multiple of 32 and >= 256, Cout % 64 == 0 but not % 256) runs gemm_x6<H2>; a geometry with neither
 * form is refused, it does not fall back to another kernel.  M = Nimg*Ho*Wo.  The optional arguments go into the launch unchanged
 * (NULL / 0 = absent); what the launchers refuse comes back as RELAX_ERR_INVALID with their message and nothing of it runs:
 *   amax_out       DEVICE uint32 [Nimg], zeroed here: the bits of each image's largest output (needs act == 1: the integer maximum
 *                  of float bits orders non-negative values only)
 *   out_h2         DEVICE [M][Cout*4 B]: the outputs as two fp16 planes (csrc/h2.h: per 16 values 16 x hi, 16 x lo), image i's rows
 *                  scaled by img_out_scale[i] (DEVICE fp32 [Nimg], powers of two from the caller); narrow form: needs act == 1
 *   residual_h2    DEVICE [M][Cout*4 B] with img_res_inv [Nimg]: the residual as planes, (hi + lo) * img_res_inv[image], instead of
 *                  `residual` (wide form only)
 *   gap_groups     DEVICE fp32 [M/g][Cout]: the first stage of the fused spatial mean, sums over aligned groups of g rows; g = 4 on
 *                  the wide form, 16 on the narrow form (4 where Ho*Wo % 16 != 0); needs Ho*Wo % 4 == 0.  Groups that start below
 *                  gap_rows are written, rows below out_rows get the fp32 `out` (0 = all); `out` may be NULL if another output is asked for
 *   no_split       never cut tail tiles along K
 *   w3, bias3, Cout3   the back-to-back form, plain variant (narrow form, Cout = 64 or 128, act == 1, Ho*Wo >= 256 and % 16 == 0):
 *                  relu(conv(in) + bias) stays on the chip as the A operand of a 1x1 onto Cout3 columns, w3 fp32 [Cout3][Cout] (packed
 *                  here with the driver's K permutation), bias3 [Cout3]; `residual` (fp32, required), `out`, `out_h2`, `amax_out`
 *                  and `gap_groups` then describe relu(that 1x1 + bias3 + residual), [M][Cout3].  The first-block variant (second
 *                  conv3 source, concatenated downsample weights) and the stride-2 plane sample are not reachable from here. */
int relax_op_conv2d_nhwc_ex(relax_handle* h, const float* in, const float* w, const float* bias, const float* residual,
                            const void* residual_h2, const float* img_res_inv, float* out, void* out_h2, const float* img_out_scale,
                            uint32_t* amax_out, float* gap_groups, int gap_rows, int out_rows, int no_split, const float* w3,
                            const float* bias3, int Cout3, int Nimg, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                            int pad, int act, relax_stream stream);
/* rows of `dim` floats: y = (x-mean)/sqrt(var+eps)*gamma+beta */
int relax_op_layernorm(relax_handle* h, const float* x, const float* gamma, const float* beta, float* y,
                       int rows, int dim, float eps, relax_stream stream);
/* qkv [Nimg*197, 3*heads*64] -> out [Nimg*197, heads*64]; softmax(q k^T / 8) v per (image, head) */
int relax_op_attention(relax_handle* h, const float* qkv, float* out, int Nimg, int heads, relax_stream stream);
/* The streaming kernel (csrc/attention_stream.hip: key tiles of 32, online softmax) at ANY token count ntok >= 1 - also at 197,
 * where the forwards run the single-tile kernels (a test / benchmark entry point): qkv [Nimg*ntok, 3*heads*64] -> out
 * [Nimg*ntok, heads*64].  The arithmetic is the one the ViT forward's attention has under the current "gemm_precision": exact
 * fp32 MFMA under 0 (and 1), bf16x6 under 2, and under 3 the f16x2 kernel (csrc/attention_stream_h2.hip: key tiles of 64, one scale
 * from the tensor's measured maximum) with "att_h2" and "att_h2_stream" on, bf16x6 otherwise. */
int relax_op_attention_ex(relax_handle* h, const float* qkv, float* out, int Nimg, int ntok, int heads, relax_stream stream);
/* relu(x*scale[c]+shift[c]) then 3x3/s2/p1 max-pool: [Nimg,H,W,C] -> [Nimg,H/2,W/2,C] */
int relax_op_bn_relu_maxpool(relax_handle* h, const float* x, const float* scale, const float* shift, float* y,
                             int Nimg, int H, int W, int C, relax_stream stream);
/* ... and with amax_out (DEVICE uint32 [Nimg], or NULL): the bits of each image's largest output, as ResNet-50's stem posts them
 * (a test path).  Needs whole 256-thread blocks per image: (H/2)*(W/2)*(C/4) % 256 == 0; any other map is refused. */
int relax_op_bn_relu_maxpool_amax(relax_handle* h, const float* x, const float* scale, const float* shift, float* y,
                                  uint32_t* amax_out, int Nimg, int H, int W, int C, relax_stream stream);
/* spatial mean: x [Nimg,HW,C] -> out[n*out_stride + c] */
int relax_op_gap(relax_handle* h, const float* x, float* out, int Nimg, int HW, int C, int64_t out_stride,
                 relax_stream stream);
/* The tail of the pool vectors as an op (a test entry point; the forwards reach the same kernel after the avgpool / fc2): row i of v
 * (DEVICE fp32, n rows of dim floats, v_stride >= dim floats apart) -> out[i*out_stride + 0 .. dim-1] = the row, bit for bit, then its
 * mean, max and population std at dim, dim + 1, dim + 2 (out_stride >= dim + 3; nothing else of `out` is written).  dim is 2048
 * (ResNet-50's pool vector) or 4096 (VGG-16's); any other dim is refused, the message names it.  Enqueued on `stream`. */
int relax_op_pool_stats(relax_handle* h, const float* v, int64_t v_stride, float* out, int64_t out_stride, int n, int dim,
                        relax_stream stream);

/* x [Nimg, tokens, dim] -> out [Nimg, 3*dim] = per-channel mean | max | population std over tokens
 * (process_video_feature, vit branch: src/main_residual_fragment.py:128-136; src/main_fragment_pool.py:124-133) */
int relax_op_token_stats(relax_handle* h, const float* x, float* out, int Nimg, int tokens, int dim,
                         relax_stream stream);
/* One tap of relax_vit_intermediate_layers as an op (csrc/vit_layers.hip): LayerNorm of x [Nimg, ntok, dim] fused with the statistics of
 * its rows - cls_out [Nimg, dim] = the normed row 0, pooled_out [Nimg, 3*dim] = mean | max | std over the normed rows 1 .. ntok - 1 (either
 * may be NULL, not both); the bits of relax_op_layernorm followed by relax_op_token_stats on rows 1...  dim a multiple of 64 up to 768,
 * ntok 2 .. 4097. */
int relax_op_vit_norm_token_stats(relax_handle* h, const float* x, const float* gamma, const float* beta, float eps, float* cls_out,
                                  float* pooled_out, int Nimg, int ntok, int dim, relax_stream stream);

/* Device-to-device copy on the caller's stream (the fragment batch of one backbone duplicated for the other). */
int relax_copy_bytes(relax_handle* h, const void* src, void* dst, int64_t n_bytes, relax_stream stream);

/* Per-clip mean over frames (src/demo_test.py:171-175, src/data_processing/extract_npy2mat.py:121-126) of one column block
 * of a per-frame feature matrix: dst[s, dst_col0 + c] = mean of src[row0 + r, c] over r in [seg_offsets[s], seg_offsets[s+1]),
 * c < ncols.  seg_offsets: HOST int32 [nseg + 1] (prefix sums of the frames per clip; passed to the kernel by value, so the
 * call stays capturable into a HIP graph).  Rows are summed in order. */
int relax_segment_mean(relax_handle* h, const float* src, int64_t src_stride, int ncols, int row0, const int32_t* seg_offsets,
                       int nseg, float* dst, int64_t dst_stride, int dst_col0, relax_stream stream);

/* ---- PNG decode ------------------------------------------------------------------------------- */
/* Per-image status words of relax_png_decode (0 = decoded). */
#define RELAX_PNG_OK 0
#define RELAX_PNG_BAD_ARGS 1             /* geometry refused, or a buffer range of the item out of bounds */
#define RELAX_PNG_BAD_ZLIB_HEADER 2      /* CMF/FLG: not deflate, window > 32 KiB or check bits wrong */
#define RELAX_PNG_PRESET_DICT 3          /* FDICT set: a preset dictionary is refused */
#define RELAX_PNG_TRUNCATED 4            /* the stream ends before its last block or its Adler-32 */
#define RELAX_PNG_BAD_BLOCK_TYPE 5       /* reserved block type 3 */
#define RELAX_PNG_BAD_STORED_LEN 6       /* stored block: LEN != ~NLEN */
#define RELAX_PNG_BAD_CODE_LENGTHS 7     /* over-subscribed or incomplete code, bad repeat, too many lengths, no end-of-block */
#define RELAX_PNG_BAD_SYMBOL 8           /* a literal/length or distance code that the block's code does not define */
#define RELAX_PNG_DIST_TOO_FAR 9         /* a distance reaching before the first byte */
#define RELAX_PNG_OUTPUT_TOO_LONG 10     /* more than H * (1 + W*C) bytes */
#define RELAX_PNG_OUTPUT_TOO_SHORT 11    /* fewer than H * (1 + W*C) bytes */
#define RELAX_PNG_BAD_FILTER 12          /* a row filter byte above 4 */
#define RELAX_PNG_BAD_ADLER 13           /* the Adler-32 of the inflated bytes differs from the stream's */
#define RELAX_PNG_OUT_TOO_SMALL 14       /* relax_png_encode: the item's output slot is shorter than its stream */

/* The image data of N PNG files -> uint8 BGR, as cv2.imread (src/main_fragment_layerstack.py:295-296) returns it: RGB
 * swapped, alpha dropped, gray replicated.  The caller parses the container (signature, IHDR, chunk CRCs) and concatenates
 * each file's IDAT payloads into one zlib stream; only 8-bit, non-interlaced gray (C = 1), RGB (3) and RGBA (4) images with
 * W*C <= 16384 come here, every other file is decoded on the host.
 *   src     DEVICE bytes [src_bytes]: the zlib streams
 *   items   DEVICE int64 [N][8]: src offset, src length, raw offset, out offset, H, W, C, 0
 *   out     DEVICE uint8 [out_bytes]: image n is written as [H][W][3] at out + out offset (n * item_stride for a batch tensor;
 *           any slot of a clip tensor [T,2,H,W,3])
 *   raw     DEVICE uint8 [raw_bytes]: scratch, H * (1 + W*C) bytes per image at its raw offset (the inflated rows)
 *   status  DEVICE int32 [N]: RELAX_PNG_* per image
 * One 64-lane workgroup per image, on `stream`.  Every read of image n stays inside its stream and every write inside its raw
 * range and its output slot (ranges outside the buffers give RELAX_PNG_BAD_ARGS); a corrupt stream stops only its own image.
 * No handle and no library state: the caller owns all memory, so loader threads may call this at the same time, each with its
 * own scratch and its own stream (the Python layer keeps one decoder, stream and scratch per thread).  Returns
 * RELAX_ERR_INVALID for bad arguments, RELAX_ERR_HIP if the launch fails; the per-image outcome is in `status`. */
int relax_png_decode(const uint8_t* src, int64_t src_bytes, const int64_t* items, int N, uint8_t* out, int64_t out_bytes,
                     uint8_t* raw, int64_t raw_bytes, int32_t* status, relax_stream stream);

/* ---- PNG encode ------------------------------------------------------------------------------- */
/* Device images -> the zlib streams of their PNG files, what cv2.imwrite leaves behind for the fragments, residuals, flow
 * images and overlays (src/main_fragment_layerstack.py:310,325, src/main_residual.py:230,241, src/demo_test.py:120,135): BGR
 * (C = 3) is written as RGB, colour type 2; C = 1 is colour type 0.  Equality with OpenCV's files is on the decoded pixels.
 * The caller wraps each stream into the container (signature, IHDR, IDAT, IEND, CRCs).  The stream is cut into bands of whole
 * rows, one workgroup per band, all bands of all N images in one launch; per band: the row filter with the smallest sum of
 * absolute values (ties to the lower number), run-length matches (distance 1), one dynamic Huffman block or - where shorter -
 * a stored block, and an empty stored block that byte-aligns the band; a second pass places the bands of each image behind the
 * header 78 01 and appends the combined Adler-32.
 *
 * relax_png_encode_bound: host arithmetic.  Returns the largest stream an H x W x C image can produce (exactly what an
 * incompressible image produces), < 0 for a refused geometry (C not 1 or 3, W*C > 16384, H > 2^24, filter outside -1..4);
 * *scratch_bytes = the scratch the image needs (a call needs the sum over its items), *band_rows = rows per band. */
int64_t relax_png_encode_bound(int H, int W, int C, int filter, int64_t* scratch_bytes, int* band_rows);
/*   images  DEVICE uint8 [images_bytes]
 *   items   DEVICE int64 [N][8]: image offset, row stride (bytes, >= W*C), H, W, C (1 or 3), out offset, out capacity,
 *           filter (-1: chosen per row, 0..4: that filter for every row)
 *   out     DEVICE uint8 [out_bytes]: item n's stream at its out offset
 *   scratch DEVICE uint8 [scratch_bytes], 8-byte aligned, at least 64 + 64 * N bytes; contents on entry are ignored
 *   lengths DEVICE int64 [N]: stream length (0 unless status is RELAX_PNG_OK)
 *   status  DEVICE int32 [N]: RELAX_PNG_OK, RELAX_PNG_BAD_ARGS (geometry, or a range of the item outside images / out /
 *           scratch) or RELAX_PNG_OUT_TOO_SMALL
 * Every read of item n stays inside its rows and every write inside its scratch range and its output slot; a bad item stops
 * only itself.  No handle and no library state, as relax_png_decode: writer threads may call it at the same time, each with
 * its own scratch and stream.  The same input gives the same bytes on every call (and the bytes of the host build of
 * csrc/png_deflate.h).  Returns RELAX_ERR_INVALID for bad arguments, RELAX_ERR_HIP if a launch fails. */
int relax_png_encode(const uint8_t* images, int64_t images_bytes, const int64_t* items, int N, uint8_t* out, int64_t out_bytes,
                     uint8_t* scratch, int64_t scratch_bytes, int64_t* lengths, int32_t* status, relax_stream stream);
/* The same call cut into its launches, for measurement (tools/png_encode_bench.py times the compaction alone on a scratch
 * that PLAN | BANDS of an earlier call left behind): `passes` is a set of the bits below, run in this order; all of them is
 * relax_png_encode.  PLACE and COPY read only what the same arguments' PLAN and BANDS wrote into `scratch`. */
#define RELAX_PNG_ENCODE_PLAN 1          /* items -> bands and their scratch slots (one workgroup) */
#define RELAX_PNG_ENCODE_BANDS 2         /* filter + deflate, one workgroup per band */
#define RELAX_PNG_ENCODE_PLACE 4         /* per image: prefix sums, zlib header, Adler-32, length, status */
#define RELAX_PNG_ENCODE_COPY 8          /* every band to its place in the output slot */
#define RELAX_PNG_ENCODE_ALL 15
int relax_png_encode_passes(const uint8_t* images, int64_t images_bytes, const int64_t* items, int N, uint8_t* out,
                            int64_t out_bytes, uint8_t* scratch, int64_t scratch_bytes, int64_t* lengths, int32_t* status,
                            int passes, relax_stream stream);

/* ---- raw YUV frames ---------------------------------------------------------------------------- */
/* Headerless 8-bit YUV video -> uint8 HWC BGR: the frames the reference has ffmpeg cut out of raw files
 * (`-s WxH -pix_fmt yuv420p -framerate r -i file.yuv`, src/video_frames_extract.py:29-49,76-100; the input path of the
 * live_qualcomm dataset), converted on the device from the file's own bytes.
 *
 * Arithmetic, per pixel, integers throughout, >> an arithmetic shift, U' = U - 128, V' = V - 128:
 *     y = cy*(Y - oy) + 32768
 *     R = clip8((y + crv*V') >> 16)    G = clip8((y - cgu*U' - cgv*V') >> 16)    B = clip8((y + cbu*U') >> 16)
 *                                  cy   oy     crv     cbu    cgu    cgv
 *     BT.601 limited (yuv420p..)  76309  16  104597  132201  25675  53279   what swscale assumes for untagged raw input
 *     BT.601 full    (yuvj*)      65536   0   91881  116130  22553  46801
 *     BT.709 limited              76309  16  117489  138438  13975  34925   round(65536 * coefficient), Kr 0.2126, Kb 0.0722,
 *     BT.709 full                 65536   0  103206  121609  12276  30679   limited: chroma * 255/224, cy = 255/219
 * Within 1 code value of the float64 conversion on every (Y,U,V) triple.  Chroma is replicated, as swscale's unscaled
 * yuv->rgb path does it: pixel (r, c) takes chroma sample (r>>1, c>>1) for 4:2:0 and NV12, (r, c>>1) for 4:2:2, (r, c) for
 * 4:4:4; odd W or H have chroma planes of ceil(W/2) x ceil(H/2), ffmpeg's raw frame layout.  The output is pinned to this
 * formula, not to any ffmpeg build (swscale's SIMD paths are not bit-exact with its own C path). */
#define RELAX_YUV_420P 0   /* Y[H][W], U[ch][cw], V[ch][cw]; yuv420p / yuvj420p */
#define RELAX_YUV_422P 1   /* Y[H][W], U[H][cw], V[H][cw] */
#define RELAX_YUV_444P 2   /* Y[H][W], U[H][W], V[H][W] */
#define RELAX_YUV_NV12 3   /* Y, then interleaved UV: what hardware decoders emit */
#define RELAX_YUV_BT601 0
#define RELAX_YUV_BT709 1
#define RELAX_YUV_MAX_DIM 16384          /* W and H: 1..16384 */
/* Per-item status words of relax_yuv_to_bgr. */
#define RELAX_YUV_OK 0
#define RELAX_YUV_OUT_OF_RANGE 1         /* the item's frame leaves src or its slot leaves out: nothing of it was written */

/* Bytes of one frame; host arithmetic.  < 0: layout, H or W refused. */
int64_t relax_yuv_frame_bytes(int layout, int H, int W);

/* The table above, from the library: out[6] = cy, oy, crv, cbu, cgu, cgv (HOST memory; host arithmetic).  RELAX_ERR_INVALID for
 * another matrix or range.  The Python layer reads its constants here, so host and device share one table. */
int relax_yuv_coefficients(int matrix, int full_range, int32_t* out);

/*   src     DEVICE bytes [src_bytes]: whole frames, anywhere in it (frame k of a raw file starts at k * frame_bytes)
 *   items   DEVICE int64 [N][2]: source offset of the frame, output offset
 *   out     DEVICE uint8 [out_bytes]: item n is written as [H][W][3] BGR at out + output offset - any slot of a clip tensor
 *           [T,2,H,W,3]; a sampled frame and its successor are two items, so one launch fills a clip
 *   status  DEVICE int32 [N]: RELAX_YUV_* per item, always written
 * Every read of item n stays inside [offset, offset + frame_bytes) and every write inside its H*W*3 slot; an item whose
 * ranges leave src or out writes nothing and gets RELAX_YUV_OUT_OF_RANGE, the other items of the call are unaffected.
 * Each lane converts 16 pixels of the two rows that share a chroma row (one row for 4:2:2 and 4:4:4).  An item moves 16 bytes
 * per access (Y 16, U and V 8 each - 16 for 4:4:4 and for NV12's interleaved row -, output 3 x 16) only when W is a multiple
 * of 16 and both src + source offset and out + output offset are 16-byte-aligned addresses; any one of them off puts THAT
 * item on the much slower bytewise path (frame_bytes of a raw file is often no multiple of 16: copy the frames to aligned
 * slots, as sampling.GpuYuvLoader does).  Plain vector loads and stores, no inline assembly (csrc/yuv.hip; layout and
 * bounds arithmetic in csrc/yuv_core.h, which the CPU tests run on the host).
 * No handle and no library state, as relax_png_decode: loader threads call it at the same time on their own streams.
 * Returns RELAX_ERR_INVALID, with the offending value in relax_last_error(NULL), for any other layout or matrix, full_range
 * outside 0..1, W or H outside 1..RELAX_YUV_MAX_DIM, or bad buffers; RELAX_ERR_HIP if the launch fails. */
int relax_yuv_to_bgr(const uint8_t* src, int64_t src_bytes, const int64_t* items, int N, int layout, int H, int W, int matrix,
                     int full_range, uint8_t* out, int64_t out_bytes, int32_t* status, relax_stream stream);

/* ---- raw YUV frames: 10 / 12-bit, packed 4:2:2, 4:1:1, 4:1:0 and NV21 -------------------------------- */
/* The pixel formats that `ffmpeg -f rawvideo` leaves behind for the reference's datasets (metadata column `pixfmt`; the frames
 * of src/video_frames_extract.py:29-49,76-100): the `_ex` entries take a FORMAT where relax_yuv_to_bgr takes a layout.
 * Formats 0..3 are RELAX_YUV_420P/422P/444P/NV12 and run relax_yuv_to_bgr's own kernels: the same bytes.  A frame, as
 * ffmpeg writes it raw (cw = ceil(W / 2^hshift), ch = ceil(H / 2^vshift)):
 *     NV21                as NV12 with V first
 *     YUYV422, UYVY422    one plane: rows of ceil(W/2) four-byte groups Y0 U Y1 V / U Y0 V Y1; for odd W the last group's second
 *                         luma is padding - present in the file, never shown
 *     411P                Y[H][W], U and V [H][ceil(W/4)]
 *     410P                Y[H][W], U and V [ceil(H/4)][ceil(W/4)]
 *     4xxP10LE, 4xxP12LE  the 8-bit planar layouts with 2-byte little-endian samples; the value sits in the low `depth` bits,
 *                         HIGHER BITS ARE MASKED OFF
 *     P010LE              NV12's layout with 2-byte samples; the value is the HIGH 10 bits (word >> 6), the low 6 are ignored
 * Chroma is replicated: pixel (r, c) takes sample (r >> vshift, c >> hshift), no interpolation.
 *
 * Arithmetic, one formula for every depth, s = depth - 8, the coefficient table of relax_yuv_to_bgr unchanged:
 *     y = cy*(Y - (oy << s))      u = U - (128 << s)      v = V - (128 << s)
 *     channel = clamp(sum + (1 << (15+s)), 0, 2^(24+s) - 1) >> (16+s)        sum = y + crv*v | y - cgu*u - cgv*v | y + cbu*u
 * At s = 0 this is relax_yuv_to_bgr's formula bit for bit.  depth <= 12 keeps every sum inside int32.  Within 1 code value of
 * the float64 BT.601 / BT.709 conversion rounded to 8 bits.  The output is pinned to this formula and to float64 BT.601 /
 * BT.709, not to any ffmpeg build; for sources deeper than 8 bits ffmpeg's PNG path goes through 16-bit RGB and OpenCV
 * reduces that to 8 bits - that rounding is NOT pinned here. */
#define RELAX_YUVF_420P 0
#define RELAX_YUVF_422P 1
#define RELAX_YUVF_444P 2
#define RELAX_YUVF_NV12 3
#define RELAX_YUVF_NV21 4
#define RELAX_YUVF_YUYV422 5
#define RELAX_YUVF_UYVY422 6
#define RELAX_YUVF_411P 7
#define RELAX_YUVF_410P 8
#define RELAX_YUVF_420P10LE 9
#define RELAX_YUVF_422P10LE 10
#define RELAX_YUVF_444P10LE 11
#define RELAX_YUVF_420P12LE 12
#define RELAX_YUVF_422P12LE 13
#define RELAX_YUVF_444P12LE 14
#define RELAX_YUVF_P010LE 15
#define RELAX_YUVF_COUNT 16
#define RELAX_YUV_PACKING_PLANAR 0
#define RELAX_YUV_PACKING_SEMIPLANAR 1
#define RELAX_YUV_PACKING_PACKED 2
#define RELAX_YUV_FORMAT_INFO_WORDS 8

/* Bytes of one frame (src/video_frames_extract.py:29-49,76-100: what one `-s WxH -pix_fmt F` frame occupies in the raw file);
 * host arithmetic, answers without a GPU.  -1: format, H or W refused. */
int64_t relax_yuv_frame_bytes_ex(int format, int H, int W);

/* The one format table (csrc/yuv_core.h), for the layers that restate the layout of src/video_frames_extract.py:29-49,76-100's
 * input: out[RELAX_YUV_FORMAT_INFO_WORDS] (HOST memory) = bytes per sample, depth, shift (sample = (word >> shift) & (2^depth - 1)),
 * hshift, vshift, packing (RELAX_YUV_PACKING_*), swap (semi-planar: 1 = V first; packed: 1 = chroma first), 0.
 * RELAX_ERR_INVALID, naming the value, for a format outside 0..RELAX_YUVF_COUNT-1 or a NULL out. */
int relax_yuv_format_info(int format, int32_t* out);

/* relax_yuv_to_bgr (the frames of src/video_frames_extract.py:29-49,76-100) for every RELAX_YUVF_* format: the same arguments,
 * item rule, status words and refusals, `format` in place of `layout`.  One lane takes 16 pixels of the 1, 2 or 4 rows that share
 * a chroma row; all of its loads are in flight before its first store; each row leaves as three 16-byte stores.  The 16-byte path
 * under relax_yuv_to_bgr's conditions (W a multiple of 16, frame and slot at 16-byte-aligned addresses): per lane and row two
 * 16-byte loads of 16-bit luma or of a packed row (which holds its chroma), per lane one 16-byte load per plane of 16-bit 4:2:0 /
 * 4:2:2 chroma, two of 16-bit 4:4:4 chroma and of P010's interleaved pairs, one dword per plane of 4:1:1 / 4:1:0 chroma;
 * everything else bytewise with every index under its bound.  Kernels specialised on sample bytes, packing, hshift and vshift
 * (csrc/yuv.hip); offsets, widths and arithmetic in csrc/yuv_core.h, which csrc/yuv_ex_host.cpp walks on the host. */
int relax_yuv_to_bgr_ex(const uint8_t* src, int64_t src_bytes, const int64_t* items, int N, int format, int H, int W, int matrix,
                        int full_range, uint8_t* out, int64_t out_bytes, int32_t* status, relax_stream stream);

/* relax_yuv_greyscale_scan (the screen of the frames of src/video_frames_extract.py:29-49,76-100) for every RELAX_YUVF_* format:
 * each pixel converted in registers by the arithmetic above and folded into the record, no BGR written, no shortcut on neutral
 * chroma.  For every frame the record equals relax_greyscale_scan's on relax_yuv_to_bgr_ex's output.  Arguments, status and
 * refusals as relax_yuv_greyscale_scan, `format` in place of `layout`. */
int relax_yuv_greyscale_scan_ex(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, int N, int format, int H, int W,
                                int matrix, int full_range, int32_t* out, relax_stream stream);

/* ---- greyscale screen ----------------------------------------------------------------------------- */
/* The pixel rule of the reference's src/data_processing/check_greyscale.py (is_greyscale_image, :25-35): a BGR frame is
 * greyscale iff the largest b-g, b-r and g-r over its pixels are all <= 3 - where b, g and r are uint8, so each difference
 * WRAPS modulo 256 before the maximum is taken (b - g = -1 counts as 255).  Both entries reduce every frame to one record of
 * RELAX_GREYSCALE_RECORD_WORDS int32:
 *     [0..2]  max over the pixels of (b-g) mod 256, (b-r) mod 256, (g-r) mod 256      the reference's rule
 *     [3..5]  max over the pixels of |b-g|, |b-r|, |g-r|                              the rule without the wrap
 *     [6]     status: RELAX_YUV_OK, or RELAX_YUV_OUT_OF_RANGE (relax_yuv_greyscale_scan only; the maxima are 0 then)
 *     [7]     0
 * so any threshold, under either rule, is a comparison on the record.  Every word of every record is defined by the call,
 * whatever `out` held; maxima do not depend on the order of arrival, so the records are the same bits on every run.  No handle
 * and no library state (as relax_yuv_to_bgr): loader threads call them at the same time on their own streams.  Plain vector
 * loads, a wave and block maximum, one atomicMax per block and word; no inline assembly (csrc/greyscale.hip; the per-lane
 * arithmetic in csrc/greyscale_core.h, which the CPU tests run on the host). */
#define RELAX_GREYSCALE_RECORD_WORDS 8

/*   frames  DEVICE uint8: frame n is [H][W][3] BGR with packed rows at frames + n * frame_stride (frame_stride >= H*W*3 bytes when
 *           N > 1: the frames of a [N,H,W,3] tensor, the slots of a [T,2,H,W,3] clip, or a strided view of either)
 *   out     DEVICE int32 [N][RELAX_GREYSCALE_RECORD_WORDS]
 * A frame is read as H*W consecutive pixels, 16 to a lane: three 16-byte loads when the frame's first byte lies at a
 * 16-byte-aligned address (any W: 48 bytes per lane keep every lane aligned), with the last H*W mod 16 pixels bytewise; a frame at
 * any other address goes bytewise altogether.  N beyond 65535 is split over launches.
 * Returns RELAX_ERR_INVALID, with the offending value in relax_last_error(NULL), for H or W outside 1..RELAX_YUV_MAX_DIM,
 * N < 0, a frame_stride below H*W*3 with N > 1, or a NULL buffer with N > 0 - before anything is launched; RELAX_ERR_HIP if a
 * launch fails. */
int relax_greyscale_scan(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int32_t* out, relax_stream stream);

/* The same records straight from raw YUV frames: each pixel is converted in registers by relax_yuv_to_bgr's arithmetic and goes
 * into the maxima; no BGR is written.  For every frame the record equals relax_greyscale_scan's on relax_yuv_to_bgr's output
 * for that frame (no shortcut on U == V == 128: the rule is on the converted BGR).
 *   src      DEVICE bytes [src_bytes]; offsets  DEVICE int64 [N]: where frame n starts in src
 *   layout, H, W, matrix, full_range: as relax_yuv_to_bgr, with its 16-byte path under its conditions (W a multiple of 16,
 *   src + offset 16-byte aligned) and its bytewise path otherwise, per frame
 * A frame whose range leaves src gets status RELAX_YUV_OUT_OF_RANGE and zero maxima, and is not read; the other frames of the
 * call are unaffected.  Refusals as relax_yuv_to_bgr's. */
int relax_yuv_greyscale_scan(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, int N, int layout, int H, int W,
                             int matrix, int full_range, int32_t* out, relax_stream stream);

/* ---- measurement ----------------------------------------------------------------------------- */
/* While enabled, every launch of the contraction kernel (GEMM / implicit-GEMM conv) and of the patch-score
 * kernel is bracketed by HIP events on the caller's stream.  relax_profile_read synchronises those events and
 * returns totals since the last enable: kind 0 = fp32 / bf16x3 contraction launches (work = algorithmic FLOPs), kind 1 =
 * patch score (work = bytes), kind 2 = kind 0 again with work = algorithmic HBM bytes (operands and results touched once),
 * kind 3 / 4 = the same two views of the bf16x6 contraction launches, kind 7 / 8 = those of the f16x2 launches, kind 9 / 10 = those of the
 * plain f16x2 GEMMs alone (gemm_h3 without the convolution form: the ViT's GEMMs, the dominant kernel of the headline), kind 5 = flow_iteration, the dominant kernel of the
 * Farneback stage (one launch per iteration; work = algorithmic bytes: 56 per pixel, level and iteration), kind 6 = the whole
 * Farneback stage of a relax_optical_flow chunk, first launch to last (work = the algorithmic bytes of all its kernels: every
 * kernel's inputs read once and outputs written once; launches = chunks). */
int relax_profile_enable(relax_handle* h, int on);
int relax_profile_read(relax_handle* h, int kind, double* total_ms, double* total_work, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* RELAX_HIP_H */
