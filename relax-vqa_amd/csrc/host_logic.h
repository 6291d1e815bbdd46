// Pure-host half of librelax_hip.so: everything the model loaders and the launchers compute on the CPU before a byte goes
// to the GPU - state-dict key matching, reading and folding a BatchNorm (read_bn), OIHW -> packed [Cout][K] weight layout, the Hoelder
// constants of a folded convolution (conv_hoelder), the quality head's fc1 + BatchNorm1d fold, the tail split-K cost model of the
// contraction launchers, and the options of a handle (GemmOptions and the table relax_set_option / relax_get_option / relax_create go by).  No HIP type appears here, so the file
// builds with plain g++ and runs under AddressSanitizer / UBSan on a CPU box (tests/test_host_logic_sanitized.py drives it with the
// synthetic and the deliberately malformed state dicts; sanitizers are never run on the GPU).
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <utility>

namespace relax {

// Tuning / reproducibility switches of the contraction kernel (relax_set_option; env defaults RELAX_GEMM_*): plain data, one
// row of host::kOptions per field.
struct GemmOptions {
    int precision = 3; // "gemm_precision": 3 = f16x2 (default,  fp32-grade: two fp16 planes, four products in two MFMAs - gemm_h2.hip - for the
                       // plain GEMMs with N % 256 == 0, i.e. the whole ViT; everything else as under 2), 2 = bf16x6 (fp32-grade), 0 = exact fp32
                       // MFMA, 1 = bf16x3 split products (~1e-5 relative)
    int h2_stages = 3; // "h2_stages": LDS stages of the 16-k form of the f16x2 kernel (3 or 4; same bits)
    int h2_form = 1;   // "h2_form": 1 = 32-k steps, three products (al bl dropped) for K >= 256, four below; 0 = 16-k steps, four products;
                       // 2 = 32-k steps, four products
    int split_k = 1;   // "gemm_split_k": tail split-K on (1) / off (0: K sums are batch-invariant bit for bit)
    int variant = -1;  // "gemm_variant": exact-fp32 kernel only: pin the tile variant for N % 128 == 0 problems, -1 = automatic
    int variant_n64 = -1;  // "gemm_variant_n64": same for N % 128 != 0 (N = 64 layers)
    int group_m = 8;   // "gemm_group_m": row-tiles per L2 group
    int flow_max_pairs = 0;  // "flow_max_pairs": cap on the pairs per optical-flow chunk (0 = by workspace size only)
    int flow_seg_rows = 0;       // "flow_seg_rows": rows per block of the Farneback iteration kernels, 0 = by the level's geometry (tests: the segmentation
                                 // restarts the running column sums - the flow must not depend on it)
    int flow_pyramid_fused = 1;  // "flow_pyramid_fused": 1 = the four pyramid-level inputs of a frame in one pass over its bytes (pyramid_fused; frames whose
                                 // height and width are multiples of 8), 0 = gray plane + per-level blur / resize kernels (any size) - same bits
    int flow_fused = 1;      // "flow_fused": 1 = one kernel per Farneback iteration (flow_iteration: M never leaves the chip); 0 = update_matrices_k +
                             // box_solve_fused (M through HBM) - same bits, the A/B switch of a test
    int rn_h2 = 1;         // "rn_h2": under "gemm_precision" 3, ResNet-50's layer3 / layer4 (the matrix-pipe-bound third of its time) run f16x2 with
                           // per-image scales; 0 = the whole network on bf16x6 (the A/B switch of a test)
    int att_h2 = 1;        // "att_h2": under "gemm_precision" 3 the ViT's attention runs on fp16 planes too (attention_h2.hip: the qkv GEMM writes planes,
                           // three products, no conversion passes); 0 = attention_x6 on the fp32 qkv output (three bf16 planes, six products)
    int att_h2_stream = 1;   // "att_h2_stream": with "att_h2", token counts other than 197 (patch-8 models, other canvases) run attention on fp16 planes too
                           // (attention_stream_h2.hip: the streaming form of attention_h2); 0 = attention_stream's bf16x6 form on the fp32 qkv output
    int rn_h2_early = 1;   // "rn_h2_early": with "rn_h2", the stem and the 3x3 convolutions of layer1 / layer2 (the MFMA-bound launches in front of layer3) run f16x2 too,
                           // on the four-wave tiles of gemm_x6.hip (conv1 writes its output as fp16 planes with the image's Hoelder scale); 0 = bf16x6 there
    int rn_c1_h2 = 1;      // "rn_c1_h2": with "rn_h2_early", the conv1 (1x1) of the layer1 / layer2 blocks whose input travels as fp32 rows runs f16x2 too: the rows
                           // are split into two fp16 planes in the K loop with the image's scale (from its measured maximum); 0 = bf16x6 (three planes, six products)
    int rn_fuse = 1;       // "rn_fuse": with "rn_h2_early", the blocks of layer1 / layer2 without a downsample branch run conv2 and conv3 back to back in ONE
                           // launch (the 3x3's output tile stays in registers as the A operand of the 1x1: no write and re-read of it, conv3 on f16x2
                           // with one scale per pixel row); 0 = two launches, conv3 on bf16x6 (the A/B switch of a test)
    int b2b_rows = 256;    // "b2b_rows": rows per tile of the back-to-back launches: 256 (two workgroups of four waves per CU) or 128 (three: measured
                           // slower, 2.49 against 2.13 ms per launch of layer1) - same bits
    int fp32_rows = 1;     // "x6_fp32_rows": bf16x6 contractions onto 64 / 128 columns take fp32 activation rows and split them in the K loop
                           // (ResNet-50 layer1 / layer2 block outputs travel as fp32); 0 = split planes everywhere (same bits, more bytes: the A/B switch of a test)
    int debug_poison = 0;  // "debug_poison": fill every workspace with 0xFF bytes when it is requested (test mode: reads of unwritten workspace surface as NaN)
};

namespace host {

// name -> (host pointer, element count) of a checkpoint as the C-ABI receives it (relax_load_resnet50 / _vit / _mlp_head)
struct StateDict {
    std::map<std::string, std::pair<const float*, int64_t>> t;
    // strip_module: drop a leading "module." (the reference's fix_state_dict, src/demo_test.py:25-35)
    void add(const char* name, const float* data, int64_t numel, bool strip_module = false);
    // the tensor under `key` if it has exactly `numel` elements (numel <= 0: any size); otherwise nullptr and a message in err
    const float* get(const std::string& key, int64_t numel, std::string& err, const char* what = "state dict") const;
    int64_t numel(const std::string& key) const;   // -1 if absent
};

// eval-mode BatchNorm as y = x * scale + shift:  scale = gamma / sqrt(var + eps),  shift = beta - mean * scale
void fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int channels, float* scale,
             float* shift);

// The BatchNorm under `prefix` (.weight, .bias, .running_mean, .running_var, `channels` values each) folded into scale / shift [channels];
// false and StateDict::get's message (it names the key) if one of the four is missing or mis-sized
bool read_bn(const StateDict& sd, const std::string& prefix, int channels, float eps, float* scale, float* shift, std::string& err);

// Hoelder constants of a convolution as packed rows [cout][k]:  |out[n]| <= l1max * max |in| + bmax  - what every per-image fp16 scale of the
// f16x2 ResNet-50 and VGG-16 rests on.  l1max = max_n (float)(sum_k |rows[n][k]| * (1 + 1e-6)), the sum in double in column order;
// bmax = max_n |bias[n]|, 0 without a bias
void conv_hoelder(const float* rows, const float* bias_or_null, int cout, int k, float* l1max, float* bmax);

// K of a packed convolution weight row: KH*KW*cin_pad rounded up to a multiple of 32
int conv_kpad(int k, int cin_pad);

// OIHW [cout][cin][k][k] -> [cout][kpad], column (dy*k + dx)*cin_pad + c, rows scaled by scale[o] (nullptr: 1), padding zero.
// out must hold cout * kpad floats.
void pack_conv_oihw(const float* w, const float* scale, int cout, int cin, int cin_pad, int k, int kpad, float* out);

// fc1 [h1][f] + BatchNorm1d(h1) -> w1p [h1][fpad] (zero padded), b1p [h1]:  y = (x W^T + b - mu) * s + beta
void fold_fc_bn(const float* w1, const float* b1, const float* gamma, const float* beta, const float* mean, const float* var,
                float eps, int h1, int f, int fpad, float* w1p, float* b1p);

// Tail split-K of a contraction launch.  `ntiles` output tiles over `slots` resident workgroups: the last, partial round
// (rem = ntiles % slots tiles) would leave most CUs idle, so its tiles may be cut along K into S slices.  Time of the tail in
// rounds = ceil(rem*S/slots)/S plus 4 % of a round per slice for writing and re-reading the partial tiles; S is kept at 1 unless
// splitting wins by more than 5 % of a round.  S <= 16 and every slice keeps at least `min_steps` K steps of the nk.
struct TailSplit {
    int full_tiles;   // tiles that run unsplit (launched first)
    int nsplit;       // slices per remaining tile (1 = no split)
};
TailSplit choose_tail_split(int ntiles, int slots, int nk, int min_steps, bool can_split);

// ---- Pillow's 8-bit resample on the host (resize.hip; relax_resize_table, relax_resize_output_size) ------------------------------------------
// The table of one pass, in_size -> out_size samples under filter 0 (BILINEAR, support 1) or 1 (LANCZOS, support 3): libImaging/Resample.c's
// precompute_coeffs for the box (0, in_size) + normalize_coeffs_8bpc, in the same double arithmetic - per output sample its first tap and tap
// count (bounds [out_size][2]) and its taps as 22-bit fixed point (coeffs [out_size][ksize], zero behind the count).
constexpr int kResizeMaxOut = 2048;    // output height / width (RELAX_RESIZE_MAX_OUT)
constexpr int kResizeMaxIn = 16384;    // input height, and in_size of a table (RELAX_RESIZE_MAX_IN_H)
int resize_ksize(int in_size, int out_size, int filt);
void resize_table(int in_size, int out_size, int filt, int32_t* bounds, int32_t* coeffs);
// The output size transforms.Resize(size) with an int gives a PIL image of H x W (torchvision's _compute_resized_output_size): the shorter
// side becomes `size`, the longer int(size * long / short); W is the shorter side when W <= H.  size * long stays below 2^26 inside the
// limits (H, W 1..kResizeMaxIn; size 1..kResizeMaxOut), so Python's correctly rounded true division cannot round a quotient with a
// fraction (at least 1 / short away from the next integer) up to that integer - that takes quotient * short near 2^53 -, and the integer division
// here is int() of Python's double.  false and a message naming the value: H, W or size outside the limits, or a longer side above kResizeMaxOut.
bool resize_output_size(int H, int W, int size, int* out_h, int* out_w, std::string& err);

// ---- Farneback's parameters and pyramid on the host (flow.hip; relax_optical_flow_ex, relax_flow_plan) -----------------------------------
// The limits of relax_optical_flow_ex (RELAX_FLOW_* of relax_hip.h) and what calcOpticalFlowFarneback derives from (H, W, pyr_scale, levels):
// OpenCV's own loop - `scale` by repeated multiplication in double, a level is dropped (and every coarser one) when a side times the scale
// falls under 32 pixels, sigma = (1 / scale - 1) / 2, smoothing kernel max(cvRound(5 sigma) | 1, 3) taps, level size cvRound(side * scale).
constexpr double kFlowMinPyrScale = 0.5, kFlowMaxPyrScale = 0.95;
constexpr int kFlowMaxLevels = 8;
constexpr double kFlowMinScale = 1.0 / 32;     // coarsest scale a call may use: 79 smoothing taps
constexpr int kFlowMaxTaps = 79;
constexpr int kFlowMinWinsize = 3, kFlowMaxWinsize = 63;
constexpr int kFlowMaxIterations = 10;
struct FlowLevel {
    int h, w, ksize;
    double scale, sigma;
};
// false and a message that names the offending value: anything outside the limits, an even winsize, flags other than 0 (the Gaussian
// window, 256, and the initial flow, 4, by name)
bool flow_check_params(double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags, std::string& err);
// the levels used below the full-size one (*n_levels, 0..levels) and lv[0 .. *n_levels], COARSEST FIRST (lv[*n_levels] is the full-size
// level: scale 1, sigma 0, 3 taps); lv must hold kFlowMaxLevels + 1 entries.  false and a message: H or W under 16, pyr_scale or levels
// outside the limits, or a coarsest used scale under kFlowMinScale.
bool flow_plan(int H, int W, double pyr_scale, int levels, int* n_levels, FlowLevel* lv, std::string& err);

// ---- the two flag bits of relax_optical_flow_flags (flow.hip: gauss_solve_any, resize_area_f32x2) ------------------------------------------
// Both are pinned to the formulas stated here (restated in tests/flow_flag_ref.py in float64), not to an OpenCV build: there is none to run.
constexpr int kFlowFlagInitial = 4, kFlowFlagGaussian = 256;      // OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_FARNEBACK_GAUSSIAN
constexpr int kFlowMaxHalfWindow = kFlowMaxWinsize / 2;           // half_taps holds winsize / 2 + 1 <= 32 floats
// The Gaussian window of FarnebackUpdateFlow_GaussianBlur, one half of it: m = winsize / 2, sigma = 0.3 m, k[0] = 1,
// k[i] = (float)exp(-i^2 / (2 sigma^2)), s = 1 / (1 + 2 sum k[1..m]) in double, k[i] = (float)(k[i] s).  half_taps[0 .. m]; all 2 m + 1 taps are
// used (the outermost is 3.9e-3 of the centre).  winsize: odd, kFlowMinWinsize .. kFlowMaxWinsize (anything else: false, nothing written).
bool flow_gauss_window(int winsize, float* half_taps);
// cv::resize(INTER_AREA)'s table for one axis, src >= dst >= 1: with S = src / dst in double, cell d covers [d S, d S + S), cw = min(S, src - d S);
// full pixels s1 = ceil(d S) .. s2 = min(floor(d S + S), src - 1) exclusive (s1 = min(s1, s2)) at 1 / cw, the left partial pixel s1 - 1 at
// (s1 - d S) / cw and the right one s2 at min(d S + S - s2, 1, cw) / cw where the overlap exceeds 1e-3 (a smaller one is DROPPED, as OpenCV does:
// such a row sums to a little under 1; it needs dst / gcd(src, dst) >= 1000).  first[d], count[d] and weights[d * flow_area_taps(src, dst) + j],
// j < count[d], source pixels first[d] + j in order.  With dst == src: a copy (one weight of exactly 1 per cell).
inline int flow_area_taps(int src, int dst) { return src / dst + 2; }
bool flow_area_table(int src, int dst, int32_t* first, int32_t* count, double* weights);
// flow_check_params' rules and wording for the six parameters; flags: any of 0, 4, 256, 260 - another bit is refused with the value named
bool flow_check_params_flags(double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags, std::string& err);

// ---- the launch schedule of a Farneback chunk (flow.hip: flow_chunk executes it) -------------------------------------------------------------
// Every route is decided here, before anything launches and before a profiler span opens; flow.hip's kernels use these constants or
// static_assert equality with them.
constexpr int kFlowWinsize = 15;                              // the literal window: the register-ring kernels (box_solve_fused, flow_iteration)
constexpr int kFlowFusedBand = 240;                           // their output columns per block (FUSE_OUT, IT_OUT)
constexpr int kFlowMaxGauss = 32, kFlowMaxGaussWide = 80;     // smoothing taps the pyramid kernels hold: the literal pyramid's | down to scale 1/32
constexpr int kFlowGhSeg = 1280, kFlowGhSegWide = 4352;       // floats of source row per block of gauss_h_sampled, and of its wide instantiation
constexpr int kFlowGaussTileH = 32, kFlowGaussTileW = 64;     // a block of gauss_solve_any (GS_TH, GS_TW)
constexpr int flow_poly_band(int poly_n) { return 256 - 2 * poly_n; }            // output columns per block of poly_expansion<N>
constexpr int flow_box_band(int winsize) { return winsize == kFlowWinsize ? kFlowFusedBand : (256 - 2 * (winsize / 2)) & ~3; }
// The workspace of a chunk: 27 floats per pixel and pair (gray, tmp, blur, I: 2 each; R 10; M 5; the two flow buffers 2 each) and 16 bytes per
// pair for the magnitude range (2 words used).  The chunk size budgets kFlowWsBytesPerPixel, which covers it from the smallest frame on.
constexpr int kFlowArenaFloatsPerPixel = 27, kFlowWsBytesPerPixel = 112;
static_assert(kFlowWsBytesPerPixel * 16 * 16 >= kFlowArenaFloatsPerPixel * 4 * 16 * 16 + 16, "the chunk budget covers the carve at 16 x 16 and above");
// pairs per chunk of a call of T pairs: what ws_gb GB hold, capped by "flow_max_pairs" (> 0) and T, at least 1
int flow_chunk_pairs(int H, int W, int64_t ws_gb, int flow_max_pairs, int T);

// What calcOpticalFlowFarneback takes besides the frames (flags: host::kFlowFlag*; 0 outside relax_optical_flow_flags)
struct FlowParams {
    double pyr_scale;
    int levels, winsize, iterations, poly_n;
    double poly_sigma;
    int flags;
};
// What the dispatch reads of the call: the pairs of the chunk, the outputs asked for, whether the caller gave a field, and the facts about
// the buffers - pair_stride % 4 == 0, both frame pointers 4-byte aligned, the arena base 16-byte aligned (flow_gray_v4, gauss3_v4)
struct FlowRequest { int H, W, P, want_image, want_flow, have_init, stride4, frames4, arena16; };
struct FlowOptions { int fused, pyramid_fused, seg_rows; };       // "flow_fused", "flow_pyramid_fused", "flow_seg_rows"
enum FlowPyramid {       // how a level's input is made
    kFlowPyrFused = 0,   // pyramid_fused: the four level inputs in one pass over the frames (three levels at pyr_scale 0.5, sides multiples of 8)
    kFlowPyrSampled,     // gauss_h_sampled + gauss_v_sampled_resize: scale < 1/2, the blur only where the resize samples
    kFlowPyrSampledWide, // their wide instantiations: more than kFlowMaxGauss taps or a row stage past kFlowGhSeg floats
    kFlowPyrGauss3V4,    // gauss3_v4: three taps, rows of whole 16-byte groups
    kFlowPyrGaussPass    // gauss_pass<false> + gauss_pass<true>
};                       // (the last two: + resize_linear_f32<1> below full size, FlowLevelPlan::resize)
enum FlowUp {            // how the coarser flow arrives
    kFlowUpZeros = 0,    // coarsest level
    kFlowUpArea,         // coarsest level, OPTFLOW_USE_INITIAL_FLOW: resize_area_f32x2 of the caller's field
    kFlowUpFusedX2,      // pyr_scale 0.5: read inside the first matrix update (x 2 is written into flow_up_value)
    kFlowUpResize        // any other pyr_scale: resize_linear_f32<2>, x (float)(1 / pyr_scale)
};
enum FlowIteration {     // one iteration
    kFlowItFused = 0,    // flow_iteration: M stays on the chip ("flow_fused", the box window of 15)
    kFlowItBoxFused,     // update_matrices_k + box_solve_fused (window 15)
    kFlowItBoxAny,       // update_matrices_k + box_solve_any (every other window)
    kFlowItGaussAny      // update_matrices_k + gauss_solve_any (OPTFLOW_FARNEBACK_GAUSSIAN, every window, 15 too)
};
enum FlowGray { kFlowGrayNone = 0, kFlowGrayV4, kFlowGray };      // none under pyramid_fused
// One iteration: the flow buffer (0 = A, 1 = B) it reads and the one it writes.  flow_iteration ping-pongs (a block reads rows its neighbours
// may already have rewritten otherwise); the two-kernel routes solve in place.  The first iteration under kFlowUpFusedX2 reads the coarser level's result.
struct FlowStep { int in, out, minmax; };     // minmax: the magnitude range rides on this launch (the last one of level 0 when an image is asked for)
struct FlowLevelPlan {
    FlowLevel lv;
    int pyramid, resize;                      // FlowPyramid; resize_linear_f32<1> follows
    int up, start;                            // FlowUp; the buffer the zeros / the resized field land in (== step[0].in except under kFlowUpFusedX2)
    int poly_n, poly_bands, poly_seg;         // poly_expansion<poly_n>: bands of flow_poly_band columns, rows per block (shorter for few pairs: the only entry P changes)
    int iteration;                            // FlowIteration
    int bands, out_cols, seg, segments;       // its grid: bands of out_cols columns x segments of seg rows (gauss_solve_any: tiles)
    int um_gx, um_rows;                       // update_matrices_k: blocks per row, rows per block of its 8 row groups
    FlowStep step[kFlowMaxIterations];
    double it_bytes;                          // algorithmic bytes of one flow_iteration / update_matrices_k launch (relax_profile_read kind 5)
    double bytes;                             // of the whole level (pyramid, pyramid step, poly_expansion, iterations)
};
struct FlowSchedule {
    int n_levels;                             // used below the full-size one; lvl[0 .. n_levels], coarsest first
    int iterations, gray, result;             // FlowGray; the buffer that holds the flow of level 0
    int64_t gray_off, tmp_off, blur_off, I_off, R_off, M_off, flow_off[2], mm_off;     // the arena in floats (mm: 2 P words)
    int64_t pyr_off[4];                       // pyramid_fused's outputs, levels 0..3: blur, I, tmp, tmp + 2 P (HW / 16)
    int64_t arena_bytes;
    double bytes;                             // the stage's algorithmic bytes (relax_profile_read kind 6): frames and gray, the levels, copy-free outputs, the image
    FlowLevelPlan lvl[kFlowMaxLevels + 1];
};
// Rows per block of the box kernels: a multiple of the window, by the level's geometry only (never the pairs of the launch: the running column
// sums restart at a segment's first row, so the segmentation fixes the last bits of the flow); seg_rows > 0 forces one (rounded up to the window)
int flow_segment_rows(int seg_rows, int bands, int h, int winsize);
// What another parameter value changes from the literal set's launches: pyr_scale / levels - the per-level pyramid kernels instead of
// pyramid_fused and resize_linear_f32<2> for the pyramid step; winsize - update_matrices_k + box_solve_any; poly_n / poly_sigma -
// poly_expansion<7>, other constants; iterations - the loop count; flags 256 - update_matrices_k + gauss_solve_any; flags 4 - kFlowUpArea.
// false and a message: flow_plan's refusals, frames past the 2 GB of a buffer resource, a smoothing kernel or row stage past the wide
// kernels, no Gaussian window for the winsize (none of the last three is reachable for parameters flow_check_params_flags accepts).
bool flow_schedule(const FlowParams& fp, const FlowRequest& rq, const FlowOptions& o, FlowSchedule* sc, std::string& err);

// ---- the options table: every relax_set_option / relax_get_option key once ------------------------------------------------------------------
// How a row takes a value: as given; != 0; a non-positive value becomes `a`; one of {a, b}; the closed range [a, b].  The last two refuse
// anything else with "relax_set_option: <key> must be <must_be>" and leave the stored value as it was.
enum OptRule { kOptAsGiven = 0, kOptBool, kOptFloor, kOptOneOf, kOptRange };
struct OptionRow {
    const char* key;
    int GemmOptions::*member;
    OptRule rule;
    int a, b;
    const char* must_be;      // the refusal's text (kOptOneOf, kOptRange)
    const char* env;          // the variable relax_create reads the initial value from, or nullptr
    int env_fallback;         // what a variable's value that the rule refuses becomes
};
extern const OptionRow kOptions[];
extern const int kNumOptions;
// false and the message of relax_set_option (NULL key, unknown key, refused value); the stored value changes only on true
bool option_set(GemmOptions& o, const char* key, int value, std::string& err);
// false and the message of relax_get_option (NULL argument, unknown key)
bool option_get(const GemmOptions& o, const char* key, int* value, std::string& err);
// the variables of the table over `o`: lookup(name) is getenv's contract (nullptr = not set); a value is read with atoi (an unparsable one
// is 0) and taken by the row's rule
void options_from_env(GemmOptions& o, const std::function<const char*(const char*)>& lookup);

// ---- VGG-16 (torchvision configuration D, no BatchNorm) -----------------------------------------------------------------------
// The 13 convolutions features.{0,2,5,7,10,12,14,17,19,21,24,26,28} (3x3, pad 1) and the two classifier layers the features read
// (classifier.0: 25088 -> 4096, classifier.3: 4096 -> 4096; classifier.6 is never run).
constexpr int kVggConvs = 13;
extern const int kVggFeatureIndex[kVggConvs];
extern const int kVggConvCout[kVggConvs];
extern const int kVggConvCin[kVggConvs];
extern const int kVggConvSide[kVggConvs];     // side of the square map a convolution reads and writes (3x3, pad 1): 224 down to 14
extern const int kVggPoolAfter[kVggConvs];    // 1: features[index + 2] is the 2x2 / stride-2 max-pool (behind conv1_2, 2_2, 3_3, 4_3, 5_3)
// Every weight / bias the VGG-16 loader reads is present with its torchvision size: true, or false and a message naming the key.
bool vgg16_check_keys(const StateDict& sd, std::string& err);
// classifier.0.weight [rows][C*HW] in torchvision's NCHW flatten order (column c*HW + p) -> the same rows in NHWC order
// (column p*C + c), so fc1 is a plain GEMM over the pool5 rows as the NHWC driver stores them.  out must hold rows * C * HW floats.
void vgg16_fc1_to_nhwc(const float* w, int rows, int C, int HW, float* out);

// The forward of one chunk of images, decided before anything launches (vgg16.hip executes it): the route of every step, the buffer every tensor
// lies in, the fp32 copies, the fused-mean group sizes and the per-image scale slots.  Host arithmetic only.
constexpr int kVggChunk = 32;     // images per pass through the network (the 224^2 x 64 maps are 12.8 MB per image in fp32)
constexpr int kVggSlots = 24;     // per-image tables {maximum, scale, 1 / scale} the arena reserves (the f16x2 schedule uses 20)
constexpr int kVggTaps = 15;      // the 13 convolutions, fc1, fc2
constexpr int kVggSteps = kVggConvs + 5 + 2;   // 13 convolutions, 5 max-pools, fc1, fc2
struct VggOptions { int precision; };          // "gemm_precision": 3 f16x2, 2 bf16x6, 0 / 1 fp32 rows into the exact-fp32 (bf16x3) kernel
// N <= kVggChunk images; bit t of taps: tap t is exported
struct VggRequest { int N, want_layer_stack, want_pool; unsigned taps; };
enum VggRoute {
    kVggConv11 = 0,    // vgg_conv1_1: the streaming kernel that reads the uint8 fragments
    kVggConvH3,        // gemm_h3, convolution form (f16x2 onto Cout % 256 == 0: conv3_x .. conv5_x and the classifier as 1x1 convolutions over 1x1 images)
    kVggConvX6H2,      // gemm_x6 on fp16 planes (f16x2 onto 64 / 128 channels)
    kVggConvX6,        // gemm_x6 on split planes (bf16x6)
    kVggConvF32,       // the exact-fp32 (bf16x3) kernel on fp32 rows
    kVggPoolH2,        // vgg_maxpool2x2 writing fp16 planes with the image's scale,
    kVggPoolSp3,       // ... split planes,
    kVggPoolF32        // ... fp32 rows
};
inline bool vgg_is_pool(int route) { return route >= kVggPoolH2; }
enum VggBuffer { kVggBufNone = 0, kVggBufA32, kVggBufPlanes0, kVggBufPlanes1, kVggBufFc1, kVggBufFc2 };
// One step, in launch order.  s_*: slots of the per-image tables, -1 = unused; a slot's scale is written by the step whose s_out it is (from the
// maximum in s_in_max, measured by an earlier step), its maximum by that step's epilogue where measure_max is set.
struct VggLayerPlan {
    int route;
    int layer;                   // the tap index of a convolution (0 .. 12) or classifier layer (13, 14); a pool: that of the convolution in front of it
    int side, cin, cout;         // the input map is side x side x cin (a classifier layer: 1 x 1 x K; a pool writes side / 2)
    int in;                      // VggBuffer the step reads (conv1_1: none, it reads the fragments)
    int out32;                   // ... its output as fp32 rows goes to: what a pool, an export, a launch_gap mean or the pool vector reads - and, under
                                 // the fp32 route, the next step (then it is a plane buffer holding rows)
    int out_planes;              // ... its output as planes of the arithmetic goes to (the next contraction's input)
    int want_mean;               // the tap's spatial mean goes into the layer stack ...
    int gap_group;               // ... finished from sums over groups of 16 / 4 rows formed in the epilogue; 0: launch_gap over the fp32 copy
    int want_export, no_split;
    int s_in, s_out, s_in_max;   // scale of the input planes; scale of the output (Hoelder's bound over the maximum in s_in_max; a pool: that maximum itself)
    int measure_max;             // the epilogue measures the per-image maximum of the output into slot s_out
};
// per-image float offsets of the arena's parts in carving order, and their total
struct VggArena { int64_t a32, planes0, planes1, groups, fc1, fc2, slots, floats; };
VggArena vgg_arena();
inline int64_t vgg_arena_bytes(int n) { return (int64_t)sizeof(float) * vgg_arena().floats * (n < kVggChunk ? n : kVggChunk); }   // the workspace of a call on n images
struct VggPlan {
    int n_slots;                 // slots of the schedule with its classifier (their numbers do not depend on the request)
    int classifier;              // 0: neither the pool vector nor fc1 / fc2 is asked for, the forward ends behind pool5
    int n_rows;                  // kVggSteps, or kVggSteps - 2 without the classifier
    VggLayerPlan row[kVggSteps];
    VggArena arena;
};
// false and a message if the schedule needs more than max_slots per-image tables
bool vgg_plan(const VggOptions& o, const VggRequest& rq, int max_slots, VggPlan* plan, std::string& err);

// ---- scales of the two-plane fp16 format (csrc/h2.h): powers of two from RIGOROUS bounds, so no value can leave the fp16 range --------
// The power of two that puts `amax` into [2^14, 2^15) (so twice the bound still fits below 65504); 1 for zero / non-finite.
float h2_scale_for_bound(double amax);
// Per-row weight scales: scale[n] = h2_scale_for_bound(max_k |W[n, k]|), W [rows][K] row-major.
void h2_weight_row_scales(const float* W, int rows, int K, float* scale);
// LayerNorm output bound: y_i = gamma_i z_i + beta_i with |z_i| <= sqrt(dim - 1) for EVERY input row (z has mean 0 and
// sum z^2 <= dim)  ->  max_i (|gamma_i| sqrt(dim - 1) + |beta_i|).
double layernorm_out_bound(const float* gamma, const float* beta, int dim);
// Bound of the outputs n in [n0, n1) of Linear(LayerNorm(x)):  |sum_i z_i gamma_i W[n,i] + (beta . W[n,:] + b[n])| <=
// sqrt(dim) * ||gamma * W[n,:]||_2 + |beta . W[n,:] + b[n]|   (Cauchy-Schwarz with ||z||_2 <= sqrt(dim)); the maximum over the range.
// Everything that is a convex combination or a contraction of such outputs (attention output: rows of V; GELU: |GELU(x)| <= |x|)
// inherits the bound.  W [N][dim] row-major, b may be null.
double linear_of_layernorm_bound(const float* W, const float* b, const float* gamma, const float* beta, int dim, int n0, int n1);

// ---- ResNet-50 under bf16x6 / f16x2: which launches a forward issues and in which form every tensor travels (resnet50.hip executes it) --------
constexpr int kRnBlocks = 16;
constexpr int kRnFirstH2Block = 7;   // layer3[0]: from here on the blocks run f16x2 under "gemm_precision" 3 (with "rn_h2")
struct RnBlockGeom {
    int block, layer, index;          // 0 .. 15 = layer<layer>.<index> of the state dict
    int cin, width, cout, stride;     // conv1 cin -> width, conv2 3x3 (stride) width -> width, conv3 width -> cout; downsample cin -> cout (stride)
    int has_down, tap;                // tap: layer-stack tap index, -1 if not tapped (layer3 blocks 4, 5)
};
const RnBlockGeom* rn_geometry();     // the kRnBlocks bottlenecks of torchvision's ResNet-50

// "This block can run form X": the loader builds the derived weights of a form where its predicate holds, the planner launches the form
// only there.  A convolution of layer1 / layer2 on the four-wave f16x2 tiles of gemm_x6.hip (64 / 128 columns: "rn_h2_early") ...
inline bool rn_early(const RnBlockGeom& k) { return k.block < kRnFirstH2Block; }
inline bool rn_early_h2(int cin, int cout) { return cin % 16 == 0 && cout % 64 == 0 && cout % 256 != 0; }
// ... its conv1 on fp32 rows split into fp16 planes in the K loop ("rn_c1_h2"; layer2: MFMA-bound on six products)
inline bool rn_can_c1_h2(const RnBlockGeom& k) { return rn_early(k) && rn_early_h2(k.cin, k.width) && k.cin >= 256 && k.width % 128 == 0; }
// ... the downsample convolution of a stride-2 first block (layer2[0]) as an f16x2 launch of its own, whose output is the fused conv3's fp32 residual
inline bool rn_can_down_launch(const RnBlockGeom& k) {
    return rn_early(k) && k.has_down && k.stride == 2 && k.cin % 16 == 0 && k.cout % 128 == 0 && k.cin >= 256;
}
// ... conv2 -> conv3 back to back ("rn_fuse": 64-wide blocks on four waves, 128-wide on eight; a 128-wide FIRST block too - layer2[0]: its
// downsample branch arrives as a residual)
inline bool rn_can_b2b(const RnBlockGeom& k) {
    return rn_early(k) && (k.width == 64 || k.width == 128) && (!k.has_down || (k.width == 128 && k.stride == 2));
}
// ... back to back with the downsample convolution in conv3's accumulator (layer1[0]: 64-wide, 64 input channels, no stride)
inline bool rn_can_b2b_x2(const RnBlockGeom& k) { return rn_early(k) && k.has_down && k.width == 64 && k.cin == 64 && k.stride == 1; }

struct RnOptions { int precision, rn_h2, rn_h2_early, rn_fuse, rn_c1_h2, fp32_rows; };   // "gemm_precision" (2 or 3), ..., "x6_fp32_rows"
// Images [0, n_ls) get layer-stack rows, images [pool_from, N) pool rows if want_pool; bit t of taps: tap t is exported
struct RnRequest { int N, n_ls, pool_from, want_pool; unsigned taps; };
// the pool vector of an image that is also in the layer stack is the last 2048 columns of its layer-stack row
inline bool rn_pool_from_stack(const RnRequest& r) { return r.want_pool && r.n_ls > 0 && r.pool_from == 0 && r.n_ls == r.N; }

enum RnForm {
    kRnFormX6 = 0,     // three bf16x6 launches (conv3 + downsample in one contraction where the block has the branch)
    kRnFormEarly,      // the same with the 3x3 on f16x2 (conv1 writes fp16 planes with the image's Hoelder scale)
    kRnFormB2B,        // conv2 -> conv3 back to back in one launch
    kRnFormB2BX2,      // ... with the downsample convolution folded into its conv3 (layer1[0])
    kRnFormB2BDown,    // ... behind a downsample launch of its own (layer2[0])
    kRnFormH2          // f16x2 with per-image scales (gemm_h2.hip: layer3 / layer4)
};
enum RnTensor { kRnNone = 0, kRnF32, kRnSp3, kRnH2 };   // fp32 rows / three bf16 planes / two fp16 planes with one scale per image
enum RnSample { kRnNoSample = 0, kRnSampleSp3, kRnSampleH2 };   // + the stride-2 sample's planes, compacted (for the next block's downsample branch)

// One bottleneck of the schedule.  s_*: slots of the per-image tables {maximum, scale, 1 / scale}, -1 = unused; a slot is written (its maximum by a
// launch's epilogue, its scale from maxima written earlier) before anything reads it.
struct RnBlockPlan {
    int form, c1_h2;
    int in_form, in_sample, out_form, out_sample;
    int need32, rows32;          // the output also as fp32 rows [0, rows32): every image, or the layer-stack images only
    int want_mean, fuse_mean;    // the tap's spatial mean of the layer-stack images; formed in conv3's epilogue (else from the fp32 copy)
    int want_export, no_split;
    int handover, pre_handover;  // the two blocks in front of the f16x2 ones: block 5 measures its output maximum (the residual term of block 6's
                                 // bound), block 6 its conv2 maximum, and its output leaves as fp16 planes with its Hoelder scale + its maximum
    int s_in_max;                // measured maximum of the block input (its producer's epilogue)
    int s_in;                    // scale of the block input's fp16 planes (kRnH2)
    int s_dr_in;                 // scale of the input's compact fp16 planes (kRnSampleH2)
    int s_c1;                    // conv1 on f16x2: scale of the fp32 input rows, from their measured maximum
    int s_t1, s_t1m;             // conv1's output: its scale from Hoelder's bound; its MEASURED maximum (what a back-to-back launch bounds planes it writes from)
    int s_t2;                    // conv2's output: scale (kRnFormH2) / measured maximum (hand-over block)
    int s_out;                   // the block output: scale (fp16 planes) and measured maximum
    int s_dr_out;                // scale of the compact fp16 planes this block leaves
};
struct RnPlan {
    int conv1_h2;                // the stem on f16x2
    int pool_f32;                // the max-pool writes fp32 rows (block 0 folds its downsample convolution in), else bf16 planes
    int s_stem;                  // the max-pool measures the maximum of its output here
    int n_slots;
    RnBlockPlan blk[kRnBlocks];
};
// The schedule of one forward: host arithmetic only.  false and a message if it needs more than max_slots per-image tables.
bool rn_plan(const RnOptions& o, const RnRequest& rq, int max_slots, RnPlan* plan, std::string& err);

// ---- ResNet-50 on any accepted canvas -------------------------------------------------------------------------------------------------------
// The model takes any input size (convolutions, one 3x3/2 max-pool, an adaptive average pool); the kernels take the canvases on which every
// stage map is even down to layer4 and the stem's output is whole 256-pixel tiles per image: Hc and Wc multiples of 32 in [64, 1024].
constexpr int kRnTaps = 15;
constexpr int kRnCanvasDefault = 224, kRnCanvasStep = 32, kRnCanvasMin = 64, kRnCanvasMax = 1024;
constexpr int kRnCanvasAny = 1;   // RELAX_RN_CANVAS_ANY: Hc and Wc any integers in [kRnCanvasMin, kRnCanvasMax] (odd maps, partial stem tiles)
// force_any: under kRnCanvasAny, run the any-size stem and max-pool also where the default rule takes the canvas (tools/resnet_anysize_bench.py times the
// two forms on one canvas with it; nothing else sets it)
struct RnCanvas { int Hc = kRnCanvasDefault, Wc = kRnCanvasDefault, flags = 0, force_any = 0; };
// Map sizes and the per-image floats of the forward's arena (resnet50.hip carves it in this order; every count is a multiple of 4).
struct RnCanvasGeometry {
    int tap_hw[kRnTaps][2];       // {h, w} of every tap: the stem's raw output, then the tapped blocks (224 x 224: 112, 56 x 3, 28 x 4, 14 x 4, 7 x 3)
    int64_t x0;                   // the preprocessed input, NHWC4 (exact-fp32 path)
    int64_t big;                  // the stem's raw output == a layer1 block output: the largest block input / output
    int64_t t1, t2;               // the largest conv1-of-block output (layer2[0] before its stride), the largest conv2 output
    int64_t gap_ws;               // spatial-mean workspace: the two-stage kernel's partial sums (16 x 2048) or the largest table of fused group sums
    int64_t block_max;            // block maxima of the max-pool (one word per 256-thread block of an image), rounded up to 64
    int64_t floats_f32, floats_x6;   // the exact-fp32 carving and the bf16x6 / f16x2 one; the arena holds the larger
};
// false and a message that names the offending value (height before width) for anything but an accepted canvas
bool rn_canvas_geometry(int Hc, int Wc, RnCanvasGeometry* g, std::string& err);
// the same under `flags`: 0 is the rule above with its messages; kRnCanvasAny takes every Hc, Wc in [64, 1024] - torch's floor rule per stage, so
// maps may be odd (then `big` is the larger of the stem's output and a layer1 block's, which the halving no longer makes equal); any other bit is
// refused by name
bool rn_canvas_geometry(int Hc, int Wc, int flags, RnCanvasGeometry* g, std::string& err);
// whether the default rule takes the canvas (Hc and Wc multiples of 32 in [64, 1024])
inline bool rn_canvas_default_rule(int Hc, int Wc) {
    return Hc >= kRnCanvasMin && Hc <= kRnCanvasMax && Hc % kRnCanvasStep == 0 && Wc >= kRnCanvasMin && Wc <= kRnCanvasMax && Wc % kRnCanvasStep == 0;
}
constexpr int kRnAvgFloats = 2048, kRnImgSlots = 64;   // per image: the avgpool vector; the per-image tables {maximum, scale, 1 / scale} of the f16x2 launches

// What a launch form asks of the MAPS of the block it runs on, restated from the kernels' own preconditions: a form is planned for a block only
// where they hold, else the block falls to the next form that does, down to plain bf16x6 (which takes any map).
// back to back (gemm_x6.hip, launch_conv_x6: "images of >= 256 pixels (a multiple of 16)")
inline bool rn_maps_b2b(int Ho, int Wo) { return Ho * Wo >= 256 && (Ho * Wo) % 16 == 0; }
// the spatial mean fused into conv3's epilogue (gemm_x6.hip / gemm_h2.hip: "the fused spatial mean needs Ho*Wo % 4 == 0")
inline bool rn_maps_fused_mean(int Ho, int Wo) { return (Ho * Wo) % 4 == 0; }
// the planes of the output's stride-2 sample (gemm_x6.hip: "the stride-2 plane output goes with ... even maps")
inline bool rn_maps_sample2(int Ho, int Wo) { return Ho % 2 == 0 && Wo % 2 == 0; }
// per-image maxima of the max-pool's Hp x Wp x C output (layers.hip: "per-image maxima need whole blocks per image": 256 threads x 4 channels)
inline bool rn_maps_pool_maxima(int Hp, int Wp, int C) { return ((int64_t)Hp * Wp * (C / 4)) % 256 == 0; }
// The schedule on an accepted canvas (the caller has run rn_canvas_geometry).  At 224 x 224 it is rn_plan's above, int for int.
bool rn_plan(const RnOptions& o, const RnRequest& rq, const RnCanvas& cv, int max_slots, RnPlan* plan, std::string& err);
// The launches in front of the blocks (RnPlan keeps its layout: these facts live here).  A canvas the default rule takes runs the forms it always
// ran, whatever the flags; the any-size forms run only on the canvases that rule refuses.
enum RnStemForm { kRnStem224 = 0, kRnStemTiles, kRnStemAny };   // conv1_x6 / conv1_x6_canvas (whole 16 x 16 tiles) / conv1_x6_any (partial tiles, rows at any alignment)
enum RnPoolForm { kRnPoolEven = 0, kRnPoolAny };                // bn_relu_maxpool_nhwc (even maps, block maxima) / bn_relu_maxpool_any (any map, a ragged last block per image)
struct RnStemPlan {
    int stem_form, pool_form;
    int stem_fused_mean;         // tap 0's 16-pixel group sums formed in the stem's epilogue (else the mean is taken from the raw output)
};
// the any-size stem fuses the mean where 16 consecutive pixels never cross a row end: output rows of whole 16-pixel groups
inline bool rn_maps_stem_fused_mean(int Ho, int Wo) { return Ho > 0 && Wo % 16 == 0; }
bool rn_stem_plan(const RnCanvas& cv, RnStemPlan* plan, std::string& err);

// ---- DINO ViT geometry (224x224 input, 64-d heads) and the streaming attention kernel's plan (vit.hip, attention_stream.hip) ----------
struct VitGeometry { int patch, side, npatch, ntok, patch_k; };   // patch 16: 14 per side, 196 patches, 197 tokens, K = 768; patch 8: 28, 784, 785, 192
// the geometry of patch size 8 or 16; anything else is refused (false and a message)
bool vit_geometry(int patch, VitGeometry* g, std::string& err);
// The patch grid of one CALL: an [Hc, Wc] canvas under patch size `patch` (8 or 16).  gh = Hc / patch, gw = Wc / patch are floors - the
// reference's stride-p convolution ignores the trailing rows and columns of pixels -, npatch = gh * gw, ntok = npatch + 1; identity: the grid is
// the loaded table's (gh == gw == side), where interpolate_pos_encoding returns pos_embed as it is.  Refused (false and a message): a patch
// size vit_geometry refuses, Hc or Wc below the patch size (the value is named), more than kVitMaxPatches patches (Hc and Wc are named).
constexpr int kVitMaxPatches = 4096;   // the one declared limit: 1024^2 px at patch 16, 512^2 at patch 8 (4097 tokens with the class token)
struct VitCanvasGeometry { int gh, gw, npatch, ntok, identity; };
bool vit_canvas_geometry(int patch, int Hc, int Wc, VitCanvasGeometry* g, std::string& err);
// One axis of interpolate_pos_encoding's bicubic resampling, side -> g positions, as torch evaluates F.interpolate(scale_factor = (g + 0.1) /
// side, mode = 'bicubic', align_corners = False) on fp32: the coordinate scale is 1 / scale_factor computed in double and rounded to fp32, the
// source coordinate scale * (dst + 0.5) - 0.5 (one fused multiply-add, as torch's builds evaluate it) and the cubic-convolution weights
// (A = -0.75) are evaluated in fp32.  Output position i reads
// source positions idx[4 i .. 4 i + 3] (floor - 1 .. floor + 2, clamped to [0, side - 1]) with weights w[4 i .. 4 i + 3].
void pos_interp_taps(int side, int g, int32_t* idx, float* w);
// The forward's arena: per-image float offsets of its slots, by role and in carving order, and their total.  Two layouts: exact fp32 (every slot
// fp32 rows; `final`, the final norm's output, is the operand slot again) and planes (bf16x6 / f16x2: the GEMM operands - patches, operand,
// hidden - take the 6 bytes per value of split planes, fp16 planes use 4 of them; `final` is a slot of its own behind qkv).
struct VitArena { int64_t patches, embedded, residual, operand, qkv, final, hidden, floats; };
VitArena vit_arena(bool planes, int dim, int ntok, int npatch, int patch_k);
// The routes of one forward (vit.hip executes them): host arithmetic only.  Every block runs the same launches, so there is no per-launch table.
enum VitArith { kVitF32 = 0, kVitX6, kVitH2 };   // exact fp32 (or bf16x3: the fp32 GEMM's own choice) / bf16x6 / f16x2
enum VitAttention { kVitAttention = 0, kVitAttentionStreamF32, kVitAttentionX6, kVitAttentionStreamX6, kVitAttentionH2, kVitAttentionStreamH2 };
struct VitOptions { int precision, att_h2, att_h2_stream; };
struct VitModel { int dim, depth, heads, patch, patch_k; };
struct VitRequest { int ntok, npatch, want_tokens, want_pooled, want_cls_attention, n_last; };   // n_last: taps after the last n blocks, 0 = none
struct VitPlan {
    int arith;            // VitArith of the forward: f16x2 under precision 3 where the tile takes the width (dim % 256 == 0), bf16x6 under 2 and above
    int patch_embed;      // VitArith of the patchify kernel and the patch-embed GEMM: `arith`, but bf16x6 for patch 8 under f16x2 (K = 192 < 256)
    int qkv_planes;       // qkv leaves its GEMM as fp16 planes, which attention and vit_cls_attention read as they are
    int attention;        // VitAttention: 197 tokens run the single-tile kernels, any other count the streaming ones
    int attention_only;   // CLS attention alone: the forward ends behind the last block's qkv GEMM
    int final_norm;       // not under taps (the last tap is the final norm) nor under attention_only
    VitArena arena;       // the layout `arith` runs in (the arena itself holds the larger one, planes: vit_arena_bytes)
};
VitPlan vit_plan(const VitOptions& o, const VitModel& m, const VitRequest& rq);

// attention_stream.hip: one workgroup = one (image, head, block of kAttStreamQBlock queries); it walks ceil(ntok / 32) key tiles, the K and V
// images of ONE tile in LDS at a time (fp32 rows under kAttStreamF32, bf16 plane images under kAttStreamX6)
constexpr int kAttStreamQBlock = 128;     // 4 waves x 32 queries
constexpr int kAttStreamKeyTile = 32;
constexpr int kAttStreamKLdF32 = 68, kAttStreamVLdF32 = 72;             // floats per K / V row of the fp32 images (conflict-free reads)
constexpr int kAttStreamKRowX6 = 4 * 96 + 16, kAttStreamVRowX6 = 2 * 96 + 16;   // bytes per key of the K image, per d of the V^T image
constexpr int kAttStreamLdsF32 = 4 * kAttStreamKeyTile * (kAttStreamKLdF32 + kAttStreamVLdF32);
constexpr int kAttStreamLdsX6 = kAttStreamKeyTile * kAttStreamKRowX6 + 64 * kAttStreamVRowX6;
constexpr int kLdsBytesPerCu = 160 * 1024;
enum AttStreamArith { kAttStreamF32 = 0, kAttStreamX6 = 1 };
struct AttStreamPlan {
    int qblock;        // queries per item
    int qblocks;       // items per (image, head): query block b covers queries [b * qblock, min(ntok, (b + 1) * qblock))
    int key_tiles;     // ceil(ntok / 32); the last one may hold padding keys (masked)
    int lds_bytes;
    int items;         // Nimg * heads * qblocks = workgroups of the launch
};
// false and a message for Nimg / heads / ntok < 1, an image whose qkv rows pass 2^31 bytes (buffer-resource range) or more than 2^31 - 1 items
bool att_stream_plan(int Nimg, int heads, int ntok, int arith, AttStreamPlan* plan, std::string& err);

// attention_stream_h2.hip (f16x2): one workgroup = one (image, head, block of kAttStreamH2QBlock queries); it walks ceil(ntok / 64) key tiles,
// the K and V rows of a tile as fp16-plane images of 256 bytes per key (attention_h2.hip's), two tiles resident (the next one lands by LDS-DMA
// under the current one's math)
constexpr int kAttStreamH2QBlock = 128;    // 4 waves x 32 queries
constexpr int kAttStreamH2KeyTile = 64;
constexpr int kAttStreamH2RowBytes = 256;  // one key of one image: 4 chunks of [16 hi][16 lo] fp16
constexpr int kAttStreamH2Lds = 2 * 2 * kAttStreamH2KeyTile * kAttStreamH2RowBytes;   // (K image + V image) x two buffers = 65536
constexpr int kAttStreamH2WgsPerCu = 2;    // what the kernel's registers (<= 256 a lane) and 2 x 64 KB of LDS allow
static_assert(kAttStreamH2Lds * kAttStreamH2WgsPerCu <= kLdsBytesPerCu, "two workgroups of the f16x2 streaming attention share a CU's LDS");
struct AttStreamH2Plan {
    int key_tile;      // keys per tile
    int qblock;        // queries per item
    int qblocks;       // items per (image, head): query block b covers queries [b * qblock, min(ntok, (b + 1) * qblock))
    int key_tiles;     // ceil(ntok / key_tile); the last one may hold padding keys (masked)
    int lds_bytes;
    int wgs_per_cu;    // resident workgroups per CU the LDS size is chosen for
    int items;         // Nimg * heads * qblocks = workgroups of the launch
};
// false and a message for Nimg / heads / ntok < 1, an image whose plane rows (ntok + one tile, 3 * dim * 4 bytes each) pass 2^31 bytes
// (buffer-resource range) or more than 2^31 - 1 items
bool att_stream_h2_plan(int Nimg, int heads, int ntok, AttStreamH2Plan* plan, std::string& err);

}  // namespace host
}  // namespace relax
