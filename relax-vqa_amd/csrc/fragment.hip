// Stage A of the ReLaX-VQA hot path on gfx950: fused residual + PxP patch score (P = 8, 16 or 32), exact top-n
// selection, fragment gather onto a target x target canvas, 50/50 merge.  Integer/byte work, HBM-bound: every input byte
// is read once by the score kernel (16-byte coalesced loads, v_sad_u8), the residual frame is never
// materialised, and the gather touches only the selected patches ((target / P)^2 slots: 196 at 16 / 224).
//
// Reference semantics (file:line in xinyiW915/ReLaX-VQA):
//   src/main_fragment_layerstack.py:302      cv2.absdiff
//   src/main_fragment_layerstack.py:177-189  get_patch_diff  (sum of bytes per patch_size x patch_size x 3 patch)
//   src/main_fragment_layerstack.py:191-210  extract_important_patches (top_n patches, raster re-tile)
//   src/main_fragment_layerstack.py:212-230  get_original_frame_patches
//   src/main_fragment_layerstack.py:242-245  merge_fragments (addWeighted .5/.5 -> round half even)
#include "relax_internal.h"

namespace relax {

// The patch size P is a template parameter of every kernel below: P = 16 (RELAX_PATCH) instantiates the code that was written for
// the one geometry, P = 8 and P = 32 change the chunk-to-patch map alone.  A patch row is 3 P bytes: 24 / 48 / 96.
constexpr int MAX_TARGET = 448;           // largest canvas side: (448 / 8)^2 = 3136 slots

// ---- patch score ------------------------------------------------------------------------------
// One workgroup per (patch row py, item t): a strip of P image rows.  A lane owns one 16-byte
// chunk column c for the P rows; lanes are consecutive chunks, so a wave reads 1 KiB
// of contiguous frame bytes per instruction and keeps 16 such loads in flight (8 at P = 8).
// Chunk-to-patch map: P = 16: patch c/3; P = 32: patch c/6; P = 8 (24-byte patch rows): chunks 3g and 3g+2 lie in patches 2g and
// 2g+1, chunk 3g+1 straddles them - its low 8 bytes go to patch 2g, its high 8 bytes to patch 2g+1.  nchunks = ceil(3 P pw / 16)
// stops at the last whole patch (W*3 is a multiple of 16 here, so the last chunk ends inside the row).  W*3 % 16 == 0 means
// W % 16 == 0, so pw is even at P = 8 and its last chunk is a whole one; the p_hi < pw guard only keeps the map safe on its own.
template <bool PAIR, int P>
__global__ __launch_bounds__(512) void patch_score_aligned(const uint8_t* __restrict__ a_base,
                                                           const uint8_t* __restrict__ b_base,
                                                           int64_t item_stride, int W, int pw, int ph, int nchunks,
                                                           uint32_t* __restrict__ scores) {
    extern __shared__ uint32_t lds_sum[];  // [pw]
    const int py = blockIdx.x;
    const int t = blockIdx.y;
    const int row_bytes = W * 3;
    for (int p = threadIdx.x; p < pw; p += blockDim.x) lds_sum[p] = 0;
    __syncthreads();
    const uint8_t* a = a_base + t * item_stride + (int64_t)py * P * row_bytes;
    const uint8_t* b = PAIR ? b_base + t * item_stride + (int64_t)py * P * row_bytes : nullptr;
    // a lane owns chunk column c for all P rows of the strip: 8 rows (16 x 16-byte loads) in flight at a time
    for (int c = threadIdx.x; c < nchunks; c += blockDim.x) {
        uint32_t s = 0, s_hi = 0;   // s_hi: the high 8 bytes of a chunk (P = 8 only)
#pragma unroll
        for (int r0 = 0; r0 < P; r0 += 8) {
            uint4 va[8], vb[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int64_t off = (int64_t)(r0 + r) * row_bytes + c * 16;
                va[r] = *reinterpret_cast<const uint4*>(a + off);
                if (PAIR) vb[r] = *reinterpret_cast<const uint4*>(b + off);
                else vb[r] = make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                s = __builtin_amdgcn_sad_u8(va[r].x, vb[r].x, s);
                s = __builtin_amdgcn_sad_u8(va[r].y, vb[r].y, s);
                if (P == 8) {
                    s_hi = __builtin_amdgcn_sad_u8(va[r].z, vb[r].z, s_hi);
                    s_hi = __builtin_amdgcn_sad_u8(va[r].w, vb[r].w, s_hi);
                } else {
                    s = __builtin_amdgcn_sad_u8(va[r].z, vb[r].z, s);
                    s = __builtin_amdgcn_sad_u8(va[r].w, vb[r].w, s);
                }
            }
        }
        // integer LDS atomics: order-independent, exact
        if (P == 8) {
            const int g = c / 3, j = c - 3 * g;           // chunk j of the 48-byte group of patches 2g, 2g+1
            const int p_lo = 2 * g + (j == 2), p_hi = 2 * g + (j != 0);
            if (p_lo == p_hi) {
                atomicAdd(&lds_sum[p_lo], s + s_hi);      // (p_lo < pw: nchunks ends at the last whole patch)
            } else {
                atomicAdd(&lds_sum[p_lo], s);
                if (p_hi < pw) atomicAdd(&lds_sum[p_hi], s_hi);
            }
        } else {
            atomicAdd(&lds_sum[c / (P * 3 / 16)], s);
        }
    }
    __syncthreads();
    uint32_t* out = scores + ((int64_t)t * ph + py) * pw;
    for (int p = threadIdx.x; p < pw; p += blockDim.x) out[p] = lds_sum[p];
}

// Any width / alignment: byte loads.  Work item = (row r, patch p): 3 P bytes.
template <bool PAIR, int P>
__global__ __launch_bounds__(256) void patch_score_generic(const uint8_t* __restrict__ a_base,
                                                           const uint8_t* __restrict__ b_base,
                                                           int64_t item_stride, int W, int pw, int ph,
                                                           uint32_t* __restrict__ scores) {
    extern __shared__ uint32_t lds_sum[];
    const int py = blockIdx.x;
    const int t = blockIdx.y;
    const int row_bytes = W * 3;
    for (int p = threadIdx.x; p < pw; p += blockDim.x) lds_sum[p] = 0;
    __syncthreads();
    const uint8_t* a = a_base + t * item_stride + (int64_t)py * P * row_bytes;
    const uint8_t* b = PAIR ? b_base + t * item_stride + (int64_t)py * P * row_bytes : nullptr;
    for (int item = threadIdx.x; item < pw * P; item += blockDim.x) {
        const int r = item / pw, p = item % pw;
        const int64_t off = (int64_t)r * row_bytes + p * (P * 3);
        uint32_t s = 0;
        for (int i = 0; i < P * 3; ++i) {
            const int x = a[off + i];
            const int y = PAIR ? (int)b[off + i] : 0;
            s += (uint32_t)(x > y ? x - y : y - x);
        }
        atomicAdd(&lds_sum[p], s);
    }
    __syncthreads();
    uint32_t* out = scores + ((int64_t)t * ph + py) * pw;
    for (int p = threadIdx.x; p < pw; p += blockDim.x) out[p] = lds_sum[p];
}

// ---- exact top-n selection ------------------------------------------------------------------------
// One workgroup per item.  Order = (score desc, flat index asc); output = the selected flat
// indices in ascending order (== the reference's re-sort by (y,x)).  Two-level 16-bit radix select
// for the n-th largest score, then an ordered compaction with a block-wide prefix sum.
constexpr int SEL_THREADS = 256;   // 4 waves per pair: the work is latency, not bandwidth (32 KB of scores per 1080p pair)
constexpr int SEL_BINS = 1024;

__device__ inline uint32_t wave_inclusive_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(v, off);
        if (lane >= off) v += u;
    }
    return v;
}

// exclusive prefix sum over the 256 threads (wave scans by lane shuffles, then the 4 wave totals through LDS)
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_tot, uint32_t* total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t incl = wave_inclusive_scan(v);
    __syncthreads();                       // wave_tot may still be read from the previous scan
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
        const uint32_t t = wave_tot[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    *total = all;
    return before + incl - v;
}

// positions: [slots, 2] per item, (-1, -1) from the selection's end to `slots` (top_n <= slots, checked by the driver).
__global__ __launch_bounds__(SEL_THREADS) void select_topn(const uint32_t* __restrict__ scores, int npatch, int pw,
                                                           int top_n, int slots, int32_t* __restrict__ positions,
                                                           int32_t* __restrict__ counts) {
    __shared__ uint32_t hist[SEL_BINS];  // 10 bits per level x 2 levels = 20-bit scores (max 32*32*3*255 = 783360 < 2^20)
    __shared__ uint32_t wave_tot[SEL_THREADS / 64];
    __shared__ uint32_t sh_digit, sh_remaining;
    const int t = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t* s = scores + (int64_t)t * npatch;
    int32_t* pos = positions + (int64_t)t * slots * 2;
    const int want = top_n < npatch ? top_n : npatch;

    // scores are < 2^20 (P <= 32: 32*32*3*255 = 783360; 16*16*3*255 = 195840); two 10-bit levels cover 2^20
    uint32_t thr = 0;        // the want-th largest score
    uint32_t need_ties = 0;  // how many entries == thr are selected (lowest indices first)
    if (want == 0) {
        thr = 0xffffffffu;        // nothing is selected (top_n = 0): no score exceeds or equals this
        need_ties = 0;            // (the digit search below never finds a bin for remaining = 0 and would leave thr undefined)
    } else if (want == npatch) {
        thr = 0;
        need_ties = 0xffffffffu;  // everything is selected
    } else {
        uint32_t remaining = (uint32_t)want;
        uint32_t prefix = 0;
        for (int level = 1; level >= 0; --level) {
            const int shift = level * 10;
            for (int b = tid; b < SEL_BINS; b += SEL_THREADS) hist[b] = 0;
            __syncthreads();
            for (int i = tid; i < npatch; i += SEL_THREADS) {
                const uint32_t v = s[i];
                if (level == 1 || (v >> 10) == prefix) atomicAdd(&hist[(v >> shift) & 1023u], 1u);
            }
            __syncthreads();
            // the digit d with  count(bins > d) < remaining <= count(bins >= d):  thread k owns the 4 bins
            // 1023-4k .. 1020-4k (descending), a block scan gives the count of everything above its bins
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = hist[1023 - 4 * tid - j];
            uint32_t tot;
            uint32_t above = block_exclusive_scan(h[0] + h[1] + h[2] + h[3], wave_tot, &tot);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (above < remaining && above + h[j] >= remaining) {   // exactly one (thread, j) satisfies this
                    sh_digit = (uint32_t)(1023 - 4 * tid - j);
                    sh_remaining = remaining - above;  // still to take from bin d (>= 1)
                }
                above += h[j];
            }
            __syncthreads();
            remaining = sh_remaining;
            if (level == 1) prefix = sh_digit;
            else thr = (prefix << 10) | sh_digit;
            __syncthreads();
        }
        need_ties = remaining;
    }

    // ordered compaction: each thread owns a contiguous run of flat indices
    const int per = (npatch + SEL_THREADS - 1) / SEL_THREADS;
    const int lo = tid * per < npatch ? tid * per : npatch;
    const int hi = lo + per < npatch ? lo + per : npatch;
    uint32_t n_gt = 0, n_eq = 0;
    for (int i = lo; i < hi; ++i) {
        const uint32_t v = s[i];
        n_gt += v > thr;
        n_eq += v == thr;
    }
    uint32_t total_eq, total_sel;
    const uint32_t eq_before = block_exclusive_scan(n_eq, wave_tot, &total_eq);
    uint32_t eq_take = 0;
    if (need_ties == 0xffffffffu) eq_take = n_eq;
    else if (eq_before < need_ties) eq_take = (need_ties - eq_before) < n_eq ? (need_ties - eq_before) : n_eq;
    const uint32_t out_before = block_exclusive_scan(n_gt + eq_take, wave_tot, &total_sel);
    uint32_t o = out_before, eq_left = eq_take;
    for (int i = lo; i < hi; ++i) {
        const uint32_t v = s[i];
        bool take = v > thr;
        if (!take && v == thr && eq_left > 0) { take = true; --eq_left; }
        if (take) {
            pos[2 * o] = i / pw;
            pos[2 * o + 1] = i % pw;
            ++o;
        }
    }
    for (int k = (int)total_sel + tid; k < slots; k += SEL_THREADS) {
        pos[2 * k] = -1;
        pos[2 * k + 1] = -1;
    }
    if (tid == 0) counts[t] = (int32_t)total_sel;
}

// ---- fragment gather --------------------------------------------------------------------------------
// (absdiff_u8x4: relax_internal.h, shared with the pair resize)

// MODE 0: copy patches of `a`; MODE 1: |b - a| patches.  One work item = one vector unit of a patch row: a 16-byte chunk at
// P = 16 / 32 (3 / 6 per row); at P = 8 source (24 x) and destination (24 k) of a patch row are only 8-byte aligned, so the unit
// is 8 bytes (3 per row).  Canvas: target x target pixels, tiles of P x P in raster order, rows of 3 target bytes.
template <int VEC> struct vec_of;
template <> struct vec_of<16> { typedef uint4 type; };
template <> struct vec_of<8> { typedef uint2 type; };

__device__ inline uint4 absdiff_vec(uint4 v, uint4 w) {
    return make_uint4(absdiff_u8x4(v.x, w.x), absdiff_u8x4(v.y, w.y), absdiff_u8x4(v.z, w.z), absdiff_u8x4(v.w, w.w));
}
__device__ inline uint2 absdiff_vec(uint2 v, uint2 w) { return make_uint2(absdiff_u8x4(v.x, w.x), absdiff_u8x4(v.y, w.y)); }

template <int MODE, bool ALIGNED, int P>
__global__ __launch_bounds__(256) void gather_fragment(const uint8_t* __restrict__ a_base,
                                                       const uint8_t* __restrict__ b_base, int64_t item_stride,
                                                       int H, int W, int target, int slots,
                                                       const int32_t* __restrict__ positions,
                                                       const int32_t* __restrict__ counts,
                                                       uint8_t* __restrict__ frag) {
    constexpr int VEC = P == 8 ? 8 : 16;
    constexpr int UPR = P * 3 / VEC;          // units per patch row: 3 / 3 / 6
    typedef typename vec_of<VEC>::type vec_t;
    const int t = blockIdx.y;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;  // (k, r, c): slots * P * UPR
    if (item >= slots * P * UPR) return;
    const int k = item / (P * UPR);
    const int rem = item % (P * UPR);
    const int r = rem / UPR, c = rem % UPR;
    const int tiles_per_row = target / P;
    uint8_t* dst = frag + (int64_t)t * target * target * 3 +
                   ((int64_t)((k / tiles_per_row) * P + r) * (target * 3)) + (k % tiles_per_row) * (P * 3) +
                   c * VEC;
    vec_t v;
    memset(&v, 0, sizeof(v));
    if (k < counts[t]) {
        const int y = positions[((int64_t)t * slots + k) * 2];
        const int x = positions[((int64_t)t * slots + k) * 2 + 1];
        // caller-supplied positions (relax_gather_patches) are not trusted: an out-of-range patch yields a zero tile
        if ((unsigned)y >= (unsigned)(H / P) || (unsigned)x >= (unsigned)(W / P)) {
            *reinterpret_cast<vec_t*>(dst) = v;
            return;
        }
        const int64_t off = t * item_stride + ((int64_t)(y * P + r) * W + (int64_t)x * P) * 3 + c * VEC;
        if (ALIGNED) {
            v = *reinterpret_cast<const vec_t*>(a_base + off);
            if (MODE == 1) v = absdiff_vec(v, *reinterpret_cast<const vec_t*>(b_base + off));
        } else {
            uint32_t words[VEC / 4] = {};
            for (int i = 0; i < VEC; ++i) {
                int x0 = a_base[off + i];
                if (MODE == 1) {
                    const int y0 = b_base[off + i];
                    x0 = x0 > y0 ? x0 - y0 : y0 - x0;
                }
                words[i >> 2] |= (uint32_t)x0 << ((i & 3) * 8);
            }
            memcpy(&v, words, sizeof(v));
        }
    }
    *reinterpret_cast<vec_t*>(dst) = v;  // canvas rows are 3 target bytes, tiles 3 P: every unit is VEC-aligned
}

// ---- merge: round-half-to-even(0.5a + 0.5b) on uint8 ------------------------------------------------
__device__ inline uint32_t merge_u8x4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const uint32_t sum = ((a >> s) & 255u) + ((b >> s) & 255u);
        const uint32_t half = sum >> 1;
        r |= (half + ((sum & 1u) & (half & 1u))) << s;
    }
    return r;
}

__global__ __launch_bounds__(256) void merge_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                    uint8_t* __restrict__ out, int64_t n, bool vec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec) {
        const int64_t n16 = n / 16;
        if (i < n16) {
            const uint4 x = reinterpret_cast<const uint4*>(a)[i];
            const uint4 y = reinterpret_cast<const uint4*>(b)[i];
            reinterpret_cast<uint4*>(out)[i] =
                make_uint4(merge_u8x4(x.x, y.x), merge_u8x4(x.y, y.y), merge_u8x4(x.z, y.z), merge_u8x4(x.w, y.w));
        }
        if (i < n - n16 * 16) {
            const int64_t j = n16 * 16 + i;
            out[j] = (uint8_t)merge_u8x4(a[j], b[j]);
        }
    } else if (i < n) {
        out[i] = (uint8_t)merge_u8x4(a[i], b[i]);
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The supported geometry (include/relax_hip.h): patch_size 8 / 16 / 32, target_size a positive multiple of it up to 448,
// top_n in [0, slots] (has_top_n = false: the gather alone has none).  Names the offending value; launches nothing.
static int check_geometry(relax_handle* h, const char* who, int patch, int target, bool has_top_n, int top_n) {
    RELAX_REQUIRE(h, patch <= 32, "%s: patch_size=%d: a score sums patch_size^2 * 3 bytes and the selection's two 10-bit radix levels "
                  "hold 2^20 (32*32*3*255 = 783360 is the largest that fits); built for 8, 16 and 32", who, patch);
    RELAX_REQUIRE(h, patch == 8 || patch == 16 || patch == 32, "%s: patch_size=%d is not built (8, 16 or 32)", who, patch);
    RELAX_REQUIRE(h, target > 0 && target % patch == 0 && target <= MAX_TARGET,
                  "%s: target_size=%d must be a positive multiple of patch_size=%d, at most %d", who, target, patch, MAX_TARGET);
    const int slots = (target / patch) * (target / patch);
    RELAX_REQUIRE(h, !has_top_n || (top_n >= 0 && top_n <= slots), "%s: top_n=%d must be in [0,%d]", who, top_n, slots);
    return RELAX_OK;
}

template <int P>
static void launch_gather(bool diff, bool al, dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, int64_t item_stride, int H,
                          int W, int target, int slots, const int32_t* positions, const int32_t* counts, uint8_t* frag) {
    if (diff) {
        if (al) hipLaunchKernelGGL((gather_fragment<1, true, P>), grid, 256, 0, s, a, b, item_stride, H, W, target, slots, positions, counts, frag);
        else hipLaunchKernelGGL((gather_fragment<1, false, P>), grid, 256, 0, s, a, b, item_stride, H, W, target, slots, positions, counts, frag);
    } else {
        if (al) hipLaunchKernelGGL((gather_fragment<0, true, P>), grid, 256, 0, s, a, b, item_stride, H, W, target, slots, positions, counts, frag);
        else hipLaunchKernelGGL((gather_fragment<0, false, P>), grid, 256, 0, s, a, b, item_stride, H, W, target, slots, positions, counts, frag);
    }
}

template <int P>
static dim3 gather_grid(int slots, int T) {
    constexpr int UPR = P == 8 ? 3 : P * 3 / 16;
    return dim3((slots * P * UPR + 255) / 256, T);
}

// shared driver for relax_fragment_pairs / relax_fragment_image at patch size P (arguments already checked)
template <int P>
static int fragment_run(relax_handle* h, bool pair, const uint8_t* a, const uint8_t* b, int64_t item_stride,
                        int T, int H, int W, int target, int top_n, int32_t* positions, int32_t* counts, uint8_t* frag_a,
                        uint8_t* frag_diff, uint32_t* scores, hipStream_t s) {
    const int slots = (target / P) * (target / P);
    const size_t frag_bytes = (size_t)target * target * 3;
    const int ph = H / P, pw = W / P;
    const int npatch = ph * pw;
    if (npatch == 0) {  // frame smaller than one patch: empty selection, zero canvases
        RELAX_HIP_CHECK(h, fill_async(counts, 0, sizeof(int32_t) * T, s));
        RELAX_HIP_CHECK(h, fill_async(positions, 0xff, sizeof(int32_t) * 2 * slots * T, s));
        if (frag_a) RELAX_HIP_CHECK(h, fill_async(frag_a, 0, frag_bytes * T, s));
        if (frag_diff) RELAX_HIP_CHECK(h, fill_async(frag_diff, 0, frag_bytes * T, s));
        return RELAX_OK;
    }
    if (!scores) {
        RELAX_TRY(ensure_buf(h, h->scratch, sizeof(uint32_t) * (size_t)npatch * T));
        scores = static_cast<uint32_t*>(h->scratch.p);
    }
    const bool al = ((W * 3) % 16 == 0) && (item_stride % 16 == 0) && aligned16(a) && (!pair || aligned16(b));
    const size_t lds = sizeof(uint32_t) * pw;
    const double bytes = (pair ? 2.0 : 1.0) * ph * P * (double)pw * (P * 3) * T + 4.0 * npatch * T;
    int span;
    RELAX_TRY(prof_begin(h, s, 1, bytes, &span));
    dim3 grid(ph, T);
    const int nchunks = (pw * P * 3 + 15) / 16;   // up to the last whole patch; the columns past it are never read
    const int passes = (nchunks + 511) / 512;
    const int ablock = (((nchunks + passes - 1) / passes + 63) / 64) * 64;  // 1080p at P = 16: 360 chunks -> 384 lanes, 1 pass
    if (pair) {
        if (al) hipLaunchKernelGGL((patch_score_aligned<true, P>), grid, ablock, lds, s, a, b, item_stride, W, pw, ph, nchunks, scores);
        else hipLaunchKernelGGL((patch_score_generic<true, P>), grid, 256, lds, s, a, b, item_stride, W, pw, ph, scores);
    } else {
        if (al) hipLaunchKernelGGL((patch_score_aligned<false, P>), grid, ablock, lds, s, a, b, item_stride, W, pw, ph, nchunks, scores);
        else hipLaunchKernelGGL((patch_score_generic<false, P>), grid, 256, lds, s, a, b, item_stride, W, pw, ph, scores);
    }
    RELAX_TRY(prof_end(h, s, span));
    hipLaunchKernelGGL(select_topn, dim3(T), SEL_THREADS, 0, s, scores, npatch, pw, top_n, slots, positions, counts);
    const dim3 ggrid = gather_grid<P>(slots, T);
    if (frag_a) launch_gather<P>(false, al, ggrid, s, a, b, item_stride, H, W, target, slots, positions, counts, frag_a);
    if (frag_diff && pair) launch_gather<P>(true, al, ggrid, s, a, b, item_stride, H, W, target, slots, positions, counts, frag_diff);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

static int fragment_common(relax_handle* h, bool pair, const uint8_t* a, const uint8_t* b, int64_t item_stride,
                           int T, int H, int W, int patch, int target, int top_n, int32_t* positions, int32_t* counts,
                           uint8_t* frag_a, uint8_t* frag_diff, uint32_t* scores, hipStream_t s) {
    RELAX_REQUIRE(h, a && (!pair || b), "fragment: NULL frame pointer");
    RELAX_REQUIRE(h, T > 0 && H > 0 && W > 0, "fragment: bad shape T=%d H=%d W=%d", T, H, W);
    RELAX_TRY(check_geometry(h, "fragment", patch, target, true, top_n));
    RELAX_REQUIRE(h, positions && counts, "fragment: positions/counts must not be NULL");
    RELAX_REQUIRE(h, item_stride >= (int64_t)H * W * 3 || T == 1, "fragment: item stride smaller than a frame");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    switch (patch) {
        case 8: return fragment_run<8>(h, pair, a, b, item_stride, T, H, W, target, top_n, positions, counts, frag_a, frag_diff, scores, s);
        case 16: return fragment_run<16>(h, pair, a, b, item_stride, T, H, W, target, top_n, positions, counts, frag_a, frag_diff, scores, s);
        default: return fragment_run<32>(h, pair, a, b, item_stride, T, H, W, target, top_n, positions, counts, frag_a, frag_diff, scores, s);
    }
}

}  // namespace relax

using namespace relax;

extern "C" {

int relax_fragment_pairs_ex(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T,
                            int H, int W, int patch_size, int target_size, int top_n, int32_t* positions, int32_t* counts,
                            uint8_t* ori_frag, uint8_t* diff_frag, uint32_t* scores, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    return fragment_common(h, true, orig, next, pair_stride, T, H, W, patch_size, target_size, top_n, positions, counts, ori_frag,
                           diff_frag, scores, static_cast<hipStream_t>(stream));
}

int relax_fragment_pairs(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T,
                         int H, int W, int top_n, int32_t* positions, int32_t* counts, uint8_t* ori_frag,
                         uint8_t* diff_frag, uint32_t* scores, relax_stream stream) {
    return relax_fragment_pairs_ex(h, orig, next, pair_stride, T, H, W, RELAX_PATCH, RELAX_TARGET, top_n, positions, counts, ori_frag,
                                   diff_frag, scores, stream);
}

int relax_fragment_image_ex(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W, int patch_size,
                            int target_size, int top_n, int32_t* positions, int32_t* counts, uint8_t* frag, uint32_t* scores,
                            relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    return fragment_common(h, false, image, nullptr, item_stride, T, H, W, patch_size, target_size, top_n, positions, counts, frag,
                           nullptr, scores, static_cast<hipStream_t>(stream));
}

int relax_fragment_image(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W, int top_n,
                         int32_t* positions, int32_t* counts, uint8_t* frag, uint32_t* scores, relax_stream stream) {
    return relax_fragment_image_ex(h, image, item_stride, T, H, W, RELAX_PATCH, RELAX_TARGET, top_n, positions, counts, frag, scores,
                                   stream);
}

int relax_gather_patches_ex(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W, int patch_size,
                            int target_size, const int32_t* positions, const int32_t* counts, uint8_t* frag, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, image && positions && counts && frag, "relax_gather_patches: NULL pointer");
    RELAX_REQUIRE(h, T > 0 && H > 0 && W > 0, "relax_gather_patches: bad shape");
    RELAX_TRY(check_geometry(h, "relax_gather_patches", patch_size, target_size, false, 0));
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool al = ((W * 3) % 16 == 0) && (item_stride % 16 == 0) && aligned16(image);
    const int slots = (target_size / patch_size) * (target_size / patch_size);
    switch (patch_size) {
        case 8: launch_gather<8>(false, al, gather_grid<8>(slots, T), s, image, image, item_stride, H, W, target_size, slots, positions, counts, frag); break;
        case 16: launch_gather<16>(false, al, gather_grid<16>(slots, T), s, image, image, item_stride, H, W, target_size, slots, positions, counts, frag); break;
        default: launch_gather<32>(false, al, gather_grid<32>(slots, T), s, image, image, item_stride, H, W, target_size, slots, positions, counts, frag); break;
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_gather_patches(relax_handle* h, const uint8_t* image, int64_t item_stride, int T, int H, int W,
                         const int32_t* positions, const int32_t* counts, uint8_t* frag, relax_stream stream) {
    return relax_gather_patches_ex(h, image, item_stride, T, H, W, RELAX_PATCH, RELAX_TARGET, positions, counts, frag, stream);
}

int relax_merge_fragments(relax_handle* h, const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n_bytes,
                          relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, a && b && out && n_bytes >= 0, "relax_merge_fragments: bad arguments");
    if (n_bytes == 0) return RELAX_OK;
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    const bool vec = aligned16(a) && aligned16(b) && aligned16(out);
    const int64_t threads = vec ? (n_bytes / 16 > 16 ? n_bytes / 16 : 16) : n_bytes;
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((threads + 255) / 256)), 256, 0, static_cast<hipStream_t>(stream), a,
                       b, out, n_bytes, vec);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // extern "C"
