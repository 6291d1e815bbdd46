// DINO ViT (patch 16 or 8, 64-d heads) feature extractor on gfx950.  The patch size and the position table's side are properties of the
// loaded checkpoint (VitW::patch / ntok / npatch / patch_k, from host::vit_geometry: the 224x224 table, 197 or 785 tokens); the canvas is a
// property of the CALL (host::vit_canvas_geometry: gh x gw patches of an [Hc, Wc] image, any token count up to 4097), its position table the
// loaded one resampled bicubically (vit_pos_interp).  197 tokens run the single-tile attention kernels, any other count the streaming ones
// (attention_stream.hip).
//
// Reference semantics (file:line in xinyiW915/ReLaX-VQA, src/extractor/visualise_vit_layer.py):
//   :466-470,339-342,492-494  input: PIL RGB, /255, no mean/std normalisation
//   :132-149  PatchEmbed conv pxp/p               -> patchify kernel + GEMM (K = 3*p*p = 768 / 192)
//   :197-219  interpolate_pos_encoding             -> vit_pos_interp (the loaded table itself on the 224x224 grid, :200-201)
//   :221-232  cls token prepend, + pos_embed       -> vit_assemble
//   :93-129   pre-LN blocks: qkv, softmax(q k^T/8) v, proj, MLP with exact-erf GELU
//   :234-239  final LayerNorm (eps 1e-6, :287-289), patch tokens x[:,1:]
//   src/main_fragment_pool.py:124-133  mean / max / population-std over the 196 tokens
#include "relax_internal.h"
#include "host_logic.h"
#include "sp3.h"
#include "h2.h"

namespace relax {

// patch geometry of a launch: lp = log2(patch), images [Hc][Wc] cut into rows of gw patches (npatch = gh * gw: pixels to the right of column
// gw * patch and below row gh * patch are never read); k = (c << 2 lp) + (py << lp) + px
struct PatchGeom { int lp, gw, npatch, patch_k, Hc, Wc; };
__device__ inline const uint8_t* patch_src(const uint8_t* frag, const PatchGeom g, int64_t n, int p, int k) {
    const int pm = (1 << g.lp) - 1;
    const int c = k >> (2 * g.lp), py = (k >> g.lp) & pm, px = k & pm;
    const int y = ((p / g.gw) << g.lp) + py, x = ((p % g.gw) << g.lp) + px;
    return frag + ((n * g.Hc + y) * g.Wc + x) * 3 + (2 - c);
}
constexpr float kLnEps = 1e-6f;
constexpr float kPatchScale = 16384.f;   // patch values are value/255 in [0, 1]: as fp16 planes of value * 2^14 (csrc/h2.h)

// uint8 BGR [N,Hc,Wc,3] -> fp32 [N*npatch, patch_k], k = (c*p + py)*p + px with c in RGB order, value/255
__global__ __launch_bounds__(256) void vit_patchify(const uint8_t* __restrict__ frag, float* __restrict__ P,
                                                    int64_t total, const PatchGeom g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % g.patch_k);
    const int64_t row = i / g.patch_k;
    const int p = (int)(row % g.npatch);
    const int64_t n = row / g.npatch;
    P[i] = (float)*patch_src(frag, g, n, p, k) / 255.0f;
}

// the same patches as split planes (bf16 hi + mid + lo of value/255, gemm_x6.hip): one thread per 8 k (8 pixels of a patch row: half a row
// at patch 16, a whole one at patch 8)
__global__ __launch_bounds__(256) void vit_patchify_sp3(const uint8_t* __restrict__ frag, char* __restrict__ P, int64_t total8, const PatchGeom g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int k = (int)(i % (g.patch_k / 8)) * 8;
    const int64_t row = i / (g.patch_k / 8);
    const int p = (int)(row % g.npatch);
    const int64_t n = row / g.npatch;
    const uint8_t* src = patch_src(frag, g, n, p, k);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)src[3 * j] / 255.0f;
    store_sp3_x8(P + row * (g.patch_k * 6), k, (sp3_f32x4){v[0], v[1], v[2], v[3]}, (sp3_f32x4){v[4], v[5], v[6], v[7]});
}

// the same patches as two fp16 planes of value/255 * scale (csrc/h2.h; the values are in [0, 1]: scale 2^14)
__global__ __launch_bounds__(256) void vit_patchify_h2(const uint8_t* __restrict__ frag, char* __restrict__ P, int64_t total8, float scale, const PatchGeom g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int k = (int)(i % (g.patch_k / 8)) * 8;
    const int64_t row = i / (g.patch_k / 8);
    const int p = (int)(row % g.npatch);
    const int64_t n = row / g.npatch;
    const uint8_t* src = patch_src(frag, g, n, p, k);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)src[3 * j] / 255.0f;
    store_h2_x8(P + row * (g.patch_k * 4), k, (h2_f32x4){v[0], v[1], v[2], v[3]}, (h2_f32x4){v[4], v[5], v[6], v[7]}, scale);
}

// X[n,0,:] = cls + pos[0];  X[n,1+p,:] = PE[n*npatch+p,:] + pos[1+p]     (ntok = npatch + 1)
__global__ __launch_bounds__(256) void vit_assemble(const float* __restrict__ PE, const float* __restrict__ cls,
                                                    const float* __restrict__ pos, float* __restrict__ X, int dim4,
                                                    int64_t total, int ntok) {
    const int NTOK = ntok, NPATCH = ntok - 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = (int)(i % dim4);
    const int64_t row = i / dim4;
    const int tok = (int)(row % NTOK);
    const int64_t n = row / NTOK;
    const float4 pp = reinterpret_cast<const float4*>(pos)[(int64_t)tok * dim4 + d];
    const float4 v = tok == 0 ? reinterpret_cast<const float4*>(cls)[d]
                              : reinterpret_cast<const float4*>(PE)[(n * NPATCH + (tok - 1)) * dim4 + d];
    reinterpret_cast<float4*>(X)[i] = make_float4(v.x + pp.x, v.y + pp.y, v.z + pp.z, v.w + pp.w);
}

// interpolate_pos_encoding for a gh x gw grid: out[0] = pos[0]; out[1 + oy*gw + ox] = sum_a wy[4 oy + a] * (sum_b wx[4 ox + b] *
// pos[1 + iy[4 oy + a] * side + ix[4 ox + b]]) - across x first, then across y, each sum in tap order: the order of torch's bicubic kernel.
// taps: [iy 4 gh | ix 4 gw] int32 and [wy 4 gh | wx 4 gw] fp32 from host::pos_interp_taps (indices clamped to [0, side - 1] there).
// One thread per 4 channels of an output row (16-byte loads along dim).
__global__ __launch_bounds__(256) void vit_pos_interp(const float* __restrict__ pos, const int32_t* __restrict__ tap_idx,
                                                      const float* __restrict__ tap_w, float* __restrict__ out, int dim4, int side,
                                                      int gh, int gw, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = (int)(i % dim4);
    const int row = (int)(i / dim4);
    const float4* P = reinterpret_cast<const float4*>(pos);
    if (row == 0) {
        reinterpret_cast<float4*>(out)[i] = P[d];
        return;
    }
    const int oy = (row - 1) / gw, ox = (row - 1) % gw;
    const int32_t *iy = tap_idx + 4 * oy, *ix = tap_idx + 4 * gh + 4 * ox;
    const float *wy = tap_w + 4 * oy, *wx = tap_w + 4 * gh + 4 * ox;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float4* line = P + ((int64_t)1 + (int64_t)iy[a] * side) * dim4 + d;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float4 v = line[(int64_t)ix[b] * dim4];
            const float w = wx[b];
            r = b == 0 ? make_float4(v.x * w, v.y * w, v.z * w, v.w * w) : make_float4(r.x + v.x * w, r.y + v.y * w, r.z + v.z * w, r.w + v.w * w);
        }
        const float w = wy[a];
        acc = a == 0 ? make_float4(r.x * w, r.y * w, r.z * w, r.w * w) : make_float4(acc.x + r.x * w, acc.y + r.y * w, acc.z + r.z * w, acc.w + r.w * w);
    }
    reinterpret_cast<float4*>(out)[i] = acc;
}

// Y [N,ntok,dim] -> tokens [N,ntok-1,dim] (drop cls)
__global__ __launch_bounds__(256) void vit_drop_cls(const float* __restrict__ Y, float* __restrict__ T, int dim4,
                                                    int64_t total, int ntok) {
    const int NTOK = ntok, NPATCH = ntok - 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = (int)(i % dim4);
    const int64_t row = i / dim4;
    const int p = (int)(row % NPATCH);
    const int64_t n = row / NPATCH;
    reinterpret_cast<float4*>(T)[i] = reinterpret_cast<const float4*>(Y)[(n * NTOK + 1 + p) * dim4 + d];
}

// per (image, channel): mean, max, population std over tokens first .. first+count-1 (the forward: the patch tokens 1 .. npatch) -> out[n, 0:dim | dim:2dim | 2dim:3dim]
__global__ __launch_bounds__(256) void vit_token_stats(const float* __restrict__ Y, float* __restrict__ out, int dim,
                                                       int tok_per_img, int first, int count) {
    __shared__ float red[4][64];
    __shared__ float s_mean[64];
    const int n = blockIdx.y;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int grp = threadIdx.x >> 6;  // 4 groups stride the tokens
    const float* yb = Y + ((int64_t)n * tok_per_img + first) * dim + c;
    float s = 0.f, m = -INFINITY;
    for (int p = grp; p < count; p += 4) {
        const float v = yb[(int64_t)p * dim];
        s += v;
        m = fmaxf(m, v);
    }
    red[grp][threadIdx.x & 63] = s;
    __syncthreads();
    if (grp == 0) s_mean[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x])) / (float)count;
    __syncthreads();
    const float mean = s_mean[threadIdx.x & 63];
    __syncthreads();
    red[grp][threadIdx.x & 63] = m;
    __syncthreads();
    float mx = 0.f;
    if (grp == 0) mx = fmaxf(fmaxf(red[0][threadIdx.x], red[1][threadIdx.x]), fmaxf(red[2][threadIdx.x], red[3][threadIdx.x]));
    __syncthreads();
    float q = 0.f;
    for (int p = grp; p < count; p += 4) {
        const float dv = yb[(int64_t)p * dim] - mean;
        q += dv * dv;
    }
    red[grp][threadIdx.x & 63] = q;
    __syncthreads();
    if (grp == 0) {
        const float var = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x])) / (float)count;
        float* o = out + (int64_t)n * 3 * dim;
        o[c] = mean;
        o[dim + c] = mx;
        o[2 * dim + c] = sqrtf(var);
    }
}

void free_vit(relax_handle* h) {
    for (VitPosTable& t : h->vit.pos_cache)
        if (t.table) (void)hipFree(t.table);
    h->vit.mem.release();
    h->vit = VitW();
}

size_t vit_arena_bytes(const VitW& v, int n, int ntok, int npatch) {
    const int64_t a = host::vit_arena(false, v.dim, ntok, npatch, v.patch_k).floats, b = host::vit_arena(true, v.dim, ntok, npatch, v.patch_k).floats;
    return sizeof(float) * (size_t)(a > b ? a : b) * (size_t)n;
}
size_t vit_arena_bytes(const VitW& v, int n) { return vit_arena_bytes(v, n, v.ntok, v.npatch); }

// The position table of a gh x gw grid (g from host::vit_canvas_geometry): the loaded table on the identity grid, else the cached table of
// the grid, built on a miss (taps on the host, vit_pos_interp on `s`, then a wait for `s`: a cached table is complete, whatever stream reads
// it next; the least recently used of the kVitPosCache entries is replaced).
static int vit_pos_table(relax_handle* h, const host::VitCanvasGeometry& g, hipStream_t s, const float** out) {
    VitW& v = h->vit;
    if (g.identity) {
        *out = v.pos;
        return RELAX_OK;
    }
    VitPosTable* slot = &v.pos_cache[0];
    for (VitPosTable& t : v.pos_cache) {
        if (t.table && t.gh == g.gh && t.gw == g.gw) {
            t.used = ++v.pos_clock;
            *out = t.table;
            return RELAX_OK;
        }
        if (t.used < slot->used) slot = &t;
    }
    const int side = 224 / v.patch, ntaps = 4 * (g.gh + g.gw);
    std::vector<int32_t> idx((size_t)ntaps);
    std::vector<float> w((size_t)ntaps);
    host::pos_interp_taps(side, g.gh, idx.data(), w.data());
    host::pos_interp_taps(side, g.gw, idx.data() + 4 * g.gh, w.data() + 4 * g.gh);
    if (slot->table) {   // (hipFree waits for the device: no launch still reads the table that goes)
        RELAX_HIP_CHECK(h, hipFree(slot->table));
        *slot = VitPosTable();
    }
    // [table (1 + gh*gw) * dim floats | tap indices | tap weights] in one allocation
    const size_t table_floats = (size_t)g.ntok * v.dim;
    float* mem = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&mem), sizeof(float) * (table_floats + 2 * (size_t)ntaps));
    if (e != hipSuccess) {
        set_error(h, "hipMalloc of the %d x %d position table (%zu floats) failed: %s", g.gh, g.gw, table_floats, hipGetErrorString(e));
        return RELAX_ERR_NOMEM;
    }
    int32_t* d_idx = reinterpret_cast<int32_t*>(mem + table_floats);
    float* d_w = mem + table_floats + ntaps;
    const int64_t total = (int64_t)g.ntok * (v.dim / 4);
    hipError_t rc = hipMemcpyAsync(d_idx, idx.data(), sizeof(int32_t) * (size_t)ntaps, hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) rc = hipMemcpyAsync(d_w, w.data(), sizeof(float) * (size_t)ntaps, hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) {
        hipLaunchKernelGGL(vit_pos_interp, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, v.pos, d_idx, d_w, mem, v.dim / 4, side, g.gh,
                           g.gw, total);
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipStreamSynchronize(s);   // (the host tap arrays live until here)
    if (rc != hipSuccess) {
        (void)hipFree(mem);
        set_error(h, "vit_pos_interp (%d x %d) failed: %s", g.gh, g.gw, hipGetErrorString(rc));
        return RELAX_ERR_HIP;
    }
    slot->gh = g.gh; slot->gw = g.gw; slot->table = mem; slot->used = ++v.pos_clock;
    *out = mem;
    return RELAX_OK;
}

// everything relax_load_vit_ex puts on the device; the caller frees it all if this fails
static int load_vit(relax_handle* h, const host::StateDict& sd, const host::VitGeometry& geo, int dim, int depth, int heads) {
    VitW& v = h->vit;
    auto host_of = [&](const std::string& key, int64_t numel) -> const float* {
        std::string err;
        const float* src = sd.get(key, numel, err, "vit state dict");
        if (!src) set_error(h, "%s", err.c_str());
        return src;
    };
    auto up = [&](const std::string& key, int64_t numel, float** dst) -> int {
        const float* src = host_of(key, numel);
        return src ? v.mem.upload(h, src, (size_t)numel, dst) : RELAX_ERR_INVALID;
    };
    auto lin = [&](const std::string& p, int in, int out, LinearW* l) -> int {
        l->in = in;
        l->out = out;
        RELAX_TRY(up(p + ".weight", (int64_t)in * out, &l->w));
        return up(p + ".bias", out, &l->b);
    };
    v.dim = dim; v.depth = depth; v.heads = heads;
    v.patch = geo.patch; v.ntok = geo.ntok; v.npatch = geo.npatch; v.patch_k = geo.patch_k;
    RELAX_TRY(up("cls_token", dim, &v.cls));
    RELAX_TRY(up("pos_embed", (int64_t)geo.ntok * dim, &v.pos));
    RELAX_TRY(lin("patch_embed.proj", geo.patch_k, dim, &v.patch_w));  // OIHW [dim][3][p][p] is already [dim][(c*p+py)*p+px]
    v.blocks.resize(depth);
    for (int i = 0; i < depth; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        VitBlockW& b = v.blocks[i];
        RELAX_TRY(up(p + "norm1.weight", dim, &b.ln1_g));
        RELAX_TRY(up(p + "norm1.bias", dim, &b.ln1_b));
        RELAX_TRY(lin(p + "attn.qkv", dim, 3 * dim, &b.qkv));
        RELAX_TRY(lin(p + "attn.proj", dim, dim, &b.proj));
        RELAX_TRY(up(p + "norm2.weight", dim, &b.ln2_g));
        RELAX_TRY(up(p + "norm2.bias", dim, &b.ln2_b));
        RELAX_TRY(lin(p + "mlp.fc1", dim, 4 * dim, &b.fc1));
        RELAX_TRY(lin(p + "mlp.fc2", 4 * dim, dim, &b.fc2));
    }
    RELAX_TRY(up("norm.weight", dim, &v.norm_g));
    RELAX_TRY(up("norm.bias", dim, &v.norm_b));
    // split planes of every GEMM weight for the bf16x6 kernel (made on the device from the uploaded fp32 copy)
    auto sp3 = [&](LinearW* l) { return derive_sp3(h, v.mem, l->w, l->out, l->in, &l->w_sp3, "vit split-plane weights"); };
    RELAX_TRY(sp3(&v.patch_w));
    for (VitBlockW& b : v.blocks) {
        RELAX_TRY(sp3(&b.qkv));
        RELAX_TRY(sp3(&b.proj));
        RELAX_TRY(sp3(&b.fc1));
        RELAX_TRY(sp3(&b.fc2));
    }
    // two fp16 planes of every GEMM weight for the f16x2 kernel: row n scaled by 2^t_n (from the row's maximum); colscale[n] =
    // 2^-t_n / (the static scale of the activation tensor the layer reads).  The activation scales come from bounds that hold for
    // EVERY input (host_logic.h), evaluated here in double on the host copies of the weights (present: `up` has checked every key).
    std::vector<float> tmp_scale, tmp_col;
    auto h2w = [&](LinearW* l, const std::string& p, float act_scale) -> int {
        const float* hw = host_of(p + ".weight", (int64_t)l->in * l->out);
        tmp_scale.resize((size_t)l->out);
        tmp_col.resize((size_t)l->out);
        host::h2_weight_row_scales(hw, l->out, l->in, tmp_scale.data());
        for (int n = 0; n < l->out; ++n) tmp_col[(size_t)n] = (1.f / tmp_scale[(size_t)n]) * (1.f / act_scale);   // powers of two: exact
        float* d_scale = nullptr;
        l->w_h2 = v.mem.keep(h, (size_t)l->in * l->out * 4, "vit fp16-plane weights");
        if (!l->w_h2) return RELAX_ERR_NOMEM;
        RELAX_TRY(v.mem.upload(h, tmp_scale.data(), (size_t)l->out, &d_scale));
        RELAX_TRY(v.mem.upload(h, tmp_col.data(), (size_t)l->out, &l->colscale));
        return launch_to_h2(h, l->w, l->in, l->w_h2, l->out, l->in, 1.f, d_scale, nullptr);
    };
    if (dim % 256 == 0) {   // (the f16x2 tile takes N % 256 == 0: ViT-B; smaller models run bf16x6 under "gemm_precision" 3)
        // (patch 8: the patch-embed GEMM runs on bf16x6 under f16x2 too - host::vit_plan's patch_embed - and needs no fp16 planes)
        if (geo.patch == 16) RELAX_TRY(h2w(&v.patch_w, "patch_embed.proj", kPatchScale));
        for (int i = 0; i < depth; ++i) {
            const std::string p = "blocks." + std::to_string(i) + ".";
            VitBlockW& b = v.blocks[i];
            const float *g1 = host_of(p + "norm1.weight", dim), *b1 = host_of(p + "norm1.bias", dim);
            const float *g2 = host_of(p + "norm2.weight", dim), *b2 = host_of(p + "norm2.bias", dim);
            b.s_ln1 = host::h2_scale_for_bound(host::layernorm_out_bound(g1, b1, dim));
            b.s_ln2 = host::h2_scale_for_bound(host::layernorm_out_bound(g2, b2, dim));
            // attention output = convex combinations of the V rows of qkv(LayerNorm1(x)): columns 2 dim .. 3 dim of the qkv Linear
            b.s_att = host::h2_scale_for_bound(host::linear_of_layernorm_bound(host_of(p + "attn.qkv.weight", (int64_t)3 * dim * dim),
                                                                               host_of(p + "attn.qkv.bias", 3 * dim), g1, b1, dim, 2 * dim, 3 * dim));
            b.s_qkv = host::h2_scale_for_bound(host::linear_of_layernorm_bound(host_of(p + "attn.qkv.weight", (int64_t)3 * dim * dim),
                                                                               host_of(p + "attn.qkv.bias", 3 * dim), g1, b1, dim, 0, 3 * dim));
            // |GELU(x)| <= |x|, x = fc1(LayerNorm2(.))
            b.s_hid = host::h2_scale_for_bound(host::linear_of_layernorm_bound(host_of(p + "mlp.fc1.weight", (int64_t)4 * dim * dim),
                                                                               host_of(p + "mlp.fc1.bias", 4 * dim), g2, b2, dim, 0, 4 * dim));
            RELAX_TRY(h2w(&b.qkv, p + "attn.qkv", b.s_ln1));
            RELAX_TRY(h2w(&b.proj, p + "attn.proj", b.s_att));
            RELAX_TRY(h2w(&b.fc1, p + "mlp.fc1", b.s_ln2));
            RELAX_TRY(h2w(&b.fc2, p + "mlp.fc2", b.s_hid));
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) {
        set_error(h, "vit: weight conversion failed");
        return RELAX_ERR_HIP;
    }
    return RELAX_OK;
}

}  // namespace relax

using namespace relax;

extern "C" {

int relax_load_vit(relax_handle* h, const float* const* tensors, const char* const* names, const int64_t* numels,
                   int n, int dim, int depth, int heads) {
    return relax_load_vit_ex(h, tensors, names, numels, n, dim, depth, heads, 16);
}

int relax_load_vit_ex(relax_handle* h, const float* const* tensors, const char* const* names, const int64_t* numels,
                      int n, int dim, int depth, int heads, int patch_size) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, tensors && names && numels && n > 0, "relax_load_vit: bad arguments");
    RELAX_REQUIRE(h, heads > 0 && dim == heads * 64, "relax_load_vit: dim=%d must be heads*64 (heads=%d)", dim, heads);
    RELAX_REQUIRE(h, dim <= 768 && depth > 0, "relax_load_vit: dim=%d depth=%d unsupported", dim, depth);
    host::VitGeometry geo;
    {
        std::string err;
        RELAX_REQUIRE(h, host::vit_geometry(patch_size, &geo, err), "relax_load_vit: %s", err.c_str());
    }
    host::StateDict sd;
    for (int i = 0; i < n; ++i) sd.add(names[i], tensors[i], numels[i]);
    // the two tensors that carry the geometry, checked before anything is freed or uploaded: a checkpoint of the other patch size is
    // refused with both counts in the message
    const int64_t n_pos = sd.numel("pos_embed"), n_pw = sd.numel("patch_embed.proj.weight");
    RELAX_REQUIRE(h, n_pos < 0 || n_pos == (int64_t)geo.ntok * dim,
                  "vit state dict: pos_embed has %lld values = %lld tokens of dim %d, patch size %d needs %d tokens", (long long)n_pos,
                  (long long)(n_pos / dim), dim, geo.patch, geo.ntok);
    RELAX_REQUIRE(h, n_pw < 0 || n_pw == (int64_t)dim * geo.patch_k,
                  "vit state dict: patch_embed.proj.weight has %lld values = %lld per output channel of %d, patch size %d needs %d (3 x %d x %d)",
                  (long long)n_pw, (long long)(n_pw / dim), dim, geo.patch, geo.patch_k, geo.patch, geo.patch);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    free_vit(h);
    const int rc = load_vit(h, sd, geo, dim, depth, heads);
    if (rc == RELAX_OK) h->vit.loaded = true;
    else free_vit(h);   // a failed load leaves nothing behind
    return rc;
}

}  // extern "C"

// frags: N images [Hc][Wc][3].  Hc = Wc = 224 is the loaded geometry: v.pos, the arena relax_reserve sized, the launches of always.
// `what`: the entry point that was called, for the messages.
// taps (relax_vit_intermediate_layers; NULL from every other entry point, whose launches are then the ones of always): after each of the
// last n_last blocks the final norm of the residual stream - the whole normed rows into tokens[k] (launch_layernorm straight into the caller's
// [n, N, ntok, dim]), the normed CLS row and the patch-token statistics into cls[k] / pooled[k] (vit_norm_token_stats, csrc/vit_layers.hip) -,
// k = 0 for block depth - n_last.  The last tap IS the forward's final norm, which is then not launched again.
struct VitTaps { int n_last; float *tokens, *cls, *pooled; };
static int vit_tap(relax_handle* h, const VitTaps& t, int block, const float* X, int N, int ntok, hipStream_t s) {
    const VitW& v = h->vit;
    const int k = block - (v.depth - t.n_last);
    if (k < 0) return RELAX_OK;
    const size_t dim = (size_t)v.dim, per_tap = (size_t)N * dim;
    if (t.tokens) RELAX_TRY(launch_layernorm(h, X, v.norm_g, v.norm_b, t.tokens + (size_t)k * per_tap * ntok, N * ntok, v.dim, kLnEps, s));
    if (t.cls || t.pooled)
        RELAX_TRY(launch_vit_norm_token_stats(h, X, v.norm_g, v.norm_b, kLnEps, t.cls ? t.cls + (size_t)k * per_tap : nullptr,
                                              t.pooled ? t.pooled + (size_t)k * per_tap * 3 : nullptr, N, ntok, v.dim, s));
    return RELAX_OK;
}

static int vit_forward(relax_handle* h, const char* what, const uint8_t* frags, int N, int Hc, int Wc, float* tokens, float* pooled,
                       float* cls_attention, relax_stream stream, const VitTaps* taps = nullptr) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->vit.loaded, "%s: call relax_load_vit first", what);
    RELAX_REQUIRE(h, frags && N > 0, "%s: bad arguments", what);
    host::VitCanvasGeometry cg;
    {
        std::string err;
        RELAX_REQUIRE(h, host::vit_canvas_geometry(h->vit.patch, Hc, Wc, &cg, err), "%s: %s", what, err.c_str());
    }
    RELAX_REQUIRE(h, (int64_t)N * cg.ntok <= (int64_t)INT32_MAX, "%s: %d images of %d tokens pass 2^31 - 1 rows", what, N, cg.ntok);
    const VitW& v = h->vit;
    const int dim = v.dim, NTOK = cg.ntok, NPATCH = cg.npatch, PATCH_K = v.patch_k, rows = N * NTOK;
    // which arithmetic, which kernels, where the forward ends and where its buffers lie: host::vit_plan; below, the one sequence that runs it
    const host::VitPlan pl = host::vit_plan({h->gemm.precision, h->gemm.att_h2, h->gemm.att_h2_stream}, {dim, v.depth, v.heads, v.patch, PATCH_K},
                                            {NTOK, NPATCH, tokens != nullptr, pooled != nullptr, cls_attention != nullptr, taps ? taps->n_last : 0});
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* pos = nullptr;
    RELAX_TRY(vit_pos_table(h, cg, s, &pos));
    RELAX_TRY(ensure_buf(h, h->arena, vit_arena_bytes(v, N, NTOK, NPATCH)));
    // GEMM inputs (P, Y, Hid) travel in the arithmetic's operand form, written by the kernel that produces them: fp32 rows, bf16 split planes, or
    // two fp16 planes of (value x a static power of two).  GEMM outputs that feed LayerNorm / attention / the residual stream X stay fp32.
    auto slot = [&](int64_t floats_per_image) { return static_cast<float*>(h->arena.p) + (size_t)floats_per_image * (size_t)N; };
    float *P = slot(pl.arena.patches), *PE = slot(pl.arena.embedded), *X = slot(pl.arena.residual), *Y = slot(pl.arena.operand);
    float *QKV = slot(pl.arena.qkv), *Final = slot(pl.arena.final), *Hid = slot(pl.arena.hidden);

    // out = act(A W^T + bias) (+ residual) as fp32 rows into out_f32, or as the next GEMM's operand into out_operand (f16x2: of value x out_scale)
    auto linear = [&](int arith, const float* A, const LinearW& l, const float* residual, float* out_f32, float* out_operand, float out_scale, int M, int act) {
        switch (arith) {
            case host::kVitF32: return launch_gemm(h, A, l.w, l.b, residual, out_f32 ? out_f32 : out_operand, M, l.out, l.in, act, s);
            case host::kVitX6: return launch_gemm_x6(h, A, l.w_sp3, l.b, residual, out_f32, out_operand, M, l.out, l.in, act, s);
        }
        GemmDescH2 d{};
        d.a = A; d.w = l.w_h2; d.colscale = l.colscale; d.bias = l.b; d.residual = residual; d.out = out_f32; d.out_h2 = out_operand;
        d.out_scale = out_scale; d.M = M; d.N = l.out; d.K = l.in; d.act = act;
        return launch_gemm_h2(h, d, s);
    };
    auto patchify_embed = [&]() {
        const int64_t total = (int64_t)N * NPATCH * PATCH_K, p8 = total / 8;
        const PatchGeom pg{v.patch == 8 ? 3 : 4, cg.gw, NPATCH, PATCH_K, Hc, Wc};
        char* Pc = reinterpret_cast<char*>(P);
        switch (pl.patch_embed) {
            case host::kVitF32: hipLaunchKernelGGL(vit_patchify, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frags, P, total, pg); break;
            case host::kVitX6: hipLaunchKernelGGL(vit_patchify_sp3, dim3((unsigned)((p8 + 255) / 256)), dim3(256), 0, s, frags, Pc, p8, pg); break;
            default: hipLaunchKernelGGL(vit_patchify_h2, dim3((unsigned)((p8 + 255) / 256)), dim3(256), 0, s, frags, Pc, p8, kPatchScale, pg);
        }
        return linear(pl.patch_embed, P, v.patch_w, nullptr, PE, nullptr, 0.f, N * NPATCH, 0);
    };
    auto norm_to_operand = [&](const float* g, const float* b, float scale) {
        switch (pl.arith) {
            case host::kVitF32: return launch_layernorm(h, X, g, b, Y, rows, dim, kLnEps, s);
            case host::kVitX6: return launch_layernorm_sp3(h, X, g, b, Y, rows, dim, kLnEps, s);
        }
        return launch_layernorm_h2(h, X, g, b, Y, scale, rows, dim, kLnEps, s);
    };
    // QKV -> Y in the operand form.  The bf16x6 kernels serve f16x2 too when qkv is fp32 rows: they write fp16 planes of value x s_att then
    auto attention = [&](const VitBlockW& b) {
        const float x6_h2_scale = pl.arith == host::kVitH2 ? b.s_att : 0.f;
        switch (pl.attention) {
            case host::kVitAttention: return launch_attention(h, QKV, Y, N, v.heads, s);
            case host::kVitAttentionStreamF32: return launch_attention_stream_f32(h, QKV, Y, N, NTOK, v.heads, s);
            case host::kVitAttentionX6: return launch_attention_x6(h, QKV, nullptr, Y, N, v.heads, s, x6_h2_scale);
            case host::kVitAttentionStreamX6: return launch_attention_stream_x6(h, QKV, nullptr, Y, N, NTOK, v.heads, s, x6_h2_scale);
            case host::kVitAttentionH2: return launch_attention_h2(h, QKV, b.s_qkv, Y, b.s_att, N, v.heads, s);
        }
        return launch_attention_stream_h2(h, QKV, b.s_qkv, Y, b.s_att, N, NTOK, v.heads, s);
    };

    RELAX_TRY(patchify_embed());
    const int64_t at = (int64_t)rows * (dim / 4);
    hipLaunchKernelGGL(vit_assemble, dim3((unsigned)((at + 255) / 256)), dim3(256), 0, s, PE, v.cls, pos, X, dim / 4, at, NTOK);
    RELAX_HIP_CHECK(h, hipGetLastError());
    // cls_attention: block `last`'s CLS row, launched right after its qkv GEMM (before its attention core, so nothing later in the
    // forward can overwrite the qkv buffer first).  Without tokens / pooled the forward stops there (get_last_selfattention).
    const int last = v.depth - 1;
    for (int i = 0; i < v.depth; ++i) {
        const VitBlockW& b = v.blocks[i];
        const float s_qkv = pl.qkv_planes ? b.s_qkv : 0.f;
        RELAX_TRY(norm_to_operand(b.ln1_g, b.ln1_b, b.s_ln1));
        RELAX_TRY(linear(pl.arith, Y, b.qkv, nullptr, pl.qkv_planes ? nullptr : QKV, pl.qkv_planes ? QKV : nullptr, s_qkv, rows, 0));
        if (cls_attention && i == last) RELAX_TRY(launch_vit_cls_attention(h, QKV, pl.qkv_planes, s_qkv, cls_attention, N, NTOK, v.heads, s));
        if (pl.attention_only && i == last) return RELAX_OK;
        RELAX_TRY(attention(b));
        RELAX_TRY(linear(pl.arith, Y, b.proj, X, X, nullptr, 0.f, rows, 0));         // x += proj(attn)
        RELAX_TRY(norm_to_operand(b.ln2_g, b.ln2_b, b.s_ln2));
        RELAX_TRY(linear(pl.arith, Y, b.fc1, nullptr, nullptr, Hid, b.s_hid, rows, 2));   // GELU(erf) -> operand form
        RELAX_TRY(linear(pl.arith, Hid, b.fc2, X, X, nullptr, 0.f, rows, 0));        // x += mlp
        if (taps) RELAX_TRY(vit_tap(h, *taps, i, X, N, NTOK, s));
    }
    if (!pl.final_norm) return RELAX_OK;
    RELAX_TRY(launch_layernorm(h, X, v.norm_g, v.norm_b, Final, rows, dim, kLnEps, s));
    if (tokens) {
        const int64_t t = (int64_t)N * NPATCH * (dim / 4);
        hipLaunchKernelGGL(vit_drop_cls, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, Final, tokens, dim / 4, t, NTOK);
    }
    if (pooled) hipLaunchKernelGGL(vit_token_stats, dim3(dim / 64, N), dim3(256), 0, s, Final, pooled, dim, NTOK, 1, NPATCH);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

extern "C" {

int relax_vit_features(relax_handle* h, const uint8_t* frags, int N, float* tokens, float* pooled,
                       relax_stream stream) {
    return vit_forward(h, "relax_vit_features", frags, N, 224, 224, tokens, pooled, nullptr, stream);
}

int relax_vit_features_ex(relax_handle* h, const uint8_t* frags, int N, float* tokens, float* pooled, float* cls_attention,
                          relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, tokens || pooled || cls_attention, "relax_vit_features_ex: no output requested");
    return vit_forward(h, "relax_vit_features", frags, N, 224, 224, tokens, pooled, cls_attention, stream);
}

int relax_vit_features_canvas(relax_handle* h, const uint8_t* images, int N, int Hc, int Wc, float* tokens, float* pooled,
                              float* cls_attention, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, tokens || pooled || cls_attention, "relax_vit_features_canvas: no output requested");
    return vit_forward(h, "relax_vit_features_canvas", images, N, Hc, Wc, tokens, pooled, cls_attention, stream);
}

int relax_vit_intermediate_layers(relax_handle* h, const uint8_t* images, int N, int Hc, int Wc, int n_last, float* tokens, float* cls,
                                  float* pooled, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->vit.loaded, "relax_vit_intermediate_layers: call relax_load_vit first");
    RELAX_REQUIRE(h, n_last >= 1 && n_last <= h->vit.depth, "relax_vit_intermediate_layers: n_last=%d outside [1, %d] (the loaded model's depth)",
                  n_last, h->vit.depth);
    RELAX_REQUIRE(h, tokens || cls || pooled, "relax_vit_intermediate_layers: no output requested");
    const VitTaps taps{n_last, tokens, cls, pooled};
    return vit_forward(h, "relax_vit_intermediate_layers", images, N, Hc, Wc, nullptr, nullptr, nullptr, stream, &taps);
}

int relax_vit_canvas_geometry(relax_handle* h, int Hc, int Wc, int* gh, int* gw, int* ntok) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->vit.loaded, "relax_vit_canvas_geometry: call relax_load_vit first");
    host::VitCanvasGeometry cg;
    std::string err;
    RELAX_REQUIRE(h, host::vit_canvas_geometry(h->vit.patch, Hc, Wc, &cg, err), "relax_vit_canvas_geometry: %s", err.c_str());
    if (gh) *gh = cg.gh;
    if (gw) *gw = cg.gw;
    if (ntok) *ntok = cg.ntok;
    return RELAX_OK;
}

int relax_vit_pos_embed(relax_handle* h, int gh, int gw, float* out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->vit.loaded, "relax_vit_pos_embed: call relax_load_vit first");
    RELAX_REQUIRE(h, out, "relax_vit_pos_embed: out is NULL");
    RELAX_REQUIRE(h, gh >= 1 && gw >= 1 && (int64_t)gh * gw <= host::kVitMaxPatches, "relax_vit_pos_embed: grid %d x %d (at least 1 x 1, at most %d patches)",
                  gh, gw, host::kVitMaxPatches);
    const int side = 224 / h->vit.patch;
    const host::VitCanvasGeometry cg{gh, gw, gh * gw, gh * gw + 1, gh == side && gw == side};
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* table = nullptr;
    RELAX_TRY(vit_pos_table(h, cg, s, &table));
    RELAX_HIP_CHECK(h, hipMemcpyAsync(out, table, sizeof(float) * (size_t)cg.ntok * h->vit.dim, hipMemcpyDeviceToDevice, s));
    return RELAX_OK;
}

int relax_vit_geometry(relax_handle* h, int* patch, int* ntok, int* dim, int* heads) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->vit.loaded, "relax_vit_geometry: call relax_load_vit first");
    if (patch) *patch = h->vit.patch;
    if (ntok) *ntok = h->vit.ntok;
    if (dim) *dim = h->vit.dim;
    if (heads) *heads = h->vit.heads;
    return RELAX_OK;
}

int relax_op_token_stats(relax_handle* h, const float* x, float* out, int Nimg, int tokens, int dim,
                         relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, x && out && Nimg > 0 && tokens > 0 && dim > 0 && dim % 64 == 0,
                  "relax_op_token_stats: bad arguments (dim must be a multiple of 64)");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(vit_token_stats, dim3(dim / 64, Nimg), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, dim,
                       tokens, 0, tokens);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // extern "C"
