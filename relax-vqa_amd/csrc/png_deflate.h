// PNG image-data encode core: the five PNG row filters with libpng's minimum-sum-of-absolute-values choice, run-length
// tokens (zlib's Z_RLE idea: distance-1 matches only), one dynamic Huffman block per band (or stored blocks where those are
// shorter), the per-band Adler-32 and the compaction into one zlib stream per image.  One source, two builds:
//   - png_encode.hip: one 256-thread workgroup per band on gfx950, the band's filtered bytes and its output bits in LDS.
//   - png_encode_host.cpp: PNGE_NT = 1.  The host build runs the same phases over the same kThreads "virtual threads" in
//     a serial loop and the same integer arithmetic, so it produces the same bytes as the device for the same input.
// The stream is cut into bands of whole rows; a band is a plain byte string (its data block has BFINAL = 0 and it ends with
// an empty stored block that byte-aligns it; the last band's empty block carries BFINAL = 1), so the bands of an image
// concatenate into one valid deflate stream.  Every read stays inside the image's rows, every write inside the scratch
// range of the item and its output slot; a refused item stops only itself.
#pragma once
#include <stdint.h>

#include "relax_hip.h"

#if defined(__HIPCC__)
#define PNGE_HD __host__ __device__
#else
#define PNGE_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PNGE_TID ((int)threadIdx.x)
#define PNGE_NT 256
#define PNGE_WLANES 64
#define PNGE_SYNC() __syncthreads()
#else
#define PNGE_TID 0
#define PNGE_NT 1
#define PNGE_WLANES 1
#define PNGE_SYNC() ((void)0)
#endif
// one pass of every (virtual) thread: the device runs one iteration per thread, the host all of them in turn
#define PNGE_FOR_T(t) for (int t = PNGE_TID; t < pnge::kThreads; t += PNGE_NT)

namespace pnge {

constexpr int kThreads = 256;           // threads of a workgroup = chunks a band is cut into for the token passes
constexpr int kBandBytes = 24576;       // filtered bytes of one band (rows * (1 + W*C)); one row of the widest image fits
constexpr int kMaxRowBytes = 16384;     // W*C limit, the decoder's
constexpr int kSyms = 286;              // literal/length alphabet
constexpr int kBandTail = 10;           // worst band: 5 (stored block header) + 5 (the empty stored block that ends it)
constexpr int kPlanHeader = 64;         // scratch: [header][N plan entries of 64 B][16 B of meta per band][band slots]
constexpr int kPlanEntry = 64;
constexpr int kBandMeta = 16;
static_assert(kBandBytes <= 65535, "a band must fit one stored block");
static_assert(kBandBytes >= kMaxRowBytes + 1, "a band holds at least one row");

// plan entry of one item (int64 words)
enum { P_BAND0 = 0, P_NBANDS, P_ROWS, P_SLOT, P_DATA, P_STATUS, P_LEN, P_WORDS = 8 };

struct Shared {
    uint8_t f[kBandBytes];                      // the band's filtered bytes
    uint32_t out[(kBandBytes + 16) / 4];        // the dynamic block's bits; before that, the Huffman build's work memory
    uint32_t hist[288];
    uint16_t code[288];                         // bit-reversed canonical codes
    uint8_t len[288];
    uint16_t lead[kThreads], trail[kThreads];   // per chunk: length of the run at its start / at its end
    uint64_t scan[kThreads];
    uint32_t blcount[16], nextcode[16];
    uint32_t nused, extra, adler_a, adler_b, nlit, stored;
};

// Huffman build work memory, laid over Shared::out (which is cleared after the build)
struct Build {
    uint32_t freq[2 * kSyms];
    uint16_t parent[2 * kSyms];
    uint16_t depth[2 * kSyms];
    uint16_t order[kSyms];                      // used symbols by ascending (count, symbol)
};
static_assert(sizeof(Build) <= sizeof(uint32_t) * ((kBandBytes + 16) / 4), "the build memory fits the output buffer");

PNGE_HD inline void add32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
PNGE_HD inline void or32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
// sum over the lanes of a wave (the host's wave has one lane)
PNGE_HD inline uint32_t wave_sum(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
#endif
    return v;
}

// In-place exclusive prefix sum of a[0, kThreads) -> the total.  Called by every thread.
PNGE_HD inline uint64_t scan_array(uint64_t* a) {
    PNGE_SYNC();
#if defined(__HIP_DEVICE_COMPILE__)
    const int t = PNGE_TID;
    const uint64_t own = a[t];
    uint64_t v = own;
    for (int o = 1; o < kThreads; o <<= 1) {
        const uint64_t u = t >= o ? a[t - o] : 0;
        PNGE_SYNC();
        v += u;
        a[t] = v;
        PNGE_SYNC();
    }
    const uint64_t total = a[kThreads - 1];
    PNGE_SYNC();
    a[t] = v - own;
    PNGE_SYNC();
    return total;
#else
    uint64_t run = 0;
    for (int t = 0; t < kThreads; ++t) {
        const uint64_t v = a[t];
        a[t] = run;
        run += v;
    }
    return run;
#endif
}

// ---- geometry --------------------------------------------------------------------------------------------------------
// Rows per band for rows of rb = W*C bytes.
PNGE_HD inline int64_t band_rows(int64_t rb) { return kBandBytes / (rb + 1) > 0 ? kBandBytes / (rb + 1) : 1; }

// -> the largest zlib stream of an H x W x C image (< 0: refused geometry); *scratch: the scratch bytes the item needs
// (the sum over a call's items is what relax_png_encode wants); *rows: rows per band; *nbands, *slot: the band count and
// the scratch slot of one band.
PNGE_HD inline int64_t bound(int64_t H, int64_t W, int64_t C, int64_t filter, int64_t* scratch, int64_t* rows, int64_t* nbands,
                             int64_t* slot) {
    if (H < 1 || H > (1 << 24) || W < 1 || W > kMaxRowBytes || !(C == 1 || C == 3) || W * C > kMaxRowBytes || filter < -1 ||
        filter > 4)
        return -1;
    const int64_t rb = W * C, R = band_rows(rb);
    const int64_t nb = (H + R - 1) / R;
    const int64_t sl = ((R < H ? R : H) * (rb + 1) + kBandTail + 15) / 16 * 16;
    if (scratch) *scratch = kPlanHeader + kPlanEntry + nb * (kBandMeta + sl);
    if (rows) *rows = R;
    if (nbands) *nbands = nb;
    if (slot) *slot = sl;
    return 2 + H * (rb + 1) + kBandTail * nb + 4;
}

// ---- plan: one workgroup per call ------------------------------------------------------------------------------------
// Validates every item, cuts it into bands and lays the bands out in the scratch.  scratch[0] = total bands.
PNGE_HD inline void plan(uint64_t* tmp, const int64_t* items, int N, int64_t images_bytes, int64_t out_bytes, uint8_t* scratch,
                         int64_t scratch_bytes, int64_t* lengths, int32_t* status) {
    int64_t* hdr = (int64_t*)scratch;
    int64_t* plans = (int64_t*)(scratch + kPlanHeader);
    int64_t band0 = 0;
    // pass 1: geometry and ranges; band counts -> band0
    for (int base = 0; base < N; base += kThreads) {
        PNGE_FOR_T(t) {
            const int n = base + t;
            uint64_t nb = 0;
            if (n < N) {
                const int64_t* it = items + (int64_t)n * 8;
                const int64_t io = it[0], stride = it[1], H = it[2], W = it[3], Cc = it[4], oo = it[5], oc = it[6], ft = it[7];
                int64_t R = 0, nbands = 0, slot = 0;
                const int64_t b = bound(H, W, Cc, ft, nullptr, &R, &nbands, &slot);
                bool ok = b > 0 && io >= 0 && oo >= 0 && oc >= 0 && oo <= out_bytes && oc <= out_bytes - oo;
                if (ok) {
                    // the last row ends inside the images: by division, (H - 1) * stride cannot be formed safely for every item
                    const int64_t rb = W * Cc, room = images_bytes - io - rb;
                    ok = room >= 0 && (H == 1 || (stride >= rb && H - 1 <= room / stride));
                }
                int64_t* p = plans + (int64_t)n * P_WORDS;
                p[P_NBANDS] = ok ? nbands : 0;
                p[P_ROWS] = R;
                p[P_SLOT] = slot;
                p[P_STATUS] = ok ? RELAX_PNG_OK : RELAX_PNG_BAD_ARGS;
                p[P_LEN] = 0;
                nb = ok ? (uint64_t)nbands : 0;
            }
            tmp[t] = nb;
        }
        const uint64_t total = scan_array(tmp);
        PNGE_FOR_T(t) {
            const int n = base + t;
            if (n < N) plans[(int64_t)n * P_WORDS + P_BAND0] = band0 + (int64_t)tmp[t];
        }
        band0 += (int64_t)total;
        PNGE_SYNC();
    }
    // pass 2: the band slots.  An item whose slots do not fit the scratch is refused and takes none (its bands keep their
    // meta entries, which are counted below before anything else is laid out).
    const int64_t total_bands = band0;
    const int64_t data0 = kPlanHeader + (int64_t)kPlanEntry * N + kBandMeta * total_bands;
    int64_t at = data0;
    for (int base = 0; base < N; base += kThreads) {
        PNGE_FOR_T(t) {
            const int n = base + t;
            tmp[t] = n < N ? (uint64_t)(plans[(int64_t)n * P_WORDS + P_NBANDS] * plans[(int64_t)n * P_WORDS + P_SLOT]) : 0;
        }
        const uint64_t total = scan_array(tmp);
        PNGE_FOR_T(t) {
            const int n = base + t;
            if (n < N) {
                int64_t* p = plans + (int64_t)n * P_WORDS;
                const int64_t d = at + (int64_t)tmp[t];
                p[P_DATA] = d;
                if (data0 > scratch_bytes || d > scratch_bytes || p[P_NBANDS] * p[P_SLOT] > scratch_bytes - d) {
                    p[P_STATUS] = RELAX_PNG_BAD_ARGS;
                    p[P_ROWS] = 0;          // its bands are skipped
                }
                if (p[P_STATUS] != RELAX_PNG_OK) {
                    status[n] = (int32_t)p[P_STATUS];
                    lengths[n] = 0;
                }
            }
        }
        at += (int64_t)total;
        PNGE_SYNC();
    }
    if (PNGE_TID == 0) {
        hdr[0] = data0 <= scratch_bytes ? total_bands : 0;
        hdr[1] = N;
    }
}

// ---- filter ----------------------------------------------------------------------------------------------------------
PNGE_HD inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// Byte i of the PNG row (RGB order) in a source row (BGR order for C = 3).
PNGE_HD inline int src_index(int i, int C) {
    if (C == 1) return i;
    const int px = i / 3;
    return 3 * px + 2 - (i - 3 * px);
}

PNGE_HD inline uint32_t abs_signed(int v) {
    v &= 255;
    return (uint32_t)(v < 128 ? v : 256 - v);
}

// Rows [y0, y0 + rows) of the image -> s.f: each row's filter byte and its filtered bytes.  A wave takes a row at a time:
// the five candidate sums are integer sums over the row, so their value does not depend on how the lanes split it.
PNGE_HD inline void filter_band(Shared& s, const uint8_t* img, int64_t stride, int y0, int rows, int W, int C, int forced) {
    const int rb = W * C;
    const int wave = PNGE_TID / PNGE_WLANES, wlane = PNGE_TID % PNGE_WLANES, waves = PNGE_NT / PNGE_WLANES;
    for (int r = wave; r < rows; r += waves) {
        const int y = y0 + r;
        const uint8_t* cur = img + (int64_t)y * stride;
        const uint8_t* up = y > 0 ? img + (int64_t)(y - 1) * stride : nullptr;
        int ft = forced;
        if (ft < 0) {
            uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
            for (int i = wlane; i < rb; i += PNGE_WLANES) {
                const int k = src_index(i, C);
                const int x = cur[k], a = i >= C ? cur[k - C] : 0, b = up ? up[k] : 0, c = (up && i >= C) ? up[k - C] : 0;
                s0 += abs_signed(x);
                s1 += abs_signed(x - a);
                s2 += abs_signed(x - b);
                s3 += abs_signed(x - ((a + b) >> 1));
                s4 += abs_signed(x - paeth(a, b, c));
            }
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            s3 = wave_sum(s3);
            s4 = wave_sum(s4);
            ft = 0;
            uint32_t best = s0;
            if (s1 < best) { best = s1; ft = 1; }
            if (s2 < best) { best = s2; ft = 2; }
            if (s3 < best) { best = s3; ft = 3; }
            if (s4 < best) { best = s4; ft = 4; }
        }
        uint8_t* dst = s.f + (int64_t)r * (rb + 1);
        if (wlane == 0) dst[0] = (uint8_t)ft;
        for (int i = wlane; i < rb; i += PNGE_WLANES) {
            const int k = src_index(i, C);
            const int x = cur[k], a = i >= C ? cur[k - C] : 0, b = up ? up[k] : 0, c = (up && i >= C) ? up[k - C] : 0;
            int v;
            if (ft == 0) v = x;
            else if (ft == 1) v = x - a;
            else if (ft == 2) v = x - b;
            else if (ft == 3) v = x - ((a + b) >> 1);
            else v = x - paeth(a, b, c);
            dst[1 + i] = (uint8_t)v;
        }
    }
    PNGE_SYNC();
}

// ---- tokens ----------------------------------------------------------------------------------------------------------
// Length 3..258 -> symbol, extra bits and their count (RFC 1951 section 3.2.5).
PNGE_HD inline void length_code(int len, int* sym, int* ebits, int* eval) {
    if (len == 258) {
        *sym = 285; *ebits = 0; *eval = 0;
        return;
    }
    const int l = len - 3;
    if (l < 8) {
        *sym = 257 + l; *ebits = 0; *eval = 0;
        return;
    }
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    *sym = 257 + 4 + 4 * e + ((l >> e) - 4);
    *ebits = e;
    *eval = l & ((1 << e) - 1);
}

// The chunk [c0, c1) of thread t in a band of n bytes.
PNGE_HD inline void chunk_of(int t, int n, int* c0, int* c1) {
    const int cs = (n + kThreads - 1) / kThreads;
    int a = t * cs, b = a + cs;
    if (a > n) a = n;
    if (b > n) b = n;
    *c0 = a;
    *c1 = b;
}

// Per chunk: the length of the run of equal bytes at its start and at its end (both = the chunk's size if it is one run).
PNGE_HD inline void chunk_runs(Shared& s, int n) {
    PNGE_FOR_T(t) {
        int c0, c1;
        chunk_of(t, n, &c0, &c1);
        int lead = 0, trail = 0;
        if (c1 > c0) {
            lead = 1;
            while (c0 + lead < c1 && s.f[c0 + lead] == s.f[c0]) ++lead;
            trail = 1;
            while (c1 - 1 - trail >= c0 && s.f[c1 - 1 - trail] == s.f[c1 - 1]) ++trail;
        }
        s.lead[t] = (uint16_t)lead;
        s.trail[t] = (uint16_t)trail;
    }
    PNGE_SYNC();
}

// The tokens whose first byte lies in thread t's chunk, in order.  A run of L equal bytes is its first byte as a literal,
// then distance-1 matches of up to 258 bytes over the L - 1 bytes that follow; a piece of 1 or 2 bytes is literals.  The
// run a chunk starts or ends in is measured across the neighbouring chunks (chunk_runs), so the tokens do not depend on
// where the chunks are cut; no run reaches before the band's first byte.
template <class OnLiteral, class OnMatch>
PNGE_HD inline void for_each_token(const Shared& s, int n, int t, OnLiteral lit, OnMatch match) {
    int c0, c1;
    chunk_of(t, n, &c0, &c1);
    if (c0 >= c1) return;
    const int cs = (n + kThreads - 1) / kThreads;
    int i = c0;
    while (i < c1) {
        const uint8_t v = s.f[i];
        int rs = i;
        if (i == c0) {          // bytes equal to v before the chunk
            for (int u = t - 1; u >= 0; --u) {
                if (s.f[(u + 1) * cs - 1] != v) break;
                rs -= s.trail[u];
                if (s.trail[u] < cs) break;
            }
        }
        int re = i + 1;
        if (i == c0) re = c0 + s.lead[t];
        else
            while (re < c1 && s.f[re] == v) ++re;
        if (re == c1 && c1 < n) {          // bytes equal to v after the chunk
            for (int u = t + 1; u < kThreads; ++u) {
                int u0, u1;
                chunk_of(u, n, &u0, &u1);
                if (u0 >= u1 || s.f[u0] != v) break;
                re += s.lead[u];
                if (s.lead[u] < u1 - u0) break;
            }
        }
        const int L = re - rs, stop = re < c1 ? re : c1;
        int p = i;
        while (p < stop) {
            const int k = p - rs;
            if (k == 0) {
                lit(v);
                ++p;
                continue;
            }
            const int j = k - 1, q = j / 258, o = j - q * 258;
            const int rest = (L - 1) - 258 * q, cl = rest < 258 ? rest : 258;
            if (cl < 3) {
                lit(v);
                ++p;
            } else if (o == 0) {
                match(cl);
                p += cl;
            } else {
                p += cl - o;      // inside a match that began in an earlier chunk
            }
        }
        i = stop;
    }
}

// ---- Huffman ---------------------------------------------------------------------------------------------------------
// s.hist -> s.len (a complete code of at most 15 bits over the used symbols, which are at least two: a literal and
// end-of-block) and s.code (bit-reversed).  Returns false only if the length limiting failed (never seen; the band is
// then stored).
PNGE_HD inline bool build_code(Shared& s) {
    Build& b = *reinterpret_cast<Build*>(s.out);
    if (PNGE_TID == 0) s.nused = 0;
    PNGE_SYNC();
    // rank the used symbols by (count, symbol)
    for (int v = PNGE_TID; v < kSyms; v += PNGE_NT) {
        s.len[v] = 0;
        s.code[v] = 0;
        const uint32_t h = s.hist[v];
        if (!h) continue;
        int rank = 0;
        for (int u = 0; u < kSyms; ++u) {
            const uint32_t g = s.hist[u];
            rank += (g && (g < h || (g == h && u < v))) ? 1 : 0;
        }
        b.order[rank] = (uint16_t)v;
        add32(&s.nused, 1);
    }
    PNGE_SYNC();
    if (PNGE_TID == 0) {
        const int m = (int)s.nused;
        bool ok = m >= 2;
        if (ok) {
            for (int i = 0; i < m; ++i) b.freq[i] = s.hist[b.order[i]];
            int li = 0, ii = m, ni = m;           // next leaf, next unmerged internal node, next node to make
            for (int k = 0; k < m - 1; ++k) {
                int pick[2];
                for (int e = 0; e < 2; ++e) {
                    if (li < m && (ii >= ni || b.freq[li] <= b.freq[ii])) pick[e] = li++;
                    else pick[e] = ii++;
                }
                b.freq[ni] = b.freq[pick[0]] + b.freq[pick[1]];
                b.parent[pick[0]] = b.parent[pick[1]] = (uint16_t)ni;
                ++ni;
            }
            const int root = 2 * m - 2;
            b.depth[root] = 0;
            for (int k = root - 1; k >= 0; --k) b.depth[k] = (uint16_t)(b.depth[b.parent[k]] + 1);
            for (int l = 0; l < 16; ++l) s.blcount[l] = 0;
            for (int i = 0; i < m; ++i) s.blcount[b.depth[i] < 15 ? b.depth[i] : 15]++;
            // Kraft sum in units of 2^-15: clipping can only have raised it above 1.  Moving the deepest leaf above level 15
            // one level down and pairing it with a level-15 leaf lowers the sum by exactly one unit (zlib's repair).
            uint32_t kraft = 0;
            for (int l = 1; l < 16; ++l) kraft += s.blcount[l] << (15 - l);
            while (ok && kraft > (1u << 15)) {
                int bits = 14;
                while (bits > 0 && s.blcount[bits] == 0) --bits;
                if (bits == 0 || s.blcount[15] == 0) {
                    ok = false;
                    break;
                }
                s.blcount[bits]--;
                s.blcount[bits + 1] += 2;
                s.blcount[15]--;
                --kraft;
            }
            ok = ok && kraft == (1u << 15);
        }
        if (ok) {
            int i = 0;                            // the rarest symbols take the longest codes
            for (int l = 15; l >= 1; --l)
                for (uint32_t c = 0; c < s.blcount[l]; ++c) s.len[b.order[i++]] = (uint8_t)l;
            uint32_t code = 0;
            s.blcount[0] = 0;
            for (int l = 1; l < 16; ++l) {
                code = (code + s.blcount[l - 1]) << 1;
                s.nextcode[l] = code;
            }
            int nlit = kSyms;
            while (nlit > 257 && s.len[nlit - 1] == 0) --nlit;
            s.nlit = (uint32_t)nlit;
        }
        s.stored = ok ? 0 : 1;
    }
    PNGE_SYNC();
    if (s.stored) return false;
    for (int v = PNGE_TID; v < kSyms; v += PNGE_NT) {
        const int l = s.len[v];
        if (!l) continue;
        uint32_t code = s.nextcode[l];
        for (int u = 0; u < v; ++u) code += s.len[u] == l ? 1 : 0;
        uint32_t rev = 0;
        for (int k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
        s.code[v] = (uint16_t)rev;
    }
    PNGE_SYNC();
    return true;
}

// A thread's bit writer into the shared output words: whole words and the two partial ones are OR-ed in.
struct BitOut {
    uint32_t* words;
    uint64_t acc;
    int filled;
    int64_t w;
    PNGE_HD void init(uint32_t* base, int64_t bitpos) {
        words = base;
        w = bitpos >> 5;
        filled = (int)(bitpos & 31);
        acc = 0;
    }
    PNGE_HD void put(uint32_t v, int nbits) {     // nbits <= 32, v < 2^nbits
        acc |= (uint64_t)v << filled;
        filled += nbits;
        if (filled >= 32) {
            or32(words + w, (uint32_t)acc);
            ++w;
            acc >>= 32;
            filled -= 32;
        }
    }
    PNGE_HD void finish() {
        if (filled > 0) or32(words + w, (uint32_t)acc);
    }
};

// ---- one band --------------------------------------------------------------------------------------------------------
// s.f[0, n) -> dst[0, return value): the band's deflate bytes; *adler = the Adler-32 of s.f[0, n) on its own.
PNGE_HD inline int deflate_band(Shared& s, int n, bool last, uint8_t* dst, uint32_t* adler) {
    for (int v = PNGE_TID; v < 288; v += PNGE_NT) s.hist[v] = 0;
    if (PNGE_TID == 0) s.extra = s.adler_a = s.adler_b = 0;
    chunk_runs(s, n);           // (syncs)
    // pass 1: the histogram, the extra bits, and the Adler-32 sums of the chunk
    PNGE_FOR_T(t) {
        uint32_t extra = 0;
        for_each_token(
            s, n, t, [&](uint8_t v) { add32(&s.hist[v], 1); },
            [&](int len) {
                int sym, eb, ev;
                length_code(len, &sym, &eb, &ev);
                add32(&s.hist[sym], 1);
                extra += (uint32_t)eb + 1;        // + the one-bit distance code
            });
        int c0, c1;
        chunk_of(t, n, &c0, &c1);
        uint32_t a = 0;
        uint64_t b = 0;
        for (int i = c0; i < c1; ++i) {
            a += s.f[i];
            b += (uint64_t)(n - i) * s.f[i];
        }
        if (c1 > c0) {
            add32(&s.extra, extra);
            add32(&s.adler_a, a % 65521u);
            add32(&s.adler_b, (uint32_t)(b % 65521u));
        }
    }
    if (PNGE_TID == 0) s.hist[256] = 1;
    PNGE_SYNC();
    *adler = (((s.adler_b + (uint32_t)n) % 65521u) << 16) | ((1u + s.adler_a) % 65521u);
    const bool coded = build_code(s);
    const int64_t stored_bits = 8 * (int64_t)(5 + n);
    int64_t dyn_bits = stored_bits + 1;
    int hb = 0;
    if (coded) {
        hb = 17 + 19 * 3 + 4 * ((int)s.nlit + 2);
        dyn_bits = hb + s.extra;
        for (int v = 0; v < kSyms; ++v) dyn_bits += (int64_t)s.hist[v] * s.len[v];
    }
    PNGE_SYNC();                // the build memory is read no more
    if (dyn_bits > stored_bits) {
        // one stored block (n <= 65535), then the empty one
        if (PNGE_TID == 0) {
            dst[0] = 0;
            dst[1] = (uint8_t)(n & 255);
            dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)(~n & 255);
            dst[4] = (uint8_t)((~n >> 8) & 255);
            uint8_t* e = dst + 5 + n;
            e[0] = last ? 1 : 0;
            e[1] = 0; e[2] = 0; e[3] = 0xff; e[4] = 0xff;
        }
        for (int i = PNGE_TID; i < n; i += PNGE_NT) dst[5 + i] = s.f[i];
        return n + 10;
    }
    const int total = (int)((dyn_bits + 3 + 7) / 8) + 4;       // + the empty stored block: 3 bits, pad, 00 00 FF FF
    const int words = (total + 3) / 4;
    for (int i = PNGE_TID; i < words; i += PNGE_NT) s.out[i] = 0;
    // pass 2: bits per chunk -> where each chunk's bits start
    PNGE_FOR_T(t) {
        uint64_t bits = 0;
        for_each_token(
            s, n, t, [&](uint8_t v) { bits += s.len[v]; },
            [&](int len) {
                int sym, eb, ev;
                length_code(len, &sym, &eb, &ev);
                bits += (uint64_t)s.len[sym] + eb + 1;
            });
        s.scan[t] = bits;
    }
    scan_array(s.scan);         // (syncs: the cleared words too)
    {
        // the header: BFINAL 0, BTYPE 2, HLIT, HDIST = 2 codes, HCLEN = 19; a code-length code of sixteen 4-bit codes for the
        // lengths 0..15 (16, 17 and 18 unused), in which length v is the code v; then every length plainly
        if (PNGE_TID == 0) {
            BitOut o;
            o.init(s.out, 0);
            o.put(0, 1);
            o.put(2, 2);
            o.put(s.nlit - 257, 5);
            o.put(1, 5);
            o.put(15, 4);
            for (int k = 0; k < 19; ++k) o.put(k < 3 ? 0 : 4, 3);
            o.finish();
        }
        const int nl = (int)s.nlit;
        for (int k = PNGE_TID; k < nl + 2; k += PNGE_NT) {
            const uint32_t l = k < nl ? s.len[k] : 1;            // the two distance codes: one bit each
            const uint32_t rev = ((l & 1) << 3) | ((l & 2) << 1) | ((l & 4) >> 1) | ((l & 8) >> 3);
            BitOut o;
            o.init(s.out, 74 + 4 * (int64_t)k);
            o.put(rev, 4);
            o.finish();
        }
    }
    // pass 3: the tokens
    PNGE_FOR_T(t) {
        BitOut o;
        o.init(s.out, hb + (int64_t)s.scan[t]);
        for_each_token(
            s, n, t, [&](uint8_t v) { o.put(s.code[v], s.len[v]); },
            [&](int len) {
                int sym, eb, ev;
                length_code(len, &sym, &eb, &ev);
                // code, extra bits, then distance symbol 0 (distance 1): the bit 0
                o.put((uint32_t)s.code[sym] | ((uint32_t)ev << s.len[sym]), s.len[sym] + eb + 1);
            });
        o.finish();
    }
    if (PNGE_TID == 0) {
        BitOut o;
        o.init(s.out, dyn_bits - s.len[256]);
        o.put(s.code[256], s.len[256]);
        o.put(last ? 1 : 0, 3);              // the empty stored block: BFINAL, BTYPE 0
        o.finish();
        const int64_t at = (dyn_bits + 3 + 7) / 8;           // LEN 00 00 is already there; NLEN FF FF follows it
        for (int k = 2; k < 4; ++k) {
            const int64_t q = at + k;
            or32(&s.out[q >> 2], 0xffu << ((q & 3) * 8));
        }
    }
    PNGE_SYNC();
    for (int i = PNGE_TID; i < total; i += PNGE_NT) dst[i] = (uint8_t)(s.out[i >> 2] >> ((i & 3) * 8));
    return total;
}

// ---- encode: one workgroup per band ------------------------------------------------------------------------------------
// Band g of the call: finds its item in the plan, filters its rows, deflates them into its scratch slot.
PNGE_HD inline void encode_band(Shared& s, const uint8_t* images, const int64_t* items, int N, uint8_t* scratch, int64_t g) {
    const int64_t* plans = (const int64_t*)(scratch + kPlanHeader);
    int lo = 0, hi = N - 1;                // the last item whose first band is <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plans[(int64_t)mid * P_WORDS + P_BAND0] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* p = plans + (int64_t)lo * P_WORDS;
    const int64_t k = g - p[P_BAND0];
    if (p[P_STATUS] != RELAX_PNG_OK || p[P_ROWS] < 1 || k < 0 || k >= p[P_NBANDS]) return;
    const int64_t* it = items + (int64_t)lo * 8;
    const int H = (int)it[2], W = (int)it[3], C = (int)it[4];
    const int64_t stride = H == 1 ? 0 : it[1];
    const int R = (int)p[P_ROWS];
    const int y0 = (int)(k * R);
    const int rows = H - y0 < R ? H - y0 : R;
    const int n = rows * (W * C + 1);
    PNGE_SYNC();                // the previous band of this workgroup has left the shared memory
    filter_band(s, images + it[0], stride, y0, rows, W, C, (int)it[7]);
    uint8_t* dst = scratch + p[P_DATA] + k * p[P_SLOT];
    uint32_t adler = 0;
    const int len = deflate_band(s, n, k == p[P_NBANDS] - 1, dst, &adler);
    if (PNGE_TID == 0) {
        uint32_t* meta = (uint32_t*)(scratch + kPlanHeader + (int64_t)kPlanEntry * N + kBandMeta * g);
        meta[0] = (uint32_t)len;
        meta[1] = adler;
    }
}

// ---- compaction --------------------------------------------------------------------------------------------------------
// Item n: prefix sums of its band lengths -> each band's place in the output slot (meta word 1 of 64 bits), the zlib
// header 78 01, the combined Adler-32 big-endian, the stream length and the status.  The combine is zlib's
// adler32_combine carried over all bands at once: with a_b = A_b - 1 and S_b = the filtered bytes that follow band b,
// A = 1 + sum a_b and B = sum (B_b + S_b * a_b), everything mod 65521 in 64-bit arithmetic.
PNGE_HD inline void place_bands(uint64_t* tmp, const int64_t* items, int N, int n, uint8_t* out, uint8_t* scratch,
                                int64_t* lengths, int32_t* status) {
    int64_t* p = (int64_t*)(scratch + kPlanHeader) + (int64_t)n * P_WORDS;
    if (p[P_STATUS] != RELAX_PNG_OK) return;          // plan() has written its status
    const int64_t* it = items + (int64_t)n * 8;
    const int64_t H = it[2], rb = it[3] * it[4], oo = it[5], oc = it[6];
    const int64_t nb = p[P_NBANDS], R = p[P_ROWS], g0 = p[P_BAND0];
    uint8_t* metas = scratch + kPlanHeader + (int64_t)kPlanEntry * N;
    const int64_t raw = H * (rb + 1);
    int64_t at = 2;
    uint64_t sa = 0, sb = 0;            // this thread's share of sum a_b and sum (B_b + S_b * a_b)
    for (int64_t base = 0; base < nb; base += kThreads) {
        PNGE_FOR_T(t) {
            const int64_t k = base + t;
            uint64_t len = 0;
            if (k < nb) {
                const uint32_t* m = (const uint32_t*)(metas + kBandMeta * (g0 + k));
                len = m[0];
                const uint64_t A = m[1] & 0xffffu, B = m[1] >> 16;
                const int64_t done = ((k + 1) * R < H ? (k + 1) * R : H) * (rb + 1);
                const uint64_t after = (uint64_t)((raw - done) % 65521);
                const uint64_t a = (A + 65521u - 1u) % 65521u;
                sa = (sa + a) % 65521u;
                sb = (sb + B + after * a) % 65521u;
            }
            tmp[t] = len;
        }
        const uint64_t total = scan_array(tmp);
        PNGE_FOR_T(t) {
            const int64_t k = base + t;
            if (k < nb) *(int64_t*)(metas + kBandMeta * (g0 + k) + 8) = at + (int64_t)tmp[t];
        }
        at += (int64_t)total;
        PNGE_SYNC();
    }
#if defined(__HIP_DEVICE_COMPILE__)
    tmp[PNGE_TID] = sa;
    const uint64_t ta = scan_array(tmp) % 65521u;
    tmp[PNGE_TID] = sb;
    const uint64_t tb = scan_array(tmp) % 65521u;
#else
    const uint64_t ta = sa, tb = sb;    // the one host thread has summed every band
#endif
    const int64_t total = at + 4;
    const bool fits = total <= oc;
    if (PNGE_TID == 0) {
        if (fits) {
            uint8_t* o = out + oo;
            const uint32_t A = (uint32_t)((1 + ta) % 65521u), B = (uint32_t)tb;
            o[0] = 0x78;
            o[1] = 0x01;
            o[at] = (uint8_t)(B >> 8);
            o[at + 1] = (uint8_t)B;
            o[at + 2] = (uint8_t)(A >> 8);
            o[at + 3] = (uint8_t)A;
        }
        lengths[n] = fits ? total : 0;
        status[n] = fits ? RELAX_PNG_OK : RELAX_PNG_OUT_TOO_SMALL;
        p[P_LEN] = fits ? total : 0;
    }
}

// Band g: its bytes from the scratch slot to its place in the item's output slot.
PNGE_HD inline void copy_band(const int64_t* items, int N, uint8_t* out, const uint8_t* scratch, int64_t g) {
    const int64_t* plans = (const int64_t*)(scratch + kPlanHeader);
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plans[(int64_t)mid * P_WORDS + P_BAND0] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* p = plans + (int64_t)lo * P_WORDS;
    const int64_t k = g - p[P_BAND0];
    if (p[P_STATUS] != RELAX_PNG_OK || p[P_LEN] == 0 || k < 0 || k >= p[P_NBANDS]) return;
    const uint8_t* meta = scratch + kPlanHeader + (int64_t)kPlanEntry * N + kBandMeta * g;
    const int64_t len = *(const uint32_t*)meta, at = *(const int64_t*)(meta + 8);
    const uint8_t* src = scratch + p[P_DATA] + k * p[P_SLOT];
    uint8_t* dst = out + items[(int64_t)lo * 8 + 5] + at;
    // bytes up to the first 4-aligned destination address, then words (the source may sit at any address), then the rest
    int64_t head = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    const int64_t nwords = (len - head) / 4;
    for (int64_t i = PNGE_TID; i < head; i += PNGE_NT) dst[i] = src[i];
    for (int64_t i = PNGE_TID; i < nwords; i += PNGE_NT) {
        uint32_t v;
        __builtin_memcpy(&v, src + head + 4 * i, 4);
        *(uint32_t*)(dst + head + 4 * i) = v;
    }
    for (int64_t i = head + 4 * nwords + PNGE_TID; i < len; i += PNGE_NT) dst[i] = src[i];
}

}  // namespace pnge
