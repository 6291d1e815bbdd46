// PNG image-data decode core: zlib header, deflate (stored / fixed / dynamic blocks), Adler-32, the five PNG row filters and
// the conversion to cv2.imread's uint8 BGR.  One source, two builds:
//   - png_decode.hip: one 64-lane workgroup per image on gfx950.  The Huffman decode is wave-uniform (every lane walks the same
//     bit stream, so no lane ever waits on another for the decoder state); the lanes split literal runs, LZ77 copies, table
//     fills, output flushes, the un-filter of None / Up rows, the colour conversion and the Adler-32 sums.
//   - png_host.cpp: PNGD_LANES = 1, built alone under AddressSanitizer + UBSan for tests/test_png_decode_sanitized.py.
// Every read of the compressed stream is bounded by its length, every write by the raw size (H * (1 + W*C)) or the output slot
// (H * W * 3 bytes); a malformed stream ends its own image with a RELAX_PNG_* status and nothing else.
#pragma once
#include <stdint.h>

#include "relax_hip.h"

#if defined(__HIPCC__)
#define PNGD_HD __host__ __device__
#else
#define PNGD_HD
#endif

// byte loops over the lanes: unrolled, so that several loads are in flight before the first result is waited for
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGD_UNROLL _Pragma("unroll 8")
#define PNGD_LANE ((int)threadIdx.x)
#define PNGD_LANES 64
#define PNGD_SYNC() __syncthreads()
#else
#define PNGD_UNROLL
#define PNGD_LANE 0
#define PNGD_LANES 1
#define PNGD_SYNC() ((void)0)
#endif

namespace pngd {

constexpr int kWindow = 32768;          // deflate's window: the LDS ring the LZ77 copies read from
constexpr int kMask = kWindow - 1;
constexpr int kFlush = 8192;            // ring -> raw buffer once this many bytes are pending (pending + 258 stays < kWindow)
constexpr int kFastBits = 10;           // first-level table: codes up to 10 bits; longer codes take the canonical walk
constexpr int kMaxRowBytes = 16384;     // W*C limit: the previous and the current row share the ring during the un-filter
constexpr int64_t kMaxRaw = (int64_t)1 << 31;
constexpr int kStage = 1024;            // compressed bytes staged in LDS at a time (one load latency per KiB, not per word)

// Work memory of one image: LDS on the GPU (40 KiB: four workgroups per CU), heap memory on the host.
struct Shared {
    uint8_t ring[kWindow];
    uint16_t lfast[1 << kFastBits];     // (symbol << 4) | length, 0 = longer code
    uint16_t dfast[1 << kFastBits];
    uint16_t lcount[16], dcount[16];    // codes per length
    uint16_t lsym[320], dsym[32];       // symbols in canonical order
    uint16_t first[16], start[16], next[16];   // table build: first code and first sorted index of each length
    uint8_t lens[19 + 286 + 30];        // code-length code, then the literal/length and distance lengths (fixed: 288 + 32)
    uint8_t stage[kStage + 4];          // input bytes [sbase, sbase + kStage), zero past the end of the stream
    uint64_t red[2 * 64];               // Adler-32 partial sums, one pair per lane
    int32_t flag;
};

// Raw size of an image with W*C bytes per row, or -1 if the geometry is refused.
PNGD_HD inline int64_t raw_size(int64_t H, int64_t W, int64_t C) {
    if (H < 1 || W < 1 || !(C == 1 || C == 3 || C == 4) || W * C > kMaxRowBytes) return -1;
    const int64_t n = H * (1 + W * C);
    return n >= kMaxRaw ? -1 : n;
}

// The bit reader.  Every lane holds the same state.  The compressed bytes come through an LDS stage the lanes fill together,
// kStage bytes at a time; bytes past the end read as zero, and consumed() > 8 * len means the decoder has read into them (a
// truncated stream).
struct Bits {
    const uint8_t* in;
    uint8_t* stage;
    int64_t len;
    int64_t sbase;     // input index of stage[0]
    int64_t pos;       // input index of `word`
    uint64_t buf;
    int cnt;
    uint32_t word;

    PNGD_HD void restage() {
        PNGD_SYNC();
        sbase = pos;
        PNGD_UNROLL
        for (int k = PNGD_LANE; k < kStage; k += PNGD_LANES) {
            const int64_t q = sbase + k;
            stage[k] = (q >= 0 && q < len) ? in[q] : 0;
        }
        PNGD_SYNC();
    }
    PNGD_HD void load() {
        if (pos < sbase || pos + 4 > sbase + kStage) restage();
        const uint8_t* w = stage + (pos - sbase);
        word = (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
    }
    PNGD_HD void init(const uint8_t* p, uint8_t* st, int64_t n, int64_t at) {
        in = p; stage = st; len = n; pos = at; buf = 0; cnt = 0; sbase = -(int64_t)kStage - 8;
        load();
    }
    PNGD_HD void fill() {
        if (cnt <= 32) {
            buf |= (uint64_t)word << cnt;
            cnt += 32;
            pos += 4;
            load();
        }
    }
    PNGD_HD uint32_t take(int n) {          // n <= 32 and n <= cnt
        const uint32_t v = (uint32_t)(buf & ((1ull << n) - 1));
        buf >>= n;
        cnt -= n;
        return v;
    }
    PNGD_HD int64_t consumed() const { return 8 * pos - cnt; }
    PNGD_HD bool overrun() const { return consumed() > 8 * len; }
    // drop to a byte boundary -> input index of the next unread byte
    PNGD_HD int64_t align() const { return (consumed() + 7) >> 3; }
};

// Canonical Huffman decode: first-level table, then the bit-serial walk for longer codes.  -1: no such code.
PNGD_HD inline int decode_sym(Bits& b, const uint16_t* fast, const uint16_t* count, const uint16_t* sym) {
    const uint32_t e = fast[b.buf & ((1u << kFastBits) - 1)];
    if (e) {
        const int l = e & 15;
        b.buf >>= l;
        b.cnt -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    uint64_t bb = b.buf;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(bb & 1);
        bb >>= 1;
        const int c = count[l];
        if (code - c < first) {
            b.buf >>= l;
            b.cnt -= l;
            return sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// Build the tables of one code from s.lens[off, off + n).  codes: the code-length code, which must be complete.  A
// literal/length or distance code may be incomplete only as a single one-bit code (zlib's rule); all-zero distance
// lengths are allowed (a distance then used is an invalid symbol).
PNGD_HD inline int build(Shared& s, int off, int n, uint16_t* fast, uint16_t* count, uint16_t* sym, bool codes) {
    PNGD_SYNC();
    for (int i = PNGD_LANE; i < (1 << kFastBits); i += PNGD_LANES) fast[i] = 0;
    if (PNGD_LANE == 0) {
        for (int l = 0; l < 16; ++l) count[l] = 0;
        for (int i = 0; i < n; ++i) count[s.lens[off + i]]++;
        count[0] = 0;
        int left = 1, maxl = 0, total = 0;
        for (int l = 1; l < 16; ++l) {
            left = (left << 1) - count[l];
            if (left < 0) break;
            if (count[l]) maxl = l;
            total += count[l];
        }
        int err = 0;
        if (left < 0) err = RELAX_PNG_BAD_CODE_LENGTHS;                              // over-subscribed
        else if (codes && total == 0) err = RELAX_PNG_BAD_CODE_LENGTHS;
        else if (left > 0 && total > 0 && (codes || maxl != 1)) err = RELAX_PNG_BAD_CODE_LENGTHS;   // incomplete
        if (!err) {
            int code = 0, idx = 0;
            for (int l = 1; l < 16; ++l) {
                s.first[l] = (uint16_t)code;
                s.start[l] = (uint16_t)idx;
                code = (code + count[l]) << 1;
                idx += count[l];
            }
            for (int l = 1; l < 16; ++l) s.next[l] = s.start[l];
            for (int i = 0; i < n; ++i)
                if (s.lens[off + i]) sym[s.next[s.lens[off + i]]++] = (uint16_t)i;
            s.start[0] = (uint16_t)total;
        }
        s.flag = err;
    }
    PNGD_SYNC();
    if (s.flag) return s.flag;
    const int total = s.start[0];
    for (int i = PNGD_LANE; i < total; i += PNGD_LANES) {
        const int v = sym[i];
        const int l = s.lens[off + v];
        if (l > kFastBits) continue;
        const uint32_t code = s.first[l] + (uint32_t)(i - s.start[l]);
        uint32_t rev = 0;
        for (int k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
        for (uint32_t e = rev; e < (1u << kFastBits); e += 1u << l) fast[e] = (uint16_t)((v << 4) | l);
    }
    PNGD_SYNC();
    return 0;
}

// ring -> raw for the bytes [flushed, p)
PNGD_HD inline void flush(Shared& s, uint8_t* raw, int64_t& flushed, int64_t p) {
    PNGD_SYNC();
    PNGD_UNROLL
    for (int64_t q = flushed + PNGD_LANE; q < p; q += PNGD_LANES) raw[q] = s.ring[q & kMask];
    flushed = p;
}

// LZ77 copy of len bytes from dist back to position p.  Byte k is out[p - dist + k % dist]: every source lies before p,
// so the lanes take 64 bytes per step with no ordering among them, whatever the distance.
PNGD_HD inline void lz_copy(Shared& s, int64_t p, int dist, int len) {
    PNGD_SYNC();
    for (int base = 0; base < len; base += PNGD_LANES) {
        const int k = base + PNGD_LANE;
        uint8_t v = 0;
        if (k < len) {
            const int j = k < dist ? k : k % dist;
            v = s.ring[(p - dist + j) & kMask];
        }
        PNGD_SYNC();
        if (k < len) s.ring[(p + k) & kMask] = v;
    }
}

// Inflate the zlib stream z[0, zlen) into raw[0, n).  -> status; *adler_out = the stream's stored Adler-32.
PNGD_HD inline int inflate(Shared& s, const uint8_t* z, int64_t zlen, uint8_t* raw, int64_t n, uint32_t* adler_out) {
    if (zlen < 2) return RELAX_PNG_TRUNCATED;
    const int cmf = z[0], flg = z[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0) return RELAX_PNG_BAD_ZLIB_HEADER;
    if (flg & 0x20) return RELAX_PNG_PRESET_DICT;
    Bits b;
    b.init(z, s.stage, zlen, 2);
    int64_t p = 0, flushed = 0;
    int last = 0;
    while (!last) {
        b.fill();
        last = (int)b.take(1);
        const int type = (int)b.take(2);
        if (b.overrun()) return RELAX_PNG_TRUNCATED;
        if (type == 3) return RELAX_PNG_BAD_BLOCK_TYPE;
        if (type == 0) {
            const int64_t at = b.align();
            if (at + 4 > zlen) return RELAX_PNG_TRUNCATED;
            const uint32_t len = z[at] | ((uint32_t)z[at + 1] << 8);
            const uint32_t nlen = z[at + 2] | ((uint32_t)z[at + 3] << 8);
            if ((len ^ 0xffffu) != nlen) return RELAX_PNG_BAD_STORED_LEN;
            if (at + 4 + (int64_t)len > zlen) return RELAX_PNG_TRUNCATED;
            if (p + (int64_t)len > n) return RELAX_PNG_OUTPUT_TOO_LONG;
            const uint8_t* src = z + at + 4;
            for (int64_t done = 0; done < (int64_t)len; done += 4096) {
                const int64_t m = (int64_t)len - done < 4096 ? (int64_t)len - done : 4096;
                PNGD_SYNC();
                PNGD_UNROLL
                for (int64_t k = PNGD_LANE; k < m; k += PNGD_LANES) s.ring[(p + k) & kMask] = src[done + k];
                p += m;
                if (p - flushed >= kFlush) flush(s, raw, flushed, p);
            }
            b.init(z, s.stage, zlen, at + 4 + (int64_t)len);
            continue;
        }
        int st;
        if (type == 1) {
            if (PNGD_LANE == 0) {
                for (int i = 0; i < 288; ++i) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
                for (int i = 0; i < 32; ++i) s.lens[288 + i] = 5;     // 30 and 31 complete the code; decoding one is an error
            }
            if ((st = build(s, 0, 288, s.lfast, s.lcount, s.lsym, false))) return st;
            if ((st = build(s, 288, 32, s.dfast, s.dcount, s.dsym, false))) return st;
        } else {
            const int hlit = (int)b.take(5) + 257, hdist = (int)b.take(5) + 1, hclen = (int)b.take(4) + 4;
            if (hlit > 286 || hdist > 30) return RELAX_PNG_BAD_CODE_LENGTHS;
            PNGD_SYNC();
            if (PNGD_LANE == 0)
                for (int i = 0; i < 19; ++i) s.lens[i] = 0;
            const char* order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
            for (int i = 0; i < hclen; ++i) {
                b.fill();
                const uint8_t v = (uint8_t)b.take(3);
                if (PNGD_LANE == 0) s.lens[(uint8_t)order[i]] = v;
            }
            if (b.overrun()) return RELAX_PNG_TRUNCATED;
            if ((st = build(s, 0, 19, s.lfast, s.lcount, s.lsym, true))) return st;
            int i = 0, prev = -1;
            const int total = hlit + hdist;
            while (i < total) {
                b.fill();
                const int sym = decode_sym(b, s.lfast, s.lcount, s.lsym);
                if (sym < 0) return RELAX_PNG_BAD_CODE_LENGTHS;
                int rep = 1, val = sym;
                if (sym == 16) {
                    if (prev < 0) return RELAX_PNG_BAD_CODE_LENGTHS;
                    val = prev;
                    rep = 3 + (int)b.take(2);
                } else if (sym == 17) {
                    val = 0;
                    rep = 3 + (int)b.take(3);
                } else if (sym == 18) {
                    val = 0;
                    rep = 11 + (int)b.take(7);
                }
                if (b.overrun()) return RELAX_PNG_TRUNCATED;
                if (i + rep > total) return RELAX_PNG_BAD_CODE_LENGTHS;
                // the code-length code's own table is read from lfast/lsym, the lengths go to lens[19 + ...]: no overlap
                if (PNGD_LANE == 0)
                    for (int k = 0; k < rep; ++k) s.lens[19 + i + k] = (uint8_t)val;
                i += rep;
                prev = val;
            }
            PNGD_SYNC();
            if (s.lens[19 + 256] == 0) return RELAX_PNG_BAD_CODE_LENGTHS;   // no end-of-block code
            if ((st = build(s, 19, hlit, s.lfast, s.lcount, s.lsym, false))) return st;
            if ((st = build(s, 19 + hlit, hdist, s.dfast, s.dcount, s.dsym, false))) return st;
        }
        for (;;) {
            b.fill();
            int sym = decode_sym(b, s.lfast, s.lcount, s.lsym);
            if (sym < 0) return b.overrun() ? RELAX_PNG_TRUNCATED : RELAX_PNG_BAD_SYMBOL;
            if (sym < 256) {
                if (b.overrun()) return RELAX_PNG_TRUNCATED;
                if (p >= n) return RELAX_PNG_OUTPUT_TOO_LONG;
                if (PNGD_LANE == 0) s.ring[p & kMask] = (uint8_t)sym;
                ++p;
                if (p - flushed >= kFlush) flush(s, raw, flushed, p);
                continue;
            }
            if (sym == 256) {
                if (b.overrun()) return RELAX_PNG_TRUNCATED;
                break;
            }
            sym -= 257;
            if (sym >= 29) return RELAX_PNG_BAD_SYMBOL;
            int len;
            if (sym < 8) len = 3 + sym;
            else if (sym == 28) len = 258;
            else {
                const int e = (sym - 4) >> 2;
                len = ((4 + ((sym - 4) & 3)) << e) + 3 + (int)b.take(e);
            }
            b.fill();
            const int ds = decode_sym(b, s.dfast, s.dcount, s.dsym);
            if (ds < 0 || ds >= 30) return b.overrun() ? RELAX_PNG_TRUNCATED : RELAX_PNG_BAD_SYMBOL;
            int dist;
            if (ds < 4) dist = 1 + ds;
            else {
                const int e = (ds - 2) >> 1;
                dist = ((2 + (ds & 1)) << e) + 1 + (int)b.take(e);
            }
            if (b.overrun()) return RELAX_PNG_TRUNCATED;
            if ((int64_t)dist > p) return RELAX_PNG_DIST_TOO_FAR;
            if (p + len > n) return RELAX_PNG_OUTPUT_TOO_LONG;
            lz_copy(s, p, dist, len);
            p += len;
            if (p - flushed >= kFlush) flush(s, raw, flushed, p);
        }
    }
    flush(s, raw, flushed, p);
    if (p != n) return RELAX_PNG_OUTPUT_TOO_SHORT;
    const int64_t at = b.align();
    if (at + 4 > zlen) return RELAX_PNG_TRUNCATED;
    *adler_out = ((uint32_t)z[at] << 24) | ((uint32_t)z[at + 1] << 16) | ((uint32_t)z[at + 2] << 8) | z[at + 3];
    return 0;
}

PNGD_HD inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// Un-filter raw[0, H*(1+W*C)) row by row (the previous and the current row in the ring), write BGR to out[0, H*W*3) and
// check the Adler-32 of the raw bytes against `adler`.
PNGD_HD inline int unfilter(Shared& s, const uint8_t* raw, int H, int W, int C, uint32_t adler, uint8_t* out) {
    const int rb = W * C;
    const int64_t n = (int64_t)H * (rb + 1);
    uint8_t* prev = s.ring;
    uint8_t* cur = s.ring + kMaxRowBytes;
    PNGD_SYNC();
    for (int i = PNGD_LANE; i < rb; i += PNGD_LANES) prev[i] = 0;
    uint64_t sa = 0, sb = 0;       // this lane's sum of bytes and of (n - j) * byte_j, weights taken mod 65521
    for (int y = 0; y < H; ++y) {
        const int64_t row = (int64_t)y * (rb + 1);
        const int ft = raw[row];
        if (ft > 4) return RELAX_PNG_BAD_FILTER;
        const uint32_t w0 = (uint32_t)((n - row - 1) % 65521);     // weight of the row's first data byte
        if (PNGD_LANE == 0) {
            sa += (uint32_t)ft;
            sb += (uint64_t)((w0 + 1) % 65521) * (uint32_t)ft;
        }
        PNGD_UNROLL
        for (int i = PNGD_LANE; i < rb; i += PNGD_LANES) {
            const uint32_t x = raw[row + 1 + i];
            const uint32_t wi = w0 >= (uint32_t)i ? w0 - (uint32_t)i : w0 + 65521u - (uint32_t)i;
            sa += x;
            sb += (uint64_t)wi * x;
            cur[i] = (uint8_t)(ft == 2 ? x + prev[i] : x);
        }
        PNGD_SYNC();
        for (int ch = PNGD_LANE; (ft == 1 || ft == 3 || ft == 4) && ch < C; ch += PNGD_LANES) {
            // serial along each of the C interleaved chains: lane ch carries its left (a) and upper-left (ul) neighbours
            int a = 0, ul = 0;
            for (int i = ch; i < rb; i += C) {
                const int x = cur[i], up = prev[i];
                int v;
                if (ft == 1) v = x + a;
                else if (ft == 3) v = x + ((a + up) >> 1);
                else v = x + paeth(a, up, ul);
                v &= 255;
                cur[i] = (uint8_t)v;
                a = v;
                ul = up;
            }
        }
        PNGD_SYNC();
        uint8_t* o = out + (int64_t)y * W * 3;
        PNGD_UNROLL
        for (int x = PNGD_LANE; x < W; x += PNGD_LANES) {
            uint8_t bl, gr, rd;
            if (C == 1) {
                bl = gr = rd = cur[x];
            } else {
                rd = cur[x * C];
                gr = cur[x * C + 1];
                bl = cur[x * C + 2];
            }
            o[3 * x] = bl;
            o[3 * x + 1] = gr;
            o[3 * x + 2] = rd;
        }
        uint8_t* t = prev;
        prev = cur;
        cur = t;
    }
    s.red[2 * PNGD_LANE] = sa;
    s.red[2 * PNGD_LANE + 1] = sb;
    PNGD_SYNC();
    uint64_t ta = 0, tb = 0;
    for (int l = 0; l < PNGD_LANES; ++l) {
        ta += s.red[2 * l];
        tb += s.red[2 * l + 1];
    }
    const uint32_t A = (uint32_t)((1 + ta) % 65521), B = (uint32_t)((tb + (uint64_t)(n % 65521)) % 65521);
    if (((B << 16) | A) != adler) return RELAX_PNG_BAD_ADLER;
    return 0;
}

// One image: zlib stream z[0, zlen) of an 8-bit, non-interlaced H x W image with C channels (1 gray, 3 RGB, 4 RGBA)
// -> BGR out[0, H*W*3), using raw[0, raw_size(H, W, C)) as the inflate buffer.
PNGD_HD inline int decode_image(Shared& s, const uint8_t* z, int64_t zlen, int H, int W, int C, uint8_t* raw, uint8_t* out) {
    const int64_t n = raw_size(H, W, C);
    if (n < 0 || zlen < 0) return RELAX_PNG_BAD_ARGS;
    uint32_t adler = 0;
    int st = inflate(s, z, zlen, raw, n, &adler);
    if (st) return st;
    PNGD_SYNC();                    // the raw bytes other lanes flushed
    return unfilter(s, raw, H, W, C, adler, out);
}

}  // namespace pngd
