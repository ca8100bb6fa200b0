// vd_overlay.hip — detections, tracks and ground truth drawn onto video frames on the device (viddet_amd/overlay.py is the
// definition): rings, tags of text, trails along tracks, ground-truth rings, onto uint8 RGB or NV12 frames.
//
// Arithmetic: two fp32 steps, operation for operation what overlay_host does (no product and sum is contracted into an FMA,
// `/` is the correctly rounded division): the scaling of a box to source pixels and the two decimals of a score.  Everything
// else is integer arithmetic, the segment test in int64.
//
// Launches:
//   k_ovl_prims   a workgroup per frame, a thread per row.  The track words and centres of the valid rows of the L frames
//                 before it (inside the frame's clip) are staged in LDS; every row and every ground-truth row gets ONE
//                 128-byte record at a fixed place of the workspace: the pixel box, the tag box, its text and colours, the
//                 trail's vertices.  An invalid row's record is zero.  Nothing is compacted; no atomics; no order dependence.
//                 The frame's `painted` is set to 0.
//   k_ovl_paint   a workgroup per (frame, tile of 64 x 16 pixels), a thread per 4 adjacent pixels: pixel-centric, so that
//                 overlapping primitives cannot race.  The frame's records are walked top layer first - tags, rings, trails,
//                 ground truth - in batches of 256 units (a row; for trails a (row, vertex) pair: the vertex's square and the
//                 segment to the vertex before it).  A batch is culled against the tile's rectangle and compacted by ballot
//                 into LDS in unit order, then every thread tests its pixels that have no colour yet against the survivors
//                 in that order: the first hit is the topmost primitive.  Nothing limits the primitives of a tile.  The font
//                 and the palette sit in LDS.  out == frames: only threads with a hit write; out != frames: every pixel is read
//                 and written.  Where every row starts 4-byte aligned and W0 % 4 == 0 a thread moves its 4 pixels as dwords
//                 (RGB: three, NV12: one of luma and on even rows one of chroma), else byte by byte.  `painted` takes one integer
//                 atomicAdd per workgroup with a hit: a sum of integers, bit-reproducible.
// Every record index is f * N + i with f < F, i < N (ground truth: F * N + f * G + g); a vertex count read back from the
// workspace is clamped to trail + 1 and every pixel address is formed from coordinates checked against H0 and W0: whatever the
// workspace holds (vd_overlay_stages), nothing outside the frames is read or written.
#include "vd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kMaxN = 128;
constexpr int kMaxL = 16;
constexpr int kMaxV = kMaxL + 1;                      // vertices of a trail
constexpr int kRowThreads = 128;                      // k_ovl_prims: a thread per row
constexpr int kPaintThreads = 256;
constexpr int kTileW = 64, kTileH = 16;               // 16 threads of 4 pixels a row, 16 rows
constexpr int kBatch = kPaintThreads;                 // units per batch: one per thread
constexpr int kColGt = 256, kColBlack = 257, kColWhite = 258, kPalWords = 259;
constexpr int kMaxText = 32, kMaxSize = 8192;
constexpr int kMaxY = 65535;

struct Rec {                                          // overlay.REC_DTYPE
    int16_t box[4];                                   // px0, py0, px1, py1, inclusive
    int16_t tag[4];                                   // tx0, ty0, tx1, ty1, inclusive, not cut at the frame's edges
    uint16_t col, gcol;                               // palette words of the row's colour and of its glyphs
    uint8_t valid, len;
    int16_t nv;
    uint8_t text[kMaxText];
    int16_t vx[kMaxV][2];
    int32_t pad;
};
static_assert(sizeof(Rec) == VD_OVERLAY_WS_PER_ROW, "the record is VD_OVERLAY_WS_PER_ROW bytes");

__device__ inline bool is_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ inline bool row_valid(float id, float score, const float4 b, float thresh) {
    return id >= 0.f && score >= thresh && is_finite(b.x) && is_finite(b.y) && is_finite(b.z) && is_finite(b.w) && b.x <= b.z &&
           b.y <= b.w;
}

__device__ inline int class_int(float id) { return id >= 2147483648.f ? 0x7fffffff : (int)id; }

__device__ inline int to_pixel(float v, float s, int hi) {
    float p = floorf(v * s);
    p = fmaxf(p, 0.f);
    p = fminf(p, (float)hi);
    return (int)p;
}

__device__ inline void pixel_box(const float4 b, float sx, float sy, int H0, int W0, int& x0, int& y0, int& x1, int& y1) {
    x0 = to_pixel(b.x, sx, W0 - 1);
    y0 = to_pixel(b.y, sy, H0 - 1);
    x1 = to_pixel(b.z, sx, W0 - 1);
    y1 = to_pixel(b.w, sy, H0 - 1);
}

__device__ inline int put_char(uint8_t* text, int n, int c) {
    if (n < kMaxText) text[n] = (uint8_t)c;
    return n + 1;
}

__device__ inline int put_dec(uint8_t* text, int n, unsigned v) {
    bool started = false;
    for (unsigned p = 1000000000u;; p /= 10u) {
        const unsigned d = v / p;
        v -= d * p;
        if (d != 0u || started || p == 1u) {
            n = put_char(text, n, '0' + (int)d);
            started = true;
        }
        if (p == 1u) break;
    }
    return n;
}

__device__ inline int put_name(uint8_t* text, int n, int cls, const uint8_t* __restrict__ names, int n_names) {
    if (names && cls < n_names) {
        for (int k = 0; k < 15; ++k) {
            const int c = names[(int64_t)cls * 16 + k];
            if (c == 0) break;
            n = put_char(text, n, c);
        }
        return n;
    }
    return put_dec(text, n, (unsigned)cls);
}

// the header of a record: box and tag, colours, length - the text and the vertices are written by their own stores
__device__ inline void put_header(Rec* r, int x0, int y0, int x1, int y1, int s, int len, int col, const uint32_t* __restrict__ pal) {
    r->box[0] = (int16_t)x0, r->box[1] = (int16_t)y0, r->box[2] = (int16_t)x1, r->box[3] = (int16_t)y1;
    const int ty0 = y0 - 9 * s >= 0 ? y0 - 9 * s : y0;
    r->tag[0] = (int16_t)x0, r->tag[1] = (int16_t)ty0;
    r->tag[2] = (int16_t)(x0 + 6 * s * len + s - 1), r->tag[3] = (int16_t)(ty0 + 9 * s - 1);
    r->col = (uint16_t)col;
    r->gcol = (uint16_t)(((pal[col] >> 24) & 1u) ? kColWhite : kColBlack);
    r->valid = 1;
    r->len = (uint8_t)len;
}

__global__ __launch_bounds__(kRowThreads) void k_ovl_prims(const float* __restrict__ ids, const float* __restrict__ scores,
                                                           const float* __restrict__ bboxes, const int32_t* __restrict__ track,
                                                           const float* __restrict__ gt, int gt_stride,
                                                           const int32_t* __restrict__ clip_start, int V, int F, int N, int G, int Hn,
                                                           int Wn, int H0, int W0, float thresh, int s, int L, int by_track,
                                                           const uint8_t* __restrict__ names, int n_names,
                                                           const uint32_t* __restrict__ pal, Rec* __restrict__ recs,
                                                           int32_t* __restrict__ painted) {
    __shared__ int s_u[kMaxL][kMaxN];                 // frame f - 1 - d: the track of a valid row, else -1
    __shared__ int s_c[kMaxL][kMaxN];                 // and its centre, x | y << 16
    __shared__ int s_red[kRowThreads];
    const int i = threadIdx.x;
    const float sx = (float)W0 / (float)Wn, sy = (float)H0 / (float)Hn;
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        // the first frame a trail may reach back to: the largest offset of clip_start that is <= f, else 0
        int t0 = 0;
        if (clip_start) {
            int m = 0;
            for (int v = i; v <= V; v += kRowThreads) {
                const int c = clip_start[v];
                if (c <= f && c > m) m = c;
            }
            s_red[i] = m;
            __syncthreads();
            for (int o = kRowThreads / 2; o > 0; o >>= 1) {
                if (i < o) s_red[i] = s_red[i] > s_red[i + o] ? s_red[i] : s_red[i + o];
                __syncthreads();
            }
            t0 = s_red[0];
        }
        for (int d = 1; d <= L; ++d) {
            const int g = f - d;
            int u = -1, c = 0;
            if (g >= t0 && i < N && track) {
                const int64_t row = (int64_t)g * N + i;
                const float4 b = reinterpret_cast<const float4*>(bboxes)[row];
                const int tu = track[row];
                if (tu >= 0 && row_valid(ids[row], scores[row], b, thresh)) {
                    int x0, y0, x1, y1;
                    pixel_box(b, sx, sy, H0, W0, x0, y0, x1, y1);
                    u = tu;
                    c = ((x0 + x1) >> 1) | (((y0 + y1) >> 1) << 16);
                }
            }
            s_u[d - 1][i] = u;
            s_c[d - 1][i] = c;
        }
        __syncthreads();
        if (i == 0) painted[f] = 0;
        if (i < N) {
            const int64_t row = (int64_t)f * N + i;
            Rec* r = recs + row;
            uint4* r4 = reinterpret_cast<uint4*>(r);
#pragma unroll
            for (int k = 0; k < (int)(sizeof(Rec) / 16); ++k) r4[k] = make_uint4(0u, 0u, 0u, 0u);
            const float4 b = reinterpret_cast<const float4*>(bboxes)[row];
            const float id = ids[row], sc = scores[row];
            if (row_valid(id, sc, b, thresh)) {
                int x0, y0, x1, y1;
                pixel_box(b, sx, sy, H0, W0, x0, y0, x1, y1);
                const int cls = class_int(id);
                const int u = track ? track[row] : -1;
                int n = 0;
                if (u >= 0) {
                    n = put_char(r->text, n, '#');
                    n = put_dec(r->text, n, (unsigned)u);
                    n = put_char(r->text, n, ' ');
                }
                n = put_name(r->text, n, cls, names, n_names);
                n = put_char(r->text, n, ' ');
                const float v = sc * 100.0f + 0.5f;   // two operations (contraction is off)
                const int q = v >= 999.0f ? 999 : (v > 0.f ? (int)v : 0);
                n = put_char(r->text, n, '0' + q / 100);
                n = put_char(r->text, n, '.');
                n = put_char(r->text, n, '0' + (q / 10) % 10);
                n = put_char(r->text, n, '0' + q % 10);
                const int len = n < kMaxText ? n : kMaxText;
                put_header(r, x0, y0, x1, y1, s, len, (by_track && u >= 0) ? (u & 255) : (cls & 255), pal);
                int nv = 0;
                if (u >= 0) {
                    r->vx[0][0] = (int16_t)((x0 + x1) >> 1), r->vx[0][1] = (int16_t)((y0 + y1) >> 1);
                    nv = 1;
                    for (int d = 1; d <= L && f - d >= t0; ++d)
                        for (int j = 0; j < N; ++j)
                            if (s_u[d - 1][j] == u) {
                                const int c = s_c[d - 1][j];
                                r->vx[nv][0] = (int16_t)(c & 0xffff), r->vx[nv][1] = (int16_t)(c >> 16);
                                ++nv;
                                break;
                            }
                }
                r->nv = (int16_t)nv;
            }
        }
        if (i < G) {
            const int64_t row = (int64_t)f * G + i;
            Rec* r = recs + (int64_t)F * N + row;
            uint4* r4 = reinterpret_cast<uint4*>(r);
#pragma unroll
            for (int k = 0; k < (int)(sizeof(Rec) / 16); ++k) r4[k] = make_uint4(0u, 0u, 0u, 0u);
            const float* g = gt + row * gt_stride;
            const float4 b = make_float4(g[0], g[1], g[2], g[3]);
            const float id = g[4];
            if (row_valid(id, 0.f, b, 0.f)) {
                int x0, y0, x1, y1;
                pixel_box(b, sx, sy, H0, W0, x0, y0, x1, y1);
                const int n = put_name(r->text, 0, class_int(id), names, n_names);
                put_header(r, x0, y0, x1, y1, s, n < kMaxText ? n : kMaxText, kColGt, pal);
            }
        }
        __syncthreads();                              // s_u, s_c and s_red before the next frame overwrites them
    }
}

// ---- paint
struct RowEnt {                                       // a surviving row of a batch: 56 bytes
    int16_t box[4], tag[4];
    uint16_t col, gcol, len, pad;
    uint32_t text[kMaxText / 4];
};
struct SegEnt {                                       // a surviving (row, vertex): the vertex b, the one before it a
    int16_t ax, ay, bx, by;
    uint16_t col, seg;
};

struct Lds {
    RowEnt row[kBatch];
    SegEnt seg[kBatch];
    uint32_t pal[kPalWords];
    uint32_t font[95 * 2];                            // 7 row bytes and a pad per glyph
    int cnt[kPaintThreads / kWave];
    int hits[kPaintThreads / kWave];
};

struct Px {
    int x, y;                                         // the thread's first pixel
    int c[4];                                         // the palette word of each, -1: none yet
    unsigned live;                                    // bit e: pixel e lies in the frame and has no colour yet
};

// the position of this thread's survivor in the compacted batch (unit order is kept), and the number of survivors
__device__ inline int compact(Lds& l, bool hit, int& total) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) l.cnt[wave] = __popcll(votes);
    __syncthreads();
    int pos = __popcll(votes & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < kPaintThreads / kWave; ++w) {
        if (w < wave) pos += l.cnt[w];
        total += l.cnt[w];
    }
    return pos;
}

__device__ inline bool glyph_at(const Lds& l, const RowEnt& e, int x, int y, int s) {
    const int rx = x - (e.tag[0] + s), ry = y - (e.tag[1] + s);
    if (rx < 0 || ry < 0) return false;
    const int cell = 6 * s;
    const int k = rx / cell, gx = (rx - k * cell) / s, gy = ry / s;
    if (k >= e.len || gx >= 5 || gy >= 7) return false;
    const unsigned ch = ((e.text[k >> 2] >> (8 * (k & 3))) & 255u) - 32u;
    if (ch >= 95u) return false;
    const unsigned bits = (l.font[ch * 2 + (gy >> 2)] >> (8 * (gy & 3))) & 255u;
    return (bits >> (4 - gx)) & 1u;
}

// a colour read back from the workspace, kept inside the palette
__device__ inline uint16_t pal_word(unsigned c) { return (uint16_t)(c < (unsigned)kPalWords ? c : kPalWords - 1); }

constexpr int kModeTag = 1, kModeRing = 2;

// one layer of rows: `count` records from `base`, lower index on top; with both modes a row's tag lies over its own ring
__device__ inline void walk_rows(Lds& l, const Rec* __restrict__ base, int count, int mode, int tx0, int ty0, int t, int s, Px& p) {
    const int tid = threadIdx.x;
    for (int b0 = 0; b0 < count; b0 += kBatch) {
        const int k = b0 + tid;
        bool hit = false;
        uint4 h0 = make_uint4(0u, 0u, 0u, 0u), h1 = h0;
        if (k < count) {
            h0 = reinterpret_cast<const uint4*>(base + k)[0];     // box, tag
            h1 = reinterpret_cast<const uint4*>(base + k)[1];     // col, gcol, valid, len, nv, 8 bytes of text
            if ((h1.y & 0xffu) != 0u) {
                const int bx0 = (int16_t)(h0.x & 0xffffu), by0 = (int16_t)(h0.x >> 16), bx1 = (int16_t)(h0.y & 0xffffu),
                          by1 = (int16_t)(h0.y >> 16);
                const int gx0 = (int16_t)(h0.z & 0xffffu), gy0 = (int16_t)(h0.z >> 16), gx1 = (int16_t)(h0.w & 0xffffu),
                          gy1 = (int16_t)(h0.w >> 16);
                const bool in_ring = bx0 < tx0 + kTileW && bx1 >= tx0 && by0 < ty0 + kTileH && by1 >= ty0;
                const bool in_tag = gx0 < tx0 + kTileW && gx1 >= tx0 && gy0 < ty0 + kTileH && gy1 >= ty0;
                hit = ((mode & kModeRing) && in_ring) || ((mode & kModeTag) && in_tag);
            }
        }
        int total;
        const int pos = compact(l, hit, total);
        if (hit) {
            RowEnt& e = l.row[pos];
            uint32_t* w = reinterpret_cast<uint32_t*>(&e);
            w[0] = h0.x, w[1] = h0.y, w[2] = h0.z, w[3] = h0.w;
            e.col = pal_word(h1.x & 0xffffu), e.gcol = pal_word(h1.x >> 16);
            int len = (int)((h1.y >> 8) & 0xffu);
            e.len = (uint16_t)(len < kMaxText ? len : kMaxText), e.pad = 0;
            const uint32_t* tw = reinterpret_cast<const uint32_t*>((base + k)->text);
#pragma unroll
            for (int q = 0; q < kMaxText / 4; ++q) e.text[q] = tw[q];
        }
        __syncthreads();
        if (p.live)
            for (int n = 0; n < total && p.live; ++n) {
                const RowEnt& e = l.row[n];
                if (mode & kModeTag) {
                    if (p.y >= e.tag[1] && p.y <= e.tag[3] && p.x + 3 >= e.tag[0] && p.x <= e.tag[2]) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int x = p.x + q;
                            if ((p.live & (1u << q)) && x >= e.tag[0] && x <= e.tag[2]) {
                                p.c[q] = glyph_at(l, e, x, p.y, s) ? e.gcol : e.col;
                                p.live &= ~(1u << q);
                            }
                        }
                    }
                }
                if (mode & kModeRing) {
                    if (p.y >= e.box[1] && p.y <= e.box[3] && p.x + 3 >= e.box[0] && p.x <= e.box[2]) {
                        const bool yedge = p.y < e.box[1] + t || p.y > e.box[3] - t;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int x = p.x + q;
                            if ((p.live & (1u << q)) && x >= e.box[0] && x <= e.box[2] &&
                                (yedge || x < e.box[0] + t || x > e.box[2] - t)) {
                                p.c[q] = e.col;
                                p.live &= ~(1u << q);
                            }
                        }
                    }
                }
            }
        __syncthreads();                              // the batch before the next one overwrites it
    }
}

// the trails: unit (row, k) is vertex k of the row - its t x t square, and for k >= 1 the segment from vertex k - 1
__device__ inline void walk_trails(Lds& l, const Rec* __restrict__ base, int N, int nvmax, int tx0, int ty0, int t, Px& p) {
    const int tid = threadIdx.x;
    const int units = N * nvmax;                      // a row has trail + 1 vertices at most
    for (int b0 = 0; b0 < units; b0 += kBatch) {
        const int unit = b0 + tid;
        bool hit = false;
        int ax = 0, ay = 0, bx = 0, by = 0, col = 0, k = 0;
        if (unit < units) {
            const int row = unit / nvmax;
            k = unit - row * nvmax;
            const Rec* r = base + row;
            int nv = r->nv;
            nv = nv < nvmax ? nv : nvmax;
            if (r->valid && k < nv) {
                bx = r->vx[k][0], by = r->vx[k][1];
                ax = bx, ay = by;
                if (k > 0) ax = r->vx[k - 1][0], ay = r->vx[k - 1][1];
                col = r->col;
                const int lo_x = (ax < bx ? ax : bx) - t, hi_x = (ax > bx ? ax : bx) + t;
                const int lo_y = (ay < by ? ay : by) - t, hi_y = (ay > by ? ay : by) + t;
                hit = lo_x < tx0 + kTileW && hi_x >= tx0 && lo_y < ty0 + kTileH && hi_y >= ty0;
            }
        }
        int total;
        const int pos = compact(l, hit, total);
        if (hit) {
            SegEnt& e = l.seg[pos];
            e.ax = (int16_t)ax, e.ay = (int16_t)ay, e.bx = (int16_t)bx, e.by = (int16_t)by;
            e.col = pal_word((unsigned)col), e.seg = (uint16_t)(k > 0);
        }
        __syncthreads();
        if (p.live)
            for (int n = 0; n < total && p.live; ++n) {
                const SegEnt e = l.seg[n];
                const int sq_x = e.bx - (t >> 1), sq_y = e.by - (t >> 1);
                const bool sq_row = p.y >= sq_y && p.y < sq_y + t;
                const int64_t dx = e.bx - e.ax, dy = e.by - e.ay;
                const int64_t dd = dx * dx + dy * dy;
                const bool seg = e.seg && dd != 0;
                if (!sq_row && !seg) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!(p.live & (1u << q))) continue;
                    const int x = p.x + q;
                    bool on = sq_row && x >= sq_x && x < sq_x + t;
                    if (!on && seg) {
                        const int64_t vx = x - e.ax, vy = p.y - e.ay;
                        const int64_t dot = vx * dx + vy * dy, cr = vx * dy - vy * dx;
                        on = dot >= 0 && dot <= dd && 4 * cr * cr <= (int64_t)(t * t) * dd;
                    }
                    if (on) {
                        p.c[q] = e.col;
                        p.live &= ~(1u << q);
                    }
                }
            }
        __syncthreads();
    }
}

template <bool NV12>
__global__ __launch_bounds__(kPaintThreads) void k_ovl_paint(const uint8_t* src, uint8_t* dst,
                                                             int64_t frame_stride, int64_t pitch, int64_t uv_offset, int F, int N,
                                                             int G, int H0, int W0, int t, int s, int L, const uint32_t* __restrict__ pal,
                                                             const uint32_t* __restrict__ font, const Rec* __restrict__ recs,
                                                             int32_t* __restrict__ painted, int tiles_x, int vec) {
    __shared__ Lds l;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int k = tid; k < kPalWords; k += kPaintThreads) l.pal[k] = pal[k];
    for (int k = tid; k < 95 * 2; k += kPaintThreads) l.font[k] = font[k];
    __syncthreads();
    const bool inplace = src == dst;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int tx0 = tile_x * kTileW, ty0 = tile_y * kTileH;
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
        Px p;
        p.x = tx0 + 4 * (tid & 15);
        p.y = ty0 + (tid >> 4);
        p.live = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p.c[q] = -1;
            if (p.y < H0 && p.x + q < W0) p.live |= 1u << q;
        }
        const unsigned inside = p.live;
        const Rec* rows = recs + (int64_t)f * N;
        walk_rows(l, rows, N, kModeTag, tx0, ty0, t, s, p);
        walk_rows(l, rows, N, kModeRing, tx0, ty0, t, s, p);
        walk_trails(l, rows, N, L + 1, tx0, ty0, t, p);
        if (G > 0) walk_rows(l, recs + (int64_t)F * N + (int64_t)f * G, G, kModeTag | kModeRing, tx0, ty0, t, s, p);
        const unsigned got = inside & ~p.live;        // the pixels that took a colour
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = p.c[q] >= 0 ? l.pal[p.c[q]] : 0u;
        if (inside && (got || !inplace)) {
            const int64_t fo = (int64_t)f * frame_stride;
            if (!NV12) {
                const int64_t o = fo + (int64_t)p.y * pitch + 3 * (int64_t)p.x;
                if (vec) {                            // W0 % 4 == 0: the four pixels are all inside
                    const uint32_t* sp = reinterpret_cast<const uint32_t*>(src + o);
                    uint32_t a = sp[0], b = sp[1], c = sp[2];
                    if (got & 1u) a = (a & 0xff000000u) | (w[0] & 0xffffffu);
                    if (got & 2u) a = (a & 0x00ffffffu) | (w[1] << 24), b = (b & 0xffff0000u) | ((w[1] >> 8) & 0xffffu);
                    if (got & 4u) b = (b & 0x0000ffffu) | (w[2] << 16), c = (c & 0xffffff00u) | ((w[2] >> 16) & 0xffu);
                    if (got & 8u) c = (c & 0x000000ffu) | (w[3] << 8);
                    uint32_t* dp = reinterpret_cast<uint32_t*>(dst + o);
                    dp[0] = a, dp[1] = b, dp[2] = c;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (!(inside & (1u << q))) continue;
                        const int64_t oq = o + 3 * q;
                        if (got & (1u << q)) {
                            dst[oq] = (uint8_t)w[q], dst[oq + 1] = (uint8_t)(w[q] >> 8), dst[oq + 2] = (uint8_t)(w[q] >> 16);
                        } else if (!inplace) {
                            dst[oq] = src[oq], dst[oq + 1] = src[oq + 1], dst[oq + 2] = src[oq + 2];
                        }
                    }
                }
            } else {
                // luma: a byte a pixel; chroma: pair (y >> 1, x >> 1) follows luma pixel (y, x) with y and x even
                const int64_t o = fo + (int64_t)p.y * pitch + p.x;
                const int64_t oc = fo + uv_offset + (int64_t)(p.y >> 1) * pitch + p.x;
                const bool chroma = (p.y & 1) == 0 && ((got & 5u) || !inplace);
                if (vec) {
                    uint32_t a = *reinterpret_cast<const uint32_t*>(src + o);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (got & (1u << q)) a = (a & ~(0xffu << (8 * q))) | ((w[q] & 0xffu) << (8 * q));
                    *reinterpret_cast<uint32_t*>(dst + o) = a;
                    if (chroma) {
                        uint32_t c = *reinterpret_cast<const uint32_t*>(src + oc);
                        if (got & 1u) c = (c & 0xffff0000u) | ((w[0] >> 8) & 0xffffu);
                        if (got & 4u) c = (c & 0x0000ffffu) | (((w[2] >> 8) & 0xffffu) << 16);
                        *reinterpret_cast<uint32_t*>(dst + oc) = c;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (!(inside & (1u << q))) continue;
                        if (got & (1u << q))
                            dst[o + q] = (uint8_t)w[q];
                        else if (!inplace)
                            dst[o + q] = src[o + q];
                        if ((q & 1) == 0 && (p.y & 1) == 0) {     // W0 is even: the pair's two bytes are inside with pixel q
                            if (got & (1u << q)) {
                                dst[oc + q] = (uint8_t)(w[q] >> 8), dst[oc + q + 1] = (uint8_t)(w[q] >> 16);
                            } else if (!inplace) {
                                dst[oc + q] = src[oc + q], dst[oc + q + 1] = src[oc + q + 1];
                            }
                        }
                    }
                }
            }
        }
        // the frame's count: the pixels of this tile that took a colour
        int n = __popc(got);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) n += __shfl_xor(n, off);
        if (lane == 0) l.hits[wave] = n;
        __syncthreads();
        if (tid == 0) {
            int sum = 0;
#pragma unroll
            for (int q = 0; q < kPaintThreads / kWave; ++q) sum += l.hits[q];
            if (sum > 0) atomicAdd(painted + f, sum);
        }
        __syncthreads();                              // l.hits before the next frame overwrites it
    }
}

}  // namespace

extern "C" {

int64_t vd_overlay_ws_bytes(int F, int N, int G) {
    if (F < 1 || N < 1 || N > kMaxN || G < 0 || G > kMaxN || (int64_t)F * (N + G) > 0x7fffffff / VD_OVERLAY_WS_PER_ROW) return -1;
    return (int64_t)VD_OVERLAY_WS_PER_ROW * F * (N + G);
}

int vd_overlay_stages(const uint8_t* frames, uint8_t* out, int64_t frame_stride, int64_t pitch, int64_t uv_offset, int fmt, int F,
                      int H0, int W0, const float* ids, const float* scores, const float* bboxes, const int32_t* track,
                      const float* gt, int gt_stride, const int32_t* clip_start, int V, int N, int G, int Hn, int Wn, float thresh,
                      int thickness, int scale, int trail, int by_track, const uint8_t* names, int n_names,
                      const uint32_t* palette, const uint8_t* font, int32_t* painted, void* ws, int64_t ws_bytes, int stages,
                      void* stream) {
    VD_REQUIRE(frames && out, "vd_overlay: frames and out must not be NULL");
    VD_REQUIRE(ids && scores && bboxes, "vd_overlay: ids, scores and bboxes must not be NULL");
    VD_REQUIRE(palette && font && painted && ws, "vd_overlay: palette, font, painted and ws must not be NULL");
    VD_REQUIRE(fmt == 0 || fmt == 1, "vd_overlay: fmt=%d, 0 (RGB) and 1 (NV12) are taken", fmt);
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_overlay: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(G >= 0 && G <= kMaxN, "vd_overlay: G=%d ground-truth rows per frame, 0 <= G <= %d are taken", G, kMaxN);
    VD_REQUIRE(G == 0 || (gt && gt_stride >= 5), "vd_overlay: G=%d needs gt with gt_stride >= 5 floats a row, got gt_stride=%d", G,
               gt_stride);
    VD_REQUIRE(F >= 1 && (int64_t)F * (N + G) <= 0x7fffffff / VD_OVERLAY_WS_PER_ROW,
               "vd_overlay: F=%d frames, F >= 1 and F * (N + G) <= %d are taken", F, 0x7fffffff / VD_OVERLAY_WS_PER_ROW);
    VD_REQUIRE(clip_start ? V >= 1 : V == 1, "vd_overlay: clip_start may be NULL only with V == 1, and V >= 1 is needed, got V=%d", V);
    VD_REQUIRE(thickness >= 1 && thickness <= 8, "vd_overlay: thickness=%d, 1 <= thickness <= 8 are taken", thickness);
    VD_REQUIRE(scale >= 1 && scale <= 4, "vd_overlay: scale=%d, 1 <= scale <= 4 are taken", scale);
    VD_REQUIRE(trail >= 0 && trail <= kMaxL, "vd_overlay: trail=%d, 0 <= trail <= %d are taken", trail, kMaxL);
    VD_REQUIRE(by_track == 0 || by_track == 1, "vd_overlay: by_track=%d, 0 and 1 are taken", by_track);
    VD_REQUIRE(H0 >= 1 && W0 >= 1 && H0 <= kMaxSize && W0 <= kMaxSize, "vd_overlay: H0=%d W0=%d, frames of 1 .. %d pixels a side are taken",
               H0, W0, kMaxSize);
    VD_REQUIRE(Hn >= 1 && Wn >= 1, "vd_overlay: the network's size Hn=%d Wn=%d must be positive", Hn, Wn);
    VD_REQUIRE(thresh == thresh, "vd_overlay: thresh is a NaN");
    VD_REQUIRE(names ? n_names >= 1 : n_names == 0, "vd_overlay: n_names=%d does not fit names (NULL takes 0)", n_names);
    int64_t span;                                     // the bytes of one frame that are touched
    if (fmt == 1) {
        VD_REQUIRE(H0 % 2 == 0 && W0 % 2 == 0, "vd_overlay: NV12 needs an even frame size, got H0=%d W0=%d", H0, W0);
        VD_REQUIRE(pitch >= W0 && pitch < (1ll << 31), "vd_overlay: pitch=%lld, W0=%d <= pitch < 2^31 needed", (long long)pitch, W0);
        VD_REQUIRE(uv_offset >= pitch * H0, "vd_overlay: uv_offset=%lld lies inside the luma plane (pitch * H0 = %lld)",
                   (long long)uv_offset, (long long)(pitch * H0));
        span = uv_offset + pitch * (H0 / 2 - 1) + W0;
    } else {
        VD_REQUIRE(pitch >= 3ll * W0 && pitch < (1ll << 31), "vd_overlay: pitch=%lld, 3 * W0 = %d <= pitch < 2^31 needed",
                   (long long)pitch, 3 * W0);
        span = pitch * (H0 - 1) + 3ll * W0;
    }
    VD_REQUIRE(frame_stride >= span && frame_stride < (1ll << 40), "vd_overlay: frame_stride=%lld, a frame's %lld bytes <= frame_stride < 2^40 needed",
               (long long)frame_stride, (long long)span);
    const int64_t total = (int64_t)(F - 1) * frame_stride + span;
    VD_REQUIRE(out == frames || out + total <= frames || frames + total <= out,
               "vd_overlay: out overlaps frames; out == frames (in place) or two ranges of %lld bytes apart are taken", (long long)total);
    const int64_t need = (int64_t)VD_OVERLAY_WS_PER_ROW * F * (N + G);
    VD_REQUIRE(ws_bytes >= need, "vd_overlay: ws_bytes=%lld, %d * F * (N + G) = %lld needed", (long long)ws_bytes, VD_OVERLAY_WS_PER_ROW,
               (long long)need);
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)ws) % 16) == 0, "vd_overlay: bboxes and ws must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)gt | (uintptr_t)clip_start | (uintptr_t)palette |
                 (uintptr_t)font | (uintptr_t)painted) % 4) == 0,
               "vd_overlay: ids, scores, track, gt, clip_start, palette, font and painted must be 4-byte aligned");
    VD_REQUIRE(stages >= 1 && stages <= 3, "vd_overlay: stages=%d, a mask of 1 (primitives) and 2 (paint) is taken", stages);
    hipStream_t st = (hipStream_t)stream;
    Rec* recs = (Rec*)ws;
    if (stages & 1) {
        hipLaunchKernelGGL(k_ovl_prims, dim3((unsigned)(F < kMaxY ? F : kMaxY)), dim3(kRowThreads), 0, st, ids, scores, bboxes, track, gt,
                           gt_stride, clip_start, V, F, N, G, Hn, Wn, H0, W0, thresh, scale, trail, by_track, names, n_names, palette,
                           recs, painted);
        VD_CHECK_LAUNCH("vd_overlay");
    }
    if (stages & 2) {
        const int tiles_x = (int)vd_cdiv(W0, kTileW), tiles_y = (int)vd_cdiv(H0, kTileH);
        // dwords: every row of both tensors starts 4-byte aligned and a thread's four pixels are all inside
        const int vec = W0 % 4 == 0 && pitch % 4 == 0 && frame_stride % 4 == 0 && (fmt == 0 || uv_offset % 4 == 0) &&
                        (((uintptr_t)frames | (uintptr_t)out) % 4) == 0;
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(F < kMaxY ? F : kMaxY));
        if (fmt == 1)
            hipLaunchKernelGGL(k_ovl_paint<true>, grid, dim3(kPaintThreads), 0, st, frames, out, frame_stride, pitch, uv_offset, F, N, G,
                               H0, W0, thickness, scale, trail, palette, (const uint32_t*)font, (const Rec*)recs, painted, tiles_x, vec);
        else
            hipLaunchKernelGGL(k_ovl_paint<false>, grid, dim3(kPaintThreads), 0, st, frames, out, frame_stride, pitch, uv_offset, F, N, G,
                               H0, W0, thickness, scale, trail, palette, (const uint32_t*)font, (const Rec*)recs, painted, tiles_x, vec);
        VD_CHECK_LAUNCH("vd_overlay");
    }
    return VD_OK;
}

int vd_overlay(const uint8_t* frames, uint8_t* out, int64_t frame_stride, int64_t pitch, int64_t uv_offset, int fmt, int F, int H0,
               int W0, const float* ids, const float* scores, const float* bboxes, const int32_t* track, const float* gt,
               int gt_stride, const int32_t* clip_start, int V, int N, int G, int Hn, int Wn, float thresh, int thickness, int scale,
               int trail, int by_track, const uint8_t* names, int n_names, const uint32_t* palette, const uint8_t* font,
               int32_t* painted, void* ws, int64_t ws_bytes, void* stream) {
    return vd_overlay_stages(frames, out, frame_stride, pitch, uv_offset, fmt, F, H0, W0, ids, scores, bboxes, track, gt, gt_stride,
                             clip_start, V, N, G, Hn, Wn, thresh, thickness, scale, trail, by_track, names, n_names, palette, font,
                             painted, ws, ws_bytes, 3, stream);
}

}  // extern "C"
