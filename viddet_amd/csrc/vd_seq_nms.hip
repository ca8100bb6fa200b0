// vd_seq_nms.hip — sequence NMS over the detections of video clips on the device (viddet_amd/seq_nms.py is the definition,
// DESIGN.md 27): boxes of adjacent frames are linked, the highest-scoring sequence is taken and its rows get the sequence's
// score, what overlaps them is suppressed, and that repeats until every row is decided.
//
// Arithmetic: fp32, operation for operation what seq_nms_host does (no product and sum is contracted into an FMA, `/` is the
// correctly rounded division, comparisons are the plain > so that a NaN decides as it does in NumPy):
//   iou  = (iw*ih) / ((a1 + a2) - iw*ih) where iw = min(x2) - max(x1) > 0 and ih > 0, else 0 (min / max propagate a NaN)
//   best = score + b, one add;  avg = (((0 + s0) + s1) + ...) / n in frame order
//
// Three launches on the stream, no synchronisation between workgroups inside one:
//   a. k_seq_link, a workgroup per frame, a thread per row: the row's class (-1: no candidate), its 128-bit mask of the rows of
//      the NEXT frame of its clip with the same class and iou > link_thresh, and of the rows of its OWN frame with the same
//      class and iou > nms_thresh (not itself).  The sweep never computes an IoU, and the table does not grow with the classes.
//   b. k_seq_sweep, ONE wavefront per (clip, class), lane l owning rows l and l + 64 of every frame.  A row's state byte
//      (1 alive, 2 final, 3 dead) is only ever touched by its own lane.  Per round: frames from last to first - the alive set
//      of a frame is two ballots, `best` of the frame and of the one after it sit in LDS, a row's step is a first-max walk over
//      the set bits of (its link mask & the next frame's alive set) - each lane keeping the best start it has seen; a shuffle
//      reduction picks the start (largest best, lowest frame, lowest row); the sequence is walked twice along `next`, once for
//      its score, once to finalise its rows and kill what their same-frame masks cover.  A class with no row in the clip ends
//      after its first sweep.
//   c. k_seq_sort, a wavefront per frame: the stable rank of every final row by new score, the four outputs, -1 rows behind.
// No atomics: every output is the same on every run.  The inputs are never written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_clip_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxN = 128;
constexpr int kNone = 255;                            // `next`: the sequence ends here

// np.minimum / np.maximum of a pair: a NaN on either side gives NaN
__device__ inline float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ inline float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }

__device__ inline float iou(const float4 a, const float4 b) {
    const float iw = np_min(a.z, b.z) - np_max(a.x, b.x);
    const float ih = np_min(a.w, b.w) - np_max(a.y, b.y);
    if (!(iw > 0.f && ih > 0.f)) return 0.f;
    const float inter = iw * ih;
    const float aa = (a.z - a.x) * (a.w - a.y), ab = (b.z - b.x) * (b.w - b.y);
    return inter / ((aa + ab) - inter);
}

// the workspace: [F*N][4] link words, [F*N][4] same-frame words, [F*N] new scores, [F*N] classes, [F*N] states, [F*N] next rows
struct Ws {
    uint32_t* link;
    uint32_t* nms;
    float* score;
    int32_t* cls;
    uint8_t* state;
    uint8_t* next;
};
__host__ __device__ inline Ws ws_split(void* ws, int64_t FN) {
    uint8_t* p = (uint8_t*)ws;
    Ws w;
    w.link = (uint32_t*)p;
    w.nms = (uint32_t*)(p + 16 * FN);
    w.score = (float*)(p + 32 * FN);
    w.cls = (int32_t*)(p + 36 * FN);
    w.state = p + 40 * FN;
    w.next = p + 41 * FN;
    return w;
}

__global__ __launch_bounds__(kMaxN) void k_seq_link(const float* __restrict__ ids, const float* __restrict__ scores,
                                                    const float* __restrict__ bboxes, const int32_t* __restrict__ clip_start,
                                                    int V, int F, int N, int num_class, float link_thresh, float nms_thresh,
                                                    void* ws_) {
    __shared__ float4 s_box[2][kMaxN];                // this frame's rows, the next frame's
    __shared__ int s_cls[2][kMaxN];
    const int i = threadIdx.x;
    const int64_t t = blockIdx.x;
    const Ws ws = ws_split(ws_, (int64_t)F * N);
    // frame t + 1 belongs to the same clip unless a clip starts there (the first offset >= t + 1 is t + 1 itself)
    bool has_next = t + 1 < F;
    if (has_next && clip_start) {
        int lo = 0, hi = V;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (clip_start[mid] < t + 1) lo = mid + 1;
            else hi = mid;
        }
        has_next = clip_start[lo] != t + 1;           // lo <= V: inside the V + 1 offsets
    }
    if (i < N) {
        const int64_t r = t * N + i;
        s_box[0][i] = reinterpret_cast<const float4*>(bboxes)[r];
        s_cls[0][i] = row_class(ids[r], scores[r], num_class);
        if (has_next) {
            s_box[1][i] = reinterpret_cast<const float4*>(bboxes)[r + N];
            s_cls[1][i] = row_class(ids[r + N], scores[r + N], num_class);
        }
    }
    __syncthreads();
    if (i >= N) return;
    const float4 me = s_box[0][i];
    const int c = s_cls[0][i];
    uint32_t link[4] = {0, 0, 0, 0}, same[4] = {0, 0, 0, 0};
    if (c >= 0) {
        for (int j = 0; j < N; ++j) {
            if (has_next && s_cls[1][j] == c && iou(me, s_box[1][j]) > link_thresh) link[j >> 5] |= 1u << (j & 31);
            if (j != i && s_cls[0][j] == c && iou(me, s_box[0][j]) > nms_thresh) same[j >> 5] |= 1u << (j & 31);
        }
    }
    const int64_t r = t * N + i;
    reinterpret_cast<uint4*>(ws.link)[r] = make_uint4(link[0], link[1], link[2], link[3]);
    reinterpret_cast<uint4*>(ws.nms)[r] = make_uint4(same[0], same[1], same[2], same[3]);
    ws.score[r] = 0.f;
    ws.cls[r] = c;
    ws.state[r] = c >= 0 ? 1 : 0;
    ws.next[r] = (uint8_t)kNone;
}

// (value, frame, row) of a start; frame < 0: none.  Larger value first, then the lower frame, then the lower row
__device__ inline bool start_before(float v, int t, int r, float bv, int bt, int br) {
    return t >= 0 && (bt < 0 || v > bv || (v == bv && (t < bt || (t == bt && r < br))));
}

__global__ __launch_bounds__(kWave) void k_seq_sweep(const float* __restrict__ scores, const int32_t* __restrict__ clip_start,
                                                     int F, int N, int rescore, void* ws_) {
    __shared__ float s_best[2][kMaxN];                // by frame parity
    const int lane = threadIdx.x;
    const int c = blockIdx.y;
    const Ws ws = ws_split(ws_, (int64_t)F * N);
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    if (t0 >= t1) return;

    for (;;) {
        float mv = 0.f;
        int mt = -1, mr = 0;                          // the best start this lane has seen
        unsigned long long nx_lo = 0, nx_hi = 0;      // the alive rows of frame t + 1
        for (int t = t1 - 1; t >= t0; --t) {
            const int64_t base = (int64_t)t * N;
            float* __restrict__ cur = s_best[t & 1];
            const float* __restrict__ nxt = s_best[(t + 1) & 1];
            bool alive[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = lane + h * kWave;
                alive[h] = r < N && ws.cls[base + r] == c && ws.state[base + r] == 1;
            }
            const unsigned long long al_lo = __ballot(alive[0]), al_hi = __ballot(alive[1]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!alive[h]) continue;
                const int r = lane + h * kWave;
                const uint4 m = reinterpret_cast<const uint4*>(ws.link)[base + r];
                unsigned long long lo = (((unsigned long long)m.y << 32) | m.x) & nx_lo;
                unsigned long long hi = (((unsigned long long)m.w << 32) | m.z) & nx_hi;
                float b = 0.f;
                int p = kNone;
                while (lo) {                          // set bits in row order, the first maximum by strict >
                    const int j = __ffsll((long long)lo) - 1;
                    lo &= lo - 1;
                    const float v = nxt[j];
                    if (v > b) b = v, p = j;
                }
                while (hi) {
                    const int j = __ffsll((long long)hi) - 1 + kWave;
                    hi &= hi - 1;
                    const float v = nxt[j];
                    if (v > b) b = v, p = j;
                }
                const float v = scores[base + r] + b;
                cur[r] = v;
                ws.next[base + r] = (uint8_t)p;
                if (start_before(v, t, r, mv, mt, mr)) mv = v, mt = t, mr = r;
            }
            nx_lo = al_lo, nx_hi = al_hi;
            __syncthreads();                          // one wavefront: this frame's best before the frame below reads it
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(mv, off, kWave);
            const int ot = __shfl_xor(mt, off, kWave), orow = __shfl_xor(mr, off, kWave);
            if (start_before(ov, ot, orow, mv, mt, mr)) mv = ov, mt = ot, mr = orow;
        }
        if (mt < 0) return;                           // nothing alive (every lane holds the same start)

        // the sequence's score: every lane walks the same rows
        float acc = rescore == 0 ? 0.f : scores[(int64_t)mt * N + mr];
        int n = 0;
        for (int t = mt, i = mr; ; ++t) {
            const float s = scores[(int64_t)t * N + i];
            if (rescore == 0) acc = acc + s;
            else if (s > acc) acc = s;
            ++n;
            i = ws.next[(int64_t)t * N + i];
            if (i >= N || t + 1 >= t1) break;         // kNone >= N
        }
        if (rescore == 0) acc = acc / (float)n;
        // its rows are final, what they cover in their frames is dead
        for (int t = mt, i = mr; ; ++t) {
            const int64_t base = (int64_t)t * N;
            const uint4 m = reinterpret_cast<const uint4*>(ws.nms)[base + i];
            const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = lane + h * kWave;
                if (r >= N) continue;
                if (r == i) {
                    ws.state[base + r] = 2;
                    ws.score[base + r] = acc;
                } else if (((mw[2 * h + (lane >> 5)] >> (lane & 31)) & 1u) && ws.cls[base + r] == c && ws.state[base + r] == 1) {
                    ws.state[base + r] = 3;
                }
            }
            i = ws.next[base + i];
            if (i >= N || t + 1 >= t1) break;
        }
        __syncthreads();                              // the walks are over before the next sweep rewrites `next`
    }
}

__global__ __launch_bounds__(kWave) void k_seq_sort(const float* __restrict__ ids, const float* __restrict__ bboxes, int F, int N,
                                                    float* __restrict__ out_ids, float* __restrict__ out_scores,
                                                    float* __restrict__ out_bboxes, int32_t* __restrict__ out_perm, void* ws_) {
    __shared__ float s_score[kMaxN];
    __shared__ unsigned char s_final[kMaxN];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * N;
    const Ws ws = ws_split(ws_, (int64_t)F * N);
    bool fin[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = lane + h * kWave;
        fin[h] = r < N && ws.state[base + r] == 2;
        if (r < N) {
            s_score[r] = ws.score[base + r];
            s_final[r] = fin[h];
        }
    }
    const int nfinal = __popcll(__ballot(fin[0])) + __popcll(__ballot(fin[1]));
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = lane + h * kWave;
        if (fin[h]) {
            const float s = s_score[r];
            int rank = 0;                             // the final rows a stable sort by -score puts in front
            for (int j = 0; j < N; ++j)
                if (s_final[j] && (s_score[j] > s || (s_score[j] == s && j < r))) ++rank;
            const int64_t o = base + rank;            // a permutation of [0, nfinal)
            out_ids[o] = ids[base + r];
            out_scores[o] = s;
            reinterpret_cast<float4*>(out_bboxes)[o] = reinterpret_cast<const float4*>(bboxes)[base + r];
            out_perm[o] = r;
        }
        if (r < N && r >= nfinal) {
            out_ids[base + r] = -1.f;
            out_scores[base + r] = -1.f;
            reinterpret_cast<float4*>(out_bboxes)[base + r] = make_float4(-1.f, -1.f, -1.f, -1.f);
            out_perm[base + r] = -1;
        }
    }
}

}  // namespace

extern "C" {

int vd_seq_nms_stages(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
                      int num_class, float link_thresh, float nms_thresh, int rescore, float* out_ids, float* out_scores,
                      float* out_bboxes, int32_t* out_perm, void* ws, int64_t ws_bytes, int stages, void* stream) {
    VD_REQUIRE(ids && scores && bboxes, "vd_seq_nms: ids, scores and bboxes must not be NULL");
    VD_REQUIRE(out_ids && out_scores && out_bboxes && out_perm, "vd_seq_nms: the four output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_seq_nms: ws must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_seq_nms: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_seq_nms: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(clip_start || V == 1, "vd_seq_nms: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1 && num_class <= 65535, "vd_seq_nms: 1 <= num_class <= 65535 needed, got %d", num_class);
    VD_REQUIRE(rescore == 0 || rescore == 1, "vd_seq_nms: rescore must be 0 (avg) or 1 (max), got %d", rescore);
    VD_REQUIRE(ws_bytes >= (int64_t)48 * F * N, "vd_seq_nms: ws_bytes=%lld, 48 * F * N = %lld needed", (long long)ws_bytes,
               (long long)((int64_t)48 * F * N));
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)out_bboxes | (uintptr_t)ws) % 16) == 0,
               "vd_seq_nms: bboxes, out_bboxes and ws must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)clip_start | (uintptr_t)out_ids | (uintptr_t)out_scores |
                 (uintptr_t)out_perm) % 4) == 0,
               "vd_seq_nms: ids, scores, clip_start, out_ids, out_scores and out_perm must be 4-byte aligned");
    VD_REQUIRE(stages == 1 || stages == 3 || stages == 7, "vd_seq_nms: stages must be 1, 3 or 7 (the launches made, in order), got %d",
               stages);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_seq_link, dim3((unsigned)F), dim3(kMaxN), 0, s, ids, scores, bboxes, clip_start, V, F, N, num_class,
                       link_thresh, nms_thresh, ws);
    VD_CHECK_LAUNCH("vd_seq_nms");
    if (!(stages & 2)) return VD_OK;
    hipLaunchKernelGGL(k_seq_sweep, dim3((unsigned)V, (unsigned)num_class), dim3(kWave), 0, s, scores, clip_start, F, N, rescore, ws);
    VD_CHECK_LAUNCH("vd_seq_nms");
    if (!(stages & 4)) return VD_OK;
    hipLaunchKernelGGL(k_seq_sort, dim3((unsigned)F), dim3(kWave), 0, s, ids, bboxes, F, N, out_ids, out_scores, out_bboxes,
                       out_perm, ws);
    VD_CHECK_LAUNCH("vd_seq_nms");
    return VD_OK;
}

int vd_seq_nms(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
               int num_class, float link_thresh, float nms_thresh, int rescore, float* out_ids, float* out_scores,
               float* out_bboxes, int32_t* out_perm, void* ws, int64_t ws_bytes, void* stream) {
    return vd_seq_nms_stages(ids, scores, bboxes, clip_start, V, F, N, num_class, link_thresh, nms_thresh, rescore, out_ids,
                             out_scores, out_bboxes, out_perm, ws, ws_bytes, 7, stream);
}

}  // extern "C"
