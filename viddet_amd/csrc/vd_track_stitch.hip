// vd_track_stitch.hip — the track fragments of video clips re-linked across long gaps on the device (viddet_amd/stitch.py is the
// definition): every track's Kalman filter (vd_track_kf.h) is run over its members, its state at its last row is
// extrapolated over the gap to another track's first row, tails and heads are matched by the minimum-cost assignment the
// trackers use, and every chain of fragments takes its first fragment's id.  What stitch_host computes, bit for bit, on all five
// outputs.
//
// Arithmetic: fp32, operation for operation what stitch_host does: no product and sum is contracted into an FMA, `/` and sqrtf
// are the correctly rounded ones (hipcc's default; the Makefile sets no fast-math flag), the IoU is vd_track_math.h's, `iou >=
// sigma_iou` and `s > m` the plain comparisons; q = int(iou * 2^20) is exact; the assignment is integers, its potentials and
// slacks int64.
//
// Launches: vd_clip_rows.h's fill only with clip_start (every row as a frame that no clip covers has it: -1 / 0 / -1), then k_track_stitch,
// ONE workgroup of 256 threads per clip; no communication between workgroups.  Per clip:
//   members    the frames in order, a thread per row: k_smo_member's rule - a present row whose id is usable and that no lower
//              row of its frame carries is the id's member in the frame.  A member's track lives in the clip's table in the
//              workspace, indexed by id: the 17-float filter state field-major, the last frame, the members so far, the maximum
//              score, the first member's row and the classes of the first and the last member.  The first member starts the
//              state, a later one predicts `t - last` times and updates.  The ids of a frame's members differ, so no two
//              threads touch one entry; a barrier stands between frames
//   compact    the used ids in ascending order by ballots and a prefix count; the first 512 are the participants: their tails
//              (x, xd, r, frame, class), heads (box, frame, class), ids, lengths and maxima go into LDS
//   assign     the `assign` loop of vd_track_byte.hip (mot_metric.assign_host operation for operation) on up to 512 rows - the
//              participants as tails - and 1024 columns - the participants as heads, then a dummy per row.  A cell's cost is
//              formed where it is read; ahead of every step of a path max_gap threads extrapolate the step's tail by 1 ..
//              max_gap predictions of the mean (kf_predict's `s + ds <= 0` rule included) into LDS, so a cell is one IoU
//   chains     a thread per participant follows the predecessors to the chain's first track (512 steps at most), then the
//              successors from there, adding the lengths and folding the maxima in chain order; then a thread per row writes the
//              three per-row outputs
// Where things live.  LDS: 58,432 bytes static, so two workgroups fit a CU's 160 KiB; 77 VGPRs, no scratch.  Workspace: 100 bytes per (frame, row) -
// the member id of every row, then the table's 24 words per id; a clip's ids lie in [0, (t1 - t0) * N), so its slice of every
// field starts at its first row.  Only the clip's workgroup touches its slice.  A barrier (which orders global memory within the
// workgroup) stands between every writer and another thread's read.
// Every id read from `track` is checked against [0, (t1 - t0) * N) before it indexes anything, every row and slot read back from
// the workspace likewise; every loop is bounded by F, N, 512, 32 or the clip's rows.  No atomics; plain vector loads and stores;
// the inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"
#include "vd_track_kf.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxTracks = VD_TRACK_STITCH_MAX_TRACKS;
constexpr int kMaxStitchGap = VD_TRACK_STITCH_MAX_GAP;
constexpr int kPartPer = kMaxTracks / kThreads;       // participants of a thread
constexpr int kMaxCols = 2 * kMaxTracks;              // the assignment's columns: the heads, then a dummy per row
constexpr int kColPer = kMaxCols / kThreads;
constexpr long long kInf = 1ll << 62;                 // a forbidden cell, a column that no path reaches
constexpr long long kDummy = 1ll << 27;
constexpr int kQOne = 1 << 20;
constexpr int kFields = kStateFloats + 7;             // the table's words per id

// the workspace of F * N rows: every field is an array of `rows` words
struct Ws {
    int32_t* mem;                                     // [rows] the id the row is a member of, -1: none
    float* st;                                        // [17][rows] the track's filter state after its last member, field-major
    int32_t* last;                                    // [rows] the frame of its last member
    int32_t* cnt;                                     // [rows] its members so far; 0: no track
    float* max;                                       // [rows] its maximum score
    int32_t* head;                                    // [rows] the row (t * N + i) of its first member
    int32_t* tcls;                                    // [rows] the class of its last member
    int32_t* hcls;                                    // [rows] and of its first
    int32_t* slot;                                    // [rows] its place among the participants, -1: beyond them
};

__device__ inline Ws ws_of(void* ws, int64_t rows) {
    Ws w;
    w.mem = (int32_t*)ws;
    w.st = (float*)(w.mem + rows);
    w.last = (int32_t*)(w.st + kStateFloats * rows);
    w.cnt = w.last + rows;
    w.max = (float*)(w.cnt + rows);
    w.head = (int32_t*)(w.max + rows);
    w.tcls = w.head + rows;
    w.hcls = w.tcls + rows;
    w.slot = w.hcls + rows;
    return w;
}

// the 17-float state of entry `e` in a field-major table of `rows` entries
__device__ inline void sti_load(const float* st, int64_t rows, int64_t e, Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.x[i] = st[(0 + i) * rows + e];
        s.xd[i] = st[(3 + i) * rows + e];
        s.p00[i] = st[(6 + i) * rows + e];
        s.p01[i] = st[(9 + i) * rows + e];
        s.p11[i] = st[(12 + i) * rows + e];
    }
    s.r = st[15 * rows + e];
    s.p = st[16 * rows + e];
}

__device__ inline void sti_store(float* st, int64_t rows, int64_t e, const Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        st[(0 + i) * rows + e] = s.x[i];
        st[(3 + i) * rows + e] = s.xd[i];
        st[(6 + i) * rows + e] = s.p00[i];
        st[(9 + i) * rows + e] = s.p01[i];
        st[(12 + i) * rows + e] = s.p11[i];
    }
    st[15 * rows + e] = s.r;
    st[16 * rows + e] = s.p;
}

// The participants of the clip, in LDS
struct Parts {
    float x[3][kMaxTracks], xd[3][kMaxTracks], r[kMaxTracks];   // the tail: the mean of the state after the last member,
    int tf[kMaxTracks], tc[kMaxTracks];                         // its frame and class
    float4 hbox[kMaxTracks];                                    // the head: the first member's input box,
    int hf[kMaxTracks], hc[kMaxTracks];                         // its frame and class
    int id[kMaxTracks], cnt[kMaxTracks];                        // the track's id and members
    float max[kMaxTracks];                                      // and its maximum score
};

// assign_host on the P participants as tails (rows) against the P participants as heads and a dummy per row: column c < P is
// head c, column P + r the dummy of row r.  vd_track_byte.hip's loop; only the cell's cost differs.  Called by the whole
// workgroup alike, with P >= 2.  Leaves s_rowof[c], the row of column c or -1, behind a barrier.
__device__ __forceinline__ void assign(const Parts& p, int P, int max_gap, float thr, float4* s_pb, int* s_way, int* s_rowof,
                                       long long* s_u, long long* s_red_v, int* s_red_j, int tid, int lane, int wave) {
    const int R = P, K = P, C = K + R;
    long long v[kColPer], minv[kColPer];
#pragma unroll
    for (int j = 0; j < kColPer; ++j) {
        const int c = tid + j * kThreads;
        v[j] = 0;
        if (c < C) s_rowof[c] = -1;
    }
    for (int r = tid; r < R; r += kThreads) s_u[r] = 0;
    __syncthreads();
    for (int i = 0; i < R; ++i) {
        unsigned used = 0u;                           // bit j: column tid + j * kThreads is in the tree
#pragma unroll
        for (int j = 0; j < kColPer; ++j) {
            const int c = tid + j * kThreads;
            minv[j] = kInf;
            if (c < C) s_way[c] = -1;
        }
        int i0 = i, j0 = -1;
        for (int step = 0; step <= R; ++step) {       // a path visits a matched column once: i + 1 steps at most
            // the tail of row i0 after 1 .. max_gap predictions: thread g - 1 holds g
            if (tid < max_gap) {
                Kf s;
#pragma unroll
                for (int k = 0; k < 3; ++k) s.x[k] = p.x[k][i0], s.xd[k] = p.xd[k][i0], s.p00[k] = 0.f, s.p01[k] = 0.f, s.p11[k] = 0.f;
                s.r = p.r[i0], s.p = 0.f;             // kf_box reads x and r only
                for (int g = 0; g <= tid; ++g) kf_predict(s);
                s_pb[tid] = kf_box(s);
            }
            __syncthreads();
            const long long ui = s_u[i0];
            const int tf = p.tf[i0], tc = p.tc[i0];
            long long bv = kInf;
            int bj = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < kColPer; ++j) {
                const int c = tid + j * kThreads;
                if (c < C && !((used >> j) & 1u)) {
                    long long cst = kInf;
                    if (c < K) {
                        const int g = p.hf[c] - tf;
                        if (c != i0 && g >= 1 && g <= max_gap && p.hc[c] == tc) {
                            const float q = iou(s_pb[g - 1], p.hbox[c]);
                            if (q >= thr) cst = kQOne - (long long)(int)(q * 1048576.f);
                        }
                    } else if (c - K == i0) {
                        cst = kDummy;
                    }
                    if (cst != kInf) {
                        const long long now = cst - ui - v[j];
                        if (now < minv[j]) minv[j] = now, s_way[c] = j0;
                    }
                    if (minv[j] < bv) bv = minv[j], bj = c;           // c ascends with j: the lowest column of a tie stays
                }
            }
            // the workgroup's minimum over (slack, column): the lowest column of a tie
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const long long ov = __shfl_xor(bv, off, kWave);
                const int oj = __shfl_xor(bj, off, kWave);
                if (ov < bv || (ov == bv && oj < bj)) bv = ov, bj = oj;
            }
            if (lane == 0) s_red_v[wave] = bv, s_red_j[wave] = bj;
            __syncthreads();
            long long delta = s_red_v[0];
            int j1 = s_red_j[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                const long long ov = s_red_v[w];
                const int oj = s_red_j[w];
                if (ov < delta || (ov == delta && oj < j1)) delta = ov, j1 = oj;
            }
            if (delta == kInf || j1 < 0 || j1 >= C) {                // cannot be: the row's dummy is always reachable
                j0 = -1;
                break;                                               // the whole workgroup alike
            }
#pragma unroll
            for (int j = 0; j < kColPer; ++j) {
                const int c = tid + j * kThreads;
                if (c < C) {
                    if ((used >> j) & 1u) {
                        const int ro = s_rowof[c];                   // the used columns are matched, to rows of their own
                        if (ro >= 0 && ro < R) s_u[ro] += delta;
                        v[j] -= delta;
                    } else if (minv[j] != kInf) {
                        minv[j] -= delta;
                    }
                }
            }
            if (tid == 0) s_u[i] += delta;
            if ((j1 & (kThreads - 1)) == tid) used |= 1u << (j1 / kThreads);
            j0 = j1;
            const int r1 = s_rowof[j1];
            __syncthreads();                                         // the potentials before the next step reads them
            if (r1 < 0 || r1 >= R) break;
            i0 = r1;
        }
        if (tid == 0) {                                              // the path back to the new row, every column handed on
            int j = j0;
            for (int n = 0; n < C && j >= 0 && j < C; ++n) {
                const int jp = s_way[j];
                s_rowof[j] = (jp >= 0 && jp < C) ? s_rowof[jp] : i;
                j = jp;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_track_stitch(const float* __restrict__ ids, const float* __restrict__ scores,
                                                           const float* __restrict__ bboxes, const int32_t* __restrict__ track,
                                                           const int32_t* __restrict__ clip_start, int F, int N, int num_class,
                                                           int max_gap, float sigma_iou, int32_t* __restrict__ out_track,
                                                           int32_t* __restrict__ out_len, float* __restrict__ out_score,
                                                           int32_t* __restrict__ out_stitches, int32_t* __restrict__ out_overflow,
                                                           void* ws) {
    __shared__ Parts p;
    __shared__ float4 s_pb[kMaxStitchGap];            // the tail of the path's row after 1 .. 32 predictions
    __shared__ int s_way[kMaxCols];
    __shared__ int s_rowof[kMaxCols];                 // the row (a tail) a column is matched to, -1: none
    __shared__ long long s_u[kMaxTracks];             // the potentials of the assignment's rows
    __shared__ long long s_red_v[kWaves];
    __shared__ int s_red_j[kWaves];
    __shared__ int s_succ[kMaxTracks];                // the head a tail is linked to, -1: none
    __shared__ int c_root[kMaxTracks];                // per participant: the id of its chain's first track,
    __shared__ int c_len[kMaxTracks];                 // the chain's members
    __shared__ float c_max[kMaxTracks];               // and its maximum
    __shared__ int s_uid[kMaxN];                      // the usable ids of a frame's rows
    __shared__ int s_wcnt[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int v = blockIdx.x;
    int t0, t1;
    clip_of(clip_start, v, F, t0, t1);
    if (t0 >= t1) {                                   // the whole workgroup alike
        if (tid == 0) out_stitches[v] = 0, out_overflow[v] = 0;
        return;
    }
    const int64_t rows = (int64_t)F * N;
    const Ws w = ws_of(ws, rows);
    const int64_t lo = (int64_t)t0 * N;               // the clip's rows [lo, lo + clip_rows), and its ids' entries
    const int64_t clip_rows = (int64_t)(t1 - t0) * N;
    const unsigned long long below = (1ull << lane) - 1ull;
    const float4* box = reinterpret_cast<const float4*>(bboxes);

    for (int64_t i = tid; i < clip_rows; i += kThreads) w.cnt[lo + i] = 0;
    __syncthreads();

    // members: the frames in order, a thread per row
    for (int t = t0; t < t1; ++t) {
        const int64_t row = (int64_t)t * N + tid;
        int u = -1, cls = -1;
        float sc = 0.f;
        if (tid < N) {
            const int id = track[row];
            sc = scores[row];
            cls = row_class(ids[row], sc, num_class);
            if (cls >= 0 && id >= 0 && id < clip_rows) u = id;
        }
        if (tid < kMaxN) s_uid[tid] = u;
        __syncthreads();
        if (tid < N) {
            if (u >= 0)
                for (int j = 0; j < tid; ++j)
                    if (s_uid[j] == u) {              // a lower row of the frame carries the id
                        u = -1;
                        break;
                    }
            w.mem[row] = u;
            if (u >= 0) {
                const int64_t e = lo + u;
                const int n = w.cnt[e];
                float z[4];
                Kf s;
                kf_measure(box[row], z);
                if (n <= 0) {
                    kf_start(z, s);
                    w.head[e] = (int)row;
                    w.hcls[e] = cls;
                    w.max[e] = sc;
                } else {
                    sti_load(w.st, rows, e, s);
                    const int g = t - w.last[e];      // >= 1: the track's last member lies in an earlier frame
                    for (int j = 0; j < g && j < F; ++j) kf_predict(s);
                    kf_update(s, z);
                    if (sc > w.max[e]) w.max[e] = sc;
                }
                sti_store(w.st, rows, e, s);
                w.last[e] = t;
                w.cnt[e] = n <= 0 ? 1 : n + 1;
                w.tcls[e] = cls;
            }
        }
        __syncthreads();                              // s_uid before the next frame overwrites it; the table
    }

    // compact: the used ids in ascending order; the first kMaxTracks are the participants
    int total = 0;                                    // every thread alike
    for (int64_t b = 0; b < clip_rows; b += kThreads) {
        const int64_t i = b + tid;
        const bool on = i < clip_rows && w.cnt[lo + i] > 0;
        const unsigned long long votes = __ballot(on);
        if (lane == 0) s_wcnt[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const int n = s_wcnt[k];
            if (k < wave) before += n;
            all += n;
        }
        if (on) {
            const int64_t e = lo + i;
            const int64_t at = (int64_t)total + before + __popcll(votes & below);
            const int k = at < kMaxTracks ? (int)at : -1;
            w.slot[e] = k;
            if (k >= 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) p.x[c][k] = w.st[(0 + c) * rows + e], p.xd[c][k] = w.st[(3 + c) * rows + e];
                p.r[k] = w.st[15 * rows + e];
                p.tf[k] = w.last[e];
                p.tc[k] = w.tcls[e];
                int64_t h = w.head[e];
                if (h < lo || h >= lo + clip_rows) h = lo;           // cannot be: the members pass wrote it
                p.hbox[k] = box[h];
                p.hf[k] = (int)(h / N);
                p.hc[k] = w.hcls[e];
                p.id[k] = (int)i;
                p.cnt[k] = w.cnt[e];
                p.max[k] = w.max[e];
            }
        }
        total = (int)(total + all < 0x7fffffff ? total + all : 0x7fffffff);
        __syncthreads();                              // s_wcnt before the next round overwrites it; the participants
    }
    const int P = total < kMaxTracks ? total : kMaxTracks;

    // the assignment: tails against heads
    if (P >= 2) {
        assign(p, P, max_gap, sigma_iou, s_pb, s_way, s_rowof, s_u, s_red_v, s_red_j, tid, lane, wave);
    } else {
        if (tid < P) s_rowof[tid] = -1;
    }
#pragma unroll
    for (int j = 0; j < kPartPer; ++j) {
        const int k = tid + j * kThreads;
        if (k < P) s_succ[k] = -1;
    }
    __syncthreads();
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kPartPer; ++j) {
        const int c = tid + j * kThreads;
        if (c < P) {
            const int a = s_rowof[c];                 // the rows of two columns differ
            if (a >= 0 && a < P) s_succ[a] = c, ++mine;
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, kWave);
    if (lane == 0) s_wcnt[wave] = mine;
    __syncthreads();

    // chains: back to the first track, then forward through the chain
#pragma unroll
    for (int j = 0; j < kPartPer; ++j) {
        const int k = tid + j * kThreads;
        if (k < P) {
            int r = k;
            for (int n = 0; n < kMaxTracks; ++n) {
                const int a = s_rowof[r];
                if (a < 0 || a >= P) break;
                r = a;
            }
            int len = p.cnt[r], c = r;
            float m = p.max[r];
            for (int n = 0; n < kMaxTracks; ++n) {
                const int nx = s_succ[c];
                if (nx < 0 || nx >= P) break;
                c = nx;
                len += p.cnt[c];
                if (p.max[c] > m) m = p.max[c];
            }
            c_root[k] = p.id[r];
            c_len[k] = len;
            c_max[k] = m;
        }
    }
    if (tid == 0) {
        int links = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) links += s_wcnt[k];
        out_stitches[v] = links;
        out_overflow[v] = total - P;
    }
    __syncthreads();

    // the rows
    for (int64_t i = tid; i < clip_rows; i += kThreads) {
        const int u = w.mem[lo + i];
        int id = -1, len = 0;
        float mx = -1.f;
        if (u >= 0 && u < clip_rows) {
            const int64_t e = lo + u;
            const int k = w.slot[e];
            if (k >= 0 && k < P)
                id = c_root[k], len = c_len[k], mx = c_max[k];
            else
                id = u, len = w.cnt[e], mx = w.max[e];
        }
        out_track[lo + i] = id;
        out_len[lo + i] = len;
        out_score[lo + i] = mx;
    }
}

}  // namespace

extern "C" {

int64_t vd_track_stitch_ws_bytes(int F, int N) {
    if (F < 1 || N < 1 || N > kMaxN || (int64_t)F * N > 0x7fffffff) return -1;
    return (int64_t)VD_TRACK_STITCH_WS_PER_ROW * F * N;
}

int vd_track_stitch(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start,
                    int V, int F, int N, int num_class, int max_gap, float sigma_iou, int32_t* out_track, int32_t* out_len,
                    float* out_score, int32_t* out_stitches, int32_t* out_overflow, void* ws, int64_t ws_bytes, void* stream) {
    static_assert(VD_TRACK_STITCH_WS_PER_ROW == 4 * (1 + kFields), "the workspace: the member id and the table's 24 words a row");
    static_assert(sizeof(Parts) + sizeof(float4) * kMaxStitchGap + 4 * (2 * kMaxCols + 4 * kMaxTracks + kMaxN + 2 * kWaves) +
                          8 * (kMaxTracks + kWaves) < 64 * 1024,
                  "two workgroups a CU");
    VD_REQUIRE(ids && scores && bboxes && track, "vd_track_stitch: ids, scores, bboxes and track must not be NULL");
    VD_REQUIRE(out_track && out_len && out_score && out_stitches && out_overflow,
               "vd_track_stitch: the five output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_track_stitch: ws must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_track_stitch: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_track_stitch: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE((int64_t)F * N <= 0x7fffffff, "vd_track_stitch: F * N = %lld rows, at most 2^31 - 1 are taken", (long long)((int64_t)F * N));
    VD_REQUIRE(clip_start || V == 1, "vd_track_stitch: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1, "vd_track_stitch: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(max_gap >= 1 && max_gap <= kMaxStitchGap, "vd_track_stitch: max_gap=%d, 1 <= max_gap <= %d are taken", max_gap,
               kMaxStitchGap);
    VD_REQUIRE(sigma_iou == sigma_iou, "vd_track_stitch: sigma_iou must not be NaN");
    VD_REQUIRE(ws_bytes >= (int64_t)VD_TRACK_STITCH_WS_PER_ROW * F * N, "vd_track_stitch: ws_bytes=%lld, %d * F * N = %lld needed",
               (long long)ws_bytes, VD_TRACK_STITCH_WS_PER_ROW, (long long)((int64_t)VD_TRACK_STITCH_WS_PER_ROW * F * N));
    VD_REQUIRE(((uintptr_t)bboxes % 16) == 0, "vd_track_stitch: bboxes must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)clip_start | (uintptr_t)out_track |
                 (uintptr_t)out_len | (uintptr_t)out_score | (uintptr_t)out_stitches | (uintptr_t)out_overflow | (uintptr_t)ws) % 4) == 0,
               "vd_track_stitch: ids, scores, track, clip_start, the five outputs and ws must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (clip_start) {                                 // a frame that no clip covers comes out as rows of -1 / 0 / -1
        fill_uncovered<false>(s, (int64_t)F * N, out_track, out_len, out_score);
        VD_CHECK_LAUNCH("vd_track_stitch");
    }
    hipLaunchKernelGGL(k_track_stitch, dim3((unsigned)V), dim3(kThreads), 0, s, ids, scores, bboxes, track, clip_start, F, N,
                       num_class, max_gap, sigma_iou, out_track, out_len, out_score, out_stitches, out_overflow, ws);
    VD_CHECK_LAUNCH("vd_track_stitch");
    return VD_OK;
}

}  // extern "C"
