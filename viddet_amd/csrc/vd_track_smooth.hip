// vd_track_smooth.hip — fixed-interval (Rauch-Tung-Striebel) smoothing of the boxes of video clips along their tracks on the
// device (viddet_amd/smooth.py is the definition): the forward pass is the Kalman filter of vd_track_kf.h, the
// backward pass carries the later frames' evidence back through every member of a segment.
//
// Arithmetic: fp32, operation for operation what smooth_host does: no product and sum is contracted into an FMA, `/` and sqrtf
// are the correctly rounded ones.
//
// Launches (the workspace, 80 bytes per (frame, row), carries everything from one to the next; a kernel boundary stands between
// every writer and the readers of another thread):
//   k_smo_clear    only with clip_start: every row as a frame that no clip covers has it (the input box, slen 0)
//   k_smo_member   a workgroup per (clip, frame): k_tub_member's rule - a present row whose id is usable and that no lower row of
//                  its frame carries is the id's member in the frame: w_mem[row] is that id, else -1
//   k_smo_link     a workgroup per (clip, frame), a thread per row, fully parallel: the member ids of the max_gap + 1 frames on
//                  either side are staged in LDS; a member's predecessor (w_prev) is the member of its id in the nearest earlier
//                  of them, its successor (w_next) the one in the nearest later of them, -1 where there is none.  The ids of a
//                  frame's members differ, so either is unique, and b is a's successor iff a is b's predecessor: the segments
//                  partition the members.  Every row of the frame gets its default output: the input box, slen 0
//   k_smo_seg      a thread per row; the thread of a segment's head (a member without predecessor) walks the successors forward
//                  - predict over the gap, update, the posterior state into the workspace (field-major, indexed by row) - and
//                  then back through the predecessors with the smoothed state in registers, writing sbox and slen.  The states
//                  a_j of a gap are recomputed from a_0 = the stored posterior (at most 36 predicts for the widest gap): no
//                  runtime-indexed local array.  Segments are independent: a clip of T frames is T dependent steps at most
// A row index read from the workspace is checked against the clip's rows [t0 * N, t1 * N) before it indexes anything, and a walk
// goes on only while the next member's frame is strictly later (forward) or strictly earlier (backward) and the gap is at most
// max_gap + 1: it is bounded by the clip's frames whatever the workspace holds.  No atomics; plain vector loads and stores; the
// inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_kf.h"
#include "vd_track_smooth_math.h"

namespace {

constexpr int kMaxGap = 7;
constexpr int kRowThreads = 128;                      // a thread per row
constexpr int kMaxY = 128;                            // workgroups of a clip in the per-frame launches
constexpr int kLinkFrames = 2 * (kMaxGap + 1) + 1;    // k_smo_link's window: the frame and max_gap + 1 on either side

struct Ws {
    int32_t* mem;                                     // [F*N] the id the row is a member of, -1: none
    int32_t* prev;                                    // [F*N] the row (t * N + i) of the segment's member before this one, -1: head
    int32_t* next;                                    // [F*N] and of the one after it, -1: the segment's last
    float* post;                                      // [17][F*N] the member's posterior state, field-major
};

__device__ inline Ws ws_of(void* ws, int64_t rows) {
    Ws w;
    w.mem = (int32_t*)ws;
    w.prev = w.mem + rows;
    w.next = w.prev + rows;
    w.post = (float*)(w.next + rows);
    return w;
}

// the 17-float state of row `row` in a field-major table of `rows` rows
__device__ inline void smo_load(const float* st, int64_t rows, int64_t row, Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.x[i] = st[(0 + i) * rows + row];
        s.xd[i] = st[(3 + i) * rows + row];
        s.p00[i] = st[(6 + i) * rows + row];
        s.p01[i] = st[(9 + i) * rows + row];
        s.p11[i] = st[(12 + i) * rows + row];
    }
    s.r = st[15 * rows + row];
    s.p = st[16 * rows + row];
}

__device__ inline void smo_store(float* st, int64_t rows, int64_t row, const Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        st[(0 + i) * rows + row] = s.x[i];
        st[(3 + i) * rows + row] = s.xd[i];
        st[(6 + i) * rows + row] = s.p00[i];
        st[(9 + i) * rows + row] = s.p01[i];
        st[(12 + i) * rows + row] = s.p11[i];
    }
    st[15 * rows + row] = s.r;
    st[16 * rows + row] = s.p;
}

__global__ void k_smo_clear(int64_t rows, const float* __restrict__ bboxes, float* __restrict__ out_sbox,
                            int32_t* __restrict__ out_slen) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        reinterpret_cast<float4*>(out_sbox)[i] = reinterpret_cast<const float4*>(bboxes)[i];
        out_slen[i] = 0;
    }
}

__global__ __launch_bounds__(kRowThreads) void k_smo_member(const float* __restrict__ ids, const float* __restrict__ scores,
                                                            const int32_t* __restrict__ track,
                                                            const int32_t* __restrict__ clip_start, int F, int N, int num_class,
                                                            void* ws) {
    __shared__ int s_u[kMaxN];
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const Ws w = ws_of(ws, (int64_t)F * N);
    const int64_t limit = (int64_t)(t1 - t0) * N;     // the clip's ids: [0, limit)
    const int i = threadIdx.x;
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        const int64_t row = (int64_t)t * N + i;
        int u = -1;
        if (i < N) {
            const int id = track[row];
            if (row_present(ids[row], scores[row], num_class) && id >= 0 && id < limit) u = id;
            s_u[i] = u;
        }
        __syncthreads();
        if (i < N) {
            if (u >= 0)
                for (int j = 0; j < i; ++j)
                    if (s_u[j] == u) {                // a lower row of the frame carries the id
                        u = -1;
                        break;
                    }
            w.mem[row] = u;
        }
        __syncthreads();                              // s_u before the next frame overwrites it
    }
}

__global__ __launch_bounds__(kRowThreads) void k_smo_link(const float* __restrict__ bboxes, const int32_t* __restrict__ clip_start,
                                                          int F, int N, int max_gap, float* __restrict__ out_sbox,
                                                          int32_t* __restrict__ out_slen, void* ws) {
    __shared__ int s_mem[kLinkFrames * kMaxN];        // slot (f - (t - W)) * N + i: the member id of row i of frame f, -1: none
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const Ws w = ws_of(ws, (int64_t)F * N);
    const int W = max_gap + 1;                        // <= kMaxGap + 1
    const int i = threadIdx.x;
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        for (int c = i; c < (2 * W + 1) * N; c += kRowThreads) {
            const int d = c / N, f = t - W + d;
            s_mem[c] = (f >= t0 && f < t1) ? w.mem[(int64_t)f * N + (c - d * N)] : -1;
        }
        __syncthreads();
        if (i < N) {
            const int64_t row = (int64_t)t * N + i;
            const int u = s_mem[W * N + i];
            int prev = -1, next = -1;
            if (u >= 0) {
                for (int d = 1; d <= W && prev < 0; ++d)
                    for (int j = 0; j < N; ++j)
                        if (s_mem[(W - d) * N + j] == u) {
                            prev = (t - d) * N + j;
                            break;
                        }
                for (int d = 1; d <= W && next < 0; ++d)
                    for (int j = 0; j < N; ++j)
                        if (s_mem[(W + d) * N + j] == u) {
                            next = (t + d) * N + j;
                            break;
                        }
            }
            w.prev[row] = prev;
            w.next[row] = next;
            reinterpret_cast<float4*>(out_sbox)[row] = reinterpret_cast<const float4*>(bboxes)[row];
            out_slen[row] = 0;
        }
        __syncthreads();                              // s_mem before the next frame overwrites it
    }
}

__global__ __launch_bounds__(kRowThreads) void k_smo_seg(const float* __restrict__ bboxes, const int32_t* __restrict__ clip_start,
                                                         int F, int N, int max_gap, float* __restrict__ out_sbox,
                                                         int32_t* __restrict__ out_slen, void* ws) {
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const int64_t rows = (int64_t)F * N;
    const Ws w = ws_of(ws, rows);
    const int64_t lo = (int64_t)t0 * N, hi = (int64_t)t1 * N;      // the clip's rows: [lo, hi)
    const int W = max_gap + 1;
    const int i = threadIdx.x;
    if (i >= N) return;                               // no barrier in this kernel
    const float4* box = reinterpret_cast<const float4*>(bboxes);
    float4* sbox = reinterpret_cast<float4*>(out_sbox);
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        const int64_t head = (int64_t)t * N + i;
        if (w.mem[head] < 0 || w.prev[head] >= 0) continue;       // a segment's head only
        // forward: the posterior of every member into the workspace
        Kf s;
        float z[4];
        kf_measure(box[head], z);
        kf_start(z, s);
        smo_store(w.post, rows, head, s);
        int64_t cur = head;
        int f_cur = t, n = 1;
        for (;;) {
            const int64_t nx = w.next[cur];
            if (nx < lo || nx >= hi) break;
            const int f_nx = (int)(nx / N);
            const int g = f_nx - f_cur;
            if (g < 1 || g > W) break;                // strictly later, and no wider than a segment's gap
            for (int j = 0; j < g; ++j) kf_predict(s);
            kf_measure(box[nx], z);
            kf_update(s, z);
            smo_store(w.post, rows, nx, s);
            cur = nx, f_cur = f_nx, ++n;
        }
        out_slen[head] = n;
        if (n == 1) continue;                         // it keeps its input box (k_smo_link wrote it)
        // backward: `s` is the last member's posterior
        Sm S;
#pragma unroll
        for (int k = 0; k < 3; ++k) S.x[k] = s.x[k], S.xd[k] = s.xd[k];
        S.r = s.r;
        {
            const float4 b = kf_box(s);
            if (finite4(b)) sbox[cur] = b;
            if (cur != head) out_slen[cur] = n;
        }
        for (int step = 1; step < n; ++step) {        // n - 1 predecessors, as the forward walk counted them
            const int64_t pv = w.prev[cur];
            if (pv < lo || pv >= hi) break;
            const int f_pv = (int)(pv / N);
            const int g = f_cur - f_pv;
            if (g < 1 || g > W) break;                // strictly earlier
            Kf a0;
            smo_load(w.post, rows, pv, a0);
            for (int j = g - 1; j >= 0; --j) {
                Kf f = a0;
                for (int q = 0; q < j; ++q) kf_predict(f);
                Kf p = f;
                kf_predict(p);
                smo_back(S, f, p);
            }
            Kf o;                                     // kf_box reads x and r only
#pragma unroll
            for (int k = 0; k < 3; ++k) o.x[k] = S.x[k], o.xd[k] = 0.f, o.p00[k] = 0.f, o.p01[k] = 0.f, o.p11[k] = 0.f;
            o.r = S.r, o.p = 0.f;
            const float4 b = kf_box(o);
            if (finite4(b)) sbox[pv] = b;
            out_slen[pv] = n;
            cur = pv, f_cur = f_pv;
        }
    }
}

}  // namespace

extern "C" {

int64_t vd_track_smooth_ws_bytes(int F, int N) {
    if (F < 1 || N < 1 || N > kMaxN || (int64_t)F * N > 0x7fffffff) return -1;
    return (int64_t)VD_TRACK_SMOOTH_WS_PER_ROW * F * N;
}

int vd_track_smooth_stages(const float* ids, const float* scores, const float* bboxes, const int32_t* track,
                           const int32_t* clip_start, int V, int F, int N, int num_class, int max_gap, float* out_sbox,
                           int32_t* out_slen, void* ws, int64_t ws_bytes, int stages, void* stream) {
    static_assert(VD_TRACK_SMOOTH_WS_PER_ROW == 3 * 4 + kStateFloats * 4, "the workspace: mem, prev, next and a 17-float state a row");
    VD_REQUIRE(ids && scores && bboxes && track, "vd_track_smooth: ids, scores, bboxes and track must not be NULL");
    VD_REQUIRE(out_sbox && out_slen, "vd_track_smooth: the two output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_track_smooth: ws must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_track_smooth: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_track_smooth: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE((int64_t)F * N <= 0x7fffffff, "vd_track_smooth: F * N = %lld rows, at most 2^31 - 1 are taken", (long long)((int64_t)F * N));
    VD_REQUIRE(clip_start || V == 1, "vd_track_smooth: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1, "vd_track_smooth: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(max_gap >= 0 && max_gap <= kMaxGap, "vd_track_smooth: max_gap=%d, 0 <= max_gap <= %d are taken", max_gap, kMaxGap);
    VD_REQUIRE(ws_bytes >= (int64_t)VD_TRACK_SMOOTH_WS_PER_ROW * F * N, "vd_track_smooth: ws_bytes=%lld, %d * F * N = %lld needed",
               (long long)ws_bytes, VD_TRACK_SMOOTH_WS_PER_ROW, (long long)((int64_t)VD_TRACK_SMOOTH_WS_PER_ROW * F * N));
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)out_sbox) % 16) == 0, "vd_track_smooth: bboxes and out_sbox must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)clip_start | (uintptr_t)out_slen |
                 (uintptr_t)ws) % 4) == 0,
               "vd_track_smooth: ids, scores, track, clip_start, out_slen and ws must be 4-byte aligned");
    VD_REQUIRE(stages >= 1 && stages <= 15, "vd_track_smooth: stages=%d, a mask of 1 (clear), 2 (members), 4 (links), 8 (segments) is taken", stages);
    hipStream_t s = (hipStream_t)stream;
    if (clip_start && (stages & 1)) {                                 // a frame that no clip covers keeps its input boxes
        const int64_t n = (int64_t)F * N;
        const int64_t blocks = vd_cdiv(n, 256);
        hipLaunchKernelGGL(k_smo_clear, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, n, bboxes, out_sbox,
                           out_slen);
        VD_CHECK_LAUNCH("vd_track_smooth");
    }
    const dim3 per_frame((unsigned)V, (unsigned)(F < kMaxY ? F : kMaxY));
    if (stages & 2)
        hipLaunchKernelGGL(k_smo_member, per_frame, dim3(kRowThreads), 0, s, ids, scores, track, clip_start, F, N, num_class, ws);
    VD_CHECK_LAUNCH("vd_track_smooth");
    if (stages & 4)
        hipLaunchKernelGGL(k_smo_link, per_frame, dim3(kRowThreads), 0, s, bboxes, clip_start, F, N, max_gap, out_sbox, out_slen, ws);
    VD_CHECK_LAUNCH("vd_track_smooth");
    if (stages & 8)
        hipLaunchKernelGGL(k_smo_seg, per_frame, dim3(kRowThreads), 0, s, bboxes, clip_start, F, N, max_gap, out_sbox, out_slen, ws);
    VD_CHECK_LAUNCH("vd_track_smooth");
    return VD_OK;
}

int vd_track_smooth(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start,
                    int V, int F, int N, int num_class, int max_gap, float* out_sbox, int32_t* out_slen, void* ws, int64_t ws_bytes,
                    void* stream) {
    return vd_track_smooth_stages(ids, scores, bboxes, track, clip_start, V, F, N, num_class, max_gap, out_sbox, out_slen, ws,
                                  ws_bytes, 15, stream);
}

}  // extern "C"
