// vd_tubelet.hip — tubelet rescoring and gap filling over the tracks of video clips on the device (viddet_amd/tubelet.py is the
// definition): the rows of a track take the track's score, the frames a track skipped get an interpolated box,
// every frame is re-sorted.
//
// Arithmetic: fp32, operation for operation what tubelet_host does: no product and sum is contracted into an FMA, `/` is the
// correctly rounded division, the sum of a track's scores is accumulated in frame order from 0.
//
// Launches (the workspace, 24 bytes per (frame, row), carries everything from one to the next; a kernel boundary stands between
// every writer and the readers of another workgroup):
//   k_tub_clear    only with clip_start: every output as a frame that no clip covers has it (rows of -1, dropped 0)
//   k_tub_member   a workgroup per (clip, frame): a present row whose id is usable and that no lower row of its frame carries
//                  is the id's member in the frame - w_mem[row] is that id, else -1; the frame's N slots of the per-track tables
//                  (sum, count, last member) are reset, which covers the clip's slice [t0 * N, t1 * N) exactly
//   k_tub_chain    ONE workgroup per clip walks its frames in order, a thread per row: a member adds its score to its track's
//                  sum, raises the maximum, takes the track's last member as its predecessor (w_prev) and becomes the last
//                  member.  The ids of a frame's members differ, so no two threads of a frame touch one slot; a barrier stands
//                  between frames: the sum is in frame order by construction.  Then every track's score: sum / count, or the
//                  maximum
//   k_tub_frame    a workgroup per (clip, frame): the kept rows compacted in row order (two ballots); the fill candidates of the
//                  frame are the members of the next max_gap frames whose predecessor lies before this frame and at most
//                  max_gap + 1 frames back - a track has one such pair at most, so the candidates' ids differ and a candidate's
//                  rank is the number of smaller ids; kept + rank < N admits it; then the rank sort: an entry's output row is the
//                  number of entries with a larger score, or an equal one and a lower entry index (no score is a NaN: the
//                  members' scores are finite, sums and interpolations overflow to an infinity at most)
// A track id indexes the tables only after 0 <= id < (t1 - t0) * N has been checked, and the slice starts at t0 * N: whatever
// the table holds, nothing outside the workspace is read or written.  No atomics; plain vector loads and stores; the inputs are
// never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_clip_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxN = 128;
constexpr int kMaxGap = 7;
constexpr int kRowThreads = 128;                      // k_tub_member, k_tub_chain: a thread per row
constexpr int kFrameThreads = 256;                    // k_tub_frame
constexpr int kMaxCand = kMaxN * kMaxGap;
constexpr int kNone = 0x7fffffff;
constexpr int kMaxY = 128;                            // workgroups of a clip in the per-frame launches

struct Ws {
    int32_t* mem;                                     // [F*N] the id the row is a member of, -1: none
    int32_t* prev;                                    // [F*N] the row (t * N + i) of the track's member before this one, -1: first
    float* sum;                                       // per track, at t0 * N + id: the sum, after k_tub_chain the track's score
    int32_t* cnt;
    float* mx;
    int32_t* last;
};

__device__ inline Ws ws_of(void* ws, int64_t rows) {
    Ws w;
    w.mem = (int32_t*)ws;
    w.prev = w.mem + rows;
    w.sum = (float*)(w.prev + rows);
    w.cnt = (int32_t*)(w.sum + rows);
    w.mx = (float*)(w.cnt + rows);
    w.last = (int32_t*)(w.mx + rows);
    return w;
}

__global__ void k_tub_clear(int64_t rows, int F, float* __restrict__ out_ids, float* __restrict__ out_scores,
                            float* __restrict__ out_bboxes, int32_t* __restrict__ perm, int32_t* __restrict__ track_out,
                            int32_t* __restrict__ dropped) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        out_ids[i] = -1.f;
        out_scores[i] = -1.f;
        reinterpret_cast<float4*>(out_bboxes)[i] = make_float4(-1.f, -1.f, -1.f, -1.f);
        perm[i] = -1;
        track_out[i] = -1;
        if (i < F) dropped[i] = 0;
    }
}

__global__ __launch_bounds__(kRowThreads) void k_tub_member(const float* __restrict__ ids, const float* __restrict__ scores,
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
            w.sum[row] = 0.f;                         // slot t * N + i of the tables: the frames of the clip cover its slice
            w.cnt[row] = 0;
            w.last[row] = -1;
        }
        __syncthreads();                              // s_u before the next frame overwrites it
    }
}

__global__ __launch_bounds__(kRowThreads) void k_tub_chain(const float* __restrict__ scores, const int32_t* __restrict__ clip_start,
                                                           int F, int N, int rescore, void* ws) {
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    if (t0 >= t1) return;                             // the whole workgroup alike
    const Ws w = ws_of(ws, (int64_t)F * N);
    const int64_t first = (int64_t)t0 * N;
    float* t_sum = w.sum + first;
    int32_t* t_cnt = w.cnt + first;
    float* t_max = w.mx + first;
    int32_t* t_last = w.last + first;
    const int64_t slots = (int64_t)(t1 - t0) * N;     // the clip's ids: [0, slots)
    const int i = threadIdx.x;
    int u = -1;
    float s = 0.f;
    if (i < N) u = w.mem[first + i], s = scores[first + i];
    if (u >= slots) u = -1;                           // k_tub_member checked it; a launch of this kernel alone checks again
    for (int t = t0; t < t1; ++t) {
        const int64_t row = (int64_t)t * N + i;
        int nu = -1;                                  // the next frame's row, asked for ahead of this frame's chain of loads
        float ns = 0.f;
        if (i < N && t + 1 < t1) nu = w.mem[row + N], ns = scores[row + N];
        if (nu >= slots) nu = -1;
        if (u >= 0) {
            const int c = t_cnt[u];
            const float m = t_max[u];
            t_sum[u] = t_sum[u] + s;
            t_max[u] = (c == 0 || s > m) ? s : m;
            t_cnt[u] = c + 1;
            w.prev[row] = t_last[u];
            t_last[u] = (int)row;
        }
        __syncthreads();                              // this frame's tables before the next frame's members read them
        u = nu, s = ns;
    }
    if (rescore == 0) return;
    for (int64_t k = i; k < slots; k += kRowThreads) {
        const int c = t_cnt[k];
        if (c > 0) t_sum[k] = rescore == 1 ? t_sum[k] / (float)c : t_max[k];
    }
}

__global__ __launch_bounds__(kFrameThreads) void k_tub_frame(const float* __restrict__ ids, const float* __restrict__ scores,
                                                             const float* __restrict__ bboxes,
                                                             const int32_t* __restrict__ clip_start, int F, int N, int num_class,
                                                             int rescore, int max_gap, int drop_untracked,
                                                             float* __restrict__ out_ids, float* __restrict__ out_scores,
                                                             float* __restrict__ out_bboxes, int32_t* __restrict__ perm,
                                                             int32_t* __restrict__ track_out, int32_t* __restrict__ dropped,
                                                             const void* ws) {
    __shared__ int c_u[kMaxCand];                     // the fill candidates' ids, kNone where the slot holds none
    __shared__ int c_p[kMaxCand];                     // and the row of the member before the hole
    __shared__ float4 e_box[kMaxN];                   // the entries: kept rows, then admitted fills
    __shared__ float e_score[kMaxN];
    __shared__ float e_id[kMaxN];
    __shared__ int e_perm[kMaxN];
    __shared__ int e_trk[kMaxN];
    __shared__ int s_kept[2];
    __shared__ int s_cand;
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const Ws w = ws_of(const_cast<void*>(ws), (int64_t)F * N);
    const int64_t first = (int64_t)t0 * N;
    const int64_t limit = (int64_t)(t1 - t0) * N;     // an id read back from the workspace is checked again: a launch of this
                                                      // kernel alone (vd_tubelet_stages) meets whatever the workspace holds
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_slots = max_gap * N;                  // <= kMaxCand
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        const int64_t base = (int64_t)t * N;
        // the kept rows, in row order
        bool kept = false;
        int u = -1;
        float id = -1.f, sc = -1.f;
        if (tid < N) {
            id = ids[base + tid];
            sc = scores[base + tid];
            u = w.mem[base + tid];
            if (u >= limit) u = -1;
            kept = row_present(id, sc, num_class) && (!drop_untracked || u >= 0);
            if (u >= 0 && rescore != 0) sc = w.sum[first + u];
        }
        const unsigned long long votes = __ballot(kept);
        if (wave < 2 && lane == 0) s_kept[wave] = __popcll(votes);
        if (tid == 0) s_cand = 0;
        // the fill candidates: slot (j - 1) * N + i is row i of frame t + j
        for (int c = tid; c < n_slots; c += kFrameThreads) {
            const int j = c / N + 1, i = c - (j - 1) * N, f1 = t + j;
            int key = kNone, p = -1;
            if (f1 < t1) {
                const int64_t q = (int64_t)f1 * N + i;
                const int cu = w.mem[q];
                if (cu >= 0 && cu < limit) {
                    p = w.prev[q];
                    const int f0 = p >= 0 ? p / N : -1;
                    if (f0 >= t0 && f0 < t && f1 - f0 <= max_gap + 1) key = cu;
                }
            }
            c_u[c] = key;
            c_p[c] = p;
        }
        __syncthreads();
        const int n_kept = s_kept[0] + s_kept[1];
        if (kept) {
            const int e = (wave == 1 ? s_kept[0] : 0) + __popcll(votes & below);
            e_score[e] = sc;
            e_id[e] = id;
            e_box[e] = reinterpret_cast<const float4*>(bboxes)[base + tid];
            e_perm[e] = tid;
            e_trk[e] = u;
        }
        for (int c = tid; c < n_slots; c += kFrameThreads) {
            const int key = c_u[c];
            if (key == kNone) continue;
            int rank = 0, total = 0;
            for (int k = 0; k < n_slots; ++k) {
                const int o = c_u[k];
                rank += o < key;
                total += o != kNone;
            }
            if (rank == 0) s_cand = total;            // the lowest id's thread, one per frame
            if (n_kept + rank < N) {
                const int j = c / N + 1, i = c - (j - 1) * N;
                const int64_t q = (int64_t)(t + j) * N + i;
                const int p = c_p[c], f0 = p / N;
                const float wgt = (float)(t - f0) / (float)(t + j - f0);
                const float4 a = reinterpret_cast<const float4*>(bboxes)[p], b = reinterpret_cast<const float4*>(bboxes)[q];
                const int e = n_kept + rank;
                e_box[e] = make_float4(a.x + (b.x - a.x) * wgt, a.y + (b.y - a.y) * wgt, a.z + (b.z - a.z) * wgt,
                                       a.w + (b.w - a.w) * wgt);
                float s;
                if (rescore != 0) {
                    s = w.sum[first + key];
                } else {
                    const float sa = scores[p], sb = scores[q];
                    s = sa + (sb - sa) * wgt;
                }
                e_score[e] = s;
                e_id[e] = ids[p];
                e_perm[e] = -2;
                e_trk[e] = key;
            }
        }
        __syncthreads();
        const int n_cand = s_cand;
        const int room = N - n_kept;
        const int n = n_kept + (n_cand < room ? n_cand : room);
        if (tid == 0) dropped[t] = n_cand > room ? n_cand - room : 0;
        if (tid < N) {
            if (tid < n) {
                const float s = e_score[tid];
                int r = 0;
                for (int k = 0; k < n; ++k) {
                    const float o = e_score[k];
                    r += (o > s) || (o == s && k < tid);
                }
                out_ids[base + r] = e_id[tid];
                out_scores[base + r] = s;
                reinterpret_cast<float4*>(out_bboxes)[base + r] = e_box[tid];
                perm[base + r] = e_perm[tid];
                track_out[base + r] = e_trk[tid];
            } else {
                out_ids[base + tid] = -1.f;
                out_scores[base + tid] = -1.f;
                reinterpret_cast<float4*>(out_bboxes)[base + tid] = make_float4(-1.f, -1.f, -1.f, -1.f);
                perm[base + tid] = -1;
                track_out[base + tid] = -1;
            }
        }
        __syncthreads();                              // the entries and counts before the next frame overwrites them
    }
}

}  // namespace

extern "C" {

int64_t vd_tubelet_ws_bytes(int F, int N) {
    if (F < 1 || N < 1 || N > kMaxN || (int64_t)F * N > 0x7fffffff) return -1;
    return (int64_t)VD_TUBELET_WS_PER_ROW * F * N;
}

int vd_tubelet_stages(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start,
                      int V, int F, int N, int num_class, int rescore, int max_gap, int drop_untracked, float* out_ids,
                      float* out_scores, float* out_bboxes, int32_t* perm, int32_t* track_out, int32_t* dropped, void* ws,
                      int64_t ws_bytes, int stages, void* stream) {
    VD_REQUIRE(ids && scores && bboxes && track, "vd_tubelet: ids, scores, bboxes and track must not be NULL");
    VD_REQUIRE(out_ids && out_scores && out_bboxes && perm && track_out && dropped, "vd_tubelet: the six output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_tubelet: ws must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_tubelet: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_tubelet: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE((int64_t)F * N <= 0x7fffffff, "vd_tubelet: F * N = %lld rows, at most 2^31 - 1 are taken", (long long)((int64_t)F * N));
    VD_REQUIRE(clip_start || V == 1, "vd_tubelet: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1, "vd_tubelet: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(rescore >= 0 && rescore <= 2, "vd_tubelet: rescore=%d, 0 (none), 1 (avg) and 2 (max) are taken", rescore);
    VD_REQUIRE(max_gap >= 0 && max_gap <= kMaxGap, "vd_tubelet: max_gap=%d, 0 <= max_gap <= %d are taken", max_gap, kMaxGap);
    VD_REQUIRE(drop_untracked == 0 || drop_untracked == 1, "vd_tubelet: drop_untracked=%d, 0 and 1 are taken", drop_untracked);
    VD_REQUIRE(ws_bytes >= (int64_t)VD_TUBELET_WS_PER_ROW * F * N, "vd_tubelet: ws_bytes=%lld, %d * F * N = %lld needed",
               (long long)ws_bytes, VD_TUBELET_WS_PER_ROW, (long long)((int64_t)VD_TUBELET_WS_PER_ROW * F * N));
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)out_bboxes) % 16) == 0, "vd_tubelet: bboxes and out_bboxes must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)clip_start | (uintptr_t)out_ids |
                 (uintptr_t)out_scores | (uintptr_t)perm | (uintptr_t)track_out | (uintptr_t)dropped | (uintptr_t)ws) % 4) == 0,
               "vd_tubelet: ids, scores, track, clip_start, out_ids, out_scores, perm, track_out, dropped and ws must be 4-byte aligned");
    VD_REQUIRE(stages >= 1 && stages <= 15, "vd_tubelet: stages=%d, a mask of 1 (clear), 2 (members), 4 (chain), 8 (frames) is taken", stages);
    hipStream_t s = (hipStream_t)stream;
    if (clip_start && (stages & 1)) {                 // a frame that no clip covers comes out empty
        const int64_t n = (int64_t)F * N;
        const int64_t blocks = vd_cdiv(n, 256);
        hipLaunchKernelGGL(k_tub_clear, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, n, F, out_ids, out_scores,
                           out_bboxes, perm, track_out, dropped);
        VD_CHECK_LAUNCH("vd_tubelet");
    }
    const dim3 per_frame((unsigned)V, (unsigned)(F < kMaxY ? F : kMaxY));
    if (stages & 2)
        hipLaunchKernelGGL(k_tub_member, per_frame, dim3(kRowThreads), 0, s, ids, scores, track, clip_start, F, N, num_class, ws);
    VD_CHECK_LAUNCH("vd_tubelet");
    if (stages & 4)
        hipLaunchKernelGGL(k_tub_chain, dim3((unsigned)V), dim3(kRowThreads), 0, s, scores, clip_start, F, N, rescore, ws);
    VD_CHECK_LAUNCH("vd_tubelet");
    if (stages & 8)
        hipLaunchKernelGGL(k_tub_frame, per_frame, dim3(kFrameThreads), 0, s, ids, scores, bboxes, clip_start, F, N, num_class,
                           rescore, max_gap, drop_untracked, out_ids, out_scores, out_bboxes, perm, track_out, dropped,
                           (const void*)ws);
    VD_CHECK_LAUNCH("vd_tubelet");
    return VD_OK;
}

int vd_tubelet(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start, int V,
               int F, int N, int num_class, int rescore, int max_gap, int drop_untracked, float* out_ids, float* out_scores,
               float* out_bboxes, int32_t* perm, int32_t* track_out, int32_t* dropped, void* ws, int64_t ws_bytes, void* stream) {
    return vd_tubelet_stages(ids, scores, bboxes, track, clip_start, V, F, N, num_class, rescore, max_gap, drop_untracked, out_ids,
                             out_scores, out_bboxes, perm, track_out, dropped, ws, ws_bytes, 15, stream);
}

}  // extern "C"
