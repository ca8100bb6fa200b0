// vd_track_sort_app.hip — SORT with appearance association on the device (viddet_amd/appearance.py::app_sort_host is the
// definition): vd_track_sort.hip's tracker with one thing replaced, the cost of a cell.  A cell (candidate row i,
// active track k) of equal classes is admissible iff iou >= sigma_iou (`adm`) or iou >= sigma_prox and the cosine of the two
// int8 descriptors, on the 2^20 scale, reaches the threshold (`app`); it costs 2^20 - max(iou_q if adm, cos_q if app).  A
// track's descriptor is that of its most recent matched row that had one; a zero vector is no descriptor.  What app_sort_host
// computes, bit for bit, on all four outputs; with `emb` all zero, what vd_track_sort computes.
//
// Arithmetic: the filter and the IoU are vd_track_sort's, fp32, nothing contracted.  The dot product and the squared norms are
// exact integers - v_dot4_i32_i8, four int8 products a lane and instruction, accumulated in int32 (|dot| <= 1024 * 127^2): the
// i8 MFMA is exact too, but a cell needs its dot product only where it is `near` and both sides hold a descriptor, a few cells
// of a frame and no dense tile.  cos_q = floor(double(dot) * 2^20 / sqrt(double(na) * double(nb))), each float64 operation
// correctly rounded, all three integers exact in float64.
//
// One launch, ONE workgroup of 256 threads per clip walks its frames in order, as k_track_sort does; per frame
//   predict    as k_track_sort
//   cells      the workgroup strides over the R x K cells (candidate rows x active tracks, at most 128 x 1024) and writes each
//              cell's similarity - max(iou_q if adm, cos_q if app), -1 where it is forbidden - into the clip's int32 table in
//              the workspace, row pitch 1024
//   associate  assign_table (vd_track_assign.h): assign_host on the cells READ from the table, not formed again at every step
//   update     as k_track_sort; a matched track takes the flat index and squared norm of its row's descriptor where the row
//              has one - `emb` is never copied
//   start      as k_track_sort; the row's own descriptor or none
// Where things live.  LDS (59,528 bytes static): k_track_sort's arrays, the squared norm of every row of the frame, the
// descriptor row and squared norm of every active track.  Workspace: vd_track_sort's, then per clip the table of 128 x 1024
// int32 cells (512 KiB, it stays in L2).  Only this workgroup touches its clip's tables; a barrier (which orders global memory
// within the workgroup) stands between every writer and another thread's read.
// Every index read from memory is range-checked before it indexes anything; every loop is bounded by F, N, C, 1024 or
// N * (N + 1024).  No atomics; plain vector loads and stores; the inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"
#include "vd_track_kf.h"
#include "vd_track_assign.h"

namespace {

constexpr int kAppMinC = 8, kAppMaxC = 1024;
constexpr int64_t kTableBytes = (int64_t)kMaxN * kMaxActive * 4;

// the exact dot product of two int8 vectors of `words` 4-byte words
__device__ inline int dot_i8(const int* a, const int* b, int words) {
    int s = 0;
    for (int i = 0; i < words; ++i) s = __builtin_amdgcn_sdot4(a[i], b[i], s, false);
    return s;
}

__global__ __launch_bounds__(kThreads) void k_track_sort_app(const float* __restrict__ ids, const float* __restrict__ scores,
                                                             const float* __restrict__ bboxes, const int8_t* __restrict__ emb, int C,
                                                             const int32_t* __restrict__ clip_start, int F, int N, int num_class,
                                                             float sigma_l, float sigma_h, float sigma_iou, int t_min, int max_age,
                                                             float sigma_prox, int thr_app, int32_t* out_track, int32_t* out_len,
                                                             float* out_score, float4* out_tbox, void* ws, int64_t tab_off) {
    __shared__ float4 s_box[kMaxN];                   // this frame's rows
    __shared__ float s_score[kMaxN];
    __shared__ int s_cls[kMaxN];
    __shared__ int s_norm[kMaxN];                     // the squared norm of the row's descriptor, 0: none
    __shared__ int s_rg[kMaxN];                       // the candidate rows in row order: the assignment's rows
    __shared__ float4 a_pbox[kMaxActive];             // the active tracks, in order of creation: the predicted box,
    __shared__ int a_cls[kMaxActive];
    __shared__ int a_id[kMaxActive];
    __shared__ int a_miss[kMaxActive];
    __shared__ int a_len[kMaxActive];
    __shared__ float a_max[kMaxActive];
    __shared__ int a_desc[kMaxActive];                // the flat row (frame * N + row) of the track's descriptor, -1: none
    __shared__ int a_norm[kMaxActive];                // and its squared norm
    __shared__ int s_way[kMaxCols];
    __shared__ int s_rowof[kMaxCols];                 // the assignment row a column is matched to, -1: none
    __shared__ long long s_u[kMaxN];                  // the potentials of the assignment's rows
    __shared__ long long s_red_v[kWaves];
    __shared__ int s_red_j[kWaves];
    __shared__ int s_cnt[kTrackPer * kWaves];         // the survivors of every (pass, wavefront)
    __shared__ int s_cnt_row[2];                      // the candidates of rows 0 .. 63 and 64 .. 127
    __shared__ int s_cnt_new[2];                      // the candidates among them that start a track
    __shared__ int s_nact;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    if (t0 >= t1) return;                             // the whole workgroup alike
    const int64_t clip_rows = (int64_t)(t1 - t0) * N;
    const int64_t all_rows = (int64_t)F * N;
    int32_t* w_len = (int32_t*)ws + (int64_t)t0 * N;
    float* w_max = (float*)ws + (int64_t)F * N + (int64_t)t0 * N;
    float* st = (float*)ws + 2 * (int64_t)F * N + (int64_t)blockIdx.x * (2 * kStateFloats * kMaxActive);
    int32_t* tab = (int32_t*)((char*)ws + tab_off + (int64_t)blockIdx.x * kTableBytes);
    const int words = C >> 2;
    const int* ew = reinterpret_cast<const int*>(emb);
    const unsigned long long below = (1ull << lane) - 1ull;
    const float4 none = make_float4(-1.f, -1.f, -1.f, -1.f);

    if (tid == 0) s_nact = 0;
    int next_id = 0, cur = 0;                         // every thread alike
    for (int t = t0; t < t1; ++t) {
        const int64_t base = (int64_t)t * N;
        float* cs = st + cur * (kStateFloats * kMaxActive);
        float* ns = st + (cur ^ 1) * (kStateFloats * kMaxActive);
        // the frame's rows: thread r < N holds row r
        int my_cls = -1, my_norm = 0;
        float my_sc = 0.f;
        float4 my_box = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < N) {
            my_sc = scores[base + tid];
            my_box = reinterpret_cast<const float4*>(bboxes)[base + tid];
            my_cls = row_class(ids[base + tid], my_sc, num_class, sigma_l);
            if (my_cls >= 0) {
                const int* e = ew + (base + tid) * words;
                my_norm = dot_i8(e, e, words);
            }
        }
        if (tid < kMaxN) {
            s_box[tid] = my_box;
            s_score[tid] = my_sc;
            s_cls[tid] = my_cls;
            s_norm[tid] = my_norm;
        }
        const unsigned long long cvotes = __ballot(my_cls >= 0);       // wavefronts 2 and 3 hold no row
        if (lane == 0 && wave < 2) s_cnt_row[wave] = __popcll(cvotes);
        __syncthreads();                              // the rows; last frame's table and count
        int K = s_nact;
        if (K > kMaxActive) K = kMaxActive;
        const int R = s_cnt_row[0] + s_cnt_row[1];    // <= N
        int my_pool = -1;
        if (my_cls >= 0) {
            my_pool = (wave ? s_cnt_row[0] : 0) + __popcll(cvotes & below);
            s_rg[my_pool] = tid;
        }
        // predict
#pragma unroll
        for (int j = 0; j < kTrackPer; ++j) {
            const int k = tid + j * kThreads;
            if (k < K) {
                Kf s;
                kf_load(cs, k, s);
                kf_predict(s);
                kf_store(cs, k, s);
                a_pbox[k] = kf_box(s);
            }
        }
        __syncthreads();                              // the predicted boxes, the assignment's rows
        const bool assigned = R > 0 && K > 0;
        if (assigned) {
            // cells: assignment row i against track k, at tab[i * kMaxActive + k]
            const int cells = R * K;                  // <= 128 * 1024
            for (int cell = tid; cell < cells; cell += kThreads) {
                const int i = cell / K, k = cell - i * K;
                int g = s_rg[i];
                if (g < 0 || g >= kMaxN) g = 0;       // cannot be: the rows of this frame
                int sim = -1;
                if (a_cls[k] == s_cls[g]) {
                    const float q = iou(a_pbox[k], s_box[g]);
                    if (q >= sigma_iou) sim = (int)(q * 1048576.f);
                    const int na = s_norm[g], nb = a_norm[k], dr = a_desc[k];
                    if (q >= sigma_prox && na > 0 && nb > 0 && dr >= 0 && dr < all_rows) {
                        const int dot = dot_i8(ew + (base + g) * words, ew + (int64_t)dr * words, words);
                        int cq = 0;
                        if (dot > 0) cq = (int)floor((double)dot * 1048576.0 / sqrt((double)na * (double)nb));
                        if (cq >= thr_app && cq > sim) sim = cq;
                    }
                }
                tab[i * kMaxActive + k] = sim;
            }
            __syncthreads();                          // the cells
            assign_table(R, K, tab, kMaxActive, s_way, s_rowof, s_u, s_red_v, s_red_j, tid, lane, wave);
        }
        // update: every thread takes its tracks' words into registers; the survivors of every (pass, wavefront) are counted
        int u_id[kTrackPer], u_cls[kTrackPer], u_miss[kTrackPer], u_len[kTrackPer], u_row[kTrackPer], u_desc[kTrackPer],
            u_norm[kTrackPer];
        float u_max[kTrackPer];
        unsigned long long votes[kTrackPer];
#pragma unroll
        for (int j = 0; j < kTrackPer; ++j) {
            const int k = tid + j * kThreads;
            bool live = false;
            u_id[j] = u_cls[j] = u_miss[j] = u_len[j] = u_norm[j] = 0, u_row[j] = u_desc[j] = -1, u_max[j] = 0.f;
            if (k < K) {
                u_id[j] = a_id[k], u_cls[j] = a_cls[k], u_len[j] = a_len[k], u_max[j] = a_max[k];
                u_desc[j] = a_desc[k], u_norm[j] = a_norm[k];
                int g = -1;
                if (assigned) {
                    const int pr = s_rowof[k];
                    if (pr >= 0 && pr < R) g = s_rg[pr];
                    if (g < 0 || g >= N) g = -1;
                }
                u_row[j] = g;
                u_miss[j] = g >= 0 ? 0 : a_miss[k] + 1;
                live = u_miss[j] <= max_age;
            }
            votes[j] = __ballot(live);
            if (lane == 0) s_cnt[j * kWaves + wave] = __popcll(votes[j]);
        }
        // a candidate starts a track iff it took its dummy, or no assignment was made
        bool fresh = my_pool >= 0;
        if (fresh && assigned) fresh = s_rowof[K + my_pool] == my_pool;
        const unsigned long long fvotes = __ballot(fresh);
        if (lane == 0 && wave < 2) s_cnt_new[wave] = __popcll(fvotes);
        __syncthreads();                              // every word of the table is in a register; the counts
        int W = 0;
#pragma unroll
        for (int j = 0; j < kTrackPer; ++j) {
            const int k = tid + j * kThreads;
            int before = 0;                           // the survivors ahead of this (pass, wavefront)
#pragma unroll
            for (int e = 0; e < kTrackPer * kWaves; ++e) {
                const int n = s_cnt[e];
                if (e < j * kWaves + wave) before += n;
                if (j == 0) W += n;
            }
            if (k < K && ((votes[j] >> lane) & 1ull)) {
                const int pos = before + __popcll(votes[j] & below);   // <= k
                Kf s;
                kf_load(cs, k, s);
                const int g = u_row[j], id = u_id[j];
                if (g >= 0) {
                    float z[4];
                    kf_measure(s_box[g], z);
                    kf_update(s, z);
                    const float sc = s_score[g];
                    ++u_len[j];
                    if (sc > u_max[j]) u_max[j] = sc;
                    const int gn = s_norm[g];
                    if (gn > 0) u_desc[j] = (int)(base + g), u_norm[j] = gn;
                    out_track[base + g] = id;
                    out_tbox[base + g] = kf_box(s);
                    if (id >= 0 && id < clip_rows) w_len[id] = u_len[j], w_max[id] = u_max[j];
                }
                kf_store(ns, pos, s);
                a_cls[pos] = u_cls[j];
                a_id[pos] = id;
                a_miss[pos] = u_miss[j];
                a_len[pos] = u_len[j];
                a_max[pos] = u_max[j];
                a_desc[pos] = u_desc[j];
                a_norm[pos] = u_norm[j];
            }
        }
        // start: the fresh candidates in row order, behind the survivors
        const int n_new = s_cnt_new[0] + s_cnt_new[1];
        if (tid < N) {
            if (fresh) {
                const int rank = (wave ? s_cnt_new[0] : 0) + __popcll(fvotes & below);
                const int pos = W + rank, id = next_id + rank;
                float z[4];
                Kf s;
                kf_measure(my_box, z);
                kf_start(z, s);
                if (pos < kMaxActive) {               // always: W + n_new <= N * (max_age + 1)
                    kf_store(ns, pos, s);
                    a_cls[pos] = my_cls;
                    a_id[pos] = id;
                    a_miss[pos] = 0;
                    a_len[pos] = 1;
                    a_max[pos] = my_sc;
                    a_desc[pos] = my_norm > 0 ? (int)(base + tid) : -1;
                    a_norm[pos] = my_norm;
                }
                if (id < clip_rows) w_len[id] = 1, w_max[id] = my_sc;   // always: id < the rows of the clip so far
                out_track[base + tid] = id;
                out_tbox[base + tid] = kf_box(s);
            } else if (my_pool < 0) {                 // no candidate; a matched row is written by its track's thread
                out_track[base + tid] = -1;
                out_tbox[base + tid] = none;
            }
        }
        if (tid == 0) s_nact = W + n_new < kMaxActive ? W + n_new : kMaxActive;
        next_id += n_new;
        cur ^= 1;
        __syncthreads();                              // this frame's rows are read no more; the table and the states
    }
    // decide: a row keeps its id where its track's maximum >= sigma_h and its length >= t_min
    const int64_t first = (int64_t)t0 * N;
    for (int64_t i = tid; i < clip_rows; i += kThreads) {
        const int id = out_track[first + i];
        int len = 0;
        float mx = -1.f;
        bool keep = false;
        if (id >= 0 && id < clip_rows) {
            len = w_len[id];
            mx = w_max[id];
            keep = mx >= sigma_h && len >= t_min;
        }
        out_track[first + i] = keep ? id : -1;
        out_len[first + i] = keep ? len : 0;
        out_score[first + i] = keep ? mx : -1.f;
        if (!keep) out_tbox[first + i] = none;
    }
}

}  // namespace

extern "C" {

int64_t vd_track_sort_app_ws_bytes(int V, int F, int N) {
    const int64_t link = kalman_link_ws_bytes(V, F, N, kMaxN);
    return link < 0 ? -1 : link + kTableBytes * V;
}

int vd_track_sort_app(const float* ids, const float* scores, const float* bboxes, const int8_t* emb, int C, const int32_t* clip_start,
                      int V, int F, int N, int num_class, float sigma_l, float sigma_h, float sigma_iou, int t_min, int max_age,
                      float sigma_app, float sigma_prox, int32_t* out_track, int32_t* out_len, float* out_score, float* out_tbox,
                      void* ws, int64_t ws_bytes, void* stream) {
    static_assert(VD_TRACK_SORT_APP_WS_PER_CLIP == VD_TRACK_SORT_WS_PER_CLIP + kTableBytes, "two state tables and the cells per clip");
    const KalmanLinkArgs a = {"vd_track_sort_app", ids, scores, bboxes, clip_start, V, F, N, num_class, t_min, max_age, out_track,
                              out_len, out_score, out_tbox, ws, ws_bytes};
    if (const int e = kalman_link_rows(a, kMaxN)) return e;
    VD_REQUIRE(emb && ((uintptr_t)emb % 4) == 0, "vd_track_sort_app: emb must not be NULL and must be 4-byte aligned");
    VD_REQUIRE(C >= kAppMinC && C <= kAppMaxC && (C & (C - 1)) == 0, "vd_track_sort_app: C=%d, a power of two in [%d, %d] is taken", C,
               kAppMinC, kAppMaxC);
    VD_REQUIRE(sigma_l == sigma_l && sigma_h == sigma_h && sigma_iou == sigma_iou,
               "vd_track_sort_app: sigma_l, sigma_h and sigma_iou must not be NaN");
    VD_REQUIRE(sigma_app >= 0.f && sigma_app <= 1.f && sigma_prox >= 0.f && sigma_prox <= 1.f,
               "vd_track_sort_app: sigma_app=%g and sigma_prox=%g must lie in [0, 1]", (double)sigma_app, (double)sigma_prox);
    if (const int e = kalman_link_ws(a, kMaxN, kMaxAge)) return e;
    const int64_t link = kalman_link_ws_bytes(V, F, N, kMaxN), need = link + kTableBytes * V;
    VD_REQUIRE(ws_bytes >= need, "vd_track_sort_app: ws_bytes=%lld, %d * F * N + %d * V = %lld needed", (long long)ws_bytes,
               VD_TRACK_SORT_WS_PER_ROW, VD_TRACK_SORT_APP_WS_PER_CLIP, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    if (clip_start) {                                 // a frame that no clip covers comes out as rows of -1 / 0 / -1 / -1
        fill_uncovered<true>(s, (int64_t)F * N, out_track, out_len, out_score, out_tbox);
        VD_CHECK_LAUNCH("vd_track_sort_app");
    }
    const int thr_app = (int)(sigma_app * 1048576.f);
    hipLaunchKernelGGL(k_track_sort_app, dim3((unsigned)V), dim3(kThreads), 0, s, ids, scores, bboxes, emb, C, clip_start, F, N,
                       num_class, sigma_l, sigma_h, sigma_iou, t_min, max_age, sigma_prox, thr_app, out_track, out_len, out_score,
                       (float4*)out_tbox, ws, link);
    VD_CHECK_LAUNCH("vd_track_sort_app");
    return VD_OK;
}

}  // extern "C"
