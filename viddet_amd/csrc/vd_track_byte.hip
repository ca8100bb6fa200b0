// vd_track_byte.hip — the detections of video clips linked into tracks by BYTE on the device (viddet_amd/byte.py is the
// definition): Zhang et al., "ByteTrack: Multi-Object Tracking by Associating Every Detection Box" (ECCV 2022) -
// every active track predicted by SORT's constant-velocity Kalman filter (vd_track_kf.h), the predictions matched to the frame's
// HIGH-score rows by a minimum-cost assignment, then the tracks this left over and that were seen in the last frame matched to
// the LOW-score rows by a second one; a low-score row never starts a track.  What byte_host computes, bit for bit, on all four
// outputs.
//
// Arithmetic: fp32, operation for operation what byte_host does: no product and sum is contracted into an FMA, `/` and sqrtf
// are the correctly rounded ones (hipcc's default; the Makefile sets no fast-math flag), the IoU is vd_track_math.h's; `score >=
// sigma_l`, `score >= sigma_d`, `score >= sigma_new`, `iou >= sigma_iou`, `iou >= sigma_iou2`, `max >= sigma_h` the plain >=;
// q = int(iou * 2^20) is exact; the assignment is integers, its potentials and slacks int64.
//
// One launch, ONE workgroup of 256 threads per clip walks its frames in order; no communication between workgroups.  It is
// vd_track_sort.hip's kernel with another frame body.  Per frame:
//   rows       thread r < N holds row r; two ballots split the candidates into the high list (score >= sigma_d) and the low
//              list (every other candidate), both in row order
//   predict    a thread per active track (track k: thread k % 256): the 17-float state read, predicted, written back; the
//              predicted box into LDS
//   associate  twice, the same loop (`assign`, vd_track_assign.h: mot_metric.assign_host operation for operation, as k_track_sort does).
//              The passes differ in three things only: the row list (high, low), the threshold (sigma_iou, sigma_iou2) and the
//              columns' eligibility - all tracks in the first pass; in the second the tracks the first did not match whose miss
//              count was 0 on entry to the frame, a bit per column in the registers of the column's thread.  An ineligible
//              column stays where it is and every cell of it is forbidden, so the lowest-column tie rule sees byte_host's
//              order.  A pass is entered only when its list has a row and a track is active.  Between the passes every thread
//              takes what the first one decided for its tracks and its row into registers (the second pass reuses the LDS).
//   update     as k_track_sort: a thread per track; the track's row is the one of whichever pass matched it; the miss counts;
//              the survivors' new positions by ballots and a prefix count, order kept, the words held in registers across a
//              barrier
//   start      the high rows that took their dummy in the first pass (all of them where it was skipped) with score >=
//              sigma_new: two ballots, a prefix count gives every one its slot behind the survivors and its id
// Where things live.  LDS (51,344 bytes static, so three workgroups fit a CU's 160 KiB): k_track_sort's arrays and the second
// row list.  Workspace: as vd_track_sort's - the length and maximum of every track made, then per clip TWO tables of 17 x 1024
// state floats, field-major; the update reads a track's state from one table and writes it at its new position into the other,
// so no thread overwrites what another has yet to read.  Only this workgroup touches its clip's tables.  A barrier (which orders
// global memory within the workgroup) stands between every writer and another thread's read.
// Every index read from memory is range-checked before it indexes anything; every loop is bounded by F, N, 1024 or
// N * (N + 1024).  No atomics; plain vector loads and stores; the inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"
#include "vd_track_kf.h"
#include "vd_track_assign.h"

namespace {

__global__ __launch_bounds__(kThreads) void k_track_byte(const float* __restrict__ ids, const float* __restrict__ scores,
                                                         const float* __restrict__ bboxes, const int32_t* __restrict__ clip_start,
                                                         int F, int N, int num_class, float sigma_l, float sigma_d, float sigma_new,
                                                         float sigma_h, float sigma_iou, float sigma_iou2, int t_min, int max_age,
                                                         int32_t* out_track, int32_t* out_len, float* out_score, float4* out_tbox,
                                                         void* ws) {
    __shared__ float4 s_box[kMaxN];                   // this frame's rows
    __shared__ float s_score[kMaxN];
    __shared__ int s_cls[kMaxN];
    __shared__ int s_rg[kMaxN];                       // the high rows in row order: the first assignment's rows
    __shared__ int s_rg2[kMaxN];                      // the low rows in row order: the second assignment's
    __shared__ float4 a_pbox[kMaxActive];             // the active tracks, in order of creation: the predicted box,
    __shared__ int a_cls[kMaxActive];
    __shared__ int a_id[kMaxActive];
    __shared__ int a_miss[kMaxActive];
    __shared__ int a_len[kMaxActive];
    __shared__ float a_max[kMaxActive];
    __shared__ int s_way[kMaxCols];
    __shared__ int s_rowof[kMaxCols];                 // the assignment row a column is matched to, -1: none
    __shared__ long long s_u[kMaxN];                  // the potentials of the assignment's rows
    __shared__ long long s_red_v[kWaves];
    __shared__ int s_red_j[kWaves];
    __shared__ int s_cnt[kTrackPer * kWaves];         // the survivors of every (pass, wavefront)
    __shared__ int s_cnt_hi[2];                       // the high rows of rows 0 .. 63 and 64 .. 127
    __shared__ int s_cnt_lo[2];                       // the low rows
    __shared__ int s_cnt_new[2];                      // the high rows among them that start a track
    __shared__ int s_nact;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    if (t0 >= t1) return;                             // the whole workgroup alike
    // the clip's tracks: ids [0, (t1 - t0) * N), so its slice of the two per-track tables starts at its first row
    const int64_t clip_rows = (int64_t)(t1 - t0) * N;
    int32_t* w_len = (int32_t*)ws + (int64_t)t0 * N;
    float* w_max = (float*)ws + (int64_t)F * N + (int64_t)t0 * N;
    float* st = (float*)ws + 2 * (int64_t)F * N + (int64_t)blockIdx.x * (2 * kStateFloats * kMaxActive);
    const unsigned long long below = (1ull << lane) - 1ull;
    const float4 none = make_float4(-1.f, -1.f, -1.f, -1.f);

    if (tid == 0) s_nact = 0;
    int next_id = 0, cur = 0;                         // every thread alike
    for (int t = t0; t < t1; ++t) {
        const int64_t base = (int64_t)t * N;
        float* cs = st + cur * (kStateFloats * kMaxActive);
        float* ns = st + (cur ^ 1) * (kStateFloats * kMaxActive);
        // the frame's rows: thread r < N holds row r
        int my_cls = -1;
        float my_sc = 0.f;
        float4 my_box = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < N) {
            my_sc = scores[base + tid];
            my_box = reinterpret_cast<const float4*>(bboxes)[base + tid];
            my_cls = row_class(ids[base + tid], my_sc, num_class, sigma_l);
        }
        if (tid < kMaxN) {
            s_box[tid] = my_box;
            s_score[tid] = my_sc;
            s_cls[tid] = my_cls;
        }
        const bool is_high = my_cls >= 0 && my_sc >= sigma_d;          // a candidate's score is finite
        const bool is_low = my_cls >= 0 && !is_high;
        const unsigned long long hvotes = __ballot(is_high);           // wavefronts 2 and 3 hold no row
        const unsigned long long lvotes = __ballot(is_low);
        if (lane == 0 && wave < 2) s_cnt_hi[wave] = __popcll(hvotes), s_cnt_lo[wave] = __popcll(lvotes);
        __syncthreads();                              // the rows; last frame's table and count
        int K = s_nact;
        if (K > kMaxActive) K = kMaxActive;
        const int RH = s_cnt_hi[0] + s_cnt_hi[1];     // RH + RL <= N
        const int RL = s_cnt_lo[0] + s_cnt_lo[1];
        int my_pool = -1;                             // the row's place in its list
        if (is_high) {
            my_pool = (wave ? s_cnt_hi[0] : 0) + __popcll(hvotes & below);
            s_rg[my_pool] = tid;
        } else if (is_low) {
            my_pool = (wave ? s_cnt_lo[0] : 0) + __popcll(lvotes & below);
            s_rg2[my_pool] = tid;
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
        __syncthreads();                              // the predicted boxes, the two row lists
        // the first association: the high rows against every track
        const bool pass1 = RH > 0 && K > 0, pass2 = RL > 0 && K > 0;
        if (pass1)
            assign(s_rg, RH, K, sigma_iou, ~0u, s_box, s_cls, a_pbox, a_cls, s_way, s_rowof, s_u, s_red_v, s_red_j, tid, lane, wave);
        // what it decided, into registers: the row of each of this thread's tracks, whether this thread's row found a track; a
        // track is eligible for the second association iff it has no row yet and was seen in the last frame
        int u_row[kTrackPer];
        unsigned elig = 0u;
#pragma unroll
        for (int j = 0; j < kTrackPer; ++j) {
            const int k = tid + j * kThreads;
            u_row[j] = -1;
            if (k < K) {
                int g = -1;
                if (pass1) {
                    const int pr = s_rowof[k];
                    if (pr >= 0 && pr < RH) g = s_rg[pr];
                    if (g < 0 || g >= N) g = -1;
                }
                u_row[j] = g;
                if (g < 0 && a_miss[k] == 0) elig |= 1u << j;
            }
        }
        bool matched = false;                         // this thread's row has a track
        if (is_high && pass1) matched = s_rowof[K + my_pool] != my_pool;
        const bool fresh = is_high && !matched && my_sc >= sigma_new;
        // the second association: the low rows against the eligible tracks
        if (pass2) {
            __syncthreads();                          // the first one's s_rowof is read by now
            assign(s_rg2, RL, K, sigma_iou2, elig, s_box, s_cls, a_pbox, a_cls, s_way, s_rowof, s_u, s_red_v, s_red_j, tid, lane, wave);
            if (is_low) matched = s_rowof[K + my_pool] != my_pool;
        }
        // update: every thread takes its tracks' words into registers; the survivors of every (pass, wavefront) are counted
        int u_id[kTrackPer], u_cls[kTrackPer], u_miss[kTrackPer], u_len[kTrackPer];
        float u_max[kTrackPer];
        unsigned long long votes[kTrackPer];
#pragma unroll
        for (int j = 0; j < kTrackPer; ++j) {
            const int k = tid + j * kThreads;
            bool live = false;
            u_id[j] = u_cls[j] = u_miss[j] = u_len[j] = 0, u_max[j] = 0.f;
            if (k < K) {
                u_id[j] = a_id[k], u_cls[j] = a_cls[k], u_len[j] = a_len[k], u_max[j] = a_max[k];
                if (pass2 && ((elig >> j) & 1u)) {    // an eligible track has no row of the first pass
                    int g = -1;
                    const int pr = s_rowof[k];
                    if (pr >= 0 && pr < RL) g = s_rg2[pr];
                    if (g < 0 || g >= N) g = -1;
                    u_row[j] = g;
                }
                u_miss[j] = u_row[j] >= 0 ? 0 : a_miss[k] + 1;
                live = u_miss[j] <= max_age;
            }
            votes[j] = __ballot(live);
            if (lane == 0) s_cnt[j * kWaves + wave] = __popcll(votes[j]);
        }
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
            }
        }
        // start: the fresh high rows in row order, behind the survivors
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
                }
                if (id < clip_rows) w_len[id] = 1, w_max[id] = my_sc;   // always: id < the rows of the clip so far
                out_track[base + tid] = id;
                out_tbox[base + tid] = kf_box(s);
            } else if (!matched) {                    // no candidate, or one left alone; a matched row is written by its track's thread
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

int64_t vd_track_byte_ws_bytes(int V, int F, int N) { return kalman_link_ws_bytes(V, F, N, kMaxN); }

int vd_track_byte(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
                  int num_class, float sigma_l, float sigma_d, float sigma_new, float sigma_h, float sigma_iou, float sigma_iou2,
                  int t_min, int max_age, int32_t* out_track, int32_t* out_len, float* out_score, float* out_tbox, void* ws,
                  int64_t ws_bytes, void* stream) {
    static_assert(VD_TRACK_SORT_WS_PER_CLIP == 2 * kStateFloats * kMaxActive * 4, "two state tables per clip");
    const KalmanLinkArgs a = {"vd_track_byte", ids, scores, bboxes, clip_start, V, F, N, num_class, t_min, max_age, out_track, out_len,
                              out_score, out_tbox, ws, ws_bytes};
    if (const int e = kalman_link_rows(a, kMaxN)) return e;
    VD_REQUIRE(sigma_l == sigma_l && sigma_d == sigma_d && sigma_new == sigma_new && sigma_h == sigma_h && sigma_iou == sigma_iou &&
                   sigma_iou2 == sigma_iou2,
               "vd_track_byte: sigma_l, sigma_d, sigma_new, sigma_h, sigma_iou and sigma_iou2 must not be NaN");
    if (const int e = kalman_link_ws(a, kMaxN, kMaxAge)) return e;
    hipStream_t s = (hipStream_t)stream;
    if (clip_start) {                                 // a frame that no clip covers comes out as rows of -1 / 0 / -1 / -1
        fill_uncovered<true>(s, (int64_t)F * N, out_track, out_len, out_score, out_tbox);
        VD_CHECK_LAUNCH("vd_track_byte");
    }
    hipLaunchKernelGGL(k_track_byte, dim3((unsigned)V), dim3(kThreads), 0, s, ids, scores, bboxes, clip_start, F, N, num_class,
                       sigma_l, sigma_d, sigma_new, sigma_h, sigma_iou, sigma_iou2, t_min, max_age, out_track, out_len, out_score,
                       (float4*)out_tbox, ws);
    VD_CHECK_LAUNCH("vd_track_byte");
    return VD_OK;
}

}  // extern "C"
