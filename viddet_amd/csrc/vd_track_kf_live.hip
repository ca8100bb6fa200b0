// vd_track_kf_live.hip — the Kalman trackers of vd_track_sort.hip and vd_track_byte.hip in resumable form: vd_track_kf_push runs
// BYTE's frame body on the frames of one push and carries the active tracks - their words and their filter states - from launch
// to launch in a state block in HBM, so that a stream of frames that never says where it ends keeps its tracks
// (viddet_amd/byte.py::byte_online_host and viddet_amd/sort.py::sort_online_host are the definition).  One kernel
// serves both methods: with sigma_d = sigma_new = sigma_l every candidate is a high row that may start a track, the low list is
// empty, the second association is never entered, and what is left is sort_step operation for operation.
//
// Arithmetic: k_track_byte's, the same functions (vd_track_math.h, vd_track_kf.h, vd_track_assign.h): fp32, no product and sum
// contracted into an FMA, `/` and sqrtf the correctly rounded ones, the plain >= on every threshold, the assignment in integers.
// Nothing is decided on the device: per row the track's id (a creation number counted over the whole stream), its length so far,
// its maximum score so far and its posterior box come out; track.finalize_tracks makes sort_host's / byte_host's arrays of a
// finished clip from them.
//
// One launch, ONE workgroup of 256 threads per stream walks the stream's F frames in order; no communication between workgroups.
// The frame body is k_track_byte's, barrier for barrier: rows, predict, the two calls of `assign`, update, start (its head
// comment describes them).  What differs:
//   the state   a block of VD_TRACK_KF_STATE_BYTES per stream in place of the workspace:
//                 int32 n_active, next_id, cur, unused                                           16 bytes
//                 int32 class[1024], id[1024], misses[1024], length[1024], float maximum[1024]   20,480 bytes
//                 float table[2][17][1024], the filter states, field-major                        139,264 bytes
//               in order of creation, the first n_active entries live; table `cur` holds their filters.  All zero bytes are a
//               fresh stream.  At entry the words of the live tracks go to LDS (n_active clamped into [0, 1024] and cur into
//               {0, 1} before either indexes anything); the filter tables are used in place, as k_track_byte uses its
//               workspace: a frame reads table cur and writes the survivors at their new positions into the other.  At exit,
//               behind a barrier, the live words and the header are written back with plain vector stores.
//   the outputs per row, every element written: out_track, out_len and out_score SO FAR, out_tbox.  No decide pass, no
//               per-track length / maximum workspace, no clip_start: the input is [V][F][N], stream v owns frames
//               [v * F, (v + 1) * F).
// LDS: 51,344 bytes static, k_track_byte's arrays exactly (next_id and cur live in registers, every thread alike), so three
// workgroups fit a CU's 160 KiB.  Only this workgroup touches its stream's state.  A barrier (which orders global memory within
// the workgroup) stands between every writer and another thread's read.  n_active and cur are the only words of the state that
// index anything, and both are range-checked first; every loop is bounded by F, N, 1024 or N * (N + 1024).  No atomics; plain
// vector loads and stores; the inputs are never written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"
#include "vd_track_kf.h"
#include "vd_track_assign.h"

namespace {

constexpr int kHeaderBytes = 16;
constexpr int kWordBytes = 5 * 4 * kMaxActive;        // class, id, misses, length, maximum
constexpr int kTableFloats = kStateFloats * kMaxActive;

static_assert(VD_TRACK_KF_STATE_BYTES == kHeaderBytes + kWordBytes + 2 * kTableFloats * 4, "the state layout and the header disagree");
static_assert(VD_TRACK_KF_STATE_BYTES % 16 == 0, "every stream's block must stay 16-byte aligned");

__global__ __launch_bounds__(kThreads) void k_track_kf_push(const float* __restrict__ ids, const float* __restrict__ scores,
                                                            const float* __restrict__ bboxes, int F, int N, int num_class,
                                                            float sigma_l, float sigma_d, float sigma_new, float sigma_iou,
                                                            float sigma_iou2, int max_age, void* state, int32_t* out_track,
                                                            int32_t* out_len, float* out_score, float4* out_tbox) {
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
    const unsigned long long below = (1ull << lane) - 1ull;
    const float4 none = make_float4(-1.f, -1.f, -1.f, -1.f);

    // this stream's state
    char* blk = (char*)state + (int64_t)blockIdx.x * VD_TRACK_KF_STATE_BYTES;
    int32_t* g_hdr = (int32_t*)blk;
    int32_t* g_cls = (int32_t*)(blk + kHeaderBytes);
    int32_t* g_id = g_cls + kMaxActive;
    int32_t* g_miss = g_id + kMaxActive;
    int32_t* g_len = g_miss + kMaxActive;
    float* g_max = (float*)(g_len + kMaxActive);
    float* st = (float*)(blk + kHeaderBytes + kWordBytes);
    int n0 = g_hdr[0];
    n0 = n0 < 0 ? 0 : (n0 > kMaxActive ? kMaxActive : n0);        // before it indexes anything
    int next_id = g_hdr[1], cur = g_hdr[2] == 1 ? 1 : 0;          // every thread alike; cur is 0 or 1 whatever the word holds
    for (int i = tid; i < n0; i += kThreads) {
        a_cls[i] = g_cls[i];
        a_id[i] = g_id[i];
        a_miss[i] = g_miss[i];
        a_len[i] = g_len[i];
        a_max[i] = g_max[i];
    }
    if (tid == 0) s_nact = n0;

    const int64_t first = (int64_t)blockIdx.x * F * N;
    for (int t = 0; t < F; ++t) {
        const int64_t base = first + (int64_t)t * N;
        float* cs = st + cur * kTableFloats;
        float* ns = st + (cur ^ 1) * kTableFloats;
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
        __syncthreads();                              // the rows; the words just read, or last frame's table and count
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
                    out_len[base + g] = u_len[j];
                    out_score[base + g] = u_max[j];
                    out_tbox[base + g] = kf_box(s);
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
                if (pos < kMaxActive) {               // always from a state this kernel wrote: W + n_new <= N * (max_age + 1)
                    kf_store(ns, pos, s);
                    a_cls[pos] = my_cls;
                    a_id[pos] = id;
                    a_miss[pos] = 0;
                    a_len[pos] = 1;
                    a_max[pos] = my_sc;
                }
                out_track[base + tid] = id;
                out_len[base + tid] = 1;
                out_score[base + tid] = my_sc;
                out_tbox[base + tid] = kf_box(s);
            } else if (!matched) {                    // no candidate, or one left alone; a matched row is written by its track's thread
                out_track[base + tid] = -1;
                out_len[base + tid] = 0;
                out_score[base + tid] = -1.f;
                out_tbox[base + tid] = none;
            }
        }
        if (tid == 0) s_nact = W + n_new < kMaxActive ? W + n_new : kMaxActive;
        next_id += n_new;
        cur ^= 1;
        __syncthreads();                              // this frame's rows are read no more; the table and the states
    }
    __syncthreads();                                  // the table and the count before they are written back
    const int n1 = s_nact;                            // <= kMaxActive
    for (int i = tid; i < n1; i += kThreads) {
        g_cls[i] = a_cls[i];
        g_id[i] = a_id[i];
        g_miss[i] = a_miss[i];
        g_len[i] = a_len[i];
        g_max[i] = a_max[i];
    }
    if (tid == 0) g_hdr[0] = n1, g_hdr[1] = next_id, g_hdr[2] = cur, g_hdr[3] = 0;
}

}  // namespace

extern "C" {

int vd_track_kf_push(const float* ids, const float* scores, const float* bboxes, int V, int F, int N, int num_class, float sigma_l,
                     float sigma_d, float sigma_new, float sigma_iou, float sigma_iou2, int max_age, void* state,
                     int64_t state_bytes, int32_t* out_track, int32_t* out_len, float* out_score, float* out_tbox, void* stream) {
    VD_REQUIRE(ids && scores && bboxes, "vd_track_kf_push: ids, scores and bboxes must not be NULL");
    VD_REQUIRE(out_track && out_len && out_score && out_tbox, "vd_track_kf_push: the four output pointers must not be NULL");
    VD_REQUIRE(state, "vd_track_kf_push: state must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_track_kf_push: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_track_kf_push: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(num_class >= 1, "vd_track_kf_push: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(sigma_l == sigma_l && sigma_d == sigma_d && sigma_new == sigma_new && sigma_iou == sigma_iou && sigma_iou2 == sigma_iou2,
               "vd_track_kf_push: sigma_l, sigma_d, sigma_new, sigma_iou and sigma_iou2 must not be NaN");
    VD_REQUIRE(max_age >= 0 && max_age <= kMaxAge, "vd_track_kf_push: max_age=%d, 0 <= max_age <= %d are taken", max_age, kMaxAge);
    VD_REQUIRE(state_bytes >= (int64_t)VD_TRACK_KF_STATE_BYTES * V, "vd_track_kf_push: state_bytes=%lld, %d * V = %lld needed",
               (long long)state_bytes, VD_TRACK_KF_STATE_BYTES, (long long)((int64_t)VD_TRACK_KF_STATE_BYTES * V));
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)out_tbox | (uintptr_t)state) % 16) == 0,
               "vd_track_kf_push: bboxes, out_tbox and state must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)out_track | (uintptr_t)out_len | (uintptr_t)out_score) % 4) == 0,
               "vd_track_kf_push: ids, scores, out_track, out_len and out_score must be 4-byte aligned");
    hipLaunchKernelGGL(k_track_kf_push, dim3((unsigned)V), dim3(kThreads), 0, (hipStream_t)stream, ids, scores, bboxes, F, N,
                       num_class, sigma_l, sigma_d, sigma_new, sigma_iou, sigma_iou2, max_age, state, out_track, out_len, out_score,
                       (float4*)out_tbox);
    VD_CHECK_LAUNCH("vd_track_kf_push");
    return VD_OK;
}

}  // extern "C"
