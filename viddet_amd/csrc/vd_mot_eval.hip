// vd_mot_eval.hip — the per-frame matching of the MOT tracking metric on the device (viddet_amd/mot_metric.py is the definition,
// DESIGN.md 33): ground-truth rows against tracked prediction rows, frame by frame, with the CLEAR MOT carry-over and a
// minimum-cost assignment of the rest.  What mot_match_host computes, bit for bit, on all four outputs.
//
// Arithmetic: the IoU is vd_seq_nms.hip's fp32 one (no product and sum is contracted into an FMA, `/` is the correctly rounded
// division), `iou >= iou_thresh` the plain >=; q = int(iou * 2^20) is exact; everything else is integers, the assignment's
// potentials and slacks int64.
//
// Launches (the workspace, 4 bytes per (frame, row) of either side, carries the candidate tables from the second to the third; a
// kernel boundary stands between every writer and the readers of another workgroup):
//   k_mot_clear   only with clip_start: every output as a frame that no clip covers has it (-2 / 0 / 0 / 0)
//   k_mot_pairs   a workgroup per (clip, frame): the candidate rows of both sides as in k_tub_member (a compare loop, no
//                 atomics) - w_g[row] / w_p[row] is the candidate's id, else -1 -, then the admissible pairs: a thread per pair, a
//                 wavefront per 64 prediction rows of a ground-truth row, its ballot is two words of adm
//   k_mot_assign  ONE workgroup per clip walks its frames in order, the next frame's rows loaded ahead; last[1024] stays in LDS
//                 for the whole clip.  Per frame: the carry-over (a thread per ground-truth row finds the row that carries its
//                 last id; of several that want one prediction row the lowest admissible takes it - a compare loop), the two
//                 pools compacted by ballots, then assign_host operation for operation: a thread per column (the pool's
//                 prediction rows, then a dummy per ground-truth row), per step the slack of every column against the row at
//                 the tree's tip, the workgroup's minimum over (slack, column), the update of potentials and slacks; the
//                 augmenting path is walked by one thread.  The cost of a cell is formed again from the boxes where it is read
//                 (a division a step; a 128 x 128 tile of them would be the only LDS array of size).  Entered only when both
//                 pools hold a row.  Then the records, and last[] takes the matched ids.
// Every id read from memory is range-checked before it indexes anything: a ground-truth id indexes last[] only after
// 0 <= id < 1024 (checked again where it is read back from the workspace); a prediction's track id is only ever compared.  Every
// loop is bounded by F, G, N or G * (G + N).  No atomics; plain vector loads and stores; the inputs are never written; every
// output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"

namespace {

constexpr int kMaxRows = 128;                         // G and N
constexpr int kThreads = 256;                         // both kernels: 4 wavefronts; the assignment's columns: G + N at most
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxGtId = 1024;
constexpr int kMaxY = 128;                            // workgroups of a clip in k_mot_pairs
constexpr long long kInf = 1ll << 62;                 // a forbidden cell, a column that no path reaches
constexpr long long kDummy = 1ll << 27;
constexpr int kQOne = 1 << 20;

__global__ void k_mot_clear(int64_t rows, int32_t* __restrict__ match, float* __restrict__ miou, int32_t* __restrict__ flags,
                            uint32_t* __restrict__ adm) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        match[i] = -2;
        miou[i] = 0.f;
        flags[i] = 0;
        reinterpret_cast<uint4*>(adm)[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(kThreads) void k_mot_pairs(const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_cls,
                                                        const int32_t* __restrict__ gt_id, const float* __restrict__ ids,
                                                        const float* __restrict__ scores, const float* __restrict__ bboxes,
                                                        const int32_t* __restrict__ track, const int32_t* __restrict__ clip_start,
                                                        int F, int G, int N, int num_class, float thr, int agnostic,
                                                        uint32_t* __restrict__ adm, int32_t* __restrict__ w_g,
                                                        int32_t* __restrict__ w_p) {
    __shared__ float4 s_box[2 * kMaxRows];            // the ground-truth rows, then the prediction rows
    __shared__ int s_cls[2 * kMaxRows];
    __shared__ int s_el[2 * kMaxRows];                // the id of an eligible row, else -1
    __shared__ int s_cand[2 * kMaxRows];              // the id of a candidate row, else -1
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const bool pred = tid >= kMaxRows;                // threads 0 .. 127: a ground-truth row each; 128 .. 255: a prediction row
    const int r = pred ? tid - kMaxRows : tid;
    const bool have = r < (pred ? N : G);
    const int first = pred ? kMaxRows : 0;            // the side's first slot
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        int el = -1, cls = -1;
        float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have) {
            if (pred) {
                const int64_t row = (int64_t)t * N + r;
                box = reinterpret_cast<const float4*>(bboxes)[row];
                cls = row_class(ids[row], scores[row], num_class);
                const int u = track[row];
                if (cls >= 0 && u >= 0) el = u;
            } else {
                const int64_t row = (int64_t)t * G + r;
                box = reinterpret_cast<const float4*>(gt_boxes)[row];
                cls = gt_cls[row];
                const int a = gt_id[row];
                if (cls >= 0 && a >= 0 && a < kMaxGtId) el = a;
            }
        }
        s_box[tid] = box;
        s_cls[tid] = cls;
        s_el[tid] = el;
        __syncthreads();
        int cand = el;
        if (cand >= 0)
            for (int k = 0; k < r; ++k)
                if (s_el[first + k] == cand) {        // a lower eligible row of the frame carries the id
                    cand = -1;
                    break;
                }
        s_cand[tid] = cand;
        if (have) (pred ? w_p : w_g)[(int64_t)t * (pred ? N : G) + r] = cand;
        __syncthreads();
        // the admissible pairs: wavefronts 0, 1 hold row g0, wavefronts 2, 3 row g0 + 1; a wavefront 64 prediction rows
        const int j = tid & (kMaxRows - 1);
        const float4 pb = s_box[kMaxRows + j];
        const int pc = s_cls[kMaxRows + j];
        const bool pok = j < N && s_cand[kMaxRows + j] >= 0;
        for (int g0 = 0; g0 < G; g0 += 2) {
            const int g = g0 + (wave >> 1);           // wavefront-uniform
            bool ok = false;
            if (g < G && pok && s_cand[g] >= 0 && (agnostic || s_cls[g] == pc)) ok = iou(s_box[g], pb) >= thr;
            const unsigned long long votes = __ballot(ok);
            if (g < G && lane == 0) {
                uint32_t* out = adm + ((int64_t)t * G + g) * 4 + (wave & 1) * 2;
                out[0] = (uint32_t)votes;
                out[1] = (uint32_t)(votes >> 32);
            }
        }
        __syncthreads();                              // the rows before the next frame overwrites them
    }
}

__global__ __launch_bounds__(kThreads) void k_mot_assign(const float* __restrict__ gt_boxes, const float* __restrict__ bboxes,
                                                         const int32_t* __restrict__ clip_start, int F, int G, int N,
                                                         const uint32_t* __restrict__ adm, const int32_t* __restrict__ w_g,
                                                         const int32_t* __restrict__ w_p, int32_t* __restrict__ match,
                                                         float* __restrict__ miou, int32_t* __restrict__ flags) {
    __shared__ float4 s_gbox[kMaxRows];
    __shared__ float4 s_pbox[kMaxRows];
    __shared__ int s_gid[kMaxRows];                   // the candidate's ground-truth id, -1: no candidate
    __shared__ int s_pid[kMaxRows];                   // the candidate's track id, -1: no candidate
    __shared__ uint32_t s_adm[kMaxRows * 4];
    __shared__ int s_last[kMaxGtId];                  // the prediction id a ground-truth id was matched to last, -1: none
    __shared__ int s_want[kMaxRows];
    __shared__ int s_match[kMaxRows];
    __shared__ int s_carry[kMaxRows];
    __shared__ int s_taken[kMaxRows];
    __shared__ int s_rg[kMaxRows];                    // the pools: ground-truth rows, prediction rows, in row order
    __shared__ int s_cp[kMaxRows];
    __shared__ int s_cnt[kWaves];
    __shared__ long long s_u[kMaxRows];               // the potentials of the pool's ground-truth rows
    __shared__ int s_way[kThreads];
    __shared__ int s_rowof[kThreads];                 // the pool row a column is matched to, -1: none
    __shared__ long long s_red_v[kWaves];
    __shared__ int s_red_j[kWaves];
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    if (t0 >= t1) return;                             // the whole workgroup alike
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = tid; k < kMaxGtId; k += kThreads) s_last[k] = -1;
    const int words = G * 4;                          // of adm, per frame: <= 512, two a thread
    // the first frame's rows; inside the loop the next frame's, asked for ahead of this frame's work
    float4 n_gbox = make_float4(0.f, 0.f, 0.f, 0.f), n_pbox = n_gbox;
    int n_gid = -1, n_pid = -1;
    uint32_t n_adm[2] = {0u, 0u};
    auto load = [&](int t) {
        if (tid < G) {
            n_gbox = reinterpret_cast<const float4*>(gt_boxes)[(int64_t)t * G + tid];
            n_gid = w_g[(int64_t)t * G + tid];
        }
        if (tid < N) {
            n_pbox = reinterpret_cast<const float4*>(bboxes)[(int64_t)t * N + tid];
            n_pid = w_p[(int64_t)t * N + tid];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (tid + h * kThreads < words) n_adm[h] = adm[(int64_t)t * words + tid + h * kThreads];
    };
    load(t0);
    for (int t = t0; t < t1; ++t) {
        if (tid < kMaxRows) {
            s_gbox[tid] = n_gbox;
            s_pbox[tid] = n_pbox;
            // read back from the workspace: checked again before anything is indexed with it
            s_gid[tid] = (tid < G && n_gid >= 0 && n_gid < kMaxGtId) ? n_gid : -1;
            s_pid[tid] = (tid < N && n_pid >= 0) ? n_pid : -1;
            s_taken[tid] = 0;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (tid + h * kThreads < words) s_adm[tid + h * kThreads] = n_adm[h];
        __syncthreads();
        if (t + 1 < t1) load(t + 1);
        // the carry-over: the row that carries the id this ground-truth id was matched to last
        const int a = tid < kMaxRows ? s_gid[tid] : -1;
        int want = -1;
        if (a >= 0) {
            const int p = s_last[a];
            if (p >= 0)
                for (int j = 0; j < N; ++j)
                    if (s_pid[j] == p) {              // the candidates' ids differ: one row at most
                        if ((s_adm[tid * 4 + (j >> 5)] >> (j & 31)) & 1u) want = j;
                        break;
                    }
        }
        if (tid < kMaxRows) s_want[tid] = want;
        __syncthreads();
        if (tid < kMaxRows) {
            bool won = want >= 0;
            if (won)
                for (int k = 0; k < tid; ++k)
                    if (s_want[k] == want) {          // a lower ground-truth row took the prediction row
                        won = false;
                        break;
                    }
            s_match[tid] = won ? want : (a >= 0 ? -1 : -2);
            s_carry[tid] = won;
            if (won) s_taken[want] = 1;
        }
        __syncthreads();
        // the pools: wavefronts 0, 1 the ground-truth rows left, wavefronts 2, 3 the prediction rows left
        const int r = tid & (kMaxRows - 1);
        const bool in_pool = tid < kMaxRows ? (s_gid[r] >= 0 && s_match[r] == -1) : (s_pid[r] >= 0 && !s_taken[r]);
        const unsigned long long votes = __ballot(in_pool);
        if (lane == 0) s_cnt[wave] = __popcll(votes);
        __syncthreads();
        if (in_pool) (tid < kMaxRows ? s_rg : s_cp)[((wave & 1) ? s_cnt[wave - 1] : 0) + __popcll(votes & below)] = r;
        const int R = s_cnt[0] + s_cnt[1], P = s_cnt[2] + s_cnt[3];
        __syncthreads();
        if (R > 0 && P > 0) {
            // assign_host: column c < P is prediction row s_cp[c], column P + r the dummy of pool row r
            const int C = P + R;
            const int c = tid;
            const bool col = c < C;
            const int my_j = c < P ? s_cp[c] : 0;
            const float4 pb = s_pbox[my_j];
            long long v = 0;
            s_rowof[c] = -1;
            if (c < R) s_u[c] = 0;
            __syncthreads();
            for (int i = 0; i < R; ++i) {
                long long minv = kInf;
                bool used = false;
                s_way[c] = -1;
                int i0 = i, j0 = -1;
                for (int step = 0; step <= R; ++step) {              // a path visits a matched column once: i + 1 steps at most
                    const int g = s_rg[i0];
                    const long long ui = s_u[i0];
                    if (col && !used) {
                        long long cst = kInf;
                        if (c < P) {
                            if ((s_adm[g * 4 + (my_j >> 5)] >> (my_j & 31)) & 1u) cst = kQOne - (long long)(int)(iou(s_gbox[g], pb) * 1048576.f);
                        } else if (c - P == i0) {
                            cst = kDummy;
                        }
                        if (cst != kInf) {
                            const long long cur = cst - ui - v;
                            if (cur < minv) minv = cur, s_way[c] = j0;
                        }
                    }
                    // the workgroup's minimum over (slack, column): the lowest column of a tie
                    long long bv = (col && !used) ? minv : kInf;
                    int bj = c;
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
                    if (delta == kInf) {                             // cannot be: the row's dummy is always reachable
                        j0 = -1;
                        break;                                       // the whole workgroup alike
                    }
                    if (col) {
                        if (used) {
                            const int ro = s_rowof[c];               // the used columns are matched, to rows of their own
                            if (ro >= 0) s_u[ro] += delta;
                            v -= delta;
                        } else if (minv != kInf) {
                            minv -= delta;
                        }
                    }
                    if (tid == 0) s_u[i] += delta;
                    if (c == j1) used = true;
                    j0 = j1;
                    const int r1 = s_rowof[j1];
                    __syncthreads();                                 // the potentials before the next step reads them
                    if (r1 < 0) break;
                    i0 = r1;
                }
                if (tid == 0) {                                      // the path back to the new row, every column handed on
                    int j = j0;
                    for (int n = 0; n < C && j >= 0; ++n) {
                        const int jp = s_way[j];
                        s_rowof[j] = jp >= 0 ? s_rowof[jp] : i;
                        j = jp;
                    }
                }
                __syncthreads();
            }
            if (c < P && s_rowof[c] >= 0) s_match[s_rg[s_rowof[c]]] = my_j;
            __syncthreads();
        }
        // the records
        if (tid < G) {
            const int m = s_match[tid];
            float o = 0.f;
            int f = 0;
            if (m >= 0) {
                const int p = s_pid[m], l = s_last[a];
                o = iou(s_gbox[tid], s_pbox[m]);
                f = ((l >= 0 && l != p) ? 1 : 0) | (s_carry[tid] ? 2 : 0);
                s_last[a] = p;                        // the candidates' ids differ: a slot of its own
            }
            const int64_t row = (int64_t)t * G + tid;
            match[row] = m;
            miou[row] = o;
            flags[row] = f;
        }
        __syncthreads();                              // last[] and the rows before the next frame
    }
}

}  // namespace

extern "C" {

int64_t vd_mot_match_ws_bytes(int F, int G, int N) {
    if (F < 1 || G < 1 || G > kMaxRows || N < 1 || N > kMaxRows || (int64_t)F * kMaxRows > 0x7fffffff) return -1;
    return (int64_t)VD_MOT_WS_PER_ROW * F * (G + N);
}

int vd_mot_match(const float* gt_boxes, const int32_t* gt_cls, const int32_t* gt_id, const float* ids, const float* scores,
                 const float* bboxes, const int32_t* track, const int32_t* clip_start, int V, int F, int G, int N, int num_class,
                 float iou_thresh, int agnostic, int32_t* match, float* miou, int32_t* flags, uint32_t* adm, void* ws,
                 int64_t ws_bytes, void* stream) {
    VD_REQUIRE(gt_boxes && gt_cls && gt_id, "vd_mot_match: gt_boxes, gt_cls and gt_id must not be NULL");
    VD_REQUIRE(ids && scores && bboxes && track, "vd_mot_match: ids, scores, bboxes and track must not be NULL");
    VD_REQUIRE(match && miou && flags && adm, "vd_mot_match: the four output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_mot_match: ws must not be NULL");
    VD_REQUIRE(G >= 1 && G <= kMaxRows, "vd_mot_match: G=%d label rows per frame, 1 <= G <= %d are taken", G, kMaxRows);
    VD_REQUIRE(N >= 1 && N <= kMaxRows, "vd_mot_match: N=%d prediction rows per frame, 1 <= N <= %d are taken", N, kMaxRows);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_mot_match: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE((int64_t)F * kMaxRows <= 0x7fffffff, "vd_mot_match: F=%d frames, at most %d are taken", F, 0x7fffffff / kMaxRows);
    VD_REQUIRE(clip_start || V == 1, "vd_mot_match: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1, "vd_mot_match: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(iou_thresh > 0.f && iou_thresh <= 1.f, "vd_mot_match: iou_thresh=%g, it must lie in (0, 1]", (double)iou_thresh);
    VD_REQUIRE(agnostic == 0 || agnostic == 1, "vd_mot_match: agnostic=%d, 0 and 1 are taken", agnostic);
    const int64_t need = (int64_t)VD_MOT_WS_PER_ROW * F * (G + N);
    VD_REQUIRE(ws_bytes >= need, "vd_mot_match: ws_bytes=%lld, %d * F * (G + N) = %lld needed", (long long)ws_bytes, VD_MOT_WS_PER_ROW,
               (long long)need);
    VD_REQUIRE((((uintptr_t)gt_boxes | (uintptr_t)bboxes | (uintptr_t)adm) % 16) == 0,
               "vd_mot_match: gt_boxes, bboxes and adm must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)gt_cls | (uintptr_t)gt_id | (uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)clip_start |
                 (uintptr_t)match | (uintptr_t)miou | (uintptr_t)flags | (uintptr_t)ws) % 4) == 0,
               "vd_mot_match: gt_cls, gt_id, ids, scores, track, clip_start, match, miou, flags and ws must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int32_t* w_g = (int32_t*)ws;
    int32_t* w_p = w_g + (int64_t)F * G;
    if (clip_start) {                                 // a frame that no clip covers: -2 / 0 / 0 / 0
        const int64_t n = (int64_t)F * G;
        const int64_t blocks = vd_cdiv(n, 256);
        hipLaunchKernelGGL(k_mot_clear, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, n, match, miou, flags, adm);
        VD_CHECK_LAUNCH("vd_mot_match");
    }
    hipLaunchKernelGGL(k_mot_pairs, dim3((unsigned)V, (unsigned)(F < kMaxY ? F : kMaxY)), dim3(kThreads), 0, s, gt_boxes, gt_cls,
                       gt_id, ids, scores, bboxes, track, clip_start, F, G, N, num_class, iou_thresh, agnostic, adm, w_g, w_p);
    VD_CHECK_LAUNCH("vd_mot_match");
    hipLaunchKernelGGL(k_mot_assign, dim3((unsigned)V), dim3(kThreads), 0, s, gt_boxes, bboxes, clip_start, F, G, N, (const uint32_t*)adm, (const int32_t*)w_g, (const int32_t*)w_p, match, miou, flags);
    VD_CHECK_LAUNCH("vd_mot_match");
    return VD_OK;
}

}  // extern "C"
