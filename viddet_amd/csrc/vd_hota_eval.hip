// vd_hota_eval.hip — the per-frame matching of the HOTA tracking metric on the device (viddet_amd/hota_metric.py is the
// definition): ground-truth rows against tracked prediction rows, one assignment per frame on `global alignment
// score x similarity`.  What hota_match_host computes, bit for bit, on all three outputs.
//
// Arithmetic: the IoU is vd_track_math.h's fp32 one (no product and sum is contracted into an FMA, `/` is the correctly rounded
// division); q = int(iou * 2^20) is exact; everything after it is integers, so the sums of pass one may arrive in any order: they
// are ordinary integer atomicAdds.  The assignment's potentials and slacks are int64.
//
// Ids are dense: a ground-truth id takes part iff 0 <= id < A (A <= 1024), a track id iff 0 <= id < P.  The workspace holds, per
// clip, pm [A][P] int64 (the summed normalised similarities of an id pair), then for all clips cg [A] and cp [P] int32 (the
// candidate rows of an id).
//
// Launches (a kernel boundary stands between every writer and the readers of another workgroup):
//   k_hota_clear   every output as a frame that no clip covers has it (-2 / 0 / 0), the workspace zero
//   k_hota_pairs   a workgroup per frame, all frames of all clips side by side: the candidate rows of both sides (a compare loop),
//                  q of every pair with its row sums and column sums in LDS, then n = (q << 20) / (rq + cq - q) of every
//                  admissible pair added into the clip's pm, and the candidates counted into cg / cp.  q is formed again from
//                  the boxes for the second use: a 128 x 128 tile of it would be all of the static LDS.
//   k_hota_assign  a workgroup per frame: the candidates again, the two pools compacted by ballots, then assign_host operation
//                  for operation as k_mot_assign runs it: a thread per column (the pool's prediction rows, then a dummy per
//                  ground-truth row), per step the slack of every column against the row at the tree's tip, the workgroup's
//                  minimum over (slack, column), the update of potentials and slacks; the augmenting path is walked by one
//                  thread.  The score of a cell - A[a, p] from the finished tables (a 64-bit division) times q - is formed where
//                  it is read, for the tile's reason.  Entered only when both pools hold a row.  Then the records.
// Every id read from memory is range-checked before it indexes anything.  Every loop is bounded by F, G, N or G * (G + N).
// Plain vector loads and stores; the inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"

namespace {

constexpr int kMaxRows = 128;                         // G and N
constexpr int kThreads = 256;                         // both kernels: 4 wavefronts; the assignment's columns: G + N at most
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxGtId = 1024;
constexpr int kMaxY = 1024;                           // workgroups of a clip
constexpr int kMaxFrames = 1 << 22;                   // pm << 20 stays inside int64
constexpr long long kInf = 1ll << 62;                 // a forbidden cell, a column that no path reaches
constexpr int kQOne = 1 << 20;

// the quantised similarity of two boxes: a NaN counts as 0
__device__ inline int quant(const float4 a, const float4 b) {
    const float s = iou(a, b);
    return s > 0.f ? (int)(s * 1048576.f) : 0;
}

// Frame t into LDS, the ground-truth rows in slots [0, 128), the prediction rows in [128, 256): the box, the class and the
// candidate's id - a row is eligible iff its class is >= 0 and its id lies in [0, A) or [0, P), and a candidate iff no lower
// eligible row of its frame carries the same id -, else -1.  Called by the whole workgroup; the slots are complete on return.
__device__ inline void stage(const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_cls, const int32_t* __restrict__ gt_id,
                             const float* __restrict__ ids, const float* __restrict__ scores, const float* __restrict__ bboxes,
                             const int32_t* __restrict__ track, int t, int G, int N, int A, int P, int num_class, float4* s_box,
                             int* s_cls, int* s_el, int* s_cand) {
    const int tid = threadIdx.x;
    const bool pred = tid >= kMaxRows;                // threads 0 .. 127: a ground-truth row each; 128 .. 255: a prediction row
    const int r = pred ? tid - kMaxRows : tid;
    const int first = pred ? kMaxRows : 0;            // the side's first slot
    int el = -1, cls = -1;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < (pred ? N : G)) {
        if (pred) {
            const int64_t row = (int64_t)t * N + r;
            box = reinterpret_cast<const float4*>(bboxes)[row];
            cls = row_class(ids[row], scores[row], num_class, -INFINITY);
            const int u = track[row];
            if (cls >= 0 && u >= 0 && u < P) el = u;
        } else {
            const int64_t row = (int64_t)t * G + r;
            box = reinterpret_cast<const float4*>(gt_boxes)[row];
            cls = gt_cls[row];
            const int a = gt_id[row];
            if (cls >= 0 && a >= 0 && a < A) el = a;
        }
    }
    s_box[tid] = box;
    s_cls[tid] = cls;
    s_el[tid] = el;
    __syncthreads();
    int cand = el;
    if (cand >= 0)
        for (int k = 0; k < r; ++k)
            if (s_el[first + k] == cand) {            // a lower eligible row of the frame carries the id
                cand = -1;
                break;
            }
    s_cand[tid] = cand;
    __syncthreads();
}

__global__ void k_hota_clear(int64_t rows, int32_t* __restrict__ match, float* __restrict__ msim, int32_t* __restrict__ mscore,
                             int64_t words, int32_t* __restrict__ ws) {
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, by = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = at; i < rows; i += by) {
        match[i] = -2;
        msim[i] = 0.f;
        mscore[i] = 0;
    }
    for (int64_t i = at; i < words; i += by) ws[i] = 0;
}

__global__ __launch_bounds__(kThreads) void k_hota_pairs(const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_cls,
                                                         const int32_t* __restrict__ gt_id, const float* __restrict__ ids,
                                                         const float* __restrict__ scores, const float* __restrict__ bboxes,
                                                         const int32_t* __restrict__ track, const int32_t* __restrict__ clip_start,
                                                         int F, int G, int N, int A, int P, int num_class, int agnostic,
                                                         unsigned long long* __restrict__ pm, int32_t* __restrict__ cg,
                                                         int32_t* __restrict__ cp) {
    __shared__ float4 s_box[2 * kMaxRows];            // the ground-truth rows, then the prediction rows
    __shared__ int s_cls[2 * kMaxRows];
    __shared__ int s_el[2 * kMaxRows];                // the id of an eligible row, else -1
    __shared__ int s_cand[2 * kMaxRows];              // the id of a candidate row, else -1
    __shared__ int s_sum[2 * kMaxRows];               // rq of the ground-truth rows, then cq of the prediction rows: <= 128 * 2^20
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const int tid = threadIdx.x;
    const int v = blockIdx.x;
    const int j = tid & (kMaxRows - 1), half = tid / kMaxRows;
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        stage(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, t, G, N, A, P, num_class, s_box, s_cls, s_el, s_cand);
        s_sum[tid] = 0;
        const int mine = s_cand[tid];
        if (mine >= 0) atomicAdd(tid < kMaxRows ? cg + (int64_t)v * A + mine : cp + (int64_t)v * P + mine, 1);
        __syncthreads();
        // a thread per prediction row j and half of the ground-truth rows
        const float4 pb = s_box[kMaxRows + j];
        const int pc = s_cls[kMaxRows + j];
        const int p = j < N ? s_cand[kMaxRows + j] : -1;
        int colsum = 0;
        if (p >= 0)
            for (int g = half; g < G; g += 2)
                if (s_cand[g] >= 0 && (agnostic || s_cls[g] == pc)) {
                    const int q = quant(s_box[g], pb);
                    if (q > 0) {
                        atomicAdd(&s_sum[g], q);
                        colsum += q;
                    }
                }
        if (colsum > 0) atomicAdd(&s_sum[kMaxRows + j], colsum);
        __syncthreads();
        if (colsum > 0) {                             // the column holds an admissible pair of this thread's rows
            const long long cq = s_sum[kMaxRows + j];
            for (int g = half; g < G; g += 2) {
                const int a = s_cand[g];
                if (a >= 0 && (agnostic || s_cls[g] == pc)) {
                    const long long q = quant(s_box[g], pb);
                    if (q > 0) {
                        const long long n = (q << 20) / ((long long)s_sum[g] + cq - q);
                        if (n > 0) atomicAdd(pm + ((int64_t)v * A + a) * P + p, (unsigned long long)n);
                    }
                }
            }
        }
        __syncthreads();                              // the rows before the next frame overwrites them
    }
}

__global__ __launch_bounds__(kThreads) void k_hota_assign(const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_cls,
                                                          const int32_t* __restrict__ gt_id, const float* __restrict__ ids,
                                                          const float* __restrict__ scores, const float* __restrict__ bboxes,
                                                          const int32_t* __restrict__ track, const int32_t* __restrict__ clip_start,
                                                          int F, int G, int N, int A, int P, int num_class, int agnostic,
                                                          const long long* __restrict__ pm, const int32_t* __restrict__ cg,
                                                          const int32_t* __restrict__ cp, int32_t* __restrict__ match,
                                                          float* __restrict__ msim, int32_t* __restrict__ mscore) {
    __shared__ float4 s_box[2 * kMaxRows];
    __shared__ int s_cls[2 * kMaxRows];
    __shared__ int s_el[2 * kMaxRows];
    __shared__ int s_cand[2 * kMaxRows];
    __shared__ int s_cnt[2 * kMaxRows];               // cg of a ground-truth candidate's id, then cp of a prediction candidate's
    __shared__ int s_match[kMaxRows];
    __shared__ int s_rg[kMaxRows];                    // the pools: ground-truth rows, prediction rows, in row order
    __shared__ int s_cp[kMaxRows];
    __shared__ int s_n[kWaves];
    __shared__ long long s_u[kMaxRows];               // the potentials of the pool's ground-truth rows
    __shared__ int s_way[kThreads];
    __shared__ int s_rowof[kThreads];                 // the pool row a column is matched to, -1: none
    __shared__ long long s_red_v[kWaves];
    __shared__ int s_red_j[kWaves];
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int v = blockIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the score of the cell (ground-truth row g, prediction row j), both candidates; -1: the pair is not admissible
    auto score = [&](int g, int j) -> long long {
        if (!(agnostic || s_cls[g] == s_cls[kMaxRows + j])) return -1;
        const long long q = quant(s_box[g], s_box[kMaxRows + j]);
        if (q <= 0) return -1;
        const int a = s_cand[g], p = s_cand[kMaxRows + j];           // in [0, A) and [0, P): stage() checked them
        const long long m = pm[((int64_t)v * A + a) * P + p];
        const long long den = ((long long)(s_cnt[g] + s_cnt[kMaxRows + j]) << 20) - m;
        const long long al = (m > 0 && den > 0) ? (m << 20) / den : 0;
        return (al * q) >> 20;
    };
    for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
        stage(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, t, G, N, A, P, num_class, s_box, s_cls, s_el, s_cand);
        const int mine = s_cand[tid];
        s_cnt[tid] = mine >= 0 ? (tid < kMaxRows ? cg[(int64_t)v * A + mine] : cp[(int64_t)v * P + mine]) : 0;
        if (tid < kMaxRows) s_match[tid] = mine >= 0 ? -1 : -2;
        // the pools: wavefronts 0, 1 the ground-truth candidates, wavefronts 2, 3 the prediction candidates
        const int r = tid & (kMaxRows - 1);
        const bool in_pool = mine >= 0;
        const unsigned long long votes = __ballot(in_pool);
        if (lane == 0) s_n[wave] = __popcll(votes);
        __syncthreads();
        if (in_pool) (tid < kMaxRows ? s_rg : s_cp)[((wave & 1) ? s_n[wave - 1] : 0) + __popcll(votes & below)] = r;
        const int R = s_n[0] + s_n[1], Pn = s_n[2] + s_n[3];
        __syncthreads();
        if (R > 0 && Pn > 0) {
            // assign_host: column c < Pn is prediction row s_cp[c], column Pn + r the dummy of pool row r
            const int C = Pn + R;
            const int c = tid;
            const bool col = c < C;
            const int my_j = c < Pn ? s_cp[c] : 0;
            long long pv = 0;                                        // the column's potential
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
                        if (c < Pn) {
                            const long long s = score(g, my_j);
                            if (s >= 0) cst = kQOne - s;
                        } else if (c - Pn == i0) {
                            cst = kQOne;                             // the row's own dummy: a match of score zero
                        }
                        if (cst != kInf) {
                            const long long cur = cst - ui - pv;
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
                            pv -= delta;
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
            if (c < Pn && s_rowof[c] >= 0) s_match[s_rg[s_rowof[c]]] = my_j;
            __syncthreads();
        }
        // the records
        if (tid < G) {
            const int m = s_match[tid];
            float o = 0.f;
            int sc = 0;
            if (m >= 0) {
                o = iou(s_box[tid], s_box[kMaxRows + m]);
                sc = (int)score(tid, m);
            }
            const int64_t row = (int64_t)t * G + tid;
            match[row] = m;
            msim[row] = o;
            mscore[row] = sc;
        }
        __syncthreads();                              // the rows before the next frame overwrites them
    }
}

int64_t ws_bytes(int64_t V, int64_t A, int64_t P) {
    if (V < 1 || A < 1 || A > kMaxGtId || P < 1 || P > 0x7fffffff || V > 0x7fffffff) return -1;
    const int64_t per = 8 * A * P + 4 * A + 4 * P;    // < 2^44
    if (per > 0x7fffffffffffll / V) return -1;
    return V * per;
}

}  // namespace

extern "C" {

int64_t vd_hota_ws_bytes(int V, int A, int P) { return ws_bytes(V, A, P); }

int vd_hota_match(const float* gt_boxes, const int32_t* gt_cls, const int32_t* gt_id, const float* ids, const float* scores,
                  const float* bboxes, const int32_t* track, const int32_t* clip_start, int V, int F, int G, int N, int A, int P,
                  int num_class, int agnostic, int32_t* match, float* msim, int32_t* mscore, void* ws, int64_t ws_bytes_given,
                  void* stream) {
    VD_REQUIRE(gt_boxes && gt_cls && gt_id, "vd_hota_match: gt_boxes, gt_cls and gt_id must not be NULL");
    VD_REQUIRE(ids && scores && bboxes && track, "vd_hota_match: ids, scores, bboxes and track must not be NULL");
    VD_REQUIRE(match && msim && mscore, "vd_hota_match: the three output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_hota_match: ws must not be NULL");
    VD_REQUIRE(G >= 1 && G <= kMaxRows, "vd_hota_match: G=%d label rows per frame, 1 <= G <= %d are taken", G, kMaxRows);
    VD_REQUIRE(N >= 1 && N <= kMaxRows, "vd_hota_match: N=%d prediction rows per frame, 1 <= N <= %d are taken", N, kMaxRows);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_hota_match: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(F <= kMaxFrames, "vd_hota_match: F=%d frames, at most %d are taken", F, kMaxFrames);
    VD_REQUIRE(A >= 1 && A <= kMaxGtId, "vd_hota_match: A=%d ground-truth ids, 1 <= A <= %d are taken", A, kMaxGtId);
    VD_REQUIRE(P >= 1, "vd_hota_match: P=%d track ids, P >= 1 needed", P);
    VD_REQUIRE(clip_start || V == 1, "vd_hota_match: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1, "vd_hota_match: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(agnostic == 0 || agnostic == 1, "vd_hota_match: agnostic=%d, 0 and 1 are taken", agnostic);
    const int64_t need = ws_bytes(V, A, P);
    VD_REQUIRE(need >= 0, "vd_hota_match: the workspace of V=%d clips, A=%d and P=%d ids is beyond what is taken", V, A, P);
    VD_REQUIRE(ws_bytes_given >= need, "vd_hota_match: ws_bytes=%lld, V * (8 * A * P + 4 * A + 4 * P) = %lld needed",
               (long long)ws_bytes_given, (long long)need);
    VD_REQUIRE((((uintptr_t)gt_boxes | (uintptr_t)bboxes) % 16) == 0, "vd_hota_match: gt_boxes and bboxes must be 16-byte aligned");
    VD_REQUIRE(((uintptr_t)ws % 8) == 0, "vd_hota_match: ws must be 8-byte aligned");
    VD_REQUIRE((((uintptr_t)gt_cls | (uintptr_t)gt_id | (uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)clip_start |
                 (uintptr_t)match | (uintptr_t)msim | (uintptr_t)mscore) % 4) == 0,
               "vd_hota_match: gt_cls, gt_id, ids, scores, track, clip_start, match, msim and mscore must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    long long* pm = (long long*)ws;
    int32_t* cg = (int32_t*)(pm + (int64_t)V * A * P);
    int32_t* cp = cg + (int64_t)V * A;
    const int64_t rows = (int64_t)F * G, words = need / 4;
    const int64_t blocks = vd_cdiv(rows > words ? rows : words, 256);
    hipLaunchKernelGGL(k_hota_clear, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, rows, match, msim, mscore, words,
                       (int32_t*)ws);
    VD_CHECK_LAUNCH("vd_hota_match");
    const dim3 grid((unsigned)V, (unsigned)(F < kMaxY ? F : kMaxY));
    hipLaunchKernelGGL(k_hota_pairs, grid, dim3(kThreads), 0, s, gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start, F, G, N,
                       A, P, num_class, agnostic, (unsigned long long*)pm, cg, cp);
    VD_CHECK_LAUNCH("vd_hota_match");
    hipLaunchKernelGGL(k_hota_assign, grid, dim3(kThreads), 0, s, gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start, F, G, N,
                       A, P, num_class, agnostic, (const long long*)pm, (const int32_t*)cg, (const int32_t*)cp, match, msim, mscore);
    VD_CHECK_LAUNCH("vd_hota_match");
    return VD_OK;
}

}  // extern "C"
