// vd_track_assign.h — the minimum-cost assignment of a frame's rows to the active tracks, stated once for the kernels whose
// frame body associates twice: vd_track_byte.hip (k_track_byte) and vd_track_kf_live.hip (k_track_kf_push).  It is
// mot_metric.assign_host operation for operation on a workgroup of kThreads threads (viddet_amd/byte.py is the definition,
// DESIGN.md 36): integers only, the potentials and slacks int64, the lowest column of a tie.  The only floating-point
// operation is the IoU of vd_track_math.h; every includer sets the pragma below ahead of the include, and it is repeated here
// so that the header is right on its own.  assign_table, behind it, is the same loop on cells that were formed ahead of it and
// are read from a table: vd_track_sort_app.hip's.
#pragma once
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTrackPer = kMaxActive / kThreads;      // tracks of a thread
constexpr int kMaxCols = kMaxActive + kMaxN;          // the assignment's columns: the tracks, then a dummy per row
constexpr int kColPer = (kMaxCols + kThreads - 1) / kThreads;
constexpr long long kInf = 1ll << 62;                 // a forbidden cell, a column that no path reaches
constexpr long long kDummy = 1ll << 27;
constexpr int kQOne = 1 << 20;

// assign_host on R rows (s_rg: their rows of the frame, in row order) against the K tracks and a dummy per row: column c < K is
// track c, column K + r the dummy of assignment row r.  Bit j of `elig`: this thread's column tid + j * kThreads, a track, may
// be matched (equal classes and iou >= thr still decide); a column without its bit is forbidden in every row.  Called by the
// whole workgroup alike, with R > 0 and K > 0.  Leaves s_rowof[c], the assignment row of column c or -1, behind a barrier.
__device__ __forceinline__ void assign(const int* s_rg, int R, int K, float thr, unsigned elig, const float4* s_box, const int* s_cls,
                                       const float4* a_pbox, const int* a_cls, int* s_way, int* s_rowof, long long* s_u,
                                       long long* s_red_v, int* s_red_j, int tid, int lane, int wave) {
    const int C = K + R;
    long long v[kColPer], minv[kColPer];
#pragma unroll
    for (int j = 0; j < kColPer; ++j) {
        const int c = tid + j * kThreads;
        v[j] = 0;
        if (c < C) s_rowof[c] = -1;
    }
    if (tid < R) s_u[tid] = 0;
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
            int g = s_rg[i0];
            if (g < 0 || g >= kMaxN) g = 0;           // cannot be: the rows of this frame
            const long long ui = s_u[i0];
            const float4 gb = s_box[g];
            const int gc = s_cls[g];
            long long bv = kInf;
            int bj = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < kColPer; ++j) {
                const int c = tid + j * kThreads;
                if (c < C && !((used >> j) & 1u)) {
                    long long cst = kInf;
                    if (c < K) {
                        if (((elig >> j) & 1u) && a_cls[c] == gc) {
                            const float q = iou(a_pbox[c], gb);
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

// The same assignment on cells that were formed ahead of it (vd_track_sort_app.hip): tab[r * ld + c] is the
// similarity of assignment row r and track c on the 2^20 scale, below 0 where the cell is forbidden, so a cell costs
// kQOne - tab[r * ld + c].  Everything else - the dummies, the potentials, the lowest column of a tie, what is left in
// s_rowof - is assign()'s, statement for statement; the cells are read, never written, and r < R <= kMaxN, c < K <= ld index it.
__device__ __forceinline__ void assign_table(int R, int K, const int32_t* tab, int ld, int* s_way, int* s_rowof,
                                             long long* s_u, long long* s_red_v, int* s_red_j, int tid, int lane, int wave) {
    const int C = K + R;
    long long v[kColPer], minv[kColPer];
#pragma unroll
    for (int j = 0; j < kColPer; ++j) {
        const int c = tid + j * kThreads;
        v[j] = 0;
        if (c < C) s_rowof[c] = -1;
    }
    if (tid < R) s_u[tid] = 0;
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
            const long long ui = s_u[i0];
            const int32_t* cells = tab + (int64_t)i0 * ld;
            long long bv = kInf;
            int bj = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < kColPer; ++j) {
                const int c = tid + j * kThreads;
                if (c < C && !((used >> j) & 1u)) {
                    long long cst = kInf;
                    if (c < K) {
                        const int sim = cells[c];
                        if (sim >= 0 && sim <= kQOne) cst = kQOne - (long long)sim;
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

}  // namespace
