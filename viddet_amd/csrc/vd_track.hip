// vd_track.hip — the detections of video clips linked into tracks on the device (viddet_amd/track.py is the definition,
// DESIGN.md 28): the IOU tracker of Bochinski, Eiselein and Sikora (AVSS 2017) with a max_age extension (0 is the paper).
//
// Arithmetic: fp32, operation for operation what track_host does (vd_seq_nms.hip's IoU: no product and sum is contracted into
// an FMA, `/` is the correctly rounded division; `iou >= sigma_iou`, `score >= sigma_l`, `max >= sigma_h` are the plain >=).
//
// One launch, one workgroup of kWaves wavefronts per clip, in every wavefront lane l holding rows l and l + 64 of the frame; no
// communication between workgroups.  The active tracks - last box, class, id, miss count, length, maximum score - sit in LDS
// in order of creation, at most N * (max_age + 1) <= 1024 of them (a track that is active took a row of one of the last
// max_age + 1 frames).  Per frame:
//   extend  first every track's choice among ALL candidates of its class - the largest IoU (a NaN first, as np.argmax; ties to
//           the lowest row) - the wavefronts side by side; then wavefront 0 walks the tracks in order: a choice whose row is
//           free stands, one whose row an earlier track took is made again among the free rows; a hit sets the row's bit in
//           the taken masks; the surviving track is written back at the table's write position, which never passes the read
//           position, so the table stays packed and in order without a pass of its own
//   start   the candidates not taken: two ballots, a prefix count gives every one its slot behind the survivors and its id
// Every change of a track's length and maximum is written through to the workspace, indexed by the clip's first row + the id
// (a clip makes at most one track per row).  A closing pass over the clip's rows reads them back and decides.
// No atomics: every output is the same on every run.  The inputs are never written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"

namespace {

constexpr int kWaves = 8;                             // wavefronts of a clip's workgroup
constexpr int kThreads = kWaves * kWave;

__global__ __launch_bounds__(kThreads) void k_track(const float* __restrict__ ids, const float* __restrict__ scores,
                                                    const float* __restrict__ bboxes, const int32_t* __restrict__ clip_start, int F,
                                                    int N, int num_class, float sigma_l, float sigma_h, float sigma_iou, int t_min,
                                                    int max_age, int32_t* __restrict__ out_track, int32_t* __restrict__ out_len,
                                                    float* __restrict__ out_score, void* ws) {
    __shared__ float4 s_box[kMaxN];                   // this frame's rows
    __shared__ float s_score[kMaxN];
    __shared__ float4 a_box[kMaxActive];              // the active tracks, in order of creation
    __shared__ int a_cls[kMaxActive];
    __shared__ int a_id[kMaxActive];
    __shared__ int a_miss[kMaxActive];
    __shared__ int a_len[kMaxActive];
    __shared__ float a_max[kMaxActive];
    __shared__ float p_iou[kMaxActive];               // a track's choice among ALL candidates of its class in the frame
    __shared__ int p_row[kMaxActive];
    __shared__ int s_nact;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    if (t0 >= t1) return;                             // the whole workgroup alike
    // the clip's tracks: ids [0, (t1 - t0) * N), so its slice of the tables starts at its first row
    int32_t* __restrict__ w_len = (int32_t*)ws + (int64_t)t0 * N;
    float* __restrict__ w_max = (float*)ws + (int64_t)F * N + (int64_t)t0 * N;
    const unsigned long long below = (1ull << lane) - 1ull;

    if (threadIdx.x == 0) s_nact = 0;
    int next_id = 0;                                  // wavefront 0's
    for (int t = t0; t < t1; ++t) {
        const int64_t base = (int64_t)t * N;
        int cls[2];                                   // every wavefront holds the frame's rows, lane l rows l and l + 64
        float4 box[2];
        float sc[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = lane + h * kWave;
            cls[h] = -1, sc[h] = 0.f;
            box[h] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < N) {
                sc[h] = scores[base + r];
                box[h] = reinterpret_cast<const float4*>(bboxes)[base + r];
                cls[h] = row_class(ids[base + r], sc[h], num_class, sigma_l);
                if (wave == 0) {
                    s_box[r] = box[h];
                    s_score[r] = sc[h];
                }
            }
        }
        __syncthreads();                              // last frame's table and count
        const int n_act = s_nact;                     // <= kMaxActive

        // every track's choice as if no row were taken, the wavefronts side by side
        for (int k = wave; k < n_act; k += kWaves) {
            float bv;
            int br;
            choose(a_box[k], a_cls[k], cls, box, 0ull, 0ull, lane, bv, br);
            if (lane == 0) p_iou[k] = bv, p_row[k] = br;
        }
        __syncthreads();

        if (wave == 0) {
            // in order of creation.  A choice whose row is still free is the track's choice among the free rows too (a maximum
            // of the larger set that lies in the smaller one, the lowest row of its ties included); a choice below sigma_iou
            // bounds every other row's IoU, so the track misses whatever is taken; only a track whose row an earlier track took
            // chooses again, among the free rows
            unsigned long long tk_lo = 0ull, tk_hi = 0ull;
            int mine[2] = {-1, -1};
            int w = 0;                                // survivors so far: w <= k, so nothing unread is overwritten
            for (int k = 0; k < n_act; ++k) {
                const float4 tb = a_box[k];
                const int tc = a_cls[k];
                float bv = p_iou[k];
                int br = p_row[k];
                if (br >= 0 && !(bv < sigma_iou) && (((br < kWave ? tk_lo : tk_hi) >> (br & (kWave - 1))) & 1ull))
                    choose(tb, tc, cls, box, tk_lo, tk_hi, lane, bv, br);
                // every lane holds the same choice
                const bool hit = br >= 0 && bv >= sigma_iou;
                const int id = a_id[k];
                const int miss = hit ? 0 : a_miss[k] + 1;
                int len = a_len[k];
                float mx = a_max[k];
                float4 nb = tb;
                if (hit) {
                    if (br < kWave) tk_lo |= 1ull << br;
                    else tk_hi |= 1ull << (br - kWave);
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (br == lane + h * kWave) mine[h] = id;
                    const float s = s_score[br];
                    nb = s_box[br];
                    ++len;
                    if (s > mx) mx = s;
                }
                if (hit || miss <= max_age) {
                    if (lane == 0) {
                        a_box[w] = nb;
                        a_cls[w] = tc;
                        a_id[w] = id;
                        a_miss[w] = miss;
                        a_len[w] = len;
                        a_max[w] = mx;
                        if (hit) w_len[id] = len, w_max[id] = mx;
                    }
                    ++w;
                }
            }
            // start: the candidates not taken, in row order, behind the survivors
            const bool fresh[2] = {cls[0] >= 0 && !((tk_lo >> lane) & 1ull), cls[1] >= 0 && !((tk_hi >> lane) & 1ull)};
            const unsigned long long lo = __ballot(fresh[0]), hi = __ballot(fresh[1]);
            const int n_lo = __popcll(lo), n_new = n_lo + __popcll(hi);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (fresh[h]) {
                    const int rank = h == 0 ? __popcll(lo & below) : n_lo + __popcll(hi & below);
                    const int pos = w + rank, id = next_id + rank;
                    if (pos < kMaxActive) {           // always: w + n_new <= N * (max_age + 1)
                        a_box[pos] = box[h];
                        a_cls[pos] = cls[h];
                        a_id[pos] = id;
                        a_miss[pos] = 0;
                        a_len[pos] = 1;
                        a_max[pos] = sc[h];
                    }
                    w_len[id] = 1;                    // id < the rows of the clip so far
                    w_max[id] = sc[h];
                    mine[h] = id;
                }
            }
            if (lane == 0) s_nact = w + n_new < kMaxActive ? w + n_new : kMaxActive;
            next_id += n_new;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = lane + h * kWave;
                if (r < N) out_track[base + r] = mine[h];
            }
        }
        // the next frame's first barrier stands between these writes and their readers
    }
    __syncthreads();                                  // the rows' ids and the tables before the closing pass
    // decide: a row keeps its id where its track's maximum >= sigma_h and its length >= t_min
    const int64_t first = (int64_t)t0 * N, rows = (int64_t)(t1 - t0) * N;
    for (int64_t i = threadIdx.x; i < rows; i += kThreads) {
        const int id = out_track[first + i];
        int len = 0;
        float mx = -1.f;
        bool keep = false;
        if (id >= 0) {
            len = w_len[id];
            mx = w_max[id];
            keep = mx >= sigma_h && len >= t_min;
        }
        out_track[first + i] = keep ? id : -1;
        out_len[first + i] = keep ? len : 0;
        out_score[first + i] = keep ? mx : -1.f;
    }
}

}  // namespace

extern "C" {

int vd_track(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
             int num_class, float sigma_l, float sigma_h, float sigma_iou, int t_min, int max_age, int32_t* out_track,
             int32_t* out_len, float* out_score, void* ws, int64_t ws_bytes, void* stream) {
    VD_REQUIRE(ids && scores && bboxes, "vd_track: ids, scores and bboxes must not be NULL");
    VD_REQUIRE(out_track && out_len && out_score, "vd_track: the three output pointers must not be NULL");
    VD_REQUIRE(ws, "vd_track: ws must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_track: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_track: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(clip_start || V == 1, "vd_track: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(num_class >= 1, "vd_track: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(sigma_l == sigma_l && sigma_h == sigma_h && sigma_iou == sigma_iou,
               "vd_track: sigma_l, sigma_h and sigma_iou must not be NaN");
    VD_REQUIRE(t_min >= 1, "vd_track: t_min >= 1 needed, got %d", t_min);
    VD_REQUIRE(max_age >= 0 && max_age <= kMaxAge, "vd_track: max_age=%d, 0 <= max_age <= %d are taken", max_age, kMaxAge);
    VD_REQUIRE(ws_bytes >= (int64_t)VD_TRACK_WS_PER_ROW * F * N, "vd_track: ws_bytes=%lld, %d * F * N = %lld needed",
               (long long)ws_bytes, VD_TRACK_WS_PER_ROW, (long long)((int64_t)VD_TRACK_WS_PER_ROW * F * N));
    VD_REQUIRE(((uintptr_t)bboxes % 16) == 0, "vd_track: bboxes must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)clip_start | (uintptr_t)out_track | (uintptr_t)out_len |
                 (uintptr_t)out_score | (uintptr_t)ws) % 4) == 0,
               "vd_track: ids, scores, clip_start, out_track, out_len, out_score and ws must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (clip_start) {                                 // a frame that no clip covers comes out as rows of -1 / 0 / -1
        fill_uncovered<false>(s, (int64_t)F * N, out_track, out_len, out_score);
        VD_CHECK_LAUNCH("vd_track");
    }
    hipLaunchKernelGGL(k_track, dim3((unsigned)V), dim3(kThreads), 0, s, ids, scores, bboxes, clip_start, F, N, num_class, sigma_l,
                       sigma_h, sigma_iou, t_min, max_age, out_track, out_len, out_score, ws);
    VD_CHECK_LAUNCH("vd_track");
    return VD_OK;
}

}  // extern "C"
