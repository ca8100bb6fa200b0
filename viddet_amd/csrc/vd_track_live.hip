// vd_track_live.hip — the tracker of vd_track.hip in resumable form: vd_track_push runs the extend and start steps on the frames
// of one push and carries the active tracks from launch to launch in a state block in HBM, so that a stream of frames that
// never says where it ends keeps its tracks (viddet_amd/track.py::track_online_host is the definition).
//
// Arithmetic and tie rules are k_track's, the same functions (vd_track_math.h): fp32, no product and sum contracted into an
// FMA, `/` the correctly rounded division, choice_before's order (np.argmax's: a NaN first, the larger value, the lower row).
// Nothing is decided on the device: per row the track's id (a creation number counted over the whole stream), its length so
// far and its maximum score so far come out; track.finalize_tracks makes track_host's arrays of a finished clip from them.
//
// One launch, one workgroup of kWaves wavefronts per stream.  A stream's state - VD_TRACK_STATE_BYTES - is
//   int32 n_active, int32 next_id, 8 bytes unused                                   16 bytes
//   float4 box[1024], int32 class[1024], id[1024], misses[1024], length[1024], float maximum[1024]
// in order of creation, the first n_active entries live.  It is read into LDS at entry (n_active clamped into [0, 1024] before
// it indexes anything) and the live entries and the header are written back at exit, with ordinary vector stores.  All zero
// bytes are a fresh stream.  No workspace, no atomics: every output is the same on every run.  The inputs are never written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"

namespace {

constexpr int kWaves = 8;                             // wavefronts of a stream's workgroup
constexpr int kThreads = kWaves * kWave;
constexpr int kHeaderBytes = 16;

static_assert(VD_TRACK_STATE_BYTES == kHeaderBytes + kMaxActive * (16 + 5 * 4), "the state layout and the header disagree");
static_assert(VD_TRACK_STATE_BYTES % 16 == 0, "every stream's box table must stay 16-byte aligned");

__global__ __launch_bounds__(kThreads) void k_track_push(const float* __restrict__ ids, const float* __restrict__ scores,
                                                         const float* __restrict__ bboxes, int F, int N, int num_class,
                                                         float sigma_l, float sigma_iou, int max_age, void* state,
                                                         int32_t* __restrict__ out_track, int32_t* __restrict__ out_len,
                                                         float* __restrict__ out_score) {
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
    const unsigned long long below = (1ull << lane) - 1ull;

    // this stream's state
    char* st = (char*)state + (int64_t)blockIdx.x * VD_TRACK_STATE_BYTES;
    int32_t* g_hdr = (int32_t*)st;
    float4* g_box = (float4*)(st + kHeaderBytes);
    int32_t* g_cls = (int32_t*)(st + kHeaderBytes + 16 * kMaxActive);
    int32_t* g_id = g_cls + kMaxActive;
    int32_t* g_miss = g_id + kMaxActive;
    int32_t* g_len = g_miss + kMaxActive;
    float* g_max = (float*)(g_len + kMaxActive);
    int n0 = g_hdr[0];
    n0 = n0 < 0 ? 0 : (n0 > kMaxActive ? kMaxActive : n0);        // before it indexes anything
    int next_id = g_hdr[1];                           // wavefront 0's
    for (int i = threadIdx.x; i < n0; i += kThreads) {
        a_box[i] = g_box[i];
        a_cls[i] = g_cls[i];
        a_id[i] = g_id[i];
        a_miss[i] = g_miss[i];
        a_len[i] = g_len[i];
        a_max[i] = g_max[i];
    }
    if (threadIdx.x == 0) s_nact = n0;

    const int64_t first = (int64_t)blockIdx.x * F * N;
    for (int t = 0; t < F; ++t) {
        const int64_t base = first + (int64_t)t * N;
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
        __syncthreads();                              // the state just read, or last frame's table and count
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
            // in order of creation; only a track whose row an earlier track took chooses again, among the free rows (k_track)
            unsigned long long tk_lo = 0ull, tk_hi = 0ull;
            int mine[2] = {-1, -1}, mlen[2] = {0, 0};
            float mmax[2] = {-1.f, -1.f};
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
                    const float s = s_score[br];
                    nb = s_box[br];
                    ++len;
                    if (s > mx) mx = s;
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (br == lane + h * kWave) mine[h] = id, mlen[h] = len, mmax[h] = mx;
                }
                if (hit || miss <= max_age) {
                    if (lane == 0) {
                        a_box[w] = nb;
                        a_cls[w] = tc;
                        a_id[w] = id;
                        a_miss[w] = miss;
                        a_len[w] = len;
                        a_max[w] = mx;
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
                    if (pos < kMaxActive) {           // always from a state this kernel wrote: w + n_new <= N * (max_age + 1)
                        a_box[pos] = box[h];
                        a_cls[pos] = cls[h];
                        a_id[pos] = id;
                        a_miss[pos] = 0;
                        a_len[pos] = 1;
                        a_max[pos] = sc[h];
                    }
                    mine[h] = id, mlen[h] = 1, mmax[h] = sc[h];
                }
            }
            if (lane == 0) s_nact = w + n_new < kMaxActive ? w + n_new : kMaxActive;
            next_id += n_new;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = lane + h * kWave;
                if (r < N) {
                    out_track[base + r] = mine[h];
                    out_len[base + r] = mlen[h];
                    out_score[base + r] = mmax[h];
                }
            }
        }
        // the next frame's first barrier stands between these writes and their readers
    }
    __syncthreads();                                  // the table and the count before they are written back
    const int n1 = s_nact;
    for (int i = threadIdx.x; i < n1; i += kThreads) {
        g_box[i] = a_box[i];
        g_cls[i] = a_cls[i];
        g_id[i] = a_id[i];
        g_miss[i] = a_miss[i];
        g_len[i] = a_len[i];
        g_max[i] = a_max[i];
    }
    if (threadIdx.x == 0) g_hdr[0] = n1, g_hdr[1] = next_id;
}

}  // namespace

extern "C" {

int vd_track_push(const float* ids, const float* scores, const float* bboxes, int V, int F, int N, int num_class, float sigma_l,
                  float sigma_iou, int max_age, void* state, int64_t state_bytes, int32_t* out_track, int32_t* out_len,
                  float* out_score, void* stream) {
    VD_REQUIRE(ids && scores && bboxes, "vd_track_push: ids, scores and bboxes must not be NULL");
    VD_REQUIRE(out_track && out_len && out_score, "vd_track_push: the three output pointers must not be NULL");
    VD_REQUIRE(state, "vd_track_push: state must not be NULL");
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_track_push: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 1 && V >= 1, "vd_track_push: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(num_class >= 1, "vd_track_push: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(sigma_l == sigma_l && sigma_iou == sigma_iou, "vd_track_push: sigma_l and sigma_iou must not be NaN");
    VD_REQUIRE(max_age >= 0 && max_age <= kMaxAge, "vd_track_push: max_age=%d, 0 <= max_age <= %d are taken", max_age, kMaxAge);
    VD_REQUIRE(state_bytes >= (int64_t)VD_TRACK_STATE_BYTES * V, "vd_track_push: state_bytes=%lld, %d * V = %lld needed",
               (long long)state_bytes, VD_TRACK_STATE_BYTES, (long long)((int64_t)VD_TRACK_STATE_BYTES * V));
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)state) % 16) == 0, "vd_track_push: bboxes and state must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)out_track | (uintptr_t)out_len | (uintptr_t)out_score) % 4) == 0,
               "vd_track_push: ids, scores, out_track, out_len and out_score must be 4-byte aligned");
    hipLaunchKernelGGL(k_track_push, dim3((unsigned)V), dim3(kThreads), 0, (hipStream_t)stream, ids, scores, bboxes, F, N,
                       num_class, sigma_l, sigma_iou, max_age, state, out_track, out_len, out_score);
    VD_CHECK_LAUNCH("vd_track_push");
    return VD_OK;
}

}  // extern "C"
