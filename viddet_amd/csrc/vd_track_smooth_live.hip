// vd_track_smooth_live.hip — the Rauch-Tung-Striebel smoother of vd_track_smooth.hip in fixed-lag form, resumable: for a stream
// of frames that never says where it ends, vd_track_smooth_push takes the frames of one push, keeps the last 16 frames' members
// - ids, boxes, posterior states, links - in a state block in HBM and gives every frame out `lag` frames late, smoothed against
// the frames before it and the `lag` frames after it (viddet_amd/smooth_lag.py::smooth_lag_host is the definition, DESIGN.md
// 40).
//
// Arithmetic: vd_track_smooth's, the same functions (vd_track_kf.h, vd_track_smooth_math.h): fp32, no product and sum contracted
// into an FMA, `/` and sqrtf the correctly rounded ones.
//
// One launch, ONE workgroup of 256 threads per stream walks the stream's F new frames in order; no communication between
// workgroups.  The state, a block of VD_TRACK_SMOOTH_LIVE_STATE_BYTES per stream, is a ring of 16 frame slots of 128 rows, frame
// t in slot t % 16, entry e = slot * 128 + row:
//   int32 frames, emitted, two unused words                                              16 bytes
//   int32 slot_frame[16]: the frame a slot holds                                         64 bytes
//   int32 mem[2048], prev_frame[2048], prev_row[2048], next_frame[2048], next_row[2048], pos[2048]   49,152 bytes
//   float box[2048][4]: the input box of every row                                       32,768 bytes
//   float post[17][2048]: the member's posterior state, field-major                      139,264 bytes
// All zero bytes are a fresh stream.  Per new frame t, a thread per row, a barrier between the steps:
//   1. stage: k_smo_member's rule with the causal bound 0 <= id < (t + 1) * N - the candidate ids in LDS, a lower row that
//      carries the id takes the membership away; the member id (into the LDS copy of the ring's ids as well), the box and an
//      empty successor go to slot t % 16
//   2. link: k_smo_link's search backwards over the max_gap + 1 frames before t, on the ids in LDS; the predecessor's successor
//      words are written (a frame's member ids differ, so no two rows write the same words)
//   3. forward: kf_start, or kf_predict over the gap and kf_update from the predecessor's stored posterior; the posterior, the
//      predecessor and the position go to the slot
//   4. emit frame t - lag once t >= lag: follow the successor words to the last member at a frame <= t, take its posterior, walk
//      back through the predecessor words with k_smo_seg's backward step (the states of a gap recomputed from a_0, at most 36
//      predicts) to the row itself; sbox and slen
// With flush the frames left are emitted behind the new ones, against the last frame, and the header is zeroed.
// The state's contents are never trusted: the two counts are clamped before they index; a slot counts only if its stored frame
// is the one its place in the window asks for; a (frame, row) word is checked - the row against [0, N), the frame against the
// frames the walk may reach, the target slot's stored frame and member id - before it indexes; a forward walk moves to a
// strictly later frame, a backward one to a strictly earlier one, each at most 16 steps.  Every loop is bounded by F, N, 16 or
// the gap.  A barrier (which orders global memory within the workgroup) stands between every writer and another thread's read.
// No atomics; plain vector loads and stores; the inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_kf.h"
#include "vd_track_smooth_math.h"

namespace {

constexpr int kPushThreads = 256;
constexpr int kRing = 16;                             // frame slots: lag <= 15, max_gap + 1 <= 8
constexpr int kMaxLag = kRing - 1;
constexpr int kEntries = kRing * kMaxN;               // (slot, row) entries of a stream
constexpr int kHeaderBytes = 16;
constexpr int kSlotBytes = 4 * kRing;
constexpr int kWordTables = 6;                        // mem, prev_frame, prev_row, next_frame, next_row, pos
constexpr int kBoxOffset = kHeaderBytes + kSlotBytes + kWordTables * 4 * kEntries;

static_assert(VD_TRACK_SMOOTH_LIVE_STATE_BYTES == kBoxOffset + 16 * kEntries + kStateFloats * 4 * kEntries,
              "the state layout and the header disagree");
static_assert(VD_TRACK_SMOOTH_LIVE_STATE_BYTES % 16 == 0 && kBoxOffset % 16 == 0, "every stream's block and its boxes must stay 16-byte aligned");
static_assert(kMaxAge + 1 <= kRing / 2 && (kRing & (kRing - 1)) == 0, "the ring covers the lag and the widest gap");

struct Ring {
    int32_t* hdr;                                     // frames, emitted, 0, 0
    int32_t* slot_frame;                              // [16]
    int32_t *mem, *prev_f, *prev_r, *next_f, *next_r, *pos;       // [2048] each
    float4* box;                                      // [2048]
    float* post;                                      // [17][2048]
};

__device__ inline Ring ring_of(void* state, int v) {
    char* blk = (char*)state + (int64_t)v * VD_TRACK_SMOOTH_LIVE_STATE_BYTES;
    Ring w;
    w.hdr = (int32_t*)blk;
    w.slot_frame = (int32_t*)(blk + kHeaderBytes);
    w.mem = (int32_t*)(blk + kHeaderBytes + kSlotBytes);
    w.prev_f = w.mem + kEntries;
    w.prev_r = w.prev_f + kEntries;
    w.next_f = w.prev_r + kEntries;
    w.next_r = w.next_f + kEntries;
    w.pos = w.next_r + kEntries;
    w.box = (float4*)(blk + kBoxOffset);
    w.post = (float*)(blk + kBoxOffset + 16 * kEntries);
    return w;
}

__device__ inline int entry_of(int frame, int row) { return (frame & (kRing - 1)) * kMaxN + row; }

__device__ inline void ring_load(const float* st, int e, Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.x[i] = st[(0 + i) * kEntries + e];
        s.xd[i] = st[(3 + i) * kEntries + e];
        s.p00[i] = st[(6 + i) * kEntries + e];
        s.p01[i] = st[(9 + i) * kEntries + e];
        s.p11[i] = st[(12 + i) * kEntries + e];
    }
    s.r = st[15 * kEntries + e];
    s.p = st[16 * kEntries + e];
}

__device__ inline void ring_store(float* st, int e, const Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        st[(0 + i) * kEntries + e] = s.x[i];
        st[(3 + i) * kEntries + e] = s.xd[i];
        st[(6 + i) * kEntries + e] = s.p00[i];
        st[(9 + i) * kEntries + e] = s.p01[i];
        st[(12 + i) * kEntries + e] = s.p11[i];
    }
    st[15 * kEntries + e] = s.r;
    st[16 * kEntries + e] = s.p;
}

// Row `row` of frame u against the horizon h (h - 15 <= u <= h): its smoothed box and the members of its truncated segment.
// s_mem and s_slotf are the LDS copies of the ring's member ids and of the frames its slots hold (-1: none of the window's).
__device__ inline void emit_row(const Ring& w, const int* s_mem, const int* s_slotf, int u, int h, int row, int N, int W,
                                float4& out_box, int& out_len) {
    const int e = entry_of(u, row);
    out_box = w.box[e];
    out_len = 0;
    const int id = s_slotf[u & (kRing - 1)] == u ? s_mem[e] : -1;
    if (id < 0) return;
    // forward through the successor words to the last member at a frame <= h
    int cf = u, cr = row;
    for (int step = 0; step < kRing; ++step) {
        const int ce = entry_of(cf, cr);
        const int nf = w.next_f[ce], nr = w.next_r[ce];
        if (nr < 0 || nr >= N || nf <= cf || nf > h || nf - cf > W) break;        // strictly later, inside the window
        if (s_slotf[nf & (kRing - 1)] != nf || s_mem[entry_of(nf, nr)] != id) break;  // a stale slot ends the walk
        cf = nf, cr = nr;
    }
    const int le = entry_of(cf, cr);
    const int n = (int)((unsigned)w.pos[le] + 1u);
    out_len = n;
    if (n < 2) return;                                // a segment of one keeps its input box
    Kf s;
    ring_load(w.post, le, s);
    Sm S;
#pragma unroll
    for (int k = 0; k < 3; ++k) S.x[k] = s.x[k], S.xd[k] = s.xd[k];
    S.r = s.r;
    // backward through the predecessor words to the row itself
    for (int step = 0; step < kRing && cf > u; ++step) {
        const int ce = entry_of(cf, cr);
        const int pf = w.prev_f[ce], pr = w.prev_r[ce];
        if (pr < 0 || pr >= N || pf >= cf || pf < u || cf - pf > W) return;       // strictly earlier, not behind u
        if (s_slotf[pf & (kRing - 1)] != pf || s_mem[entry_of(pf, pr)] != id) return;
        const int g = cf - pf;
        Kf a0;
        ring_load(w.post, entry_of(pf, pr), a0);
        for (int j = g - 1; j >= 0; --j) {
            Kf f = a0;
            for (int q = 0; q < j; ++q) kf_predict(f);
            Kf p = f;
            kf_predict(p);
            smo_back(S, f, p);
        }
        cf = pf, cr = pr;
    }
    if (cf != u || cr != row) return;                 // only from a state this kernel did not write
    Kf o;                                             // kf_box reads x and r only
#pragma unroll
    for (int k = 0; k < 3; ++k) o.x[k] = S.x[k], o.xd[k] = 0.f, o.p00[k] = 0.f, o.p01[k] = 0.f, o.p11[k] = 0.f;
    o.r = S.r, o.p = 0.f;
    const float4 b = kf_box(o);
    if (finite4(b)) out_box = b;
}

__global__ __launch_bounds__(kPushThreads) void k_smo_push(const float* __restrict__ ids, const float* __restrict__ scores,
                                                           const float* __restrict__ bboxes, const int32_t* __restrict__ track,
                                                           int F, int N, int num_class, int lag, int max_gap, int flush,
                                                           void* state, int m, float4* __restrict__ out_sbox,
                                                           int32_t* __restrict__ out_slen) {
    __shared__ __attribute__((aligned(16))) int s_mem[kEntries];  // the ring's member ids, -1: none and in the rows from N on
    __shared__ int s_slotf[kRing];                    // the frame a slot holds, -1: none of the window's
    __shared__ int s_u[kMaxN];
    const int tid = threadIdx.x;
    const Ring w = ring_of(state, blockIdx.x);
    const int W = max_gap + 1;                        // <= kMaxAge + 1
    int T0 = w.hdr[0], E = w.hdr[1];                  // every thread alike; clamped before either indexes anything
    T0 = T0 < 0 ? 0 : (T0 > 0x7fffffff - F ? 0x7fffffff - F : T0);
    {
        const int lo = T0 > kMaxLag ? T0 - kMaxLag : 0;
        E = E < lo ? lo : (E > T0 ? T0 : E);
    }
    const int E0 = E;
    // the window [T0 - 16, T0): a slot counts iff it holds the frame its place asks for
    if (tid < kRing) {
        int f = -1;
        if (T0 > 0) {
            f = ((T0 - 1) & ~(kRing - 1)) + tid;      // the frame of slot tid in the last frame's block of 16 ...
            if (f > T0 - 1) f -= kRing;               // ... or in the one before
        }
        s_slotf[tid] = (f >= 0 && w.slot_frame[tid] == f) ? f : -1;
    }
    __syncthreads();
    for (int c = tid; c < kEntries; c += kPushThreads) {
        const int slot = c / kMaxN, row = c - slot * kMaxN;
        s_mem[c] = (s_slotf[slot] >= 0 && row < N) ? w.mem[c] : -1;
    }
    __syncthreads();

    const float4* box4 = reinterpret_cast<const float4*>(bboxes);
    const int64_t first = (int64_t)blockIdx.x * F * N;
    const int64_t out0 = (int64_t)blockIdx.x * m * N;
    for (int k = 0; k < F; ++k) {
        const int t = T0 + k;                         // the stream's frame, < 2^31
        const int64_t base = first + (int64_t)k * N;
        const int e = entry_of(t, tid < kMaxN ? tid : 0);
        // 1. stage
        int u = -1;
        float4 my_box = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < N) {
            const int id = track[base + tid];
            if (row_present(ids[base + tid], scores[base + tid], num_class) && id >= 0 && (int64_t)id < ((int64_t)t + 1) * N) u = id;
            s_u[tid] = u;
            my_box = box4[base + tid];
        }
        __syncthreads();
        if (tid < N) {
            bool lower = false;                       // a lower row of the frame carries the id; no early exit: the reads pipeline
            for (int j = 0; j < tid; ++j) lower |= s_u[j] == u;
            if (lower) u = -1;
            s_mem[e] = u;
            w.mem[e] = u;
            w.box[e] = my_box;
            w.next_f[e] = -1;
            w.next_r[e] = -1;
        } else if (tid < kMaxN) {
            s_mem[e] = -1;
        }
        if (tid == 0) {
            s_slotf[t & (kRing - 1)] = t;
            w.slot_frame[t & (kRing - 1)] = t;
        }
        __syncthreads();
        // 2. link and 3. forward
        if (tid < N) {
            int pf = -1, pr = -1, pos = 0;
            if (u >= 0) {
                for (int d = 1; d <= W && pf < 0; ++d) {
                    const int f = t - d;
                    if (f < 0) break;
                    if (s_slotf[f & (kRing - 1)] != f) continue;
                    // a frame's member ids differ and the rows from N on hold -1: at most one hit, so the frame is read four ids
                    // at a time without an early exit and the reads pipeline
                    const int4* row_ids = reinterpret_cast<const int4*>(s_mem + (f & (kRing - 1)) * kMaxN);
                    int hit = -1;
                    for (int j = 0; j < (N + 3) / 4; ++j) {
                        const int4 q = row_ids[j];
                        if (q.x == u) hit = 4 * j;
                        if (q.y == u) hit = 4 * j + 1;
                        if (q.z == u) hit = 4 * j + 2;
                        if (q.w == u) hit = 4 * j + 3;
                    }
                    if (hit >= 0 && hit < N) pf = f, pr = hit;
                }
                Kf s;
                float z[4];
                kf_measure(my_box, z);
                if (pf >= 0) {
                    const int pe = entry_of(pf, pr);
                    ring_load(w.post, pe, s);
                    for (int j = 0; j < t - pf; ++j) kf_predict(s);       // t - pf <= W
                    kf_update(s, z);
                    pos = (int)((unsigned)w.pos[pe] + 1u);
                    w.next_f[pe] = t;
                    w.next_r[pe] = tid;
                } else {
                    kf_start(z, s);
                }
                ring_store(w.post, e, s);
            }
            w.prev_f[e] = pf;
            w.prev_r[e] = pr;
            w.pos[e] = pos;
        }
        __syncthreads();                              // this frame's words and states, its predecessors' successor words
        // 4. emit
        if (t - E >= lag) {                           // every thread alike; t - E <= 15
            const int o = E - E0;
            if (tid < N && o < m) {
                float4 b;
                int n;
                emit_row(w, s_mem, s_slotf, E, t, tid, N, W, b, n);
                out_sbox[out0 + (int64_t)o * N + tid] = b;
                out_slen[out0 + (int64_t)o * N + tid] = n;
            }
            ++E;
        }
        __syncthreads();                              // the ring is read no more before the next frame overwrites a slot
    }
    const int T1 = T0 + F;
    if (flush) {
        for (int step = 0; step < kRing && E < T1; ++step, ++E) {         // T1 - 1 - E <= 14
            const int o = E - E0;
            if (tid < N && o < m) {
                float4 b;
                int n;
                emit_row(w, s_mem, s_slotf, E, T1 - 1, tid, N, W, b, n);
                out_sbox[out0 + (int64_t)o * N + tid] = b;
                out_slen[out0 + (int64_t)o * N + tid] = n;
            }
        }
    }
    // only where the state disagrees with the caller's frame count: the surplus rows, so that every element is written
    for (int o = E - E0; o < m; ++o)
        if (tid < N) {
            out_sbox[out0 + (int64_t)o * N + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
            out_slen[out0 + (int64_t)o * N + tid] = 0;
        }
    __syncthreads();                                  // every thread has read the header and the slots
    if (flush) {
        if (tid < 4) w.hdr[tid] = 0;
        if (tid < kRing) w.slot_frame[tid] = 0;
    } else if (tid == 0) {
        w.hdr[0] = T1, w.hdr[1] = E, w.hdr[2] = 0, w.hdr[3] = 0;
    }
}

}  // namespace

extern "C" {

int vd_track_smooth_push(const float* ids, const float* scores, const float* bboxes, const int32_t* track, int V, int F, int N,
                         int num_class, int lag, int max_gap, int flush, void* state, int64_t state_bytes, int m, float* out_sbox,
                         int32_t* out_slen, void* stream) {
    VD_REQUIRE(N >= 1 && N <= kMaxN, "vd_track_smooth_push: N=%d rows per frame, 1 <= N <= %d are taken", N, kMaxN);
    VD_REQUIRE(F >= 0 && V >= 1, "vd_track_smooth_push: F >= 0 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(num_class >= 1, "vd_track_smooth_push: num_class >= 1 needed, got %d", num_class);
    VD_REQUIRE(lag >= 0 && lag <= kMaxLag, "vd_track_smooth_push: lag=%d, 0 <= lag <= %d are taken", lag, kMaxLag);
    VD_REQUIRE(max_gap >= 0 && max_gap <= kMaxAge, "vd_track_smooth_push: max_gap=%d, 0 <= max_gap <= %d are taken", max_gap, kMaxAge);
    VD_REQUIRE(F == 0 || (ids && scores && bboxes && track),
               "vd_track_smooth_push: ids, scores, bboxes and track must not be NULL with F=%d frames", F);
    VD_REQUIRE(state, "vd_track_smooth_push: state must not be NULL");
    VD_REQUIRE(state_bytes >= (int64_t)VD_TRACK_SMOOTH_LIVE_STATE_BYTES * V, "vd_track_smooth_push: state_bytes=%lld, %d * V = %lld needed",
               (long long)state_bytes, VD_TRACK_SMOOTH_LIVE_STATE_BYTES, (long long)((int64_t)VD_TRACK_SMOOTH_LIVE_STATE_BYTES * V));
    // the frames that become final: without flush one per new frame once the stream is `lag` frames long, with flush all of them
    VD_REQUIRE(flush ? (m >= F && (int64_t)m <= (int64_t)F + lag) : (m <= F && m >= 0 && m >= F - lag),
               "vd_track_smooth_push: m=%d frames cannot become final with F=%d, lag=%d, flush=%d: %s", m, F, lag, flush,
               flush ? "F <= m <= F + lag" : "max(0, F - lag) <= m <= F");
    VD_REQUIRE(m == 0 || (out_sbox && out_slen), "vd_track_smooth_push: the two output pointers must not be NULL with m=%d frames", m);
    VD_REQUIRE((((uintptr_t)bboxes | (uintptr_t)out_sbox | (uintptr_t)state) % 16) == 0,
               "vd_track_smooth_push: bboxes, out_sbox and state must be 16-byte aligned");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)scores | (uintptr_t)track | (uintptr_t)out_slen) % 4) == 0,
               "vd_track_smooth_push: ids, scores, track and out_slen must be 4-byte aligned");
    if (F == 0 && !flush) return VD_OK;               // nothing is taken and nothing becomes final
    hipLaunchKernelGGL(k_smo_push, dim3((unsigned)V), dim3(kPushThreads), 0, (hipStream_t)stream, ids, scores, bboxes, track, F, N,
                       num_class, lag, max_gap, flush, state, m, (float4*)out_sbox, out_slen);
    VD_CHECK_LAUNCH("vd_track_smooth_push");
    return VD_OK;
}

}  // extern "C"
