// fjsp_episode.hip — the slab scans: four reductions of a [T][...][N] rollout slab to records in a
// device-resident log (include/fjsp.h): episode returns (fjsp_episode_scan), the shop-floor KPIs of
// the same episodes (fjsp_kpi_scan), the per-operation schedules compacted from the held-tray words
// (fjsp_schedule_scan) and the packaging runs from the pack words (fjsp_packaging_scan).
//
// The skeleton they share, described here once.  Three launches, ordered by the stream only (no
// flags, no waits between workgroups, no atomics):
//   count    per row t and wave w of 64 envs the number of records the row writes -> temp[t][w],
//            u32 [T][W], W = ceil(N / 64).  The episode and KPI scans write one record per episode
//            end and share k_episode_count; the schedule and packaging scans walk the slab once
//            without writing (k_*_scan<false>)
//   offsets  k_episode_offsets, one workgroup: temp <- its exclusive scan in (t, w) order (the
//            row-major order a sequential reader of the slab meets the records in), the count at
//            entry kept behind the table (`base`), *count advanced by the total
//   write    one lane per env walks t forward; a record's rank is base + temp[t][w] + the records
//            of the lower lanes in that row (a ballot's popcount or a wave prefix sum), and a rank
//            at or past `cap` is counted but not written
// The walk loads EP_U rows in one batch and issues the next batch before the current one is
// consumed (as k_gae): chunk A holds t0.., B is loaded before A's rows are walked, and the other
// way round.  Rows past the slab are clamped to its last row, loaded and never used, so no load
// sits behind a branch.  What an env's open episode has accumulated so far is its carry, int32
// words [WORDS][N] read at the start of a launch and written back at its end; the carry is what
// lets a rollout be scanned chunk by chunk.  The host entries share one front (scan_front: the
// argument checks, the temp layout, W / L / offs / base / flags) and one argument head (ScanHead).
// The A / B loop and the carry's read and write lists are written out in each kernel: behind a
// shared inlined helper (a walk taking load / rows callables, a carry visitor templated on STORE)
// the compiler orders the kernels' instructions differently (profiles/scan_skeleton/README.md).
//
// Episode accounting: MultiAgentA2C.learn's per-episode bookkeeping (a2c.py:311-313
// episode_rewards[agent] += reward, :346-350 total = sum(episode_rewards.values()),
// episode_end_timesteps, :373 the printed steps) for every env of a [T][8][N] slab.
//   k_episode_count    one wave per 64 envs x EP_U rows: per row the popcount of the ballot of
//                      (term | trunc) -> temp[t][w], and per env the chunk's flags as one word
//                      (2 bits per row), u32 [ceil(T / EP_U)][64 W]
//   k_episode_scan     one workgroup of 8 waves per 64 envs, wave a = agent a's running sum of the
//                      64 envs.  Every wave reads the same flag words, so every wave derives the same
//                      rank of an episode end by itself; wave a stores by_agent[a].  Only `total`
//                      needs the eight sums in one place: they go through LDS, one barrier
//                      pair per EP_U rows (unconditional: every wave runs the same T loop), and wave
//                      j % 8 writes the record head of row j's ends (three 16-byte stores).
// The arithmetic is one fp64 add per (step, agent) and the left-to-right sum of the eight, in the
// reference's order; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fjsp.h"

int fjsp_internal_fail(const char* msg);   // fjsp_hip.hip

static_assert(sizeof(fjsp_episode_rec) == 112, "fjsp_episode_rec is 7 x 16 bytes");

namespace {

constexpr int EP_A = FJSP_NUM_AGENTS;
constexpr int EP_U = 16;       // rows per wave of k_episode_count = per load batch of k_episode_scan
constexpr int EPO_THREADS = 1024;

__device__ __forceinline__ int lanes_below(uint64_t ballot, int lane) {
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

// What every scan's arguments end with (the last member of each *Args, so that the pointers in
// front keep their kernarg offsets): the log's capacity, the count at entry (read from temp by the
// write kernel), the slab's first vector step, its first env's global id and its shape.
struct ScanHead {
    long long cap, base, step0;
    uint32_t gid0;
    int T, N;
};

__global__ void __launch_bounds__(256) k_episode_count(const uint8_t* __restrict__ term,
                                                       const uint8_t* __restrict__ trunc, int T, int N, int W,
                                                       uint32_t* __restrict__ cnt, uint32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int chunks = (T + EP_U - 1) / EP_U;
    if (g >= (long long)W * chunks) return;   // whole waves only: no lane of a live wave leaves
    const int w = (int)(g % W), t0 = (int)(g / W) * EP_U;
    const int e = w * 64 + lane;
    uint8_t te[EP_U], tr[EP_U];
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        te[j] = tr[j] = 0;
        if (e < N && t0 + j < T) {
            te[j] = term[(size_t)(t0 + j) * N + e];
            tr[j] = trunc[(size_t)(t0 + j) * N + e];
        }
    }
    uint32_t f = 0;   // bits 2j, 2j + 1 = row t0 + j terminated, truncated
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        const uint32_t fj = (te[j] ? 1u : 0u) | (tr[j] ? 2u : 0u);
        f |= fj << (2 * j);
        const uint64_t b = __ballot(fj != 0);
        if (lane == 0 && t0 + j < T) cnt[(size_t)(t0 + j) * W + w] = (uint32_t)__popcll(b);
    }
    flags[(size_t)(g / W) * ((size_t)W * 64) + e] = f;   // lanes e >= N: 0, inside the padded row
}

// Exclusive scan of cnt[0, L) in place (L = T W < 2^31 / 64, so the sums fit 32 bits): thread i
// owns the elements [i per, (i + 1) per).  base[0] <- *count (the scan kernel's seq base), *count
// advanced by the slab's total.
__global__ void __launch_bounds__(EPO_THREADS) k_episode_offsets(uint32_t* __restrict__ cnt, int L,
                                                                 long long* __restrict__ base,
                                                                 long long* __restrict__ count) {
    __shared__ uint32_t wsum[EPO_THREADS / 64];
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    const int per = (L + EPO_THREADS - 1) / EPO_THREADS;
    const int lo = min(i * per, L), hi = min(lo + per, L);
    uint32_t s = 0;
    for (int k = lo; k < hi; k++) s += cnt[k];
    uint32_t inc = s;   // inclusive scan of the threads' sums: within the wave, then over the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < EPO_THREADS / 64; k++) {
        if (k < wave) before += wsum[k];
        total += wsum[k];
    }
    uint32_t run = before + inc - s;
    for (int k = lo; k < hi; k++) {
        const uint32_t c = cnt[k];
        cnt[k] = run;
        run += c;
    }
    if (i == 0) {
        const long long c0 = *count;
        base[0] = c0;
        *count = c0 + (long long)total;
    }
}

struct EpChunk {
    double r[EP_U];
    uint32_t off[EP_U];
    uint32_t f;   // k_episode_count's flag word: 2 bits per row (terminated, truncated), 0 past the slab
};

// The loads of rows t0 .. t0 + EP_U - 1 (rows past the slab clamped to its last row: never used,
// and no branch around a load).  GUARD: the workgroup holding lanes e >= N, which load nothing
// from the slab (their flag words are 0 in temp's padded rows).
template <bool GUARD>
__device__ __forceinline__ void ep_load(EpChunk& c, const double* __restrict__ r, const uint32_t* __restrict__ flags,
                                        const uint32_t* __restrict__ offs, int t0, int T, int N, int W, int a, int e,
                                        int w, bool live) {
    const int ch = (t0 < T ? t0 : T - 1) / EP_U;
    c.f = flags[(size_t)ch * ((size_t)W * 64) + e];
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        const int t = t0 + j < T ? t0 + j : T - 1;
        // wave-uniform row pointers + the lane's 32-bit column: scalar base, vector offset
        const double* __restrict__ rr = r + ((size_t)t * EP_A + a) * N;
        c.off[j] = offs[(size_t)t * W + w];
        c.r[j] = 0.0;
        if (!GUARD || live) c.r[j] = rr[e];
    }
}

struct EpArgs {
    const int32_t* oc;
    const int32_t* pk;
    fjsp_episode_rec* recs;
    ScanHead h;
};

// Rows t0 .. t0 + EP_U - 1 of one agent's 64 envs; sh[j][a][lane] = the agent's sum at an end in
// row j.  Two barriers, reached by every wave of the workgroup for every chunk.  The episode's
// length follows from the flag word alone: the rows since the chunk's previous end, or the open
// episode's steps at the chunk's start (len) plus the rows up to this one.
__device__ __forceinline__ void ep_scan(const EpChunk& c, const uint32_t* __restrict__ offs, int t0, const EpArgs& p,
                                        int W, int a, int w, int e, int lane, double& acc, int& len,
                                        double (*sh)[EP_A][64]) {
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        const bool done = ((c.f >> (2 * j)) & 3u) != 0;   // never set past the slab
        const uint64_t b = __ballot(done);
        if (t0 + j < p.h.T) acc = acc + c.r[j];             // wave-uniform
        if (done) {
            const long long seq = p.h.base + (long long)c.off[j] + lanes_below(b, lane);
            if ((unsigned long long)seq < (unsigned long long)p.h.cap) p.recs[seq].by_agent[a] = acc;
            sh[j][a][lane] = acc;
            acc = 0.0;
        }
    }
    __syncthreads();
    for (int h = 0; h < EP_U / EP_A; h++) {   // wave a writes the heads of rows a and a + 8
        const int j = a + EP_A * h;
        const uint32_t fj = (c.f >> (2 * j)) & 3u;
        const uint64_t b = __ballot(fj != 0);
        if (fj != 0) {
            const size_t t = (size_t)(t0 + j);
            const long long seq = p.h.base + (long long)offs[t * W + w] + lanes_below(b, lane);
            if ((unsigned long long)seq < (unsigned long long)p.h.cap) {
                double total = 0.0;
#pragma unroll
                for (int k = 0; k < EP_A; k++) total = total + sh[j][k][lane];
                const uint32_t prior = c.f & ((1u << (2 * j)) - 1u);
                const int length = prior ? j - ((31 - __clz(prior)) >> 1) : len + j + 1;
                const size_t at = t * p.h.N + e;
                const int oc = p.oc ? p.oc[at] : -1, pk = p.pk ? p.pk[at] : -1;
                const long long end = p.h.step0 + (long long)t + 1;
                uint4* q = reinterpret_cast<uint4*>(p.recs + seq);
                q[0] = make_uint4(p.h.gid0 + (uint32_t)e, (uint32_t)length, (uint32_t)end,
                                  (uint32_t)((unsigned long long)end >> 32));
                q[1] = make_uint4((uint32_t)seq, (uint32_t)((unsigned long long)seq >> 32), fj, (uint32_t)oc);
                const unsigned long long tb = (unsigned long long)__double_as_longlong(total);
                q[2] = make_uint4((uint32_t)pk, 0u, (uint32_t)tb, (uint32_t)(tb >> 32));
            }
        }
    }
    const int rows = min(EP_U, p.h.T - t0);
    len = c.f ? rows - 1 - ((31 - __clz(c.f)) >> 1) : len + rows;
    __syncthreads();
}

template <bool GUARD>
__device__ __forceinline__ void ep_body(const double* __restrict__ r, const uint32_t* __restrict__ flags,
                                        const uint32_t* __restrict__ offs, const EpArgs& p, int W,
                                        double* __restrict__ accp, int32_t* __restrict__ lenp,
                                        double (*sh)[EP_A][64]) {
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = blockIdx.x, e = w * 64 + lane;
    const int T = p.h.T, N = p.h.N;
    const bool live = !GUARD || e < N;
    double acc = 0.0;
    int len = 0;
    if (live) {
        acc = accp[(size_t)a * N + e];
        len = lenp[e];
    }
    EpChunk A, B;
    int t0 = 0;
    ep_load<GUARD>(A, r, flags, offs, 0, T, N, W, a, e, w, live);
    for (;;) {   // the A / B walk, written out: a shared helper changes the kernel's code (file header)
        ep_load<GUARD>(B, r, flags, offs, t0 + EP_U, T, N, W, a, e, w, live);
        ep_scan(A, offs, t0, p, W, a, w, e, lane, acc, len, sh);
        t0 += EP_U;
        if (t0 >= T) break;
        ep_load<GUARD>(A, r, flags, offs, t0 + EP_U, T, N, W, a, e, w, live);
        ep_scan(B, offs, t0, p, W, a, w, e, lane, acc, len, sh);
        t0 += EP_U;
        if (t0 >= T) break;
    }
    if (live) {
        accp[(size_t)a * N + e] = acc;
        if (a == 0) lenp[e] = len;
    }
}

__global__ void __launch_bounds__(64 * EP_A) k_episode_scan(const double* __restrict__ r,
                                                            const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ offs,
                                                            const long long* __restrict__ base, EpArgs p, int W,
                                                            double* __restrict__ accp,
                                                            int32_t* __restrict__ lenp) {
    __shared__ double sh[EP_U][EP_A][64];
    p.h.base = base[0];
    if ((int)blockIdx.x * 64 + 64 <= p.h.N) ep_body<false>(r, flags, offs, p, W, accp, lenp, sh);
    else ep_body<true>(r, flags, offs, p, W, accp, lenp, sh);
}

// ---- shop-floor KPIs (include/fjsp.h: fjsp_kpi_scan) -------------------------------------------
// The same three launches with k_kpi_scan in k_episode_scan's place: one workgroup of 8 waves per
// 64 envs, wave a = agent a's eight result counters of the 64 envs.  Waves 0 and 1 also
// follow one infos counter each (orders_completed / packaged -> the completion-time blocks); wave 0
// writes the record's first 32 bytes (up to orders_completed), wave 1, which holds packaged, the
// next 16 (packaged, reserved, makespan: it also batches sim_time); waves 2..7 read their station's
// two obs_i8 rows.  Every wave reads the same flag words and offsets, so every wave derives the
// same rank by itself and stores only its own 16-byte segments of the record: no LDS, no barrier,
// no atomic.  Nothing is loaded at an episode's end (vmcnt retires in order, so such a load would
// wait for the whole next batch already in flight), and no load sits behind a branch.
// What makes the missing barrier safe: no word of global memory that one wave writes is read or
// written by another wave of the launch.  Every carry word and every 16-byte record segment has
// exactly one owner wave (the inputs, flags and offsets are read-only here).  That is why the open
// episode's length is carried twice: waves 0 and 1 both need it (the head's length, the step index
// l of both completion-time blocks), and each reads and writes a word of its own, so wave 1's read
// at its start cannot meet wave 0's write at its end.  The station waves need no length.
constexpr int KPI_C_LEN = 0;         // carry words [KPI_WORDS][N]: steps of the open episode, wave 0's copy
constexpr int KPI_C_TIMES = 1;       // + 5 i: first, last, step_sum lo / hi, previous value (i = 0 orders, 1 products)
constexpr int KPI_C_AGENTS = 11;     // + 8 a + k
constexpr int KPI_C_STATIONS = 75;   // + 3 s + {busy_steps, queue_sum, queue_max}
constexpr int KPI_C_LEN1 = 93;       // steps of the open episode, wave 1's copy (equal to word 0)
constexpr int KPI_WORDS = 94;
constexpr int KPI_Q_TIMES = 3, KPI_Q_AGENTS = 5, KPI_Q_STATIONS = 21;   // record segments, in 16 bytes

static_assert(sizeof(fjsp_kpi_rec) == FJSP_KPI_REC_BYTES && FJSP_KPI_REC_BYTES % 16 == 0, "fjsp_kpi_rec is 27 x 16 bytes");
static_assert(offsetof(fjsp_kpi_rec, makespan) == 40 && offsetof(fjsp_episode_rec, total) == 40, "shared 40-byte head");
static_assert(offsetof(fjsp_kpi_rec, orders) == 16 * KPI_Q_TIMES && offsetof(fjsp_kpi_rec, agents) == 16 * KPI_Q_AGENTS &&
                  offsetof(fjsp_kpi_rec, stations) == 16 * KPI_Q_STATIONS, "record segments");

struct KpiArgs {
    const uint32_t* res;
    const int8_t* obs;
    const int32_t* oc;
    const int32_t* pk;
    const double* st;
    fjsp_kpi_rec* recs;
    int32_t* carry;
    ScanHead h;
};

struct KpiChunk {
    uint32_t word[EP_U];
    int32_t x[EP_U], y[EP_U];   // station waves: is_busy, queue_length; waves 0 / 1: the infos counter, -
    double st[EP_U];            // wave 1: sim_time
    uint32_t off[EP_U];
    uint32_t f;
};

struct KpiState {
    uint32_t c[8];
    uint32_t busy, qsum;
    int32_t qmax;
    int32_t len, first, last, prev;
    unsigned long long sum;
};

// What one wave loads per row, wave-uniform: a base, a row stride and the lane's byte offset.  A slab
// that was not given reads the first words of the flag table instead (stride and lane offset 0) and
// is masked to 0: no branch around a load, so no load's first use can move up to the load.
struct KpiRows {
    const char* res;   // the agent's result words, u32
    const char* aux;   // station waves: is_busy bytes (queue_length `queue` bytes on); waves 0 / 1: the infos counter, i32
    const char* st;    // wave 1: sim_time, f64
    size_t res_stride, aux_stride, st_stride, queue;
    uint32_t res_lane, aux_lane, st_lane;
    uint32_t res_mask;
    int32_t aux_mask;
};

// Rows t0 .. t0 + EP_U - 1 (rows past the slab clamped to its last row: never used).  ROLE 0 / 1 /
// 2 = wave 0 / wave 1 / a station wave.
template <int ROLE>
__device__ __forceinline__ void kpi_load(KpiChunk& c, const KpiRows& r, const uint32_t* __restrict__ flags,
                                         const uint32_t* __restrict__ offs, int t0, int T, int W, uint32_t e, int w) {
    const int ch = (t0 < T ? t0 : T - 1) / EP_U;
    c.f = flags[(size_t)ch * ((size_t)W * 64) + e];
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        const size_t t = (size_t)(t0 + j < T ? t0 + j : T - 1);
        c.off[j] = offs[t * W + w];
        // scalar row base + the lane's 32-bit byte offset
        c.word[j] = *reinterpret_cast<const uint32_t*>(r.res + t * r.res_stride + r.res_lane) & r.res_mask;
        const char* __restrict__ ax = r.aux + t * r.aux_stride;
        if (ROLE == 2) {
            c.x[j] = (int32_t)(*reinterpret_cast<const int8_t*>(ax + r.aux_lane)) & r.aux_mask;
            c.y[j] = (int32_t)(*reinterpret_cast<const int8_t*>(ax + r.queue + r.aux_lane)) & r.aux_mask;
        } else {
            c.x[j] = *reinterpret_cast<const int32_t*>(ax + r.aux_lane) & r.aux_mask;
            c.y[j] = 0;
        }
        c.st[j] = 0.0;
        if (ROLE == 1) c.st[j] = *reinterpret_cast<const double*>(r.st + t * r.st_stride + r.st_lane);
    }
}

template <int ROLE>
__device__ __forceinline__ void kpi_scan(const KpiChunk& c, int t0, const KpiArgs& p, int a, int e, int lane,
                                         KpiState& s) {
    const int rows = min(EP_U, p.h.T - t0);
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        if (j < rows) {   // wave-uniform
            const uint32_t wd = c.word[j];
            s.len += 1;
#pragma unroll
            for (int k = 0; k < 6; k++) s.c[k] += (wd >> k) & 1u;
            s.c[6] += (wd >> 7) & 1u;
            s.c[7] += wd >> 16;
            if (ROLE == 2) {
                s.busy += c.x[j] != 0 ? 1u : 0u;
                s.qsum += (uint32_t)c.y[j];
                s.qmax = max(s.qmax, c.y[j]);
            } else {
                const long long d = (long long)c.x[j] - (long long)s.prev;
                if (d > 0) {
                    if (s.first == 0) s.first = s.len;
                    s.last = s.len;
                    s.sum += (unsigned long long)d * (unsigned long long)s.len;
                }
                s.prev = c.x[j];
            }
        }
        const uint32_t fj = (c.f >> (2 * j)) & 3u;   // never set past the slab
        const uint64_t b = __ballot(fj != 0);
        if (fj != 0) {
            const long long seq = p.h.base + (long long)c.off[j] + lanes_below(b, lane);
            if ((unsigned long long)seq < (unsigned long long)p.h.cap) {
                uint4* q = reinterpret_cast<uint4*>(p.recs + seq);
                if (ROLE != 2) {
                    // the 48 bytes in front: wave 0 the 32 that end with orders_completed, wave 1 the 16
                    // of packaged and makespan; each from its own batch (a load issued here would
                    // have to wait for the whole batch in flight behind it)
                    if (ROLE == 0) {
                        const int oc = p.oc ? c.x[j] : -1;
                        const long long end = p.h.step0 + (long long)(t0 + j) + 1;
                        q[0] = make_uint4(p.h.gid0 + (uint32_t)e, (uint32_t)s.len, (uint32_t)end,
                                          (uint32_t)((unsigned long long)end >> 32));
                        q[1] = make_uint4((uint32_t)seq, (uint32_t)((unsigned long long)seq >> 32), fj, (uint32_t)oc);
                    } else {
                        const int pk = p.pk ? c.x[j] : -1;
                        const unsigned long long mk =
                            p.st ? (unsigned long long)__double_as_longlong(c.st[j]) : 0x7FF8000000000000ull;
                        q[2] = make_uint4((uint32_t)pk, 0u, (uint32_t)mk, (uint32_t)(mk >> 32));
                    }
                    q[KPI_Q_TIMES + a] = make_uint4((uint32_t)s.first, (uint32_t)s.last, (uint32_t)s.sum,
                                                    (uint32_t)(s.sum >> 32));
                } else {
                    q[KPI_Q_STATIONS + a - 2] = make_uint4(s.busy, s.qsum, (uint32_t)s.qmax, 0u);
                }
                q[KPI_Q_AGENTS + 2 * a] = make_uint4(s.c[0], s.c[1], s.c[2], s.c[3]);
                q[KPI_Q_AGENTS + 2 * a + 1] = make_uint4(s.c[4], s.c[5], s.c[6], s.c[7]);
            }
            s = KpiState{};
        }
    }
}

template <int ROLE>
__device__ __forceinline__ void kpi_body(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                                         const KpiArgs& p, int W, int w, int a) {
    const int lane = threadIdx.x & 63;
    const int e = w * 64 + lane;
    const int T = p.h.T;
    const size_t N = (size_t)p.h.N, col = (size_t)w * 64;
    const bool live = e < p.h.N;
    // lanes e >= N load their workgroup's last env's column; their flag words are 0 (temp's padded
    // rows), so they end no episode, and their carry is neither read nor written
    const uint32_t ll = (uint32_t)min(lane, p.h.N - w * 64 - 1);
    const char* none = reinterpret_cast<const char*>(flags);
    const int32_t* info = ROLE == 0 ? p.oc : p.pk;
    KpiRows r;
    r.res = p.res ? reinterpret_cast<const char*>(p.res + (size_t)a * N + col) : none;
    r.res_stride = p.res ? (size_t)EP_A * N * 4 : 0;
    r.res_lane = p.res ? ll * 4u : 0u;
    r.res_mask = p.res ? ~0u : 0u;
    if (ROLE == 2) {
        r.aux = p.obs ? reinterpret_cast<const char*>(p.obs + (size_t)(2 * (a - 2)) * N + col) : none;
        r.aux_stride = p.obs ? (size_t)FJSP_OBS_I8 * N : 0;
        r.queue = p.obs ? N : 0;
        r.aux_lane = p.obs ? ll : 0u;
        r.aux_mask = p.obs ? -1 : 0;
    } else {
        r.aux = info ? reinterpret_cast<const char*>(info + col) : none;
        r.aux_stride = info ? N * 4 : 0;
        r.queue = 0;
        r.aux_lane = info ? ll * 4u : 0u;
        r.aux_mask = info ? -1 : 0;
    }
    const bool has_st = ROLE == 1 && p.st;
    r.st = has_st ? reinterpret_cast<const char*>(p.st + col) : none;
    r.st_stride = has_st ? N * 8 : 0;
    r.st_lane = has_st ? ll * 8u : 0u;
    int32_t* __restrict__ cy = p.carry + e;   // word k of this env: cy[k * N]
    const int ca = KPI_C_AGENTS + 8 * a, cs = KPI_C_STATIONS + 3 * (a - 2), ct = KPI_C_TIMES + 5 * a;
    const int cl = ROLE == 0 ? KPI_C_LEN : KPI_C_LEN1;   // each of the two waves its own word (see above)
    KpiState s{};
    if (live) {
        if (ROLE != 2) s.len = cy[(size_t)cl * N];
#pragma unroll
        for (int k = 0; k < 8; k++) s.c[k] = (uint32_t)cy[(size_t)(ca + k) * N];
        if (ROLE == 2) {
            s.busy = (uint32_t)cy[(size_t)cs * N];
            s.qsum = (uint32_t)cy[(size_t)(cs + 1) * N];
            s.qmax = cy[(size_t)(cs + 2) * N];
        } else {
            s.first = cy[(size_t)ct * N];
            s.last = cy[(size_t)(ct + 1) * N];
            s.sum = (unsigned long long)(uint32_t)cy[(size_t)(ct + 2) * N] |
                    ((unsigned long long)(uint32_t)cy[(size_t)(ct + 3) * N] << 32);
            s.prev = cy[(size_t)(ct + 4) * N];
        }
    }
    KpiChunk A, B;
    int t0 = 0;
    kpi_load<ROLE>(A, r, flags, offs, 0, T, W, (uint32_t)e, w);
    for (;;) {   // the A / B walk, written out: a shared helper changes the kernel's code (file header)
        kpi_load<ROLE>(B, r, flags, offs, t0 + EP_U, T, W, (uint32_t)e, w);
        kpi_scan<ROLE>(A, t0, p, a, e, lane, s);
        t0 += EP_U;
        if (t0 >= T) break;
        kpi_load<ROLE>(A, r, flags, offs, t0 + EP_U, T, W, (uint32_t)e, w);
        kpi_scan<ROLE>(B, t0, p, a, e, lane, s);
        t0 += EP_U;
        if (t0 >= T) break;
    }
    if (live) {   // the read list's mirror, written out: a STORE-templated visitor changes the kernel's code
        if (ROLE != 2) cy[(size_t)cl * N] = s.len;
#pragma unroll
        for (int k = 0; k < 8; k++) cy[(size_t)(ca + k) * N] = (int32_t)s.c[k];
        if (ROLE == 2) {
            cy[(size_t)cs * N] = (int32_t)s.busy;
            cy[(size_t)(cs + 1) * N] = (int32_t)s.qsum;
            cy[(size_t)(cs + 2) * N] = s.qmax;
        } else {
            cy[(size_t)ct * N] = s.first;
            cy[(size_t)(ct + 1) * N] = s.last;
            cy[(size_t)(ct + 2) * N] = (int32_t)(uint32_t)s.sum;
            cy[(size_t)(ct + 3) * N] = (int32_t)(uint32_t)(s.sum >> 32);
            cy[(size_t)(ct + 4) * N] = s.prev;
        }
    }
}

__global__ void __launch_bounds__(64 * EP_A) k_kpi_scan(const uint32_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ offs,
                                                        const long long* __restrict__ base, KpiArgs p, int W) {
    p.h.base = base[0];
    const int w = (int)blockIdx.x;
    const int a = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (a == 0) kpi_body<0>(flags, offs, p, W, w, a);
    else if (a == 1) kpi_body<1>(flags, offs, p, W, w, a);
    else kpi_body<2>(flags, offs, p, W, w, a);
}

// ---- per-operation schedules (include/fjsp.h: fjsp_schedule_scan) ------------------------------
// How many records a row writes depends on the ops open at that row, so the walk runs twice with
// k_episode_offsets between: k_schedule_scan<false> counts, k_schedule_scan<true> writes.  Both are
// one wave per 64 envs; per row and env they load the three result words of agents 1..3, the three
// held-tray words and the two flags, 26 bytes.
//   count  per row the three ballots of "resource r writes a record" -> cnt[t][w] = their popcounts'
//          sum (lane 0); the carry is read, never written
//   write  the same walk; a record's rank is offs[t][w] + the records of the lower lanes in the
//          three ballots + the lane's own lower resources, i.e. row-major (t, env, resource); the
//          carry is written back at the end
// A wave touches only its own cnt words, its envs' carry words and the records of its own ranks;
// launch boundaries are the only ordering between waves.
constexpr int SC_LEN = 0;      // carry words [SC_WORDS][N]: steps of the open episode,
constexpr int SC_OP = 1;       // + 2 r: the open op's word (open 0 | tray code [1,14) | from [16,20)), + 1: its start step
constexpr int SC_WORDS = 7;
constexpr int SC_R = 3;        // resources: agent 1 + r
constexpr uint32_t SC_MACHINE_LOC[SC_R] = {0u, 3u, 2u};   // LocationType SMALL_MACHINE = 3, BIG_MACHINE = 2

static_assert(sizeof(fjsp_op_rec) == FJSP_OP_REC_BYTES && FJSP_OP_REC_BYTES == 32, "fjsp_op_rec is 2 x 16 bytes");
static_assert(offsetof(fjsp_op_rec, episode_start) == 8 && offsetof(fjsp_op_rec, tray) == 16, "record halves");

struct SchedArgs {
    const uint32_t* res;
    const uint32_t* held;
    const uint8_t* term;
    const uint8_t* trunc;
    fjsp_op_rec* recs;
    int32_t* carry;
    ScanHead h;
};

struct SchedChunk {
    uint32_t res[SC_R][EP_U], held[SC_R][EP_U];
    uint8_t te[EP_U], tr[EP_U];
    uint32_t off[EP_U];
};

// Rows t0 .. t0 + EP_U - 1 of the column `col` (rows past the slab clamped to its last row, lanes
// past the envs to the last env: loaded, never used).  No branch around a load.
template <bool WRITE>
__device__ __forceinline__ void sched_load(SchedChunk& c, const SchedArgs& p, const uint32_t* __restrict__ offs, int t0,
                                           int W, int w, uint32_t col) {
    const size_t N = (size_t)p.h.N;
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        const size_t t = (size_t)(t0 + j < p.h.T ? t0 + j : p.h.T - 1);
        const uint32_t* __restrict__ rr = p.res + (t * EP_A + 1) * N;
        const uint32_t* __restrict__ hr = p.held + t * SC_R * N;
#pragma unroll
        for (int r = 0; r < SC_R; r++) {
            c.res[r][j] = rr[(size_t)r * N + col];
            c.held[r][j] = hr[(size_t)r * N + col];
        }
        c.te[j] = p.term[t * N + col];
        c.tr[j] = p.trunc[t * N + col];
        c.off[j] = WRITE ? offs[t * W + w] : 0u;
    }
}

struct SchedState {
    int32_t len;
    uint32_t op[SC_R];
    int32_t start[SC_R];
};

template <bool WRITE>
__device__ __forceinline__ void sched_rows(const SchedChunk& c, int t0, const SchedArgs& p, uint32_t* __restrict__ cnt,
                                           int W, int w, int e, int lane, bool live, SchedState& s) {
    const int rows = min(EP_U, p.h.T - t0);
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        if (j < rows) {   // wave-uniform
            const bool end = (c.te[j] | c.tr[j]) != 0;
            bool emit[SC_R];
            uint32_t info[SC_R], tray[SC_R];
            int32_t st[SC_R], en[SC_R];
            uint64_t b[SC_R];
    #pragma unroll
            for (int r = 0; r < SC_R; r++) {
                const uint32_t rw = c.res[r][j], hw = c.held[r][j];
                const uint32_t loc = r == 0 ? (hw >> FJSP_HELD_LOC_SHIFT) & 7u : SC_MACHINE_LOC[r];
                const bool opens = r == 0 ? (rw & 8u) != 0 : (rw & 2u) != 0;   // pickup_success / started_processing
                if (opens) {
                    s.op[r] = 1u | ((hw & FJSP_HELD_CODE_MASK) << 1) | (loc << 16);
                    s.start[r] = s.len;
                }
                const bool open = (s.op[r] & 1u) != 0;
                const bool fin = open && (r == 0 ? (rw & 16u) != 0 : (hw & FJSP_HELD_BUSY) == 0);   // drop_success / is_busy fell
                emit[r] = live && open && (fin || end);
                const uint32_t from = (s.op[r] >> 16) & 15u;
                const uint32_t to = r == 0 ? (fin ? loc : 0u) : from;
                info[r] = (uint32_t)(1 + r) | (fin ? 1u << 8 : 0u) | (from << 16) | (to << 20);
                tray[r] = (s.op[r] >> 1) & FJSP_HELD_CODE_MASK;
                st[r] = s.start[r];
                en[r] = fin ? s.len : -1;
                if (open && (fin || end)) {
                    s.op[r] = 0u;
                    s.start[r] = 0;
                }
                b[r] = __ballot(emit[r]);
            }
            if (!WRITE) {
                if (lane == 0) cnt[(size_t)(t0 + j) * W + w] = (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]));
            } else {
                long long rank = p.h.base + (long long)c.off[j] + lanes_below(b[0], lane) + lanes_below(b[1], lane) +
                                 lanes_below(b[2], lane);
                const long long es = p.h.step0 + (long long)(t0 + j) - (long long)s.len;
    #pragma unroll
                for (int r = 0; r < SC_R; r++) {
                    if (emit[r]) {
                        if ((unsigned long long)rank < (unsigned long long)p.h.cap) {
                            uint4* q = reinterpret_cast<uint4*>(p.recs + rank);
                            q[0] = make_uint4(p.h.gid0 + (uint32_t)e, info[r], (uint32_t)es, (uint32_t)((unsigned long long)es >> 32));
                            q[1] = make_uint4(tray[r], (uint32_t)st[r], (uint32_t)en[r], 0u);
                        }
                        rank += 1;
                    }
                }
            }
            s.len = end ? 0 : s.len + 1;
        }
    }
}

template <bool WRITE>
__global__ void __launch_bounds__(64) k_schedule_scan(SchedArgs p, uint32_t* __restrict__ cnt,
                                                      const long long* __restrict__ base, int W) {
    if (WRITE) p.h.base = base[0];
    const int lane = threadIdx.x, w = (int)blockIdx.x;
    const int e = w * 64 + lane;
    const bool live = e < p.h.N;
    const uint32_t col = (uint32_t)min(e, p.h.N - 1);
    const size_t N = (size_t)p.h.N;
    int32_t* __restrict__ cy = p.carry + col;   // word k of this env: cy[k * N]
    SchedState s{};
    s.len = cy[(size_t)SC_LEN * N];
#pragma unroll
    for (int r = 0; r < SC_R; r++) {
        s.op[r] = (uint32_t)cy[(size_t)(SC_OP + 2 * r) * N];
        s.start[r] = cy[(size_t)(SC_OP + 2 * r + 1) * N];
    }
    SchedChunk A, B;
    int t0 = 0;
    sched_load<WRITE>(A, p, cnt, 0, W, w, col);
    for (;;) {   // the A / B walk, written out: a shared helper changes the kernel's code (file header)
        sched_load<WRITE>(B, p, cnt, t0 + EP_U, W, w, col);
        sched_rows<WRITE>(A, t0, p, cnt, W, w, e, lane, live, s);
        t0 += EP_U;
        if (t0 >= p.h.T) break;
        sched_load<WRITE>(A, p, cnt, t0 + EP_U, W, w, col);
        sched_rows<WRITE>(B, t0, p, cnt, W, w, e, lane, live, s);
        t0 += EP_U;
        if (t0 >= p.h.T) break;
    }
    if (WRITE && live) {   // the read list's mirror, written out: a STORE-templated visitor changes the kernel's code
        cy[(size_t)SC_LEN * N] = s.len;
#pragma unroll
        for (int r = 0; r < SC_R; r++) {
            cy[(size_t)(SC_OP + 2 * r) * N] = (int32_t)s.op[r];
            cy[(size_t)(SC_OP + 2 * r + 1) * N] = s.start[r];
        }
    }
}

// ---- packaging runs (include/fjsp.h: fjsp_packaging_scan) --------------------------------------
// One record per tray run at a packaging station.  Per station the runs are FIFO (arrival order =
// grant order = completion order), so the records a row writes follow from the pack words'
// counters and the walk keeps k_schedule_scan's shape: k_packaging_scan<false> counts,
// k_episode_offsets, k_packaging_scan<true> writes; one wave per 64 envs.  Per row and env: the
// result words of the AGV and the four stations, the AGV's held word, the four pack words and the
// two flags, 42 bytes.
//   count  a lane's records of a row = sum over s of the runs that left station s's FIFO, plus at
//          an episode end the runs still in it; the lanes' sum -> cnt[t][w] (lane 0).  Needs the
//          words and the carry only (never the rings), writes neither
//   write  the FIFO work.  A lane can write many records in one row, so its rank is offs[t][w] +
//          an exclusive wave prefix sum of the lanes' counts (shuffles), taken only in rows where
//          some lane writes; the loops at an arrival, a START and a completion sit behind
//          wave-uniform branches of their own.  Records in (t, env, station, FIFO position) order
// FIFO: ring u32 [4][PK_RING][N] (lane-contiguous), entry = tray code [0,13) | granted 13 |
// start << 16; 8-bit head / granted / tail indices (the arena's 255 slots bound an env's pending
// runs, so 256 entries cannot overflow; a fuller FIFO could only come from rows that are not one
// env's, and then wraps inside the env's own ring).  The FIFO's length, not runs(prev), is what the
// departures are taken from (clamped to what the FIFO holds): the two are equal whenever the scan
// has seen the episode from its first row, and a log attached mid-episode stays self-consistent.
constexpr int PK_LEN = 0;      // carry words [PK_WORDS][N]: steps of the open episode,
constexpr int PK_HPREV = 1;    // the AGV's held word of the previous row,
constexpr int PK_PREV = 2;     // + s: station s's pack word of the previous row,
constexpr int PK_IDX = 6;      // + s: head [0,8) | first ungranted [8,16) | tail [16,24) of its ring
constexpr int PK_WORDS = 10;
constexpr int PK_S = 4;        // stations: agent 4 + s
constexpr int PK_RING = 256;
constexpr uint32_t PK_GRANTED = 1u << 13;

struct PackArgs {
    const uint32_t* res;
    const uint32_t* held;
    const uint32_t* pack;
    const uint8_t* term;
    const uint8_t* trunc;
    fjsp_op_rec* recs;
    int32_t* carry;
    uint32_t* ring;
    ScanHead h;
};

template <bool WRITE>
struct PackChunk {
    uint32_t agv[EP_U], pk[PK_S][EP_U];
    uint32_t st[WRITE ? PK_S : 1][EP_U], held[EP_U];   // the count pass loads neither
    uint8_t te[EP_U], tr[EP_U];
    uint32_t off[EP_U];
};

template <bool WRITE>
__device__ __forceinline__ void pack_load(PackChunk<WRITE>& c, const PackArgs& p, const uint32_t* __restrict__ offs, int t0,
                                          int W, int w, uint32_t col) {
    const size_t N = (size_t)p.h.N;
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        const size_t t = (size_t)(t0 + j < p.h.T ? t0 + j : p.h.T - 1);
        const uint32_t* __restrict__ rr = p.res + t * EP_A * N;
        const uint32_t* __restrict__ pr = p.pack + t * PK_S * N;
        c.agv[j] = rr[N + col];
#pragma unroll
        for (int s = 0; s < PK_S; s++) {
            c.pk[s][j] = pr[(size_t)s * N + col];
            if constexpr (WRITE) c.st[s][j] = rr[(size_t)(4 + s) * N + col];
        }
        if constexpr (WRITE) c.held[j] = p.held[t * SC_R * N + col];
        c.te[j] = p.term[t * N + col];
        c.tr[j] = p.trunc[t * N + col];
        c.off[j] = WRITE ? offs[t * W + w] : 0u;
    }
}

struct PackState {
    int32_t len;
    uint32_t hprev;
    uint32_t prev[PK_S], idx[PK_S];
};

__device__ __forceinline__ uint32_t pk_total(uint32_t w) { return ((w >> 8) & 0xFFFu) + (w >> 20); }   // pending + completed

template <bool WRITE>
__device__ __forceinline__ void pack_rows(const PackChunk<WRITE>& c, int t0, const PackArgs& p, uint32_t* __restrict__ cnt,
                                          int W, int w, int e, int lane, bool live, PackState& s) {
    const int rows = min(EP_U, p.h.T - t0);
    const size_t N = (size_t)p.h.N;
    uint32_t* __restrict__ ring = p.ring + (live ? e : 0);   // entry i of station q: ring[(q * PK_RING + i) * N]
#pragma unroll
    for (int j = 0; j < EP_U; j++) {
        if (j < rows) {   // wave-uniform
            const bool end = (c.te[j] | c.tr[j]) != 0;
            const bool drop = (c.agv[j] & 0x30u) == 0x30u;   // drop_success and delivered_to_packaging
            uint32_t leave[PK_S], rest[PK_S];
            uint32_t n = 0, arr = 0;   // arr: bit q = a run joins station q (at most one)
#pragma unroll
            for (int q = 0; q < PK_S; q++) {
                const uint32_t now = c.pk[q][j];
                const bool arrived = drop && pk_total(now) > pk_total(s.prev[q]);
                const uint32_t have = ((s.idx[q] >> 16) - s.idx[q] & 0xFFu) + (arrived ? 1u : 0u);
                const uint32_t stay = min(now & 0xFFu, have);
                leave[q] = have - stay;
                rest[q] = end ? stay : 0u;
                n += leave[q] + rest[q];
                arr |= arrived ? 1u << q : 0u;
                s.prev[q] = end ? 0u : now;
            }
            if (!live) n = 0;
            if constexpr (!WRITE) {
                uint32_t sum = n;   // the wave's sum: every lane gets it
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
                if (lane == 0) cnt[(size_t)(t0 + j) * W + w] = sum;
#pragma unroll
                for (int q = 0; q < PK_S; q++) {   // the indices as the write pass leaves them, lengths only
                    const uint32_t h = s.idx[q] + leave[q] & 0xFFu, tl = (s.idx[q] >> 16) + (arr >> q & 1u) & 0xFFu;
                    s.idx[q] = end ? 0u : h | h << 8 | tl << 16;
                }
            } else {
                const uint32_t ln = (uint32_t)s.len;
                if (__ballot(live && arr != 0)) {   // an arrival: the previous row's AGV code joins the tail
                    if (live && arr != 0) {
                        const uint32_t q = (uint32_t)__ffs((int)arr) - 1u;
                        uint32_t ix = s.idx[0];
#pragma unroll
                        for (int k = 1; k < PK_S; k++) ix = q == (uint32_t)k ? s.idx[k] : ix;
                        const uint32_t tl = ix >> 16 & 0xFFu;
                        ring[((size_t)q * PK_RING + tl) * N] = s.hprev & FJSP_HELD_CODE_MASK;
                        ix = (ix & 0xFFFFu) | (tl + 1u & 0xFFu) << 16;
#pragma unroll
                        for (int k = 0; k < PK_S; k++) s.idx[k] = q == (uint32_t)k ? ix : s.idx[k];
                    }
                }
                bool go[PK_S];
                bool any_go = false;
#pragma unroll
                for (int q = 0; q < PK_S; q++) {   // started_packaging with an ungranted run in the FIFO
                    go[q] = live && (c.st[q][j] & 2u) != 0 && (s.idx[q] >> 8 & 0xFFu) != (s.idx[q] >> 16 & 0xFFu);
                    any_go = any_go || go[q];
                }
                if (__ballot(any_go)) {   // a START: every ungranted run gets the grant and this step
#pragma unroll
                    for (int q = 0; q < PK_S; q++) {
                        if (go[q]) {
                            const uint32_t tl = s.idx[q] >> 16 & 0xFFu;
                            for (uint32_t i = s.idx[q] >> 8 & 0xFFu; i != tl; i = i + 1u & 0xFFu) {
                                uint32_t* __restrict__ en = ring + ((size_t)q * PK_RING + i) * N;
                                *en = (*en & FJSP_HELD_CODE_MASK) | PK_GRANTED | ln << 16;
                            }
                            s.idx[q] = (s.idx[q] & 0xFF00FFu) | tl << 8;
                        }
                    }
                }
                if (__ballot(n != 0)) {   // some lane writes: ranks by an exclusive prefix sum of the counts
                    uint32_t inc = n;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t o = __shfl_up(inc, d);
                        if (lane >= d) inc += o;
                    }
                    long long rank = p.h.base + (long long)c.off[j] + (long long)(inc - n);
                    const long long es = p.h.step0 + (long long)(t0 + j) - (long long)s.len;
                    if (n != 0) {
#pragma unroll
                        for (int q = 0; q < PK_S; q++) {
                            const uint32_t m = leave[q] + rest[q];
                            uint32_t h = s.idx[q] & 0xFFu;
                            for (uint32_t i = 0; i < m; i++) {
                                const uint32_t en = ring[((size_t)q * PK_RING + h) * N];
                                const bool fin = i < leave[q], granted = (en & PK_GRANTED) != 0;
                                if ((unsigned long long)rank < (unsigned long long)p.h.cap) {
                                    const uint32_t info = (uint32_t)(4 + q) | (fin ? 1u << 8 : 0u) | (granted ? 1u << 9 : 0u) |
                                                          5u << 16 | 5u << 20;
                                    uint4* o = reinterpret_cast<uint4*>(p.recs + rank);
                                    o[0] = make_uint4(p.h.gid0 + (uint32_t)e, info, (uint32_t)es, (uint32_t)((unsigned long long)es >> 32));
                                    o[1] = make_uint4(en & FJSP_HELD_CODE_MASK, granted ? en >> 16 : ~0u, fin ? ln : ~0u, 0u);
                                }
                                rank += 1;
                                h = h + 1u & 0xFFu;
                            }
                            s.idx[q] = (s.idx[q] & 0xFFFF00u) | h;
                        }
                    }
                }
                if (end) {
#pragma unroll
                    for (int q = 0; q < PK_S; q++) s.idx[q] = 0u;
                }
                s.hprev = end ? 0u : c.held[j];
            }
            s.len = end ? 0 : s.len + 1;
        }
    }
}

template <bool WRITE>
__global__ void __launch_bounds__(64) k_packaging_scan(PackArgs p, uint32_t* __restrict__ cnt,
                                                       const long long* __restrict__ base, int W) {
    if (WRITE) p.h.base = base[0];
    const int lane = threadIdx.x, w = (int)blockIdx.x;
    const int e = w * 64 + lane;
    const bool live = e < p.h.N;
    const uint32_t col = (uint32_t)min(e, p.h.N - 1);
    const size_t N = (size_t)p.h.N;
    int32_t* __restrict__ cy = p.carry + col;   // word k of this env: cy[k * N]
    PackState s{};
    s.len = cy[(size_t)PK_LEN * N];
    s.hprev = (uint32_t)cy[(size_t)PK_HPREV * N];
#pragma unroll
    for (int q = 0; q < PK_S; q++) {
        s.prev[q] = (uint32_t)cy[(size_t)(PK_PREV + q) * N];
        s.idx[q] = (uint32_t)cy[(size_t)(PK_IDX + q) * N];
    }
    PackChunk<WRITE> A, B;
    int t0 = 0;
    pack_load<WRITE>(A, p, cnt, 0, W, w, col);
    for (;;) {   // the A / B walk, written out: a shared helper changes the kernel's code (file header)
        pack_load<WRITE>(B, p, cnt, t0 + EP_U, W, w, col);
        pack_rows<WRITE>(A, t0, p, cnt, W, w, e, lane, live, s);
        t0 += EP_U;
        if (t0 >= p.h.T) break;
        pack_load<WRITE>(A, p, cnt, t0 + EP_U, W, w, col);
        pack_rows<WRITE>(B, t0, p, cnt, W, w, e, lane, live, s);
        t0 += EP_U;
        if (t0 >= p.h.T) break;
    }
    if (WRITE && live) {   // the read list's mirror, written out: a STORE-templated visitor changes the kernel's code
        cy[(size_t)PK_LEN * N] = s.len;
        cy[(size_t)PK_HPREV * N] = (int32_t)s.hprev;
#pragma unroll
        for (int q = 0; q < PK_S; q++) {
            cy[(size_t)(PK_PREV + q) * N] = (int32_t)s.prev[q];
            cy[(size_t)(PK_IDX + q) * N] = (int32_t)s.idx[q];
        }
    }
}

// ---- the host front the four entries share ------------------------------------------------------
// temp: the counts / offsets table u32 [T][W] (padded to 16 bytes), 16 bytes for the count at entry
// and, for the scans that k_episode_count feeds, the flag words u32 [ceil(T / EP_U)][64 W].  The
// slab's T W 64 positions may not exceed `limit`, which keeps the table's sums in 32 bits.
struct ScanKind {
    int64_t limit;
    bool with_flags;
    const char* bound;
};
constexpr ScanKind EPISODES = {INT32_MAX, true, "T * N must be < 2^31"};   // one record per env and row at most
// up to three ops per env and row; at most one packaging arrival per env and row, and 255 runs per
// env carried in
constexpr ScanKind OPS = {(int64_t)1 << 30, false, "T * N must be < 2^30"};

bool temp_layout(int32_t T, int32_t N, int64_t limit, bool with_flags, uint64_t* table, uint64_t* total) {
    const int64_t W = ((int64_t)N + 63) / 64, L = (int64_t)T * W;
    if (L * 64 > limit) return false;
    *table = ((uint64_t)L * 4 + 15) & ~(uint64_t)15;
    *total = *table + 16 + (with_flags ? (uint64_t)((T + EP_U - 1) / EP_U) * (uint64_t)W * 64 * 4 : 0);
    return true;
}

int scan_fail(const char* entry, const char* what) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", entry, what);
    return fjsp_internal_fail(msg);   // copies the text
}

int scan_temp_bytes(const char* entry, const ScanKind& kind, int32_t T, int32_t N, uint64_t* bytes) {
    if (T <= 0 || N <= 0) return scan_fail(entry, "T and N must be > 0");
    if (!bytes) return scan_fail(entry, "null pointer");
    uint64_t table;
    if (!temp_layout(T, N, kind.limit, kind.with_flags, &table, bytes)) return scan_fail(entry, kind.bound);
    return 0;
}

struct ScanFront {
    int W, L;          // waves of 64 envs per row, T W
    uint32_t* offs;    // the counts / offsets table
    long long* base;   // the count at entry
    uint32_t* flags;   // k_episode_count's flag words (null for OPS)
    hipStream_t st;
};

// The checks every scan entry makes, in the order a bad call's first error is reported in, and the
// views into temp.  null_slab: one of the entry's own required pointers is null.
int scan_front(const char* entry, const ScanKind& kind, int32_t T, int32_t N, int64_t cap, bool null_slab,
               const void* recs, const void* count, void* temp, uint64_t temp_bytes, void* stream, ScanFront* f) {
    if (T <= 0 || N <= 0) return scan_fail(entry, "T and N must be > 0");
    if (cap < 0) return scan_fail(entry, "cap must be >= 0");
    if (null_slab || !count || !temp || (cap > 0 && !recs)) return scan_fail(entry, "null buffer");
    uint64_t table, total;
    if (!temp_layout(T, N, kind.limit, kind.with_flags, &table, &total)) return scan_fail(entry, kind.bound);
    if (temp_bytes < total) return scan_fail(entry, "temp buffer too small");
    if ((((uintptr_t)recs | (uintptr_t)temp) & 15u) != 0) return scan_fail(entry, "recs and temp must be 16-byte aligned");
    f->W = (int)(((int64_t)N + 63) / 64);   // T W 64 < 2^31 (checked above)
    f->L = T * f->W;
    f->offs = (uint32_t*)temp;
    f->base = (long long*)((char*)temp + table);
    f->flags = kind.with_flags ? (uint32_t*)((char*)temp + table + 16) : nullptr;
    f->st = (hipStream_t)stream;
    return 0;
}

ScanHead scan_head(int64_t cap, int64_t step0, uint32_t gid0, int32_t T, int32_t N) {
    return ScanHead{cap, 0, step0, gid0, T, N};   // base: the write kernel reads it from temp
}

void launch_offsets(const ScanFront& f, int64_t* count) {
    hipLaunchKernelGGL(k_episode_offsets, dim3(1), dim3(EPO_THREADS), 0, f.st, f.offs, f.L, f.base, (long long*)count);
}

// The count and offsets launches of the scans that write one record per episode end.
void launch_episode_count(const ScanFront& f, const uint8_t* term, const uint8_t* trunc, int32_t T, int32_t N,
                          int64_t* count) {
    const long long waves = (long long)f.W * ((T + EP_U - 1) / EP_U);
    hipLaunchKernelGGL(k_episode_count, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, f.st, term, trunc, T, N, f.W,
                       f.offs, f.flags);
    launch_offsets(f, count);
}

int scan_launched() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fjsp_internal_fail(hipGetErrorString(e));
        return -2;
    }
    return 0;
}

}  // namespace

extern "C" {

int fjsp_episode_temp_bytes(int32_t T, int32_t N, uint64_t* bytes) {
    return scan_temp_bytes("fjsp_episode_temp_bytes", EPISODES, T, N, bytes);
}

int fjsp_episode_scan(const double* rewards, const uint8_t* term, const uint8_t* trunc, const int32_t* orders_completed,
                      const int32_t* packaged, int32_t T, int32_t N, uint32_t env_gid0, int64_t step0, double* acc,
                      int32_t* len, fjsp_episode_rec* recs, int64_t cap, int64_t* count, void* temp, uint64_t temp_bytes,
                      void* stream) {
    ScanFront f;
    if (scan_front("fjsp_episode_scan", EPISODES, T, N, cap, !rewards || !term || !trunc || !acc || !len, recs, count,
                   temp, temp_bytes, stream, &f))
        return -1;
    launch_episode_count(f, term, trunc, T, N, count);
    const EpArgs p = {orders_completed, packaged, recs, scan_head(cap, step0, env_gid0, T, N)};
    hipLaunchKernelGGL(k_episode_scan, dim3((unsigned)f.W), dim3(64 * EP_A), 0, f.st, rewards, f.flags, f.offs, f.base, p,
                       f.W, acc, len);
    return scan_launched();
}

int fjsp_kpi_carry_words(void) { return KPI_WORDS; }

int fjsp_kpi_scan(const uint32_t* results, const uint8_t* term, const uint8_t* trunc, const int8_t* obs_i8,
                  const int32_t* orders_completed, const int32_t* packaged, const double* sim_time, int32_t T,
                  int32_t N, uint32_t env_gid0, int64_t step0, int32_t* carry, fjsp_kpi_rec* recs, int64_t cap,
                  int64_t* count, void* temp, uint64_t temp_bytes, void* stream) {
    ScanFront f;
    if (scan_front("fjsp_kpi_scan", EPISODES, T, N, cap, !term || !trunc || !carry, recs, count, temp, temp_bytes, stream,
                   &f))
        return -1;
    launch_episode_count(f, term, trunc, T, N, count);
    const KpiArgs p = {results, obs_i8, orders_completed, packaged, sim_time, recs, carry,
                       scan_head(cap, step0, env_gid0, T, N)};
    hipLaunchKernelGGL(k_kpi_scan, dim3((unsigned)f.W), dim3(64 * EP_A), 0, f.st, f.flags, f.offs, f.base, p, f.W);
    return scan_launched();
}

int fjsp_schedule_carry_words(void) { return SC_WORDS; }

int fjsp_schedule_temp_bytes(int32_t T, int32_t N, uint64_t* bytes) {
    return scan_temp_bytes("fjsp_schedule_temp_bytes", OPS, T, N, bytes);
}

int fjsp_schedule_scan(const uint32_t* results, const uint32_t* held, const uint8_t* term, const uint8_t* trunc, int32_t T,
                       int32_t N, uint32_t env_gid0, int64_t step0, int32_t* carry, fjsp_op_rec* recs, int64_t cap,
                       int64_t* count, void* temp, uint64_t temp_bytes, void* stream) {
    ScanFront f;
    if (scan_front("fjsp_schedule_scan", OPS, T, N, cap, !results || !held || !term || !trunc || !carry, recs, count, temp,
                   temp_bytes, stream, &f))
        return -1;
    if ((((uintptr_t)results | (uintptr_t)held | (uintptr_t)carry) & 3u) != 0 || ((uintptr_t)count & 7u) != 0)
        return fjsp_internal_fail("fjsp_schedule_scan: results, held and carry must be 4-byte, count 8-byte aligned");
    const SchedArgs p = {results, held, term, trunc, recs, carry, scan_head(cap, step0, env_gid0, T, N)};
    hipLaunchKernelGGL(k_schedule_scan<false>, dim3((unsigned)f.W), dim3(64), 0, f.st, p, f.offs, f.base, f.W);
    launch_offsets(f, count);
    hipLaunchKernelGGL(k_schedule_scan<true>, dim3((unsigned)f.W), dim3(64), 0, f.st, p, f.offs, f.base, f.W);
    return scan_launched();
}

int fjsp_packaging_carry_words(void) { return PK_WORDS; }

int fjsp_packaging_ring_bytes(int32_t N, uint64_t* bytes) {
    if (N <= 0) return fjsp_internal_fail("fjsp_packaging_ring_bytes: N must be > 0");
    if (!bytes) return fjsp_internal_fail("fjsp_packaging_ring_bytes: null pointer");
    *bytes = (uint64_t)PK_S * PK_RING * 4 * (uint64_t)N;
    return 0;
}

int fjsp_packaging_temp_bytes(int32_t T, int32_t N, uint64_t* bytes) {
    return scan_temp_bytes("fjsp_packaging_temp_bytes", OPS, T, N, bytes);
}

int fjsp_packaging_scan(const uint32_t* results, const uint32_t* held, const uint32_t* pack, const uint8_t* term,
                        const uint8_t* trunc, int32_t T, int32_t N, uint32_t env_gid0, int64_t step0, int32_t* carry,
                        uint32_t* ring, fjsp_op_rec* recs, int64_t cap, int64_t* count, void* temp, uint64_t temp_bytes,
                        void* stream) {
    ScanFront f;
    if (scan_front("fjsp_packaging_scan", OPS, T, N, cap, !results || !held || !pack || !term || !trunc || !carry || !ring,
                   recs, count, temp, temp_bytes, stream, &f))
        return -1;
    if ((((uintptr_t)results | (uintptr_t)held | (uintptr_t)pack | (uintptr_t)carry | (uintptr_t)ring) & 3u) != 0 ||
        ((uintptr_t)count & 7u) != 0)
        return fjsp_internal_fail("fjsp_packaging_scan: results, held, pack, carry and ring must be 4-byte, count 8-byte aligned");
    const PackArgs p = {results, held, pack, term, trunc, recs, carry, ring, scan_head(cap, step0, env_gid0, T, N)};
    hipLaunchKernelGGL(k_packaging_scan<false>, dim3((unsigned)f.W), dim3(64), 0, f.st, p, f.offs, f.base, f.W);
    launch_offsets(f, count);
    hipLaunchKernelGGL(k_packaging_scan<true>, dim3((unsigned)f.W), dim3(64), 0, f.st, p, f.offs, f.base, f.W);
    return scan_launched();
}

}  // extern "C"
