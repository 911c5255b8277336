// gsss_mixing.hip -- per-target mixing metrics of retained draws (gsss_target_mixing): one pass over a block of draws, folded per
// TARGET into step[M][2] = {sum theta, sum theta^2}, theta = acos(clamp(x_r . x_{r-1}, -1, 1)) the geodesic step between
// consecutive draws of a chain, and count[M][3 + K (+ K K)]: draws, pairs, hops across the equator of the target's direction h_t,
// the occupancy of its K mode directions and, on request, the K x K mode transitions.  Every target has its own directions.
//
// Layout.  A workgroup (256 threads) takes consecutive chains, one chain per lane, and a run of the block's rows
// (component-major input: for one (row, component) a wavefront reads 64 consecutive doubles).  Builds with a compile-time
// d = 2 .. 16 keep x_{r-1}, its sign and its mode in the lane's registers, h_t as well; the one build with a run-time d keeps the
// sign and the mode and reads row r - 1 a second time (the second read meets the first in the cache, as the SPLIT groups' reads
// of gsss_moments.hip do).  Chunks of chains are cut at target boundaries as gsss_moments.hip cuts them: with m <= 256 a
// workgroup takes whole targets -- as many as 256 lanes AND the LDS budget allow --, otherwise a target takes ceil(m / 256)
// workgroups.
//
// LDS (dynamic, kMixingLdsBudget at most), per target of the workgroup: its counters (64-bit), its directions [1 + K][d] at an
// odd stride in doubles (lanes of a wavefront that spans several targets read different banks; every lane has its own base) and
// eight doubles for step 3 below.  Where one target's share exceeds the budget (large d) the directions stay in global memory.
//
// Summation order of the two floating-point sums (fixed by the arguments alone, no floating-point atomics: a call's result is
// the same bits every time).
//   1. a lane adds its chain's pairs in row order;
//   2. the lanes of a wavefront are combined by a SEGMENTED shuffle reduction (offsets 1, 2, .. 32; a lane adds its neighbour
//      only if that neighbour belongs to the same target), which leaves a target's sum in the first of its lanes;
//   3. the wavefronts a target spans are added in wavefront order through LDS by one thread per target;
//   4. where a target has a single partial (m <= 256 and the rows are not split over workgroups) that thread adds it to step;
//      otherwise the partials go to a workspace and a second kernel adds them per target in (row split, chunk) order.
// The counters are integers: a lane adds to its target's counters in LDS with integer atomics, the workgroup adds what it
// counted to count[] with integer atomics on global memory -- the same result in any order.
// The rows are split over workgroups only when the chains alone give fewer than kWantGrid workgroups; a workgroup that starts
// inside the block takes x_{r-1} from the block's earlier row.  A pair (r, r - 1) counts where row r is.
//
// Chunk, Lane and segmented_sum are those of gsss_moments.hip and gsss_autocov.hip, kept local to this unit: each of the three
// units cuts its grid its own way (series, lag groups), and their kernels stay instruction-identical only if left alone.
#include "gsss_mixing.h"
#include "gsss_launch.h"

namespace gsss {
namespace {

constexpr int kWantGrid = 1024;  // workgroups below which the rows are split as well
constexpr int kMinSplitRows = 32;
constexpr size_t kMixingLdsBudget = 48 * 1024;  // directions, counters and fold scratch of a workgroup's targets
constexpr int kFoldDoubles = 8;                 // per target: 2 sums x 4 wavefronts

using Counter = unsigned long long;

struct MixingBlock {
    const double *x;
    int64_t sr, sj;  // doubles from row to row, component to component (the chains of a (row, component) are contiguous)
    int64_t ring_rows, first_row, n_rows, n_hist;
    int64_t n, m, n_targets, n_chunks;
    int32_t d, n_modes, transitions, nc, rsplit;
    int32_t tpw;     // targets a workgroup takes (m <= 256), else 0
    int32_t cpt;     // workgroups a target takes (m > 256), else 0
    int32_t stride;  // doubles from target to target of the staged directions (odd); 0: they are read from global memory
    int64_t dn;      // doubles of a target's directions: (1 + n_modes) d
    const double *dirs;
    double *step;
    Counter *count;
    double *ws;      // NULL: a target has one partial, added to step directly; else [rsplit][n_chunks][max(tpw, 1)][2]
};

struct Chunk {
    int64_t c0, t0;  // first chain, first target
    int32_t nc, nt;  // chains, targets
    int32_t m_loc;   // chains per target within the chunk
    int64_t r0, r1;  // rows, relative to the block's first
};

__device__ __forceinline__ Chunk chunk_of(const MixingBlock &a)
{
    Chunk k;
    const int64_t b = (int64_t)blockIdx.x % a.n_chunks, split = (int64_t)blockIdx.x / a.n_chunks;
    k.r0 = a.n_rows * split / a.rsplit;
    k.r1 = a.n_rows * (split + 1) / a.rsplit;
    if (a.tpw > 0) {
        k.t0 = b * a.tpw;
        const int64_t left = a.n_targets - k.t0;
        k.nt = (int32_t)(left < a.tpw ? left : a.tpw);
        k.c0 = k.t0 * a.m;
        k.m_loc = (int32_t)a.m;
        k.nc = k.nt * k.m_loc;
    } else {
        k.t0 = b / a.cpt;
        const int64_t first = (b % a.cpt) * kBlock, left = a.m - first;
        k.c0 = k.t0 * a.m + first;
        k.nc = (int32_t)(left < kBlock ? left : kBlock);
        k.nt = 1;
        k.m_loc = k.nc;
    }
    return k;
}

struct Lane {
    int32_t wave, lc, lt;  // wavefront of the workgroup, chain within the chunk, target within the chunk
    uint32_t same;         // bit s: the lane 2^s further on belongs to the same target
    bool valid, head;
};

__device__ __forceinline__ Lane lane_of(const Chunk &k)
{
    Lane l;
    const int lane = threadIdx.x % 64;
    l.wave = threadIdx.x / 64;
    l.lc = threadIdx.x;
    l.valid = l.lc < k.nc;
    l.lt = l.valid ? l.lc / k.m_loc : -1 - lane;  // (lanes without a chain: a segment each, never merged)
    l.same = 0;
    for (int s = 0; s < 6; ++s) {
        const int other = __shfl_down(l.lt, 1 << s);
        if (lane + (1 << s) < 64 && other == l.lt) l.same |= 1u << s;
    }
    const int prev = __shfl_up(l.lt, 1);
    l.head = l.valid && (lane == 0 || prev != l.lt);
    return l;
}

__device__ __forceinline__ double segmented_sum(double v, uint32_t same)
{
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const double other = __shfl_down(v, 1 << s);
        if (same & (1u << s)) v += other;
    }
    return v;
}

// Row q of the block (relative to its first; q = -1: the history row, round the ring's end) for the workgroup's first chain.
__device__ __forceinline__ const double *row_at(const MixingBlock &a, const double *p, int64_t q)
{
    int64_t r = a.first_row + q;
    if (r < 0) r += a.ring_rows;
    return p + r * a.sr;
}

__device__ __forceinline__ int sign_of(double v) { return (v > 0.0) - (v < 0.0); }  // np.sign

// What a lane keeps of the draw before: its sign against h and its mode.  What it has summed and counted.
struct Walk {
    double s1, s2;
    Counter hops;
    int sign, mode;
};

// A draw's mode from its K products, the first maximum like np.argmax.
__device__ __forceinline__ int first_max(const double (&v)[kMixingMaxModes], int K)
{
    int best = 0;
    double bv = -INFINITY;
#pragma unroll
    for (int i = 0; i < kMixingMaxModes; ++i) {
        if (i < K && v[i] > bv) {
            bv = v[i];
            best = i;
        }
    }
    return best;
}

// Row `cur` paired with the draw before it: the step, the hop, the counters.  cnt: the target's counters in LDS.
__device__ __forceinline__ void count_pair(const MixingBlock &a, Counter *cnt, Walk &w, double dot, int sign, int mode)
{
    const double theta = acos(fmin(fmax(dot, -1.0), 1.0));
    w.s1 += theta;
    w.s2 = fma(theta, theta, w.s2);
    w.hops += sign != w.sign;
    if (a.transitions) atomicAdd(cnt + 3 + a.n_modes + w.mode * a.n_modes + mode, (Counter)1);
}

// Compile-time d: x_{r-1} and h in registers, the modes from `dir` (LDS).
template <int D>
__device__ __forceinline__ void walk_fixed(const MixingBlock &a, const Chunk &k, const double *p, const double *dir, Counter *cnt,
                                           Walk &w)
{
    const int K = a.n_modes;
    double h[D], xp[D], x[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        h[j] = dir[j];
        xp[j] = 0.0;
    }
    const bool has_prev = k.r0 > 0 || a.n_hist > 0;
    for (int64_t r = has_prev ? k.r0 - 1 : k.r0; r < k.r1; ++r) {
        const double *q = row_at(a, p, r);
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = q[j * a.sj];
        double xh = 0.0, dot = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            xh = fma(x[j], h[j], xh);
            dot = fma(xp[j], x[j], dot);
        }
        int mode = 0;
        double bv = -INFINITY;
        for (int i = 0; i < K; ++i) {
            const double *mu = dir + (i + 1) * D;
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) v = fma(x[j], mu[j], v);
            if (v > bv) {  // first maximum, like np.argmax
                bv = v;
                mode = i;
            }
        }
        const int sign = sign_of(xh);
        if (r >= k.r0) {
            if (r > k.r0 || has_prev) count_pair(a, cnt, w, dot, sign, mode);
            if (K > 0) atomicAdd(cnt + 3 + mode, (Counter)1);
        }
        w.sign = sign;
        w.mode = mode;
#pragma unroll
        for (int j = 0; j < D; ++j) xp[j] = x[j];
    }
}

// Run-time d: one pass over the components of row r and, again, of row r - 1; the K products in registers.  DIR: LDS or global.
template <class DIR>
__device__ __forceinline__ void walk_any(const MixingBlock &a, const Chunk &k, const double *p, DIR dir, Counter *cnt, Walk &w)
{
    const int K = a.n_modes, d = a.d;
    const bool has_prev = k.r0 > 0 || a.n_hist > 0;
    for (int64_t r = has_prev ? k.r0 - 1 : k.r0; r < k.r1; ++r) {
        const double *q = row_at(a, p, r);
        const bool pair = r >= k.r0 && (r > k.r0 || has_prev);
        const double *qp = pair ? row_at(a, p, r - 1) : q;
        double v[kMixingMaxModes];
#pragma unroll
        for (int i = 0; i < kMixingMaxModes; ++i) v[i] = 0.0;
        double xh = 0.0, dot = 0.0;
        for (int j = 0; j < d; ++j) {
            const double xj = q[j * a.sj], pj = qp[j * a.sj];
            xh = fma(xj, dir[j], xh);
            dot = fma(pj, xj, dot);
#pragma unroll
            for (int i = 0; i < kMixingMaxModes; ++i)
                if (i < K) v[i] = fma(xj, dir[(i + 1) * d + j], v[i]);
        }
        const int mode = first_max(v, K), sign = sign_of(xh);
        if (r >= k.r0) {
            if (pair) count_pair(a, cnt, w, dot, sign, mode);
            if (K > 0) atomicAdd(cnt + 3 + mode, (Counter)1);
        }
        w.sign = sign;
        w.mode = mode;
    }
}

// D = 0: d at run time.
template <int D>
__global__ void __launch_bounds__(kBlock) mixing_kernel(const MixingBlock a)
{
    extern __shared__ double lds[];
    const Chunk k = chunk_of(a);
    const Lane l = lane_of(k);
    const int nt_max = a.tpw > 0 ? a.tpw : 1;
    Counter *cnt = reinterpret_cast<Counter *>(lds);  // [nt_max][nc]
    double *fold = lds + (size_t)nt_max * a.nc;       // [2][4][nt_max]
    double *dirs = fold + (size_t)nt_max * kFoldDoubles;  // [nt_max][stride]
    for (int i = threadIdx.x; i < k.nt * a.nc; i += kBlock) cnt[i] = 0;
    if (a.stride > 0) {
        const double *src = a.dirs + (size_t)k.t0 * a.dn;
        const int dn = (int)a.dn;  // (staged: a few thousand doubles at most)
        for (int i = threadIdx.x; i < k.nt * dn; i += kBlock) dirs[(i / dn) * a.stride + i % dn] = src[i];
    }
    __syncthreads();
    Walk w;
    w.s1 = w.s2 = 0.0;
    w.hops = 0;
    w.sign = w.mode = 0;
    if (l.valid) {
        const double *p = a.x + k.c0 + l.lc;
        Counter *mine = cnt + l.lt * a.nc;
        if constexpr (D > 0) {
            walk_fixed<D>(a, k, p, dirs + l.lt * a.stride, mine, w);
        } else {
            if (a.stride > 0)
                walk_any(a, k, p, dirs + l.lt * a.stride, mine, w);
            else
                walk_any(a, k, p, a.dirs + (size_t)(k.t0 + l.lt) * a.dn, mine, w);
        }
        const bool has_prev = k.r0 > 0 || a.n_hist > 0;
        atomicAdd(mine, (Counter)(k.r1 - k.r0));
        atomicAdd(mine + 1, (Counter)(k.r1 - k.r0 - (has_prev ? 0 : 1)));
        atomicAdd(mine + 2, w.hops);
    }
    // steps 2 - 4 of the summation order
    const double s1 = segmented_sum(w.s1, l.same), s2 = segmented_sum(w.s2, l.same);
    if (l.head) {
        fold[l.wave * nt_max + l.lt] = s1;
        fold[(4 + l.wave) * nt_max + l.lt] = s2;
    }
    __syncthreads();
    if (l.lc < k.nt) {  // one thread per target
        const int lt = l.lc;
        const int lo = (lt * k.m_loc) / 64, hi = ((lt + 1) * k.m_loc - 1) / 64;
        double t1 = fold[lo * nt_max + lt], t2 = fold[(4 + lo) * nt_max + lt];
        for (int wv = lo + 1; wv <= hi; ++wv) {
            t1 += fold[wv * nt_max + lt];
            t2 += fold[(4 + wv) * nt_max + lt];
        }
        if (a.ws) {
            double *o = a.ws + ((size_t)blockIdx.x * nt_max + lt) * 2;
            o[0] = t1;
            o[1] = t2;
        } else {
            double *o = a.step + (size_t)(k.t0 + lt) * 2;
            o[0] += t1;
            o[1] += t2;
        }
    }
    Counter *out = a.count + (size_t)k.t0 * a.nc;
    for (int i = threadIdx.x; i < k.nt * a.nc; i += kBlock)
        if (cnt[i] != 0) atomicAdd(out + i, cnt[i]);
}

// Step 4 with a workspace: one thread per (target, sum) adds the target's partials in (row split, chunk) order.
__global__ void __launch_bounds__(kBlock) mixing_fold_kernel(const MixingBlock a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_targets * 2) return;
    const int64_t t = i / 2;
    const int ai = (int)(i % 2);
    const int64_t stride = a.tpw > 0 ? a.tpw : 1;
    const int64_t b0 = a.tpw > 0 ? t / a.tpw : t * a.cpt, lt = a.tpw > 0 ? t % a.tpw : 0;
    const int64_t nb = a.tpw > 0 ? 1 : a.cpt;
    double s = 0.0;
    for (int64_t sp = 0; sp < a.rsplit; ++sp)
        for (int64_t b = b0; b < b0 + nb; ++b) s += a.ws[(size_t)(((sp * a.n_chunks + b) * stride + lt) * 2 + ai)];
    a.step[i] += s;
}

using MixingKernel = void (*)(const MixingBlock);

}  // namespace

int launch_target_mixing(const double *ring, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist, int64_t n_chains,
                         int d, int64_t m, const double *dirs, int n_modes, bool transitions, double *step, int64_t *count,
                         hipStream_t st)
{
    MixingKernel kern = mixing_kernel<0>;
    switch (d) {
#define GSSS_MIXING_CASE(D) \
    case D: kern = mixing_kernel<D>; break;
        GSSS_MIXING_CASE(2)
        GSSS_MIXING_CASE(3)
        GSSS_MIXING_CASE(4)
        GSSS_MIXING_CASE(5)
        GSSS_MIXING_CASE(6)
        GSSS_MIXING_CASE(7)
        GSSS_MIXING_CASE(8)
        GSSS_MIXING_CASE(9)
        GSSS_MIXING_CASE(10)
        GSSS_MIXING_CASE(11)
        GSSS_MIXING_CASE(12)
        GSSS_MIXING_CASE(13)
        GSSS_MIXING_CASE(14)
        GSSS_MIXING_CASE(15)
        GSSS_MIXING_CASE(16)
#undef GSSS_MIXING_CASE
    default: break;
    }
    MixingBlock a{};
    a.x = ring;
    a.sr = (int64_t)d * n_chains;
    a.sj = n_chains;
    a.ring_rows = ring_rows;
    a.first_row = first_row;
    a.n_rows = n_rows;
    a.n_hist = n_hist;
    a.n = n_chains;
    a.m = m;
    a.n_targets = n_chains / m;
    a.d = d;
    a.n_modes = n_modes;
    a.transitions = transitions && n_modes > 0 ? 1 : 0;
    a.nc = (int32_t)mixing_counters(n_modes, transitions);
    a.dn = (int64_t)(1 + n_modes) * d;
    a.dirs = dirs;
    a.step = step;
    a.count = reinterpret_cast<Counter *>(count);
    // The LDS of one target: counters, fold scratch and, where that still fits the budget, its directions at an odd stride.
    const size_t bare = (size_t)(a.nc + kFoldDoubles) * sizeof(double);
    size_t per_target = bare + (size_t)(a.dn | 1) * sizeof(double);
    a.stride = (int32_t)(a.dn | 1);
    if (per_target > kMixingLdsBudget) {
        a.stride = 0;
        per_target = bare;
    }
    if (m <= kBlock) {
        const int64_t by_lanes = kBlock / m, by_lds = (int64_t)(kMixingLdsBudget / per_target);
        a.tpw = (int32_t)(by_lanes < by_lds ? by_lanes : by_lds);
        a.n_chunks = ceil_div(a.n_targets, a.tpw);
    } else {
        a.cpt = (int32_t)ceil_div(m, kBlock);
        a.n_chunks = a.n_targets * a.cpt;
    }
    a.rsplit = 1;
    if (a.n_chunks < kWantGrid) {
        const int64_t most = n_rows / kMinSplitRows, want = ceil_div(kWantGrid, a.n_chunks);
        a.rsplit = (int32_t)(most < 1 ? 1 : (want < most ? want : most));
    }
    if (ceil_div(m, kBlock) > 0x7FFFFFFFll || a.n_chunks * a.rsplit > 0x7FFFFFFFll || a.n_targets * 2 > 0x7FFFFFFFll * kBlock) {
        set_error("gsss_target_mixing: %lld chains of %lld per target exceed the grid", (long long)n_chains, (long long)m);
        return GSSS_E_UNSUPPORTED;
    }
    const size_t lds = per_target * (a.tpw > 0 ? a.tpw : 1);
    // A workspace only where a target has more than one partial; taken and freed in stream order, like gsss_target_moments'.
    void *ws = nullptr;
    if (a.rsplit > 1 || a.tpw == 0) {
        const size_t n_ws = (size_t)a.rsplit * a.n_chunks * (a.tpw > 0 ? a.tpw : 1) * 2;
        GSSS_HIP_TRY(hipMallocAsync(&ws, n_ws * sizeof(double), st));
        a.ws = static_cast<double *>(ws);
    }
    int rc = launch_kernel("mixing", kern, a.n_chunks * a.rsplit, lds, st, nullptr, a);
    if (rc == GSSS_OK && ws) rc = launch_kernel("mixing fold", mixing_fold_kernel, ceil_div(a.n_targets * 2, kBlock), 0, st, nullptr, a);
    if (ws) (void)hipFreeAsync(ws, st);
    return rc;
}

}  // namespace gsss
