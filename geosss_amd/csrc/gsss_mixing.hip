// gsss_mixing.hip -- per-target mixing metrics of retained draws (gsss_target_mixing): one pass over a block of draws, folded per
// TARGET into step[M][2] = {sum theta, sum theta^2}, theta = acos(clamp(x_r . x_{r-1}, -1, 1)) the geodesic step between
// consecutive draws of a chain, and count[M][3 + K (+ K K)]: draws, pairs, hops across the equator of the target's direction h_t,
// the occupancy of its K mode directions and, on request, the K x K mode transitions.  Every target has its own directions.
//
// Layout.  A workgroup (256 threads) takes consecutive chains, one chain per lane, and a run of the block's rows
// (component-major input: for one (row, component) a wavefront reads 64 consecutive doubles).  Builds with a compile-time
// d = 2 .. 16 keep x_{r-1}, its sign and its mode in the lane's registers, h_t as well; the one build with a run-time d keeps the
// sign and the mode and reads row r - 1 a second time (the second read meets the first in the cache, as the SPLIT groups' reads
// of gsss_moments.hip do).  The cut of the chains at target boundaries and the split of the rows over workgroups are
// gsss_target_fold.h's, with CW = 256, one series and the targets of a workgroup capped by the LDS budget as well.
//
// LDS (dynamic, kMixingLdsBudget at most), per target of the workgroup: its counters (64-bit), its directions [1 + K][d] at an
// odd stride in doubles (lanes of a wavefront that spans several targets read different banks; every lane has its own base) and
// eight doubles for step 3 below.  Where one target's share exceeds the budget (large d) the directions stay in global memory.
//
// Summation order of the two floating-point sums: gsss_target_fold.h's steps 1 - 4 (a lane adds its chain's PAIRS in row order).
// The counters are integers: a lane adds to its target's counters in LDS with integer atomics, the workgroup adds what it
// counted to count[] with integer atomics on global memory -- the same result in any order.
// A workgroup that starts inside the block takes x_{r-1} from the block's earlier row.  A pair (r, r - 1) counts where row r is.
#include "gsss_mixing.h"
#include "gsss_target_fold.h"

namespace gsss {
namespace {

constexpr int kMinSplitRows = 32;
constexpr size_t kMixingLdsBudget = 48 * 1024;  // directions, counters and fold scratch of a workgroup's targets
constexpr int kFoldDoubles = 8;                 // per target: 2 sums x 4 wavefronts

using Counter = unsigned long long;

struct MixingBlock {
    const double *x;
    int64_t sr, sj;  // doubles from row to row, component to component (the chains of a (row, component) are contiguous)
    TargetCut cut;   // CW = 256; tpw: also what the LDS budget allows
    int64_t ring_rows, first_row, n_hist;
    int32_t d, n_modes, transitions, nc;
    int32_t stride;  // doubles from target to target of the staged directions (odd); 0: they are read from global memory
    int64_t dn;      // doubles of a target's directions: (1 + n_modes) d
    const double *dirs;
    double *step;
    Counter *count;
    double *ws;      // NULL: a target has one partial, added to step directly; else the workspace of partials_of
};

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
    const Chunk k = chunk_of<kBlock, false>(a.cut);
    const Lane l = lane_of<kBlock>(k);
    const int nt_max = chunk_targets(a.cut);
    Counter *cnt = reinterpret_cast<Counter *>(lds);  // [nt_max][nc]
    double *sums = lds + (size_t)nt_max * a.nc;       // [2][4][nt_max]
    double *dirs = sums + (size_t)nt_max * kFoldDoubles;  // [nt_max][stride]
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
    double t[2] = {w.s1, w.s2};
    fold<kBlock, 2>(k, l, t, sums, nt_max, 4 * nt_max);
    if (l.lc < k.nt) {  // one thread per target
        if (a.ws) {
            double *o = partials_of(a.cut, a.ws, l.lc, 2);
            o[0] = t[0];
            o[1] = t[1];
        } else {
            double *o = a.step + (size_t)(k.t0 + l.lc) * 2;
            o[0] += t[0];
            o[1] += t[1];
        }
    }
    Counter *out = a.count + (size_t)k.t0 * a.nc;
    for (int i = threadIdx.x; i < k.nt * a.nc; i += kBlock)
        if (cnt[i] != 0) atomicAdd(out + i, cnt[i]);
}

// Step 4 with a workspace.
__global__ void __launch_bounds__(kBlock) mixing_fold_kernel(const TargetFold f) { fold_partials<false>(f); }

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
    a.n_hist = n_hist;
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
    if (int rc = make_cut("gsss_target_mixing", n_chains, m, kBlock, (int64_t)(kMixingLdsBudget / per_target), n_rows, kMinSplitRows,
                          1, 2, a.cut))
        return rc;
    const size_t lds = per_target * chunk_targets(a.cut);
    const TargetFold f{a.cut, nullptr, step, 2, 0, 2};
    return launch_walk_and_fold("mixing fold", mixing_fold_kernel, f, 0, st, [&](double *ws, double *) {
        a.ws = ws;
        return launch_kernel("mixing", kern, a.cut.n_chunks * a.cut.rsplit, lds, st, nullptr, a);
    });
}

}  // namespace gsss
