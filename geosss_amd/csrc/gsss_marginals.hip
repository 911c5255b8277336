// gsss_marginals.hip -- per-target marginal histograms of retained draws (gsss_target_marginals): one pass over a block of draws,
// counted per TARGET into count[M][S][B]: for each of the target's P directions v_p the histogram of u = x . v_p over [-1, 1] in B
// equal bins and, on request (series P, S = P + 1), the histogram of theta = acos(clamp(x_r . x_{r-1}, -1, 1)) over [0, pi], the
// geodesic step between consecutive draws of a chain.  Every target has its own directions.
//
// Layout.  A workgroup (256 threads) takes consecutive chains, one chain per lane, and a run of the block's rows
// (component-major input: for one (row, component) a wavefront reads 64 consecutive doubles).  Builds with a compile-time
// d = 2 .. 16 keep x_{r-1} in the lane's registers for the step series; the one build with a run-time d reads row r - 1 a second
// time (the second read meets the first in the cache, as gsss_mixing.hip's does) and keeps the P products of a draw in registers.
// The cut of the chains at target boundaries and the split of the rows over workgroups are gsss_target_fold.h's, with CW = 256,
// one series and the targets of a workgroup capped by the LDS budget as well.
//
// LDS (dynamic, kMarginalsLdsBudget at most), per target of the workgroup: its directions [P][d] at an odd stride in doubles
// (lanes of a wavefront that spans several targets read different banks; every lane has its own base) and its S B counters
// (32-bit: a workgroup adds at most 256 lanes x 2^23 rows to one of them).  Where one target's share exceeds the budget (large d)
// the directions stay in global memory.  40 KiB: four workgroups (sixteen wavefronts) fit a CU's 160 KiB whatever the shape --
// one more than gsss_mixing.hip's 48 KiB leaves the kernel this one is measured against, and what the registers allow the
// builds with d >= 11 anyway.  A workgroup takes what its targets need, not the budget (64 bins along the d = 5 axes: 1.5 KB per
// target), so the budget binds only where many small targets share a workgroup or one target's counters are large (DESIGN.md
// 5.6k).
//
// No floating-point sums: nothing to fold, no workspace, no second kernel.  The counters are integers: per (draw, series) 1 is
// added to the target's counter in LDS with an integer atomic -- lanes of a wavefront that hit the same counter first combined
// into one add of their number (add_one) --, the workgroup then adds its non-zero counters to count[] with 64-bit integer
// atomics on global memory -- the same result in any order.
// A workgroup that starts inside the block takes x_{r-1} from the block's earlier row.  A pair (r, r - 1) counts where row r is.
#include "gsss_marginals.h"
#include "gsss_target_fold.h"

namespace gsss {
namespace {

constexpr int kMinSplitRows = 32;
constexpr size_t kMarginalsLdsBudget = 40 * 1024;  // directions and counters of a workgroup's targets
constexpr double kPi = 3.14159265358979323846;     // M_PI, the double nearest pi

using Counter = unsigned long long;

struct MarginalsBlock {
    const double *x;
    int64_t sr, sj;  // doubles from row to row, component to component (the chains of a (row, component) are contiguous)
    TargetCut cut;   // CW = 256; tpw: also what the LDS budget allows
    int64_t ring_rows, first_row, n_hist;
    int32_t d, n_dirs, n_bins, steps;
    int32_t nc;      // counters per target: (n_dirs + steps) n_bins
    int32_t stride;  // doubles from target to target of the staged directions (odd); 0: they are read from global memory
    int64_t dn;      // doubles of a target's directions: n_dirs d
    double half, scale;  // 0.5 n_bins; n_bins / pi
    const double *dirs;
    Counter *count;
};

// Row q of the block (relative to its first; q = -1: the history row, round the ring's end) for the workgroup's first chain.
__device__ __forceinline__ const double *row_at(const MarginalsBlock &a, const double *p, int64_t q)
{
    int64_t r = a.first_row + q;
    if (r < 0) r += a.ring_rows;
    return p + r * a.sr;
}

// t >= 0 or t < 0, never NaN: the bin of t, the last one from n_bins on (so that no value beyond int's range is converted).
__device__ __forceinline__ int bin_of(double t, int n_bins) { return t < 0.0 ? 0 : (t >= (double)n_bins ? n_bins - 1 : (int)t); }

// Adds 1 to cnt[key] for every lane of the wavefront whose key is not negative (cnt: the workgroup's counters; every lane that
// walks calls it, in step).  On a peaked posterior the lanes of a wavefront hit one to three counters and LDS atomics to one
// address serialise, so the wavefront first combines: while the counter of its first lane left gathers kCombineMin lanes or
// more, that lane adds their number at once, kCombineRounds times at most; whoever is left adds 1 itself.  On a flat posterior
// the first look finds a lane or two and the cost is that look.  Integer adds: the same counts either way.
constexpr int kCombineMin = 8, kCombineRounds = 4;

__device__ __forceinline__ void add_one(unsigned *cnt, int key)
{
    const int lane = threadIdx.x % 64;
    unsigned long long left = __ballot(key >= 0);
    for (int round = 0; round < kCombineRounds && left != 0; ++round) {
        const int leader = __ffsll(left) - 1;
        const int k = __builtin_amdgcn_readlane(key, leader);  // (leader is the wavefront's: a scalar, no trip through LDS)
        const unsigned long long same = __ballot(key == k);
        const int n = __popcll(same);
        if (n < kCombineMin) break;
        if (lane == leader) atomicAdd(cnt + k, (unsigned)n);
        if (key == k) key = -1;
        left &= ~same;
    }
    if (key >= 0) atomicAdd(cnt + key, 1u);
}

// u = x . v_p: the lane's counter of series p, `base` the first counter of its target; -1 for NaN.
__device__ __forceinline__ int key_u(const MarginalsBlock &a, int base, int p, double u)
{
    return u != u ? -1 : base + p * a.n_bins + bin_of((u + 1.0) * a.half, a.n_bins);
}

// dot = x_r . x_{r-1}: the lane's counter of the step series; -1 for NaN.
__device__ __forceinline__ int key_step(const MarginalsBlock &a, int base, double dot)
{
    if (dot != dot) return -1;
    const double theta = acos(fmin(fmax(dot, -1.0), 1.0));
    return base + a.n_dirs * a.n_bins + bin_of(theta * a.scale, a.n_bins);
}

// Compile-time d: x_{r-1} in registers, the directions from `dir` (LDS).
template <int D>
__device__ __forceinline__ void walk_fixed(const MarginalsBlock &a, const Chunk &k, const double *p, const double *dir, unsigned *cnt,
                                           int base)
{
    const int P = a.n_dirs;
    double xp[D], x[D];
#pragma unroll
    for (int j = 0; j < D; ++j) xp[j] = 0.0;
    const bool has_prev = a.steps && (k.r0 > 0 || a.n_hist > 0);
    for (int64_t r = has_prev ? k.r0 - 1 : k.r0; r < k.r1; ++r) {
        const double *q = row_at(a, p, r);
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = q[j * a.sj];
        if (r >= k.r0) {
            for (int i = 0; i < P; ++i) {
                const double *v = dir + i * D;
                double u = 0.0;
#pragma unroll
                for (int j = 0; j < D; ++j) u = fma(x[j], v[j], u);
                add_one(cnt, key_u(a, base, i, u));
            }
            if (a.steps && (r > k.r0 || has_prev)) {
                double dot = 0.0;
#pragma unroll
                for (int j = 0; j < D; ++j) dot = fma(xp[j], x[j], dot);
                add_one(cnt, key_step(a, base, dot));
            }
        }
#pragma unroll
        for (int j = 0; j < D; ++j) xp[j] = x[j];
    }
}

// Run-time d: one pass over the components of row r and, for a pair, of row r - 1; the P products in registers.  DIR: LDS or global.
template <class DIR>
__device__ __forceinline__ void walk_any(const MarginalsBlock &a, const Chunk &k, const double *p, DIR dir, unsigned *cnt, int base)
{
    const int P = a.n_dirs, d = a.d;
    const bool has_prev = a.steps && (k.r0 > 0 || a.n_hist > 0);
    for (int64_t r = k.r0; r < k.r1; ++r) {
        const double *q = row_at(a, p, r);
        const bool pair = a.steps && (r > k.r0 || has_prev);
        const double *qp = pair ? row_at(a, p, r - 1) : q;
        double v[kMarginalsMaxDirs];
#pragma unroll
        for (int i = 0; i < kMarginalsMaxDirs; ++i) v[i] = 0.0;
        double dot = 0.0;
        for (int j = 0; j < d; ++j) {
            const double xj = q[j * a.sj], pj = qp[j * a.sj];
            dot = fma(pj, xj, dot);
#pragma unroll
            for (int i = 0; i < kMarginalsMaxDirs; ++i)
                if (i < P) v[i] = fma(xj, dir[i * d + j], v[i]);
        }
#pragma unroll
        for (int i = 0; i < kMarginalsMaxDirs; ++i)
            if (i < P) add_one(cnt, key_u(a, base, i, v[i]));
        if (pair) add_one(cnt, key_step(a, base, dot));
    }
}

// D = 0: d at run time.
template <int D>
__global__ void __launch_bounds__(kBlock) marginals_kernel(const MarginalsBlock a)
{
    extern __shared__ double lds[];
    const Chunk k = chunk_of<kBlock, false>(a.cut);
    const Lane l = lane_of<kBlock>(k);
    const int nt_max = chunk_targets(a.cut);
    double *dirs = lds;                                                             // [nt_max][stride]
    unsigned *cnt = reinterpret_cast<unsigned *>(lds + (size_t)nt_max * a.stride);  // [nt_max][nc]
    for (int i = threadIdx.x; i < k.nt * a.nc; i += kBlock) cnt[i] = 0;
    if (a.stride > 0) {
        const double *src = a.dirs + (size_t)k.t0 * a.dn;
        const int dn = (int)a.dn;  // (staged: a few thousand doubles at most)
        for (int i = threadIdx.x; i < k.nt * dn; i += kBlock) dirs[(i / dn) * a.stride + i % dn] = src[i];
    }
    __syncthreads();
    if (l.valid) {
        const double *p = a.x + k.c0 + l.lc;
        const int base = l.lt * a.nc;  // the lane's target's first counter
        if constexpr (D > 0) {
            walk_fixed<D>(a, k, p, dirs + l.lt * a.stride, cnt, base);
        } else {
            if (a.stride > 0 || a.n_dirs == 0)
                walk_any(a, k, p, dirs + l.lt * a.stride, cnt, base);
            else
                walk_any(a, k, p, a.dirs + (size_t)(k.t0 + l.lt) * a.dn, cnt, base);
        }
    }
    __syncthreads();
    Counter *out = a.count + (size_t)k.t0 * a.nc;
    for (int i = threadIdx.x; i < k.nt * a.nc; i += kBlock)
        if (cnt[i] != 0) atomicAdd(out + i, (Counter)cnt[i]);
}

using MarginalsKernel = void (*)(const MarginalsBlock);

}  // namespace

int launch_target_marginals(const double *ring, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist,
                            int64_t n_chains, int d, int64_t m, const double *dirs, int n_dirs, int n_bins, bool steps,
                            int64_t *count, hipStream_t st)
{
    MarginalsKernel kern = marginals_kernel<0>;
    switch (d) {
#define GSSS_MARGINALS_CASE(D) \
    case D: kern = marginals_kernel<D>; break;
        GSSS_MARGINALS_CASE(2)
        GSSS_MARGINALS_CASE(3)
        GSSS_MARGINALS_CASE(4)
        GSSS_MARGINALS_CASE(5)
        GSSS_MARGINALS_CASE(6)
        GSSS_MARGINALS_CASE(7)
        GSSS_MARGINALS_CASE(8)
        GSSS_MARGINALS_CASE(9)
        GSSS_MARGINALS_CASE(10)
        GSSS_MARGINALS_CASE(11)
        GSSS_MARGINALS_CASE(12)
        GSSS_MARGINALS_CASE(13)
        GSSS_MARGINALS_CASE(14)
        GSSS_MARGINALS_CASE(15)
        GSSS_MARGINALS_CASE(16)
#undef GSSS_MARGINALS_CASE
    default: break;
    }
    MarginalsBlock a{};
    a.x = ring;
    a.sr = (int64_t)d * n_chains;
    a.sj = n_chains;
    a.ring_rows = ring_rows;
    a.first_row = first_row;
    a.n_hist = steps ? n_hist : 0;
    a.d = d;
    a.n_dirs = n_dirs;
    a.n_bins = n_bins;
    a.steps = steps ? 1 : 0;
    a.nc = (int32_t)(marginal_series(n_dirs, steps) * n_bins);
    a.dn = (int64_t)n_dirs * d;
    a.half = 0.5 * n_bins;
    a.scale = (double)n_bins / kPi;
    a.dirs = dirs;
    a.count = reinterpret_cast<Counter *>(count);
    // The LDS of one target: its counters and, where that still fits the budget, its directions at an odd stride.
    const size_t bare = (size_t)a.nc * sizeof(unsigned);
    const size_t staged = n_dirs > 0 ? (size_t)(a.dn | 1) : 0;
    size_t per_target = bare + staged * sizeof(double);
    if (per_target > kMarginalsLdsBudget) per_target = bare;
    a.stride = per_target > bare ? (int32_t)staged : 0;
    if (int rc = make_cut("gsss_target_marginals", n_chains, m, kBlock, (int64_t)(kMarginalsLdsBudget / per_target), n_rows,
                          kMinSplitRows, 1, 1, a.cut))
        return rc;
    const size_t lds = per_target * chunk_targets(a.cut);
    return launch_kernel("marginals", kern, a.cut.n_chunks * a.cut.rsplit, lds, st, nullptr, a);
}

}  // namespace gsss
