// gsss_autocov.hip -- per-target lagged products of retained draws (gsss_target_autocov): one pass over a block of draws, folded
// into acc[M][d][L + 1][3] per TARGET and series: C_l = sum x_r x_{r-l}, P_l = sum x_r, Q_l = sum x_{r-l} over the target's chains
// and the rows r of the block whose partner r - l lies in the block or in the n_hist rows before it.
//
// Layout.  A workgroup (256 threads) takes CW consecutive chains, one chain per lane, ONE of the d series and a run of the block's
// rows (component-major input: for one (row, series) a wavefront reads 64 consecutive doubles).  The lags 1 .. L are split over
// SPLIT groups of wavefronts that walk the same chains, LC lags each: LC = 8, SPLIT = 1 (CW = 256) up to L = 8; LC = 16 and
// SPLIT = 1, 2, 4 (CW = 256, 128, 64) up to L = 16, 32, 64.  Group g keeps the sums of the lags 16 g + 1 .. 16 g + 16 and, as its
// delay line, the last LC values of the series DELAYED by 16 g rows (x_{r - 16 g}, a second read of a row the workgroup read 16 g
// rows earlier: it meets the first in the cache, every double leaves HBM once).  The delay line is a register ring whose slot
// index is a constant: the row loop is unrolled LC times and slot u is written in the u-th of them.  A group holds 2 LC sums
// (C and Q), the LC ring values and the LC (2 LC for g > 0) values of the rows in flight -- two operations per (value, lag);
// nothing goes to scratch.  Group 0 also keeps lag 0.
// The cut of the chains at target boundaries and the split of the rows over workgroups are gsss_target_fold.h's, with CW as
// above and the d series as its series.
//
// The block's ends.  A row before the history reads as 0, which leaves C_l and Q_l exact.  P_l takes x_r only where r - l is a
// row that exists: from the first run of LC rows in which that holds for every lag of the group, the lags share ONE sum; the
// runs before it (the first L - n_hist rows of a series at most) are walked a second time, backwards, for P_l lag by lag,
// which waits in LDS until the fold adds the shared sum to it.
//
// Summation order: gsss_target_fold.h's steps 1 - 4.  What this unit adds to them: in step 1 the lag-by-lag part of P_l is added
// in REVERSE row order, then the shared sum is added to it; in step 4 a thread adds a single partial to acc for all its lags at
// the end, so that their loads of acc are in flight together.  A workgroup that starts inside the block takes its delay line
// from the block's earlier rows.
#include "gsss_autocov.h"
#include "gsss_target_fold.h"

namespace gsss {
namespace {

constexpr int kMinSplitRows = 32;

struct AutocovBlock {
    const double *x;
    int64_t sr, sj;  // doubles from row to row, series to series (the chains of a (row, series) are contiguous)
    int64_t ring_rows, first_row, n_hist;
    TargetCut cut;   // series: d
    int32_t n_lags, na;
    double *acc;
    double *ws;      // NULL: a target has one partial, added to acc directly; else the workspace of partials_of
};

// (C, P, Q) of one lag per lane -> per target: steps 2 and 3 of the summation order.  The thread l.lc < k.nt of a group of
// wavefronts is left with the sums of target l.lc of the chunk in c, p, q.  lds: 3 x 1024 doubles.
template <int CW>
__device__ __forceinline__ void fold3(const Chunk &k, const Lane &l, double &c, double &p, double &q, double *lds)
{
    double s[3] = {c, p, q};
    fold<CW, 3>(k, l, s, lds, CW, 1024);
    c = s[0];
    p = s[1];
    q = s[2];
    __syncthreads();
}

// Step 4 for the target sums a thread holds after fold3: (C, P, Q) of `lag` (> n_lags: none), all of a thread's lags in one go.
// A single partial is added to acc -- the loads of all the lags are in flight together, one round trip to memory -- otherwise
// it goes to the workspace.
template <int N>
__device__ __forceinline__ void put_lags(const AutocovBlock &a, const Chunk &k, int lt, int lag0, double (&c)[N], double (&p)[N],
                                         double (&q)[N])
{
    double *row = a.ws ? partials_of(a.cut, a.ws, lt, a.na) : a.acc + ((size_t)(k.t0 + lt) * a.cut.series + k.j) * a.na;
    if (!a.ws) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (lag0 + i > a.n_lags) break;
            c[i] += row[3 * (lag0 + i)];
            p[i] += row[3 * (lag0 + i) + 1];
            q[i] += row[3 * (lag0 + i) + 2];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (lag0 + i > a.n_lags) break;
        row[3 * (lag0 + i)] = c[i];
        row[3 * (lag0 + i) + 1] = p[i];
        row[3 * (lag0 + i) + 2] = q[i];
    }
}

// The lane's value of row q (relative to the block's first; -n_hist <= q: the history wraps round the ring), 0 before the history.
// p: the first chain of the chunk in row 0 of the ring (uniform in the workgroup), lc: the lane's chain of the chunk.
__device__ __forceinline__ double value_at(const AutocovBlock &a, const double *p, uint32_t lc, int64_t q)
{
    if (q < -a.n_hist) return 0.0;
    int64_t r = a.first_row + q;
    if (r < 0) r += a.ring_rows;
    return (p + r * a.sr)[lc];
}

// The sums of one group of wavefronts for one chain: lag 0 in (ss0, s0); C and Q of the lags g0 + 1 .. g0 + LC in c, q; ps: the
// part of P that those lags share, the sum of the rows from which every pair of the group exists.
template <int LC>
struct LagSums {
    double c[LC], q[LC], ring[LC], s0, ss0, ps;
};

// The rows base .. min(base + LC, r1) - 1.  On entry ring[(u - i) mod LC] is the series' value i rows before row base + u - g0.
// whole: every pair (row, row - lag) of the run and the group exists.
template <int LC>
__device__ __forceinline__ void walk_run(const AutocovBlock &a, const double *p, uint32_t lc, int64_t base, int64_t r1, int g0,
                                         bool whole, LagSums<LC> &v)
{
    double x[LC], y[LC];
#pragma unroll
    for (int u = 0; u < LC; ++u) x[u] = base + u < r1 ? value_at(a, p, lc, base + u) : 0.0;
    if (g0 > 0) {
#pragma unroll
        for (int u = 0; u < LC; ++u) y[u] = base + u < r1 ? value_at(a, p, lc, base + u - g0) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < LC; ++u) {
        if (base + u >= r1) break;
        v.s0 += x[u];
        v.ss0 = fma(x[u], x[u], v.ss0);
        v.ps += whole ? x[u] : 0.0;
#pragma unroll
        for (int i = 1; i <= LC; ++i) {
            const double z = v.ring[(u - i + LC) % LC];
            v.c[i - 1] = fma(x[u], z, v.c[i - 1]);
            v.q[i - 1] += z;
        }
        v.ring[u] = g0 > 0 ? y[u] : x[u];
    }
}

// P of the rows r0 .. r1 - 1 (the runs that are not whole) for the lags g0 + 1 .. g0 + LC, into park[i * kBlock]: lag l takes x_q
// where q - l >= -n_hist, a sum over the last rows of the range, so the rows are walked backwards and the running sum is lag
// (q + n_hist)'s when row q has been added.  These are the first L - n_hist rows of a series at most, read a second time.
template <int LC>
__device__ __forceinline__ void park_partial_p(const AutocovBlock &a, const double *p, uint32_t lc, int64_t r0, int64_t r1, int g0,
                                               double *park)
{
    double s = 0.0;
    for (int64_t q = r1 - 1; q >= r0; --q) {
        s += value_at(a, p, lc, q);
        const int64_t i = q + a.n_hist - g0 - 1;
        if (i >= 0 && i < LC) park[i * kBlock] = s;
    }
    for (int i = 0; i < LC; ++i)
        if (g0 + i + 1 - a.n_hist < r0) park[i * kBlock] = s;
}

template <int LC, int SPLIT>
__global__ void __launch_bounds__(kBlock) autocov_kernel(const AutocovBlock a)
{
    constexpr int CW = kBlock / SPLIT;
    constexpr int kLds = LC * kBlock > 3072 ? LC * kBlock : 3072;  // a lane's LC partial P, then fold3's 3 x 1024
    __shared__ double lds[kLds];
    const Chunk k = chunk_of<CW, true>(a.cut);
    const Lane l = lane_of<CW>(k);
    const int g0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CW) * LC);  // uniform in a wavefront
    double *park = lds + threadIdx.x;
    LagSums<LC> v;
    v.s0 = v.ss0 = v.ps = 0.0;
#pragma unroll
    for (int i = 0; i < LC; ++i) {
        v.c[i] = v.q[i] = v.ring[i] = 0.0;
        park[i * kBlock] = 0.0;
    }
    if (l.valid) {
        const double *p = a.x + k.j * a.sj + k.c0;
        // the first run from which every pair of the group exists: the runs before it give P lag by lag
        int64_t whole_from = k.r0;
        if (whole_from - (g0 + LC) < -a.n_hist) whole_from += ceil_div(g0 + LC - a.n_hist - whole_from, LC) * LC;
        park_partial_p<LC>(a, p, l.lc, k.r0, whole_from < k.r1 ? whole_from : k.r1, g0, park);
#pragma unroll
        for (int i = 1; i <= LC; ++i) v.ring[LC - i] = value_at(a, p, l.lc, k.r0 - g0 - i);
        for (int64_t base = k.r0; base < k.r1; base += LC) walk_run<LC>(a, p, l.lc, base, k.r1, g0, base >= whole_from, v);
    }
    double p[LC], c0[1] = {v.ss0}, p0[1] = {v.s0}, q0[1] = {v.s0};
#pragma unroll
    for (int i = 0; i < LC; ++i) p[i] = park[i * kBlock] + v.ps;
    __syncthreads();
    fold3<CW>(k, l, c0[0], p0[0], q0[0], lds);
#pragma unroll
    for (int i = 0; i < LC; ++i) fold3<CW>(k, l, v.c[i], p[i], v.q[i], lds);
    if (l.lc < k.nt) {
        if (g0 == 0) put_lags(a, k, l.lc, 0, c0, p0, q0);
        put_lags(a, k, l.lc, g0 + 1, v.c, p, v.q);
    }
}

// Step 4 with a workspace.
__global__ void __launch_bounds__(kBlock) autocov_fold_kernel(const TargetFold f) { fold_partials<false>(f); }

}  // namespace

int launch_target_autocov(const double *ring, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist, int64_t n_chains,
                          int d, int64_t m, int n_lags, double *acc, hipStream_t st)
{
    auto kern = autocov_kernel<8, 1>;
    int cw = kBlock;
    if (n_lags > 32) {
        kern = autocov_kernel<16, 4>;
        cw = kBlock / 4;
    } else if (n_lags > 16) {
        kern = autocov_kernel<16, 2>;
        cw = kBlock / 2;
    } else if (n_lags > 8) {
        kern = autocov_kernel<16, 1>;
    }
    AutocovBlock a{};
    a.x = ring;
    a.sr = (int64_t)d * n_chains;
    a.sj = n_chains;
    a.ring_rows = ring_rows;
    a.first_row = first_row;
    a.n_hist = n_hist;
    a.n_lags = n_lags;
    a.na = (int32_t)autocov_sums(n_lags);
    a.acc = acc;
    if (int rc = make_cut("gsss_target_autocov", n_chains, m, cw, cw, n_rows, kMinSplitRows, d, a.na, a.cut)) return rc;
    const TargetFold f{a.cut, nullptr, acc, a.na, 0, a.na};
    return launch_walk_and_fold("autocov fold", autocov_fold_kernel, f, 0, st, [&](double *ws, double *) {
        a.ws = ws;
        return launch_kernel("autocov", kern, a.cut.n_chunks * d * a.cut.rsplit, 0, st, nullptr, a);
    });
}

}  // namespace gsss
