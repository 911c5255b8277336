// gsss_moments.hip -- per-target moments of retained draws (gsss_target_moments): one pass over a block of draws, folded into
// acc[M][1 + d + T] per TARGET (count, sum x_j, sum x_i x_j) and, optionally, the per-chain sums chain_sum[d][n].
//
// Layout.  A workgroup (256 threads) takes CW consecutive chains, one chain per lane, and a run of the block's rows; a lane
// keeps the sums of ITS chain in registers while it walks the rows (component-major input: for one (row, component) a wavefront
// reads 64 consecutive doubles).  The d + T sums of a chain are split evenly over SPLIT groups of wavefronts that walk the same
// chains -- SPLIT = 1 (CW = 256) up to d = 8, 2 (CW = 128) up to d = 12, 4 (CW = 64) up to d = 16 -- so that no lane holds more
// than 45 sums and nothing spills; the groups' reads of the same doubles meet in the cache, every double leaves HBM once.
// Chunks of chains are cut at target boundaries: with m <= CW a workgroup takes floor(CW / m) whole targets, otherwise a target
// takes ceil(m / CW) workgroups.
//
// Summation order (fixed by the arguments alone, no atomics: a call's result is the same bits every time).
//   1. a lane adds its chain's rows in row order;
//   2. the lanes of a wavefront are combined by a SEGMENTED shuffle reduction (offsets 1, 2, .. 32; a lane adds its neighbour
//      only if that neighbour belongs to the same target), which leaves a target's sum in the first of its lanes;
//   3. the wavefronts a target spans are added in wavefront order through LDS by one thread per target;
//   4. where a target has a single partial (m <= CW and the rows are not split over workgroups) that thread adds it to acc;
//      otherwise the partials go to a workspace and a second kernel adds them per target in (row split, chunk) order.
// The rows are split over workgroups only when the chains alone give fewer than kWantGrid workgroups.
#include "gsss_moments.h"
#include "gsss_launch.h"

namespace gsss {
namespace {

constexpr int kWantGrid = 1024;  // workgroups below which the rows are split as well
constexpr int kMinSplitRows = 8;

struct MomentsBlock {
    const double *x;
    int64_t sr, sj, sc;  // doubles from row to row, component to component, chain to chain
    int64_t n, n_rows, m, n_targets, n_chunks;
    int32_t d, na, acc_rows, rsplit;
    int32_t tpw;         // targets a workgroup takes (m <= CW), else 0
    int32_t cpt;         // workgroups a target takes (m > CW), else 0
    double *acc, *chain_sum;
    double *ws_t;        // NULL: a target has one partial, added to acc directly; else [rsplit][n_chunks][max(tpw, 1)][na]
    double *ws_c;        // NULL: chain sums are added to chain_sum directly; else [rsplit][d][n]
};

struct Chunk {
    int64_t c0, t0;    // first chain, first target
    int32_t nc, nt;    // chains, targets
    int32_t m_loc;     // chains per target within the chunk
    int64_t r0, r1;    // rows
    int64_t slot;      // (row split, chunk) index of the partials
    int32_t split;
};

template <int CW>
__device__ __forceinline__ Chunk chunk_of(const MomentsBlock &a)
{
    Chunk k;
    const int64_t b = (int64_t)blockIdx.x % a.n_chunks;
    k.split = (int32_t)((int64_t)blockIdx.x / a.n_chunks);
    k.slot = (int64_t)blockIdx.x;
    k.r0 = a.n_rows * k.split / a.rsplit;
    k.r1 = a.n_rows * (k.split + 1) / a.rsplit;
    if (a.tpw > 0) {
        k.t0 = b * a.tpw;
        const int64_t left = a.n_targets - k.t0;
        k.nt = (int32_t)(left < a.tpw ? left : a.tpw);
        k.c0 = k.t0 * a.m;
        k.m_loc = (int32_t)a.m;
        k.nc = k.nt * k.m_loc;
    } else {
        k.t0 = b / a.cpt;
        const int64_t first = (b % a.cpt) * CW, left = a.m - first;
        k.c0 = k.t0 * a.m + first;
        k.nc = (int32_t)(left < CW ? left : CW);
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

template <int CW>
__device__ __forceinline__ Lane lane_of(const Chunk &k)
{
    constexpr int WPP = CW / 64;
    Lane l;
    const int lane = threadIdx.x % 64;
    l.wave = threadIdx.x / 64;
    l.lc = (l.wave % WPP) * 64 + lane;
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

__device__ __forceinline__ void put_target(const MomentsBlock &a, const Chunk &k, int lt, int ai, double s)
{
    if (ai >= a.na) return;
    if (a.ws_t) {
        a.ws_t[((size_t)k.slot * (a.tpw > 0 ? a.tpw : 1) + lt) * a.na + ai] = s;
        return;
    }
    double *row = a.acc + (size_t)(k.t0 + lt) * a.acc_rows;
    row[1 + ai] += s;
    if (ai == 0) row[0] += (double)(a.m * a.n_rows);
}

__device__ __forceinline__ void put_chain(const MomentsBlock &a, const Chunk &k, const Lane &l, int j, double s)
{
    if (!a.chain_sum || !l.valid) return;
    const int64_t c = k.c0 + l.lc;
    if (a.ws_c)
        a.ws_c[((size_t)k.split * a.d + j) * a.n + c] = s;
    else
        a.chain_sum[(size_t)j * a.n + c] += s;
}

// Two sums per lane -> per target: steps 2 - 4 of the summation order.  a0, a1: which of the na sums they are (>= na: none);
// the same for every lane of a group of wavefronts.  lds: 2 x 1024 doubles.  Every thread of the workgroup calls it.
template <int CW>
__device__ __forceinline__ void fold2(const MomentsBlock &a, const Chunk &k, const Lane &l, double v0, double v1, int a0, int a1,
                                      double *lds)
{
    constexpr int WPP = CW / 64;
    v0 = segmented_sum(v0, l.same);
    v1 = segmented_sum(v1, l.same);
    if (l.head) {
        lds[l.wave * CW + l.lt] = v0;
        lds[1024 + l.wave * CW + l.lt] = v1;
    }
    __syncthreads();
    if (l.lc < k.nt) {  // one thread per (group of wavefronts, target)
        const int lt = l.lc, w0 = (l.wave / WPP) * WPP;
        const int lo = (lt * k.m_loc) / 64, hi = ((lt + 1) * k.m_loc - 1) / 64;
        double s0 = lds[(w0 + lo) * CW + lt], s1 = lds[1024 + (w0 + lo) * CW + lt];
        for (int w = lo + 1; w <= hi; ++w) {
            s0 += lds[(w0 + w) * CW + lt];
            s1 += lds[1024 + (w0 + w) * CW + lt];
        }
        put_target(a, k, lt, a0, s0);
        put_target(a, k, lt, a1, s1);
    }
    __syncthreads();
}

// Sums A0 .. A0 + NV - 1 of one chain over the rows r0 .. r1 - 1: sum index j < D is sum x_j, D + t the t-th product of the
// triangle (row-major, i <= j) or of the diagonal.  Everything is unrolled: the indices are constants, v stays in registers.
template <int D, bool DIAG, int A0, int NV, int NVP>
__device__ __forceinline__ void walk_rows(const double *__restrict__ p, int64_t sr, int64_t sj, int64_t r0, int64_t r1,
                                          double (&v)[NVP])
{
#pragma unroll 2
    for (int64_t r = r0; r < r1; ++r) {
        const double *q = p + r * sr;
        double x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = q[j * sj];
#pragma unroll
        for (int j = 0; j < D; ++j)
            if (j >= A0 && j < A0 + NV) v[j - A0] += x[j];
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int j = i; j < (DIAG ? i + 1 : D); ++j) {
                const int ai = DIAG ? D + i : D + i * D - i * (i - 1) / 2 + (j - i);
                if (ai >= A0 && ai < A0 + NV) v[ai - A0] = fma(x[i], x[j], v[ai - A0]);
            }
        }
    }
}

template <int D, bool DIAG, int SPLIT>
__global__ void __launch_bounds__(kBlock) moments_kernel(const MomentsBlock a)
{
    constexpr int CW = kBlock / SPLIT;
    constexpr int NA = D + (DIAG ? D : D * (D + 1) / 2);
    constexpr int NV = (NA + SPLIT - 1) / SPLIT;  // sums a group of wavefronts keeps
    constexpr int NVP = NV + (NV & 1);
    __shared__ double lds[2048];
    const Chunk k = chunk_of<CW>(a);
    const Lane l = lane_of<CW>(k);
    const int part = threadIdx.x / CW;  // uniform in a wavefront
    double v[NVP];
#pragma unroll
    for (int i = 0; i < NVP; ++i) v[i] = 0.0;
    if (l.valid) {
        const double *p = a.x + (k.c0 + l.lc) * a.sc;
        if (SPLIT == 1 || part == 0) walk_rows<D, DIAG, 0, NV, NVP>(p, a.sr, a.sj, k.r0, k.r1, v);
        if (SPLIT > 1 && part == 1) walk_rows<D, DIAG, (SPLIT > 1 ? NV : 0), NV, NVP>(p, a.sr, a.sj, k.r0, k.r1, v);
        if (SPLIT > 2 && part == 2) walk_rows<D, DIAG, (SPLIT > 2 ? 2 * NV : 0), NV, NVP>(p, a.sr, a.sj, k.r0, k.r1, v);
        if (SPLIT > 2 && part == 3) walk_rows<D, DIAG, (SPLIT > 2 ? 3 * NV : 0), NV, NVP>(p, a.sr, a.sj, k.r0, k.r1, v);
    }
    const int first = part * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (first + i < D) put_chain(a, k, l, first + i, v[i]);
#pragma unroll
    for (int i = 0; i < NVP; i += 2) fold2<CW>(a, k, l, v[i], v[i + 1], i < NV ? first + i : NA, i + 1 < NV ? first + i + 1 : NA, lds);
}

// Any d, the diagonal form: one component at a time (a double is still read once; for one (row, component) the chains are
// contiguous as before).
__global__ void __launch_bounds__(kBlock) moments_diag_kernel(const MomentsBlock a)
{
    constexpr int CW = kBlock;
    __shared__ double lds[2048];
    const Chunk k = chunk_of<CW>(a);
    const Lane l = lane_of<CW>(k);
    const double *p = a.x + (k.c0 + l.lc) * a.sc;
    for (int j = 0; j < a.d; ++j) {
        double s = 0.0, ss = 0.0;
        if (l.valid) {
            const double *q = p + j * a.sj;
#pragma unroll 4
            for (int64_t r = k.r0; r < k.r1; ++r) {
                const double x = q[r * a.sr];
                s += x;
                ss = fma(x, x, ss);
            }
        }
        put_chain(a, k, l, j, s);
        fold2<CW>(a, k, l, s, ss, j, a.d + j, lds);
    }
}

// Step 4 with a workspace: one thread per (target, sum) adds the target's partials in (row split, chunk) order.
__global__ void __launch_bounds__(kBlock) moments_fold_targets_kernel(const MomentsBlock a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_targets * a.na) return;
    const int64_t t = i / a.na;
    const int ai = (int)(i % a.na);
    const int64_t stride = a.tpw > 0 ? a.tpw : 1;
    const int64_t b0 = a.tpw > 0 ? t / a.tpw : t * a.cpt, lt = a.tpw > 0 ? t % a.tpw : 0;
    const int64_t nb = a.tpw > 0 ? 1 : a.cpt;
    double s = 0.0;
    for (int64_t sp = 0; sp < a.rsplit; ++sp)
        for (int64_t b = b0; b < b0 + nb; ++b) s += a.ws_t[(size_t)(((sp * a.n_chunks + b) * stride + lt) * a.na + ai)];
    double *row = a.acc + (size_t)t * a.acc_rows;
    row[1 + ai] += s;
    if (ai == 0) row[0] += (double)(a.m * a.n_rows);
}

__global__ void __launch_bounds__(kBlock) moments_fold_chains_kernel(const MomentsBlock a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)a.d * a.n) return;
    double s = 0.0;
    for (int64_t sp = 0; sp < a.rsplit; ++sp) s += a.ws_c[(size_t)(sp * a.d * a.n + i)];
    a.chain_sum[i] += s;
}

using MomentsKernel = void (*)(const MomentsBlock);

template <int D>
MomentsKernel kernel_for(bool diag)
{
    constexpr int SPLIT = D <= 8 ? 1 : (D <= 12 ? 2 : 4);
    return diag ? moments_kernel<D, true, 1> : moments_kernel<D, false, SPLIT>;
}

}  // namespace

int launch_target_moments(const double *x, int64_t n_rows, int64_t n_chains, int d, int64_t chain_rows, int64_t m, bool diag,
                          double *acc, double *chain_sum, hipStream_t st)
{
    MomentsKernel kern = moments_diag_kernel;
    int cw = kBlock;
    switch (d) {
#define GSSS_MOMENTS_CASE(D)                                      \
    case D:                                                       \
        kern = kernel_for<D>(diag);                               \
        cw = diag ? kBlock : kBlock / (D <= 8 ? 1 : (D <= 12 ? 2 : 4)); \
        break;
        GSSS_MOMENTS_CASE(2)
        GSSS_MOMENTS_CASE(3)
        GSSS_MOMENTS_CASE(4)
        GSSS_MOMENTS_CASE(5)
        GSSS_MOMENTS_CASE(6)
        GSSS_MOMENTS_CASE(7)
        GSSS_MOMENTS_CASE(8)
        GSSS_MOMENTS_CASE(9)
        GSSS_MOMENTS_CASE(10)
        GSSS_MOMENTS_CASE(11)
        GSSS_MOMENTS_CASE(12)
        GSSS_MOMENTS_CASE(13)
        GSSS_MOMENTS_CASE(14)
        GSSS_MOMENTS_CASE(15)
        GSSS_MOMENTS_CASE(16)
#undef GSSS_MOMENTS_CASE
    default:
        if (!diag) {
            set_error("the full second-moment triangle is kept for d <= %d (d = %d): use GSSS_MOMENTS_DIAG", kMomentsMaxFullDim, d);
            return GSSS_E_UNSUPPORTED;
        }
    }
    MomentsBlock a{};
    a.x = x;
    if (chain_rows > 0) {
        a.sr = d;
        a.sj = 1;
        a.sc = chain_rows * d;
    } else {
        a.sr = (int64_t)d * n_chains;
        a.sj = n_chains;
        a.sc = 1;
    }
    a.n = n_chains;
    a.n_rows = n_rows;
    a.m = m;
    a.n_targets = n_chains / m;
    a.d = d;
    a.na = (int32_t)moments_sums(d, diag);
    a.acc_rows = 1 + a.na;
    a.acc = acc;
    a.chain_sum = chain_sum;
    if (m <= cw) {
        a.tpw = (int32_t)(cw / m);
        a.n_chunks = ceil_div(a.n_targets, a.tpw);
    } else {
        a.cpt = (int32_t)ceil_div(m, cw);
        a.n_chunks = a.n_targets * a.cpt;
    }
    a.rsplit = 1;
    if (a.n_chunks < kWantGrid) {
        const int64_t most = n_rows / kMinSplitRows, want = ceil_div(kWantGrid, a.n_chunks);
        a.rsplit = (int32_t)(most < 1 ? 1 : (want < most ? want : most));
    }
    if (ceil_div(m, cw) > 0x7FFFFFFFll || a.n_chunks * a.rsplit > 0x7FFFFFFFll || a.n_targets * a.na > 0x7FFFFFFFll * kBlock ||
        n_chains * (int64_t)d > 0x7FFFFFFFll * kBlock) {
        set_error("gsss_target_moments: %lld chains of %lld per target exceed the grid", (long long)n_chains, (long long)m);
        return GSSS_E_UNSUPPORTED;
    }
    // A workspace only where a target or a chain has more than one partial; taken and freed in stream order, like gsss_run's.
    const bool ws_t = a.rsplit > 1 || a.tpw == 0, ws_c = chain_sum && a.rsplit > 1;
    const size_t n_t = ws_t ? (size_t)a.rsplit * a.n_chunks * (a.tpw > 0 ? a.tpw : 1) * a.na : 0;
    const size_t n_c = ws_c ? (size_t)a.rsplit * d * n_chains : 0;
    void *ws = nullptr;
    if (n_t + n_c > 0) {
        GSSS_HIP_TRY(hipMallocAsync(&ws, (n_t + n_c) * sizeof(double), st));
        if (ws_t) a.ws_t = static_cast<double *>(ws);
        if (ws_c) a.ws_c = static_cast<double *>(ws) + n_t;
    }
    int rc = launch_kernel("moments", kern, a.n_chunks * a.rsplit, 0, st, nullptr, a);
    if (rc == GSSS_OK && ws_t)
        rc = launch_kernel("moments fold", moments_fold_targets_kernel, ceil_div(a.n_targets * a.na, kBlock), 0, st, nullptr, a);
    if (rc == GSSS_OK && ws_c)
        rc = launch_kernel("moments fold", moments_fold_chains_kernel, ceil_div((int64_t)d * n_chains, kBlock), 0, st, nullptr, a);
    if (ws) (void)hipFreeAsync(ws, st);
    return rc;
}

}  // namespace gsss
