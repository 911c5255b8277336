// gsss_moments.hip -- per-target moments of retained draws (gsss_target_moments): one pass over a block of draws, folded into
// acc[M][1 + d + T] per TARGET (count, sum x_j, sum x_i x_j) and, optionally, the per-chain sums chain_sum[d][n].
//
// Layout.  A workgroup (256 threads) takes CW consecutive chains, one chain per lane, and a run of the block's rows; a lane
// keeps the sums of ITS chain in registers while it walks the rows (component-major input: for one (row, component) a wavefront
// reads 64 consecutive doubles).  The d + T sums of a chain are split evenly over SPLIT groups of wavefronts that walk the same
// chains -- SPLIT = 1 (CW = 256) up to d = 8, 2 (CW = 128) up to d = 12, 4 (CW = 64) up to d = 16 -- so that no lane holds more
// than 45 sums and nothing spills; the groups' reads of the same doubles meet in the cache, every double leaves HBM once.
// The cut of the chains at target boundaries, the split of the rows over workgroups and the summation order (steps 1 - 4) are
// gsss_target_fold.h's, with CW as above and one series.  A chain's sums for chain_sum are its lane's (step 1); where the rows
// are split they go to a workspace [rsplit][d][n] and a second kernel adds them per chain in row-split order.
#include "gsss_moments.h"
#include "gsss_target_fold.h"

namespace gsss {
namespace {

constexpr int kMinSplitRows = 8;

struct MomentsBlock {
    const double *x;
    int64_t sr, sj, sc;  // doubles from row to row, component to component, chain to chain
    int64_t n;
    TargetCut cut;
    int32_t d, na, acc_rows;
    double *acc, *chain_sum;
    double *ws_t;        // NULL: a target has one partial, added to acc directly; else the workspace of partials_of
    double *ws_c;        // NULL: chain sums are added to chain_sum directly; else [rsplit][d][n]
};

// Step 4 for sum ai (>= na: none) of target lt of the chunk.
__device__ __forceinline__ void put_target(const MomentsBlock &a, const Chunk &k, int lt, int ai, double s)
{
    if (ai >= a.na) return;
    if (a.ws_t) {
        partials_of(a.cut, a.ws_t, lt, a.na)[ai] = s;
        return;
    }
    double *row = a.acc + (size_t)(k.t0 + lt) * a.acc_rows;
    row[1 + ai] += s;
    if (ai == 0) row[0] += (double)(a.cut.m * a.cut.n_rows);
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
    double s[2] = {v0, v1};
    fold<CW, 2>(k, l, s, lds, CW, 1024);
    if (l.lc < k.nt) {
        put_target(a, k, l.lc, a0, s[0]);
        put_target(a, k, l.lc, a1, s[1]);
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
    const Chunk k = chunk_of<CW, false>(a.cut);
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
    const Chunk k = chunk_of<CW, false>(a.cut);
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

// Step 4 with a workspace.
__global__ void __launch_bounds__(kBlock) moments_fold_targets_kernel(const TargetFold f) { fold_partials<true>(f); }

// chain_sum where the rows are split: one thread per (component, chain) adds the chain's partials in row-split order.
__global__ void __launch_bounds__(kBlock) moments_fold_chains_kernel(const MomentsBlock a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)a.d * a.n) return;
    double s = 0.0;
    for (int64_t sp = 0; sp < a.cut.rsplit; ++sp) s += a.ws_c[(size_t)(sp * a.d * a.n + i)];
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
    a.d = d;
    a.na = (int32_t)moments_sums(d, diag);
    a.acc_rows = 1 + a.na;
    a.acc = acc;
    a.chain_sum = chain_sum;
    if (int rc = make_cut("gsss_target_moments", n_chains, m, cw, cw, n_rows, kMinSplitRows, 1, a.na, a.cut)) return rc;
    if (n_chains * (int64_t)d > 0x7FFFFFFFll * kBlock) return exceeds_grid("gsss_target_moments", n_chains, m);
    const bool ws_c = chain_sum && a.cut.rsplit > 1;  // (a chain has more than one partial)
    const size_t n_c = ws_c ? (size_t)a.cut.rsplit * d * n_chains : 0;
    const TargetFold f{a.cut, nullptr, acc, a.acc_rows, 1, a.na};
    return launch_walk_and_fold("moments fold", moments_fold_targets_kernel, f, n_c, st, [&](double *ws_t, double *ws_chains) {
        a.ws_t = ws_t;
        a.ws_c = ws_chains;
        int rc = launch_kernel("moments", kern, a.cut.n_chunks * a.cut.rsplit, 0, st, nullptr, a);
        if (rc == GSSS_OK && ws_c)
            rc = launch_kernel("moments fold", moments_fold_chains_kernel, ceil_div((int64_t)d * n_chains, kBlock), 0, st, nullptr, a);
        return rc;
    });
}

}  // namespace gsss
