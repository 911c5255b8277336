// gsss_target_fold.h -- how the per-target statistics (gsss_moments.hip, gsss_autocov.hip, gsss_mixing.hip) cut a batch's
// chains into workgroups and fold the lanes' sums into one sum per target: the one home of that policy, device and host side.
//
// The cut.  A workgroup takes CW consecutive chains, one chain per lane (CW = 256, 128 or 64: kBlock / CW groups of wavefronts
// walk the same chains and share the sums), ONE of the `series` series (autocov: the d components; 1 otherwise) and a run of the
// block's rows.  Chunks of chains are cut at target boundaries: with m <= CW a workgroup takes tpw = floor(CW / m) whole targets
// (a unit may cap tpw further), otherwise a target takes cpt = ceil(m / CW) workgroups.  The rows are split over workgroups as
// well, rsplit ways, only when chunks x series give fewer than kWantGrid workgroups, and never into runs of fewer than the
// unit's min_split_rows rows.  blockIdx.x = (row split * series + series index) * n_chunks + chunk.
//
// Summation order (fixed by the arguments alone, no floating-point atomics: a call's result is the same bits every time).
//   1. a lane adds its chain's rows in row order;
//   2. the lanes of a wavefront are combined by a SEGMENTED shuffle reduction (offsets 1, 2, .. 32; a lane adds its neighbour
//      only if that neighbour belongs to the same target), which leaves a target's sum in the first of its lanes;
//   3. the wavefronts a target spans are added in wavefront order through LDS by one thread per target;
//   4. where a target has a single partial (m <= CW and the rows are not split over workgroups) that thread adds it to the
//      output; otherwise the partials go to a workspace and a second kernel (fold_partials) adds them per target in
//      (row split, chunk) order.
// tests/test_hip_target_fold_order.py holds the kernels to this order bit for bit.
#pragma once
#include "gsss_launch.h"

namespace gsss {

constexpr int kWantGrid = 1024;  // workgroups below which the rows are split as well

struct TargetCut {
    int64_t n_rows, m, n_targets, n_chunks;
    int32_t rsplit;
    int32_t tpw;     // targets a workgroup takes (m <= CW), else 0
    int32_t cpt;     // workgroups a target takes (m > CW), else 0
    int32_t series;
};

// targets that a workgroup's partials have room for in the workspace (and in a unit's LDS)
__host__ __device__ __forceinline__ int32_t chunk_targets(const TargetCut &c) { return c.tpw > 0 ? c.tpw : 1; }

struct Chunk {
    int64_t c0, t0;    // first chain, first target
    int32_t nc, nt;    // chains, targets
    int32_t m_loc;     // chains per target within the chunk
    int64_t r0, r1;    // rows, relative to the block's first
    int32_t split, j;  // row split, series
};

// SERIES = false: the cut has one series (no division by it).
template <int CW, bool SERIES>
__device__ __forceinline__ Chunk chunk_of(const TargetCut &a)
{
    Chunk k;
    const int64_t b = (int64_t)blockIdx.x % a.n_chunks, rest = (int64_t)blockIdx.x / a.n_chunks;
    k.split = (int32_t)(SERIES ? rest / a.series : rest);
    k.j = SERIES ? (int32_t)(rest % a.series) : 0;
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

// NS sums per lane -> per target: steps 2 and 3 of the summation order.  The thread l.lc < k.nt of a group of wavefronts is left
// with the sums of target l.lc of the chunk in v (the lane's own sums have gone into them); the caller puts them out (step 4).
// lds: sum i of wavefront w and target lt at [i * sum_stride + w * wave_stride + lt].  Every thread of the workgroup calls it,
// and a workgroup that uses lds again afterwards puts a __syncthreads() between.
template <int CW, int NS>
__device__ __forceinline__ void fold(const Chunk &k, const Lane &l, double (&v)[NS], double *lds, int wave_stride, int sum_stride)
{
    constexpr int WPP = CW / 64;
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = segmented_sum(v[i], l.same);
    if (l.head) {
#pragma unroll
        for (int i = 0; i < NS; ++i) lds[i * sum_stride + l.wave * wave_stride + l.lt] = v[i];
    }
    __syncthreads();
    if (l.lc < k.nt) {  // one thread per (group of wavefronts, target)
        const int lt = l.lc, w0 = (l.wave / WPP) * WPP;
        const int lo = (lt * k.m_loc) / 64, hi = ((lt + 1) * k.m_loc - 1) / 64;
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] = lds[i * sum_stride + (w0 + lo) * wave_stride + lt];
        for (int w = lo + 1; w <= hi; ++w) {
#pragma unroll
            for (int i = 0; i < NS; ++i) v[i] += lds[i * sum_stride + (w0 + w) * wave_stride + lt];
        }
    }
}

// The workspace of step 4, [rsplit][series][n_chunks][chunk_targets][na]: where this workgroup puts the na partials of its
// target lt.
__device__ __forceinline__ double *partials_of(const TargetCut &a, double *ws, int lt, int na)
{
    return ws + ((size_t)blockIdx.x * chunk_targets(a) + lt) * na;
}

struct TargetFold {
    TargetCut cut;
    const double *ws;
    double *out;  // sum ai of (target t, series j) at [(t * series + j) * out_stride + out_offset + ai]
    int64_t out_stride;
    int32_t out_offset, na;
};

// Step 4 with a workspace, the whole body of a unit's fold kernel (kBlock threads; each unit gives the kernel its own name, so
// that no kernel symbol is shared between translation units): one thread per (target, series, sum) adds the target's partials
// in (row split, chunk) order.  COUNT: the row's first entry counts the draws (moments).
template <bool COUNT>
__device__ __forceinline__ void fold_partials(const TargetFold &f)
{
    const TargetCut &a = f.cut;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_targets * a.series * f.na) return;
    const int64_t t = i / ((int64_t)a.series * f.na), j = i / f.na % a.series;
    const int ai = (int)(i % f.na);
    const int64_t stride = chunk_targets(a);
    const int64_t b0 = a.tpw > 0 ? t / a.tpw : t * a.cpt, lt = a.tpw > 0 ? t % a.tpw : 0;
    const int64_t nb = a.tpw > 0 ? 1 : a.cpt;
    double s = 0.0;
    for (int64_t sp = 0; sp < a.rsplit; ++sp)
        for (int64_t b = b0; b < b0 + nb; ++b) s += f.ws[(size_t)((((sp * a.series + j) * a.n_chunks + b) * stride + lt) * f.na + ai)];
    double *row = f.out + (size_t)(t * a.series + j) * f.out_stride;
    row[f.out_offset + ai] += s;
    if (COUNT && ai == 0) row[0] += (double)(a.m * a.n_rows);
}

// ------------------------------------------------------------------------------------------
// Host side.
inline int exceeds_grid(const char *entry, int64_t n_chains, int64_t m)
{
    set_error("%s: %lld chains of %lld per target exceed the grid", entry, (long long)n_chains, (long long)m);
    return GSSS_E_UNSUPPORTED;
}

// The cut of n_chains chains, m per target, for workgroups of cw chains that take at most tpw_cap targets each; na sums per
// (target, series).  Refuses what the grids of the walk and of the fold cannot index.
inline int make_cut(const char *entry, int64_t n_chains, int64_t m, int cw, int64_t tpw_cap, int64_t n_rows, int min_split_rows,
                    int series, int64_t na, TargetCut &a)
{
    a = TargetCut{};
    a.n_rows = n_rows;
    a.m = m;
    a.n_targets = n_chains / m;
    a.series = series;
    if (m <= cw) {
        a.tpw = (int32_t)(cw / m < tpw_cap ? cw / m : tpw_cap);
        a.n_chunks = ceil_div(a.n_targets, a.tpw);
    } else {
        a.cpt = (int32_t)ceil_div(m, cw);
        a.n_chunks = a.n_targets * a.cpt;
    }
    a.rsplit = 1;
    if (a.n_chunks * series < kWantGrid) {
        const int64_t most = n_rows / min_split_rows, want = ceil_div(kWantGrid, a.n_chunks * series);
        a.rsplit = (int32_t)(most < 1 ? 1 : (want < most ? want : most));
    }
    if (ceil_div(m, cw) > 0x7FFFFFFFll || a.n_chunks * series * a.rsplit > 0x7FFFFFFFll ||
        a.n_targets * series * na > 0x7FFFFFFFll * kBlock)
        return exceeds_grid(entry, n_chains, m);
    return GSSS_OK;
}

// Steps 1 - 4 on the stream: walk(ws, extra) launches the unit's walk kernel on n_chunks * series * rsplit workgroups -- ws:
// where partials_of puts the targets' partials, NULL where a target has a single partial and the kernel adds it to f.out itself;
// extra: `n_extra` doubles more for the unit's own use, NULL if 0 -- then fold_kernel(f), the unit's kernel around fold_partials.
// A workspace only where something has more than one partial; taken and freed in stream order, like gsss_run's.
template <class Fold, class Walk>
int launch_walk_and_fold(const char *fold_family, Fold fold_kernel, TargetFold f, size_t n_extra, hipStream_t st, Walk &&walk)
{
    const TargetCut &a = f.cut;
    const bool partials = a.rsplit > 1 || a.tpw == 0;
    const size_t n_ws = partials ? (size_t)a.rsplit * a.series * a.n_chunks * chunk_targets(a) * f.na : 0;
    void *ws = nullptr;
    if (n_ws + n_extra > 0) GSSS_HIP_TRY(hipMallocAsync(&ws, (n_ws + n_extra) * sizeof(double), st));
    double *base = static_cast<double *>(ws);
    f.ws = partials ? base : nullptr;
    int rc = walk(partials ? base : nullptr, n_extra > 0 ? base + n_ws : nullptr);
    if (rc == GSSS_OK && partials)
        rc = launch_kernel(fold_family, fold_kernel, ceil_div(a.n_targets * a.series * f.na, kBlock), 0, st, nullptr, f);
    if (ws) (void)hipFreeAsync(ws, st);
    return rc;
}

}  // namespace gsss
