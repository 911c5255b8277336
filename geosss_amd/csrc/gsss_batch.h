// gsss_batch.h -- host side of the batch builds: many targets of one family and shape in one launch (gsss_target_create_batch).
// Target t owns the chains [t m, (t + 1) m); the grid is targets x ceil(m / chains per workgroup), and a workgroup derives its
// target and its chunk of that target's chains from blockIdx.x (BatchBlock, gsss_device.h).  The kernels are instantiations of
// their own (the BATCH flag of run_kernel, screened_kernel and fast_kernel), built in the gsss_batch_*.hip units only.
#pragma once
#include "gsss_fast_bingham_lane.h"
#include "gsss_fast_vmf_lane.h"
#include "gsss_launch.h"

namespace gsss {

struct BatchInfo {
    int32_t n_targets;  // 0: not a batch
    int64_t stride;     // doubles from one member's blob to the next
    int64_t m;          // chains per target
};

// the launch of rb.n_chains chains (a multiple of m, checked by gsss_run) in workgroups of per_block chains
inline int batch_grid(const RunBlock &rb, const BatchInfo &bi, int64_t per_block, BatchBlock &bb, int64_t &grid)
{
    bb.stride = bi.stride;
    bb.m = (int32_t)bi.m;
    bb.chunks = (int32_t)ceil_div(bi.m, per_block);
    grid = (rb.n_chains / bi.m) * (int64_t)bb.chunks;
    if (grid > 0x7FFFFFFFll) {
        set_error("target batch: %lld workgroups exceed the grid (fewer targets per launch)", (long long)grid);
        return GSSS_E_UNSUPPORTED;
    }
    return GSSS_OK;
}

// exact mode: run_kernel<.., BATCH> in the layout gsss_run selected, packed or spread
template <class V, template <class> class TT>
int do_run_batch(const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    using T = TT<V>;
    const size_t lds = (T::lds_doubles(tb.k, tb.d) + scratch_doubles<V, T>() + PhiloxDraws<V>::kLdsDoubles) * sizeof(double);
    if (lds > kMaxLdsBytes) {
        set_error("target parameters need %zu B of LDS (> %zu)", lds, kMaxLdsBytes);
        return GSSS_E_UNSUPPORTED;
    }
    auto kern = run_kernel<V, TT, PhiloxDraws, false, true, BatchBlock>;
    if (int rc = allow_lds("run batch", kern, lds)) return rc;
    BatchBlock bb;
    int64_t grid;
    if (int rc = batch_grid(rb, bi, (V::L == 1 && rb.spread) ? kBlock / 64 : kBlock / V::L, bb, grid)) return rc;
    return launch_kernel("run batch", kern, grid, lds, st, nullptr, tb, rb, bb);
}
int launch_batch_run_vmf(int vec_id, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);
int launch_batch_run_bingham(int vec_id, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);

// fast mode: one chain per lane, nothing parked, never sliced -- whatever the placement asked for
inline RunBlock batch_lane_args(const RunBlock &rb)
{
    RunBlock rbl = rb;
    rbl.spread = 0;
    rbl.one_per_lane = 1;
    rbl.stage_rows = 0;
    rbl.stats_onchip = 0;
    rbl.sched = nullptr;
    rbl.slice_steps = 0;
    rbl.sched_first = 0;
    return rbl;
}

template <int D, class TP>
int do_screened_batch(const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    const size_t lds = (TP::lds_doubles() + kTabLds) * sizeof(double);
    auto kern = screened_kernel<D, TP, false, false, false, false, true, BatchBlock>;
    if (int rc = allow_lds("screened batch", kern, lds)) return rc;
    BatchBlock bb;
    int64_t grid;
    if (int rc = batch_grid(rb, bi, kBlock, bb, grid)) return rc;
    last_launch() = LaunchInfo{grid, 0, 0.0};
    return launch_kernel("screened batch", kern, grid, lds, st, nullptr, tb, batch_lane_args(rb), bb);
}

template <int D, class TP>
int do_fast_batch(const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    const size_t lds = (TP::lds_doubles() + kTabLds) * sizeof(double);
    auto kern = fast_kernel<D, TP, false, false, false, true, BatchBlock>;
    if (int rc = allow_lds("fast batch", kern, lds)) return rc;
    BatchBlock bb;
    int64_t grid;
    if (int rc = batch_grid(rb, bi, kBlock, bb, grid)) return rc;
    last_launch() = LaunchInfo{grid, 0, 0.0};
    return launch_kernel("fast batch", kern, grid, lds, st, nullptr, tb, batch_lane_args(rb), bb);
}

// The batch launchers: a switch over the pick (gsss_fast_select.h -- the buckets, and where the batch build departs from the
// single-target one).  vMF mixtures, d = 3 .. 10: screened 3, 4, 6, 10, 16; all-double 4, 16
template <int D>
int batch_lane_vmf(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamScreened) {
        switch (p.kc) {
        case 3: return do_screened_batch<D, ScreenVmf<D, 3>>(tb, rb, bi, st);
        case 4: return do_screened_batch<D, ScreenVmf<D, 4>>(tb, rb, bi, st);
        case 6: return do_screened_batch<D, ScreenVmf<D, 6>>(tb, rb, bi, st);
        case 10: return do_screened_batch<D, ScreenVmf<D, 10>>(tb, rb, bi, st);
        case 16: return do_screened_batch<D, ScreenVmf<D, 16>>(tb, rb, bi, st);
        }
    } else if (p.family == kFamFast) {
        if (p.kc == 4) return do_fast_batch<D, FastVmf<D, 4>>(tb, rb, bi, st);
        if (p.kc == 16) return do_fast_batch<D, FastVmf<D, 16>>(tb, rb, bi, st);
    }
    return pick_error(p);
}
// d = 11 .. 16, K <= 10: screened 3, 6, 10; all-double 4, 10
template <int D>
int batch_lane_vmf_wide(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamScreened) {
        if (p.kc == 3) return do_screened_batch<D, ScreenVmf<D, 3>>(tb, rb, bi, st);
        if (p.kc == 6) return do_screened_batch<D, ScreenVmf<D, 6>>(tb, rb, bi, st);
        if (p.kc == 10) return do_screened_batch<D, ScreenVmf<D, 10>>(tb, rb, bi, st);
    } else if (p.family == kFamFast) {
        if (p.kc == 4) return do_fast_batch<D, FastVmf<D, 4>>(tb, rb, bi, st);
        if (p.kc == 10) return do_fast_batch<D, FastVmf<D, 10>>(tb, rb, bi, st);
    }
    return pick_error(p);
}
// Bingham / Fisher-Bingham, d = 3 .. 16
template <int D>
int batch_lane_bingham(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamFast) return do_fast_batch<D, FastBingham<D>>(tb, rb, bi, st);
    if (p.family != kFamScreened) return pick_error(p);
    if (p.flavour == kFlavBinghamDiag) return do_screened_batch<D, ScreenBinghamDiag<D>>(tb, rb, bi, st);
    return do_screened_batch<D, ScreenBingham<D>>(tb, rb, bi, st);
}

#define GSSS_BATCH_LANE_DIMS(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
#define GSSS_BATCH_WIDE_DIMS(X) X(11) X(12) X(13) X(14) X(15) X(16)
#define GSSS_DECLARE(D) \
    extern template int batch_lane_vmf<D>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t); \
    extern template int batch_lane_bingham<D>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
GSSS_BATCH_LANE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE
#define GSSS_DECLARE(D) \
    extern template int batch_lane_vmf_wide<D>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t); \
    extern template int batch_lane_bingham<D>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
GSSS_BATCH_WIDE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE

int launch_batch_fast_vmf(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);
int launch_batch_fast_bingham(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);

}  // namespace gsss
