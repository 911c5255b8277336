// gsss_batch.h -- host side of the batch builds: many targets of one family and shape in one launch (gsss_target_create_batch).
// Target t owns the chains [t m, (t + 1) m).  The kernels are instantiations of their own (the BATCH flag of run_kernel,
// screened_kernel and fast_kernel) and come in two workgroup layouts, told apart by the type of the block they take
// (gsss_device.h):
//   BatchBlock   one target per workgroup: the grid is targets x chunks, and a workgroup derives its target and its chunk of that
//                target's chains from blockIdx.x.  Exact mode always (chains per workgroup follow the lane group: do_run_batch);
//                fast mode when m is a multiple of the workgroup's 256 chains.
//   BatchShared  fast mode, any other m: a workgroup takes a run of consecutive chains of the launch, whichever targets they belong
//                to, and stages all of those targets' blobs (stage_shared, gsss_fast.h).
// What a fast-mode launch looks like -- the layout, chains and targets per workgroup, the grid -- is batch_plan's
// (gsss_fast_select.h), the same call gsss_batch_plan answers from; the launchers below are written once over the layout BB.
// The instantiations live in the gsss_batch_*.hip units (BatchBlock) and the gsss_batch_shared_*.hip units (BatchShared) only.
#pragma once
#include "gsss_fast_bingham_lane.h"
#include "gsss_fast_vmf_lane.h"
#include "gsss_launch.h"

namespace gsss {

static_assert(kBatchTabDoubles == kTabLds && kBatchLdsBytes == (long)kMaxLdsBytes && kBatchBlock == kBlock,
              "batch_plan budgets the LDS of these kernels");

struct BatchInfo {
    int32_t n_targets;  // 0: not a batch
    int64_t stride;     // doubles from one member's blob to the next
    int64_t m;          // chains per target
};

inline int batch_grid_fits(int64_t grid)
{
    if (grid <= 0x7FFFFFFFll) return GSSS_OK;
    set_error("target batch: %lld workgroups exceed the grid (fewer targets per launch)", (long long)grid);
    return GSSS_E_UNSUPPORTED;
}

// exact mode: run_kernel<.., BATCH> in the layout gsss_run selected, packed or spread, for the rb.n_chains chains of the launch (a
// multiple of m, checked by gsss_run)
template <class V, template <class> class TT>
int do_run_batch(const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    const int64_t per_block = (V::L == 1 && rb.spread) ? kBlock / 64 : kBlock / V::L;
    BatchBlock bb;
    bb.stride = bi.stride;
    bb.m = (int32_t)bi.m;
    bb.chunks = (int32_t)ceil_div(bi.m, per_block);
    const int64_t grid = (rb.n_chains / bi.m) * (int64_t)bb.chunks;
    if (int rc = batch_grid_fits(grid)) return rc;
    return launch_exact<V, TT, PhiloxDraws<V>::kLdsDoubles>("run batch", run_kernel<V, TT, PhiloxDraws, false, true, BatchBlock>, grid, st,
                                                            tb, rb, bb);
}
// the batch's family (vMF mixtures, else Bingham) in the layout vec_id: gsss_batch_exact.hip
int launch_batch_run(int vec_id, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);

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

// the launch of a fast-mode plan in the layout BB (bp.shared says which).  LDS: the tables and the rows of bp.targets members --
// one target's rows as they are, or those of a shared workgroup at the build's stride
template <class TP, class BB, class Kern>
int launch_batch(const char *family, Kern kern, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    constexpr bool kShared = kIsBatchShared<BB>;
    const size_t per_target = kShared ? (size_t)shared_stride<TP>() : TP::lds_doubles();
    const size_t lds = ((size_t)kTabLds + (size_t)bp.targets * per_target) * sizeof(double);
    if (int rc = allow_lds(family, kern, lds)) return rc;
    if (int rc = batch_grid_fits(bp.grid)) return rc;
    BB bb;
    bb.stride = bi.stride;
    bb.m = (int32_t)bi.m;
    if constexpr (kShared)
        bb.per_block = bp.per_block;
    else
        bb.chunks = (int32_t)(bi.m / kBlock);
    last_launch() = LaunchInfo{bp.grid, 0, 0.0};
    if (getenv("GSSS_DEBUG_OCCUPANCY")) {  // (what tests/test_hip_target_batch_shared.py holds against launch_plan)
        int per_cu = 0;
        resident_workgroups(reinterpret_cast<const void *>(kern), lds, &per_cu);
        fprintf(stderr, "gsss: %s: grid %lld, %d chains and %d targets a workgroup, %d doubles a target, %zu B of LDS, %d workgroups per CU\n",
                family, (long long)bp.grid, bp.per_block, bp.targets, (int)per_target, lds, per_cu);
    }
    return launch_kernel(family, kern, bp.grid, lds, st, nullptr, tb, batch_lane_args(rb), bb);
}

template <int D, class TP, class BB>
int do_screened_batch(const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    return launch_batch<TP, BB>(kIsBatchShared<BB> ? "screened batch shared" : "screened batch",
                                screened_kernel<D, TP, false, false, false, false, true, BB>, bp, tb, rb, bi, st);
}
template <int D, class TP, class BB>
int do_fast_batch(const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    return launch_batch<TP, BB>(kIsBatchShared<BB> ? "fast batch shared" : "fast batch", fast_kernel<D, TP, false, false, false, true, BB>, bp,
                                tb, rb, bi, st);
}

// The batch launchers: a switch over the pick (gsss_fast_select.h -- the buckets, and where the batch build departs from the
// single-target one).  vMF mixtures, d = 3 .. 10: screened 3, 4, 6, 10, 16; all-double 4, 16
template <int D, class BB>
int batch_lane_vmf(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamScreened) {
        switch (p.kc) {
        case 3: return do_screened_batch<D, ScreenVmf<D, 3>, BB>(bp, tb, rb, bi, st);
        case 4: return do_screened_batch<D, ScreenVmf<D, 4>, BB>(bp, tb, rb, bi, st);
        case 6: return do_screened_batch<D, ScreenVmf<D, 6>, BB>(bp, tb, rb, bi, st);
        case 10: return do_screened_batch<D, ScreenVmf<D, 10>, BB>(bp, tb, rb, bi, st);
        case 16: return do_screened_batch<D, ScreenVmf<D, 16>, BB>(bp, tb, rb, bi, st);
        }
    } else if (p.family == kFamFast) {
        if (p.kc == 4) return do_fast_batch<D, FastVmf<D, 4>, BB>(bp, tb, rb, bi, st);
        if (p.kc == 16) return do_fast_batch<D, FastVmf<D, 16>, BB>(bp, tb, rb, bi, st);
    }
    return pick_error(p);
}
// d = 11 .. 16, K <= 10: screened 3, 6, 10; all-double 4, 10
template <int D, class BB>
int batch_lane_vmf_wide(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamScreened) {
        if (p.kc == 3) return do_screened_batch<D, ScreenVmf<D, 3>, BB>(bp, tb, rb, bi, st);
        if (p.kc == 6) return do_screened_batch<D, ScreenVmf<D, 6>, BB>(bp, tb, rb, bi, st);
        if (p.kc == 10) return do_screened_batch<D, ScreenVmf<D, 10>, BB>(bp, tb, rb, bi, st);
    } else if (p.family == kFamFast) {
        if (p.kc == 4) return do_fast_batch<D, FastVmf<D, 4>, BB>(bp, tb, rb, bi, st);
        if (p.kc == 10) return do_fast_batch<D, FastVmf<D, 10>, BB>(bp, tb, rb, bi, st);
    }
    return pick_error(p);
}
// Bingham / Fisher-Bingham, d = 3 .. 16
template <int D, class BB>
int batch_lane_bingham(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamFast) return do_fast_batch<D, FastBingham<D>, BB>(bp, tb, rb, bi, st);
    if (p.family != kFamScreened) return pick_error(p);
    if (p.flavour == kFlavBinghamDiag) return do_screened_batch<D, ScreenBinghamDiag<D>, BB>(bp, tb, rb, bi, st);
    return do_screened_batch<D, ScreenBingham<D>, BB>(bp, tb, rb, bi, st);
}

// built per dimension and layout in the gsss_batch_*.hip / gsss_batch_shared_*.hip units
#define GSSS_BATCH_ARGS const FastPick &, const BatchPlan &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t
#define GSSS_BATCH_LANE_DIMS(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
#define GSSS_BATCH_WIDE_DIMS(X) X(11) X(12) X(13) X(14) X(15) X(16)
#define GSSS_DECLARE(D) \
    extern template int batch_lane_vmf<D, BatchBlock>(GSSS_BATCH_ARGS); \
    extern template int batch_lane_vmf<D, BatchShared>(GSSS_BATCH_ARGS);
GSSS_BATCH_LANE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE
#define GSSS_DECLARE(D) \
    extern template int batch_lane_vmf_wide<D, BatchBlock>(GSSS_BATCH_ARGS); \
    extern template int batch_lane_vmf_wide<D, BatchShared>(GSSS_BATCH_ARGS);
GSSS_BATCH_WIDE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE
#define GSSS_DECLARE(D) \
    extern template int batch_lane_bingham<D, BatchBlock>(GSSS_BATCH_ARGS); \
    extern template int batch_lane_bingham<D, BatchShared>(GSSS_BATCH_ARGS);
GSSS_BATCH_LANE_DIMS(GSSS_DECLARE)
GSSS_BATCH_WIDE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE

// GSSS_MODE_FAST launchers of a batch: the pick's dimension, in the plan's layout
template <class BB>
int launch_batch_fast_vmf(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_vmf<D, BB>(p, bp, tb, rb, bi, st);
        GSSS_BATCH_LANE_DIMS(GSSS_CASE)
#undef GSSS_CASE
#define GSSS_CASE(D) \
    case D: return batch_lane_vmf_wide<D, BB>(p, bp, tb, rb, bi, st);
        GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}
template <class BB>
int launch_batch_fast_bingham(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_bingham<D, BB>(p, bp, tb, rb, bi, st);
        GSSS_BATCH_LANE_DIMS(GSSS_CASE)
        GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
