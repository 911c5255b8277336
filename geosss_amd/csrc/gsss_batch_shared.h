// gsss_batch_shared.h -- host side of the SHARED batch builds of the lane kernels (fast mode, d = 3 .. 16): a workgroup takes a run
// of consecutive chains of the launch, whichever targets they belong to, and stages all of those targets' blobs (BatchShared,
// gsss_device.h; stage_shared, gsss_fast.h).  What a launch looks like -- chains and targets per workgroup, the grid -- is
// batch_plan's (gsss_fast_select.h), the same call gsss_batch_plan answers from; a plan that is not shared (m a multiple of the
// workgroup's chains) runs the builds of gsss_batch.h.  The instantiations live in the gsss_batch_shared_*.hip units only.
#pragma once
#include "gsss_batch.h"

namespace gsss {

static_assert(kBatchTabDoubles == kTabLds && kBatchLdsBytes == (long)kMaxLdsBytes && kBatchBlock == kBlock,
              "batch_plan budgets the LDS of these kernels");

// the launch of a shared plan: the tables, then bp.targets members at the build's stride
template <class TP, class Kern>
int launch_shared(const char *family, Kern kern, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    const size_t lds = ((size_t)kTabLds + (size_t)bp.targets * shared_stride<TP>()) * sizeof(double);
    if (int rc = allow_lds(family, kern, lds)) return rc;
    if (bp.grid > 0x7FFFFFFFll) {
        set_error("target batch: %lld workgroups exceed the grid (fewer targets per launch)", (long long)bp.grid);
        return GSSS_E_UNSUPPORTED;
    }
    BatchShared sb;
    sb.stride = bi.stride;
    sb.m = (int32_t)bi.m;
    sb.per_block = bp.per_block;
    last_launch() = LaunchInfo{bp.grid, 0, 0.0};
    if (getenv("GSSS_DEBUG_OCCUPANCY")) {  // (what tests/test_hip_target_batch_shared.py holds against launch_plan)
        int per_cu = 0;
        resident_workgroups(reinterpret_cast<const void *>(kern), lds, &per_cu);
        fprintf(stderr, "gsss: %s: grid %lld, %d chains and %d targets a workgroup, %d doubles a target, %zu B of LDS, %d workgroups per CU\n",
                family, (long long)bp.grid, bp.per_block, bp.targets, (int)shared_stride<TP>(), lds, per_cu);
    }
    return launch_kernel(family, kern, bp.grid, lds, st, nullptr, tb, batch_lane_args(rb), sb);
}

template <int D, class TP>
int do_screened_shared(const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    return launch_shared<TP>("screened batch shared", screened_kernel<D, TP, false, false, false, false, true, BatchShared>, bp, tb, rb, bi, st);
}
template <int D, class TP>
int do_fast_shared(const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    return launch_shared<TP>("fast batch shared", fast_kernel<D, TP, false, false, false, true, BatchShared>, bp, tb, rb, bi, st);
}

// the picks of gsss_batch.h's launchers, shape for shape
template <int D>
int shared_lane_vmf(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamScreened) {
        switch (p.kc) {
        case 3: return do_screened_shared<D, ScreenVmf<D, 3>>(bp, tb, rb, bi, st);
        case 4: return do_screened_shared<D, ScreenVmf<D, 4>>(bp, tb, rb, bi, st);
        case 6: return do_screened_shared<D, ScreenVmf<D, 6>>(bp, tb, rb, bi, st);
        case 10: return do_screened_shared<D, ScreenVmf<D, 10>>(bp, tb, rb, bi, st);
        case 16: return do_screened_shared<D, ScreenVmf<D, 16>>(bp, tb, rb, bi, st);
        }
    } else if (p.family == kFamFast) {
        if (p.kc == 4) return do_fast_shared<D, FastVmf<D, 4>>(bp, tb, rb, bi, st);
        if (p.kc == 16) return do_fast_shared<D, FastVmf<D, 16>>(bp, tb, rb, bi, st);
    }
    return pick_error(p);
}
template <int D>
int shared_lane_vmf_wide(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamScreened) {
        if (p.kc == 3) return do_screened_shared<D, ScreenVmf<D, 3>>(bp, tb, rb, bi, st);
        if (p.kc == 6) return do_screened_shared<D, ScreenVmf<D, 6>>(bp, tb, rb, bi, st);
        if (p.kc == 10) return do_screened_shared<D, ScreenVmf<D, 10>>(bp, tb, rb, bi, st);
    } else if (p.family == kFamFast) {
        if (p.kc == 4) return do_fast_shared<D, FastVmf<D, 4>>(bp, tb, rb, bi, st);
        if (p.kc == 10) return do_fast_shared<D, FastVmf<D, 10>>(bp, tb, rb, bi, st);
    }
    return pick_error(p);
}
template <int D>
int shared_lane_bingham(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    if (p.family == kFamFast) return do_fast_shared<D, FastBingham<D>>(bp, tb, rb, bi, st);
    if (p.family != kFamScreened) return pick_error(p);
    if (p.flavour == kFlavBinghamDiag) return do_screened_shared<D, ScreenBinghamDiag<D>>(bp, tb, rb, bi, st);
    return do_screened_shared<D, ScreenBingham<D>>(bp, tb, rb, bi, st);
}

#define GSSS_SHARED_ARGS const FastPick &, const BatchPlan &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t
#define GSSS_DECLARE(D) \
    extern template int shared_lane_vmf<D>(GSSS_SHARED_ARGS); \
    extern template int shared_lane_bingham<D>(GSSS_SHARED_ARGS);
GSSS_BATCH_LANE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE
#define GSSS_DECLARE(D) \
    extern template int shared_lane_vmf_wide<D>(GSSS_SHARED_ARGS); \
    extern template int shared_lane_bingham<D>(GSSS_SHARED_ARGS);
GSSS_BATCH_WIDE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE

int launch_shared_fast_vmf(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);
int launch_shared_fast_bingham(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st);

}  // namespace gsss
