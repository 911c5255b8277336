// Lane-per-chain fast kernels for von Mises-Fisher mixtures, any K <= 16 components at d = 3 .. 10, K <= 10 at d = 11 .. 16.
//
// Kernels are built per dimension and per component-count BUCKET KC (gsss_fast_select.h picks it; FastVmf::stage pads the
// surplus components).  Screened kernels (gsss_screen.h): buckets 3, 4, 6, 10, 16; the all-double fallback and the
// one-wavefront-per-chain kernels (gsss_fast.h): buckets 4 and 16.  One translation unit per dimension (compile time).
#pragma once
#include "gsss_screen.h"

namespace gsss {

template <int D>
int lane_vmf(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.family == kFamScreened) {
        switch (p.kc) {
        case 3: return do_screened<D, ScreenVmf<D, 3>>(p, tb, rb, replay, st);
        case 4: return do_screened<D, ScreenVmf<D, 4>>(p, tb, rb, replay, st);
        case 6: return do_screened<D, ScreenVmf<D, 6>>(p, tb, rb, replay, st);
        case 10: return do_screened<D, ScreenVmf<D, 10>>(p, tb, rb, replay, st);
        case 16: return do_screened<D, ScreenVmf<D, 16>, false>(p, tb, rb, replay, st);
        }
        return pick_error(p);
    }
    if (p.kc == 4) return do_fast<D, FastVmf<D, 4>>(p, tb, rb, replay, st);
    if (p.kc == 16) return do_fast<D, FastVmf<D, 16>>(p, tb, rb, replay, st);
    return pick_error(p);
}

// d = 11 .. 16 (round 4): the screened lane kernel alone, one chain per lane (screen_parks is false there), library stream
template <int D>
int lane_vmf_wide(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, hipStream_t st)
{
    if (p.family != kFamScreened) return pick_error(p);
    switch (p.kc) {
    case 3: return do_screened_run<D, ScreenVmf<D, 3>, false>(tb, rb, st);
    case 6: return do_screened_run<D, ScreenVmf<D, 6>, false>(tb, rb, st);
    case 10: return do_screened_run<D, ScreenVmf<D, 10>, false>(tb, rb, st);
    }
    return pick_error(p);
}
#define GSSS_VMF_WIDE_DIMS(X) X(11) X(12) X(13) X(14) X(15) X(16)
#define GSSS_DECLARE_WIDE(D) extern template int lane_vmf_wide<D>(const FastPick &, const TargetBlock &, const RunBlock &, hipStream_t);
GSSS_VMF_WIDE_DIMS(GSSS_DECLARE_WIDE)
#undef GSSS_DECLARE_WIDE

#define GSSS_VMF_LANE_DIMS(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
#define GSSS_DECLARE(D) extern template int lane_vmf<D>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
GSSS_VMF_LANE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE

}  // namespace gsss
