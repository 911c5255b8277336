// GSSS_MODE_FAST launcher and instantiations for curve-vMF targets (10 knots, the reference's brownian_curve default; which
// kernel runs: gsss_fast_select.h).
#include "gsss_screen.h"
#include "gsss_spec64.h"

namespace gsss {

// d = 3, 6, ..., 24 is the reference's own sweep (sh/submit_job_curve_varying_ndim.sh:11); d = 10 its default
#define GSSS_FAST_CURVE_DIMS(X) X(3) X(6) X(9) X(10) X(12) X(15) X(18) X(21) X(24)

// lane-per-chain kernels, built for 10 knots (FastCurve pads).  (The screened one is picked at d = 3 only -- from d = 4 a
// screened launch runs the group kernel -- and stays built for every listed dimension.)
template <int D>
static int lane_curve(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.kc != 10) return pick_error(p);
    if (p.family == kFamScreened) return do_screened<D, ScreenCurve<D, 10>, false>(p, tb, rb, replay, st);
    return do_fast<D, FastCurve<D, 10>>(p, tb, rb, replay, st);
}

int launch_fast_curve(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    switch (p.family) {
    case kFamCurveSpec: return launch_curvespec(p, tb, rb, replay, st);
    case kFamCurve64:
        if (p.nv == 12) return do_curve64<12>(tb, rb, replay, st);
        if (p.nv == 20) return do_curve64<20>(tb, rb, replay, st);
        break;
    case kFamCoopFast:
        if (p.l == 16 && p.s == 4 && p.kc == 10) return do_coopfast<CoopVec<16, 4>, CoopCurve<CoopVec<16, 4>, 10>>(tb, rb, replay, st);
        if (p.l == 16 && p.s == 4 && p.kc == 16) return do_coopfast<CoopVec<16, 4>, CoopCurve<CoopVec<16, 4>, 16>>(tb, rb, replay, st);
        if (p.l == 64 && p.s == 8 && p.kc == 10) return do_coopfast<CoopVec<64, 8>, CoopCurve<CoopVec<64, 8>, 10>>(tb, rb, replay, st);
        break;
    default:
        switch (p.d) {
#define GSSS_CASE(D) \
    case D: return lane_curve<D>(p, tb, rb, replay, st);
            GSSS_FAST_CURVE_DIMS(GSSS_CASE)
#undef GSSS_CASE
        }
    }
    return pick_error(p);
}

}  // namespace gsss
