// Screened lane kernels for Bingham / BinghamFisher targets at d = 11 .. 16, one chain per lane (round 4): the compact diagonal
// target of the paper's eigenbasis experiments and the general one (dense A, linear term).  Served: packed ensembles on the
// library stream with the screen on (or verified); everything else stays with the cooperative kernels (gsss_fast_select.h).
#pragma once
#include "gsss_screen.h"

namespace gsss {

template <int D>
int lane_bingham_wide(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, hipStream_t st)
{
    if (p.family != kFamScreened) return pick_error(p);
    if (p.flavour == kFlavBinghamDiag) return do_screened_run<D, ScreenBinghamDiag<D>, false>(tb, rb, st);
    return do_screened_run<D, ScreenBingham<D>, false>(tb, rb, st);
}
#define GSSS_BINGHAM_WIDE_DIMS(X) X(11) X(12) X(13) X(14) X(15) X(16)
#define GSSS_DECLARE_WIDE(D) extern template int lane_bingham_wide<D>(const FastPick &, const TargetBlock &, const RunBlock &, hipStream_t);
GSSS_BINGHAM_WIDE_DIMS(GSSS_DECLARE_WIDE)
#undef GSSS_DECLARE_WIDE

}  // namespace gsss
