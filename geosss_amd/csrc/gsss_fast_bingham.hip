// GSSS_MODE_FAST launcher and instantiations for Bingham targets (which kernel runs: gsss_fast_select.h).
#include "gsss_fast_bingham_lane.h"

namespace gsss {

// the plain integers gsss_fast_select.h decides the wide cooperative layout's fit with are this layout's
namespace fsd = fast_select_detail;
using WideBingham = CoopBingham<CoopVec<fsd::kWideBinghamL, fsd::kWideBinghamS>>;
static_assert(fsd::kBlockThreads == kBlock && (size_t)fsd::kLdsBytes == kMaxLdsBytes &&
                  fsd::kWideBinghamScratchPerGroup == WideBingham::kScratchPerGroup &&
                  (size_t)fsd::wide_bingham_param_doubles(100) == coop_param_doubles<WideBingham>(100),
              "gsss_fast_select.h restates coop_param_doubles<CoopBingham<CoopVec<16, 8>>> and the LDS of a workgroup");

#define GSSS_FAST_BINGHAM_DIMS(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)

template <int D>
static int lane_bingham(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.family != kFamScreened) return do_fast<D, FastBingham<D>>(p, tb, rb, replay, st);
    if (p.flavour == kFlavBinghamDiag) return do_screened<D, ScreenBinghamDiag<D>>(p, tb, rb, replay, st);
    return do_screened<D, ScreenBingham<D>>(p, tb, rb, replay, st);
}

int launch_fast_bingham(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.family == kFamCoopFast) {
#define GSSS_COOP(L, S) \
    if (p.l == L && p.s == S) return do_coopfast<CoopVec<L, S>, CoopBingham<CoopVec<L, S>>>(tb, rb, replay, st);
        GSSS_COOP(4, 4) GSSS_COOP(4, 8) GSSS_COOP(8, 8) GSSS_COOP(16, 4) GSSS_COOP(16, 8)
#undef GSSS_COOP
        return pick_error(p);
    }
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return lane_bingham<D>(p, tb, rb, replay, st);
        GSSS_FAST_BINGHAM_DIMS(GSSS_CASE)
#undef GSSS_CASE
#define GSSS_CASE(D) \
    case D: return lane_bingham_wide<D>(p, tb, rb, st);
        GSSS_BINGHAM_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
