// RWMH / spherical HMC kernels for GSSS_MIXTURE targets (gsss_mh.h), every vector layout and draw source.  As in
// gsss_target_mixture.hip the launch sizes its LDS with Mixture::launch_doubles (the components' rows behind the draws').
#include "gsss_launch.h"
#include "gsss_mh.h"

namespace gsss {

template <class V, template <class> class DR, int SAMPLER>
int do_mh_mixture(const TargetBlock &tb, const RunBlock &rb, const MhBlock &mb, hipStream_t st)
{
    static_assert(DR<V>::kLdsDoubles <= kMixDrawsReserve, "the draw source's tables must fit the reserve");
    const size_t lds = Mixture<V>::launch_doubles(tb) * sizeof(double);
    if (lds > kMaxLdsBytes) {
        set_error("mixture parameters need %zu B of LDS", lds);
        return GSSS_E_UNSUPPORTED;
    }
    auto kern = mh_kernel<V, Mixture, DR, SAMPLER>;
    if (int rc = allow_lds("MH", kern, lds)) return rc;
    return launch_kernel("MH", kern, ceil_div(rb.n_chains, kBlock / V::L), lds, st, nullptr, tb, rb, mb);
}

// one layout: every draw source x both kernels (mh_dispatch with the mixture's LDS sizing)
template <class V>
int mh_dispatch_mixture(int draws, int sampler, const TargetBlock &tb, const RunBlock &rb, const MhBlock &mb, hipStream_t st)
{
    if (sampler == GSSS_RWMH || sampler == GSSS_INDEP || sampler == GSSS_MIX) {
        if (draws == kDrawsReplay) return do_mh_mixture<V, ReplayDraws, GSSS_RWMH>(tb, rb, mb, st);
        if (draws == kDrawsNumpy) return do_mh_mixture<V, NumpyDraws, GSSS_RWMH>(tb, rb, mb, st);
        return do_mh_mixture<V, PhiloxDraws, GSSS_RWMH>(tb, rb, mb, st);
    }
    if (draws == kDrawsReplay) return do_mh_mixture<V, ReplayDraws, GSSS_HMC>(tb, rb, mb, st);
    if (draws == kDrawsNumpy) return do_mh_mixture<V, NumpyDraws, GSSS_HMC>(tb, rb, mb, st);
    return do_mh_mixture<V, PhiloxDraws, GSSS_HMC>(tb, rb, mb, st);
}

#define GSSS_MH_CASE_Mixture(ID, V, NAME) \
    case ID:                        \
        return mh_dispatch_mixture<V>(draws, sampler, tb, rb, mb, st);
GSSS_DEFINE_MH_LAUNCHER(Mixture)
}  // namespace gsss
