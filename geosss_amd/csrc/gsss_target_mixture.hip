// Kernel instantiations for GSSS_MIXTURE targets (Mixture, gsss_device.h): every vector layout x {Philox, replay, numpy}
// draws.  The components' rows sit behind the draw source's LDS (Mixture::launch_doubles), so the launchers size the
// dynamic LDS themselves instead of do_run / do_logprob.
#include "gsss_launch.h"

namespace gsss {

template <class V, template <class> class DR>
int do_run_mixture(const TargetBlock &tb, const RunBlock &rb, hipStream_t st)
{
    static_assert(DR<V>::kLdsDoubles <= kMixDrawsReserve, "the draw source's tables must fit the reserve");
    const size_t lds = Mixture<V>::launch_doubles(tb) * sizeof(double);
    if (lds > kMaxLdsBytes) {
        set_error("mixture parameters need %zu B of LDS (> %zu)", lds, kMaxLdsBytes);
        return GSSS_E_UNSUPPORTED;
    }
    auto kern = run_kernel<V, Mixture, DR, false>;
    if (rb.stats != nullptr) kern = run_kernel<V, Mixture, DR, true>;
    if (int rc = allow_lds("run", kern, lds)) return rc;
    const int64_t per_block = (V::L == 1 && rb.spread) ? kBlock / 64 : kBlock / V::L;
    return launch_kernel("run", kern, ceil_div(rb.n_chains, per_block), lds, st, nullptr, tb, rb);
}

template <class V>
int do_logprob_mixture(const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st)
{
    const size_t lds = Mixture<V>::launch_doubles(tb) * sizeof(double);
    if (lds > kMaxLdsBytes) {
        set_error("mixture parameters need %zu B of LDS (> %zu)", lds, kMaxLdsBytes);
        return GSSS_E_UNSUPPORTED;
    }
    auto kern = grad ? logprob_kernel<V, Mixture, true> : logprob_kernel<V, Mixture, false>;
    if (int rc = allow_lds("logprob", kern, lds)) return rc;
    return launch_kernel("logprob", kern, ceil_div(n, kBlock / V::L), lds, st, nullptr, tb, x, n, out);
}

#define GSSS_RUN_CASE_Mixture(ID, V, NAME) \
    case ID:                         \
        return draws == kDrawsReplay ? do_run_mixture<V, ReplayDraws>(tb, rb, st) \
               : draws == kDrawsNumpy ? do_run_mixture<V, NumpyDraws>(tb, rb, st) \
                                      : do_run_mixture<V, PhiloxDraws>(tb, rb, st);
#define GSSS_LOGPROB_CASE_Mixture(ID, V, NAME) \
    case ID:                             \
        return do_logprob_mixture<V>(tb, x, n, out, grad, st);
GSSS_DEFINE_TARGET_LAUNCHERS(Mixture)
}  // namespace gsss
