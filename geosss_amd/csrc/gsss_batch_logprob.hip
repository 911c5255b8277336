// Builds of batch_logprob_kernel (gsss_batch_logprob.h): vMF mixtures and Bingham targets in every vector layout, value and
// gradient, and their launcher.  Nothing else instantiates them.
#include "gsss_batch_logprob.h"
#include "gsss_batch.h"

namespace gsss {
namespace {

template <class V, template <class> class TT>
int do_batch_logprob(const TargetBlock &tb, BatchPoints a, int64_t n_targets, bool grad, hipStream_t st)
{
    const int64_t chunks = ceil_div(a.n, kBlock / V::L);
    // (n_targets is an int32's: the product cannot overflow once chunks fits one)
    const int64_t grid = chunks > 0x7FFFFFFFll ? chunks : n_targets * chunks;
    if (int rc = batch_grid_fits(grid)) return rc;
    a.chunks = (int32_t)chunks;
    auto kern = grad ? batch_logprob_kernel<V, TT, true> : batch_logprob_kernel<V, TT, false>;
    return launch_exact<V, TT, 0>("batch logprob", kern, grid, st, tb, a);
}

}  // namespace

int launch_batch_logprob(int vec_id, const TargetBlock &tb, BatchPoints a, int64_t n_targets, bool grad, hipStream_t st)
{
    if (tb.kind != GSSS_VMF_MIXTURE && tb.kind != GSSS_BINGHAM) {
        set_error("a target batch holds vMF mixtures or Bingham targets (kind %d)", tb.kind);
        return GSSS_E_UNSUPPORTED;
    }
    const bool vmf = tb.kind == GSSS_VMF_MIXTURE;
    return with_layout(vec_id, [&](auto v) {
        using V = decltype(v);
        return vmf ? do_batch_logprob<V, VmfMixture>(tb, a, n_targets, grad, st) : do_batch_logprob<V, Bingham>(tb, a, n_targets, grad, st);
    });
}

}  // namespace gsss
