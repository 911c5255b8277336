// Builds of ladder_eval_kernel (gsss_ladder.h): vMF mixtures and Bingham targets in every vector layout; the fold kernel, which
// no layout enters; and the launcher of a block.  Nothing else instantiates them.
#include "gsss_ladder.h"
#include "gsss_batch.h"

namespace gsss {
namespace {

// One lane per pair of chains: pair-chain e = (pair of members e / m, chain e % m), consecutive lanes consecutive chains.  The
// lane reads its ten doubles, walks the rows of the block in order and writes them back: nothing of it is shared with another
// lane.  (M, S) by the recurrence of gsss_ladder.h.
__device__ __forceinline__ void ladder_lse_step(bool first, double u, double &M, double &S)
{
    if (first) {
        M = u;
        S = 1.0;
    } else {
        const double Mn = fmax(M, u);
        S = S * exp(M - Mn) + exp(u - Mn);
        M = Mn;
    }
}

__global__ void __launch_bounds__(kBlock) ladder_fold_kernel(const LadderBlock a)
{
    const int64_t total = a.n_pairs * a.m;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;  // (no barrier below)
    const int64_t pi = e / a.m, i = e - pi * a.m;
    const int64_t g = pi / (a.R - 1), k = pi - g * (a.R - 1);
    const int64_t ca = (g * a.R + k) * a.m + i, cb = ca + a.m;
    double *__restrict__ acc = a.acc + e * kLadderSlots;
    double used = acc[0], Mu = acc[1], Su = acc[2], su = acc[3], suu = acc[4];
    double Mv = acc[5], Sv = acc[6], sv = acc[7], svv = acc[8], skipped = acc[9];
    const double *__restrict__ pa = a.lp3 + 3 * ca;
    const double *__restrict__ pb = a.lp3 + 3 * cb;
    const int64_t row_lp = 3 * a.n;
    for (int64_t r = 0; r < a.n_rows; ++r) {
        // l_a at its own and at its upper neighbour's columns, l_b at its own and at its lower neighbour's
        const double la_a = pa[0], la_b = pa[2], lb_b = pb[0], lb_a = pb[1];
        pa += row_lp;
        pb += row_lp;
        if (!(isfinite(la_a) && isfinite(la_b) && isfinite(lb_a) && isfinite(lb_b))) {
            skipped += 1.0;
            continue;
        }
        const double u = la_b - lb_b, v = lb_a - la_a;
        const bool first = used == 0.0;
        ladder_lse_step(first, u, Mu, Su);
        ladder_lse_step(first, v, Mv, Sv);
        su += u;
        suu += u * u;
        sv += v;
        svv += v * v;
        used += 1.0;
    }
    acc[0] = used;
    acc[1] = Mu;
    acc[2] = Su;
    acc[3] = su;
    acc[4] = suu;
    acc[5] = Mv;
    acc[6] = Sv;
    acc[7] = sv;
    acc[8] = svv;
    acc[9] = skipped;
}

template <class V, template <class> class TT>
int do_ladder_eval(const TargetBlock &tb, LadderBlock a, hipStream_t st)
{
    const int64_t chunks = ceil_div(a.m, kBlock / V::L);
    // (n / m is an int32's -- the batch's target count is --: the product cannot overflow once chunks fits one, nor three times
    // it once the product does)
    const int64_t sets = chunks > 0x7FFFFFFFll ? chunks : (a.n / a.m) * chunks;
    const int64_t grid = sets > 0x7FFFFFFFll ? sets : 3 * sets;
    if (int rc = batch_grid_fits(grid)) return rc;
    a.chunks = (int32_t)chunks;
    return launch_exact<V, TT, 0>("ladder eval", ladder_eval_kernel<V, TT>, grid, st, tb, a);
}

}  // namespace

int launch_batch_ladder(int vec_id, const TargetBlock &tb, LadderBlock a, hipStream_t st)
{
    if (tb.kind != GSSS_VMF_MIXTURE && tb.kind != GSSS_BINGHAM) {
        set_error("a target batch holds vMF mixtures or Bingham targets (kind %d)", tb.kind);
        return GSSS_E_UNSUPPORTED;
    }
    a.n_pairs = (a.n / a.m / a.R) * (a.R - 1);
    const int64_t fold_grid = ceil_div(a.n_pairs * a.m, kBlock);
    if (int rc = batch_grid_fits(fold_grid)) return rc;
    const bool vmf = tb.kind == GSSS_VMF_MIXTURE;
    const int rc = with_layout(vec_id, [&](auto v) {
        using V = decltype(v);
        return vmf ? do_ladder_eval<V, VmfMixture>(tb, a, st) : do_ladder_eval<V, Bingham>(tb, a, st);
    });
    if (rc != GSSS_OK) return rc;
    return launch_kernel("ladder fold", ladder_fold_kernel, fold_grid, 0, st, nullptr, a);
}

}  // namespace gsss
