// Builds of exchange_eval_kernel (gsss_exchange.h): vMF mixtures and Bingham targets in every vector layout; the swap kernel,
// which no layout enters; and the launcher of a sweep.  Nothing else instantiates them.
#include "gsss_exchange.h"
#include "gsss_batch.h"

namespace gsss {
namespace {

using Counter = unsigned long long;

// One lane per pair of chains: pair e = (pair of members e / m, chain e % m).  A workgroup's 256 consecutive pairs span at most
// 256 pairs of members (m = 1): their attempts and acceptances are summed in LDS -- a wavefront that lies within one pair of
// members adds its two ballots' counts, any other lane by lane -- and added to counts[] once per workgroup and member.
// An attempt is a pair of chains of two participating members, whether or not the rule lets it swap.
__global__ void __launch_bounds__(kBlock) exchange_swap_kernel(int d, const ExchangeBlock a)
{
    __shared__ Counter cnt[2 * kBlock];
    cnt[threadIdx.x] = 0;
    cnt[kBlock + threadIdx.x] = 0;
    __syncthreads();
    const int64_t total = a.n_pairs * a.m;
    const int64_t e0 = (int64_t)blockIdx.x * kBlock, e_raw = e0 + threadIdx.x;
    const bool valid = e_raw < total;
    const int64_t e = valid ? e_raw : total - 1;  // surplus lanes shadow the last pair and store nothing
    const int64_t pi0 = e0 / a.m, pi = e / a.m, i = e - pi * a.m;
    const int64_t g = pi / a.K, k = pi - g * a.K;
    const int64_t ta = g * a.R + 2 * k + a.parity;
    const int64_t ca = ta * a.m + i, cb = ca + a.m;
    const double la_a = a.lp[2 * ca], la_b = a.lp[2 * ca + 1], lb_b = a.lp[2 * cb], lb_a = a.lp[2 * cb + 1];
    const double log_alpha = (la_b - la_a) + (lb_a - lb_b);
    const bool finite = isfinite(la_a) && isfinite(la_b) && isfinite(lb_a) && isfinite(lb_b);
    const bool may = finite && a.err[ca] == 0 && a.err[cb] == 0;
    // the stream's counter (gsss_device.h): (block, step_lo, chain_lo, chain_hi16 | step_hi16 << 16), key = seed
    const uint64_t chain = a.chain_offset + (uint64_t)ca;
    uint32_t w[4];
    philox4x32_10(kExchangeBlock, (uint32_t)a.step, (uint32_t)chain,
                  (uint32_t)((chain >> 32) & 0xFFFFu) | ((uint32_t)((a.step >> 32) & 0xFFFFu) << 16), (uint32_t)a.seed,
                  (uint32_t)(a.seed >> 32), w);
    const double u = u53(w[0], w[1]);
    const bool swap = valid && may && log(u) < log_alpha;  // (u = 0: -inf < log alpha, a swap)
    if (swap) {
        double *__restrict__ pa = a.state + ca;
        double *__restrict__ pb = a.state + cb;
        for (int j = 0; j < d; ++j) {
            const int64_t o = (int64_t)j * a.n;
            const double va = pa[o], vb = pb[o];
            pa[o] = vb;
            pb[o] = va;
        }
        if (a.replica) {
            const int64_t ra = a.replica[ca], rb = a.replica[cb];
            a.replica[ca] = rb;
            a.replica[cb] = ra;
        }
    }
    if (valid && a.log_alpha) a.log_alpha[ca] = log_alpha;
    if (a.counts == nullptr) return;  // (uniform)
    const int rel = (int)(pi - pi0);
    const int rel0 = __builtin_amdgcn_readfirstlane(rel);
    const Counter tried = __ballot(valid), taken = __ballot(swap);
    if (__all(rel == rel0)) {
        if (threadIdx.x % 64 == 0) {
            atomicAdd(cnt + rel0, (Counter)__popcll(tried));
            atomicAdd(cnt + kBlock + rel0, (Counter)__popcll(taken));
        }
    } else {
        if (valid) atomicAdd(cnt + rel, (Counter)1);
        if (swap) atomicAdd(cnt + kBlock + rel, (Counter)1);
    }
    __syncthreads();
    const int64_t mine = pi0 + threadIdx.x;
    if (mine < a.n_pairs && cnt[threadIdx.x] != 0) {
        const int64_t mg = mine / a.K, mk = mine - mg * a.K;
        const int64_t t = mg * a.R + 2 * mk + a.parity, n_targets = a.n / a.m;
        atomicAdd(a.counts + t, cnt[threadIdx.x]);
        if (cnt[kBlock + threadIdx.x] != 0) atomicAdd(a.counts + n_targets + t, cnt[kBlock + threadIdx.x]);
    }
}

template <class V, template <class> class TT>
int do_exchange_eval(const TargetBlock &tb, ExchangeBlock a, hipStream_t st)
{
    const int64_t chunks = 2 * ceil_div(a.m, kBlock / V::L);
    // (2 n_pairs is an int32's -- the batch's target count is --: the product cannot overflow once chunks fits one)
    const int64_t grid = chunks > 0x7FFFFFFFll ? chunks : 2 * a.n_pairs * chunks;
    if (int rc = batch_grid_fits(grid)) return rc;
    a.chunks = (int32_t)chunks;
    return launch_exact<V, TT, 0>("exchange eval", exchange_eval_kernel<V, TT>, grid, st, tb, exchange_eval_args(a));
}

}  // namespace

int launch_batch_exchange(int vec_id, const TargetBlock &tb, ExchangeBlock a, hipStream_t st)
{
    if (tb.kind != GSSS_VMF_MIXTURE && tb.kind != GSSS_BINGHAM) {
        set_error("a target batch holds vMF mixtures or Bingham targets (kind %d)", tb.kind);
        return GSSS_E_UNSUPPORTED;
    }
    a.K = (a.R - a.parity) / 2;
    a.n_pairs = (a.n / a.m / a.R) * a.K;
    if (a.n_pairs == 0) return GSSS_OK;  // (R = 2, parity 1: every member sits out)
    const int64_t swap_grid = ceil_div(a.n_pairs * a.m, kBlock);
    if (int rc = batch_grid_fits(swap_grid)) return rc;
    const bool vmf = tb.kind == GSSS_VMF_MIXTURE;
    const int rc = with_layout(vec_id, [&](auto v) {
        using V = decltype(v);
        return vmf ? do_exchange_eval<V, VmfMixture>(tb, a, st) : do_exchange_eval<V, Bingham>(tb, a, st);
    });
    if (rc != GSSS_OK) return rc;
    return launch_kernel("exchange swap", exchange_swap_kernel, swap_grid, 0, st, nullptr, tb.d, a);
}

}  // namespace gsss
