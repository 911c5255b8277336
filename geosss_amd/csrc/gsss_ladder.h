// gsss_ladder.h -- log normalising constants along ladders of members of a target batch (gsss_batch_ladder, include/gsss.h): the
// sums from which the ratios Z_a / Z_b of neighbouring rungs follow, folded over a block of retained rows without storing a
// value beyond the block.  The kernels and their argument block are here, the instantiations and the launcher in
// gsss_ladder.hip only.
//
// The rule.  The n / m targets of the call form ladders of R consecutive members, rung r colder than rung r + 1.  Pair
// (a, b = a + 1) exists for every a that is not the last rung of its ladder: R - 1 pairs a ladder.  With l_t the log-density of
// member t (gsss_batch_logprob's value, bit for bit) and x_{t,i,r} chain i of member t at row r of the block
// [n_rows][d][n] (component-major, as gsss_batch_logprob_draws takes it), every row gives pair-chain (a, i) two differences
//     u = l_a(x_b) - l_b(x_b)     a draw of the HOTTER member:  E_b[exp u] = Z_a / Z_b
//     v = l_b(x_a) - l_a(x_a)     a draw of the COLDER member:  E_a[exp v] = Z_b / Z_a
// The row is USED iff all four log-densities are finite (the swap's rule, gsss_exchange.h, without err), else SKIPPED.
//
// acc[pair][i][10], pair = ladder (R - 1) + rung of a, continued from call to call:
//     0      draws used
//     1, 2   M_u = the running maximum of u, S_u = sum exp(u - M_u)
//     3, 4   sum u, sum u^2
//     5, 6   M_v, S_v
//     7, 8   sum v, sum v^2
//     9      draws skipped
// The recurrence of (M, S), for u and for v alike, per used draw and in row order:
//     M' = max(M, u);  S' = S exp(M - M') + exp(u - M')
// from M = -inf, S = 0; the FIRST used draw (slot 0 is zero) sets M = u, S = 1 directly, so that no -inf - (-inf) is formed.
// log sum exp(u) = M_u + log S_u.  A pair-chain's ten doubles depend on its own rows in their order alone: a block of 5 rows
// gives the bits of the same rows in calls of 3 and 2.  No atomics: the order of every sum is fixed by the arguments.
//
// Two launches, because l_a(x_b) and l_b(x_b) come from different members' workgroups (a workgroup stages ONE member's rows,
// which may take about 136 KB of the 160 KB; rows_fit_lds):
//   ladder_eval_kernel<V, TT>  batch_logprob_kernel's / exchange_eval_kernel's evaluation (the same policies, layout V and order
//       of products, so a value is TargetBatch.log_prob's bit for bit) with two differences.  Three column sets: a workgroup
//       belongs to (member t, which w in {0 own, 1 the lower neighbour t - 1, 2 the upper neighbour t + 1}, chunk of chains) and
//       writes l_t at those columns to lp3[row][t m + i][w]; a workgroup whose neighbour does not exist (first or last rung)
//       returns, whole and uniformly, before stage() and before any barrier, and its slots are never written and never read.
//       Stage once, loop over rows: member t's rows are staged once for the n_rows rows of the block, where
//       exchange_eval_kernel launches and stages per row.
//   ladder_fold_kernel         independent of the layout, one lane per (pair, chain i), coalesced over i: walks the block's
//       rows in order and updates the pair-chain's ten doubles.
// All index arithmetic is 64-bit.  Few chains per target use few lanes of the eval kernel, as in exchange_eval_kernel: members
// are not packed into workgroups here -- the same open lever.
#pragma once
#include "gsss_device.h"

namespace gsss {

constexpr int kLadderSlots = 10;

struct LadderBlock {
    const double *x;   // [n_rows][d][n], component-major
    double *lp3;       // [n_rows][n][3]: l_t at its own, its lower neighbour's and its upper neighbour's columns
    double *acc;       // [n_pairs][m][10]
    int64_t stride;    // doubles from one member's blob to the next
    int64_t n_rows, n, m;
    int64_t n_pairs;   // (n / m / R) (R - 1)
    int32_t R;
    int32_t chunks;    // eval: workgroups per (member, column set), ceil(m / (kBlock / V::L))
};

template <class V, template <class> class TT>
__global__ void __launch_bounds__(kBlock) ladder_eval_kernel(TargetBlock tb, const LadderBlock a)
{
    using T = TT<V>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const uint32_t q = blockIdx.x / (uint32_t)a.chunks;  // (member, column set)
    const int64_t bl = (int64_t)(blockIdx.x - q * (uint32_t)a.chunks);
    const uint32_t ut = q / 3u, w = q - 3u * ut;
    const uint32_t rung = ut % (uint32_t)a.R;
    if ((w == 1u && rung == 0u) || (w == 2u && rung + 1u == (uint32_t)a.R)) return;  // no such neighbour (uniform)
    const int64_t bt = (int64_t)ut;
    const int64_t src = w == 0u ? bt : (w == 1u ? bt - 1 : bt + 1);
    tb.blob += bt * a.stride;
    T tgt;
    tgt.stage(lds, tb);
    double *scratch = lds + T::lds_doubles(tb.k, tb.d) + (size_t)T::kScratchPerChain * (threadIdx.x / V::L);
    __syncthreads();
    const int d = tb.d;
    const int g = threadIdx.x % V::L;
    const int64_t i_raw = bl * (kBlock / V::L) + threadIdx.x / V::L;
    const bool active = i_raw < a.m;
    const int64_t i = active ? i_raw : a.m - 1;  // surplus lanes shadow the member's last chain and store nothing
    // a lane's first component, then offsets that are the same for every lane: comp(g, s) = comp(g, 0) + comp(0, s)
    const double *__restrict__ xp = a.x + ((src * a.m + i) + (int64_t)V::comp(g, 0) * a.n);
    double *__restrict__ op = a.lp3 + (3 * (bt * a.m + i) + (int64_t)w);
    const int64_t row_x = (int64_t)d * a.n, row_lp = 3 * a.n;
#pragma unroll 1
    for (int64_t r = 0; r < a.n_rows; ++r) {
        double x[V::N];
#pragma unroll
        for (int s = 0; s < V::N; ++s) {
            const int cc = V::comp(g, s);
            x[s] = (cc < d) ? xp[(int64_t)V::comp(0, s) * a.n] : 0.0;
        }
        const double lp = tgt.logp(x, g, scratch);
        if (active && g == 0) *op = lp;
        xp += row_x;
        op += row_lp;
    }
}

// vec_id: a GSSS_VEC_LIST id (select_vec_for's); tb.blob: the first member of the call.  a.chunks and a.n_pairs are filled in
// here.  GSSS_E_UNSUPPORTED: more workgroups than a grid holds.
int launch_batch_ladder(int vec_id, const TargetBlock &tb, LadderBlock a, hipStream_t st);

}  // namespace gsss
