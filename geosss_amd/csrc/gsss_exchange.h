// gsss_exchange.h -- replica exchange along ladders of members of a target batch (gsss_batch_exchange, include/gsss.h): one sweep
// of one parity over the chains of a launch, on the device.  The kernels and their argument block are here, the instantiations
// and the launcher in gsss_exchange.hip only.
//
// The rule.  The n / m targets of the call form ladders of R consecutive members.  A sweep of parity p pairs member
// a = g R + 2 k + p with b = a + 1 for every k with 2 k + p + 1 < R: K = (R - p) / 2 pairs a ladder, the other members sit out.
// Chain i of a (column c_a = a m + i of the component-major state [d][n]) is paired with chain i of b (c_b = c_a + m), and with
// l_t the log-density of member t, in double precision and in this order,
//     log alpha = (l_a(x_b) - l_a(x_a)) + (l_b(x_a) - l_b(x_b)).
// The two columns are swapped iff all four values are finite, both chains have err == 0 and log(u) < log alpha, u the first 53-bit
// uniform of Philox block kExchangeBlock at (seed, chain = chain_offset + c_a, step).  u = 0 swaps.
//
// Two launches, because two members' rows do not fit one workgroup (rows_fit_lds is a property of ONE member's rows, which may
// take about 136 KB of the 160 KB):
//   exchange_eval_kernel<V, TT>  batch_logprob_kernel's evaluation (the same policies, layout V and order of products, so a value
//       is TargetBatch.log_prob's bit for bit) for the participating members only.  A participant t has 2 m points, its own m
//       columns and its partner's: workgroup b serves chunk b % chunks of participant b / chunks -- the first half of the chunks
//       its own columns, the second half the partner's --, stages that member's blob and writes l_t(x_t) to lp[2 c] or
//       l_t(x_partner) to lp[2 c + 1], c = t m + i.  (One point per lane group, as in batch_logprob_kernel: both points in one
//       lane group cost up to twice its registers, and wavefronts per SIMD with them.)
//   exchange_swap_kernel         independent of the layout, one lane per pair of chains: log alpha, the draw, the swap of the d
//       components (coalesced over i), the replica ids, and the counts per lower member -- summed in LDS, then one 64-bit
//       atomic add per workgroup and member it spans.
// All index arithmetic is 64-bit.  Few chains per target use few lanes of the eval kernel (m = 16: 16 of 256 lanes at L = 1), as
// in batch_logprob_kernel: members are not packed into workgroups here -- an open lever.
#pragma once
#include "gsss_device.h"

namespace gsss {

// The Philox block of the exchange uniform.  The samplers draw block 0, ceil(d / 4) blocks of normals (twice that under RWMH) and
// one block per four tries -- at most 1 + 2 ceil(d / 4) + 2^29 (max_tries < 2^31): far below this one.  
constexpr uint32_t kExchangeBlock = 0xFFFFFFFFu;

struct ExchangeBlock {
    double *state;        // [d][n], component-major
    double *lp;           // [n][2]: l_t(x_t), l_t(x_partner); written for participating chains only
    const int32_t *err;   // [n]
    int64_t *replica;     // [n] or NULL
    unsigned long long *counts;  // [2][n / m]: attempts, accepts per lower member; or NULL
    double *log_alpha;    // [n], lower chains only; or NULL
    int64_t stride;       // doubles from one member's blob to the next
    int64_t n, m;         // chains of the call, chains per target
    int64_t n_pairs;      // pairs of members in the call: (n / m / R) K
    int32_t R, parity, K; // ladder length, parity, pairs per ladder
    int32_t chunks;       // eval: workgroups per participant, 2 ceil(m / (kBlock / V::L))
    uint64_t seed, chain_offset, step;
};

// what the evaluation reads of it
struct ExchangeEval {
    const double *x;   // the state
    double *lp;
    int64_t stride, n, m;
    int32_t R, parity, K, chunks;
};
inline ExchangeEval exchange_eval_args(const ExchangeBlock &a)
{
    return ExchangeEval{a.state, a.lp, a.stride, a.n, a.m, a.R, a.parity, a.K, a.chunks};
}

// participant q = 0 .. 2 n_pairs - 1 (an int32's, like the batch's target count) -> its target and its partner's, within the call
__device__ __forceinline__ void exchange_member(const ExchangeEval &a, uint32_t q, int64_t &t, int64_t &partner)
{
    const uint32_t per = 2u * (uint32_t)a.K, g = q / per, j = q - g * per;
    t = (int64_t)(g * (uint32_t)a.R + (uint32_t)a.parity + j);
    partner = (j & 1u) ? t - 1 : t + 1;
}

template <class V, template <class> class TT>
__global__ void __launch_bounds__(kBlock) exchange_eval_kernel(TargetBlock tb, const ExchangeEval a)
{
    using T = TT<V>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const uint32_t q = blockIdx.x / (uint32_t)a.chunks;
    const int64_t bl = (int64_t)(blockIdx.x - q * (uint32_t)a.chunks);
    int64_t bt, partner;
    exchange_member(a, q, bt, partner);
    tb.blob += bt * a.stride;
    T tgt;
    tgt.stage(lds, tb);
    double *scratch = lds + T::lds_doubles(tb.k, tb.d) + (size_t)T::kScratchPerChain * (threadIdx.x / V::L);
    __syncthreads();
    const int d = tb.d;
    const int g = threadIdx.x % V::L;
    // the first half of a participant's chunks takes its own m columns, the second half its partner's
    const uint32_t half = (uint32_t)a.chunks / 2u, w = (uint32_t)bl >= half ? 1u : 0u;
    const int64_t i_raw = (bl - (int64_t)(w * half)) * (kBlock / V::L) + threadIdx.x / V::L;
    const bool active = i_raw < a.m;
    const int64_t i = active ? i_raw : a.m - 1;  // surplus lanes shadow the member's last chain and store nothing
    const double *__restrict__ xp = a.x + ((w ? partner : bt) * a.m + i);
    double x[V::N];
#pragma unroll
    for (int s = 0; s < V::N; ++s) {
        const int cc = V::comp(g, s);
        x[s] = (cc < d) ? xp[(int64_t)cc * a.n] : 0.0;
    }
    const double lp = tgt.logp(x, g, scratch);
    if (active && g == 0) a.lp[2 * (bt * a.m + i) + w] = lp;
}

// vec_id: a GSSS_VEC_LIST id (select_vec_for's); tb.blob: the first member of the call.  a.chunks and a.K are filled in here.
// GSSS_E_UNSUPPORTED: more workgroups than a grid holds.
int launch_batch_exchange(int vec_id, const TargetBlock &tb, ExchangeBlock a, hipStream_t st);

}  // namespace gsss
