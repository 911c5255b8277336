// gsss_batch_logprob.h -- log_prob / gradient of every member of a target batch in one launch (gsss_batch_logprob,
// gsss_batch_gradient, gsss_batch_logprob_draws; include/gsss.h): the batch counterpart of logprob_kernel (gsss_device.h).
// The kernel and its argument block are here, the instantiations and their launcher in gsss_batch_logprob.hip only.
//
// A workgroup serves ONE target: workgroup b takes chunk b % chunks of the points of target b / chunks and stages
// blob + (b / chunks) stride, as run_kernel<.., BATCH> does -- before stage(), so both parameter paths follow: rows copied to
// LDS, and rows left in global memory (in_lds false), whose pointers stage() takes from the moved tb.blob.  The target policies
// (VmfMixture<V>, Bingham<V>), the layout V (select_vec_for) and the order of every product are logprob_kernel's, so a value is
// the member's own gsss_logprob / gsss_gradient value bit for bit.
//
// Points are addressed through strides, so that one kernel reads both layouts the project produces.  Point p of target t is
// (row p / pm, chain p % pm) and sits at  t st + row sr + chain sc,  its component j a further j sj doubles on; its value goes
// to  t ot + row orow + chain oc,  its gradient where the point is.
//   row-major [M][n][d]                 pm = 1:  st = n d, sr = d, sj = 1;        ot = n, orow = 1
//   component-major [R][d][N], m chains pm = m:  st = m, sr = d N, sc = 1, sj = N; ot = m, orow = N, oc = 1   (n = R m)
// All of it in 64-bit arithmetic: M n d exceeds 2^31 at the shapes a batch is made for.
//
// Few points per target use few lanes (16 points: 16 of 256 lanes at L = 1): targets are not packed into workgroups here.
#pragma once
#include "gsss_device.h"

namespace gsss {

struct BatchPoints {
    const double *x;
    double *out;
    int64_t stride;  // doubles from one member's blob to the next
    int64_t n;       // points per target (>= 1)
    int32_t chunks;  // workgroups per target: ceil(n / (kBlock / V::L))
    int32_t pad;
    int64_t pm;      // chains per target of a component-major block, 1 for rows
    int64_t st, sr, sc, sj;
    int64_t ot, orow, oc;
};

// x [M][n][d] -> out [M][n] (gradient: [M][n][d])
inline BatchPoints batch_points_rows(const double *x, double *out, int64_t n, int d, int64_t stride)
{
    BatchPoints a{};
    a.x = x;
    a.out = out;
    a.stride = stride;
    a.n = n;
    a.pm = 1;
    a.st = n * d;
    a.sr = d;
    a.sj = 1;
    a.ot = n;
    a.orow = 1;
    return a;
}

// x [n_rows][d][n_chains], m chains per target -> out [n_rows][n_chains]
inline BatchPoints batch_points_draws(const double *x, double *out, int64_t n_rows, int64_t n_chains, int64_t m, int d, int64_t stride)
{
    BatchPoints a{};
    a.x = x;
    a.out = out;
    a.stride = stride;
    a.n = n_rows * m;
    a.pm = m;
    a.st = m;
    a.sr = (int64_t)d * n_chains;
    a.sc = 1;
    a.sj = n_chains;
    a.ot = m;
    a.orow = n_chains;
    a.oc = 1;
    return a;
}

template <class V, template <class> class TT, bool GRAD>
__global__ void __launch_bounds__(kBlock) batch_logprob_kernel(TargetBlock tb, const BatchPoints a)
{
    using T = TT<V>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t bt = (int64_t)(blockIdx.x / (uint32_t)a.chunks), bl = (int64_t)blockIdx.x - bt * a.chunks;
    tb.blob += bt * a.stride;
    T tgt;
    tgt.stage(lds, tb);
    double *scratch = lds + T::lds_doubles(tb.k, tb.d) + (size_t)T::kScratchPerChain * (threadIdx.x / V::L);
    __syncthreads();
    const int d = tb.d;
    const int g = threadIdx.x % V::L;
    const int64_t p_raw = bl * (kBlock / V::L) + threadIdx.x / V::L;
    const bool active = p_raw < a.n;
    const int64_t p = active ? p_raw : a.n - 1;  // surplus lanes shadow the target's last point and store nothing
    int64_t row = p, chain = 0;
    if (a.pm != 1) {
        row = p / a.pm;
        chain = p - row * a.pm;
    }
    const double *__restrict__ xp = a.x + (bt * a.st + row * a.sr + chain * a.sc);
    double x[V::N];
#pragma unroll
    for (int i = 0; i < V::N; ++i) {
        const int cc = V::comp(g, i);
        x[i] = (cc < d) ? xp[(int64_t)cc * a.sj] : 0.0;
    }
    if constexpr (GRAD) {
        double gr[V::N];
        tgt.grad(x, g, scratch, gr);
        double *__restrict__ op = a.out + (bt * a.st + row * a.sr + chain * a.sc);
#pragma unroll
        for (int i = 0; i < V::N; ++i) {
            const int cc = V::comp(g, i);
            if (active && cc < d) op[(int64_t)cc * a.sj] = gr[i];
        }
    } else {
        const double lp = tgt.logp(x, g, scratch);
        if (active && g == 0) a.out[bt * a.ot + row * a.orow + chain * a.oc] = lp;
    }
}

// The launch in layout vec_id (a GSSS_VEC_LIST id: select_vec_for's) for tb.kind GSSS_VMF_MIXTURE or GSSS_BINGHAM; tb.blob is
// the first of the n_targets members served.  a.chunks is filled in here.  GSSS_E_UNSUPPORTED: more workgroups than a grid holds.
int launch_batch_logprob(int vec_id, const TargetBlock &tb, BatchPoints a, int64_t n_targets, bool grad, hipStream_t st);

}  // namespace gsss
