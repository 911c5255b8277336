// gsss_user_target.h -- user-defined targets (GSSS_USER): a policy whose log-density is C++ the user writes, compiled for one
// vector layout into a module of its own (gsss_user_module.hip, built by geosss_amd/usertarget.py) and loaded beside the library.
//
// The user's translation unit defines, in the global namespace,
//     __device__ double gsss_user_log_prob(const double *x, int d, const double *p);
//     __device__ void gsss_user_gradient(const double *x, int d, const double *p, double *g);   // optional (HMC, gradient)
// x: the d components of one point, p: the target's parameters (read-only), g: the d components of the ambient gradient.
// The policy calls them inside the exact kernels (run_kernel, logprob_kernel, mh_kernel), exactly where a built-in target's
// logp / grad would be evaluated.
#pragma once
#include "gsss_launch.h"
#include "gsss_mh.h"

#ifndef GSSS_USER_HAS_GRADIENT
#define GSSS_USER_HAS_GRADIENT 0
#endif

__device__ double gsss_user_log_prob(const double *x, int d, const double *p);
__device__ void gsss_user_gradient(const double *x, int d, const double *p, double *g);

namespace gsss {

constexpr bool kUserHasGradient = GSSS_USER_HAS_GRADIENT != 0;

// Parameters: one flat array of n_params doubles (TargetBlock::k), copied to LDS where it fits beside the groups' scratch rows
// and the largest draw-source table, else read from the blob in global memory (the same values either way).
template <class V>
struct UserTarget {
    const double *P;   // LDS copy of the parameters
    const double *Pg;  // the blob in global memory
    int d;
    bool lds;
    // cooperative layouts: the point's row, and (with a gradient) the gradient's row, per lane group
    static constexpr int kScratchPerChain = (V::L == 1) ? 0 : (kUserHasGradient ? 2 : 1) * V::DPAD + 1;
    __host__ __device__ static bool in_lds(int np)
    {
        return ((size_t)np + (size_t)kScratchPerChain * (kBlock / V::L) + kMixDrawsReserve) * sizeof(double) <= kMaxLdsBytes;
    }
    __host__ __device__ static size_t lds_doubles(int k, int /*d*/) { return in_lds(k) ? (size_t)k : 0; }
    __device__ void stage(double *l, const TargetBlock &tb)
    {
        d = tb.d;
        Pg = tb.blob;
        lds = in_lds(tb.k);
        P = l;
        if (lds)
            for (int i = threadIdx.x; i < tb.k; i += kBlock) l[i] = tb.blob[i];
    }
    // (two call sites, so that the LDS one addresses LDS directly instead of through flat pointers)
    __device__ __forceinline__ double call_logp(const double *x, int dd) const
    {
        return lds ? gsss_user_log_prob(x, dd, P) : gsss_user_log_prob(x, dd, Pg);
    }
    __device__ __forceinline__ void call_grad(const double *x, int dd, double *out) const
    {
        if constexpr (kUserHasGradient) {
            if (lds)
                gsss_user_gradient(x, dd, P, out);
            else
                gsss_user_gradient(x, dd, Pg, out);
        }
    }
    __device__ __forceinline__ double logp(const double (&y)[V::N], int g, double *scratch) const
    {
        if constexpr (V::L == 1) {
            return call_logp(y, V::N);  // lane layouts are built for d == N
        } else {
            // publish y to the group's LDS row; every lane evaluates the whole row and gets the same value
#pragma unroll
            for (int i = 0; i < V::N; ++i) scratch[V::comp(g, i)] = y[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double v = call_logp(scratch, d);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            return v;
        }
    }
    __device__ __forceinline__ void grad(const double (&y)[V::N], int g, double *scratch, double (&out)[V::N]) const
    {
#pragma unroll
        for (int i = 0; i < V::N; ++i) out[i] = 0.0;
        if constexpr (V::L == 1) {
            call_grad(y, V::N, out);
        } else {
            // the full gradient goes to the group's second row (lane 0 of the group evaluates it); each lane takes its own slots
            double *gr = scratch + V::DPAD;
#pragma unroll
            for (int i = 0; i < V::N; ++i) scratch[V::comp(g, i)] = y[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (g == 0) {
                for (int i = 0; i < d; ++i) gr[i] = 0.0;
                call_grad(scratch, d, gr);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int i = 0; i < V::N; ++i) {
                const int c = V::comp(g, i);
                out[i] = c < d ? gr[c] : 0.0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
};

// What a compiled module exports (gsss_user_module_table): the launchers of its one layout, and what it was built against.
// gsss_target_create_user checks module_abi, gsss_abi and digest before it reads anything else.
constexpr int32_t kUserModuleAbi = 1;

struct UserModuleTable {
    int32_t module_abi;    // kUserModuleAbi
    int32_t gsss_abi;      // GSSS_ABI_VERSION of the headers it was compiled with
    int32_t vec_id;        // the one vector layout it instantiates (GSSS_VEC_LIST id)
    int32_t has_gradient;  // gsss_user_gradient given: gradient and HMC kernels built
    const char *digest;    // geosss_amd/build.py source_digest() of the kernel sources it was compiled from
    int (*run)(int draws, const TargetBlock &tb, const RunBlock &rb, hipStream_t st);
    int (*logprob)(const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st);
    int (*mh)(int draws, int sampler, const TargetBlock &tb, const RunBlock &rb, const MhBlock &mb, hipStream_t st);
};

}  // namespace gsss
