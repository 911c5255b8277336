// gsss_user_module.hip -- the translation unit of a user-defined target (GSSS_USER), compiled by geosss_amd/usertarget.py,
// never by geosss_amd/build.py: it needs the user's source, a generated gsss_user_source.h found on the include path.
//   -DGSSS_USER_VEC=<id>            the one vector layout to instantiate (GSSS_VEC_LIST id: gsss_exact_layout(d))
//   -DGSSS_USER_HAS_GRADIENT=0|1    gsss_user_gradient is defined: the gradient and HMC kernels are built
//   -DGSSS_USER_DIGEST="<sha256>"   source_digest() of the kernel sources it is compiled from
// Kernels: run_kernel x {Philox, replay, numpy} x {statistics off, on}, logprob_kernel (value; gradient), mh_kernel x
// {Philox, replay, numpy} x {RWMH; HMC}.  The module links against libgsss_hip.so (set_error and the launch helpers' state stay
// the library's) and exports one symbol, gsss_user_module_table.
#include "gsss_user_target.h"

#include "gsss_user_source.h"

#ifndef GSSS_USER_VEC
#error "GSSS_USER_VEC (the vector layout id) is required"
#endif
#ifndef GSSS_USER_DIGEST
#error "GSSS_USER_DIGEST (the kernel sources' digest) is required"
#endif

namespace gsss {

template <int ID>
struct UserVec;
#define GSSS_USER_VEC_ROW(ID, V, NAME) \
    template <>                        \
    struct UserVec<ID> {               \
        using type = V;                \
    };
GSSS_VEC_LIST(GSSS_USER_VEC_ROW)
#undef GSSS_USER_VEC_ROW
using UV = UserVec<GSSS_USER_VEC>::type;

static int user_run(int draws, const TargetBlock &tb, const RunBlock &rb, hipStream_t st)
{
    static_assert(NumpyDraws<UV>::kLdsDoubles <= kMixDrawsReserve, "the draw source's tables must fit UserTarget's reserve");
    return with_draws(draws, [&](auto dr) { return do_run<UV, UserTarget>(dr, tb, rb, st); });
}

static int user_logprob(const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st)
{
    if (grad && !kUserHasGradient) {
        set_error("this user target defines no gsss_user_gradient");
        return GSSS_E_UNSUPPORTED;
    }
    return do_logprob<UV, UserTarget, kUserHasGradient>(tb, x, n, out, grad, st);
}

static int user_mh(int draws, int sampler, const TargetBlock &tb, const RunBlock &rb, const MhBlock &mb, hipStream_t st)
{
    if (!kUserHasGradient && sampler != GSSS_RWMH && sampler != GSSS_INDEP && sampler != GSSS_MIX) {
        set_error("spherical HMC needs the target's gradient: this user target defines no gsss_user_gradient");
        return GSSS_E_UNSUPPORTED;
    }
    return mh_dispatch<UV, UserTarget, kUserHasGradient>(draws, sampler, tb, rb, mb, st);
}

static const UserModuleTable kTable = {kUserModuleAbi, GSSS_ABI_VERSION, GSSS_USER_VEC, kUserHasGradient ? 1 : 0,
                                       GSSS_USER_DIGEST, user_run, user_logprob, user_mh};

}  // namespace gsss

extern "C" __attribute__((visibility("default"))) const void *gsss_user_module_table(void) { return &gsss::kTable; }
