// gsss_launch.h -- host-side dispatch from (target kind, vector layout, draw source) to a kernel.
#pragma once
#include "gsss_device.h"

namespace gsss {

// Vector layouts compiled in.  id -> type; ids are what gsss_run_args.variant selects.
using VL2 = LaneVec<2>;
using VL3 = LaneVec<3>;
using VL4 = LaneVec<4>;
using VL5 = LaneVec<5>;
using VL6 = LaneVec<6>;
using VL8 = LaneVec<8>;
using VL10 = LaneVec<10>;
using VC4x4 = CoopVec<4, 4>;
using VC4x8 = CoopVec<4, 8>;
using VC16x4 = CoopVec<16, 4>;
using VC16x8 = CoopVec<16, 8>;
using VC64x4 = CoopVec<64, 4>;
using VC64x8 = CoopVec<64, 8>;
using VC64x16 = CoopVec<64, 16>;
using VC64x32 = CoopVec<64, 32>;

#define GSSS_VEC_LIST(X) \
    X(1, VL2, "lane2")       \
    X(2, VL3, "lane3")       \
    X(3, VL4, "lane4")       \
    X(4, VL5, "lane5")       \
    X(5, VL6, "lane6")       \
    X(6, VL8, "lane8")       \
    X(7, VL10, "lane10")     \
    X(8, VC4x4, "coop4x4")   \
    X(9, VC4x8, "coop4x8")   \
    X(10, VC16x4, "coop16x4") \
    X(11, VC16x8, "coop16x8") \
    X(12, VC64x4, "coop64x4") \
    X(13, VC64x8, "coop64x8") \
    X(14, VC64x16, "coop64x16") \
    X(15, VC64x32, "coop64x32")

struct VecInfo {
    int id, L, N, dpad;
    bool exact_dim;
    const char *name;
};
const VecInfo *vec_table(int *count);
// id of the layout used for dimension d (variant == 0) or validation of a forced one; <0 on error
int select_vec(int d, int variant);

// draw source of a launch
enum : int { kDrawsPhilox = 0, kDrawsReplay = 1, kDrawsNumpy = 2 };
template <template <class> class DR>
struct DrawSource {};

// f(DrawSource<DR>{}) for the DR a launch's draw source names: the launchers below deduce DR from the tag
template <class F>
int with_draws(int draws, F &&f)
{
    if (draws == kDrawsReplay) return f(DrawSource<ReplayDraws>{});
    if (draws == kDrawsNumpy) return f(DrawSource<NumpyDraws>{});
    return f(DrawSource<PhiloxDraws>{});
}

// f(V{}) for the vector layout with this id
template <class F>
int with_layout(int vec_id, F &&f)
{
    switch (vec_id) {
#define GSSS_LAYOUT_CASE(ID, V, NAME) \
    case ID: return f(V{});
        GSSS_VEC_LIST(GSSS_LAYOUT_CASE)
#undef GSSS_LAYOUT_CASE
    }
    set_error("unknown vector layout %d", vec_id);
    return GSSS_E_INVALID;
}

template <template <class> class TT>
int launch_run(int vec_id, int draws, const TargetBlock &tb, const RunBlock &rb, hipStream_t st);
template <template <class> class TT>
int launch_logprob(int vec_id, const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st);

#define GSSS_HIP_TRY(expr)                                                              \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess) {                                                        \
            ::gsss::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return GSSS_E_HIP;                                                          \
        }                                                                               \
    } while (0)

// The dynamic LDS of an exact-mode launch of TT<V>, in doubles: the policy's rows, the lane groups' scratch rows, then kDraws
// doubles for the draw source's tables (0: the logprob kernels) -- the regions run_kernel, logprob_kernel and mh_kernel address.
// A policy that lays its LDS out itself (Mixture: launch_doubles) keeps a fixed reserve for the tables in the middle of it.
template <class T, class = void>
constexpr bool kOwnLdsLayout = false;
template <class T>
constexpr bool kOwnLdsLayout<T, decltype((void)T::launch_doubles(TargetBlock{}))> = true;

template <class V, template <class> class TT, int kDraws>
size_t exact_lds_doubles(const TargetBlock &tb)
{
    using T = TT<V>;
    if constexpr (kOwnLdsLayout<T>) {
        static_assert(kDraws <= kMixDrawsReserve, "the draw source's tables must fit the reserve");
        return T::launch_doubles(tb);
    } else {
        return T::lds_doubles(tb.k, tb.d) + scratch_doubles<V, T>() + (size_t)kDraws;
    }
}

// The one launch of an exact-mode kernel: its LDS by the rule above, refused beyond a workgroup's; kern(tb, args...) on `grid`
// workgroups.
template <class V, template <class> class TT, int kDraws, class Kern, class... Args>
int launch_exact(const char *family, Kern kern, int64_t grid, hipStream_t st, const TargetBlock &tb, const Args &...args)
{
    const size_t lds = exact_lds_doubles<V, TT, kDraws>(tb) * sizeof(double);
    if (lds > kMaxLdsBytes) {
        set_error("target parameters need %zu B of LDS (> %zu)", lds, kMaxLdsBytes);
        return GSSS_E_UNSUPPORTED;
    }
    if (int rc = allow_lds(family, kern, lds)) return rc;
    return launch_kernel(family, kern, grid, lds, st, nullptr, tb, args...);
}

template <class V, template <class> class TT, template <class> class DR>
int do_run(DrawSource<DR>, const TargetBlock &tb, const RunBlock &rb, hipStream_t st)
{
    auto kern = run_kernel<V, TT, DR, false>;
    if (rb.stats != nullptr) kern = run_kernel<V, TT, DR, true>;  // running statistics: a second build, so that the plain kernels carry none of it
    const int64_t per_block = (V::L == 1 && rb.spread) ? kBlock / 64 : kBlock / V::L;
    return launch_exact<V, TT, DR<V>::kLdsDoubles>("run", kern, ceil_div(rb.n_chains, per_block), st, tb, rb);
}

// (GRAD = false: a target without a gradient builds the value kernel alone)
template <class V, template <class> class TT, bool GRAD = true>
int do_logprob(const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st)
{
    auto kern = logprob_kernel<V, TT, false>;
    if constexpr (GRAD)
        if (grad) kern = logprob_kernel<V, TT, true>;
    return launch_exact<V, TT, 0>("logprob", kern, ceil_div(n, kBlock / V::L), st, tb, x, n, out);
}

// Each target's translation unit expands this once: run_kernel and logprob_kernel in every vector layout.
#define GSSS_DEFINE_TARGET_LAUNCHERS(TT)                                                                                       \
    template <>                                                                                                                \
    int launch_run<TT>(int vec_id, int draws, const TargetBlock &tb, const RunBlock &rb, hipStream_t st)                        \
    {                                                                                                                          \
        return with_layout(vec_id, [&](auto v) {                                                                               \
            return with_draws(draws, [&](auto dr) { return do_run<decltype(v), TT>(dr, tb, rb, st); });                        \
        });                                                                                                                    \
    }                                                                                                                          \
    template <>                                                                                                                \
    int launch_logprob<TT>(int vec_id, const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st) \
    {                                                                                                                          \
        return with_layout(vec_id, [&](auto v) { return do_logprob<decltype(v), TT>(tb, x, n, out, grad, st); });              \
    }

}  // namespace gsss
