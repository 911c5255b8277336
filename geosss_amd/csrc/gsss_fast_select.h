// gsss_fast_select.h -- which kernel a GSSS_MODE_FAST launch runs: the one table, shared by the launchers (gsss_run hands the
// pick to the family's launcher) and by the names (gsss_mode_supported, gsss_variant_name, gsss_kernel_name print the pick).
//
// Plain integers and bools only: no HIP header, no environment, no call into the library -- the header compiles with a host
// compiler alone (tests/test_fast_select.py runs it against the recorded table of tests/golden/fast_kernel_names.json).
// What a launcher decides AFTER the pick -- the stream's build (Philox, replayed, numpy), the statistics build, and everything
// do_screened_run plans from occupancy -- needs the device and is not part of it.
#pragma once
#include <stdio.h>

#include "../../include/gsss.h"

namespace gsss {

constexpr double kScreenMaxKappa = 4000.0;  // margin ~ 2e-6 kappa: beyond this a few per cent of the tries stay undecided
constexpr int kMixFastTerms = 8;            // terms of the one FastMixture build per dimension

enum FastFamily { kFamScreened, kFamFast, kFamWave, kFamCoopFast, kFamCurveSpec, kFamCurve64 };
enum FastFlavour { kFlavVmf, kFlavBingham, kFlavBinghamDiag, kFlavCurve, kFlavMixture, kFlavAcg };

struct FastAsk {
    int kind, d;     // GSSS_VMF_MIXTURE, GSSS_BINGHAM, GSSS_CURVE_VMF, GSSS_MIXTURE, GSSS_ACG
    int k;           // TargetBlock::k: components | Bingham flags (bit 0 a diagonal A, bit 1 a linear term) | knots; mix_info's terms
    bool mix_curve;  // GSSS_MIXTURE: mix_info's curve (a curve-vMF component)
    double scale;    // TargetBlock::scale
    int screen;      // RunBlock::screen: 0 all-double, 1 screened, 2 verified
    bool spread, numpy, replay, stats;  // one wavefront per chain; numpy's stream (rng_state); replayed stream; running statistics
    bool batch;      // a target batch: one lane per chain whatever the placement
    int curve_tail;  // GSSS_CURVE_TAIL (unset: 1)
    bool curve_l2;   // GSSS_CURVE_L2=1
};

struct FastPick {
    int family, flavour;
    int d;     // lane-per-chain kernels (screened, fast, wave): the D they are built for
    int l, s;  // coopfast: CoopVec<L, S>; curvespec: L lanes per chain, Q = s quads per lane
    int kc;    // the bucket the kernel is built for: components (Vmf), terms (Mixture), knots (Curve)
    int r, nv; // curvespec: tail slots per lane; curve64: NV
    bool batch;
    bool lane;  // a lane-per-chain kernel exists for this shape ("fast-lane": numpy's stream, one-wavefront placement)
};

namespace fast_select_detail {

// Kernels are built per component-count BUCKET: a mixture of K components runs the kernel of the smallest bucket >= K
// (the surplus components are padded with exact zeros, so the bucket does not change a single bit of the chain).
constexpr int kScreenBuckets[] = {3, 4, 6, 10, 16};  // screened lane kernels, d = 3 .. 10
constexpr int kWideBuckets[] = {3, 6, 10};           // screened lane kernels, d = 11 .. 16
constexpr int kDoubleBuckets[] = {4, 16};            // all-double / one-wavefront kernels, d = 3 .. 10
// (batch only) all-double at d = 11 .. 16, which a single target has no lane build of: bucket 16, the one of d <= 10, spills at
// d >= 14 (256 registers and 760 .. 1208 bytes of scratch a lane); bucket 10 takes 199 at d = 16
constexpr int kBatchWideDoubleBuckets[] = {4, 10};
constexpr int kCoopBuckets[] = {3, 5, 10, 16};       // cooperative kernels

template <int N>
constexpr int bucket(int k, const int (&b)[N])
{
    for (int i = 0; i < N; ++i)
        if (k <= b[i]) return b[i];
    return b[N - 1];
}

// d = 11 .. 16 (round 4): the screened lane kernel alone, one chain per lane.  What it does not serve -- replayed and numpy
// streams, one-wavefront placement, the all-double variant -- stays with the cooperative kernels.
constexpr bool lane_wide_serves(const FastAsk &a) { return a.screen != 0 && !a.spread && !a.numpy && !a.replay; }

// The wide cooperative Bingham layout CoopBingham<CoopVec<16, 8>>: A must fit the LDS beside the groups' scratch rows.
// (gsss_fast_bingham.hip ties these integers to coop_param_doubles, kScratchPerGroup, kBlock and kMaxLdsBytes.)
constexpr int kBlockThreads = 256;
constexpr long kLdsBytes = 160 * 1024;
constexpr int kWideBinghamL = 16, kWideBinghamS = 8, kWideBinghamDpad = kWideBinghamL * kWideBinghamS;
constexpr long wide_bingham_param_doubles(int d) { return (long)(d + 1) * kWideBinghamDpad; }  // rows of A, and b
constexpr long kWideBinghamScratchPerGroup = 2 * kWideBinghamDpad + 2;
constexpr bool wide_bingham_fits(int d)
{
    return (wide_bingham_param_doubles(d) + kWideBinghamScratchPerGroup * (kBlockThreads / kWideBinghamL)) * 8 <= kLdsBytes;
}

// a pick of a lane-per-chain kernel <D, ..KC..> / of a cooperative one <CoopVec<L, S>, ..KC..>
inline int lane_pick(FastPick &p, int family, int d, int kc = 0) { return p.family = family, p.d = d, p.kc = kc, GSSS_OK; }
inline int coop_pick(FastPick &p, int l, int s, int kc = 0) { return p.family = kFamCoopFast, p.l = l, p.s = s, p.kc = kc, GSSS_OK; }
// the all-double lane kernel, or its one-wavefront-per-chain form for a small ensemble (built for d <= 16; a replayed stream is
// a sequential source and stays with fast_kernel)
inline int double_family(const FastAsk &a) { return (a.spread && !a.replay && a.d <= 16) ? kFamWave : kFamFast; }

inline int select_vmf(const FastAsk &a, FastPick &p)
{
    const int d = a.d, k = a.k;
    p.flavour = kFlavVmf;
    const bool in_reach = a.scale <= kScreenMaxKappa;  // of the single-precision screen
    if (a.batch) {  // screened wherever the concentration allows, else all-double: no other stream, no other placement
        const bool wide = d >= 11 && d <= 16;
        if (!(k >= 1 && ((d >= 3 && d <= 10 && k <= 16) || (wide && k <= 10)))) return GSSS_E_UNSUPPORTED;
        p.lane = true;
        if (a.screen != 0 && in_reach) return lane_pick(p, kFamScreened, d, wide ? bucket(k, kWideBuckets) : bucket(k, kScreenBuckets));
        // the batch build departs from the single-target one HERE: at d = 11 .. 16 it has an all-double lane kernel
        return lane_pick(p, kFamFast, d, wide ? bucket(k, kBatchWideDoubleBuckets) : bucket(k, kDoubleBuckets));
    }
    // lane-per-chain kernels, d = 3 .. 10, any K <= 16
    if (k >= 1 && k <= 16 && d >= 3 && d <= 10) {
        p.lane = true;
        const int ks = bucket(k, kScreenBuckets);
        // the screened kernel unless the caller forces all-double arithmetic, the ensemble is small (one wavefront per chain), or
        // the concentration is so large that the margin would leave tries undecided.  numpy's stream for a packed ensemble: the
        // screened kernel too (round 4; K <= 10 -- the widest bucket stays all-double)
        if (a.screen != 0 && !a.spread && in_reach && (!a.numpy || (ks <= 10 && !a.replay))) return lane_pick(p, kFamScreened, d, ks);
        return lane_pick(p, double_family(a), d, bucket(k, kDoubleBuckets));
    }
    // d = 11 .. 16, K <= 10, packed ensembles on the library stream: still one lane per chain (round 4; rounds 1-3 dropped to the
    // four-lane cooperative kernel at d = 11: 1.3 - 2.6e10 -> ~5e9 chain-steps/s)
    if (k >= 1 && k <= 10 && d >= 11 && d <= 16 && in_reach && lane_wide_serves(a))
        return lane_pick(p, kFamScreened, d, bucket(k, kWideBuckets));
    // larger d: lanes cooperate on one chain (surplus components padded, as above)
    if (k >= 1 && k <= 16 && d > 10 && d <= 256) {
        // Lanes per chain x slots per lane (d <= lanes x slots).  The per-step serial work -- Philox and Box-Muller rounds, the
        // reductions, the try loop -- is repeated in every lane of a group, so few lanes with many slots win as long as the
        // registers hold them (16 slots: two wavefronts per SIMD).  Measured at 10^5 chains, K = 5 (10^9 chain-steps/s):
        // d = 32 <4,8> 2.8 against <16,4> 1.1; d = 50 <4,16> 2.2 / <8,8> 1.7 / <16,4> 1.1; d = 100 <8,16> 1.33 / <16,8> 1.05
        // / <64,4> 0.37; d = 200 (K = 3) <16,16> 0.92 against <64,4> 0.50.
        return coop_pick(p, d <= 64 ? 4 : (d <= 128 ? 8 : 16), d <= 16 ? 4 : (d <= 32 ? 8 : 16), bucket(k, kCoopBuckets));
    }
    return GSSS_E_UNSUPPORTED;
}

inline int select_bingham(const FastAsk &a, FastPick &p)
{
    const int d = a.d;
    // The paper's eigenbasis targets (diagonal, no linear term) run the compact screen target (three wavefronts per SIMD at
    // d = 9, 10: ScreenBinghamDiag, gsss_screen.h); a batch: when every member's A is diagonal and none has a linear term
    const int screened = a.k == 1 ? kFlavBinghamDiag : kFlavBingham;
    p.flavour = kFlavBingham;
    if (a.batch) {
        if (d < 3 || d > 16) return GSSS_E_UNSUPPORTED;
        p.lane = true;
        if (a.screen != 0) p.flavour = screened;
        // (the batch build departs from the single-target one HERE: an all-double lane kernel at d = 11 .. 16 too)
        return lane_pick(p, a.screen != 0 ? kFamScreened : kFamFast, d);
    }
    if (d >= 3 && d <= 10) {
        p.lane = true;
        if (!(a.screen != 0 && !a.spread && (!a.numpy || !a.replay))) return lane_pick(p, double_family(a), d);
        p.flavour = screened;  // (numpy's stream, packed: the screened kernel too)
        return lane_pick(p, kFamScreened, d);
    }
    // d = 11 .. 16, packed ensembles on the library stream: still one lane per chain (round 4)
    if (d >= 11 && d <= 16 && lane_wide_serves(a)) {
        p.flavour = screened;
        return lane_pick(p, kFamScreened, d);
    }
    // larger d: lanes cooperate on one chain.  A must fit the LDS beside the groups' scratch rows: d <= 126 ((d + 1) x 128 doubles
    // of rows + 16 groups x 258 of scratch in 160 KB) -- beyond, fast mode is not offered and mode "auto" runs the exact kernels
    // (which read a dense A of d > 128 from global memory)
    if (d > 10 && d <= 128 && (d <= 64 || wide_bingham_fits(d))) {
        // Lanes per chain x slots per lane, measured at 10^5 chains (10^9 chain-steps/s, eigenbasis / dense A): d <= 32 four
        // lanes with eight slots 5.3 / 3.5 against 2.4 / 1.8 for sixteen lanes with four (the per-step serial work -- Philox
        // and Box-Muller rounds, reductions, the try loop -- is repeated in every lane of a group, and sixteen groups share a
        // wavefront); d <= 64 eight lanes with eight slots for a diagonal A (3.0 against 2.6), sixteen with four for a dense
        // one (its d x d products want the lanes: 1.36 against 1.26).
        const bool diag = (a.k & 1) != 0;
        return coop_pick(p, d <= 32 ? 4 : (d <= 64 && diag ? 8 : 16), d <= 16 ? 4 : (d <= 32 || d > 64 || diag ? 8 : 4));
    }
    return GSSS_E_UNSUPPORTED;
}

// The group-speculative curve kernel (gsss_curvespec.h): L lanes per chain, L speculative single-precision tries per batch,
// Q component quads per lane (d <= 4 Q L), kernels built for 10 and for 17 knots.
inline int select_curvespec(const FastAsk &a, FastPick &p)
{
    const int d = a.d, k = a.k;
    p.family = kFamCurveSpec;
    p.kc = k <= 10 ? 10 : 17;
    auto layout = [&p](int l, int q, int r = 0) { return p.l = l, p.s = q, p.r = r, GSSS_OK; };
    // d <= 16, <= 10 knots: TWO lanes per chain with eight components each were measured in round 3 (32 chains share a
    // wavefront's per-step serial work instead of 16) and LOST: 25.6 against 20.7 ms per 10^8 chain-steps at d = 10 -- batches of
    // two speculative tries need 3.9 instead of 2.3 rounds of the single-precision curve evaluation per step, and eight
    // components per lane only fit three wavefronts per SIMD with u parked in LDS and 36 B of scratch.  GSSS_CURVE_L2=1 runs
    // them (parity-tested: the kernel is generic in L), the default stays with four-lane groups.
    if (d <= 16 && k <= 10 && a.curve_l2) return layout(2, 2);
    // Round 5: dimensions that miss a whole number of quads per lane by at most two components per lane run an UNEVEN layout -- Q
    // quads and R = 1 or 2 tail slots per lane (gsss_curvespec.h) -- in the register class of the Q-quad build instead of the
    // (Q + 1)-quad one (four quads: two wavefronts per SIMD instead of three).  Measured, ms per 10^8 chain-steps against the even
    // layout (profiles/r05_ab_curve_tail.log):
    //   <4, 1, 10, +1>  d = 17 .. 20    d = 18: 20.84 -> 19.53 (+6.7 %)      <4, 1, 10, +2>  d = 21 .. 24    d = 24 (bench): 20.74 -> 20.05 (+3.4 %)
    //   <4, 2, 10, +1>  d = 33 .. 36    d = 34: 23.80 -> 22.20 (+7.2 %)      <4, 2, 10, +2>  d = 37 .. 40    d = 38: 24.05 -> 23.12 (+4.0 %)
    //   <4, 3, 10, +1>  d = 49 .. 52    d = 50 (BASELINE cfg4): 31.40 -> 25.29 (+24 %)
    //   <4, 3, 10, +2>  d = 53 .. 56    d = 54: 31.47 -> 26.47 (+19 %) -- two tail slots stay in registers: parked in LDS the workgroup is
    //                                   54.1 KB and the CU holds two of them (32.2 ms)
    //   <8, 3, 10, +1>  d = 97 .. 104   d = 100: 52.07 -> 43.64 (+19 %)      <8, 3, 10, +2>  d = 105 .. 112  d = 108: 52.43 -> 45.06 (+16 %)
    //   <16, 3, 10, +1> d = 193 .. 208  d = 200 (cfg4): 93.78 -> 74.45 (+26 %) -- its ONE tail slot in a register for the same reason
    //   (<16, 3, 10, +2>, d = 209 .. 224: 55 KB of LDS whatever is parked, two workgroups per CU: 93.9 -> 98.8 ms; not built)
    // GSSS_CURVE_TAIL=0 turns the layouts off (A/B).  Plain and replayed launches of curves of <= 10 knots; statistics builds keep
    // the even layouts.
    if (k <= 10 && !a.stats && a.curve_tail >= 1) {
        // <L, Q, +R> holds 4 Q L + R L components: four-lane groups at d <= 64, eight at 65 .. 128, sixteen beyond
        static constexpr struct {
            int above, upto, l, q, r;
        } kTail[] = {{16, 20, 4, 1, 1},  {20, 24, 4, 1, 2},   {32, 36, 4, 2, 1},   {36, 40, 4, 2, 2},   {48, 52, 4, 3, 1},
                     {52, 56, 4, 3, 2},  {96, 104, 8, 3, 1},  {104, 112, 8, 3, 2}, {192, 208, 16, 3, 1}};
        for (const auto &t : kTail)
            if (d > t.above && d <= t.upto) return layout(t.l, t.q, t.r);
    }
    // Measured at 10^5 chains (tools/bench_curve_sweep.py, 10^9 chain-steps/s): d = 17 .. 32 <4,2> 2.6 against <16,1> 1.8;
    // d = 33 .. 48 <4,3> 2.2 / 1.8; d = 49 .. 64 <4,4> 2.1 / 1.8 -- the per-step serial work is repeated in 4 instead of 16 lanes,
    // and sixteen groups share a wavefront.  (<4,4> with 17 knots spills registers: those shapes stay with <16,1>.)
    if (d <= 16) return layout(4, 1);
    if (d <= 32) return layout(4, 2);
    if (d <= 48) return layout(4, 3);
    if (d <= 64) return k <= 10 ? layout(4, 4) : layout(16, 1);
    // d = 65 .. 128, <= 10 knots: eight-lane groups (1.6 / 1.4 against 1.2 for <16,2>)
    if (d <= 96 && k <= 10) return layout(8, 3);
    if (d <= 128) return k <= 10 ? layout(8, 4) : layout(16, 2);
    if (d <= 192) return layout(16, 3);
    return layout(16, 4);
}

// d = 3, 6, ..., 24 is the reference's own sweep (sh/submit_job_curve_varying_ndim.sh:11); d = 10 its default
constexpr bool curve_lane_dim(int d) { return d == 10 || (d >= 3 && d <= 24 && d % 3 == 0); }

inline int select_curve(const FastAsk &a, FastPick &p)
{
    const int d = a.d, k = a.k;
    p.flavour = kFlavCurve;
    if (a.batch) return GSSS_E_UNSUPPORTED;
    // (knot counts: what the all-double / one-wavefront kernels below cover too, so that a shape is either served in every
    // placement and variant or in none)
    // d >= 4: on S^2 the Philox stream draws the tangent as one angle, which only the lane kernels do.  (Round 3: from d = 4,
    // not 9 -- 10^5 chains, 10^9 chain-steps/s: d = 6 2.97 (screened lane kernel) -> 4.74, d = 4, 5, 7, 8 1.05 (sixteen-lane
    // cooperative kernel) -> 4.6 .. 4.8.)  Packed ensembles on the Philox or replay stream, screening on; the numpy stream and
    // one-wavefront-per-chain placement stay with the lane / cooperative kernels below.
    const bool spec = a.screen != 0 && !a.spread && !a.numpy && k >= 2 && k <= (d > 64 ? 17 : 16) && d >= 4 && d <= 256;
    // lane-per-chain kernels: the listed dimensions, any curve of 2 .. 10 knots (built for 10; FastCurve pads)
    if (curve_lane_dim(d) && k >= 2 && k <= 10) {
        p.lane = true;
        if (spec) return select_curvespec(a, p);
        return lane_pick(p, a.screen != 0 && !a.spread && !a.numpy ? kFamScreened : double_family(a), d, 10);
    }
    if (spec) return select_curvespec(a, p);
    // 64 < d <= 256, up to 17 knots: one chain per wavefront, four speculative tries per iteration
    if (d > 64 && d <= 256 && k >= 2 && k <= 17) {
        p.family = kFamCurve64;
        p.nv = k <= 11 ? 12 : 20;
        return GSSS_OK;
    }
    // every other d <= 64 (and 11 .. 16 knots at the lane dimensions): 16 lanes cooperate on one chain
    if (d >= 3 && d <= 64 && k >= 2 && k <= 16) return coop_pick(p, 16, 4, k <= 10 ? 10 : 16);
    if (k >= 2 && k <= 10 && d > 256 && d <= 512) return coop_pick(p, 64, 8, 10);
    return GSSS_E_UNSUPPORTED;
}

// GSSS_MIXTURE: one all-double lane build of kMixFastTerms terms per dimension d = 3 .. 16, no single-precision screen;
// everything else (a curve component, more terms, other d) is not built and mode "auto" runs the exact kernels
inline int select_mixture(const FastAsk &a, FastPick &p)
{
    p.flavour = kFlavMixture;
    if (a.batch || a.mix_curve || a.k < 1 || a.k > kMixFastTerms || a.d < 3 || a.d > 16) return GSSS_E_UNSUPPORTED;
    p.lane = true;
    return lane_pick(p, double_family(a), a.d, kMixFastTerms);
}

// GSSS_ACG: the all-double lane kernels at d = 3 .. 10 in every stream and placement that Bingham's all-double pick serves.  A try
// is three double FMAs and a comparison already (FastAcg, gsss_fast.h), so there is no single-precision screen and a.screen does
// not enter; no batch build, no cooperative kernel: other d are not built and mode "auto" runs the exact kernels
inline int select_acg(const FastAsk &a, FastPick &p)
{
    p.flavour = kFlavAcg;
    if (a.batch || a.d < 3 || a.d > 10) return GSSS_E_UNSUPPORTED;
    p.lane = true;
    return lane_pick(p, double_family(a), a.d);
}

}  // namespace fast_select_detail

// GSSS_OK and the pick, or GSSS_E_UNSUPPORTED: fast mode has no kernel for this shape with these traits
inline int fast_select(const FastAsk &a, FastPick &p)
{
    p = FastPick{};
    p.batch = a.batch;
    switch (a.kind) {
    case GSSS_VMF_MIXTURE: return fast_select_detail::select_vmf(a, p);
    case GSSS_BINGHAM: return fast_select_detail::select_bingham(a, p);
    case GSSS_CURVE_VMF: return fast_select_detail::select_curve(a, p);
    case GSSS_MIXTURE: return fast_select_detail::select_mixture(a, p);
    case GSSS_ACG: return fast_select_detail::select_acg(a, p);
    }
    return GSSS_E_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------
// The launch plan of a fast-mode batch: what gsss_run launches and gsss_batch_plan reports.  A pure function of the members'
// shape (kind, d, K) and of m, the chains per target -- not of the variant a launch asks for (screened or all-double, diagonal
// or dense Bingham), so that one answer holds for every launch of the batch: the LDS is budgeted for the widest rows any batch
// kernel of the shape stages.
//   m a multiple of the workgroup's 256 chains: the BatchBlock builds (gsss_batch.h) -- one target per workgroup, targets x m / 256
//   workgroups, every lane busy.
//   otherwise the SHARED builds (BatchShared): a workgroup takes per_block consecutive chains of the launch and stages
//   every target they touch.  per_block is the largest count <= 256 whose runs touch no more targets than the LDS SHARE holds:
//   the CU's 160 KB (128 allocation granules of 1280 B) divided among as many workgroups as the registers of the shape's batch
//   builds let a CU hold (batch_resident), so that staging more targets never costs a resident workgroup.
// ------------------------------------------------------------------------------------------
constexpr int kBatchBlock = 256;                  // = kBlock
constexpr int kBatchTabDoubles = 2 * 64 + 2;      // = kTabLds: the draw tables every lane kernel stages
constexpr long kBatchLdsBytes = 160 * 1024;       // = kMaxLdsBytes
constexpr long kBatchLdsGranule = 1280;           // LDS is allocated in granules of 320 dwords on gfx950

struct BatchPlan {
    bool shared;     // the BatchShared builds; else the BatchBlock ones (gsss_batch.h)
    int per_block;   // chains a workgroup takes
    int targets;     // the most targets a workgroup stages
    long long grid;  // workgroups: ceil(n_targets m / per_block)
    double lane_use; // chains / (grid x per_block)
    int stride;      // (shared) doubles a target is budgeted in LDS: the widest rows of the shape, padded to an odd count
};

namespace fast_select_detail {

// the widest rows (doubles) a batch kernel of the shape stages per target: vMF mixtures K_C (d + 1) in the larger of the screened
// and the all-double bucket; Bingham A and b (the diagonal screen target stages d of them)
inline int batch_rows(int kind, int d, int k)
{
    if (kind == GSSS_BINGHAM) return d * d + d;
    const bool wide = d >= 11;
    const int ks = wide ? bucket(k, kWideBuckets) : bucket(k, kScreenBuckets);
    const int kd = wide ? bucket(k, kBatchWideDoubleBuckets) : bucket(k, kDoubleBuckets);
    return (ks > kd ? ks : kd) * (d + 1);
}

// Workgroups of 256 lanes a CU holds of the batch builds of the shape -- wavefronts per SIMD of their code objects, the most
// over the shape's variants (a larger number only makes the share smaller).  tests/test_target_batch_plan.py holds the
// code objects of the shared builds to it.  Read off the BatchBlock builds: on S^2 five (88 .. 115 registers) but for
// mixtures of K >= 5, everywhere else four (Bingham d = 4 .. 8 and 11 .. 13, mixtures in the buckets 3 and 4) or fewer; mixtures
// of K >= 5 three (135 .. 168 registers screened, two for the all-double buckets 10 and 16).
inline int batch_resident(int kind, int d, int k)
{
    if (kind == GSSS_VMF_MIXTURE && k >= 5) return 3;
    return d == 3 ? 5 : 4;
}

// the most targets a run of c consecutive chains touches when runs start at multiples of c and targets at multiples of m: the
// worst start lies m - gcd(c, m) chains into a target
inline long long batch_targets_touched(long long c, long long m)
{
    long long g = c, r = m;
    while (r) {
        const long long t = g % r;
        g = r;
        r = t;
    }
    return (m - g + c - 1) / m + 1;
}

}  // namespace fast_select_detail

// GSSS_OK and the plan of a batch of n_targets members with m chains each, or GSSS_E_UNSUPPORTED: no fast batch kernel
inline int batch_plan(int kind, int d, int k, long long n_targets, long long m, BatchPlan &bp)
{
    using namespace fast_select_detail;
    FastAsk a{};
    a.kind = kind, a.d = d, a.k = kind == GSSS_BINGHAM ? 0 : k, a.screen = 1, a.batch = true;
    FastPick p;
    if ((kind != GSSS_VMF_MIXTURE && kind != GSSS_BINGHAM) || n_targets < 1 || m < 1 || fast_select(a, p) != GSSS_OK) return GSSS_E_UNSUPPORTED;
    const long long n = n_targets * m;
    bp = BatchPlan{};
    bp.per_block = kBatchBlock;
    bp.targets = 1;
    bp.stride = batch_rows(kind, d, k) | 1;
    if (m % kBatchBlock != 0) {
        const long share = (kBatchLdsBytes / kBatchLdsGranule / batch_resident(kind, d, k)) * kBatchLdsGranule;
        const long long fit = (share / 8 - kBatchTabDoubles) / bp.stride;  // >= 1: the largest rows are 272 doubles
        bp.shared = true;
        while (batch_targets_touched(bp.per_block, m) > fit) --bp.per_block;  // (one chain touches one target)
        const long long touched = batch_targets_touched(bp.per_block, m);
        bp.targets = (int)(touched < n_targets ? touched : n_targets);
    }
    bp.grid = (n + bp.per_block - 1) / bp.per_block;
    bp.lane_use = (double)n / ((double)bp.grid * bp.per_block);
    return GSSS_OK;
}

// the instantiation a pick stands for, e.g. "screened_kernel<3, ScreenVmf<3, 3>>" (", batch" appended for the batch build)
inline void fast_name(const FastPick &p, char *buf, size_t n)
{
    static const char *const kFlavour[] = {"Vmf", "Bingham", "BinghamDiag", "Curve", "Mixture", "Acg"};
    const char *flav = p.flavour >= 0 && p.flavour <= kFlavAcg ? kFlavour[p.flavour] : "?";
    const bool bucketed = p.flavour == kFlavVmf || p.flavour == kFlavCurve || p.flavour == kFlavMixture;
    char kc[16] = "";
    if (bucketed) snprintf(kc, sizeof(kc), p.family == kFamCoopFast ? "<%d>" : ", %d", p.kc);
    switch (p.family) {
    case kFamScreened:
    case kFamFast:
    case kFamWave:
        snprintf(buf, n, "%s<%d, %s%s<%d%s>%s>", p.family == kFamScreened ? "screened_kernel" : (p.family == kFamWave ? "wave_kernel" : "fast_kernel"),
                 p.d, p.family == kFamScreened ? "Screen" : "Fast", flav, p.d, kc, p.batch ? ", batch" : "");
        return;
    case kFamCoopFast: snprintf(buf, n, "coopfast_kernel<CoopVec<%d, %d>, Coop%s%s>", p.l, p.s, flav, kc); return;
    case kFamCurveSpec:
        if (p.r)
            snprintf(buf, n, "curvespec_kernel<%d, %d, %d, +%d>", p.l, p.s, p.kc, p.r);
        else
            snprintf(buf, n, "curvespec_kernel<%d, %d, %d>", p.l, p.s, p.kc);
        return;
    case kFamCurve64: snprintf(buf, n, "curve64_kernel<%d>", p.nv); return;
    }
    snprintf(buf, n, "?<family %d, flavour %d>", p.family, p.flavour);
}

}  // namespace gsss
