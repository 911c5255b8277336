/*
 * gsss.h -- C ABI of libgsss_hip.so: many-chain geodesic slice sampling on the sphere,
 * hand-written HIP for gfx950 (MI355X).
 *
 * The reference (microscopic-image-analysis/geosss) is pure Python and has no FFI for
 * this path; its boundary is the duck-typed protocol
 *     Sampler(distribution, initial_state, seed).sample(n_samples, burnin)
 *     distribution.log_prob(x)
 * (geosss/mcmc.py:28-77, 340-401; geosss/distributions.py:16-25).  The entry points
 * below are what a ctypes binding of that protocol needs; each names the reference
 * code it replaces.  INTEGRATION.md shows the binding a geosss maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success or a negative GSSS_E_* code and never throws;
 *    gsss_last_error() gives the message of the calling thread's last failure.
 *  - pointers named *_dev are DEVICE pointers on the target's device; the caller owns
 *    every buffer, the library keeps none of them past the call (asynchronous work is
 *    ordered on `stream`, so keep buffers alive until the stream has drained).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls only
 *    enqueue work; nothing synchronises except gsss_stream_synchronize/gsss_memcpy_*.
 *  - all floating point is IEEE double, as in the reference.
 *  - chain states are stored component-major ("SoA"): state_dev[j * n_chains + c] is
 *    component j of chain c, so that one wavefront reads 64 consecutive doubles.
 */
#ifndef GSSS_H
#define GSSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSSS_ABI_VERSION 10

/* target families (geosss/distributions.py) */
#define GSSS_VMF_MIXTURE 1 /* MixtureModel of VonMisesFisher  :117-160, :209-227 */
#define GSSS_BINGHAM 2     /* Bingham                         :36-103            */
#define GSSS_CURVE_VMF 3   /* CurvedVonMisesFisher+SlerpCurve :261-278, spherical_curve.py:10-32,74-102 */
#define GSSS_CPD 4         /* registration.py: CoherentPointDrift :186-293 / GaussianMixtureModel :62-118 on unit quaternions (d = 4) */
#define GSSS_MIXTURE 5     /* MixtureModel of any components :209-227 -- made by gsss_target_create_mixture, never by gsss_target_create:
                              logsumexp_c(log_prob_c + log w_c); components GSSS_VMF_MIXTURE, GSSS_BINGHAM (with or without b) or
                              GSSS_CURVE_VMF of one d, at most 16 of them and 2^20 parameter rows in all (vMF means, knots, d + 1 per
                              Bingham).  Fast mode: d = 3 .. 16, at most 8 vMF / Bingham terms, no curve component. */
#define GSSS_USER 6        /* a density the user writes in C++ (Distribution subclassed, distributions.py:16-25), compiled into a module of
                              its own for ONE vector layout and made by gsss_target_create_user, never by gsss_target_create.
                              GSSS_MODE_EXACT only; no mixture component. */
#define GSSS_ACG 7         /* ACG :199-206: log p(x) = -(d / 2) log(x^T Lambda x), unnormalised.  gsss_target_desc::A
                              carries Lambda [d][d], symmetric positive definite (GSSS_E_INVALID otherwise: gsss_target_create checks
                              the symmetry and runs a host Cholesky); mu, logc, knots and k are unused.  Every exact layout, the four
                              MH / HMC samplers, log_prob and gradient = -d Lambda x / (x^T Lambda x).  Fast mode: d = 3 .. 10, the
                              all-double lane kernels (the accept test q(theta) < q(x) U^(-2/d) needs no logarithm per try, so there
                              is no single-precision screen); other d: GSSS_E_UNSUPPORTED.  No mixture component, no batch member. */

/* samplers (geosss/mcmc.py) */
#define GSSS_SHRINK 0 /* ShrinkageSphericalSliceSampler.__next__  :382-401 */
#define GSSS_REJECT 1 /* RejectionSphericalSliceSampler.__next__  :357-374 */
#define GSSS_RWMH 2   /* MetropolisHastings.__next__ (random-walk MH)  :138-167, AdaptiveStepsize :80-115 */
#define GSSS_HMC 3    /* SphericalHMC.__next__ (leapfrog on the sphere) :270-319 */
#define GSSS_INDEP 4  /* IndependenceSampler: proposal = a uniform point of the sphere          :179-182 */
#define GSSS_MIX 5    /* MixtureRWMHIndependenceSampler: RWMH with probability alpha, else the independence proposal :185-234 */

/* arithmetic of the proposal evaluation */
#define GSSS_MODE_EXACT 0 /* y = cos*x + sin*u formed, log_prob(y) evaluated from y op by op as the reference does */
#define GSSS_MODE_FAST 1  /* log_prob restricted to the great circle: O(1) per try after O(d) per step (same value to ~1e-14) */

/* gsss_run_args.variant in GSSS_MODE_FAST: 0 = library's choice (tries screened in single precision with a rigorous error
 * margin, double precision where the margin does not decide: same chains); this value forces the all-double kernels */
#define GSSS_VARIANT_FAST_DOUBLE 100
/* verification: the library's choice of kernel with the verdicts of its single-precision screen ignored where that kernel
 * can do so (the group-speculative curve-vMF kernel and the lane kernels of d = 11 .. 16: every try is decided in double
 * precision by the same arithmetic, so the run must reproduce variant 0 bit for bit); other kernels run as with variant 0 */
#define GSSS_VARIANT_FAST_VERIFY 101

/* return codes */
#define GSSS_OK 0
#define GSSS_E_INVALID (-1)     /* bad argument */
#define GSSS_E_UNSUPPORTED (-2) /* shape outside what the kernels cover */
#define GSSS_E_HIP (-3)         /* a HIP runtime call failed */
#define GSSS_E_NO_DEVICE (-4)   /* no usable gfx950 device */

/* per-chain error bits written to gsss_run_args.err_dev */
#define GSSS_CHAIN_MAX_TRIES 1        /* shrink/reject loop hit max_tries; state left at x */
#define GSSS_CHAIN_NONFINITE 2        /* log_prob(state) was -inf/NaN (reference would spin forever, mcmc.py:394) */
#define GSSS_CHAIN_REPLAY_EXHAUSTED 4 /* replay stream shorter than the draws consumed */
#define GSSS_CHAIN_COUNTER_SATURATED 8 /* fast mode counts the proposals of ONE launch in 32 bits: more than 2^32-1 of them
                                          in a single gsss_run call leave n_tries/n_reject too small (split the call) */

/* gsss_run_args.stats_flags */
#define GSSS_STATS_NO_SECOND_MOMENT 1 /* stats_dev has no sum x_i x_j rows (T = 0 below): they grow as d^2 -- 20 100 rows at d = 200 */

typedef struct gsss_target gsss_target; /* opaque; owns a small device parameter block */

/*
 * Host-side description of a target.  All pointers are HOST pointers, copied at create.
 *   VMF_MIXTURE: k components on S^{d-1}.  mu[k][d] = kappa_k * direction_k exactly as
 *       VonMisesFisher stores it (distributions.py:126-127);  logc[k] = log(w_k) - log(2 pi)
 *       - log(i0(|mu_k|)) = the x-independent part of distributions.py:157 and :220.
 *   BINGHAM:     A[d][d] symmetric (distributions.py:67-70); if mu is non-NULL it is the vector b[d] of a
 *       BinghamFisher target, log_prob = x^T A x + x.b (distributions.py:106-114).
 *   CURVE_VMF:   knots[k][d] unit vectors, kappa (distributions.py:263-265).
 *   ACG:         A[d][d] = Lambda = C^-1, symmetric positive definite (distributions.py:199-206 with invC = Lambda).
 *   CPD:         see the fields below; GSSS_MODE_EXACT, lane-per-chain kernels; samplers GSSS_SHRINK / GSSS_REJECT / GSSS_RWMH.
 */
typedef struct gsss_target_desc {
    int32_t kind;
    int32_t d;
    int32_t k;
    int32_t reserved;
    const double *mu;
    const double *logc;
    const double *A;
    const double *knots;
    double kappa;
    /* GSSS_CPD: rigid registration of a 3-D source cloud onto a 3-D target (PointCloud source, pointcloud.py:206-270) or onto a
     * 2-D target after projection (RotationProjection source, :273-293).  The state is a unit quaternion (x, y, z, w), d = 4;
     * log_prob(q) = beta * sum_l w_l logsumexp_{i in kNN(l)} [ log w_i - |y_l - R(q) x_i|^2 / (2 sigma^2) + const ] with the
     * outlier term of CoherentPointDrift when `outlier` (registration.py:47-53, 103-118, 215-250).  k = number of source points. */
    const double *source;   /* [k][3] */
    const double *source_w; /* [k] */
    const double *target;   /* [n_target][target_dim] */
    const double *target_w; /* [n_target] */
    int32_t n_target;
    int32_t target_dim;     /* 3 or 2 */
    int32_t k_nn;           /* neighbours per target point, <= 24 and <= k */
    int32_t outlier;        /* 1: CoherentPointDrift, 0: GaussianMixtureModel */
    double sigma;
    double beta;
    double omega;
    double log_volume;      /* sum_j log(ptp(target[:, j]))  (registration.py:207-213) */
} gsss_target_desc;

/*
 * One launch: advance n_chains chains by n_steps transitions each.
 * Replaces the loop `while len(samples) < n: samples.append(next(self))` of Sampler.sample
 * (mcmc.py:66-69) for all chains at once.
 *
 * Random numbers: counter-based Philox4x32-10 keyed by `seed`; the draws of chain c at
 * step s are a pure function of (seed, chain_offset + c, step_offset + s), so any split of
 * the chains over devices or of the steps over calls reproduces the same numbers
 * (DESIGN.md §3 "Random streams").  On this stream a step draws d normals for the tangent direction as the reference does
 * (mcmc.py:387; Box-Muller pairs formed in single precision: they only set a direction) -- except on S^2 (d = 3), where the uniformly distributed unit tangent is drawn directly as one angle in
 * the tangent plane and one block carries the whole set-up of a step (same law; the two sources below keep the reference's
 * normals and draw order).  The uniform of a try (mcmc.py:395) is ONE 32-bit word of the stream, u = w / 2^32 -- try t is word t % 4
 * of block 1 + ceil(d / 4) + t / 4 ("philox-v3"; theta = lo + (hi - lo) u keeps 32 bits of resolution relative to the bracket
 * however far it has shrunk) -- the threshold uniform (mcmc.py:389) has 53 bits.
 * If replay_dev is non-NULL the draws are read from it instead:
 * per chain `replay_stride` doubles in the order the reference consumes them
 * (d normals, u_threshold, [u_theta0,] u_try, u_try, ... ; next step ...) -- this is how the
 * parity tests reproduce reference chains bit for bit.  A third source, rng_state_dev, is numpy's
 * own PCG64 + ziggurat stream restated on the device: `seed -> chain` exactly as in the reference.
 */
typedef struct gsss_run_args {
    double *state_dev;         /* [d][n_chains] in/out                                             */
    double *samples_dev;       /* NULL or the state after every thin-th step, layout per samples_chain_rows    */
    int64_t *n_reject_dev;     /* [n_chains] or NULL; rejections are ADDED (RejectionSphericalSliceSampler.n_reject) */
    int64_t *n_tries_dev;      /* [n_chains] or NULL; log_prob(y) evaluations are ADDED            */
    int32_t *err_dev;          /* [n_chains] or NULL; GSSS_CHAIN_* bits are OR-ed in               */
    const double *replay_dev;  /* [n_chains][replay_stride] or NULL                                */
    int64_t replay_stride;
    int64_t n_chains;
    int64_t n_steps;
    int64_t thin;              /* >= 1 */
    uint64_t seed;
    uint64_t chain_offset;     /* global id of chain 0 of this call (< 2^48) */
    uint64_t step_offset;      /* global id of step 0 of this call  (< 2^48 - 1) */
    int32_t sampler;           /* GSSS_SHRINK | GSSS_REJECT | GSSS_RWMH | GSSS_HMC | GSSS_INDEP | GSSS_MIX */
    int32_t mode;              /* GSSS_MODE_EXACT | GSSS_MODE_FAST */
    int32_t max_tries;         /* > 0: give up a step after this many proposals */
    int32_t variant;           /* 0 = library's choice; otherwise a kernel variant id (gsss_variant_name) */
    uint64_t *rng_state_dev;   /* [n_chains][4] or NULL.  Non-NULL selects NUMPY'S OWN STREAM instead of Philox: per chain the
                                  PCG64 words (state_hi, state_lo, inc_hi, inc_lo) of np.random.default_rng(seed).bit_generator,
                                  read at entry and written back at exit, so a chain consumes exactly the numbers the reference's
                                  sampler.rng would (mcmc.py:45, 387-395).  GSSS_MODE_EXACT, or GSSS_MODE_FAST for the lane-per-chain shapes
                                  (gsss_variant_name "fast-lane": one wavefront per chain when spread, one lane per chain when packed);
                                  `seed` and the offsets are then unused */
    int64_t samples_chain_rows; /* 0: samples_dev is [n_steps/thin][d][n_chains] (component-major, like state_dev).
                                   R > 0: samples_dev points into a [n_chains][R][d] array -- the reference's (chains, draws,
                                   dims) order -- and this call writes rows 0 .. n_steps/thin-1 of every chain's run of R rows
                                   (offset the pointer by row0*d doubles to continue a run across calls) */
    int32_t placement;         /* lane-per-chain kernels: 0 = library's choice (spread for small ensembles: <= 3072 chains in fast mode, 1536 for curve targets, 2048 in exact mode), 1 = packed
                                  (64 chains per wavefront: throughput), 2 = spread (one chain per wavefront: chains of a
                                  small ensemble do not wait for each other's shrink loops; same numbers either way) */
    int32_t stats_lags;        /* L >= 0: lags of the running autocovariance sums (see stats_dev) */
    double *stats_dev;         /* NULL or [gsss_stats_rows(d, stats_modes, stats_lags, stats_flags)][n_chains]: running statistics of the RETAINED
                                  series (every thin-th state, whether or not samples_dev is given), ADDED to across calls, so that
                                  moments, geodesic step, hopping frequency, mode occupancy and the autocorrelation / IAT / ESS of one
                                  projection need no stored draws (geosss/utils.py:96-134, sphere.py:64-68, scripts/bingham.py:23-25,
                                  scripts/vMF_diagnostics.py:335-342).  Zero it before the first call.  Rows, with T = d (d + 1) / 2 (0 with
                                  GSSS_STATS_NO_SECOND_MOMENT), K = stats_modes, L = stats_lags:
                                    0                count n of retained draws
                                    1 .. d           the last retained draw
                                    .. + d           sum of the draws
                                    .. + T           sum of x_i x_j, i <= j, row-major upper triangle
                                    .. + 1           sum over consecutive draws of arccos(clip(x_t . x_{t-1}, -1, 1))
                                    .. + 1           number of consecutive draws with sign(x_t . h) != sign(x_{t-1} . h)
                                    .. + K           number of draws whose first-largest x . mode_k is k
                                    .. + 2           sum p, sum p^2 of the projection p_t = x_t . w
                                    .. + L           sum_t p_t p_{t-l}, l = 1 .. L
                                    .. + L           ring of the last L values of p (slot t mod L)
                                    .. + L           the first L values of p
                                  Every slice-sampler kernel family accumulates them (lane, lane-group and cooperative layouts;
                                  the group layouts form the second moments through cross-lane reads: d <= 64 with them,
                                  any d with GSSS_STATS_NO_SECOND_MOMENT); GSSS_E_UNSUPPORTED for registration targets */
    const double *stats_dirs_dev; /* [2 + stats_modes][d]: w, h, then the mode directions; required with stats_dev */
    int32_t stats_modes;       /* K >= 0 */
    int32_t n_leapfrog;        /* GSSS_HMC: leapfrog steps per proposal (SphericalHMC(n_steps=10), mcmc.py:243) */
    /* GSSS_RWMH / GSSS_HMC (the baselines of the paper; GSSS_MODE_EXACT, any layout; n_tries / n_reject / stats unused): */
    double *stepsize_dev;      /* [n_chains] in/out: proposal scale / leapfrog stepsize of every chain (mcmc.py:97, 133, 241) */
    int64_t *n_accept_dev;     /* [n_chains] or NULL; accepted proposals are ADDED (MetropolisHastings.n_accept) */
    double *momenta_dev;       /* GSSS_HMC: NULL or [d][n_chains] in/out, the momentum half of the reference's state (mcmc.py:262) */
    int64_t adapt_steps;       /* the first adapt_steps steps of this call multiply the stepsize by 1.02 after an accepted and by
                                  0.98 after a rejected proposal (AdaptiveStepsize.adapt_stepsize during burn-in, mcmc.py:108-115).
                                  Draws per step, in the reference's order: RWMH gamma(d/2), d normals, one uniform; HMC d normals,
                                  one uniform (replay_dev holds the gamma variate itself; the Philox stream uses the norm of d
                                  further normals, the same chi_d law; rng_state_dev restates numpy's gamma).
                                  GSSS_INDEP: d normals, one uniform (the stepsize is adapted like RWMH's, as the reference's class
                                  inherits it, and never used).  GSSS_MIX: one uniform (RWMH iff it is < mixing_probability), then the
                                  draws of the chosen proposal, then the accept uniform; on the Philox stream the two uniforms are the
                                  two halves of block 0 (accept, mix) */
    /* GSSS_MIX (MixtureRWMHIndependenceSampler, mcmc.py:185-234): */
    double mixing_probability; /* alpha: probability of the RWMH kernel */
    int64_t *adapt_left_dev;   /* [n_chains] in/out: RWMH proposals that still adapt the stepsize.  The reference's burn-in counter
                                  only advances on RWMH proposals (mcmc.py:108-115 called from :226-228), so the adaptation of a chain
                                  ends after `burnin` RWMH proposals, not after `burnin` steps; adapt_steps is unused */
    int64_t *n_rwmh_dev;       /* [n_chains] or NULL; RWMH proposals are ADDED (rwmh_counter; indep_counter = steps - that) */
    /* ABI 9 */
    double *momenta_samples_dev; /* GSSS_HMC: NULL or the momentum half of the state after every thin-th step, laid out like
                                    samples_dev (same samples_chain_rows): SphericalHMC.sample(return_momenta=True), mcmc.py:321-332 */
    double *stepsize_trace_dev;  /* GSSS_RWMH / GSSS_INDEP / GSSS_MIX: NULL or [n_steps][n_chains]; entry [s][c] = the stepsize of chain c
                                    after step s if that step made a RWMH proposal, else NaN
                                    (MixtureRWMHIndependenceSampler.rwmh_stepsize_vals, mcmc.py:201, 228) */
    int32_t stats_flags;         /* GSSS_STATS_* bits; changes the row layout of stats_dev (gsss_stats_rows takes the same flags) */
    int32_t reserved0;
} gsss_run_args;

int gsss_abi_version(void);
const char *gsss_last_error(void);

/* sha256 (hex) over the kernel sources this library was BUILT from (the .h, .hip and .inc files of geosss_amd/csrc and this header, by name:
 * geosss_amd/build.py source_digest), "unknown" for a build that did not pass it.  Profiles are bound to the binary through it:
 * bench.py quotes the committed rocprofv3 counters only for the digest of the loaded library.  Nothing in the reference. */
const char *gsss_source_digest(void);

/* number of visible gfx950 devices (0 if none); does not fail */
int gsss_device_count(void);

/* distributions.py ctor twins: copy the parameters to `device` */
int gsss_target_create(const gsss_target_desc *desc, int device, gsss_target **out);
/* MixtureModel(components, weights) with any of the kinds above as components (GSSS_MIXTURE): each component an ordinary
 * descriptor of kind GSSS_VMF_MIXTURE, GSSS_BINGHAM or GSSS_CURVE_VMF, all of one d; log_weights[c] = log w_c, -inf for a zero
 * weight.  Nested mixtures are flattened by the caller.  GSSS_E_INVALID: components of different d, an unknown kind or a NaN /
 * +inf weight; GSSS_E_UNSUPPORTED: a GSSS_CPD component, more than 16 components or 2^20 parameter rows (gsss_last_error says
 * which).  The handle serves every call a target handle serves. */
int gsss_target_create_mixture(const gsss_target_desc *components, int32_t n_components, const double *log_weights, int device,
                               gsss_target **out);
/* A batch of targets sampled in ONE launch: n_targets descriptors of one family and one shape -- all GSSS_VMF_MIXTURE of one d and
 * one K, or all GSSS_BINGHAM of one d, all with or all without the linear term b -- packed as gsss_target_create packs each, at an
 * equal stride in one device allocation.  Target t owns the chains [t m, (t + 1) m) in GLOBAL chain ids, m = chains_per_target:
 * chain c of a gsss_run call belongs to target (chain_offset + c) / m, so the rule lives in the handle and gsss_run_args is as it
 * was.  A call covers whole targets: chain_offset and n_chains are multiples of m (any run of targets may be launched, e.g. a
 * shard of the batch).  Samplers GSSS_SHRINK / GSSS_REJECT on the library (Philox) stream; GSSS_MODE_EXACT in every layout and
 * placement, GSSS_MODE_FAST one chain per lane at d = 3 .. 16 (screened or all-double; placement is ignored there).  Chains
 * are the ones n_targets separate handles give, with the same seed and chain_offset = t m, bit for bit -- except that Bingham
 * members with a diagonal A run the diagonal fast kernels only if EVERY member's A is diagonal.  The screen's scale is the
 * maximum over the members.  GSSS_E_UNSUPPORTED (gsss_last_error says which): another kind than the two above, members of
 * different kind, d, K or b-ness; from gsss_run: another sampler, replay_dev, rng_state_dev, stats_dev, a chain_offset or n_chains
 * that is no multiple of m or reaches past the last target, a shape without a batch fast kernel in GSSS_MODE_FAST; from
 * gsss_logprob / gsss_gradient always (evaluate the members' own handles, or all of them with gsss_batch_logprob /
 * gsss_batch_gradient).  gsss_kernel_name names the batch builds
 * ("run_kernel<lane3, VmfMixture, batch>", "screened_kernel<5, ScreenBingham<5>, batch>", ...). */
int gsss_target_create_batch(const gsss_target_desc *targets, int32_t n_targets, int64_t chains_per_target, int device,
                             gsss_target **out);
/* The vector layout (an id of gsss_variant_name's list) the exact kernels run dimension d in: the layout a user module for d must
 * be compiled for (geosss_amd/usertarget.py passes it as -DGSSS_USER_VEC).  < 0: no layout covers d. */
int gsss_exact_layout(int32_t d);
/* A user-defined target (GSSS_USER).  `table` is what the compiled module's one export, gsss_user_module_table, returns: its
 * launchers (geosss_amd/csrc/gsss_user_target.h); the module is linked against this library and must stay loaded while the handle
 * lives.  params[n_params] are copied to `device` and handed, read-only, to the module's gsss_user_log_prob / gsss_user_gradient.
 * GSSS_E_UNSUPPORTED (with the reason in gsss_last_error): a module built against another ABI or from other kernel sources than
 * this library (gsss_source_digest), or for another layout than gsss_exact_layout(d).  gsss_run then takes GSSS_MODE_EXACT only
 * and no other variant than that layout; gsss_gradient and GSSS_HMC need a module with a gradient. */
int gsss_target_create_user(const void *table, int32_t d, const double *params, int64_t n_params, int device, gsss_target **out);
int gsss_target_destroy(gsss_target *t);
int gsss_target_dim(const gsss_target *t);

/* Distribution.log_prob for n points (distributions.py:84-86, :156-157, :218-221, :272-275).
 * x_dev is ROW-major [n][d] (numpy's natural layout for pdf.log_prob(samples)). */
int gsss_logprob(const gsss_target *t, const double *x_dev, int64_t n, double *out_dev, void *stream);

/* Distribution.gradient for n points (distributions.py:88-89 Bingham 2 A x -- also what BinghamFisher inherits --, :159-160
 * vMF mu, :223-227 mixture, :277-278 curve kappa * nearest; registration.py:55-60 the pose score's gradient with respect to the
 * quaternion): the functions the spherical HMC kernel evaluates (GSSS_HMC), for rows of x_dev [n][d] -> grad_dev [n][d]. */
int gsss_gradient(const gsss_target *t, const double *x_dev, int64_t n, double *grad_dev, void *stream);

/* The sampler (see gsss_run_args). */
int gsss_run(const gsss_target *t, const gsss_run_args *args, void *stream);

/* What the calling thread's last gsss_run launched, for logs and benches: the grid of the sampler kernel and the slice length if
 * the launch was SLICED (kernels whose chunks of chains do not fit the chip at once run one workgroup per (chunk, slice of steps)
 * and hand the chunk's state from slice to slice through HBM: (16 d + 32) / slice_steps more bytes per chain-step than an unsliced
 * launch; same results bit for bit; GSSS_SLICE_STEPS in the environment sets the length, 0 turns it off; a launch is cut into at
 * most 64 slices per chunk -- long launches get longer slices, n_steps = 10^6 -> 15 680 steps --, so the chain of hand-overs a
 * workgroup may wait on stays short for any n_steps < 2^31).  slice_steps 0:
 * unsliced; grid 0: a kernel family that never slices.  sliced_fraction: the share of the chains that ran sliced.
 * The lane kernels never slice their full rounds of workgroups.  With GSSS_SLICE_STEPS unset they run a launch whose chunks are
 * no whole number of rounds by a PIECE PLAN (gsss_piece_plan): every resident workgroup slot gets the same number of steps and a
 * chunk is split at most once, into a head and a tail.  Such a launch reports grid = the number of pieces, sliced_fraction =
 * split chunks / chunks and slice_steps = ceil(n_steps / 2): each split chunk is handed over once, and that is what this slice
 * length prices in the formula above.  GSSS_PIECE_PLAN=0, or GSSS_SLICE_STEPS=N > 0, selects uniform slices of a small last
 * round instead (128 steps, or N), reported as such.  Any pointer may be NULL.  There is nothing in the reference this replaces. */
int gsss_last_launch(int64_t *grid_out, int32_t *slice_steps_out, double *sliced_fraction_out);

/* The piece plan of a lane-kernel launch of n_chunks chunks of chains x n_steps steps on `resident` workgroup slots: the chunks
 * laid end to end and cut into `resident` slots of ceil(n_chunks n_steps / resident) steps, boundaries moved by less than 32
 * steps so that no part of a split chunk is shorter than 32.  table_out: NULL or `capacity` entries of four int32 -- chunk, first
 * step, steps, kind (0 a whole chunk; 1 the head [0, b) of a split chunk, at the start of a slot; 2 its tail [b, n_steps), at the
 * end of the slot before) -- in the order workgroups take them: by planned start within the slot, ties by slot, a head always
 * before its tail.  Returns the number of pieces; 0: no plan (n_chunks <= resident, a whole number of rounds, or n_steps < 256);
 * GSSS_E_INVALID for arguments < 1 or a table that does not fit the buffer.  A pure host function: no device is needed.  There
 * is nothing in the reference this replaces. */
int64_t gsss_piece_plan(int64_t n_chunks, int64_t resident, int64_t n_steps, int32_t *table_out, int64_t capacity);

/* The fast-mode launch plan of a batch of n_targets members (kind, d, k, has_b) with m chains each: chains a workgroup takes, the
 * most targets it stages, the grid, and lanes that carry a chain / lanes launched (chains / (grid x chains a workgroup takes)).
 * k: the components of a vMF mixture; ignored for GSSS_BINGHAM, like has_b -- one plan holds for every launch of a shape, screened
 * or all-double, diagonal or dense (its LDS is budgeted for the widest rows).  m a multiple of 256: one target per workgroup, 256
 * chains; otherwise a workgroup takes a run of consecutive chains and stages every target the run touches, as many as the LDS
 * holds without costing the kernel a resident workgroup.  gsss_run launches what this reports.  A pure host function: no device
 * is needed.  Any output pointer may be NULL.  GSSS_E_UNSUPPORTED where the batch has no fast kernel.  There is nothing in the
 * reference this replaces. */
int gsss_batch_plan(int32_t kind, int32_t d, int32_t k, int32_t has_b, int64_t n_targets, int64_t m,
                    int32_t *chains_per_workgroup, int32_t *targets_per_workgroup, int64_t *grid, double *lane_use);

/* Number of rows of gsss_run_args.stats_dev for dimension d, K modes, L lags and the GSSS_STATS_* flags (< 0: bad argument). */
int64_t gsss_stats_rows(int32_t d, int32_t n_modes, int32_t n_lags, int32_t flags);

/* Per-TARGET moments of a block of retained draws, for ensembles in which target t owns the chains [t m, (t + 1) m),
 * m = chains_per_target (a gsss_target_create_batch handle's chains; m = n_chains pools one target's whole ensemble): what
 * gsss_run_args.stats_dev cannot give a batch.  The block is what gsss_run wrote to samples_dev -- component-major
 * [n_rows][d][n_chains] (samples_chain_rows 0) or rows 0 .. n_rows - 1 of every chain's run of samples_chain_rows rows in a
 * [n_chains][samples_chain_rows][d] array (offset the pointer by row0 * d doubles, as for gsss_run) -- read once, by a kernel of its
 * own beside the sampler, so it serves every kernel family, mode and dimension.  Any m >= 1 that divides n_chains.
 * acc_dev [n_chains / m][gsss_moments_rows(d, flags)], ADDED to (zero it before the first block), per target:
 *     0                count of draws: m * n_rows per call
 *     1 .. d           sum of x_j
 *     .. + T           sum of x_i x_j, i <= j, row-major upper triangle (the order of stats_dev), T = d (d + 1) / 2, d <= 16;
 *                      with GSSS_MOMENTS_DIAG the d sums of x_j^2 instead (any d)
 * chain_sum_dev: NULL or [d][n_chains], ADDED to: every chain's sum of its rows of the block -- divided by the draws they are the
 * chain means, whose per-target sums and sums of squares (the between-chain variance of R-hat) are one more call of this function
 * with n_rows = 1 and GSSS_MOMENTS_DIAG (geosss_amd/diagnostics.py from_target_moments).
 * No floating-point atomics: the order of every sum is fixed by the arguments, so a call gives the same bits every time.
 * GSSS_E_INVALID: d < 2, m < 1, n_chains no multiple of m, a negative row count, 0 < samples_chain_rows < n_rows, a NULL
 * samples_dev / acc_dev, unknown flags; GSSS_E_UNSUPPORTED: the full triangle at d > 16 (gsss_moments_rows returns the same
 * codes) -- all of them before the device is touched.  n_rows = 0 does nothing.  The reference computes such summaries on the host
 * from stored chains (scripts/bingham.py, scripts/vMF_diagnostics.py); nothing there works without the stored draws. */
#define GSSS_MOMENTS_DIAG 1
int64_t gsss_moments_rows(int32_t d, int32_t flags);
int gsss_target_moments(const double *samples_dev, int64_t n_rows, int64_t n_chains, int32_t d, int64_t samples_chain_rows,
                        int64_t chains_per_target, int32_t flags, double *acc_dev, double *chain_sum_dev, int device, void *stream);

/* Distribution.log_prob / .gradient of EVERY member of a gsss_target_create_batch handle in one launch (the batch counterpart of
 * gsss_logprob / gsss_gradient, which keep refusing a batch).  x_dev is row-major [M][n_per_target][d]: member t evaluates its own
 * rows, out_dev [M][n_per_target], grad_dev [M][n_per_target][d].  A workgroup serves one target, in the vector layout and with
 * the target policy gsss_logprob uses for the shape, so every value is the member's own gsss_logprob / gsss_gradient value bit for
 * bit (a batch that mixes diagonal and dense Bingham members included: these kernels do not read the flag).  n_per_target = 0
 * does nothing.  GSSS_E_INVALID: a NULL handle, a negative count, NULL pointers with n_per_target > 0; GSSS_E_UNSUPPORTED: a handle
 * that is no batch, more workgroups (M x ceil(n_per_target / points per workgroup)) than a grid holds -- all before the device
 * is touched.  The reference evaluates pdf.log_prob(samples) per target on the host. */
int gsss_batch_logprob(const gsss_target *t, const double *x_dev, int64_t n_per_target, double *out_dev, void *stream);
int gsss_batch_gradient(const gsss_target *t, const double *x_dev, int64_t n_per_target, double *grad_dev, void *stream);
/* The same values for a block of draws where gsss_run left it: samples_dev is component-major [n_rows][d][n_chains], chain 0 of
 * the block being the first chain of target `target0` of the handle; m = the handle's chains_per_target, so the block covers the
 * targets target0 .. target0 + n_chains / m - 1 and chain c belongs to target target0 + c / m.  out_dev [n_rows][n_chains].
 * GSSS_E_INVALID: a NULL handle, negative counts, n_chains no multiple of m, a target range that reaches past the last member,
 * NULL pointers with a non-empty block; GSSS_E_UNSUPPORTED as above.  An empty block does nothing. */
int gsss_batch_logprob_draws(const gsss_target *t, const double *samples_dev, int64_t n_rows, int64_t n_chains, int64_t target0,
                             double *out_dev, void *stream);
/* gsss_target_moments for ONE scalar per draw (the log-density trace): values_dev [n_rows][n_chains], target t owning the chains
 * [t m, (t + 1) m), m = chains_per_target.  acc_dev [n_chains / m][3], ADDED to: count of draws, sum v, sum v^2; chain_sum_dev NULL
 * or [n_chains], ADDED to: every chain's sum of its rows.  The same kernels, the same fixed summation order and no atomics: a
 * call gives the same bits every time.  (gsss_target_moments itself keeps refusing d < 2: a point on a sphere has two
 * coordinates at least.)  GSSS_E_INVALID: negative counts, m < 1, n_chains no multiple of m, a NULL values_dev / acc_dev with a
 * non-empty block -- before the device is touched.  n_rows = 0 or n_chains = 0 does nothing. */
int gsss_scalar_moments(const double *values_dev, int64_t n_rows, int64_t n_chains, int64_t chains_per_target, double *acc_dev,
                        double *chain_sum_dev, int device, void *stream);

/* Per-TARGET lagged products of retained draws, streamed: what the within-chain autocorrelation, its integrated autocorrelation
 * time and N / IAT need (geosss_amd/diagnostics.py from_target_autocov), for ensembles in which target t owns the chains
 * [t m, (t + 1) m), m = chains_per_target -- the stats_dev lag rows, which a batch refuses, by a kernel of its own beside the
 * sampler, so it serves every kernel family, mode and dimension.  The series are the d coordinates of a draw (d >= 1: a scalar
 * series such as the log-density trace is d = 1).  ring_dev is component-major [ring_rows][d][n_chains], the layout gsss_run writes
 * to samples_dev.  The block is the rows first_row .. first_row + n_rows - 1 (it does not wrap); the n_hist <= n_lags draws that
 * precede it are the rows (first_row - 1 - i) mod ring_rows, i = 0 .. n_hist - 1: factors only, never leading terms.  Who holds
 * all the draws passes ring_rows = n_rows, first_row = 0, n_hist = 0; who streams windows gives the ring n_lags + window rows and
 * never copies history.
 * acc_dev [n_chains / m][d][n_lags + 1][3], ADDED to (zero it before the first block): per target t, series j and lag l, over the
 * target's chains c and the rows r of the block whose partner r - l lies in the block or in its history,
 *     0   C = sum x_{c,r,j} x_{c,r-l,j}      the lagged products
 *     1   P = sum x_{c,r,j}                  the sum of the leading factors
 *     2   Q = sum x_{c,r-l,j}                the sum of the lagging factors
 * so that successive calls over successive blocks of one series give the sums over the whole series, its ends exact: with
 * mu = P_0 / (m n) and k_l = m (n - l) pairs, cov_l = (C_l - mu (P_l + Q_l)) / k_l + mu^2 is the direct estimator of
 * utils.acf (geosss/utils.py:96-110) centred on the target's pooled mean.  gsss_autocov_rows(d, n_lags) = d (n_lags + 1) 3, the
 * doubles per target.
 * No floating-point atomics: the order of every sum is fixed by the arguments, so a call gives the same bits every time.
 * GSSS_E_INVALID: d < 1, m < 1, n_chains no multiple of m, n_lags < 1, a negative count, first_row + n_rows > ring_rows,
 * n_hist > n_lags or > ring_rows - n_rows, a NULL ring_dev / acc_dev with a non-empty block; GSSS_E_UNSUPPORTED: n_lags > 64
 * (gsss_autocov_rows returns the same codes) -- all of them before the device is touched.  n_rows = 0 does nothing.  The
 * reference computes acf / IAT / n_eff on the host from one stored chain (geosss/utils.py:96-134). */
int64_t gsss_autocov_rows(int32_t d, int32_t n_lags);
int gsss_target_autocov(const double *ring_dev, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist,
                        int64_t n_chains, int32_t d, int64_t chains_per_target, int32_t n_lags, double *acc_dev, int device,
                        void *stream);

/* Per-TARGET mixing metrics of retained draws, streamed: the mean geodesic step between consecutive draws (sphere.py:64-68), the
 * hopping frequency across a direction's equator (scripts/bingham.py:23-25) and the mode occupancy (scripts/vMF_diagnostics.py:
 * 335-342), for ensembles in which target t owns the chains [t m, (t + 1) m), m = chains_per_target, and EVERY TARGET HAS ITS OWN
 * DIRECTIONS -- the stats_dev step, hop and mode rows, which take one set of directions and which a batch refuses, by a kernel of
 * its own beside the sampler, so it serves every kernel family, mode and dimension.  ring_dev is component-major
 * [ring_rows][d][n_chains] with the block semantics of gsss_target_autocov: the block is the rows first_row .. first_row + n_rows
 * - 1 (it does not wrap); with n_hist = 1 the draw that precedes it is the row (first_row - 1) mod ring_rows, read where it lies.
 * A pair (r, r - 1) counts in the call whose block holds r.
 * dirs_dev [n_chains / m][1 + n_modes][d], per target t: the hop direction h_t, then its K = n_modes mode directions (K = 0 .. 16).
 * step_dev [n_chains / m][2], ADDED to: sum theta and sum theta^2 over the target's pairs, theta = acos(clamp(x_r . x_{r-1}, -1,
 * 1)), the product a chain of fused multiply-adds in component order (the arithmetic of the stats_dev row).
 * count_dev [n_chains / m][gsss_mixing_rows(n_modes, flags)], int64, ADDED to, per target:
 *     0                draws
 *     1                pairs
 *     2                hops: pairs with sign(x_r . h_t) != sign(x_{r-1} . h_t), the three-valued sign of np.sign
 *     3 .. 2 + K       draws whose mode is k: the FIRST maximum over k of x . mode_k, like np.argmax
 *     .. + K K         with GSSS_MIXING_TRANSITIONS: pairs by [mode of x_{r-1}][mode of x_r]
 * The two floating-point sums have an order fixed by the arguments and use no floating-point atomics: a call gives the same bits
 * every time.  The counters are integers, added with integer atomics -- the same in any order.
 * GSSS_E_INVALID: d < 2, m < 1, n_chains no multiple of m, a negative count, first_row + n_rows > ring_rows, n_hist > 1 or
 * > ring_rows - n_rows, n_modes < 0, unknown flags, a NULL ring_dev / dirs_dev / step_dev / count_dev with a non-empty block;
 * GSSS_E_UNSUPPORTED: n_modes > 16 (gsss_mixing_rows returns the same codes) -- all of them before the device is touched.
 * n_rows = 0 does nothing.  The reference computes these from one stored chain on the host. */
#define GSSS_MIXING_TRANSITIONS 1
int64_t gsss_mixing_rows(int32_t n_modes, int32_t flags);
int gsss_target_mixing(const double *ring_dev, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist,
                       int64_t n_chains, int32_t d, int64_t chains_per_target, const double *dirs_dev, int32_t n_modes,
                       int32_t flags, double *step_dev, int64_t *count_dev, int device, void *stream);

/* Per-TARGET marginal histograms of retained draws, streamed: the shape of every posterior of a batch -- the histogram of u^T x
 * the reference draws for the Bingham experiment (scripts/Bingham.ipynb), the coordinate marginals of scripts/vMF_diagnostics.py
 * and curve_3d.py::marginal_distribution_plot, the histogram of geodesic steps of curve_3d.py::geodesic_distance_plot -- for
 * ensembles in which target t owns the chains [t m, (t + 1) m), m = chains_per_target, and EVERY TARGET HAS ITS OWN DIRECTIONS, by
 * a kernel of its own beside the sampler, so it serves every kernel family, mode and dimension.  ring_dev is component-major
 * [ring_rows][d][n_chains] with the block semantics of gsss_target_mixing: the block is the rows first_row .. first_row + n_rows
 * - 1 (it does not wrap); with n_hist = 1 the draw that precedes it is the row (first_row - 1) mod ring_rows, read where it lies.
 * A pair (r, r - 1) counts in the call whose block holds r.  The history serves the step series alone: without
 * GSSS_MARGINALS_STEP n_hist = 1 is accepted and ignored, the row is not read.
 * dirs_dev [n_chains / m][n_dirs][d], per target t its P = n_dirs directions v_{t,p} (P = 0 .. 32); they need not be unit vectors.
 * count_dev [n_chains / m][S][n_bins], int64, ADDED to, S = gsss_marginal_rows / n_bins = P + (GSSS_MARGINALS_STEP ? 1 : 0), B = n_bins:
 *     series p < P     per draw of the target: u = sum_j x_j v_{t,p,j}, a chain of fused multiply-adds in component order from
 *                      0.0 (the arithmetic of gsss_target_mixing's x . h); t = (u + 1.0) * (0.5 * B); bin 0 if t < 0, else
 *                      min(B - 1, (int)t): B equal bins over [-1, 1], what lies outside counted in the first and the last
 *     series P         with GSSS_MARGINALS_STEP, per pair: theta = acos(fmin(fmax(dot, -1), 1)), dot = x_r . x_{r-1} the chain of
 *                      fused multiply-adds of gsss_target_mixing; t = theta * scale, scale = (double)B / M_PI formed once on
 *                      the host; bin min(B - 1, (int)t): B equal bins over [0, pi]
 * A NaN u is counted in no bin, nor is the step of a pair whose dot is NaN (the clamp would turn it into pi).
 * No floating-point sums are kept.  The counters are integers added with integer atomics -- 32-bit in LDS, then one 64-bit add
 * to count_dev per non-zero counter of a workgroup --: the same result in any order, and successive calls over successive blocks
 * of a series give the counts of the whole series.
 * GSSS_E_INVALID: d < 2, m < 1, n_chains no multiple of m, a negative count, first_row + n_rows > ring_rows, n_hist > 1 or
 * > ring_rows - n_rows, n_dirs < 0, n_dirs = 0 without GSSS_MARGINALS_STEP, n_bins < 2, unknown flags, a NULL ring_dev / count_dev
 * (dirs_dev with n_dirs > 0) with a non-empty block; GSSS_E_UNSUPPORTED: n_dirs > 32, n_bins > 1024, S n_bins > 8192 (32 KB of
 * 32-bit LDS counters per target; gsss_marginal_rows returns the same codes for the three arguments it takes), n_rows > 2^23 (a
 * workgroup's 32-bit counter takes 256 lanes x 2^23 rows) -- all of them before the device is touched.  n_rows = 0 does nothing.
 * The reference takes np.histogram of one stored chain on the host. */
#define GSSS_MARGINALS_STEP 1
int64_t gsss_marginal_rows(int32_t n_dirs, int32_t n_bins, int32_t flags);
int gsss_target_marginals(const double *ring_dev, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist,
                          int64_t n_chains, int32_t d, int64_t chains_per_target, const double *dirs_dev, int32_t n_dirs,
                          int32_t n_bins, int32_t flags, int64_t *count_dev, int device, void *stream);

/* Replica exchange (parallel tempering) along ladders of members of a gsss_target_create_batch handle: ONE sweep of one parity
 * over the chains of a launch.  state_dev is component-major [d][n_chains], chain 0 being the first chain of member `target0`;
 * m = the handle's chains_per_target.  The n_chains / m members form ladders of `ladder` consecutive members; a sweep of parity p
 * pairs member a = g ladder + 2 k + p of the call with b = a + 1 for every k with 2 k + p + 1 < ladder, the others sit out.
 * Chain i of a (column c_a = a m + i) is paired with chain i of b; with l_t member t's log-density (the value of
 * gsss_batch_logprob, bit for bit), in double precision and in this order,
 *     log alpha = (l_a(x_b) - l_a(x_a)) + (l_b(x_a) - l_b(x_b)),
 * and the two columns are swapped iff all four values are finite, err_dev is 0 for both chains, and log(u) < log alpha, u the
 * first 53-bit uniform of Philox block 0xFFFFFFFF at (seed, chain = chain_offset + c_a, step) -- a block no sampler draws.  u = 0
 * swaps.  An exchange between two members with their own densities leaves the product law of the batch invariant whatever the
 * members are.  Only the state columns move, and with them the entries of replica_dev [n_chains] if given; counters and err stay
 * with the slot.  scratch_dev holds gsss_exchange_scratch_doubles(n_chains) = 2 n_chains doubles (the four values of every pair).
 * counts_dev, if given, is int64 [2][n_chains / m], ADDED to: per lower member a, the pairs of chains tried (m a sweep it takes
 * part in, refused pairs included) and the pairs swapped.  log_alpha_out, if given, is [n_chains] and receives log alpha at c_a.
 * Two launches on `stream`: the members' evaluation in the layout gsss_logprob uses for the shape, then the swap.
 * GSSS_E_INVALID: ladder < 2, parity outside {0, 1}, negative counts, a target0 that is no multiple of ladder, a NULL handle,
 * n_chains no multiple of m ladder, a range that reaches past the last member, chain ids or a step beyond the stream's 48 bits,
 * a NULL state_dev / err_dev / scratch_dev with n_chains > 0; GSSS_E_UNSUPPORTED: a handle that is no batch, more workgroups than
 * a grid holds -- all before the device is touched.  n_chains = 0 does nothing.  The reference has no replica exchange. */
int64_t gsss_exchange_scratch_doubles(int64_t n_chains);
int gsss_batch_exchange(const gsss_target *batch, double *state_dev, const int32_t *err_dev, int64_t n_chains, int64_t target0,
                        int32_t ladder, int32_t parity, uint64_t seed, uint64_t chain_offset, uint64_t step, double *scratch_dev,
                        int64_t *replica_dev, int64_t *counts_dev, double *log_alpha_out, void *stream);

/* Log normalising constants along ladders of members of a gsss_target_create_batch handle: the sums from which the ratios
 * Z_a / Z_b of neighbouring rungs follow, over a block of retained rows, without stored draws.  samples_dev is component-major
 * [n_rows][d][n_chains] (as gsss_batch_logprob_draws takes it), chain 0 being the first chain of member `target0`; m = the
 * handle's chains_per_target.  The n_chains / m members form ladders of `ladder` consecutive members, rung r colder than rung
 * r + 1; pair (a, b = a + 1) exists for every a that is not the last rung of its ladder.  With l_t member t's log-density (the
 * value of gsss_batch_logprob, bit for bit) and x_a, x_b chain i of a and of b at one row,
 *     u = l_a(x_b) - l_b(x_b)   (a draw of the hotter member: E_b[exp u] = Z_a / Z_b)
 *     v = l_b(x_a) - l_a(x_a)   (a draw of the colder member: E_a[exp v] = Z_b / Z_a)
 * and the row is used iff all four log-densities are finite, else skipped.
 * acc_dev [(n_chains / m / ladder) (ladder - 1)][m][10], CONTINUED (zero it before the first block): per pair and chain i
 *     0      draws used
 *     1, 2   M_u = the running maximum of u, and S_u = sum exp(u - M_u):  log sum exp(u) = M_u + log S_u
 *     3, 4   sum u, sum u^2
 *     5, 6   M_v, S_v
 *     7, 8   sum v, sum v^2
 *     9      draws skipped
 * (M, S) per used draw, in row order:  M' = max(M, u);  S' = S exp(M - M') + exp(u - M'),  from M = -inf, S = 0; the first used
 * draw (slot 0 is zero) sets M = u, S = 1 directly, so that no -inf - (-inf) is formed and the values of slots 1, 2, 5, 6 before
 * it are not read.  A pair-chain's slots depend on its own rows in their order alone: a block of 5 rows gives the bits of the
 * same rows in calls of 3 and 2.  No atomics: the order of every sum is fixed by the arguments.
 * scratch_dev holds gsss_ladder_scratch_doubles(n_rows, n_chains) = 3 n_rows n_chains doubles (every member's values at its own
 * and at its two neighbours' columns); gsss_ladder_acc_doubles(n_chains, m, ladder) = (n_chains / m / ladder) (ladder - 1) m 10.
 * Two launches on `stream`: the members' evaluation in the layout gsss_logprob uses for the shape -- each member's rows staged
 * once for the whole block --, then the fold.
 * GSSS_E_INVALID: ladder < 2, negative counts, a target0 that is no multiple of ladder, a NULL handle, n_chains no multiple of
 * m ladder, a range that reaches past the last member, a NULL samples_dev / scratch_dev / acc_dev with a non-empty block (the two
 * size functions: a negative count, m < 1, ladder < 2, n_chains no multiple of m ladder, a size beyond 63 bits);
 * GSSS_E_UNSUPPORTED: a handle that is no batch, more workgroups than a grid holds -- all before the device is touched.
 * n_rows = 0 or n_chains = 0 does nothing.  The reference has no such estimate. */
int64_t gsss_ladder_scratch_doubles(int64_t n_rows, int64_t n_chains);
int64_t gsss_ladder_acc_doubles(int64_t n_chains, int64_t chains_per_target, int32_t ladder);
int gsss_batch_ladder(const gsss_target *batch, const double *samples_dev, int64_t n_rows, int64_t n_chains, int64_t target0,
                      int32_t ladder, double *scratch_dev, double *acc_dev, void *stream);

/* 1 if gsss_run accepts `mode` for this target's shape (fast mode is built for the shapes listed in
 * geosss_amd/csrc/gsss_fast_*.hip), else 0. */
int gsss_mode_supported(const gsss_target *t, int32_t mode);

/* Names the kernel variant gsss_run would use / the variants available, for logs and benches. */
const char *gsss_variant_name(const gsss_target *t, int32_t mode, int32_t variant);
/* The kernel instantiation gsss_run launches for this target (what a rocprofv3 kernel trace shows, template arguments
 * abbreviated), e.g. "fast_kernel<3, FastVmf<3, 3>>"; placement as in gsss_run_args (2 = spread).  "" if unsupported.
 * The string lives in thread-local storage until the thread's next call. */
const char *gsss_kernel_name(const gsss_target *t, int32_t mode, int32_t variant, int32_t placement);

/* sphere.sample_sphere twin (sphere.py:39-50): n uniform points on S^{d-1}, component-major,
 * from the reserved step id of the RNG stream. */
int gsss_sample_sphere(uint64_t seed, uint64_t chain_offset, int64_t n, int32_t d, double *state_dev, int device,
                       void *stream);

/* Verification of the library stream's set-up on S^2 (d = 3).  The reference draws z ~ N(0, I_3) and takes
 * u = sphere.spherical_projection(z, x) (mcmc.py:387, sphere.py:29-33): a uniformly distributed unit tangent at x.  The Philox
 * stream draws that tangent directly from ONE 32-bit word w: u = cos(phi) b1 + sin(phi) b2, phi = 2 pi w / 2^32, in a fixed
 * orthonormal basis (b1, b2) of the tangent plane at n = x / |x|.  This entry point evaluates exactly what the sampler kernels
 * evaluate there, for n points: x_dev [n][3] states (any norm), w_dev [n] angle words -> out_dev [n][12] = n, b1, b2, u.
 * table_driven != 0: the sincos of the throughput kernels (screened / fast / one-wavefront), 0: the exact kernels'.
 * tests/test_hip_tangent.py holds it to the reference's own tangents (tests/golden/tangent_kat.npz). */
int gsss_tangent_s2(const double *x_dev, const uint32_t *w_dev, int64_t n, int32_t table_driven, double *out_dev, int device,
                    void *stream);

/* Verification of the single-precision screen.  In fast mode four tries out of five are decided on the hardware's
 * single-precision sin / cos / 2^x / log2 / sqrt with an error margin; the decision protected is
 * mcmc.py:397 `if p(y) > threshold`, and it is the double-precision one only if each instruction's worst-case error is inside the
 * constant the margin is built from.  gsss_screen_constants: out[0..5) = the constants compiled into the library --
 * kSinCosErr32 (|v_sin/cos_f32(fl32(theta / 2 pi)) - sin/cos(theta)|, |theta| <= 2 pi, argument rounding included), kExp2Err32
 * (relative, normal results), kLog2Err32 (log2 of a double's mantissa, its rounding to single included), kSqrtRelErr32, 2^-24.
 * gsss_f32_error_sweep: evaluates EVERY float of an instruction's argument range on `device` against double precision
 * (synchronous; ~1 s) and writes four maxima to out_host:
 *   which 0  sin / cos of t revolutions, every |t| <= 1:   [0] sin, [1] cos at the float; [2], [3] with 2 pi x half an ulp of t added
 *                                                           (any theta whose revolutions round to t) -- to hold against kSinCosErr32
 *   which 1  2^x, every finite float:                       [0] relative error on normal results (kExp2Err32), [1] absolute error where
 *                                                           the result is below the normals, [2] overflows not returned as +inf (0)
 *   which 2  log2 x, every float of [0.5, 2]:               [0] at the float, [1] on [0.5, 1] with half an ulp / (x ln 2) added (kLog2Err32)
 *   which 3  sqrt x, every positive normal float:           [0] relative error (kSqrtRelErr32)
 * n_swept_out (may be NULL): how many floats were evaluated.  tests/test_hip_screen_bounds.py.  Nothing in the reference. */
int gsss_screen_constants(double *out, int32_t n);
int gsss_f32_error_sweep(int32_t which, double *out_host, uint64_t *n_swept_out, int device, void *stream);

/* Layout changes between numpy's row-major arrays and the component-major device layout.
 *   gsss_rows_to_components: in [n][d]            -> out [d][n]
 *   gsss_components_to_rows: in [d][n]            -> out [n][d]
 *   gsss_samples_to_chains:  in [n_keep][d][n]    -> out [n][n_keep][d]   (chains, draws, dims) */
int gsss_rows_to_components(const double *in_dev, double *out_dev, int64_t n, int32_t d, int device, void *stream);
int gsss_components_to_rows(const double *in_dev, double *out_dev, int64_t n, int32_t d, int device, void *stream);
int gsss_samples_to_chains(const double *in_dev, double *out_dev, int64_t n, int64_t n_keep, int32_t d, int device,
                           void *stream);

/* Minimal memory / stream helpers for callers without another HIP front-end (ctypes-only hosts). */
int gsss_malloc(void **out_dev, size_t bytes, int device);
int gsss_free(void *p_dev, int device);
int gsss_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, int device, void *stream);
int gsss_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, int device, void *stream);
int gsss_memset(void *dst_dev, int value, size_t bytes, int device, void *stream);
/* The return path of Sampler.sample (mcmc.py:55-77 returns an ndarray; its consumers read it on the host, scripts/curve_vMF.py:119-120)
 * at PCIe speed: page-locked host memory the device copies into directly (a copy into pageable memory is staged by the driver at
 * a sixth of the link's rate), and a device-to-host copy that is only ENQUEUED on `stream`, so that the copy of one block of chains
 * overlaps the kernel of the next (geosss_amd/mcmc.py sample).  The buffer must stay alive until the stream has drained. */
int gsss_malloc_host(void **out_host, size_t bytes, int device);
int gsss_free_host(void *p_host);
/* ... or the caller's own pages, page-locked where they lie (hipHostRegister): locking pages that were TOUCHED before costs 4 ms for
 * 2.4 GB, locking untouched ones 105 ms -- the page faults, taken one by one inside the call (gsss_malloc_host: 107 ms); a host with
 * several cores touches them in parallel first (11 ms on 16 threads; tools/microbench_pinning.py, geosss_amd/_pinned.py). */
int gsss_host_register(void *p_host, size_t bytes, int device);
int gsss_host_unregister(void *p_host);
int gsss_memcpy_d2h_async(void *dst_host, const void *src_dev, size_t bytes, int device, void *stream);
int gsss_stream_synchronize(int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSSS_H */
