// gsss_capi.hip -- the extern "C" surface declared in include/gsss.h, plus the layout and
// initial-state kernels.  No torch types, no exceptions across the boundary.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "gsss_batch.h"
#include "gsss_batch_logprob.h"
#include "gsss_exchange.h"
#include "gsss_ladder.h"
#include "gsss_fast.h"
#include "gsss_launch.h"
#include "gsss_mh.h"
#include "gsss_autocov.h"
#include "gsss_marginals.h"
#include "gsss_mixing.h"
#include "gsss_moments.h"
#include "gsss_user_target.h"

namespace gsss {

// ------------------------------------------------------------------------------------------
// error text (thread local)
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static thread_local LaunchInfo g_last_launch = {0, 0, 0.0};
LaunchInfo &last_launch() { return g_last_launch; }

int64_t resident_workgroups(const void *kern, size_t lds_bytes, int *per_cu_out)
{
    struct Entry {
        const void *kern;
        size_t lds;
        int dev, per_cu, cus;
    };
    static std::mutex mu;
    static std::vector<Entry> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    // GSSS_RESIDENT_PER_CU (tests): plan the launch as if the chip held this many workgroups of the kernel per CU -- the sliced
    // shapes of another box reproduced on this one.  Safe for any value: a slice waits only for workgroups that drew their ticket
    // before it (SliceSched), whatever the plan assumed to be resident.  Read per call, never cached.
    const char *env = getenv("GSSS_RESIDENT_PER_CU");
    const int forced = env ? atoi(env) : 0;
    int per_cu = 0, cus = 0;
    {
        std::lock_guard<std::mutex> lock(mu);
        for (const Entry &e : cache)
            if (e.kern == kern && e.lds == lds_bytes && e.dev == dev) {
                per_cu = e.per_cu;
                cus = e.cus;
                break;
            }
    }
    if (per_cu < 1) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBlock, lds_bytes) != hipSuccess || per_cu < 1 ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
            (void)hipGetLastError();
            return 0;
        }
        std::lock_guard<std::mutex> lock(mu);
        cache.push_back(Entry{kern, lds_bytes, dev, per_cu, cus});
    }
    if (forced > 0) per_cu = forced;
    if (per_cu_out) *per_cu_out = per_cu;
    return (int64_t)per_cu * cus;
}

const Piece *piece_table_staged(int64_t n_chunks, int64_t resident, int64_t n_steps, int64_t *count_out, int64_t *split_out)
{
    struct Entry {
        int64_t n_chunks, resident, n_steps, count, split;
        Piece *table;
    };
    // (page-locked memory is visible to every device; an entry is never written again or freed, so a copy queued from it on any
    // stream stays valid.  A process plans a handful of shapes; past kMaxTables of them the launch falls back to one workgroup
    // per chunk rather than let the cache grow without bound.)
    constexpr size_t kMaxTables = 256;
    static std::mutex mu;
    static std::vector<Entry> cache;
    std::lock_guard<std::mutex> lock(mu);
    for (const Entry &e : cache)
        if (e.n_chunks == n_chunks && e.resident == resident && e.n_steps == n_steps) {
            *count_out = e.count;
            *split_out = e.split;
            return e.table;
        }
    if (cache.size() >= kMaxTables) return nullptr;
    int64_t split = 0;
    const std::vector<Piece> table = piece_plan(n_chunks, resident, n_steps, &split);
    if (table.empty()) return nullptr;
    void *host = nullptr;
    if (hipHostMalloc(&host, table.size() * sizeof(Piece), hipHostMallocPortable) != hipSuccess || host == nullptr) {
        (void)hipGetLastError();
        return nullptr;
    }
    memcpy(host, table.data(), table.size() * sizeof(Piece));
    cache.push_back(Entry{n_chunks, resident, n_steps, (int64_t)table.size(), split, static_cast<Piece *>(host)});
    *count_out = (int64_t)table.size();
    *split_out = split;
    return cache.back().table;
}

void slice_fallback_note(const char *why)
{
    if (getenv("GSSS_DEBUG_OCCUPANCY")) fprintf(stderr, "gsss: %s\n", why);
}

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------
// vector layout table / selection
// ------------------------------------------------------------------------------------------
static const VecInfo kVecs[] = {
#define GSSS_VEC_ROW(ID, V, NAME) {ID, V::L, V::N, V::DPAD, V::kExactDim, NAME},
    GSSS_VEC_LIST(GSSS_VEC_ROW)
#undef GSSS_VEC_ROW
};

const VecInfo *vec_table(int *count)
{
    *count = (int)(sizeof(kVecs) / sizeof(kVecs[0]));
    return kVecs;
}

int select_vec(int d, int variant)
{
    int n;
    const VecInfo *v = vec_table(&n);
    if (variant != 0) {
        for (int i = 0; i < n; ++i)
            if (v[i].id == variant) {
                if (v[i].exact_dim ? v[i].dpad == d : d <= v[i].dpad) return variant;
                set_error("kernel variant %s does not cover d=%d", v[i].name, d);
                return GSSS_E_UNSUPPORTED;
            }
        set_error("unknown kernel variant %d", variant);
        return GSSS_E_INVALID;
    }
    for (int i = 0; i < n; ++i)  // lane layouts first (exact d), then the smallest cooperative one
        if (v[i].exact_dim && v[i].dpad == d) return v[i].id;
    for (int i = 0; i < n; ++i)
        if (!v[i].exact_dim && d <= v[i].dpad) return v[i].id;
    set_error("no kernel variant covers d=%d (max %d)", d, v[n - 1].dpad);
    return GSSS_E_UNSUPPORTED;
}

// The built-in families of exact mode, one row a target kind: the policy's name as gsss_kernel_name prints it, its launchers
// (gsss_target_<family>.hip, gsss_mh_<family>.hip) and the rows select_vec_for budgets (NULL: Mixture sizes its whole launch).
// Registration and user targets are not here: they dispatch on cpd_variant and on the module's table.
struct ExactFamily {
    int kind;
    const char *name;
    decltype(&launch_run<VmfMixture>) run;
    decltype(&launch_logprob<VmfMixture>) logprob;
    decltype(&launch_mh<VmfMixture>) mh;
    size_t (*row_doubles)(int k, int d, size_t dpad);
};
#define GSSS_FAMILY(KIND, TT, ROWS) {KIND, #TT, launch_run<TT>, launch_logprob<TT>, launch_mh<TT>, ROWS}
static const ExactFamily kExactFamilies[] = {
    GSSS_FAMILY(GSSS_VMF_MIXTURE, VmfMixture, vmf_row_doubles), GSSS_FAMILY(GSSS_BINGHAM, Bingham, bingham_row_doubles),
    GSSS_FAMILY(GSSS_CURVE_VMF, CurveVmf, curve_row_doubles),   GSSS_FAMILY(GSSS_MIXTURE, Mixture, nullptr),
    GSSS_FAMILY(GSSS_ACG, Acg, bingham_row_doubles),
};
#undef GSSS_FAMILY
static const ExactFamily *exact_family(int kind)
{
    for (const ExactFamily &f : kExactFamilies)
        if (f.kind == kind) return &f;
    return nullptr;
}

// The layout an exact-mode launch of this target runs in: select_vec's -- unless the target's rows (component means, knots, a
// dense A) do not fit a workgroup's LDS in it: then the smallest sixty-four-lane layout, whose kernels read such rows from global
// memory (rows_fit_lds, gsss_device.h).  A layout forced by the caller stays as asked.
static int select_vec_for(const gsss::TargetBlock &tb, int variant)
{
    const int vec = select_vec(tb.d, variant);
    if (vec < 0 || variant != 0) return vec;
    int n;
    const VecInfo *v = vec_table(&n);
    size_t dpad = 0, L = 1;
    for (int i = 0; i < n; ++i)
        if (v[i].id == vec) {
            dpad = (size_t)v[i].dpad;
            L = (size_t)v[i].L;
        }
    if (dpad >= 256) return vec;
    bool fits = true;
    if (tb.kind == GSSS_MIXTURE) {  // the whole launch: component slots, Bingham scratch rows, draw tables and rows (Mixture)
        const MixInfo mi = mix_info(tb);
        const size_t need = (size_t)mi.n * kMixSlotReserve + (L > 1 ? (dpad + 1) * ((size_t)kBlock / L) : 0) + kMixDrawsReserve +
                            (size_t)mi.rows * dpad + (size_t)mi.extra;
        fits = need * sizeof(double) <= kMaxLdsBytes;
    } else if (const ExactFamily *f = exact_family(tb.kind)) {
        fits = f->row_doubles(tb.k, tb.d, dpad) * sizeof(double) <= gsss::kRowsLdsBytes;
    }
    if (fits) return vec;
    for (int i = 0; i < n; ++i)
        if (!v[i].exact_dim && v[i].dpad >= 256 && tb.d <= v[i].dpad) return v[i].id;
    return vec;
}

// ------------------------------------------------------------------------------------------
// device guard: HIP's current device is per host thread; leave it as we found it
// ------------------------------------------------------------------------------------------
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
        if (!ok) set_error("hipSetDevice(%d) failed", device);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// ------------------------------------------------------------------------------------------
// layout kernels: out[c][r] = in[r][c] for a row-major [R][C] matrix of doubles, LDS tiled so
// that both the read and the write are 64-lane coalesced (HBM-bound; 16 B of traffic per element)
// ------------------------------------------------------------------------------------------
constexpr int kTile = 64;

__global__ void __launch_bounds__(kBlock) transpose_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                           int64_t R, int64_t C)
{
    __shared__ double tile[kTile][kTile + 1];
    const int64_t gx = (C + kTile - 1) / kTile;
    const int64_t r0 = ((int64_t)blockIdx.x / gx) * kTile, c0 = ((int64_t)blockIdx.x % gx) * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;  // 64 x 4
    for (int i = ty; i < kTile; i += kBlock / kTile) {
        const int64_t r = r0 + i, c = c0 + tx;
        if (r < R && c < C) tile[i][tx] = in[r * C + c];
    }
    __syncthreads();
    for (int i = ty; i < kTile; i += kBlock / kTile) {
        const int64_t c = c0 + i, r = r0 + tx;
        if (r < R && c < C) out[c * R + r] = tile[tx][i];
    }
}

// 16-byte variant of the tile transpose for even R, C and 16-byte aligned buffers: every lane moves
// a double2 on both sides (1 KiB per wave-instruction), the tile is transposed on its way INTO LDS.
__global__ void __launch_bounds__(kBlock) transpose_kernel_x2(const double *__restrict__ in, double *__restrict__ out,
                                                              int64_t R, int64_t C)
{
    __shared__ double tileT[kTile][kTile + 2];  // [column][row], row stride 66 doubles keeps 16-B alignment
    const int64_t gx = (C + kTile - 1) / kTile;
    const int64_t r0 = ((int64_t)blockIdx.x / gx) * kTile, c0 = ((int64_t)blockIdx.x % gx) * kTile;
    const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;  // 32 x 8
    for (int i = ty; i < kTile; i += 8) {
        const int64_t r = r0 + i, c = c0 + 2 * tx;
        if (r < R && c < C) {  // C even: c + 1 < C too
            const double2 v = *reinterpret_cast<const double2 *>(in + r * C + c);
            tileT[2 * tx][i] = v.x;
            tileT[2 * tx + 1][i] = v.y;
        }
    }
    __syncthreads();
    for (int j = ty; j < kTile; j += 8) {
        const int64_t c = c0 + j, r = r0 + 2 * tx;
        if (c < C && r < R) {
            const double2 v = *reinterpret_cast<const double2 *>(&tileT[j][2 * tx]);
            *reinterpret_cast<double2 *>(out + c * R + r) = v;
        }
    }
}

// Skinny matrices (one side <= 32, e.g. [n][3] <-> [3][n]): a 64x64 tile would be mostly empty.
// A workgroup moves 256 indices of the long side x all S of the short side through LDS so that
// the side that is contiguous in memory is read / written as one linear, fully coalesced run.
constexpr int kSkinny = 32;

template <bool SHORT_ROWS>
__global__ void __launch_bounds__(kBlock) transpose_skinny_kernel(const double *__restrict__ in,
                                                                  double *__restrict__ out, int64_t R, int64_t C)
{
    __shared__ double buf[kBlock * (kSkinny + 1)];
    const int S = (int)(SHORT_ROWS ? R : C);           // short side
    const int64_t Lg = SHORT_ROWS ? C : R;              // long side
    const int SP = S | 1;                               // odd LDS stride: conflict-free
    const int64_t l0 = (int64_t)blockIdx.x * kBlock;
    const int nl = (int)((Lg - l0) < kBlock ? (Lg - l0) : kBlock);
    const int tid = threadIdx.x;
    if (SHORT_ROWS) {
        // in[r][l] coalesced along l; out[l][r]: one contiguous run of nl*S doubles
        if (tid < nl)
            for (int r = 0; r < S; ++r) buf[tid * SP + r] = in[(int64_t)r * C + l0 + tid];
        __syncthreads();
        double *dst = out + l0 * S;
        for (int k = tid; k < nl * S; k += kBlock) dst[k] = buf[(k / S) * SP + (k % S)];
    } else {
        // in[l][c]: one contiguous run of nl*S doubles; out[c][l] coalesced along l
        const double *src = in + l0 * S;
        for (int k = tid; k < nl * S; k += kBlock) buf[(k / S) * SP + (k % S)] = src[k];
        __syncthreads();
        if (tid < nl)
            for (int c = 0; c < S; ++c) out[(int64_t)c * R + l0 + tid] = buf[tid * SP + c];
    }
}

static int transpose(const double *in, double *out, int64_t R, int64_t C, int device, hipStream_t st)
{
    if (R <= 0 || C <= 0) return GSSS_OK;
    if (!in || !out) {
        set_error("null buffer");
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    if (R <= kSkinny || C <= kSkinny) {
        const bool short_rows = R <= C;
        const int64_t longside = short_rows ? C : R;
        const int64_t grid = ceil_div(longside, kBlock);
        if (grid > 0x7FFFFFFFll) {
            set_error("transpose: %lld x %lld exceeds the grid", (long long)R, (long long)C);
            return GSSS_E_UNSUPPORTED;
        }
        return launch_kernel("transpose", short_rows ? transpose_skinny_kernel<true> : transpose_skinny_kernel<false>, grid, 0, st,
                             nullptr, in, out, R, C);
    }
    const int64_t gx = ceil_div(C, kTile), gy = ceil_div(R, kTile);
    if (gx * gy > 0x7FFFFFFFll) {
        set_error("transpose: %lld x %lld exceeds the grid", (long long)R, (long long)C);
        return GSSS_E_UNSUPPORTED;
    }
    const bool wide = (R % 2 == 0) && (C % 2 == 0) && (reinterpret_cast<uintptr_t>(in) % 16 == 0) &&
                      (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    return launch_kernel("transpose", wide ? transpose_kernel_x2 : transpose_kernel, gx * gy, 0, st, nullptr, in, out, R, C);
}

// ------------------------------------------------------------------------------------------
// sphere.sample_sphere twin: normals from the reserved step id, radially projected
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) sample_sphere_kernel(uint64_t seed, uint64_t chain_offset, int64_t n, int d,
                                                               double *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n) return;
    RunBlock rb{};
    rb.seed = seed;
    rb.chain_offset = chain_offset;
    PhiloxDraws<LaneVec<2>> dr;
    dr.init(rb, c, d);
    dr.begin_step(kInitStep);
    double ss = 0.0;
    for (int q = 0; 4 * q < d; ++q) {
        uint32_t w[4];
        double zz[4];
        dr.words(1u + (uint32_t)q, w);
        box_muller32(w[0], w[1], zz[0], zz[1]);
        box_muller32(w[2], w[3], zz[2], zz[3]);
        for (int i = 0; i < 4 && 4 * q + i < d; ++i) {
            out[(size_t)(4 * q + i) * n + c] = zz[i];
            ss = fma(zz[i], zz[i], ss);
        }
    }
    const double nrm = sqrt(ss) + 1e-100;  // sphere.py:14
    for (int j = 0; j < d; ++j) out[(size_t)j * n + c] = out[(size_t)j * n + c] / nrm;
}


// ------------------------------------------------------------------------------------------
// The S^2 tangent draw of the Philox stream, exposed for verification (gsss_tangent_s2): the very expressions the set-up of a
// step evaluates (screened_kernel / fast_kernel / wave_kernel: x.x, inv_norm, x / |x|, PhiloxDraws::tangent -> tangent3) for
// given states and angle words.  out[c][0..2] = n = x / |x|, [3..5] = b1 (the tangent at angle 0), [6..8] = b2 (at a quarter
// turn), [9..11] = the tangent for word w[c].  tab: the table-driven sincos of the throughput kernels, else the exact kernels'.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) tangent_s2_kernel(const double *__restrict__ x, const uint32_t *__restrict__ w, int64_t n,
                                                            int tab_driven, double *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) double lds[kTabLds + 2];
    const fm::Tables tab = stage_tables(lds);
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n) return;
    using V = LaneVec<3>;
    const double xs[3] = {x[3 * c], x[3 * c + 1], x[3 * c + 2]};
    const double xx = vdot<V>(xs, xs);
    double nrm[3];
    if (tab_driven) {  // gsss_screen.h / gsss_fast.h: x * rsqrt(x.x)
        const double rnx = inv_norm(xx);
        for (int j = 0; j < 3; ++j) nrm[j] = xs[j] * rnx;
    } else {           // run_kernel (gsss_device.h): x / (|x| + 1e-100), sphere.py:14
        const double nx = sqrt(xx) + 1e-100;
        for (int j = 0; j < 3; ++j) nrm[j] = xs[j] / nx;
    }
    double u[3], b1[3], b2[3];
    if (tab_driven) {
        PhiloxDraws<V, true> dr;
        dr.tab = tab;
        dr.d = 3;
        dr.tangent(nrm, u, 0, w[c]);
    } else {
        PhiloxDraws<V, false> dr;
        dr.d = 3;
        dr.tangent(nrm, u, 0, w[c]);
    }
    tangent3(nrm[0], nrm[1], nrm[2], 0.0, 1.0, b1[0], b1[1], b1[2]);
    tangent3(nrm[0], nrm[1], nrm[2], 1.0, 0.0, b2[0], b2[1], b2[2]);
    double *o = out + 12 * c;
    for (int j = 0; j < 3; ++j) {
        o[j] = nrm[j];
        o[3 + j] = b1[j];
        o[6 + j] = b2[j];
        o[9 + j] = u[j];
    }
}

}  // namespace gsss

namespace gsss {
int launch_cpd_run(int variant, int draws, const TargetBlock &tb, const RunBlock &rb, hipStream_t st);
int launch_cpd_mh(int variant, int draws, int sampler, const TargetBlock &tb, const RunBlock &rb, const MhBlock &mb, hipStream_t st);
int launch_cpd_logprob(int variant, const TargetBlock &tb, const double *x, int64_t n, double *out, bool grad, hipStream_t st);
}  // namespace gsss

// ==========================================================================================
// extern "C"
// ==========================================================================================
using namespace gsss;

struct gsss_target {
    int device;
    TargetBlock tb;
    double *blob_dev;
    size_t blob_doubles;
    int cpd_variant;  // GSSS_CPD: which registration kernel (neighbour-list size, uniform source weights)
    const UserModuleTable *user;  // GSSS_USER: the compiled module's launchers (gsss_user_target.h)
    BatchInfo batch;  // gsss_target_create_batch: n_targets > 0 -- blob_dev holds every member's blob, tb describes any one of them
};

static bool is_batch(const gsss_target *t) { return t->batch.n_targets > 0; }

// The ask of a fast-mode launch (gsss_fast_select.h): the target's shape and the launch's traits.  The two environment switches
// that take part in the selection are read here, so that fast_select itself reads nothing.
static FastAsk fast_ask(const gsss_target *t, int screen, bool spread, bool numpy = false, bool replay = false, bool stats = false)
{
    const TargetBlock &tb = t->tb;
    FastAsk a{};
    a.kind = tb.kind;
    a.d = tb.d;
    a.k = tb.k;
    if (tb.kind == GSSS_MIXTURE) {
        const MixInfo mi = mix_info(tb);
        a.k = mi.terms;
        a.mix_curve = mi.curve;
    }
    a.scale = tb.scale;
    a.screen = screen;
    a.spread = spread;
    a.numpy = numpy;
    a.replay = replay;
    a.stats = stats;
    a.batch = is_batch(t);
    a.curve_tail = 1;
    if (tb.kind == GSSS_CURVE_VMF) {
        static const bool two = [] {
            const char *e = getenv("GSSS_CURVE_L2");
            return e && e[0] == '1';
        }();
        const char *env_tail = getenv("GSSS_CURVE_TAIL");  // (read per launch: tests switch it)
        a.curve_l2 = two;
        a.curve_tail = env_tail ? atoi(env_tail) : 1;
    }
    return a;
}

// fast_select refused the shape: say which
static int fast_refused(const gsss_target *t)
{
    const TargetBlock &tb = t->tb;
    if (is_batch(t) && tb.kind == GSSS_VMF_MIXTURE)
        set_error("fast mode is not built for a batch of vMF mixtures with d=%d, K=%d: the batch kernels are the lane-per-chain ones "
                  "(d = 3 .. 10 with K <= 16; d = 11 .. 16 with K <= 10); use GSSS_MODE_EXACT", tb.d, tb.k);
    else if (is_batch(t))
        set_error("fast mode is not built for a batch of Bingham targets with d=%d: the batch kernels are the lane-per-chain ones "
                  "(d = 3 .. 16); use GSSS_MODE_EXACT", tb.d);
    else if (tb.kind == GSSS_VMF_MIXTURE)
        set_error("fast mode is not built for a vMF mixture with d=%d, K=%d", tb.d, tb.k);
    else if (tb.kind == GSSS_BINGHAM)
        set_error("fast mode is not built for a Bingham target with d=%d", tb.d);
    else if (tb.kind == GSSS_ACG)
        set_error("fast mode is not built for an angular central Gaussian target with d=%d: the lane kernels cover d = 3 .. 10; "
                  "use GSSS_MODE_EXACT", tb.d);
    else if (tb.kind == GSSS_CURVE_VMF)
        set_error("fast mode is not built for a curve-vMF target with d=%d, %d knots", tb.d, tb.k);
    else if (tb.kind == GSSS_MIXTURE) {
        const MixInfo mi = mix_info(tb);
        set_error("fast mode is not built for this mixture (d=%d, %d terms%s): d = 3 .. 16, at most %d vMF / Bingham terms, "
                  "no curve component", tb.d, mi.terms, mi.curve ? ", a curve component" : "", kMixFastTerms);
    } else
        set_error("fast mode is not built for target kind %d", tb.kind);
    return GSSS_E_UNSUPPORTED;
}

// the pick goes to its family's launcher (tb: the target, or the launch's first member of a batch)
static int fast_launch(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, bool replay, hipStream_t st)
{
    if (p.batch) {  // the plan gsss_batch_plan reports: workgroups shared among small targets, or one target per workgroup
        BatchPlan bp;
        if (batch_plan(tb.kind, tb.d, tb.k, rb.n_chains / bi.m, bi.m, bp) != GSSS_OK) {  // (it asks fast_select what the pick came from)
            set_error("target batch: no launch plan for kind %d, d=%d, k=%d with %lld chains, %lld per target", tb.kind, tb.d, tb.k,
                      (long long)rb.n_chains, (long long)bi.m);
            return GSSS_E_UNSUPPORTED;
        }
        const bool vmf = tb.kind == GSSS_VMF_MIXTURE;
        if (bp.shared) return vmf ? launch_batch_fast_vmf<BatchShared>(p, bp, tb, rb, bi, st) : launch_batch_fast_bingham<BatchShared>(p, bp, tb, rb, bi, st);
        return vmf ? launch_batch_fast_vmf<BatchBlock>(p, bp, tb, rb, bi, st) : launch_batch_fast_bingham<BatchBlock>(p, bp, tb, rb, bi, st);
    }
    switch (tb.kind) {
    case GSSS_VMF_MIXTURE: return launch_fast_vmf(p, tb, rb, replay, st);
    case GSSS_BINGHAM: return launch_fast_bingham(p, tb, rb, replay, st);
    case GSSS_CURVE_VMF: return launch_fast_curve(p, tb, rb, replay, st);
    case GSSS_MIXTURE: return launch_fast_mixture(p, tb, rb, replay, st);
    case GSSS_ACG: return launch_fast_acg(p, tb, rb, replay, st);
    }
    return pick_error(p);
}

// The parameter blob of one target (layout per kind: TargetBlock::blob); gsss_target_create, and per component
// gsss_target_create_mixture
struct PackedTarget {
    std::vector<double> blob;
    bool bingham_diagonal = false;  // GSSS_BINGHAM, GSSS_ACG: A is diagonal
    double scale = 0.0;             // TargetBlock::scale
    int cpd_variant = 0;
};

static int pack_target(const gsss_target_desc *desc, PackedTarget &out)
{
    const int d = desc->d, k = desc->k;
    std::vector<double> &blob = out.blob;
    double &scale = out.scale;
    switch (desc->kind) {
    case GSSS_VMF_MIXTURE:
        if (k < 1 || !desc->mu || !desc->logc) {
            set_error("vMF mixture needs k >= 1, mu and logc");
            return GSSS_E_INVALID;
        }
        blob.assign(desc->mu, desc->mu + (size_t)k * d);
        blob.insert(blob.end(), desc->logc, desc->logc + k);
        for (int c = 0; c < k; ++c) {
            double ss = 0.0;
            for (int i = 0; i < d; ++i) ss += desc->mu[(size_t)c * d + i] * desc->mu[(size_t)c * d + i];
            scale = std::fmax(scale, std::sqrt(ss));
        }
        break;
    case GSSS_BINGHAM:
        if (!desc->A) {
            set_error("Bingham needs A");
            return GSSS_E_INVALID;
        }
        blob.assign(desc->A, desc->A + (size_t)d * d);
        if (desc->mu)  // BinghamFisher: linear term b
            blob.insert(blob.end(), desc->mu, desc->mu + d);
        else
            blob.insert(blob.end(), (size_t)d, 0.0);
        {
            bool diag = true;
            for (int i = 0; i < d && diag; ++i)
                for (int j = 0; j < d; ++j)
                    if (i != j && desc->A[(size_t)i * d + j] != 0.0) {
                        diag = false;
                        break;
                    }
            out.bingham_diagonal = diag;
        }
        break;
    case GSSS_ACG: {
        if (!desc->A) {
            set_error("angular central Gaussian needs A (the precision matrix Lambda)");
            return GSSS_E_INVALID;
        }
        const double *L = desc->A;
        bool diag = true;
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < i; ++j) {
                if (L[(size_t)i * d + j] != L[(size_t)j * d + i]) {
                    set_error("angular central Gaussian: Lambda is not symmetric (Lambda[%d][%d] = %.17g, Lambda[%d][%d] = %.17g)", i, j,
                              L[(size_t)i * d + j], j, i, L[(size_t)j * d + i]);
                    return GSSS_E_INVALID;
                }
                if (L[(size_t)i * d + j] != 0.0) diag = false;
            }
        // positive definite: a Cholesky factorisation (lower triangle, row by row) finds a pivot that is not > 0, or a NaN / Inf.
        // (d^3 / 6 products; eight running sums keep the additions from waiting on one another: under a second at d = 2048)
        std::vector<double> c((size_t)d * d, 0.0);
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) {
                const double *ci = &c[(size_t)i * d], *cj = &c[(size_t)j * d];
                double part[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                int m = 0;
                for (; m + 8 <= j; m += 8)
                    for (int r = 0; r < 8; ++r) part[r] += ci[m + r] * cj[m + r];
                for (; m < j; ++m) part[0] += ci[m] * cj[m];
                const double s = L[(size_t)i * d + j] - (((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7])));
                if (i == j) {
                    if (!(s > 0.0) || !(s < INFINITY)) {
                        set_error("angular central Gaussian: Lambda is not positive definite (Cholesky pivot %d is %g)", i, s);
                        return GSSS_E_INVALID;
                    }
                    c[(size_t)i * d + i] = std::sqrt(s);
                } else
                    c[(size_t)i * d + j] = s / c[(size_t)j * d + j];
            }
        blob.assign(L, L + (size_t)d * d);
        blob.insert(blob.end(), (size_t)d, 0.0);  // the row where Bingham keeps b: Acg<V> runs Bingham<V>'s quadratic form
        out.bingham_diagonal = diag;
        break;
    }
    case GSSS_CURVE_VMF: {
        if (k < 2 || !desc->knots) {
            set_error("curve-vMF needs k >= 2 knots");
            return GSSS_E_INVALID;
        }
        blob.assign(desc->knots, desc->knots + (size_t)k * d);
        // per segment: theta = distance(a, b) and its cos / sin / sin + 1e-10 -- the x-independent
        // quantities distance_slerp recomputes on every call (spherical_curve.py:28-31)
        for (int s = 0; s + 1 < k; ++s) {
            const double *a = desc->knots + (size_t)s * d, *b = a + d;
            double ab = 0.0;
            for (int i = 0; i < d; ++i) ab += a[i] * b[i];
            ab = ab < -1.0 ? -1.0 : (ab > 1.0 ? 1.0 : ab);
            const double theta = std::acos(ab);
            blob.push_back(theta);
            blob.push_back(std::cos(theta));
            blob.push_back(std::sin(theta));
            blob.push_back(std::sin(theta) + 1e-10);
        }
        break;
    }
    case GSSS_CPD: {
        const int ns = k, nt = desc->n_target, dt = desc->target_dim, kn = desc->k_nn;
        if (d != 4 || ns < 1 || ns > 65535 || nt < 1 || nt > 4000 || (dt != 2 && dt != 3) || kn < 1 || kn > 24 || kn > ns ||
            !desc->source || !desc->source_w || !desc->target || !desc->target_w || !(desc->sigma > 0.0)) {
            set_error("registration target needs d = 4, 1 <= k_nn <= min(24, source points), target_dim 2 or 3, sigma > 0, "
                      "<= 65535 source and <= 4000 target points, and all four arrays");
            return GSSS_E_INVALID;
        }
        if ((size_t)(4 * ns + 4 * nt + 8) * sizeof(double) > 150 * 1024) {
            set_error("registration target: the point clouds do not fit the LDS");
            return GSSS_E_UNSUPPORTED;
        }
        const double s2 = desc->sigma * desc->sigma;
        // registration.py:215-219 (CoherentPointDrift) / :110-111 (GaussianMixtureModel)
        const double log_const = (desc->outlier ? std::log(1.0 - desc->omega) : 0.0) - 0.5 * dt * std::log(2.0 * 3.141592653589793 * s2);
        blob.assign(desc->source, desc->source + (size_t)3 * ns);
        bool uniform = true;
        for (int i = 0; i < ns; ++i) {
            blob.push_back(std::log(desc->source_w[i]) + log_const);
            uniform = uniform && desc->source_w[i] == desc->source_w[0];
        }
        for (int l = 0; l < nt; ++l)
            for (int j = 0; j < 3; ++j) blob.push_back(j < dt ? desc->target[(size_t)l * dt + j] : 0.0);
        blob.insert(blob.end(), desc->target_w, desc->target_w + nt);
        blob.push_back(std::log(desc->omega + 1e-308) - desc->log_volume);  // registration.py:236
        blob.push_back(0.5 / s2);
        blob.push_back(desc->beta);
        blob.push_back(desc->outlier ? 1.0 : 0.0);
        blob.push_back((double)dt);
        blob.push_back((double)kn);
        blob.push_back(0.0);
        blob.push_back(0.0);
        out.cpd_variant = (kn <= 8 ? 0 : 2) + (uniform ? 0 : 1);
        break;
    }
    default:
        set_error("unknown target kind %d", desc->kind);
        return GSSS_E_INVALID;
    }
    return GSSS_OK;
}

// TargetBlock::k of a Bingham target holds flags: bit 0 a diagonal A, bit 1 a linear term (BinghamFisher)
static int bingham_flags(bool diagonal, const gsss_target_desc *desc) { return (diagonal ? 1 : 0) | (desc->mu ? 2 : 0); }

// The one upload path of the target creators: `n` doubles at `host` go to `device`, and *out becomes a copy of `proto` (the
// creator's filled-in handle: TargetBlock, cpd_variant, user, batch) that owns them.  Called after every argument was checked:
// nothing before it touches the device.
static int upload_target(const double *host, size_t n, int device, const gsss_target &proto, gsss_target **out)
{
    int ndev = gsss_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) {
        set_error("device %d not available (%d HIP devices visible)", device, ndev);
        return GSSS_E_NO_DEVICE;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    gsss_target *t = new (std::nothrow) gsss_target(proto);
    if (!t) {
        set_error("out of host memory");
        return GSSS_E_INVALID;
    }
    t->device = device;
    t->blob_doubles = n;
    t->blob_dev = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->blob_dev), (n > 0 ? n : 1) * sizeof(double));
    if (e == hipSuccess && n > 0) e = hipMemcpy(t->blob_dev, host, n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("copying target parameters failed: %s", hipGetErrorString(e));
        if (t->blob_dev) (void)hipFree(t->blob_dev);
        delete t;
        return GSSS_E_HIP;
    }
    t->tb.blob = t->blob_dev;
    *out = t;
    return GSSS_OK;
}

extern "C" {

int gsss_abi_version(void) { return GSSS_ABI_VERSION; }

const char *gsss_last_error(void) { return g_err; }

int gsss_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int gsss_target_create(const gsss_target_desc *desc, int device, gsss_target **out)
{
    if (!desc || !out) {
        set_error("null argument");
        return GSSS_E_INVALID;
    }
    *out = nullptr;
    const int d = desc->d, k = desc->k;
    if (d < 2) {
        set_error("d must be >= 2 (got %d)", d);
        return GSSS_E_INVALID;
    }
    if (select_vec(d, 0) < 0) return GSSS_E_UNSUPPORTED;  // before any parameter array is touched
    PackedTarget pk;
    if (int rc = pack_target(desc, pk)) return rc;
    gsss_target proto{};
    proto.tb.kind = desc->kind;
    proto.tb.d = d;
    proto.tb.k = desc->kind == GSSS_BINGHAM ? bingham_flags(pk.bingham_diagonal, desc) : k;
    if (desc->kind == GSSS_ACG) proto.tb.k = pk.bingham_diagonal ? 1 : 0;  // bit 0 as for Bingham: a diagonal Lambda
    if (desc->kind == GSSS_CPD) proto.tb.k = k | (desc->n_target << 16);  // registration: both cloud sizes
    proto.tb.kappa = desc->kappa;
    proto.tb.scale = pk.scale;
    proto.cpd_variant = pk.cpd_variant;
    return upload_target(pk.blob.data(), pk.blob.size(), device, proto, out);
}

int gsss_target_create_mixture(const gsss_target_desc *components, int32_t n_components, const double *log_weights, int device,
                               gsss_target **out)
{
    if (!components || !log_weights || !out) {
        set_error("null argument");
        return GSSS_E_INVALID;
    }
    *out = nullptr;
    if (n_components < 1) {
        set_error("a mixture needs at least one component (got %d)", n_components);
        return GSSS_E_INVALID;
    }
    if (n_components > kMixMaxComponents) {
        set_error("a mixture takes at most %d components (got %d)", kMixMaxComponents, n_components);
        return GSSS_E_UNSUPPORTED;
    }
    const int d = components[0].d;
    if (d < 2) {
        set_error("d must be >= 2 (got %d)", d);
        return GSSS_E_INVALID;
    }
    for (int c = 0; c < n_components; ++c) {
        const int kind = components[c].kind;
        if (kind == GSSS_CPD) {
            set_error("component %d: registration targets are not built as mixture components", c);
            return GSSS_E_UNSUPPORTED;
        }
        if (kind != GSSS_VMF_MIXTURE && kind != GSSS_BINGHAM && kind != GSSS_CURVE_VMF) {
            set_error("component %d: kind %d is not a mixture component (vMF mixture, Bingham or curve-vMF; nested mixtures are "
                      "flattened by the caller)", c, kind);
            return GSSS_E_INVALID;
        }
        if (components[c].d != d) {
            set_error("mixture components must share d (component 0 has d=%d, component %d d=%d)", d, c, components[c].d);
            return GSSS_E_INVALID;
        }
        if (log_weights[c] != log_weights[c] || log_weights[c] == INFINITY) {
            set_error("component %d: log weight must be finite or -inf", c);
            return GSSS_E_INVALID;
        }
    }
    if (select_vec(d, 0) < 0) return GSSS_E_UNSUPPORTED;
    // header (gsss_device.h, Mixture), then every component's blob as gsss_target_create packs it
    std::vector<double> blob(1 + (size_t)n_components * kMixHeader, 0.0);
    blob[0] = (double)n_components;
    int64_t rows = 0, extra = 0, terms = 0;
    int nb = 0;
    bool curve = false;
    double scale_all = 0.0;
    for (int c = 0; c < n_components; ++c) {
        const gsss_target_desc *desc = components + c;
        PackedTarget pk;
        if (int rc = pack_target(desc, pk)) {
            std::string msg = g_err;
            set_error("component %d: %s", c, msg.c_str());
            return rc;
        }
        const std::vector<double> &part = pk.blob;
        const double scale = pk.scale;
        const int k = desc->kind == GSSS_BINGHAM ? bingham_flags(pk.bingham_diagonal, desc) : desc->k;
        double *h = blob.data() + 1 + (size_t)c * kMixHeader;
        h[0] = (double)desc->kind;
        h[1] = (double)k;
        h[2] = desc->kappa;
        h[3] = scale;
        h[4] = log_weights[c];
        h[5] = (double)blob.size();
        blob.insert(blob.end(), part.begin(), part.end());
        scale_all = std::fmax(scale_all, scale);
        switch (desc->kind) {
        case GSSS_VMF_MIXTURE:
            rows += desc->k;
            extra += desc->k;
            terms += desc->k;
            break;
        case GSSS_BINGHAM:
            rows += d + 1;
            ++nb;
            ++terms;
            break;
        default:
            rows += desc->k;
            extra += 4 * (int64_t)(desc->k - 1);
            curve = true;
            ++terms;
            break;
        }
    }
    if (rows > kMixMaxRows || extra > kMixMaxRows) {
        set_error("a mixture takes at most %d parameter rows in all (vMF means, knots, d + 1 per Bingham component; got %lld)",
                  kMixMaxRows, (long long)rows);
        return GSSS_E_UNSUPPORTED;
    }
    gsss_target proto{};
    proto.tb.kind = GSSS_MIXTURE;
    proto.tb.d = d;
    proto.tb.k = mix_pack_k(n_components, nb, (int)(terms < 255 ? terms : 255), curve);  // (mix_info)
    proto.tb.dpad = (int32_t)rows;
    proto.tb.kappa = (double)extra;
    proto.tb.scale = scale_all;
    return upload_target(blob.data(), blob.size(), device, proto, out);
}

int gsss_target_create_batch(const gsss_target_desc *targets, int32_t n_targets, int64_t chains_per_target, int device,
                             gsss_target **out)
{
    if (!targets || !out) {
        set_error("null argument");
        return GSSS_E_INVALID;
    }
    *out = nullptr;
    if (n_targets < 1 || chains_per_target < 1) {
        set_error("a target batch needs at least one target and one chain per target (got %d, %lld)", n_targets,
                  (long long)chains_per_target);
        return GSSS_E_INVALID;
    }
    if (chains_per_target > 0x7FFFFFFFll - 1024) {
        set_error("a target batch takes at most 2^31-1025 chains per target");
        return GSSS_E_UNSUPPORTED;
    }
    const int kind = targets[0].kind, d = targets[0].d, k = targets[0].k;
    if (kind != GSSS_VMF_MIXTURE && kind != GSSS_BINGHAM) {
        set_error("a target batch holds vMF mixtures (GSSS_VMF_MIXTURE) or Bingham / Fisher-Bingham targets (GSSS_BINGHAM): kind %d "
                  "(curve-vMF, registration, GSSS_MIXTURE and user targets) is not built as a batch member", kind);
        return GSSS_E_UNSUPPORTED;
    }
    if (d < 2) {
        set_error("d must be >= 2 (got %d)", d);
        return GSSS_E_INVALID;
    }
    if (select_vec(d, 0) < 0) return GSSS_E_UNSUPPORTED;
    // every member as gsss_target_create packs it, at an equal stride (the blob's size follows from kind, d and K)
    std::vector<double> all;
    size_t stride = 0;
    bool all_diagonal = true;
    double scale_all = 0.0;
    for (int t = 0; t < n_targets; ++t) {
        const gsss_target_desc *desc = targets + t;
        if (desc->kind != kind) {
            set_error("the members of a target batch are of one family (member 0 has kind %d, member %d kind %d)", kind, t, desc->kind);
            return GSSS_E_UNSUPPORTED;
        }
        if (desc->d != d) {
            set_error("the members of a target batch share d (member 0 has d=%d, member %d d=%d)", d, t, desc->d);
            return GSSS_E_UNSUPPORTED;
        }
        if (kind == GSSS_VMF_MIXTURE && desc->k != k) {
            set_error("the vMF mixtures of a target batch share K (member 0 has K=%d, member %d K=%d)", k, t, desc->k);
            return GSSS_E_UNSUPPORTED;
        }
        if (kind == GSSS_BINGHAM && (desc->mu != nullptr) != (targets[0].mu != nullptr)) {
            set_error("the Bingham members of a target batch all have a linear term b or none has (member 0 %s, member %d %s)",
                      targets[0].mu ? "has one" : "has none", t, desc->mu ? "has one" : "has none");
            return GSSS_E_UNSUPPORTED;
        }
        PackedTarget pk;
        if (int rc = pack_target(desc, pk)) {
            std::string msg = g_err;
            set_error("member %d: %s", t, msg.c_str());
            return rc;
        }
        const std::vector<double> &part = pk.blob;
        if (t == 0) {
            stride = part.size();
            all.reserve(stride * (size_t)n_targets);
        }
        if (part.size() != stride) {
            set_error("corrupt target batch: member %d packs to another size", t);
            return GSSS_E_INVALID;
        }
        all.insert(all.end(), part.begin(), part.end());
        all_diagonal = all_diagonal && pk.bingham_diagonal;
        scale_all = std::fmax(scale_all, pk.scale);
    }
    gsss_target proto{};
    proto.tb.kind = kind;
    proto.tb.d = d;
    // Bingham: the flags of gsss_target_create -- the diagonal kernels only if EVERY member's A is diagonal
    proto.tb.k = kind == GSSS_BINGHAM ? bingham_flags(all_diagonal, targets) : k;
    proto.tb.scale = scale_all;
    proto.batch = BatchInfo{n_targets, (int64_t)stride, chains_per_target};
    return upload_target(all.data(), all.size(), device, proto, out);
}

int gsss_exact_layout(int32_t d)
{
    if (d < 2) {
        set_error("d must be >= 2 (got %d)", d);
        return GSSS_E_INVALID;
    }
    return select_vec(d, 0);
}

int gsss_target_create_user(const void *table, int32_t d, const double *params, int64_t n_params, int device, gsss_target **out)
{
    if (!table || !out || n_params < 0 || (n_params > 0 && !params)) {
        set_error("bad argument to gsss_target_create_user");
        return GSSS_E_INVALID;
    }
    *out = nullptr;
    const UserModuleTable *m = static_cast<const UserModuleTable *>(table);
    if (m->module_abi != kUserModuleAbi || m->gsss_abi != GSSS_ABI_VERSION) {
        set_error("user module built for module ABI %d / library ABI %d, this library has %d / %d: recompile it", m->module_abi,
                  m->gsss_abi, kUserModuleAbi, GSSS_ABI_VERSION);
        return GSSS_E_UNSUPPORTED;
    }
    if (!m->digest || strcmp(m->digest, gsss_source_digest()) != 0) {
        set_error("user module compiled from other kernel sources (digest %.12s) than this library (%.12s): recompile it",
                  m->digest ? m->digest : "none", gsss_source_digest());
        return GSSS_E_UNSUPPORTED;
    }
    if (d < 2) {
        set_error("d must be >= 2 (got %d)", d);
        return GSSS_E_INVALID;
    }
    const int vec = select_vec(d, 0);
    if (vec < 0) return vec;
    if (vec != m->vec_id) {
        set_error("user module built for vector layout %d, d=%d runs in layout %d", m->vec_id, d, vec);
        return GSSS_E_UNSUPPORTED;
    }
    if (n_params > 0x7FFFFFFFll) {
        set_error("a user target takes at most 2^31-1 parameters");
        return GSSS_E_UNSUPPORTED;
    }
    gsss_target proto{};
    proto.tb.kind = GSSS_USER;
    proto.tb.d = d;
    proto.tb.k = (int32_t)n_params;
    proto.user = m;
    return upload_target(params, (size_t)n_params, device, proto, out);
}

int gsss_target_destroy(gsss_target *t)
{
    if (!t) return GSSS_OK;
    DeviceGuard guard(t->device);
    if (t->blob_dev) (void)hipFree(t->blob_dev);
    delete t;
    return GSSS_OK;
}

int gsss_target_dim(const gsss_target *t) { return t ? t->tb.d : GSSS_E_INVALID; }

static int logprob_or_gradient(const gsss_target *t, const double *x_dev, int64_t n, double *out_dev, bool grad, void *stream)
{
    if (!t || n < 0 || (n > 0 && (!x_dev || !out_dev))) {
        set_error(grad ? "bad argument to gsss_gradient" : "bad argument to gsss_logprob");
        return GSSS_E_INVALID;
    }
    if (is_batch(t)) {
        set_error("%s is not built for a target batch: evaluate the members' own handles", grad ? "gsss_gradient" : "gsss_logprob");
        return GSSS_E_UNSUPPORTED;
    }
    if (n == 0) return GSSS_OK;
    const int vec = select_vec_for(t->tb, 0);
    if (vec < 0) return vec;
    DeviceGuard guard(t->device);
    if (!guard.ok) return GSSS_E_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const ExactFamily *f = exact_family(t->tb.kind)) return f->logprob(vec, t->tb, x_dev, n, out_dev, grad, st);
    if (t->tb.kind == GSSS_CPD) return launch_cpd_logprob(t->cpd_variant, t->tb, x_dev, n, out_dev, grad, st);
    if (t->tb.kind == GSSS_USER) {
        if (grad && !t->user->has_gradient) {
            set_error("this user target defines no gsss_user_gradient");
            return GSSS_E_UNSUPPORTED;
        }
        return t->user->logprob(t->tb, x_dev, n, out_dev, grad, st);
    }
    set_error("corrupt target");
    return GSSS_E_INVALID;
}

int gsss_logprob(const gsss_target *t, const double *x_dev, int64_t n, double *out_dev, void *stream)
{
    return logprob_or_gradient(t, x_dev, n, out_dev, false, stream);
}

int gsss_gradient(const gsss_target *t, const double *x_dev, int64_t n, double *grad_dev, void *stream)
{
    return logprob_or_gradient(t, x_dev, n, grad_dev, true, stream);
}

// every member of a batch handle at its own rows of x_dev [M][n][d]
static int batch_logprob_or_gradient(const gsss_target *t, const double *x_dev, int64_t n, double *out_dev, bool grad, void *stream)
{
    const char *fn = grad ? "gsss_batch_gradient" : "gsss_batch_logprob";
    if (!t || n < 0) {
        set_error("%s: %s", fn, t ? "n_per_target must be >= 0" : "null handle");
        return GSSS_E_INVALID;
    }
    if (!is_batch(t)) {
        set_error("%s takes a gsss_target_create_batch handle: a single target is evaluated by %s", fn, grad ? "gsss_gradient" : "gsss_logprob");
        return GSSS_E_UNSUPPORTED;
    }
    if (n == 0) return GSSS_OK;
    if (!x_dev || !out_dev) {
        set_error("%s: %s is null", fn, x_dev ? "the output" : "x_dev");
        return GSSS_E_INVALID;
    }
    const int vec = select_vec_for(t->tb, 0);
    if (vec < 0) return vec;
    DeviceGuard guard(t->device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_batch_logprob(vec, t->tb, batch_points_rows(x_dev, out_dev, n, t->tb.d, t->batch.stride), t->batch.n_targets, grad,
                                static_cast<hipStream_t>(stream));
}

int gsss_batch_logprob(const gsss_target *t, const double *x_dev, int64_t n_per_target, double *out_dev, void *stream)
{
    return batch_logprob_or_gradient(t, x_dev, n_per_target, out_dev, false, stream);
}

int gsss_batch_gradient(const gsss_target *t, const double *x_dev, int64_t n_per_target, double *grad_dev, void *stream)
{
    return batch_logprob_or_gradient(t, x_dev, n_per_target, grad_dev, true, stream);
}

int gsss_batch_logprob_draws(const gsss_target *t, const double *samples_dev, int64_t n_rows, int64_t n_chains, int64_t target0,
                             double *out_dev, void *stream)
{
    if (!t || n_rows < 0 || n_chains < 0 || target0 < 0) {
        set_error("gsss_batch_logprob_draws: %s", t ? "n_rows, n_chains and target0 must be >= 0" : "null handle");
        return GSSS_E_INVALID;
    }
    if (!is_batch(t)) {
        set_error("gsss_batch_logprob_draws takes a gsss_target_create_batch handle");
        return GSSS_E_UNSUPPORTED;
    }
    const int64_t m = t->batch.m;
    if (n_chains % m != 0 || target0 > t->batch.n_targets || n_chains / m > t->batch.n_targets - target0) {
        set_error("gsss_batch_logprob_draws: %lld chains from target %lld on are no run of whole targets of the batch (%lld chains per "
                  "target, %d targets)", (long long)n_chains, (long long)target0, (long long)m, t->batch.n_targets);
        return GSSS_E_INVALID;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    if (!samples_dev || !out_dev) {
        set_error("gsss_batch_logprob_draws: %s is null", samples_dev ? "out_dev" : "samples_dev");
        return GSSS_E_INVALID;
    }
    const int vec = select_vec_for(t->tb, 0);
    if (vec < 0) return vec;
    DeviceGuard guard(t->device);
    if (!guard.ok) return GSSS_E_HIP;
    TargetBlock tbb = t->tb;
    tbb.blob += target0 * t->batch.stride;
    return launch_batch_logprob(vec, tbb, batch_points_draws(samples_dev, out_dev, n_rows, n_chains, m, tbb.d, t->batch.stride),
                                n_chains / m, false, static_cast<hipStream_t>(stream));
}

int64_t gsss_exchange_scratch_doubles(int64_t n_chains) { return n_chains < 0 ? GSSS_E_INVALID : 2 * n_chains; }

int gsss_batch_exchange(const gsss_target *t, double *state_dev, const int32_t *err_dev, int64_t n_chains, int64_t target0,
                        int32_t ladder, int32_t parity, uint64_t seed, uint64_t chain_offset, uint64_t step, double *scratch_dev,
                        int64_t *replica_dev, int64_t *counts_dev, double *log_alpha_out, void *stream)
{
    if (ladder < 2 || (parity != 0 && parity != 1)) {
        set_error("gsss_batch_exchange: need ladder >= 2 and parity 0 or 1 (ladder = %d, parity = %d)", ladder, parity);
        return GSSS_E_INVALID;
    }
    if (n_chains < 0 || target0 < 0 || target0 % ladder != 0) {
        set_error("gsss_batch_exchange: n_chains (%lld) must be >= 0 and target0 (%lld) a multiple of the ladder (%d) >= 0",
                  (long long)n_chains, (long long)target0, ladder);
        return GSSS_E_INVALID;
    }
    if (!t) {
        set_error("gsss_batch_exchange: null handle");
        return GSSS_E_INVALID;
    }
    if (!is_batch(t)) {
        set_error("gsss_batch_exchange takes a gsss_target_create_batch handle: a ladder is a run of a batch's members");
        return GSSS_E_UNSUPPORTED;
    }
    const int64_t m = t->batch.m;
    if (n_chains % (m * ladder) != 0 || target0 > t->batch.n_targets || n_chains / m > t->batch.n_targets - target0) {
        set_error("gsss_batch_exchange: %lld chains from target %lld on are no run of whole ladders of %d members of the batch (%lld "
                  "chains per target, %d targets)", (long long)n_chains, (long long)target0, ladder, (long long)m, t->batch.n_targets);
        return GSSS_E_INVALID;
    }
    if (chain_offset + (uint64_t)n_chains > (1ull << 48) || step >= kInitStep) {
        set_error("gsss_batch_exchange: chain ids and steps are 48-bit words of the stream's counter");
        return GSSS_E_INVALID;
    }
    if (n_chains == 0) return GSSS_OK;
    if (!state_dev || !err_dev || !scratch_dev) {
        set_error("gsss_batch_exchange: %s is null", !state_dev ? "state_dev" : (!err_dev ? "err_dev" : "scratch_dev"));
        return GSSS_E_INVALID;
    }
    const int vec = select_vec_for(t->tb, 0);
    if (vec < 0) return vec;
    DeviceGuard guard(t->device);
    if (!guard.ok) return GSSS_E_HIP;
    TargetBlock tbb = t->tb;
    tbb.blob += target0 * t->batch.stride;
    ExchangeBlock a{};
    a.state = state_dev;
    a.lp = scratch_dev;
    a.err = err_dev;
    a.replica = replica_dev;
    a.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    a.log_alpha = log_alpha_out;
    a.stride = t->batch.stride;
    a.n = n_chains;
    a.m = m;
    a.R = ladder;
    a.parity = parity;
    a.seed = seed;
    a.chain_offset = chain_offset;
    a.step = step;
    return launch_batch_exchange(vec, tbb, a, static_cast<hipStream_t>(stream));
}

int64_t gsss_ladder_scratch_doubles(int64_t n_rows, int64_t n_chains)
{
    if (n_rows < 0 || n_chains < 0) return GSSS_E_INVALID;
    if (n_rows == 0 || n_chains == 0) return 0;
    if (n_chains > INT64_MAX / 3 || n_rows > INT64_MAX / (3 * n_chains)) return GSSS_E_INVALID;
    return 3 * n_rows * n_chains;
}

int64_t gsss_ladder_acc_doubles(int64_t n_chains, int64_t chains_per_target, int32_t ladder)
{
    if (n_chains < 0 || chains_per_target < 1 || ladder < 2) return GSSS_E_INVALID;
    if (chains_per_target > INT64_MAX / ladder || n_chains % (chains_per_target * ladder) != 0) return GSSS_E_INVALID;
    if (n_chains > INT64_MAX / kLadderSlots) return GSSS_E_INVALID;
    return (n_chains / chains_per_target / ladder) * (ladder - 1) * chains_per_target * kLadderSlots;
}

int gsss_batch_ladder(const gsss_target *t, const double *samples_dev, int64_t n_rows, int64_t n_chains, int64_t target0,
                      int32_t ladder, double *scratch_dev, double *acc_dev, void *stream)
{
    if (ladder < 2) {
        set_error("gsss_batch_ladder: need ladder >= 2 (ladder = %d)", ladder);
        return GSSS_E_INVALID;
    }
    if (n_rows < 0 || n_chains < 0 || target0 < 0 || target0 % ladder != 0) {
        set_error("gsss_batch_ladder: n_rows (%lld) and n_chains (%lld) must be >= 0 and target0 (%lld) a multiple of the ladder (%d) "
                  ">= 0", (long long)n_rows, (long long)n_chains, (long long)target0, ladder);
        return GSSS_E_INVALID;
    }
    if (!t) {
        set_error("gsss_batch_ladder: null handle");
        return GSSS_E_INVALID;
    }
    if (!is_batch(t)) {
        set_error("gsss_batch_ladder takes a gsss_target_create_batch handle: a ladder is a run of a batch's members");
        return GSSS_E_UNSUPPORTED;
    }
    const int64_t m = t->batch.m;
    if (n_chains % (m * ladder) != 0 || target0 > t->batch.n_targets || n_chains / m > t->batch.n_targets - target0) {
        set_error("gsss_batch_ladder: %lld chains from target %lld on are no run of whole ladders of %d members of the batch (%lld "
                  "chains per target, %d targets)", (long long)n_chains, (long long)target0, ladder, (long long)m, t->batch.n_targets);
        return GSSS_E_INVALID;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    if (!samples_dev || !scratch_dev || !acc_dev) {
        set_error("gsss_batch_ladder: %s is null", !samples_dev ? "samples_dev" : (!scratch_dev ? "scratch_dev" : "acc_dev"));
        return GSSS_E_INVALID;
    }
    const int vec = select_vec_for(t->tb, 0);
    if (vec < 0) return vec;
    DeviceGuard guard(t->device);
    if (!guard.ok) return GSSS_E_HIP;
    TargetBlock tbb = t->tb;
    tbb.blob += target0 * t->batch.stride;
    LadderBlock a{};
    a.x = samples_dev;
    a.lp3 = scratch_dev;
    a.acc = acc_dev;
    a.stride = t->batch.stride;
    a.n_rows = n_rows;
    a.n = n_chains;
    a.m = m;
    a.R = ladder;
    return launch_batch_ladder(vec, tbb, a, static_cast<hipStream_t>(stream));
}

int gsss_run(const gsss_target *t, const gsss_run_args *a, void *stream)
{
    if (!t || !a) {
        set_error("null argument");
        return GSSS_E_INVALID;
    }
    if (a->n_chains < 0 || a->n_steps < 0 || a->thin < 1 || a->max_tries < 1) {
        set_error("need n_chains >= 0, n_steps >= 0, thin >= 1, max_tries >= 1");
        return GSSS_E_INVALID;
    }
    const bool mh = a->sampler == GSSS_RWMH || a->sampler == GSSS_HMC || a->sampler == GSSS_INDEP || a->sampler == GSSS_MIX;
    if (a->sampler != GSSS_SHRINK && a->sampler != GSSS_REJECT && !mh) {
        set_error("unknown sampler %d", a->sampler);
        return GSSS_E_INVALID;
    }
    if (mh && (a->mode != GSSS_MODE_EXACT || !a->stepsize_dev || a->adapt_steps < 0 || a->stats_dev ||
               (a->sampler == GSSS_HMC && a->n_leapfrog < 1))) {
        set_error("GSSS_RWMH / GSSS_HMC / GSSS_INDEP / GSSS_MIX need GSSS_MODE_EXACT, stepsize_dev, adapt_steps >= 0, no stats_dev "
                  "(HMC: n_leapfrog >= 1)");
        return GSSS_E_INVALID;
    }
    if (a->sampler == GSSS_MIX && (!(a->mixing_probability >= 0.0 && a->mixing_probability <= 1.0) || !a->adapt_left_dev)) {
        set_error("GSSS_MIX needs 0 <= mixing_probability <= 1 and adapt_left_dev");
        return GSSS_E_INVALID;
    }
    if (a->mode != GSSS_MODE_EXACT && a->mode != GSSS_MODE_FAST) {
        set_error("unknown mode %d", a->mode);
        return GSSS_E_INVALID;
    }
    if (a->chain_offset + (uint64_t)a->n_chains > (1ull << 48) || a->step_offset + (uint64_t)a->n_steps >= kInitStep) {
        set_error("chain / step ids exceed the 48-bit counter space");
        return GSSS_E_INVALID;
    }
    if (is_batch(t)) {  // (before anything runs: a refused launch of a batch leaves every buffer as it was)
        const int64_t m = t->batch.m;
        if (mh) {
            set_error("a target batch is sampled by GSSS_SHRINK and GSSS_REJECT only: the Metropolis-Hastings / HMC kernels (sampler %d) "
                      "have no batch build", a->sampler);
            return GSSS_E_UNSUPPORTED;
        }
        if (a->replay_dev || a->rng_state_dev) {
            set_error("a target batch runs on the library (Philox) stream only: no %s", a->replay_dev ? "replay_dev" : "rng_state_dev");
            return GSSS_E_UNSUPPORTED;
        }
        if (a->stats_dev) {
            set_error("running statistics (stats_dev) take one set of directions: they are not built for a target batch");
            return GSSS_E_UNSUPPORTED;
        }
        if (a->chain_offset % (uint64_t)m != 0) {
            set_error("target batch: chain_offset %llu is not a multiple of the %lld chains per target (a launch starts at a target's "
                      "first chain)", (unsigned long long)a->chain_offset, (long long)m);
            return GSSS_E_UNSUPPORTED;
        }
        if (a->n_chains % m != 0) {
            set_error("target batch: n_chains %lld is not a multiple of the %lld chains per target (a launch ends at a target's last "
                      "chain)", (long long)a->n_chains, (long long)m);
            return GSSS_E_UNSUPPORTED;
        }
        if (a->chain_offset / (uint64_t)m + (uint64_t)(a->n_chains / m) > (uint64_t)t->batch.n_targets) {
            set_error("target batch: chains %llu .. %llu belong to targets up to %llu, the batch holds %d",
                      (unsigned long long)a->chain_offset, (unsigned long long)(a->chain_offset + (uint64_t)a->n_chains),
                      (unsigned long long)(a->chain_offset / (uint64_t)m + (uint64_t)(a->n_chains / m)), t->batch.n_targets);
            return GSSS_E_UNSUPPORTED;
        }
    }
    last_launch() = LaunchInfo{0, 0, 0.0};
    if (a->n_chains == 0) return GSSS_OK;
    if (!a->state_dev) {
        set_error("state_dev is null");
        return GSSS_E_INVALID;
    }
    if (a->samples_chain_rows < 0 || (a->samples_chain_rows > 0 && a->samples_chain_rows < a->n_steps / a->thin)) {
        set_error("samples_chain_rows must be 0 or >= the rows this call writes");
        return GSSS_E_INVALID;
    }
    if (a->replay_dev && a->replay_stride < 1) {
        set_error("replay_stride must be >= 1");
        return GSSS_E_INVALID;
    }
    if (t->tb.kind == GSSS_USER && a->mode == GSSS_MODE_FAST) {
        set_error("fast mode is not built for user targets (GSSS_USER): use GSSS_MODE_EXACT");
        return GSSS_E_UNSUPPORTED;
    }
    if (a->mode == GSSS_MODE_FAST && a->variant != 0 && a->variant != GSSS_VARIANT_FAST_DOUBLE && a->variant != GSSS_VARIANT_FAST_VERIFY) {
        set_error("fast mode takes variant 0, GSSS_VARIANT_FAST_DOUBLE or GSSS_VARIANT_FAST_VERIFY");
        return GSSS_E_INVALID;
    }
    const int vec = a->mode == GSSS_MODE_FAST ? 0 : select_vec_for(t->tb, a->variant);
    if (vec < 0) return vec;
    if (t->tb.kind == GSSS_USER && vec != t->user->vec_id) {
        set_error("user module is built for vector layout %d only (variant %d asked for)", t->user->vec_id, a->variant);
        return GSSS_E_UNSUPPORTED;
    }
    RunBlock rb{};
    rb.state = a->state_dev;
    rb.samples = a->samples_dev;
    rb.n_reject = a->n_reject_dev;
    rb.n_tries = a->n_tries_dev;
    rb.err = a->err_dev;
    rb.replay = a->replay_dev;
    rb.rng_state = a->rng_state_dev;
    rb.replay_stride = a->replay_stride;
    rb.n_chains = a->n_chains;
    rb.n_steps = a->n_steps;
    rb.thin = a->thin;
    rb.seed = a->seed;
    rb.chain_offset = a->chain_offset;
    rb.step_offset = a->step_offset;
    const CounterWords cw = counter_words(a->chain_offset, a->n_chains, a->step_offset, a->n_steps);
    rb.ctr32 = cw.ok;
    rb.ctr_chain_lo = cw.chain_lo;
    rb.ctr_step_lo = cw.step_lo;
    rb.ctr_c3 = cw.c3;
    rb.sampler = a->sampler;
    rb.max_tries = a->max_tries;
    rb.keep_rows = a->samples_chain_rows;
    if (a->placement < 0 || a->placement > 2) {
        set_error("placement must be 0 (auto), 1 (packed) or 2 (spread)");
        return GSSS_E_INVALID;
    }
    // The library's choice: one wavefront per chain while that beats the packed throughput kernels (tools/bench_placement.py,
    // fast mode, chain-steps/s packed (one chain per lane at these sizes) | spread: README mixture 3072 chains 8.3e8 | 9.0e8,
    // 4096 1.11e9 | 0.95e9; K = 10 mixture 2048 3.7e8 | 4.4e8, 3072 5.5e8 | 4.5e8; Bingham d = 10 3072 6.9e8 | 8.0e8, 4096
    // 9.2e8 | 8.4e8; curve d = 10 (group kernel) 1024 chains 1.3e8 | 2.0e8, 2048 2.6e8 | 2.0e8).
    const int64_t spread_max = a->mode != GSSS_MODE_FAST ? 2048 : (t->tb.kind == GSSS_CURVE_VMF ? 1536 : 3072);
    rb.spread = a->placement == 2 || (a->placement == 0 && a->n_chains <= spread_max) ? 1 : 0;
    rb.screen = (a->mode == GSSS_MODE_FAST && a->variant == GSSS_VARIANT_FAST_DOUBLE) ? 0 : (a->variant == GSSS_VARIANT_FAST_VERIFY ? 2 : 1);
    rb.stats = a->stats_dev;
    rb.stats_dirs = a->stats_dirs_dev;
    rb.stats_lags = a->stats_lags;
    rb.stats_modes = a->stats_modes;
    rb.stats_flags = a->stats_flags;
    if (a->stats_dev != nullptr) {
        if (!a->stats_dirs_dev || a->stats_lags < 0 || a->stats_modes < 0 || a->stats_lags > 4096 || a->stats_modes > 4096 ||
            (a->stats_flags & ~GSSS_STATS_NO_SECOND_MOMENT)) {
            set_error("stats_dev needs stats_dirs_dev, 0 <= stats_lags <= 4096, 0 <= stats_modes <= 4096 and known stats_flags");
            return GSSS_E_INVALID;
        }
        // the lane-group layouts form the d (d + 1) / 2 second-moment sums through cross-lane reads: small d only
        if (!(a->stats_flags & GSSS_STATS_NO_SECOND_MOMENT) && t->tb.d > 64) {
            set_error("second moments are accumulated for d <= 64 (d (d + 1) / 2 rows per chain): set GSSS_STATS_NO_SECOND_MOMENT");
            return GSSS_E_UNSUPPORTED;
        }
    }
    DeviceGuard guard(t->device);
    if (!guard.ok) return GSSS_E_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool replay = a->replay_dev != nullptr;
    if (replay && a->rng_state_dev) {
        set_error("replay_dev and rng_state_dev are mutually exclusive");
        return GSSS_E_INVALID;
    }

    if (is_batch(t)) {  // chain c of the launch belongs to target (chain_offset + c) / m: the launch's first target leads the blobs
        TargetBlock tbb = t->tb;
        tbb.blob += (int64_t)(a->chain_offset / (uint64_t)t->batch.m) * t->batch.stride;
        if (a->mode == GSSS_MODE_FAST) {
            if (a->n_steps > 0x7FFFFFFFll || a->thin > 0x7FFFFFFFll || a->n_chains > 0x7FFFFFFFll - 1024) {
                set_error("fast mode takes at most 2^31-1 steps / chains per call");
                return GSSS_E_INVALID;
            }
            if (a->samples_dev && !kept_rows_fit32(a->samples_chain_rows, a->n_steps, a->thin, t->tb.d)) {
                set_error("the lane-per-chain kernels keep at most 2^31-1 doubles per chain (samples_chain_rows d) and per call and chain (rows d)");
                return GSSS_E_INVALID;
            }
            FastPick pick;
            if (fast_select(fast_ask(t, rb.screen, false), pick) != GSSS_OK) return fast_refused(t);
            return fast_launch(pick, tbb, rb, t->batch, false, st);
        }
        return launch_batch_run(vec, tbb, rb, t->batch, st);
    }
    const int draws = replay ? kDrawsReplay : (a->rng_state_dev ? kDrawsNumpy : kDrawsPhilox);
    if (a->mode == GSSS_MODE_FAST) {
        FastPick pick;
        const bool numpy = a->rng_state_dev != nullptr;
        const int served = fast_select(fast_ask(t, rb.screen, rb.spread != 0, numpy, replay, rb.stats != nullptr), pick);
        if (numpy && (served != GSSS_OK || !pick.lane)) {  // a generator per chain: the lane-per-chain shapes only
            set_error("in fast mode the numpy stream is served by the lane-per-chain kernels only (gsss_variant_name: "
                      "\"fast-lane\"); use GSSS_MODE_EXACT");
            return GSSS_E_UNSUPPORTED;
        }
        if (a->n_steps > 0x7FFFFFFFll || a->thin > 0x7FFFFFFFll || a->n_chains > 0x7FFFFFFFll - 1024 ||
            a->replay_stride > 0x7FFFFFFFll) {
            set_error("fast mode takes at most 2^31-1 steps / chains per call");
            return GSSS_E_INVALID;
        }
        if (served != GSSS_OK) return fast_refused(t);
        // (the lane kernels address a kept row in 32 x 32 -> 64 bit arithmetic: kept_row, gsss_device.h)
        if (pick.lane && a->samples_dev && !kept_rows_fit32(a->samples_chain_rows, a->n_steps, a->thin, t->tb.d)) {
            set_error("the lane-per-chain kernels keep at most 2^31-1 doubles per chain (samples_chain_rows d) and per call and chain (rows d)");
            return GSSS_E_INVALID;
        }
        return fast_launch(pick, t->tb, rb, t->batch, replay, st);
    }
    if (mh) {
        if (a->rng_state_dev && (a->sampler == GSSS_RWMH || a->sampler == GSSS_MIX) && t->tb.d < 3) {
            set_error("numpy's gamma(1) is an exponential ziggurat, not restated: RWMH on numpy's stream needs d >= 3");
            return GSSS_E_UNSUPPORTED;
        }
        MhBlock mb;
        mb.stepsize = a->stepsize_dev;
        mb.n_accept = a->n_accept_dev;
        mb.momenta = a->sampler == GSSS_HMC ? a->momenta_dev : nullptr;
        mb.adapt_steps = a->adapt_steps;
        mb.n_leapfrog = a->n_leapfrog;
        mb.kind = a->sampler;
        mb.mix_alpha = a->mixing_probability;
        mb.adapt_left = a->adapt_left_dev;
        mb.n_rwmh = a->n_rwmh_dev;
        mb.momenta_samples = a->sampler == GSSS_HMC ? a->momenta_samples_dev : nullptr;
        mb.stepsize_trace = a->sampler == GSSS_HMC ? nullptr : a->stepsize_trace_dev;
        if (t->tb.kind == GSSS_CPD) return launch_cpd_mh(t->cpd_variant, draws, a->sampler, t->tb, rb, mb, st);
        if (t->tb.kind == GSSS_USER) {
            if (a->sampler == GSSS_HMC && !t->user->has_gradient) {
                set_error("spherical HMC needs the target's gradient: this user target defines no gsss_user_gradient");
                return GSSS_E_UNSUPPORTED;
            }
            return t->user->mh(draws, a->sampler, t->tb, rb, mb, st);
        }
        if (const ExactFamily *f = exact_family(t->tb.kind)) return f->mh(vec, draws, a->sampler, t->tb, rb, mb, st);
        set_error("corrupt target");
        return GSSS_E_INVALID;
    }
    if (t->tb.kind == GSSS_CPD) {
        if (a->stats_dev) {
            set_error("running statistics are not built for registration targets");
            return GSSS_E_UNSUPPORTED;
        }
        return launch_cpd_run(t->cpd_variant, draws, t->tb, rb, st);
    }
    if (const ExactFamily *f = exact_family(t->tb.kind)) return f->run(vec, draws, t->tb, rb, st);
    if (t->tb.kind == GSSS_USER) return t->user->run(draws, t->tb, rb, st);
    set_error("corrupt target");
    return GSSS_E_INVALID;
}

int gsss_batch_plan(int32_t kind, int32_t d, int32_t k, int32_t has_b, int64_t n_targets, int64_t m, int32_t *chains_per_workgroup,
                    int32_t *targets_per_workgroup, int64_t *grid, double *lane_use)
{
    (void)has_b;  // (the rows of a Bingham member hold b either way; with the all-diagonal flag in k it names the shape in full)
    BatchPlan bp;
    if (batch_plan(kind, d, k, n_targets, m, bp) != GSSS_OK) {
        set_error("no fast-mode batch kernel for kind %d, d=%d, k=%d with %lld targets of %lld chains (vMF mixtures: d = 3 .. 10 with "
                  "K <= 16, d = 11 .. 16 with K <= 10; Bingham: d = 3 .. 16)", kind, d, k, (long long)n_targets, (long long)m);
        return GSSS_E_UNSUPPORTED;
    }
    if (chains_per_workgroup) *chains_per_workgroup = bp.per_block;
    if (targets_per_workgroup) *targets_per_workgroup = bp.targets;
    if (grid) *grid = bp.grid;
    if (lane_use) *lane_use = bp.lane_use;
    return GSSS_OK;
}

int64_t gsss_piece_plan(int64_t n_chunks, int64_t resident, int64_t n_steps, int32_t *table_out, int64_t capacity)
{
    if (n_chunks < 1 || resident < 1 || n_steps < 1 || capacity < 0) {
        set_error("gsss_piece_plan: need n_chunks, resident, n_steps >= 1 and capacity >= 0 (%lld, %lld, %lld, %lld)", (long long)n_chunks,
                  (long long)resident, (long long)n_steps, (long long)capacity);
        return GSSS_E_INVALID;
    }
    const std::vector<Piece> table = piece_plan(n_chunks, resident, n_steps);
    if (table_out != nullptr) {
        if ((int64_t)table.size() > capacity) {
            set_error("gsss_piece_plan: the table has %lld pieces, the buffer holds %lld", (long long)table.size(), (long long)capacity);
            return GSSS_E_INVALID;
        }
        if (!table.empty()) memcpy(table_out, table.data(), table.size() * sizeof(Piece));
    }
    return (int64_t)table.size();
}

int gsss_last_launch(int64_t *grid_out, int32_t *slice_steps_out, double *sliced_fraction_out)
{
    if (grid_out) *grid_out = last_launch().grid;
    if (slice_steps_out) *slice_steps_out = last_launch().slice_steps;
    if (sliced_fraction_out) *sliced_fraction_out = last_launch().sliced_fraction;
    return GSSS_OK;
}

int64_t gsss_stats_rows(int32_t d, int32_t n_modes, int32_t n_lags, int32_t flags)
{
    if (d < 2 || n_modes < 0 || n_lags < 0 || (flags & ~GSSS_STATS_NO_SECOND_MOMENT)) return GSSS_E_INVALID;
    const int64_t second = (flags & GSSS_STATS_NO_SECOND_MOMENT) ? 0 : (int64_t)d * (d + 1) / 2;
    return 1 + 2 * (int64_t)d + second + 2 + n_modes + 2 + 3 * (int64_t)n_lags;
}

int64_t gsss_moments_rows(int32_t d, int32_t flags)
{
    if (d < 2 || (flags & ~GSSS_MOMENTS_DIAG)) return GSSS_E_INVALID;
    const bool diag = (flags & GSSS_MOMENTS_DIAG) != 0;
    if (!diag && d > kMomentsMaxFullDim) return GSSS_E_UNSUPPORTED;
    return 1 + moments_sums(d, diag);
}

// The checks that the per-target statistics share.  entry: the entry point's name, for the message.
static int check_chains_per_target(const char *entry, int64_t n_chains, int64_t chains_per_target)
{
    if (chains_per_target >= 1 && n_chains >= 0 && n_chains % chains_per_target == 0) return GSSS_OK;
    set_error("%s: n_chains (%lld) must be a multiple of chains_per_target (%lld) >= 1", entry, (long long)n_chains,
              (long long)chains_per_target);
    return GSSS_E_INVALID;
}

static int check_ring(const char *entry, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist)
{
    if (ring_rows >= 0 && first_row >= 0 && n_rows >= 0 && n_hist >= 0 && n_rows <= ring_rows && first_row <= ring_rows - n_rows)
        return GSSS_OK;
    set_error("%s: the rows %lld .. + %lld do not lie in a ring of %lld rows", entry, (long long)first_row, (long long)n_rows,
              (long long)ring_rows);
    return GSSS_E_INVALID;
}

int gsss_target_moments(const double *samples_dev, int64_t n_rows, int64_t n_chains, int32_t d, int64_t samples_chain_rows,
                        int64_t chains_per_target, int32_t flags, double *acc_dev, double *chain_sum_dev, int device, void *stream)
{
    if (d < 2 || (flags & ~GSSS_MOMENTS_DIAG)) {
        set_error("gsss_target_moments: need d >= 2 and known flags (d = %d, flags = %d)", d, flags);
        return GSSS_E_INVALID;
    }
    if (int rc = check_chains_per_target("gsss_target_moments", n_chains, chains_per_target)) return rc;
    if (n_rows < 0 || samples_chain_rows < 0 || (samples_chain_rows > 0 && samples_chain_rows < n_rows)) {
        set_error("gsss_target_moments: need n_rows >= 0 and samples_chain_rows 0 or >= n_rows (%lld rows, %lld per chain)",
                  (long long)n_rows, (long long)samples_chain_rows);
        return GSSS_E_INVALID;
    }
    if (!samples_dev || !acc_dev) {
        set_error("gsss_target_moments: %s is null", samples_dev ? "acc_dev" : "samples_dev");
        return GSSS_E_INVALID;
    }
    const bool diag = (flags & GSSS_MOMENTS_DIAG) != 0;
    if (!diag && d > kMomentsMaxFullDim) {
        set_error("gsss_target_moments: the full second-moment triangle is kept for d <= %d (d = %d): pass GSSS_MOMENTS_DIAG",
                  kMomentsMaxFullDim, d);
        return GSSS_E_UNSUPPORTED;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_target_moments(samples_dev, n_rows, n_chains, d, samples_chain_rows, chains_per_target, diag, acc_dev, chain_sum_dev,
                                 static_cast<hipStream_t>(stream));
}

int gsss_scalar_moments(const double *values_dev, int64_t n_rows, int64_t n_chains, int64_t chains_per_target, double *acc_dev,
                        double *chain_sum_dev, int device, void *stream)
{
    if (int rc = check_chains_per_target("gsss_scalar_moments", n_chains, chains_per_target)) return rc;
    if (n_rows < 0) {
        set_error("gsss_scalar_moments: need n_rows >= 0 (%lld)", (long long)n_rows);
        return GSSS_E_INVALID;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    if (!values_dev || !acc_dev) {
        set_error("gsss_scalar_moments: %s is null", values_dev ? "acc_dev" : "values_dev");
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    // [n_rows][1][n_chains] through the any-d diagonal kernel: acc rows count, sum v, sum v^2
    return launch_target_moments(values_dev, n_rows, n_chains, 1, 0, chains_per_target, true, acc_dev, chain_sum_dev,
                                 static_cast<hipStream_t>(stream));
}

int64_t gsss_autocov_rows(int32_t d, int32_t n_lags)
{
    if (d < 1 || n_lags < 1) return GSSS_E_INVALID;
    if (n_lags > kAutocovMaxLags) return GSSS_E_UNSUPPORTED;
    return (int64_t)d * autocov_sums(n_lags);
}

int gsss_target_autocov(const double *ring_dev, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist, int64_t n_chains,
                        int32_t d, int64_t chains_per_target, int32_t n_lags, double *acc_dev, int device, void *stream)
{
    if (d < 1 || n_lags < 1) {
        set_error("gsss_target_autocov: need d >= 1 and n_lags >= 1 (d = %d, n_lags = %d)", d, n_lags);
        return GSSS_E_INVALID;
    }
    if (int rc = check_chains_per_target("gsss_target_autocov", n_chains, chains_per_target)) return rc;
    if (int rc = check_ring("gsss_target_autocov", ring_rows, first_row, n_rows, n_hist)) return rc;
    if (n_hist > n_lags || n_hist > ring_rows - n_rows) {
        set_error("gsss_target_autocov: n_hist (%lld) exceeds n_lags (%d) or the ring's rows outside the block (%lld)",
                  (long long)n_hist, n_lags, (long long)(ring_rows - n_rows));
        return GSSS_E_INVALID;
    }
    if (n_lags > kAutocovMaxLags) {
        set_error("gsss_target_autocov: at most %d lags are kept (n_lags = %d)", kAutocovMaxLags, n_lags);
        return GSSS_E_UNSUPPORTED;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    if (!ring_dev || !acc_dev) {
        set_error("gsss_target_autocov: %s is null", ring_dev ? "acc_dev" : "ring_dev");
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_target_autocov(ring_dev, ring_rows, first_row, n_rows, n_hist, n_chains, d, chains_per_target, n_lags, acc_dev,
                                 static_cast<hipStream_t>(stream));
}

int64_t gsss_mixing_rows(int32_t n_modes, int32_t flags)
{
    if (n_modes < 0 || (flags & ~GSSS_MIXING_TRANSITIONS)) return GSSS_E_INVALID;
    if (n_modes > kMixingMaxModes) return GSSS_E_UNSUPPORTED;
    return mixing_counters(n_modes, (flags & GSSS_MIXING_TRANSITIONS) != 0);
}

int gsss_target_mixing(const double *ring_dev, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist, int64_t n_chains,
                       int32_t d, int64_t chains_per_target, const double *dirs_dev, int32_t n_modes, int32_t flags, double *step_dev,
                       int64_t *count_dev, int device, void *stream)
{
    if (d < 2 || n_modes < 0 || (flags & ~GSSS_MIXING_TRANSITIONS)) {
        set_error("gsss_target_mixing: need d >= 2, n_modes >= 0 and known flags (d = %d, n_modes = %d, flags = %d)", d, n_modes,
                  flags);
        return GSSS_E_INVALID;
    }
    if (int rc = check_chains_per_target("gsss_target_mixing", n_chains, chains_per_target)) return rc;
    if (int rc = check_ring("gsss_target_mixing", ring_rows, first_row, n_rows, n_hist)) return rc;
    if (n_hist > 1 || n_hist > ring_rows - n_rows) {
        set_error("gsss_target_mixing: n_hist (%lld) exceeds the one row of history or the ring's rows outside the block (%lld)",
                  (long long)n_hist, (long long)(ring_rows - n_rows));
        return GSSS_E_INVALID;
    }
    if (n_modes > kMixingMaxModes) {
        set_error("gsss_target_mixing: at most %d mode directions are kept (n_modes = %d)", kMixingMaxModes, n_modes);
        return GSSS_E_UNSUPPORTED;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    if (!ring_dev || !dirs_dev || !step_dev || !count_dev) {
        set_error("gsss_target_mixing: %s is null",
                  !ring_dev ? "ring_dev" : (!dirs_dev ? "dirs_dev" : (!step_dev ? "step_dev" : "count_dev")));
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_target_mixing(ring_dev, ring_rows, first_row, n_rows, n_hist, n_chains, d, chains_per_target, dirs_dev, n_modes,
                                (flags & GSSS_MIXING_TRANSITIONS) != 0, step_dev, count_dev, static_cast<hipStream_t>(stream));
}

// The shape of a target's histograms: GSSS_OK, or the code gsss_marginal_rows returns (message set for `entry`).
static int check_marginal_shape(const char *entry, int32_t n_dirs, int32_t n_bins, int32_t flags)
{
    const bool steps = (flags & GSSS_MARGINALS_STEP) != 0;
    if (n_dirs < 0 || (n_dirs == 0 && !steps) || n_bins < 2 || (flags & ~GSSS_MARGINALS_STEP)) {
        set_error("%s: need n_dirs >= 0 (>= 1 without GSSS_MARGINALS_STEP), n_bins >= 2 and known flags (n_dirs = %d, n_bins = %d, "
                  "flags = %d)", entry, n_dirs, n_bins, flags);
        return GSSS_E_INVALID;
    }
    if (n_dirs > kMarginalsMaxDirs || n_bins > kMarginalsMaxBins || marginal_series(n_dirs, steps) * n_bins > kMarginalsMaxCounters) {
        set_error("%s: at most %d directions, %d bins and %d counters per target are kept (n_dirs = %d, n_bins = %d: %lld counters)",
                  entry, kMarginalsMaxDirs, kMarginalsMaxBins, kMarginalsMaxCounters, n_dirs, n_bins,
                  (long long)(marginal_series(n_dirs, steps) * n_bins));
        return GSSS_E_UNSUPPORTED;
    }
    return GSSS_OK;
}

int64_t gsss_marginal_rows(int32_t n_dirs, int32_t n_bins, int32_t flags)
{
    if (int rc = check_marginal_shape("gsss_marginal_rows", n_dirs, n_bins, flags)) return rc;
    return marginal_series(n_dirs, (flags & GSSS_MARGINALS_STEP) != 0) * n_bins;
}

int gsss_target_marginals(const double *ring_dev, int64_t ring_rows, int64_t first_row, int64_t n_rows, int64_t n_hist,
                          int64_t n_chains, int32_t d, int64_t chains_per_target, const double *dirs_dev, int32_t n_dirs,
                          int32_t n_bins, int32_t flags, int64_t *count_dev, int device, void *stream)
{
    if (d < 2) {
        set_error("gsss_target_marginals: need d >= 2 (d = %d)", d);
        return GSSS_E_INVALID;
    }
    if (int rc = check_chains_per_target("gsss_target_marginals", n_chains, chains_per_target)) return rc;
    if (int rc = check_ring("gsss_target_marginals", ring_rows, first_row, n_rows, n_hist)) return rc;
    if (n_hist > 1 || n_hist > ring_rows - n_rows) {
        set_error("gsss_target_marginals: n_hist (%lld) exceeds the one row of history or the ring's rows outside the block (%lld)",
                  (long long)n_hist, (long long)(ring_rows - n_rows));
        return GSSS_E_INVALID;
    }
    if (int rc = check_marginal_shape("gsss_target_marginals", n_dirs, n_bins, flags)) return rc;
    if (n_rows > kMarginalsMaxRows) {
        set_error("gsss_target_marginals: a block has at most 2^23 rows (n_rows = %lld): fold it in several calls", (long long)n_rows);
        return GSSS_E_UNSUPPORTED;
    }
    if (n_rows == 0 || n_chains == 0) return GSSS_OK;
    if (!ring_dev || !count_dev || (n_dirs > 0 && !dirs_dev)) {
        set_error("gsss_target_marginals: %s is null", !ring_dev ? "ring_dev" : (!count_dev ? "count_dev" : "dirs_dev"));
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_target_marginals(ring_dev, ring_rows, first_row, n_rows, n_hist, n_chains, d, chains_per_target, dirs_dev, n_dirs,
                                   n_bins, (flags & GSSS_MARGINALS_STEP) != 0, count_dev, static_cast<hipStream_t>(stream));
}

int gsss_mode_supported(const gsss_target *t, int32_t mode)
{
    if (!t) return 0;
    if (mode == GSSS_MODE_EXACT) return select_vec(t->tb.d, 0) >= 0;
    if (mode == GSSS_MODE_FAST) {  // (every shape with a batch fast kernel has the screened and the all-double one)
        FastPick pick;
        return fast_select(fast_ask(t, is_batch(t) ? 1 : 0, false), pick) == GSSS_OK;
    }
    return 0;
}

const char *gsss_variant_name(const gsss_target *t, int32_t mode, int32_t variant)
{
    if (!t) return "";
    if (mode == GSSS_MODE_FAST) {
        FastPick pick;
        if (fast_select(fast_ask(t, is_batch(t) ? 1 : 0, false), pick) != GSSS_OK) return "";
        return pick.lane ? "fast-lane" : "fast-coop";
    }
    const int vec = select_vec_for(t->tb, variant);
    if (vec < 0) return "";
    int n;
    const VecInfo *v = vec_table(&n);
    for (int i = 0; i < n; ++i)
        if (v[i].id == vec) return v[i].name;
    return "";
}

const char *gsss_kernel_name(const gsss_target *t, int32_t mode, int32_t variant, int32_t placement)
{
    static thread_local char name[200];
    name[0] = 0;
    if (!t) return name;
    if (mode == GSSS_MODE_FAST) {  // placement 2: one wavefront per chain (a batch: one lane per chain whatever the placement)
        const int screen = variant == GSSS_VARIANT_FAST_DOUBLE ? 0 : (variant == GSSS_VARIANT_FAST_VERIFY ? 2 : 1);
        FastPick pick;
        if (fast_select(fast_ask(t, screen, placement == 2), pick) == GSSS_OK) fast_name(pick, name, sizeof(name));
        return name;
    }
    const char *vec = gsss_variant_name(t, mode, variant);
    const ExactFamily *f = exact_family(t->tb.kind);
    const char *tgt = f ? f->name : t->tb.kind == GSSS_USER ? "UserTarget" : "CurveVmf";  // (a registration handle prints CurveVmf)
    if (vec[0]) snprintf(name, sizeof(name), "run_kernel<%s, %s%s>", vec, tgt, is_batch(t) ? ", batch" : "");
    return name;
}

int gsss_sample_sphere(uint64_t seed, uint64_t chain_offset, int64_t n, int32_t d, double *state_dev, int device,
                       void *stream)
{
    if (n < 0 || d < 2 || (n > 0 && !state_dev)) {
        set_error("bad argument to gsss_sample_sphere");
        return GSSS_E_INVALID;
    }
    if (n == 0) return GSSS_OK;
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_kernel("sample_sphere", sample_sphere_kernel, ceil_div(n, kBlock), 0, static_cast<hipStream_t>(stream), nullptr,
                         seed, chain_offset, n, (int)d, state_dev);
}

int gsss_tangent_s2(const double *x_dev, const uint32_t *w_dev, int64_t n, int32_t table_driven, double *out_dev, int device, void *stream)
{
    if (n < 0 || (n > 0 && (!x_dev || !w_dev || !out_dev))) {
        set_error("bad argument to gsss_tangent_s2");
        return GSSS_E_INVALID;
    }
    if (n == 0) return GSSS_OK;
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    return launch_kernel("tangent_s2", tangent_s2_kernel, ceil_div(n, kBlock), 0, static_cast<hipStream_t>(stream), nullptr, x_dev,
                         w_dev, n, (int)table_driven, out_dev);
}

int gsss_rows_to_components(const double *in_dev, double *out_dev, int64_t n, int32_t d, int device, void *stream)
{
    return transpose(in_dev, out_dev, n, d, device, static_cast<hipStream_t>(stream));
}

int gsss_components_to_rows(const double *in_dev, double *out_dev, int64_t n, int32_t d, int device, void *stream)
{
    return transpose(in_dev, out_dev, d, n, device, static_cast<hipStream_t>(stream));
}

int gsss_samples_to_chains(const double *in_dev, double *out_dev, int64_t n, int64_t n_keep, int32_t d, int device,
                           void *stream)
{
    // [n_keep][d][n] -> [n][n_keep][d] is the transpose of an [n_keep*d][n] matrix
    return transpose(in_dev, out_dev, n_keep * d, n, device, static_cast<hipStream_t>(stream));
}

int gsss_malloc(void **out_dev, size_t bytes, int device)
{
    if (!out_dev) {
        set_error("null argument");
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipMalloc(out_dev, bytes ? bytes : 1));
    return GSSS_OK;
}

int gsss_free(void *p_dev, int device)
{
    if (!p_dev) return GSSS_OK;
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipFree(p_dev));
    return GSSS_OK;
}

int gsss_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, int device, void *stream)
{
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GSSS_HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, st));
    GSSS_HIP_TRY(hipStreamSynchronize(st));
    return GSSS_OK;
}

int gsss_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, int device, void *stream)
{
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GSSS_HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
    GSSS_HIP_TRY(hipStreamSynchronize(st));
    return GSSS_OK;
}

int gsss_malloc_host(void **out_host, size_t bytes, int device)
{
    if (!out_host) {
        set_error("null argument");
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipHostMalloc(out_host, bytes ? bytes : 1, hipHostMallocDefault));
    return GSSS_OK;
}

int gsss_free_host(void *p_host)
{
    if (!p_host) return GSSS_OK;
    GSSS_HIP_TRY(hipHostFree(p_host));
    return GSSS_OK;
}

int gsss_host_register(void *p_host, size_t bytes, int device)
{
    if (!p_host || bytes == 0) {
        set_error("bad argument to gsss_host_register");
        return GSSS_E_INVALID;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipHostRegister(p_host, bytes, hipHostRegisterDefault));
    return GSSS_OK;
}

int gsss_host_unregister(void *p_host)
{
    if (!p_host) return GSSS_OK;
    GSSS_HIP_TRY(hipHostUnregister(p_host));
    return GSSS_OK;
}

int gsss_memcpy_d2h_async(void *dst_host, const void *src_dev, size_t bytes, int device, void *stream)
{
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    return GSSS_OK;
}

int gsss_memset(void *dst_dev, int value, size_t bytes, int device, void *stream)
{
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, static_cast<hipStream_t>(stream)));
    return GSSS_OK;
}

int gsss_stream_synchronize(int device, void *stream)
{
    DeviceGuard guard(device);
    if (!guard.ok) return GSSS_E_HIP;
    GSSS_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return GSSS_OK;
}

}  // extern "C"
