"""Log normalising constants along ladders without a GPU: the host restatement (ladder_cases.host_fold, host_estimates) against
sums taken without a recurrence, the estimators of diagnostics.from_target_ladder against the restatement, the two Jensen
inequalities, TargetBatch.hot_log_z, the refusals that need no device and the resource budget of the ladder kernels."""
import math
import re

import numpy as np
import pytest
import torch

import geosss_amd as gs
import ladder_cases as lz
from geosss_amd import _lib, diagnostics, mcmc

LD = np.longdouble
E_INVALID = -1
BOGUS = 4096  # some non-NULL address that is never read


# ------------------------------------------------------------------------------------------ the restatement
def _close(got, want, tol):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    same = (got == want) | (np.isnan(got) & np.isnan(want))            # (equal infinities included)
    with np.errstate(all="ignore"):
        err = np.where(same, 0, np.abs(got - want) / np.maximum(1, np.abs(want)))
    return bool(np.all(err <= tol)), float(np.max(err))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recurrence_against_direct_sums(seed):
    """host_fold's (M, S) against a maximum and one sum over the used rows, on tables with NaN and infinite entries, a first
    draw that is the maximum, and a chain that is never used; counts exact."""
    ladder = 4
    lp3 = lz.synthetic_table(seed, ladder=ladder)
    acc = lz.host_fold(lp3, ladder)
    want = lz.direct_sums(lp3, ladder)
    assert acc.shape == (2, ladder - 1, 5, 10)
    assert np.array_equal(acc[..., 0], want["used"]) and np.array_equal(acc[..., 9], want["skipped"])
    assert np.all(acc[..., 0] + acc[..., 9] == lp3.shape[0])
    # what the table was built to contain
    assert acc[0, 0, 2, 9] == 1 and acc[0, 1, 2, 9] == 1 and acc[0, 0, 1, 9] == 1 and acc[0, 1, 0, 9] == 1
    assert acc[1, 0, 4, 0] == 0 and acc[1, 0, 4, 9] == lp3.shape[0] and acc[1, 0, 4, 1] == -np.inf and acc[1, 0, 4, 2] == 0
    assert int(acc[..., 9].sum()) == 6 + lp3.shape[0]
    assert acc[0, 2, 1, 1] > 300 and acc[0, 2, 3, 1] > 300          # the first and the last draw as the maximum
    with np.errstate(all="ignore"):
        lse_u, lse_v = acc[..., 1] + np.log(acc[..., 2]), acc[..., 5] + np.log(acc[..., 6])
    lse_u, lse_v = np.where(acc[..., 0] > 0, lse_u, -np.inf), np.where(acc[..., 0] > 0, lse_v, -np.inf)
    for got, key in ((lse_u, "lse_u"), (lse_v, "lse_v"), (acc[..., 3], "sum_u"), (acc[..., 4], "sum_uu"), (acc[..., 7], "sum_v"),
                     (acc[..., 8], "sum_vv")):
        ok, err = _close(got, want[key], 1e-15)
        assert ok, (key, err)
    assert np.all(np.isfinite(acc[..., 2])) and np.all(np.isfinite(acc[..., 6]))       # no -inf - (-inf) was formed


def test_fold_continues():
    """Rows in calls of 3 and 2 and of 1 + 4: the same accumulators as the five rows at once, to the last bit."""
    lp3 = lz.synthetic_table(5, rows=8)[:5]
    whole = lz.host_fold(lp3, 4)
    for cut in (3, 1, 0, 5):
        parts = lz.host_fold(lp3[cut:], 4, acc=lz.host_fold(lp3[:cut], 4))
        assert np.array_equal(whole, parts, equal_nan=True), cut


@pytest.mark.parametrize("seed", [1, 2])
def test_estimators_and_jensen(seed):
    """from_target_ladder (CPU tensors, double) against the longdouble restatement, and the two exact inequalities
    log_z_lower <= log_z_ratio_forward, log_z_ratio_backward <= log_z_upper for the very sample, in both."""
    lp3 = lz.synthetic_table(seed, rows=60, ladder=4)
    lp3[0, 2, 1, 2] -= 400.0                          # (moderate weights here: the two outliers of the table are taken back)
    lp3[-1, 2, 3, 2] -= 400.0
    acc = lz.host_fold(lp3, 4)
    acc64 = np.where(np.isfinite(acc[..., :]), acc, 0).astype(np.float64)       # (the device's start: zeros, not -inf)
    hot = np.array([1.5, -2.25])
    want = lz.host_estimates(acc, hot)
    got = diagnostics.from_target_ladder(torch.from_numpy(acc64), hot_log_z=hot)
    assert set(got) == set(want)
    for key, val in got.items():
        ok, err = _close(val.numpy(), want[key], 1e-12)
        assert ok, (key, err)
    assert tuple(got["log_z"].shape) == (2, 4) and np.array_equal(got["log_z"][:, -1].numpy(), hot)
    assert torch.equal(got["log_z_ratio"], got["log_z_ratio_forward"])
    # a NaN hot constant (the hottest rung is not flat) leaves that ladder relative to its hottest rung
    rel = diagnostics.from_target_ladder(torch.from_numpy(acc64), hot_log_z=np.array([np.nan, -2.25]))["log_z"]
    assert torch.equal(rel[1], got["log_z"][1]) and rel[0, -1] == 0 and torch.equal(rel[0], diagnostics.from_target_ladder(torch.from_numpy(acc64))["log_z"][0])
    # log Z of rung r is the hot constant plus the forward ratios of the pairs r .. R - 2
    f = got["log_z_ratio_forward"].numpy()
    assert np.allclose(got["log_z"][:, 0].numpy(), hot + f.sum(1), rtol=0, atol=1e-12)
    # ladder 1, pair 0 has a chain without a used draw: it counts in nothing
    assert want["used"][1, 0] == 4 * 60 - 1 and np.isfinite(got["log_z_ratio_forward"][1, 0])
    for est in (want, {k: v.numpy() for k, v in got.items()}):
        assert np.all(est["log_z_lower"] <= est["log_z_ratio_forward"])
        assert np.all(est["log_z_ratio_backward"] <= est["log_z_upper"])
    # the between-chain standard error is the spread of the per-chain estimates
    with np.errstate(all="ignore"):
        per = (acc[0, 1, :, 1] + np.log(acc[0, 1, :, 2]) - np.log(acc[0, 1, :, 0])).astype(np.float64)
    assert abs(float(got["log_z_ratio_se"][0, 1]) - per.std(ddof=1) / math.sqrt(5)) < 1e-12


def test_known_ratio_from_a_table():
    """u constant: exp u = Z_a / Z_b for every draw, so both estimates and both bounds are that constant."""
    rows, M, m = 7, 2, 3
    lp3 = np.zeros((rows, M, m, 3))
    lp3[:, 0, :, 2] = 2.5              # l_0(x_1) - l_1(x_1) = 2.5
    lp3[:, 1, :, 1] = -2.5             # l_1(x_0) - l_0(x_0) = -2.5
    est = lz.host_estimates(lz.host_fold(lp3, 2))
    for key in ("log_z_ratio", "log_z_ratio_backward", "log_z_lower", "log_z_upper"):
        assert abs(float(est[key][0, 0]) - 2.5) < 1e-15, key
    assert est["log_z_ratio_se"][0, 0] < 1e-15 and est["used"][0, 0] == rows * m
    assert abs(float(est["log_z"][0, 0]) - 2.5) < 1e-15 and est["log_z"][0, 1] == 0


# ------------------------------------------------------------------------------------------ hot_log_z
def _log_area(d):
    return math.log(2.0) + 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d)


def _sym(d, seed):
    a = np.random.default_rng(seed).standard_normal((d, d))
    return a + a.T


@pytest.mark.parametrize("d", [3, 5, 16])
def test_hot_log_z_of_a_flat_bingham(d):
    b = np.arange(1.0, d + 1.0)
    flat = gs.TargetBatch.tempered([gs.Bingham(_sym(d, 1)), gs.Bingham(_sym(d, 2))], [1.0, 0.5, 0.0])
    assert np.array_equal(flat.hot_log_z(), [0.0 + _log_area(d)] * 2)
    assert abs(_log_area(3) - math.log(4 * math.pi)) < 1e-15
    fb = gs.TargetBatch.tempered(gs.BinghamFisher(_sym(d, 3), b), [1.0, 0.5, 0.0])
    assert np.array_equal(fb.hot_log_z(), [_log_area(d)])
    warm = gs.TargetBatch.tempered(gs.Bingham(_sym(d, 1)), [1.0, 0.5, 0.25])
    assert np.isnan(warm.hot_log_z()).all() and warm.hot_log_z().shape == (1,)
    # constancy is decided from A and b: a zero A with a linear term is not flat
    assert np.isnan(gs.TargetBatch([gs.BinghamFisher(_sym(d, 3), b), gs.BinghamFisher(np.zeros((d, d)), b)]).hot_log_z(2)).all()
    # the ladder is the argument's where given: six members as three ladders of two, the middle one ending flat
    six = gs.TargetBatch([gs.Bingham(_sym(d, 1)), gs.Bingham(_sym(d, 2)), gs.Bingham(_sym(d, 3)), gs.Uniform(d), gs.Bingham(_sym(d, 4)),
                          gs.Bingham(_sym(d, 5))])
    got = six.hot_log_z(2)
    assert np.isnan(got[0]) and got[1] == _log_area(d) and np.isnan(got[2])
    with pytest.raises(ValueError, match="ladder"):
        six.hot_log_z()
    with pytest.raises(ValueError, match="whole ladders"):
        six.hot_log_z(4)


def test_hot_log_z_of_vmf_members():
    """mu = 0 packs: the vMF's constant -log 2 pi - log i0(0) is part of its log-density, and of the value."""
    vmf = gs.TargetBatch.tempered(gs.VonMisesFisher(np.array([0.0, 3.0, 4.0])), [1.0, 0.5, 0.0])
    assert abs(vmf.hot_log_z()[0] - (-math.log(2 * math.pi) + _log_area(3))) < 1e-15
    assert np.isnan(gs.TargetBatch.tempered(gs.VonMisesFisher(np.array([0.0, 3.0, 4.0])), [1.0, 0.5]).hot_log_z()).all()
    mix = gs.MixtureModel([gs.VonMisesFisher(np.array([5.0, 0.0, 0.0])), gs.VonMisesFisher(np.array([0.0, 2.0, 0.0]))], [1.0, 3.0])
    lad = gs.TargetBatch.tempered(mix, [1.0, 0.0])
    assert abs(lad.hot_log_z()[0] - (-math.log(2 * math.pi) + _log_area(3))) < 1e-14        # (the weights sum to one)


# ------------------------------------------------------------------------------------------ refusals
def test_symbols_and_sizes():
    lib = _lib.load()
    for name in ("gsss_batch_ladder", "gsss_ladder_scratch_doubles", "gsss_ladder_acc_doubles"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.gsss_abi_version() == _lib.ABI_VERSION
    assert lib.gsss_ladder_scratch_doubles(16, 1000) == 48000 and lib.gsss_ladder_scratch_doubles(0, 1000) == 0
    assert lib.gsss_ladder_scratch_doubles(-1, 10) == E_INVALID and lib.gsss_ladder_scratch_doubles(1, -10) == E_INVALID
    assert lib.gsss_ladder_scratch_doubles(2 ** 40, 2 ** 40) == E_INVALID
    assert lib.gsss_ladder_acc_doubles(6 * 7, 7, 3) == 2 * 2 * 7 * 10 and lib.gsss_ladder_acc_doubles(0, 7, 3) == 0
    for args in ((6 * 7, 7, 1), (6 * 7, 0, 3), (-42, 7, 3), (5 * 7, 7, 3), (6 * 7 + 1, 7, 3)):
        assert lib.gsss_ladder_acc_doubles(*args) == E_INVALID, args


# (handle, n_rows, n_chains, target0, ladder) -> the word its message carries
@pytest.mark.parametrize("args, word", [
    ((1, 5, 24, 0, 1), "ladder"),           # ladder < 2
    ((1, 5, 24, 0, 0), "ladder"),
    ((1, 5, 24, 0, -3), "ladder"),
    ((1, 5, 24, 4, 3), "target0"),          # target0 no multiple of the ladder
    ((1, 5, 24, -3, 3), "target0"),
    ((1, 5, -24, 0, 3), "n_chains"),
    ((1, -5, 24, 0, 3), "n_rows"),
    ((0, 5, 24, 0, 3), "null handle"),
])
def test_batch_ladder_refusals_need_no_device(args, word):
    lib = _lib.load()
    h, rows, n, t0, ladder = args
    rc = lib.gsss_batch_ladder(BOGUS if h else None, BOGUS, rows, n, t0, ladder, BOGUS, BOGUS, None)
    assert rc == E_INVALID and word in lib.gsss_last_error().decode()


class _NoDevice(mcmc.ShrinkageSphericalSliceSampler):
    """The sampler's argument checks, which come before anything touches a device, on an object that has none."""

    def __init__(self, batch_m, n_chains, chain_offset=0, target=None):
        self._batch_m, self.n_chains, self.chain_offset, self.d = batch_m, n_chains, chain_offset, 3
        if target is not None:
            self.target = target


def test_summarize_refusals():
    single = _NoDevice(None, 64)
    for log_z in (True, dict(ladder=2)):
        with pytest.raises(ValueError, match="holds no TargetBatch"):
            single.summarize(4, log_z=log_z)
    with pytest.raises(ValueError, match="holds no TargetBatch"):        # worded like log_prob=True's: it names the remedy
        single.summarize(4, log_z=True, exchange=dict(ladder=2, every=1))
    plain = gs.TargetBatch([gs.VonMisesFisher(np.array([1.0, 2.0, k])) for k in range(6)])
    s = _NoDevice(8, 6 * 8, target=plain)
    with pytest.raises(ValueError, match="batch.ladder"):                # neither exchange= nor a tempered batch
        s.summarize(4, log_z=True)
    with pytest.raises(ValueError, match="dict"):
        s.summarize(4, log_z=dict(rungs=3))
    with pytest.raises(ValueError, match="dict"):
        s.summarize(4, log_z=3)
    with pytest.raises(ValueError, match="whole ladders"):               # M = 6 is no multiple of 4
        s.summarize(4, log_z=dict(ladder=4))
    with pytest.raises(ValueError, match="whole ladders"):
        s.summarize(4, log_z=dict(ladder=1))
    with pytest.raises(ValueError, match="different ladders"):
        s.summarize(4, log_z=dict(ladder=2), exchange=dict(ladder=3, every=1))
    with pytest.raises(ValueError, match="whole ladders"):               # a shard that starts inside a ladder
        _NoDevice(8, 6 * 8, chain_offset=8, target=plain).summarize(4, log_z=dict(ladder=3))
    tempered = gs.TargetBatch.tempered(gs.VonMisesFisher(np.array([1.0, 2.0, 3.0])), [1.0, 0.5, 0.25, 0.1])
    with pytest.raises(ValueError, match="whole ladders"):               # batch.ladder = 4 is taken, and 6 members are not 4 k
        _NoDevice(8, 6 * 8, target=tempered).summarize(4, log_z=True)


def test_target_ladder_refusals():
    batch = gs.TargetBatch([gs.VonMisesFisher(np.array([1.0, 2.0, k])) for k in range(6)])
    with pytest.raises(ValueError, match="CUDA float64"):
        diagnostics.target_ladder(batch, torch.zeros((5, 3, 12), dtype=torch.float64), 3)
    with pytest.raises(ValueError, match=r"\(G, R - 1, m, 10\)"):
        diagnostics.from_target_ladder(torch.zeros((2, 2, 4, 9), dtype=torch.float64))


# ------------------------------------------------------------------------------------------ resource budget
def _layout_family(name, pattern):
    """The template arguments <V, TT> of a mangled kernel name."""
    m = re.search(pattern, name)
    return m.group(1) if m else None


# The one build that misses exchange_eval_kernel's wavefronts per SIMD in the same layout and family, held to its own figure
# (DESIGN.md 5.6j): the Bingham target at ten components a lane holds the hundred products' operands and comes out at 74 vector
# registers around the row loop, two past the 72 that seven wavefronts allow.
OWN_WAVES = {"NS_7LaneVecILi10EEENS_7BinghamE": 6}


def test_resource_budget():
    """The 30 builds of ladder_eval_kernel (15 layouts x {VmfMixture, Bingham}) against exchange_eval_kernel in the same layout
    and family: no scratch memory at all, no fewer wavefronts per SIMD (OWN_WAVES: those held to their own figure); the fold
    kernel spills nothing and runs eight wavefronts."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_ladder.hip")
    evals = {_layout_family(k, r"18ladder_eval_kernelI(.+)EEvNS_11TargetBlockE"): r for k, r in ru.items() if "ladder_eval_kernel" in k}
    folds = [r for k, r in ru.items() if "ladder_fold_kernel" in k]
    assert len(ru) == 31 and len(evals) == 30 and None not in evals and len(folds) == 1, sorted(ru)
    parent = {}
    for name, r in build.resource_usage("gsss_exchange.hip").items():
        key = _layout_family(name, r"20exchange_eval_kernelI(.+)EEvNS_11TargetBlockE")
        if key is not None:
            parent[key] = r
    assert len(parent) == 30 and set(parent) == set(evals), (sorted(parent), sorted(evals))
    for key, r in sorted(evals.items()):
        p = parent[key]
        print(f"{key}: vgprs {r['vgprs']} ({p['vgprs']}), scratch {r['scratch']} ({p['scratch']}), waves {r['occupancy']} ({p['occupancy']})")
        waves = OWN_WAVES.get(key, p["occupancy"])
        assert r["scratch"] == 0 and r["occupancy"] >= waves, (key, r, p)
    print("fold:", folds[0])
    assert folds[0]["scratch"] == 0 and folds[0]["occupancy"] >= 8
