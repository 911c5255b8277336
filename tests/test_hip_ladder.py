"""Log normalising constants along ladders on the device (gsss_batch_ladder; diagnostics.target_ladder, summarize(log_z=)).

The accumulators are held to ladder_cases.host_fold (numpy longdouble) fed with TargetBatch.log_prob's values of the same rows;
cuts into calls, sub-ranges of ladders and the skip rule to the device's own bits; summarize(log_z=) to sample() + target_ladder
bit for bit; and the estimate to two constants known in closed form, within five standard errors that the test takes itself, in
numpy, from the draws of a second run -- never from the code under test -- and that must stay under 0.15."""
import math

import numpy as np
import pytest
import torch

import geosss_amd as gs
import ladder_cases as lz
from geosss_amd import diagnostics

pytestmark = pytest.mark.gpu

LD = np.longdouble
_device_rows = lz.device_rows


# ------------------------------------------------------------------------------------------ device against host restatement
@pytest.mark.parametrize("key", lz.cases(), ids=lz.case_id)
def test_accumulators_against_the_host_restatement(key):
    """ladder_cases.check_accumulators: the counts equal, the six quantities within ladder_cases.TOL (1e-10, device against
    host: only exp differs), chain_major the same bits."""
    lz.check_accumulators(key)


SHARED = [("vmf3", "lane"), ("binghamfisher", "coop16"), lz.GLOBAL]


@pytest.mark.parametrize("key", SHARED, ids=lz.case_id)
def test_split_blocks_and_repeat(key):
    """5 rows in one call equal 3 + 2 rows and 1 + 4 rows, and a second run of the same call, bit for bit."""
    pdfs, m, x = lz.case_rows(key)
    batch = gs.TargetBatch(list(pdfs))
    xt = _device_rows(x)
    whole = diagnostics.target_ladder(batch, xt, lz.R)
    assert torch.equal(whole, diagnostics.target_ladder(batch, xt, lz.R))
    for cut in (3, 1):
        parts = diagnostics.target_ladder(batch, xt[:cut], lz.R)
        back = diagnostics.target_ladder(batch, xt[cut:], lz.R, acc=parts)
        assert back is parts and torch.equal(whole, parts), cut
    assert float(whole[..., 0].min()) == lz.N_ROWS


@pytest.mark.parametrize("key", SHARED, ids=lz.case_id)
def test_second_ladder_alone(key):
    """target0 = R, the second ladder's chains alone: the second ladder's slice of the whole call, bit for bit."""
    pdfs, m, x = lz.case_rows(key)
    batch = gs.TargetBatch(list(pdfs))
    xt = _device_rows(x)
    whole = diagnostics.target_ladder(batch, xt, lz.R)
    tgt = batch._device_target(xt.device, chains_per_target=m)
    n = lz.R * m
    sub = xt[:, :, n:].contiguous()
    acc = torch.zeros((1, lz.R - 1, m, 10), dtype=torch.float64, device="cuda")
    scratch = torch.empty(int(tgt.lib.gsss_ladder_scratch_doubles(lz.N_ROWS, n)), dtype=torch.float64, device="cuda")
    assert acc.numel() == tgt.lib.gsss_ladder_acc_doubles(n, m, lz.R)
    diagnostics._ladder_fold(tgt.handle, tgt.lib, sub, lz.N_ROWS, n, lz.R, lz.R, scratch, acc)
    assert torch.equal(acc[0], whole[1]) and not torch.equal(whole[0], whole[1])


@pytest.mark.parametrize("key", SHARED, ids=lz.case_id)
def test_skip_rule(key):
    """One chain's row set to NaN: one skipped draw for exactly the pairs that chain enters, every other pair-chain unchanged."""
    pdfs, m, x = lz.case_rows(key)
    batch = gs.TargetBatch(list(pdfs))
    clean = diagnostics.target_ladder(batch, _device_rows(x), lz.R)
    bad = x.copy()
    chain, row = 3, 2
    bad[row, 1 * m + chain, :] = np.nan             # ladder 0, the middle rung: the pairs (0, 1) and (1, 2)
    got = diagnostics.target_ladder(batch, _device_rows(bad), lz.R)
    hit = torch.zeros(clean.shape[:3], dtype=torch.bool, device="cuda")
    hit[0, :, chain] = True
    assert torch.equal(got[~hit], clean[~hit])
    assert torch.all(got[hit][:, 9] == 1) and torch.all(got[hit][:, 0] == lz.N_ROWS - 1)
    assert float(got[..., 9].sum()) == 2 and torch.isfinite(got).all()
    # the four rows that were used give what they give alone
    rest = diagnostics.target_ladder(batch, _device_rows(np.delete(x, row, axis=0)), lz.R)
    assert torch.equal(got[hit][:, :9], rest[hit][:, :9])


# ------------------------------------------------------------------------------------------ summarize against sample
def _tempered(m=40, G=2, seed=5):
    """Two tempered ladders of three vMF mixtures at d = 5, m chains a rung (a rung spans wavefronts, a ladder workgroups)."""
    import batch_layout_cases as bc
    pdfs = bc.members("vmf3", 5)[:G]
    batch = gs.TargetBatch.tempered(list(pdfs), [1.0, 0.5, 0.2])
    x = bc.points("ladder-summarize", 1, len(batch) * m, 5)[0]
    return batch, (lambda: gs.ShrinkageSphericalSliceSampler(batch, x, seed=seed))


@pytest.mark.parametrize("kw", [dict(), dict(exchange=dict(ladder=3, every=2)), dict(lags=2), dict(window=2),
                                dict(lags=2, window=2, exchange=dict(ladder=3, every=2))],
                         ids=["plain", "exchange", "ring", "window", "all"])
def test_summarize_against_sample(kw):
    batch, make = _tempered()
    tm = make().summarize(6, burnin=2, log_z=True, **kw)
    ex = {k: v for k, v in kw.items() if k == "exchange"}
    draws = make().sample(6, burnin=2, as_tensor=True, **ex)
    want = diagnostics.target_ladder(batch, draws, 3, chain_major=True)
    assert tm.ladder == 3 and torch.equal(tm.ladder_acc, want) and float(want[..., 0].min()) == 6
    # (stats() of a summary with lags=2 stops in the autocorrelation's pair sums, which need three lags: the ring cases take
    # the ladder's part of stats() alone)
    st = tm.stats() if "lags" not in kw else dict(diagnostics.from_target_ladder(tm.ladder_acc, hot_log_z=tm.ladder_hot_log_z),
                                                  hot_log_z=torch.as_tensor(tm.ladder_hot_log_z))
    ref = diagnostics.from_target_ladder(want)
    assert torch.equal(st["log_z_ratio"], ref["log_z_ratio"]) and tuple(st["log_z"].shape) == (2, 3)
    # beta = 0.2, the hottest rung is not flat: log_z is relative to it
    assert torch.isnan(st["hot_log_z"]).all() and torch.all(st["log_z"][:, -1] == 0) and torch.isfinite(st["log_z"]).all()
    assert torch.all(st["log_z_lower"] <= st["log_z_ratio_forward"]) and torch.all(st["log_z_ratio_backward"] <= st["log_z_upper"])


def test_summarize_continues_and_takes_the_ladder_from_its_arguments():
    batch, make = _tempered()
    one = make().summarize(7, burnin=2, log_z=dict(ladder=3))
    s = make()
    first = s.summarize(4, burnin=2, log_z=True)
    both = s.summarize(3, burnin=1, into=first)                      # (a summary that carries the sums goes on carrying them)
    # (the moments add per-window partial sums, so they agree to rounding; the ladder's sums are the same bits in any cut)
    assert both is first and torch.equal(one.ladder_acc, both.ladder_acc) and torch.allclose(one.acc, both.acc, rtol=1e-13, atol=1e-13)
    plain = make().summarize(7, burnin=2)
    assert plain.ladder_acc is None and "log_z" not in plain.stats() and torch.equal(plain.acc, one.acc)
    with pytest.raises(ValueError, match="cannot take them up"):
        make().summarize(3, burnin=1, into=plain, log_z=True)
    # a batch without a ladder of its own: exchange= names it
    bare = gs.TargetBatch(list(batch.pdfs))
    x = make().state_rows().cpu().numpy()
    tm = gs.ShrinkageSphericalSliceSampler(bare, x, seed=5).summarize(6, burnin=2, log_z=True, exchange=dict(ladder=3, every=2))
    want = make().summarize(6, burnin=2, log_z=True, exchange=dict(ladder=3, every=2))
    assert torch.equal(tm.ladder_acc, want.ladder_acc)


# ------------------------------------------------------------------------------------------ truth
SE_CAP = 0.15   # the condition on the test's own standard error: with per-draw weight CV <= 1.02 a rung (quadrature, for the
                # coarser halving ladder) and >= 1000 effective draws a rung, a rung's SE is <= 0.033 and eleven rungs' <= 0.11


def _own_standard_error(batch, draws, m, R):
    """From the draws (N, rows, d) of a sample() run, in numpy: per pair the per-chain forward estimates
    log mean_r exp(l_a(x_b) - l_b(x_b)) from TargetBatch.log_prob, their standard deviation / sqrt(m); -> (the standard errors
    (R - 1,), their sum in quadrature, the ratio estimates (R - 1,) pooled over the chains)."""
    N, rows, d = draws.shape
    xm = draws.reshape(R, m * rows, d)
    own = batch.log_prob(np.ascontiguousarray(xm)).reshape(R, m, rows)
    up = batch.log_prob(np.ascontiguousarray(xm[np.minimum(np.arange(R) + 1, R - 1)])).reshape(R, m, rows)   # l_t at x_{t+1}
    u = (up[:-1] - own[1:]).astype(LD)                                   # (R - 1, m, rows)
    top = u.max(axis=2, keepdims=True)
    per_chain = (top[..., 0] + np.log(np.mean(np.exp(u - top), axis=2))).astype(np.float64)
    se = per_chain.std(axis=1, ddof=1) / math.sqrt(m)
    top = u.max(axis=(1, 2), keepdims=True)
    pooled = (top[:, 0, 0] + np.log(np.mean(np.exp(u - top), axis=(1, 2)))).astype(np.float64)
    return se, float(np.sqrt(np.sum(se * se))), pooled


def _log_area(d):
    return math.log(2.0) + 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d)


def test_bingham_normaliser():
    """Truth 1: exact powers and a flat hottest rung.  Bingham(20 mu mu^T) at d = 5: Z(kappa) = area(S^3) int_{-1}^{1}
    exp(kappa t^2) (1 - t^2) dt; log Z(20) - log Z(0) = 13.7761 before adding log area(S^4)."""
    from scipy.integrate import quad
    d, kappa, m = 5, 20.0, 64
    mu = np.zeros(d)
    mu[0] = 1.0
    betas = np.concatenate([0.7 ** np.arange(10), [0.0]])
    R = len(betas)
    batch = gs.TargetBatch.tempered(gs.Bingham(kappa * np.outer(mu, mu)), betas)
    x0 = lz.lc._unit(np.random.default_rng(11).standard_normal((R * m, d)))
    ex = dict(ladder=R, every=2)
    tm = gs.ShrinkageSphericalSliceSampler(batch, x0, seed=21).summarize(200, burnin=100, exchange=ex, log_z=True)
    st = tm.stats()
    integral = quad(lambda t: math.exp(kappa * (t * t - 1.0)) * (1.0 - t * t), -1.0, 1.0, epsabs=0.0, epsrel=1e-12)[0]
    truth = _log_area(4) + math.log(integral) + kappa
    flat = quad(lambda t: 1.0 - t * t, -1.0, 1.0)[0]
    assert abs(_log_area(4) + math.log(flat) - _log_area(5)) < 1e-12 and abs(truth - _log_area(5) - 13.7761) < 1e-4
    assert float(st["hot_log_z"][0]) == _log_area(5) and float(st["log_z"][0, R - 1]) == _log_area(5)
    draws = gs.ShrinkageSphericalSliceSampler(batch, x0, seed=21).sample(200, burnin=100, exchange=ex)
    se, total, pooled = _own_standard_error(batch, draws, m, R)
    got = float(st["log_z"][0, 0])
    print(f"log Z: {got:.4f}, truth {truth:.4f}, deviation {got - truth:+.4f}, own SE {total:.4f} (per rung {np.round(se, 4)}), "
          f"reported SE {float(torch.sqrt((st['log_z_ratio_se'] ** 2).sum())):.4f}, skipped {float(st['skipped'].sum())}")
    assert total < SE_CAP
    assert abs(got - truth) <= 5.0 * total
    # the same draws give the same ratios through numpy (only exp and the order of the sums differ)
    assert np.allclose(st["log_z_ratio"][0].cpu().numpy(), pooled, rtol=0, atol=1e-9)
    assert float(st["used"].min()) == 200 * m and float(st["skipped"].sum()) == 0


def test_vmf_normaliser_with_the_library_constants():
    """Truth 2: no flat rung; the library's -log 2 pi - log i0(kappa) is part of the log-density, so log Z of rung r is
    log(4 pi sinh(kappa_r) / kappa_r) + (l_r(e_0) - kappa_r), and the sum of the ratios is the difference of the two ends'."""
    d, kappa, m = 3, 15.0, 64
    e0 = np.zeros(d)
    e0[0] = 1.0
    betas = 0.7 ** np.arange(8)
    R = len(betas)
    batch = gs.TargetBatch.tempered(gs.VonMisesFisher(kappa * e0), betas)
    x0 = lz.lc._unit(np.random.default_rng(12).standard_normal((R * m, d)))
    ex = dict(ladder=R, every=2)
    st = gs.ShrinkageSphericalSliceSampler(batch, x0, seed=22).summarize(200, burnin=100, exchange=ex, log_z=True).stats()
    at_e0 = batch.log_prob(np.tile(e0, (R, 1, 1)))[:, 0]
    k = kappa * betas
    log_z = np.log(4.0 * np.pi) + (k + np.log1p(-np.exp(-2.0 * k)) - np.log(2.0 * k)) + (at_e0 - k)      # log sinh k = k + log((1 - e^-2k) / 2)
    truth = log_z[0] - log_z[R - 1]
    assert torch.isnan(st["hot_log_z"]).all()
    got = float(st["log_z"][0, 0] - st["log_z"][0, R - 1])
    draws = gs.ShrinkageSphericalSliceSampler(batch, x0, seed=22).sample(200, burnin=100, exchange=ex)
    se, total, pooled = _own_standard_error(batch, draws, m, R)
    print(f"log Z_0 - log Z_7: {got:.4f}, truth {truth:.4f}, deviation {got - truth:+.4f}, own SE {total:.4f} (per rung {np.round(se, 4)})")
    assert total < SE_CAP
    assert abs(got - truth) <= 5.0 * total
    assert np.allclose(st["log_z_ratio"][0].cpu().numpy(), pooled, rtol=0, atol=1e-9)
