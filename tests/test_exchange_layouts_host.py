"""The conditions of the exchange and ladder layout sweep (test_hip_exchange_layouts.py), stated without a GPU: the sweep's dims
name all fifteen layouts and no case moves to a global-row layout; no pair of any new exchange case lies within
exchange_cases.MARGIN of its decision, and both decisions, the error pair and the NaN pair occur in every one; the ladder cases
use every row, and the host restatement they are held to agrees with sums taken without a recurrence on tables of
reference_math values; the flat hottest rungs are flat; and the oracle's stream at chain and step ids above 2^32 is the counter
layout of DESIGN.md section 3, restated here."""
import math

import numpy as np
import pytest

import batch_layout_cases as bc
import exchange_cases as ec
import ladder_cases as lz
import reference_math as rm

LD = np.longdouble
NEW_SWEEPS = ec.layout_cases() + ec.flat_cases()


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    lz.release()    # (dense members at d >= 1025 are 33 MB each)


# ------------------------------------------------------------------------------------------ what the sweep reaches
def test_sweep_dims_name_every_layout():
    dims = ec.layout_dims()
    assert [bc.natural_layout(d) for d in dims if bc.lanes(bc.natural_layout(d)) == 1] == bc.LAYOUTS[:7]   # a lane layout: one d
    assert {bc.natural_layout(d) for d in dims} == set(bc.LAYOUTS) and len(bc.LAYOUTS) == 15
    for name in bc.LAYOUTS[7:]:                                 # a cooperative layout: a ragged d and a full one
        ds = [d for d in dims if bc.natural_layout(d) == name]
        assert len(ds) == 2 and ds[0] < ds[1] == bc.DPAD[name], (name, ds)     # (the full d fills the padded row)
        assert ds[1] == max(d for d in bc.DIMS if bc.natural_layout(d) == name) and ds[0] == min(d for d in bc.DIMS if bc.natural_layout(d) == name)
    assert len(dims) == 23 and set(dims) <= set(bc.DIMS)
    assert len(ec.layout_cases()) == 46 and len(lz.layout_cases()) == 46
    # one flat case per layout family and target policy
    assert [bc.layout_family(bc.natural_layout(d)) for d in ec.flat_dims()] == ["lane", "coop4", "coop16", "coop64"]
    assert ec.flat_dims() == (5, 17, lz.shapes()["coop16"][0], 130)


@pytest.mark.parametrize("key", ec.layout_cases(), ids=ec.case_id)
def test_no_sweep_case_moves_to_a_global_row_layout(key):
    family, d = key
    layout = bc.natural_layout(d)
    # (a dense member above d = 128 has its rows in global memory in its own sixty-four-lane layout: that moves nothing)
    assert bc.layout_of((family, d, ec.SWEEP_R * ec.SWEEP_G)) == layout
    assert bc.rows_in_lds((family, d, ec.SWEEP_R * ec.SWEEP_G)) == (family == "vmf3" or d <= 128)
    assert ec.sweep_m(key) == bc.chains_per_target(layout) == lz.case_m(("layout",) + key) == bc.BLOCK // bc.lanes(layout) + 3


@pytest.mark.parametrize("key", ec.flat_cases(), ids=ec.case_id)
def test_flat_cases_stay_in_their_layout_and_end_flat(key):
    _, family, d = key
    batch = ec.flat_batch(family, d)
    layout = bc.natural_layout(d)
    assert len(batch) == 6 and batch.ladder == 3 and np.array_equal(batch.betas, ec.FLAT_BETAS)
    dpad = bc.DPAD.get(layout, d)
    assert dpad >= 256 or bc.row_doubles(batch.pdfs, dpad) * 8 <= bc.ROWS_LDS_BYTES   # (layout_of's rule: the layout stays)
    assert ec.sweep_m(key) == lz.case_m(key) == bc.chains_per_target(layout)
    assert ec.sweep_members(key) == lz.case_members(key)                        # the same objects
    for g in range(2):
        hot = batch.pdfs[3 * g + 2]
        if family == "vmf3":
            assert len(hot.pdfs) == 3 and not any(np.any(p.mu) for p in hot.pdfs)
        else:
            assert not np.any(hot.A) and not np.any(hot.b)
        assert np.any(batch.pdfs[3 * g + 1].pdfs[0].mu if family == "vmf3" else batch.pdfs[3 * g + 1].A)
    assert np.all(np.isfinite(batch.hot_log_z()))


# ------------------------------------------------------------------------------------------ exchange: the decision margin
def _sweep_conditions(key):
    """-> the pairs the draw refused.  test_exchange_host.py::test_sweep_cases_keep_the_decision_margin's conditions."""
    pdfs, m, x, err, refs = ec.sweep_case(key)
    assert len(pdfs) == 6 and x.shape == (6 * m, pdfs[0].d) and m == ec.sweep_m(key)
    refused = 0
    for parity, ref in enumerate(refs):
        may = np.isfinite(ref["margin"])
        assert ref["margin"].min() > ec.MARGIN, (key, parity, ref["margin"].min())      # the cap on pairs left out is zero
        assert ref["lower"].sum() == 2 * m and may.sum() == 2 * m - 2, (key, parity)    # one error pair, one NaN pair
        assert ref["swap"].sum() > 0, (key, parity)
        assert ref["attempts"].sum() == 2 * m and ref["accepts"].sum() == ref["swap"].sum()
        lo_err, lo_nan = (0 * m + 2, 3 * m + 1) if parity == 0 else (1 * m + 2, 4 * m + 1)
        assert ref["lower"][lo_err] and not may[lo_err] and not ref["swap"][lo_err]
        assert ref["lower"][lo_nan] and not may[lo_nan] and not ref["swap"][lo_nan] and np.isnan(float(ref["log_alpha"][lo_nan]))
        out = 2 if parity == 0 else 0                                                   # members that sit out: untouched
        for g in range(2):
            rows = slice((3 * g + out) * m, (3 * g + out + 1) * m)
            assert np.array_equal(ref["x"][rows], x[rows], equal_nan=True) and not ref["lower"][rows].any()
        assert np.array_equal(ref["x"], x[ref["replica"]], equal_nan=True)
        refused += int((may & ~ref["swap"]).sum())
    return refused


_refused = {}


@pytest.mark.parametrize("key", NEW_SWEEPS, ids=ec.case_id)
def test_new_sweep_cases_keep_the_decision_margin(key):
    _refused[key] = _sweep_conditions(key)


def test_both_decisions_occur_in_number():
    """(a case of m = 7 may swap all of its 12 pairs: the cases together have several hundred refusals by the draw)"""
    total = sum(_refused[key] if key in _refused else _sweep_conditions(key) for key in NEW_SWEEPS)
    print(f"{total} pairs refused by the draw over {len(NEW_SWEEPS)} cases")
    assert total > 300


# ------------------------------------------------------------------------------------------ ladder: the restatement
@pytest.mark.parametrize("key", lz.layout_cases() + lz.flat_cases(), ids=lz.case_id)
def test_host_fold_on_reference_values(key):
    """host_fold over a table of reference_math values of the case's rows against direct_sums; every row is used."""
    pdfs, m, x = lz.case_rows(key)
    rows, N, d = x.shape
    M = len(pdfs)
    assert (rows, N) == (lz.N_ROWS, M * m) and M == lz.R * lz.G and np.all(np.isfinite(x))
    assert np.allclose(np.linalg.norm(x, axis=-1), 1.0, rtol=0, atol=1e-14)
    xm = x.reshape(rows, M, m, d)
    lp3 = np.full((rows, M, m, 3), np.nan, dtype=LD)
    for t, p in enumerate(pdfs):
        for w, src in ((0, t), (1, t - 1), (2, t + 1)):
            if (w == 1 and t % lz.R == 0) or (w == 2 and t % lz.R == lz.R - 1):
                continue                                                         # no such neighbour: never read
            lp3[:, t, :, w] = rm.log_prob(p, xm[:, src].reshape(rows * m, d)).reshape(rows, m)
    acc = lz.host_fold(lp3, lz.R)
    want = lz.direct_sums(lp3, lz.R)
    assert acc.shape == (lz.G, lz.R - 1, m, 10)
    assert np.all(acc[..., 0] == lz.N_ROWS) and not acc[..., 9].any()           # all rows are used
    assert np.array_equal(acc[..., 0], want["used"]) and np.array_equal(acc[..., 9], want["skipped"])
    lse_u, lse_v = acc[..., 1] + np.log(acc[..., 2]), acc[..., 5] + np.log(acc[..., 6])
    for got, name in ((lse_u, "lse_u"), (lse_v, "lse_v"), (acc[..., 3], "sum_u"), (acc[..., 4], "sum_uu"), (acc[..., 7], "sum_v"),
                      (acc[..., 8], "sum_vv")):
        err = float(np.max(np.abs(got - want[name]) / np.maximum(1, np.abs(want[name]))))
        assert err <= 1e-15, (name, err)                                         # (test_ladder_host.py's bar)
    if key[0] == "flat":    # the pair (beta = 0.5, beta = 0): the flat member's two values cancel, u and v are the warm member's alone
        flat = lp3[:, 2::3, :, 0]
        assert np.all(flat == flat[0, :, :1])


# ------------------------------------------------------------------------------------------ counter words
B = 1 << 32


def _u53(a, b):
    return float(((int(a) >> 5) << 26) | (int(b) >> 6)) / float(1 << 53)


def _exchange_uniform(orc, seed, chain, step):
    """counter (block, step_lo32, chain_lo32, chain_hi16 | step_hi16 << 16), key the 64-bit seed; the
    first 53-bit uniform of the block."""
    ctr = [ec.EXCHANGE_BLOCK, step % B, chain % B, ((chain >> 32) & 0xFFFF) | (((step >> 32) & 0xFFFF) << 16)]
    w = orc.philox4x32_10(ctr, [seed % B, seed >> 32])
    return _u53(w[0], w[1])


def test_stream_block_above_two_to_the_32():
    orc = ec._oracle()
    assert B < ec.HIGH_CHAIN_OFFSET < 1 << 48 and B < ec.HIGH_STEP < (1 << 48) - 1
    assert ec.HIGH_CHAIN_OFFSET % B == 0 and ec.HIGH_STEP % B == ec.SWEEP_STEP       # the low words of the plain sweep
    pdfs, m, sub, sub_err, high, low = ec.high_case()
    chains = [0, 1, m, 3 * m - 1]
    for seed in (ec.SWEEP_SEED, (0xABCDEF << 32) | 12345):
        for c in chains:
            for chain, step in ((ec.HIGH_CHAIN_OFFSET + c, ec.HIGH_STEP), (c, ec.SWEEP_STEP), (ec.HIGH_CHAIN_OFFSET + c, ec.SWEEP_STEP),
                                (c, ec.HIGH_STEP), ((0xFFFF << 32) | (B - 1 - c), (0xFFFF << 32) | 7)):
                assert orc.stream_block(seed, chain, step, ec.EXCHANGE_BLOCK)[0] == _exchange_uniform(orc, seed, chain, step)
    # each high word enters: dropping either gives another uniform
    u = [orc.stream_block(ec.SWEEP_SEED, ch, st, ec.EXCHANGE_BLOCK)[0]
         for ch, st in ((ec.HIGH_CHAIN_OFFSET, ec.HIGH_STEP), (0, ec.HIGH_STEP), (ec.HIGH_CHAIN_OFFSET, ec.SWEEP_STEP), (0, ec.SWEEP_STEP))]
    assert len(set(u)) == 4
    assert np.array_equal(ec.uniforms(ec.SWEEP_SEED, ec.HIGH_CHAIN_OFFSET + np.arange(4), ec.HIGH_STEP),
                          [_exchange_uniform(orc, ec.SWEEP_SEED, ec.HIGH_CHAIN_OFFSET + c, ec.HIGH_STEP) for c in range(4)])


def test_counter_word_case_keeps_the_margin_and_differs_from_the_plain_sweep():
    pdfs, m, sub, sub_err, high, low = ec.high_case()
    assert len(pdfs) == 6 and sub.shape == (3 * m, 5) and not sub_err.any() and np.isnan(sub[1 * m + 1]).any()
    for parity in (0, 1):
        ref, plain = high[parity], low[parity]
        may = np.isfinite(ref["margin"])
        assert ref["margin"].min() > ec.MARGIN and plain["margin"].min() > ec.MARGIN
        assert ref["lower"].sum() == m and may.sum() == m - 1                       # the NaN pair
        assert 0 < ref["swap"].sum() < may.sum()                                   # both decisions
        assert np.array_equal(ref["lower"], plain["lower"])
        assert np.array_equal(ref["log_alpha"], plain["log_alpha"], equal_nan=True)  # the same rows, the same members
        differ = int((ref["swap"] != plain["swap"]).sum())
        print(f"parity {parity}: {int(ref['swap'].sum())} of {int(may.sum())} swap, {differ} decisions differ from offset 0, step {ec.SWEEP_STEP}")
        # (a pair with log alpha >= 0 swaps whatever the draw: only the pairs with 0 < alpha < 1 can tell two streams apart, and
        # one such decision is enough for a sweep that dropped the high words to fail)
        assert differ > 0 and not np.array_equal(ref["x"], plain["x"], equal_nan=True)


def test_log_area_of_the_flat_rungs():
    """hot_log_z of the flat cases is the flat member's reference value plus the log area of the sphere."""
    for _, family, d in ec.flat_cases():
        batch = ec.flat_batch(family, d)
        e0 = np.eye(d)[0]
        log_area = math.log(2.0) + 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d)
        for g, got in enumerate(batch.hot_log_z()):
            want = float(rm.log_prob(batch.pdfs[3 * g + 2], e0)) + log_area
            assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (family, d, g, got, want)
