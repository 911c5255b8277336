"""Replica exchange and the ladder sums in every vector layout: exchange_eval_kernel<V, TT> and ladder_eval_kernel<V, TT> for the
fifteen layouts and both target policies, at both ends of every layout's range of d (exchange_cases.layout_dims), with a full
chunk, a ragged chunk and a workgroup boundary inside every member (chains per target = the layout's chains per workgroup + 3).

The assertions are those of test_hip_exchange.py::test_one_sweep_against_the_reference and
test_hip_ladder.py::test_accumulators_against_the_host_restatement (exchange_cases.check_sweep,
ladder_cases.check_accumulators), on more cases: the layout sweep; tempered ladders whose hottest rung is flat (beta = 0), one
per layout family and policy; and one sweep of the second ladder alone with chain ids and a step above 2^32, so that the high
words of the stream's counter are not zero.  The conditions of the cases -- no pair within exchange_cases.MARGIN of its
decision, both decisions present -- are asserted on the CPU by test_exchange_layouts_host.py.

Worst deviations per layout family, MI355X (measured, not asserted; the bar is 1e-10 throughout): DESIGN.md sections 5.6i, 5.6j."""
import math

import numpy as np
import pytest

import batch_layout_cases as bc
import exchange_cases as ec
import ladder_cases as lz
import reference_math as rm

pytestmark = pytest.mark.gpu

TOL = bc.TOL


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    lz.release()  # the cached members (33 MB each at d >= 1025) and their device copies go with the module
    torch.cuda.synchronize()


def kernel_layout(gs, pdfs, m):
    """The layout the batch's exact-mode kernels run in, read off a device copy (gsss_kernel_name)."""
    h = gs.TargetBatch(list(pdfs))._device_target(chains_per_target=m).handle
    name = gs._lib.load().gsss_kernel_name(h, 0, 0, bc.PLACEMENTS["packed"]).decode()
    return name[len("run_kernel<"):].split(",")[0]


# ------------------------------------------------------------------------------------------ the layout sweep
@pytest.mark.parametrize("key", ec.layout_cases(), ids=ec.case_id)
def test_exchange_in_every_layout(gs, key):
    pdfs, m = ec.sweep_members(key), ec.sweep_m(key)
    assert kernel_layout(gs, pdfs, m) == bc.natural_layout(key[1])
    ec.check_sweep(key)


@pytest.mark.parametrize("key", lz.layout_cases(), ids=lz.case_id)
def test_ladder_in_every_layout(gs, key):
    pdfs, m, _ = lz.case_rows(key)
    assert kernel_layout(gs, pdfs, m) == bc.natural_layout(key[2])
    lz.check_accumulators(key)


def test_sweep_names_every_layout():
    """(the two tests above assert of every case that the device runs it in the layout of its d: together, all fifteen)"""
    assert {bc.natural_layout(d) for _, d in ec.layout_cases()} == set(bc.LAYOUTS) == {bc.natural_layout(d) for _, _, d in lz.layout_cases()}


# ------------------------------------------------------------------------------------------ a flat hottest rung
@pytest.mark.parametrize("key", ec.flat_cases(), ids=ec.case_id)
def test_flat_hottest_rung(gs, key):
    _, family, d = key
    batch, m = ec.flat_batch(family, d), ec.sweep_m(key)
    pdfs, _, x = lz.case_rows(key)
    assert pdfs == tuple(batch.pdfs) and kernel_layout(gs, pdfs, m) == bc.natural_layout(d)
    # the flat members' log_prob over all points of the case: one value, the reference's, and hot_log_z less the log area
    pts = np.concatenate([x.reshape(-1, d), ec.sweep_case(key)[2]])
    pts = pts[np.all(np.isfinite(pts), axis=1)]
    lp = batch.log_prob(np.ascontiguousarray(np.broadcast_to(pts, (len(batch),) + pts.shape)))
    log_area = math.log(2.0) + 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d)
    hot = batch.hot_log_z()
    for g in range(ec.SWEEP_G):
        t = ec.SWEEP_R * g + ec.SWEEP_R - 1
        assert np.all(lp[t] == lp[t, 0]), (t, np.unique(lp[t]))
        ref = rm.log_prob(batch.pdfs[t], pts[:4])
        dev = [bc.lc.rel(lp[t, :4], ref), abs(float(lp[t, 0]) + log_area - hot[g]) / max(1.0, abs(hot[g]))]
        print(f"{ec.case_id(key)} flat member {t}: log_prob {float(lp[t, 0])!r}, reference within {dev[0]:.1e}, hot_log_z within {dev[1]:.1e}")
        assert dev[0] < TOL and dev[1] < TOL
        assert not np.all(lp[t - 1] == lp[t - 1, 0])                               # (the rung below is not flat)
    # the sweep's and the ladder's assertions hold on these batches too
    out = ec.check_sweep(key)
    lz.check_accumulators(key)
    # parity 1 pairs (beta = 0.5, beta = 0): the flat member's bracket is exactly zero, log alpha = l_a(x_b) - l_a(x_a)
    la, own, across = out[1]["la"], out[1]["own"], out[1]["across"]
    x_sweep = ec.sweep_case(key)[2]
    for g in range(ec.SWEEP_G):
        lo = np.arange((ec.SWEEP_R * g + 1) * m, (ec.SWEEP_R * g + 2) * m)
        ok = np.all(np.isfinite(x_sweep[lo]), axis=1) & np.all(np.isfinite(x_sweep[lo + m]), axis=1)
        assert ok.sum() >= m - 1
        assert np.all(across[lo + m][ok] - own[lo + m][ok] == 0.0)
        assert np.array_equal(la[lo][ok], across[lo][ok] - own[lo][ok])


# ------------------------------------------------------------------------------------------ counter words and target0
def _second_ladder_sweep(gs, parity, chain_offset, step):
    """gsss_batch_exchange on the second ladder's chains alone (target0 = R), reached as test_hip_ladder.py::test_second_ladder_alone
    reaches gsss_batch_ladder.  -> (rows after, replica, counts (2, 3), log alpha)"""
    import torch
    pdfs, m, sub, sub_err, _, _ = ec.high_case()
    R, n, d = ec.SWEEP_R, ec.SWEEP_R * m, sub.shape[1]
    from geosss_amd.sphere import current_stream_ptr
    batch = gs.TargetBatch(list(pdfs))
    state = torch.from_numpy(np.ascontiguousarray(sub.T)).cuda()                    # component-major (d, n)
    tgt = batch._device_target(state.device, chains_per_target=m)
    err = torch.from_numpy(sub_err).cuda()
    scratch = torch.empty(int(tgt.lib.gsss_exchange_scratch_doubles(n)), dtype=torch.float64, device="cuda")
    replica = torch.arange(n, dtype=torch.int64, device="cuda")
    counts = torch.zeros((2, R), dtype=torch.int64, device="cuda")
    log_alpha = torch.full((n,), 7.25, dtype=torch.float64, device="cuda")
    assert state.shape == (d, n) and scratch.numel() == 2 * n and err.dtype == torch.int32
    gs._lib.check(tgt.lib.gsss_batch_exchange(tgt.handle, state.data_ptr(), err.data_ptr(), n, R, R, parity, ec.SWEEP_SEED, chain_offset,
                                              step, scratch.data_ptr(), replica.data_ptr(), counts.data_ptr(), log_alpha.data_ptr(),
                                              current_stream_ptr(state.device.index)))
    torch.cuda.synchronize()
    return state.cpu().numpy().T, replica.cpu().numpy(), counts.cpu().numpy(), log_alpha.cpu().numpy()


@pytest.mark.parametrize("parity", [0, 1])
def test_high_counter_words_on_the_second_ladder_alone(gs, parity):
    pdfs, m, sub, sub_err, high, low = ec.high_case()
    ref, plain = high[parity], low[parity]
    assert ref["margin"].min() > ec.MARGIN and plain["margin"].min() > ec.MARGIN
    # on the reference: the high words change decisions, so ignoring them cannot pass
    assert (ref["swap"] != plain["swap"]).sum() > 0
    for want, (offset, step) in ((ref, (ec.HIGH_CHAIN_OFFSET, ec.HIGH_STEP)), (plain, (0, ec.SWEEP_STEP))):
        after, replica, counts, la = _second_ladder_sweep(gs, parity, offset, step)
        lower = want["lower"]
        assert np.array_equal(after, want["x"], equal_nan=True) and np.array_equal(after, sub[want["replica"]], equal_nan=True)
        assert np.array_equal(replica, want["replica"])
        assert np.array_equal(counts[0], want["attempts"]) and np.array_equal(counts[1], want["accepts"])
        assert np.all(la[~lower] == 7.25)
        fin = np.isfinite(want["log_alpha"][lower].astype(np.float64))
        rel = np.abs(la[lower][fin] - want["log_alpha"][lower][fin]).astype(np.float64) / want["scale"][lower][fin]
        assert fin.sum() == m - 1 and rel.max() < TOL
    print(f"parity {parity}: {int(ref['swap'].sum())} swaps with the high words, {int(plain['swap'].sum())} without, "
          f"{int((ref['swap'] != plain['swap']).sum())} decisions differ")


def test_second_ladder_alone_has_the_whole_sweeps_log_alpha(gs):
    """target0 = R serves the second ladder's members: log alpha of the sub-call equals the whole batch's at the same chains."""
    import torch
    pdfs, m, x, err, _ = ec.sweep_case(ec.HIGH_KEY)
    n = len(x)
    for parity in (0, 1):
        s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(list(pdfs)), x, seed=ec.SWEEP_SEED, mode="exact", step_offset=ec.SWEEP_STEP)
        whole = torch.full((n,), 7.25, dtype=torch.float64, device="cuda")
        s.exchange(ec.SWEEP_R, parity, log_alpha=whole)
        la = _second_ladder_sweep(gs, parity, ec.HIGH_CHAIN_OFFSET, ec.HIGH_STEP)[3]
        assert np.array_equal(la, whole.cpu().numpy()[ec.SWEEP_R * m:], equal_nan=True)
