"""Replica exchange on the device (gsss_batch_exchange; sampler.exchange, advance / sample / summarize(exchange=)).

One sweep is held to exchange_cases.reference_sweep (numpy longdouble, the oracle's stream): the decisions, the permuted columns
bit for bit, replica, counts and log alpha.  No case contains a pair within exchange_cases.MARGIN of its decision -- a condition
of the cases, asserted on the CPU by test_exchange_host.py and again here before the device is asked.  The schedule tests hold
advance(exchange=) to its own definition, a loop of advance(every) and exchange(); the end-to-end test holds the d = 10 ladder
to the tolerance the CPU reference recorded (exchange_cases.OCC_TOL), never to a figure of the device run."""
import numpy as np
import pytest
import torch

import exchange_cases as ec
import geosss_amd as gs

pytestmark = pytest.mark.gpu


def _sampler(pdfs, x, seed, mode="exact", step=0, cls=None, **kw):
    cls = cls or gs.ShrinkageSphericalSliceSampler
    return cls(gs.TargetBatch(list(pdfs)), x, seed=seed, mode=mode, step_offset=step, **kw)


# ------------------------------------------------------------------------------------------ one sweep
@pytest.mark.parametrize("key", ec.SWEEP_CASES + ec.SWEEP_GLOBAL, ids=lambda k: k if isinstance(k, str) else f"{k[0]}-{k[1]}")
def test_one_sweep_against_the_reference(key):
    """exchange_cases.check_sweep: log alpha, decisions, permuted rows, replica and counts of both parities."""
    ec.check_sweep(key)


def test_identical_members_always_swap():
    """Ladders of identical members: log alpha = 0 exactly, every pair with u > 0 swaps, the states are the permutation."""
    import batch_layout_cases as bc
    p = bc.members("vmf3", 5)[0]
    R, G, m = 4, 2, 70
    x = bc.points("exchange-identical", 1, R * G * m, 5)[0]
    for parity in (0, 1):
        s = _sampler([p] * (R * G), x, 11, step=3)
        la = torch.zeros(R * G * m, dtype=torch.float64, device="cuda")
        s.exchange(R, parity, log_alpha=la)
        t = np.arange(R * G) % R
        lower_t = (t % 2 == parity) & (t + 1 < R)
        lo = np.flatnonzero(np.repeat(lower_t, m))
        u = ec.uniforms(11, lo, 3)
        assert (u > 0).all()
        la = la.cpu().numpy()
        assert np.all(la == 0.0) and not np.signbit(la[lo]).any()
        perm = np.arange(len(x))
        perm[lo], perm[lo + m] = lo + m, lo
        assert np.array_equal(s.state_rows().cpu().numpy(), x[perm]) and np.array_equal(s.replica.cpu().numpy(), perm)
        st = s.exchange_stats()
        assert np.array_equal(st["attempts"].cpu().numpy(), m * lower_t) and np.array_equal(st["accepts"].cpu().numpy(), m * lower_t)


# ------------------------------------------------------------------------------------------ the schedule
def _ladder_sampler(mode, seed=5, m=40, G=2, step=0):
    """Two tempered ladders of four vMF mixtures at d = 5, m chains a rung (a rung spans wavefronts, a ladder workgroups)."""
    import batch_layout_cases as bc
    pdfs = bc.members("vmf3", 5)[:G]
    batch = gs.TargetBatch.tempered(list(pdfs), [1.0, 0.6, 0.3, 0.1])
    x = bc.points("exchange-schedule", 1, len(batch) * m, 5)[0]
    return gs.ShrinkageSphericalSliceSampler(batch, x, seed=seed, mode=mode, step_offset=step)


def _same(a, b):
    assert torch.equal(a.state_device, b.state_device) and torch.equal(a.replica, b.replica)
    sa, sb = a.exchange_stats(), b.exchange_stats()
    assert torch.equal(sa["attempts"], sb["attempts"]) and torch.equal(sa["accepts"], sb["accepts"])
    assert np.array_equal(a.n_tries_per_chain, b.n_tries_per_chain) and a._step == b._step


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_schedule_is_a_function_of_the_step(mode):
    every, ex = 2, dict(ladder=4, every=2)
    one, two, hand, resumed = (_ladder_sampler(mode, step=3) for _ in range(4))     # (an odd start: the first sweep after one step)
    rows = one.advance(20, thin=every, exchange=ex)
    first, second = two.advance(10, thin=every, exchange=ex), two.advance(10, thin=every, exchange=ex)
    _same(one, two)
    assert torch.equal(rows, torch.cat([first, second]))
    kept = []
    while hand._step < 23:                                    # the definition, step by step: sweep after the even steps
        hand.advance(1)
        if hand._step % every == 1:                            # (steps 3 + 2 j of the call: the kept rows)
            kept.append(hand.state_device.clone())
        else:
            hand.exchange(4, every=every)
    _same(one, hand)
    assert torch.equal(rows, torch.stack(kept))
    # from an even step on, the loop the schedule is named after: advance(every) keeping its last state, then exchange()
    a, b = _ladder_sampler(mode), _ladder_sampler(mode)
    rows = a.advance(8, thin=every, exchange=ex)
    kept = []
    for _ in range(4):
        kept.append(b.advance(every, thin=every)[0])           # (the row is the state before the sweep)
        b.exchange(4, every=every)
    _same(a, b)
    assert torch.equal(rows, torch.stack(kept))
    acc = one.exchange_stats()
    assert int(acc["accepts"].sum()) > 0 and int(acc["attempts"][3::4].sum()) == 0 and not torch.equal(one.replica, torch.arange(320, device="cuda"))
    # state_dict round-trips mid-run
    resumed.advance(9, exchange=ex)
    fresh = _ladder_sampler(mode)
    fresh.load_state_dict(resumed.state_dict())
    fresh.advance(11, exchange=ex)
    _same(one, fresh)


def test_exchange_none_is_todays_code_path():
    """advance, sample and summarize with exchange=None against a sampler that never touches the feature -- after the first has
    used it, so that the buffers exist -- bit for bit."""
    used, plain = _ladder_sampler("fast"), _ladder_sampler("fast")
    used.exchange(4)
    used.exchange(4)                                           # (identical parity twice is no identity in general:
    used.load_state_dict(plain.state_dict())                   #  put the states back where the plain sampler's are)
    a, b = used.advance(6, thin=2, exchange=None), plain.advance(6, thin=2)
    assert torch.equal(a, b) and torch.equal(used.state_device, plain.state_device)
    assert np.array_equal(used.sample(5, burnin=2, exchange=None), plain.sample(5, burnin=2))
    su, sp = used.summarize(6, burnin=1, mixing=True, exchange=None), plain.summarize(6, burnin=1, mixing=True)
    assert torch.equal(su.acc, sp.acc) and torch.equal(su.mix_counts, sp.mix_counts) and torch.equal(su.mix_step, sp.mix_step)
    assert torch.equal(used.state_device, plain.state_device) and plain._xchg is None


def test_sample_in_two_chain_blocks_equals_one():
    ex = dict(ladder=4, every=2)
    one, two = _ladder_sampler("fast"), _ladder_sampler("fast")
    a = one.sample(7, burnin=3, blocks=1, exchange=ex)
    b = two.sample(7, burnin=3, blocks=2, exchange=ex)         # blocks are cut at multiples of R m: one ladder each
    assert np.array_equal(a, b)
    _same(one, two)
    assert int(one.exchange_stats()["accepts"].sum()) > 0


# ------------------------------------------------------------------------------------------ end to end
def test_exchange_unsticks_the_coldest_member():
    """The host module's d = 10 ladder in fast mode through summarize(mixing=True): without exchange the coldest member never
    leaves mode 1; with it, its occupancy of mode 2 lies within the CPU reference's tolerance of 0.5."""
    _, batch, x0 = ec.ladder_case()
    n_keep = ec.N_STEPS - ec.BURNIN + 1                        # draw 0 is the state after the burn-in
    plain = gs.ShrinkageSphericalSliceSampler(batch, x0, seed=ec.LADDER_SEED, mode="fast")
    st = plain.summarize(n_keep, burnin=ec.BURNIN, mixing=True).stats()
    assert float(st["hop_frequency"][0]) == 0.0 and float(st["mode_occupancy"][0, 1]) == 0.0
    s = gs.ShrinkageSphericalSliceSampler(batch, x0, seed=ec.LADDER_SEED, mode="fast")
    st = s.summarize(n_keep, burnin=ec.BURNIN, mixing=True, exchange=dict(ladder=ec.LADDER_R, every=ec.LADDER_EVERY)).stats()
    occ = float(st["mode_occupancy"][0, 1])
    rate = s.exchange_stats()["rate"].cpu().numpy()
    print(f"occupancy of mode 2: {occ:.4f} (tolerance {ec.OCC_TOL:.4f} about 0.5), hop frequency {float(st['hop_frequency'][0]):.4f}, "
          f"rates {np.round(rate, 3)}")
    assert abs(occ - 0.5) <= ec.OCC_TOL
    assert np.all((rate[:-1] > 0) & (rate[:-1] < 1)) and np.isnan(rate[-1])       # (the hottest rung is never the lower member)
    assert float(st["hop_frequency"][0]) > 0.0
