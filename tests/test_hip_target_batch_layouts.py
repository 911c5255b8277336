"""TargetBatch in exact mode in every vector layout: run_kernel<V, Target, PhiloxDraws, false, BATCH> and batch_logprob_kernel for
the fifteen layouts and both target policies, at the shapes where a target is a few chains wide and a workgroup boundary falls
inside every target (tests/batch_layout_cases.py: chains per target = the layout's chains per workgroup + 3).

A batch's chains are held to two references: the M separate samplers on the members with chain_offset = t m, bit for bit (kept
rows, final states, tries, rejections, error bits), and the CPU oracle's chains of the members -- states within the 1e-10 the
suite holds between device and oracle (tests/test_hip_parity.py), tries and rejections exactly, no error bit.  log_prob and
gradient of the batch are the members' own bit for bit and within 1e-10 of tests/reference_math.py."""
import numpy as np
import pytest

import batch_layout_cases as bc

pytestmark = pytest.mark.gpu

TOL = bc.TOL
LOGPROB_KEYS = bc.SWEEP + bc.GLOBAL_CASES


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    bc.release()  # the cached members' device copies go with the module
    torch.cuda.synchronize()


def sampler_cls(gs, sampler):
    return gs.ShrinkageSphericalSliceSampler if sampler == "shrink" else gs.RejectionSphericalSliceSampler


def outputs(s, calls=((bc.FIRST, bc.THIN), (bc.N_STEPS - bc.FIRST, bc.THIN))):
    draws = np.concatenate([s.advance(steps, thin=thin).cpu().numpy() for steps, thin in calls])
    return {"draws": draws, "state": s.state, "tries": s.n_tries_per_chain, "reject": s.n_reject_per_chain, "errors": s.errors}


def separate(gs, cls, pdfs, x0, m, placement, t0=0):
    """One sampler per member, chain_offset = t m: the loop a batch replaces."""
    parts = [outputs(cls(p, x0[i * m:(i + 1) * m], bc.SEED, chain_offset=(t0 + i) * m, mode="exact", placement=placement))
             for i, p in enumerate(pdfs)]
    return {k: np.concatenate([q[k] for q in parts], axis=2 if k == "draws" else 0) for k in parts[0]}


def assert_same(got, want, what=""):
    """tests/test_hip_target_batch.py's: every output, bit for bit."""
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int(np.sum(got[k] != want[k])))
    assert not got["errors"].any()


def oracle_error(got, ref):
    """-> max |dx| over kept rows and final states; tries, rejections and error bits are asserted exactly."""
    assert not ref["err"].any() and not got["errors"].any()
    assert np.array_equal(got["tries"], ref["n_tries"]), int(np.sum(got["tries"] != ref["n_tries"]))
    assert np.array_equal(got["reject"], ref["n_reject"])
    kept = got["draws"].transpose(2, 0, 1)                              # (chains, kept rows, d)
    assert kept.shape == ref["samples"].shape
    return max(float(np.max(np.abs(kept - ref["samples"]))), float(np.max(np.abs(got["state"] - ref["state"]))))


def batch_kernel_name(gs, handle, placement):
    return gs._lib.load().gsss_kernel_name(handle, 0, 0, bc.PLACEMENTS[placement]).decode()


def expected_name(key):
    return f"run_kernel<{bc.layout_of(key)}, {'VmfMixture' if bc.is_vmf(key) else 'Bingham'}, batch>"


def run_batch(gs, key, placement, sampler):
    pdfs, m, x0 = bc.pdfs_of(key), bc.chains(key, placement), bc.x0(key, placement)
    cls = sampler_cls(gs, sampler)
    s = cls(gs.TargetBatch(pdfs), x0, bc.SEED, mode="exact", placement=placement)
    assert s.mode == "exact" and s._batch_m == m
    name = batch_kernel_name(gs, s._target_dev.handle, placement)
    assert name == expected_name(key), name
    got = outputs(s)
    assert got["draws"].shape == (bc.N_STEPS // bc.THIN, pdfs[0].d, len(pdfs) * m)
    assert_same(got, separate(gs, cls, pdfs, x0, m, placement), (key, placement, sampler))
    err = oracle_error(got, bc.oracle_chains(key, sampler, placement))
    print(f"{bc.case_id(key)} {placement} {sampler} ({name}, m = {m}): max |dx| against the oracle {err:.1e}, "
          f"largest try count {int(got['tries'].max())}")
    assert err < TOL, err
    return got


# ------------------------------------------------------------------------------------------ (a) chains, every layout
@pytest.mark.parametrize("key,placement,sampler", bc.sweep_params(), ids=bc.case_id)
def test_batch_chains(gs, key, placement, sampler):
    run_batch(gs, key, placement, sampler)


# ------------------------------------------------------------------------------------------ (b) a run of targets, cooperative layouts
@pytest.mark.parametrize("family", ["vmf3", "binghamfisher"])
@pytest.mark.parametrize("d", [17, 130, 600])
def test_a_run_of_the_targets(gs, d, family):
    """A sampler on targets 1 .. 3 of four (chain_offset = m, chains_per_target = m) gives rows m .. of the whole batch bit for
    bit; two advance calls equal one."""
    key = (family, d, 4)
    pdfs, m, x0 = bc.pdfs_of(key), bc.chains(key), bc.x0(key)
    assert len(pdfs) == 4 and bc.lanes(bc.layout_of(key)) > 1
    cls = sampler_cls(gs, "shrink")
    batch = gs.TargetBatch(pdfs)
    whole = cls(batch, x0, bc.SEED, mode="exact", placement="packed")
    assert batch_kernel_name(gs, whole._target_dev.handle, "packed") == expected_name(key)
    full = outputs(whole)
    part = outputs(cls(batch, x0[m:], bc.SEED, mode="exact", placement="packed", chain_offset=m, chains_per_target=m))
    for k in full:
        assert np.array_equal(part[k], full[k][..., m:] if k == "draws" else full[k][m:]), k
    assert not full["errors"].any()
    assert_same(full, separate(gs, cls, pdfs, x0, m, "packed"), key)
    one = outputs(cls(batch, x0, bc.SEED, mode="exact", placement="packed"), calls=((bc.N_STEPS, bc.THIN),))
    assert_same(one, full, "one advance call")


# ------------------------------------------------------------------------------------------ (c) rows in global memory
@pytest.mark.parametrize("sampler", bc.SAMPLERS)
@pytest.mark.parametrize("key", bc.GLOBAL_CASES)
def test_rows_in_global_memory(gs, key, sampler):
    """The members' rows (K = 7000 means; 40 means of 600; a dense A above d = 128) are read through the moved blob.  The
    second member is not the first: its oracle chains are not those of member 0 on the same rows, so a stride of zero cannot pass."""
    assert not bc.rows_in_lds(key)
    m = bc.chains(key)
    ref = bc.oracle_chains(key, sampler)
    gap = float(np.max(np.abs(bc.oracle_chains_of_wrong_member(key, sampler) - ref["samples"][m:2 * m])))
    assert gap > 1e-3, gap
    run_batch(gs, key, "packed", sampler)


# ------------------------------------------------------------------------------------------ (d) diagonal and dense members mixed
@pytest.mark.parametrize("sampler", bc.SAMPLERS)
def test_diagonal_and_dense_members_mixed(gs, sampler):
    """d = 24, four lanes a chain.  States within 1e-10 of the members alone and of the oracle (a mixed
    batch is held at 1e-10, not bitwise), tries, rejections and error bits exactly."""
    pdfs, m, x0, ref = bc.mixed_case(sampler)
    cls = sampler_cls(gs, sampler)
    s = cls(gs.TargetBatch(pdfs), x0, bc.SEED, mode="exact", placement="packed")
    assert batch_kernel_name(gs, s._target_dev.handle, "packed") == "run_kernel<coop4x8, Bingham, batch>"
    got = outputs(s)
    want = separate(gs, cls, pdfs, x0, m, "packed")
    for k in ("draws", "state"):
        err = float(np.max(np.abs(got[k] - want[k])))
        print(f"mixed diagonal / dense batch, {sampler}, {k}: max |dx| against the members {err:.1e}")
        assert err < TOL, (k, err)
    for k in ("tries", "reject", "errors"):
        assert np.array_equal(got[k], want[k]), k
    err = oracle_error(got, ref)
    print(f"mixed diagonal / dense batch, {sampler}: max |dx| against the oracle {err:.1e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------ (e) log_prob / gradient
@pytest.mark.parametrize("key", LOGPROB_KEYS, ids=bc.case_id)
def test_log_prob_and_gradient(gs, key):
    """One point, and a full workgroup of points + 3, per member."""
    pdfs = bc.pdfs_of(key)
    batch = gs.TargetBatch(pdfs)
    assert batch_kernel_name(gs, batch._device_target().handle, "packed") == expected_name(key)
    bc.check_logprob(gs, pdfs, bc.case_id(key), (1, bc.chains(key)))


@pytest.mark.parametrize("family", ["vmf3", "binghamfisher"])
@pytest.mark.parametrize("d", [5, 24, 100, 600])
def test_component_major_draws(gs, d, family):
    """gsss_batch_logprob_draws, one d per layout family: target_log_prob on (R, d, N) blocks == log_prob of the same points
    gathered into (M, R m, d), bit for bit; target0 > 0 serves the later targets; the chain-major form gives the same values
    (the pattern of tests/test_hip_batch_logprob.py::test_component_major_draws)."""
    import torch
    from geosss_amd import diagnostics
    key = (family, d)
    pdfs, m, R = bc.pdfs_of(key), bc.chains(key), 2
    M = len(pdfs)
    for p in pdfs:
        p._invalidate()
    batch = gs.TargetBatch(pdfs)
    for t0 in (0, 1):
        Mc = M - t0
        N = Mc * m
        x = torch.from_numpy(np.ascontiguousarray(bc.points(("draws", family, t0), R, N, d).transpose(0, 2, 1))).cuda()   # (R, d, N)
        got = diagnostics.target_log_prob(batch, x, target0=t0)
        assert tuple(got.shape) == (R, N)
        gathered = x.reshape(R, d, Mc, m).permute(2, 0, 3, 1).reshape(Mc, R * m, d).contiguous()
        want = gs.TargetBatch(pdfs[t0:]).log_prob(gathered)                                               # (Mc, R m)
        assert torch.equal(got.reshape(R, Mc, m).permute(1, 0, 2).reshape(Mc, R * m), want), (key, t0)
        cm = diagnostics.target_log_prob(batch, x.permute(2, 0, 1).contiguous(), chain_major=True, target0=t0)
        assert tuple(cm.shape) == (N, R) and torch.equal(cm, got.t())
        # and the values are the reference's
        rows = gathered.cpu().numpy()
        worst = max(bc.lc.rel(want[i].cpu().numpy(), bc.rm.log_prob(p, rows[i])) for i, p in enumerate(pdfs[t0:]))
        print(f"{bc.case_id(key)} target0={t0}: log_prob {worst:.1e}")
        assert worst < TOL
    assert not any("_targets" in p.__dict__ for p in pdfs)


# ------------------------------------------------------------------------------------------ what the sweep reached
def test_sweep_reaches_every_layout(gs):
    """The names the sweep's tests assert, read off a device copy of the cheapest family of each policy at every d: all fifteen
    layouts with a vMF batch and with a Bingham batch, for the sampler and (the same select_vec_for) log_prob / gradient."""
    lib = gs._lib.load()
    assert {lib.gsss_exact_layout(d) for d in bc.DIMS} == set(range(1, len(bc.LAYOUTS) + 1))
    for family, policy in (("vmf1", "VmfMixture"), ("bingham_diag", "Bingham")):
        reached = set()
        for d in bc.DIMS:
            key = (family, d)
            assert (key, "packed", "shrink") in bc.sweep_params() and key in LOGPROB_KEYS
            h = gs.TargetBatch(bc.pdfs_of(key))._device_target(chains_per_target=bc.chains(key)).handle
            name = batch_kernel_name(gs, h, "packed")
            assert name == expected_name(key) and name.endswith(f", {policy}, batch>"), name
            reached.add(name[len("run_kernel<"):].split(",")[0])
        assert reached == set(bc.LAYOUTS), (family, sorted(set(bc.LAYOUTS) - reached))
