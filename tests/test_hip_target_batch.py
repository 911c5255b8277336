"""TargetBatch on the device: a batch run IS M separate samplers -- each on member t alone, with the same seed,
chain_offset = t m, the same mode / screen and rows [t m, (t + 1) m) of x0 -- bit for bit: kept draws, final states,
n_tries_per_chain, n_reject_per_chain and errors (np.array_equal, no tolerance).  The stream is a pure function of (seed, global
chain id, step), and one chain per lane == two, sliced == unsliced and spread == packed hold bit for bit (DESIGN.md sections 2,
5.1), so nothing but the target a chain reads distinguishes the two runs.

One thing about the separate side at d = 11 .. 16.  A member alone gets the lane kernel there only as a packed ensemble with the
screen on: a small ensemble, or screen=False, runs the cooperative kernel, another arithmetic (held to the lane kernel at 1e-10,
not bit for bit).  The batch's fast kernels are lane kernels in both arithmetics, and the screened and the all-double lane kernel
take the same decisions by construction, so the reference for BOTH fast modes of a batch at these d is
the member's packed, screened run -- bit for bit, like every other case."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20241
README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])


@pytest.fixture(scope="module")
def gs():
    import geosss_amd
    return geosss_amd


def _rotation(g, d):
    q, r = np.linalg.qr(g.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def members(gs, case, M):
    """M members that really differ, of the issue's families."""
    g = np.random.default_rng(sum(case.encode()) + 7)
    if case == "vmfmix_d3_k3":   # the README target, then scaled / rotated variants
        out = [gs.MixtureModel([gs.VonMisesFisher(m) for m in README_MUS])]
        for _ in range(M - 1):
            mus = (0.25 + 1.5 * g.random()) * README_MUS @ _rotation(g, 3).T
            out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], g.random(3) + 0.5))
        return out
    if case == "vmfmix_d8_k10":
        out = []
        for _ in range(M):
            mus = g.standard_normal((10, 8))
            mus *= (30.0 + 170.0 * g.random((10, 1))) / np.linalg.norm(mus, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], g.random(10) + 0.2))
        return out
    if case == "vmfmix_d14_k5":   # (beyond the issue's list: the wide vMF kernels, screened bucket 6, all-double bucket 10)
        out = []
        for _ in range(M):
            mus = g.standard_normal((5, 14))
            mus *= (20.0 + 80.0 * g.random((5, 1))) / np.linalg.norm(mus, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], g.random(5) + 0.2))
        return out
    if case == "vmf_d4_kappa_sweep":
        dirs = g.standard_normal((M, 4))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        return [gs.VonMisesFisher(k * v) for k, v in zip(np.geomspace(0.5, 500.0, M), dirs)]
    if case in ("bingham_d5_dense", "bingham_d12_dense", "bingham_d24_dense"):
        d = int(case.split("_")[1][1:])
        return [gs.random_bingham(d, vmax=10.0 + 40.0 * g.random(), vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(M)]
    if case == "bingham_d10_diag":
        return [gs.random_bingham(10, vmax=10.0 + 40.0 * g.random(), vmin=0.0, eigensystem=True, seed=int(g.integers(1 << 30)))
                for _ in range(M)]
    if case == "binghamfisher_d6":
        return [gs.BinghamFisher(gs.random_bingham(6, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))).A,
                                 (1.0 + 9.0 * g.random()) * g.standard_normal(6)) for _ in range(M)]
    raise KeyError(case)


def x0_for(gs, d, n):
    return gs.sample_sphere(d - 1, n, seed=11)


def outputs(s, steps, thin):
    draws = s.advance(steps, thin=thin)
    return {"draws": draws.cpu().numpy(), "state": s.state, "tries": s.n_tries_per_chain, "reject": s.n_reject_per_chain,
            "errors": s.errors}


def separate(gs, cls, pdfs, x0, m, steps, thin, t0=0, **kw):
    """The loop a user writes today: one sampler per target, chain_offset = t m."""
    if kw.get("mode") == "fast" and pdfs[0].d > 10:   # the member's lane kernel (see the module's docstring)
        kw["placement"], kw["screen"] = "packed", True
    parts = [outputs(cls(p, x0[i * m:(i + 1) * m], SEED, chain_offset=(t0 + i) * m, **kw), steps, thin) for i, p in enumerate(pdfs)]
    return {k: np.concatenate([q[k] for q in parts], axis=2 if k == "draws" else 0) for k in parts[0]}


def assert_same(got, want, what=""):
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int(np.sum(got[k] != want[k])))
    assert not got["errors"].any()


CASES = ["vmfmix_d3_k3", "vmfmix_d8_k10", "vmf_d4_kappa_sweep", "bingham_d5_dense", "bingham_d12_dense", "bingham_d10_diag",
         "binghamfisher_d6", "vmfmix_d14_k5"]
MODES = [("exact", True), ("fast", True), ("fast", False)]


@pytest.mark.parametrize("sampler", ["ShrinkageSphericalSliceSampler", "RejectionSphericalSliceSampler"])
@pytest.mark.parametrize("mode,screen", MODES, ids=["exact", "fast", "fast-double"])
@pytest.mark.parametrize("case", CASES)
def test_batch_is_the_separate_samplers(gs, case, mode, screen, sampler):
    cls = getattr(gs, sampler)
    M, m, steps, thin = 7, 64, 20, 2
    pdfs = members(gs, case, M)
    x0 = x0_for(gs, pdfs[0].d, M * m)
    s = cls(gs.TargetBatch(pdfs), x0, SEED, mode=mode, screen=screen)
    assert s.mode == mode and s._batch_m == m
    got = outputs(s, steps, thin)
    assert got["draws"].shape == (steps // thin, pdfs[0].d, M * m)
    assert_same(got, separate(gs, cls, pdfs, x0, m, steps, thin, mode=mode, screen=screen), case)
    assert got["tries"].min() >= steps


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("M,m", [(1, 64), (1, 256), (1, 300), (7, 256), (7, 300), (1000, 300)])
def test_sizes(gs, M, m, mode):
    """m = 300: a ragged last chunk per target; 64: less than one workgroup; M = 1000 x 300 chains x 20 steps."""
    cls = gs.ShrinkageSphericalSliceSampler
    pdfs = members(gs, "vmfmix_d3_k3", M)
    x0 = x0_for(gs, 3, M * m)
    got = outputs(cls(gs.TargetBatch(pdfs), x0, SEED, mode=mode), 20, 5)
    assert_same(got, separate(gs, cls, pdfs, x0, m, 20, 5, mode=mode), (M, m))


@pytest.mark.parametrize("M,m", [(1, 300), (7, 64), (1000, 300)])
def test_sizes_bingham_fast(gs, M, m):
    cls = gs.RejectionSphericalSliceSampler
    pdfs = members(gs, "bingham_d5_dense", M)
    x0 = x0_for(gs, 5, M * m)
    got = outputs(cls(gs.TargetBatch(pdfs), x0, SEED, mode="fast"), 20, 4)
    assert_same(got, separate(gs, cls, pdfs, x0, m, 20, 4, mode="fast"), (M, m))


@pytest.mark.parametrize("placement", ["packed", "spread"])
@pytest.mark.parametrize("case,m", [("vmfmix_d3_k3", 300), ("bingham_d5_dense", 64), ("vmfmix_d8_k10", 70)])
def test_exact_mode_packed_and_spread(gs, case, m, placement):
    cls = gs.ShrinkageSphericalSliceSampler
    M = 5
    pdfs = members(gs, case, M)
    x0 = x0_for(gs, pdfs[0].d, M * m)
    got = outputs(cls(gs.TargetBatch(pdfs), x0, SEED, mode="exact", placement=placement), 20, 2)
    assert_same(got, separate(gs, cls, pdfs, x0, m, 20, 2, mode="exact"), (case, placement))


def test_cooperative_layout_in_exact_mode(gs):
    """Bingham at d = 24: four lanes per chain, 64 chains per workgroup; m = 100 leaves a ragged last chunk per target."""
    cls = gs.ShrinkageSphericalSliceSampler
    M, m = 4, 100
    pdfs = members(gs, "bingham_d24_dense", M)
    x0 = x0_for(gs, 24, M * m)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        s = cls(gs.TargetBatch(pdfs), x0, SEED)          # no batch fast kernel at d = 24: mode "auto" runs the exact kernels
    assert s.mode == "exact"
    name = gs._lib.load().gsss_kernel_name(s._target_dev.handle, 0, 0, 0).decode()
    assert name.startswith("run_kernel<coop") and name.endswith(", batch>")
    with pytest.raises(ValueError, match="no batch fast kernel"):
        cls(gs.TargetBatch(pdfs), x0, SEED, mode="fast")
    assert_same(outputs(s, 20, 2), separate(gs, cls, pdfs, x0, m, 20, 2, mode="exact"))


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_two_advance_calls_are_one(gs, mode):
    cls = gs.ShrinkageSphericalSliceSampler
    M, m = 7, 100
    pdfs = members(gs, "binghamfisher_d6", M)
    x0 = x0_for(gs, 6, M * m)
    one = cls(gs.TargetBatch(pdfs), x0, SEED, mode=mode)
    a = one.advance(20, thin=2).cpu().numpy()
    two = cls(gs.TargetBatch(pdfs), x0, SEED, mode=mode)
    b = np.concatenate([two.advance(8, thin=2).cpu().numpy(), two.advance(12, thin=2).cpu().numpy()])
    assert np.array_equal(a, b) and np.array_equal(one.state, two.state)
    assert np.array_equal(one.n_tries_per_chain, two.n_tries_per_chain)
    assert np.array_equal(one.n_reject_per_chain, two.n_reject_per_chain)


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_a_run_of_the_targets(gs, mode):
    """chain_offset = 3 m: the sampler runs members 3 .. of the batch, and gives the same rows as the full run."""
    cls = gs.ShrinkageSphericalSliceSampler
    M, m = 7, 100
    pdfs = members(gs, "vmfmix_d3_k3", M)
    batch = gs.TargetBatch(pdfs)
    x0 = x0_for(gs, 3, M * m)
    full = outputs(cls(batch, x0, SEED, mode=mode), 20, 2)
    part = outputs(cls(batch, x0[3 * m:], SEED, mode=mode, chain_offset=3 * m, chains_per_target=m), 20, 2)
    for k in full:
        assert np.array_equal(part[k], full[k][..., 3 * m:] if k == "draws" else full[k][3 * m:]), k


def test_sample_in_blocks_is_one_piece(gs):
    cls = gs.ShrinkageSphericalSliceSampler
    M, m = 10, 64
    pdfs = members(gs, "bingham_d5_dense", M)
    x0 = x0_for(gs, 5, M * m)
    ref = cls(gs.TargetBatch(pdfs), x0, SEED).sample(12, burnin=6, blocks=1)
    assert ref.shape == (M * m, 12, 5)
    for blocks in (2, 5, 1000):                      # (1000: clipped to one target per block)
        s = cls(gs.TargetBatch(pdfs), x0, SEED)
        assert np.array_equal(s.sample(12, burnin=6, blocks=blocks), ref), blocks
    # the documented call: draws per target
    sep = np.stack([cls(p, x0[t * m:(t + 1) * m], SEED, chain_offset=t * m).sample(12, burnin=6) for t, p in enumerate(pdfs)])
    assert np.array_equal(ref.reshape(M, m, 12, 5), sep)


def test_diagonal_and_dense_members_mixed(gs):
    """A batch that mixes diagonal and dense A runs the dense kernels; its diagonal members alone run the diagonal ones, another
    arithmetic: compared at the project's 1e-10 over 20 steps, integer outputs exact (the pattern of
    tests/test_hip_parity.py::test_fast_equals_exact_on_the_philox_stream)."""
    cls = gs.ShrinkageSphericalSliceSampler
    m = 128
    pdfs = members(gs, "bingham_d10_diag", 3) + [gs.random_bingham(10, vmax=30.0, vmin=0.0, seed=5 + t) for t in range(3)]
    pdfs = [pdfs[i] for i in (0, 3, 1, 4, 2, 5)]
    x0 = x0_for(gs, 10, 6 * m)
    lib = gs._lib.load()
    s = cls(gs.TargetBatch(pdfs), x0, SEED, mode="fast")
    assert lib.gsss_kernel_name(s._target_dev.handle, 1, 0, 0) == b"screened_kernel<10, ScreenBingham<10>, batch>"
    alld = cls(gs.TargetBatch(pdfs[::2]), x0[:3 * m], SEED, mode="fast")
    assert lib.gsss_kernel_name(alld._target_dev.handle, 1, 0, 0) == b"screened_kernel<10, ScreenBinghamDiag<10>, batch>"
    got = outputs(s, 20, 2)
    want = separate(gs, cls, pdfs, x0, m, 20, 2, mode="fast")
    for k in ("draws", "state"):
        err = float(np.max(np.abs(got[k] - want[k])))
        print(f"mixed diagonal / dense batch, {k}: max |dx| = {err:.3e}")
        assert err < 1e-10, (k, err)
    for k in ("tries", "reject", "errors"):
        assert np.array_equal(got[k], want[k]), k


def test_kernel_names_say_batch(gs):
    lib = gs._lib.load()
    h = gs.TargetBatch(members(gs, "vmfmix_d3_k3", 3))._device_target(0, chains_per_target=64).handle
    assert lib.gsss_kernel_name(h, 0, 0, 0) == b"run_kernel<lane3, VmfMixture, batch>"
    assert lib.gsss_kernel_name(h, 1, 0, 0) == b"screened_kernel<3, ScreenVmf<3, 3>, batch>"
    assert lib.gsss_kernel_name(h, 1, 0, 2) == b"screened_kernel<3, ScreenVmf<3, 3>, batch>"      # one lane per chain whatever the placement
    assert lib.gsss_kernel_name(h, 1, gs._lib.VARIANT_FAST_DOUBLE, 0) == b"fast_kernel<3, FastVmf<3, 4>, batch>"
    assert lib.gsss_mode_supported(h, 0) == 1 and lib.gsss_mode_supported(h, 1) == 1 and lib.gsss_target_dim(h) == 3
    assert lib.gsss_variant_name(h, 1, 0) == b"fast-lane" and lib.gsss_variant_name(h, 0, 0) == b"lane3"
    hb = gs.TargetBatch(members(gs, "bingham_d12_dense", 2))._device_target(0, chains_per_target=8).handle
    assert lib.gsss_kernel_name(hb, 1, 0, 0) == b"screened_kernel<12, ScreenBingham<12>, batch>"
    assert lib.gsss_kernel_name(hb, 1, gs._lib.VARIANT_FAST_DOUBLE, 0) == b"fast_kernel<12, FastBingham<12>, batch>"
    assert lib.gsss_kernel_name(hb, 0, 0, 0) == b"run_kernel<coop4x4, Bingham, batch>"


def test_python_refusals_on_the_device(gs):
    cls = gs.ShrinkageSphericalSliceSampler
    pdfs = members(gs, "bingham_d5_dense", 4)
    batch = gs.TargetBatch(pdfs)
    x0 = x0_for(gs, 5, 4 * 32)
    s = cls(batch, x0, SEED)
    with pytest.raises(ValueError, match="running statistics"):
        s.enable_stats()
    with pytest.raises(ValueError, match="replay"):
        s.advance(1, replay=np.zeros((4 * 32, 16)))
    x = x0.reshape(4, 32, 5)
    lp = batch.log_prob(x)
    assert lp.shape == (4, 32) and np.array_equal(lp, np.stack([p.log_prob(x[t]) for t, p in enumerate(pdfs)]))
    gr = batch.gradient(x)
    assert gr.shape == (4, 32, 5) and np.array_equal(gr, np.stack([p.gradient(x[t]) for t, p in enumerate(pdfs)]))
    with pytest.raises(ValueError, match=r"\(M, n, d\)"):
        batch.log_prob(x0)
    # an edited member is uploaded again
    before = cls(batch, x0, SEED).sample(3)
    pdfs[2].A *= 2.0
    after = cls(batch, x0, SEED).sample(3)
    assert np.array_equal(before[:64], after[:64]) and not np.array_equal(before[64:96], after[64:96])


def test_c_abi_runs_a_batch_and_refuses_with_reasons(gs):
    """Through the C ABI alone (ctypes and the library's own memory helpers), as a host without Python bindings would."""
    from geosss_amd import _lib
    lib = _lib.load()
    M, m, d, steps = 3, 40, 5, 10
    pdfs = members(gs, "bingham_d5_dense", M)
    As = [np.ascontiguousarray(p.A) for p in pdfs]

    def desc(A, b=None, kind=_lib.BINGHAM, d=d):
        return _lib.TargetDesc(kind, d, 0, 0, b.ctypes.data_as(C.c_void_p) if b is not None else None, None,
                               A.ctypes.data_as(C.c_void_p), None, 0.0)

    def create(descs, m=m):
        arr = (_lib.TargetDesc * len(descs))(*descs)
        h = C.c_void_p()
        rc = lib.gsss_target_create_batch(arr, len(descs), m, 0, C.byref(h))
        return rc, h, lib.gsss_last_error().decode()

    rc, h, _ = create([desc(A) for A in As])
    assert rc == 0 and h.value and lib.gsss_target_dim(h) == d
    n = M * m
    x0 = np.ascontiguousarray(x0_for(gs, d, n).T)                     # component-major [d][n]
    bufs = {}
    for name, nbytes in (("state", 8 * d * n), ("tries", 8 * n), ("reject", 8 * n), ("err", 4 * n)):
        p = C.c_void_p()
        assert lib.gsss_malloc(C.byref(p), nbytes, 0) == 0
        assert lib.gsss_memset(p, 0, nbytes, 0, None) == 0
        bufs[name] = p
    assert lib.gsss_memcpy_h2d(bufs["state"], x0.ctypes.data, x0.nbytes, 0, None) == 0

    def args(**kw):
        a = _lib.RunArgs(state_dev=bufs["state"].value, n_tries_dev=bufs["tries"].value, n_reject_dev=bufs["reject"].value,
                         err_dev=bufs["err"].value, n_chains=n, n_steps=steps, thin=1, seed=SEED, sampler=_lib.SHRINK,
                         mode=_lib.MODE_FAST, max_tries=1 << 20)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    # every refusal first (nothing is launched: the buffers stay as they are), each with its code and its reason
    junk = bufs["tries"].value
    for kw, word in ((dict(sampler=_lib.RWMH, mode=0, stepsize_dev=junk), "Metropolis"), (dict(sampler=_lib.HMC, mode=0, stepsize_dev=junk, n_leapfrog=3), "HMC"),
                     (dict(replay_dev=junk, replay_stride=64), "replay_dev"), (dict(rng_state_dev=junk), "rng_state_dev"),
                     (dict(stats_dev=junk, stats_dirs_dev=junk), "statistics"), (dict(chain_offset=7), "chain_offset 7"),
                     (dict(n_chains=n - 1), "n_chains"), (dict(chain_offset=2 * m), "the batch holds 3")):
        a = args(**kw)
        assert lib.gsss_run(h, C.byref(a), None) == -2, kw
        assert word in lib.gsss_last_error().decode(), (kw, lib.gsss_last_error())
    out = C.c_void_p()
    assert lib.gsss_malloc(C.byref(out), 8 * n * d, 0) == 0
    assert lib.gsss_logprob(h, bufs["state"], n, out, None) == -2 and b"target batch" in lib.gsss_last_error()
    assert lib.gsss_gradient(h, bufs["state"], n, out, None) == -2 and b"target batch" in lib.gsss_last_error()
    assert lib.gsss_free(out, 0) == 0
    knots = np.ascontiguousarray(gs.brownian_curve(4, d))
    curve = _lib.TargetDesc(_lib.CURVE_VMF, d, 4, 0, None, None, None, knots.ctypes.data_as(C.c_void_p), 100.0)
    bvec = np.ones(d)
    mu1, lc1, mu2, lc2 = np.ones((1, d)), np.zeros(1), np.ones((2, d)), np.zeros(2)

    def vmf(mu, lc):
        return _lib.TargetDesc(_lib.VMF_MIXTURE, d, len(lc), 0, mu.ctypes.data_as(C.c_void_p), lc.ctypes.data_as(C.c_void_p), None, None, 0.0)

    A6 = np.eye(6)
    for descs, word in (([curve, curve], "kind 3"), ([desc(As[0]), vmf(mu1, lc1)], "one family"), ([desc(As[0]), desc(A6, d=6)], "share d"),
                        ([vmf(mu1, lc1), vmf(mu2, lc2)], "share K"), ([desc(As[0]), desc(As[1], bvec)], "linear term"),
                        ([_lib.TargetDesc(_lib.MIXTURE, d, 1, 0, None, None, None, None, 0.0)], "kind 5"),
                        ([_lib.TargetDesc(_lib.USER, d, 1, 0, None, None, None, None, 0.0)], "kind 6"),
                        ([_lib.TargetDesc(_lib.CPD, 4, 1, 0, None, None, None, None, 0.0)], "kind 4")):
        rc, hh, msg = create(descs)
        assert rc == -2 and not hh.value and word in msg, (word, rc, msg)
    assert create([desc(As[0])], m=0)[0] == -1

    # the run itself: two calls (a split launch), against the Python samplers on the members alone
    a = args(n_steps=4)
    assert lib.gsss_run(h, C.byref(a), None) == 0
    a = args(n_steps=steps - 4, step_offset=4)
    assert lib.gsss_run(h, C.byref(a), None) == 0
    assert lib.gsss_stream_synchronize(0, None) == 0
    state, tries, reject, err = np.empty((d, n)), np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int32)
    for arr, name in ((state, "state"), (tries, "tries"), (reject, "reject"), (err, "err")):
        assert lib.gsss_memcpy_d2h(arr.ctypes.data, bufs[name], arr.nbytes, 0, None) == 0
    for t, p in enumerate(pdfs):
        s = gs.ShrinkageSphericalSliceSampler(p, x0.T[t * m:(t + 1) * m], SEED, chain_offset=t * m, mode="fast")
        s.advance(steps)
        assert np.array_equal(state[:, t * m:(t + 1) * m].T, s.state), t
        assert np.array_equal(tries[t * m:(t + 1) * m], s.n_tries_per_chain)
        assert np.array_equal(reject[t * m:(t + 1) * m], s.n_reject_per_chain)
    assert not err.any()
    for p in bufs.values():
        assert lib.gsss_free(p, 0) == 0
    assert lib.gsss_target_destroy(h) == 0
