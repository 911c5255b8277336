"""Per-target step length, hopping and mode occupancy without a GPU: the row counts and refusals of gsss_target_mixing (no
device is touched), the register budget of its kernels, from_target_mixing on CPU tensors against a numpy evaluation from stored
series, and TargetBatch.mixing_directions against the members' own defaults."""
import numpy as np
import pytest
import torch

import geosss_amd as gs
from geosss_amd import _lib, diagnostics

E_INVALID, E_UNSUPPORTED = -1, -2
TRANSITIONS = 1


def test_mixing_rows():
    lib = _lib.load()
    for K in (0, 1, 3, 16):
        assert lib.gsss_mixing_rows(K, 0) == 3 + K
        assert lib.gsss_mixing_rows(K, TRANSITIONS) == 3 + K + K * K
    assert lib.gsss_mixing_rows(-1, 0) == E_INVALID and lib.gsss_mixing_rows(3, 2) == E_INVALID
    assert lib.gsss_mixing_rows(17, 0) == E_UNSUPPORTED and lib.gsss_mixing_rows(17, TRANSITIONS) == E_UNSUPPORTED
    assert _lib.MIXING_TRANSITIONS == TRANSITIONS


def test_abi_version_is_unchanged():
    assert _lib.load().gsss_abi_version() == 10 == _lib.ABI_VERSION


# (ring, ring_rows, first_row, n_rows, n_hist, n_chains, d, m, dirs, n_modes, flags, step, count) -> code; pointers: 1 = some
# non-NULL address that is never read
@pytest.mark.parametrize("args, code", [
    ((1, 12, 0, 4, 0, 8, 1, 4, 1, 3, 0, 1, 1), E_INVALID),        # d < 2
    ((1, 12, 0, 4, 0, 8, 3, 0, 1, 3, 0, 1, 1), E_INVALID),        # m < 1
    ((1, 12, 0, 4, 0, 8, 3, 3, 1, 3, 0, 1, 1), E_INVALID),        # n_chains % m
    ((1, 12, 0, -1, 0, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),       # negative row count
    ((1, 12, -1, 4, 0, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),       # negative first row
    ((1, 12, 0, 4, -1, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),       # negative history
    ((1, 12, 0, 4, 0, -8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),       # negative chain count
    ((1, -12, 0, 4, 0, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),       # negative ring
    ((1, 12, 9, 4, 0, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),        # first_row + n_rows > ring_rows
    ((1, 12, 0, 4, 2, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),        # n_hist > 1
    ((1, 12, 0, 12, 1, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),       # n_hist > ring_rows - n_rows
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, -1, 0, 1, 1), E_INVALID),       # n_modes < 0
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 2, 1, 1), E_INVALID),        # unknown flags
    ((0, 12, 0, 4, 0, 8, 3, 4, 1, 3, 0, 1, 1), E_INVALID),        # NULL ring
    ((1, 12, 0, 4, 0, 8, 3, 4, 0, 3, 0, 1, 1), E_INVALID),        # NULL dirs
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 0, 0, 1), E_INVALID),        # NULL step
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 0, 1, 0), E_INVALID),        # NULL count
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 17, 0, 1, 1), E_UNSUPPORTED),   # more than 16 modes
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 17, 1, 1, 1), E_UNSUPPORTED),
])
def test_refusals_need_no_device(args, code):
    lib = _lib.load()
    r, ring_rows, first_row, n_rows, n_hist, n, d, m, dr, K, flags, s, c = args
    bogus = 4096
    assert lib.gsss_target_mixing(bogus if r else None, ring_rows, first_row, n_rows, n_hist, n, d, m, bogus if dr else None, K,
                                  flags, bogus if s else None, bogus if c else None, 0, None) == code
    assert lib.gsss_last_error()


def test_no_rows_is_a_no_op():
    lib = _lib.load()
    assert lib.gsss_target_mixing(4096, 12, 3, 0, 1, 8, 3, 4, 4096, 3, 1, 4096, 4096, 0, None) == 0
    assert lib.gsss_target_mixing(None, 0, 0, 0, 0, 8, 2, 4, None, 0, 0, None, None, 0, None) == 0


def test_mixing_kernels_do_not_spill():
    """The fifteen builds with a compile-time d = 2 .. 16, the one with a run-time d and the fold kernel keep a lane's draws
    and sums in registers: no scratch."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_mixing.hip")
    assert sum("mixing_kernel" in k for k in ru) == 16 and sum("mixing_fold_kernel" in k for k in ru) == 1 and len(ru) == 17, sorted(ru)
    for name, r in ru.items():
        assert r["scratch"] == 0, (name, r)


def _walk(M, m, n, d, seed):
    """(n, d, M m): random walks on the sphere, steps log-uniform in 1e-3 .. pi."""
    g = np.random.default_rng(seed)
    x = np.empty((n, M * m, d))
    x[0] = g.standard_normal((M * m, d))
    x[0] /= np.linalg.norm(x[0], axis=1, keepdims=True)
    for r in range(1, n):
        t = g.standard_normal((M * m, d))
        t -= (t * x[r - 1]).sum(1, keepdims=True) * x[r - 1]
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        th = np.exp(g.uniform(np.log(1e-3), np.log(np.pi), (M * m, 1)))
        x[r] = np.cos(th) * x[r - 1] + np.sin(th) * t
        x[r] /= np.linalg.norm(x[r], axis=1, keepdims=True)
    return np.ascontiguousarray(x.transpose(0, 2, 1))


def _accumulators(x, m, hop, modes, transitions):
    """step (M, 2) and counts (M, 3 + K [+ K K]) of stored series x (n, d, M m) against hop (M, d) and modes (M, K, d)."""
    n, d, N = x.shape
    M, K = N // m, modes.shape[1]
    xs = x.transpose(2, 0, 1).reshape(M, m, n, d)                                    # (M, m, n, d)
    theta = np.arccos(np.clip((xs[:, :, 1:] * xs[:, :, :-1]).sum(-1), -1.0, 1.0))
    step = np.stack([theta.sum((1, 2)), (theta * theta).sum((1, 2))], 1)
    side = np.sign(np.einsum("tcnd,td->tcn", xs, hop))
    counts = np.zeros((M, 3 + K + (K * K if transitions else 0)), dtype=np.int64)
    counts[:, 0], counts[:, 1] = m * n, m * (n - 1)
    counts[:, 2] = (side[:, :, 1:] != side[:, :, :-1]).sum((1, 2))
    if K:
        mode = np.argmax(np.einsum("tcnd,tkd->tcnk", xs, modes), -1)                 # (M, m, n)
        for t in range(M):
            counts[t, 3:3 + K] = np.bincount(mode[t].ravel(), minlength=K)
            if transitions:
                pair = mode[t, :, :-1] * K + mode[t, :, 1:]
                counts[t, 3 + K:] = np.bincount(pair.ravel(), minlength=K * K)
    return step, counts


def _directions(M, K, d, seed):
    g = np.random.default_rng(seed)
    v = g.standard_normal((M, 1 + K, d))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return v[:, 0], v[:, 1:]


@pytest.mark.parametrize("M, m, n, d, K", [(4, 5, 57, 3, 3), (3, 1, 40, 2, 0), (2, 16, 66, 16, 16)])
@pytest.mark.parametrize("transitions", [False, True])
def test_from_target_mixing_against_numpy(M, m, n, d, K, transitions):
    x = _walk(M, m, n, d, seed=n + K)
    hop, modes = _directions(M, K, d, seed=d)
    step, counts = _accumulators(x, m, hop, modes, transitions)
    g = np.random.default_rng(K)
    weights = g.random((M, K)) + 0.1
    weights /= weights.sum(1, keepdims=True)
    out = diagnostics.from_target_mixing(torch.from_numpy(step), torch.from_numpy(counts), K, weights=weights if K else None)
    pairs, draws = counts[:, 1].astype(np.float64), counts[:, 0].astype(np.float64)
    assert np.array_equal(pairs, np.full(M, m * (n - 1))) and np.array_equal(draws, np.full(M, m * n))

    def close(got, want):
        got = got.numpy()
        assert got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), (got, want)

    close(out["geodesic_step"], step[:, 0] / pairs)
    close(out["hop_frequency"], counts[:, 2] / pairs)
    close(out["mode_occupancy"], counts[:, 3:3 + K] / draws[:, None])
    # the variance is a difference of two terms of the size of E[theta^2]: a few roundings of that, under the root
    mean = step[:, 0] / pairs
    var = step[:, 1] / pairs - mean * mean
    assert np.all(var > 1e-3)
    assert np.all(np.abs(out["geodesic_step_sd"].numpy() - np.sqrt(var)) <= 8 * 2.0 ** -52 * (step[:, 1] / pairs) / np.sqrt(var))
    if K:
        assert np.array_equal(counts[:, 3:3 + K].sum(1), draws)
        for t in range(M):
            want = diagnostics.mode_kl(counts[t, 3:3 + K] / draws[t], weights[t])
            assert abs(float(out["mode_kl"][t]) - want) <= 1e-15 * max(abs(want), 1.0)
        shared = diagnostics.from_target_mixing(step, counts, K, weights=weights[0])
        assert abs(float(shared["mode_kl"][0]) - float(out["mode_kl"][0])) <= 1e-15
    else:
        assert "mode_kl" not in out and tuple(out["mode_occupancy"].shape) == (M, 0)
        with pytest.raises(ValueError):
            diagnostics.from_target_mixing(step, counts, K, weights=np.ones(1))
    if transitions and K:
        tr = counts[:, 3 + K:].reshape(M, K, K).astype(np.float64)
        assert np.array_equal(tr.sum((1, 2)), pairs)
        with np.errstate(invalid="ignore"):
            want = tr / tr.sum(-1, keepdims=True)
        got = out["mode_transitions"].numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.all(np.abs(got - want)[~np.isnan(want)] <= 1e-15 * want[~np.isnan(want)])
        close(out["mode_switch_frequency"], (pairs - np.trace(tr, axis1=1, axis2=2)) / pairs)
    else:
        assert "mode_transitions" not in out and "mode_switch_frequency" not in out


def test_an_empty_mode_takes_the_floor_of_mode_kl():
    step = torch.tensor([[3.0, 2.0]], dtype=torch.float64)
    counts = torch.tensor([[10, 9, 0, 10, 0]])
    out = diagnostics.from_target_mixing(step, counts, 2, weights=[0.5, 0.5])
    assert float(out["mode_kl"][0]) == diagnostics.mode_kl(np.array([1.0, 0.0]), np.array([0.5, 0.5]))


def test_mixing_directions_of_a_vmf_mixture_batch():
    g = np.random.default_rng(4)
    pdfs = []
    for _ in range(5):
        mu = g.standard_normal((3, 4))
        mu *= (5.0 + 20.0 * g.random((3, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
        pdfs.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(3) + 0.5))
    hop, modes, weights = gs.TargetBatch(pdfs).mixing_directions()
    assert hop.shape == (5, 4) and modes.shape == (5, 3, 4) and weights.shape == (5, 3)
    for t, p in enumerate(pdfs):
        assert np.array_equal(modes[t], np.array(p._modes()))
        assert np.array_equal(hop[t], np.array(p._modes())[0])
        assert np.array_equal(weights[t], p.weights) and abs(weights[t].sum() - 1.0) < 1e-15
    # single vMF members: one term each
    single = [gs.VonMisesFisher(10.0 * np.eye(3)[i]) for i in range(3)]
    hop, modes, weights = gs.TargetBatch(single).mixing_directions()
    assert modes.shape == (3, 1, 3) and np.array_equal(weights, np.ones((3, 1)))
    for t, p in enumerate(single):
        assert np.array_equal(modes[t, 0], p.mu) and np.array_equal(hop[t], p.mu)


def test_mixing_directions_of_a_bingham_batch():
    pdfs = [gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=s) for s in (3, 4, 5, 6)]
    hop, modes, weights = gs.TargetBatch(pdfs).mixing_directions()
    assert hop.shape == (4, 5) and modes.shape == (4, 0, 5) and weights is None
    for t, p in enumerate(pdfs):
        assert np.array_equal(hop[t], p.mode)


def test_arguments_are_checked():
    x = torch.zeros((4, 3, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        diagnostics.target_mixing(x, 4)                                               # not a device tensor
    with pytest.raises(ValueError, match="CUDA"):
        diagnostics.target_mixing(x, 4, hop=np.ones(3), modes=np.ones((2, 5, 3)))     # right shapes, still no device tensor
    with pytest.raises(ValueError, match="hop"):
        diagnostics.target_mixing(x, 4, hop=np.ones(4))
    with pytest.raises(ValueError, match="hop"):
        diagnostics.target_mixing(x, 4, hop=np.ones((3, 3)))
    with pytest.raises(ValueError, match="modes"):
        diagnostics.target_mixing(x, 4, modes=np.ones((2, 4)))
    with pytest.raises(ValueError, match="modes"):
        diagnostics.target_mixing(x, 4, modes=np.ones((3, 2, 3)))
    with pytest.raises(ValueError, match="16"):
        diagnostics.target_mixing(x, 4, modes=np.ones((17, 3)))
    with pytest.raises(ValueError):
        diagnostics.target_mixing(x, 3)                                               # n_chains % m
    with pytest.raises(ValueError):
        diagnostics.from_target_mixing(torch.zeros((2, 2)), torch.zeros((2, 7), dtype=torch.int64), 3)   # neither 6 nor 15 columns
    with pytest.raises(ValueError):
        diagnostics.from_target_mixing(torch.zeros((2, 2)), torch.zeros((2, 6), dtype=torch.int64), 3, weights=np.ones(2))
