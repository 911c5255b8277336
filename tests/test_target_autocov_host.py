"""Per-target lagged products without a GPU: the row counts and refusals of gsss_target_autocov (no device is touched), the
register budget of its kernels, and from_target_autocov on CPU tensors against a numpy longdouble evaluation of the estimator
from stored series and, at one chain per target, against diagnostics.acf / iat_from_acf."""
import numpy as np
import pytest
import torch

from geosss_amd import _lib, diagnostics

E_INVALID, E_UNSUPPORTED = -1, -2


def test_autocov_rows():
    lib = _lib.load()
    assert lib.gsss_autocov_rows(1, 1) == 1 * 2 * 3
    assert lib.gsss_autocov_rows(5, 32) == 5 * 33 * 3
    assert lib.gsss_autocov_rows(40, 64) == 40 * 65 * 3
    assert lib.gsss_autocov_rows(0, 8) == E_INVALID and lib.gsss_autocov_rows(3, 0) == E_INVALID
    assert lib.gsss_autocov_rows(3, 65) == E_UNSUPPORTED


def test_abi_version_is_unchanged():
    assert _lib.load().gsss_abi_version() == 10 == _lib.ABI_VERSION


# (ring, ring_rows, first_row, n_rows, n_hist, n_chains, d, m, n_lags, acc) -> code; pointers: 1 = some non-NULL address that is
# never read
@pytest.mark.parametrize("args, code", [
    ((1, 12, 0, 4, 0, 8, 0, 4, 8, 1), E_INVALID),        # d < 1
    ((1, 12, 0, 4, 0, 8, 3, 0, 8, 1), E_INVALID),        # m < 1
    ((1, 12, 0, 4, 0, 8, 3, 3, 8, 1), E_INVALID),        # n_chains % m
    ((1, 12, 0, 4, 0, 8, 3, 4, 0, 1), E_INVALID),        # n_lags < 1
    ((1, 12, 0, -1, 0, 8, 3, 4, 8, 1), E_INVALID),       # negative row count
    ((1, 12, -1, 4, 0, 8, 3, 4, 8, 1), E_INVALID),       # negative first row
    ((1, 12, 0, 4, -1, 8, 3, 4, 8, 1), E_INVALID),       # negative history
    ((1, 12, 0, 4, 0, -8, 3, 4, 8, 1), E_INVALID),       # negative chain count
    ((1, 12, 9, 4, 0, 8, 3, 4, 8, 1), E_INVALID),        # first_row + n_rows > ring_rows
    ((1, 20, 0, 4, 9, 8, 3, 4, 8, 1), E_INVALID),        # n_hist > n_lags
    ((1, 12, 0, 8, 5, 8, 3, 4, 8, 1), E_INVALID),        # n_hist > ring_rows - n_rows
    ((0, 12, 0, 4, 0, 8, 3, 4, 8, 1), E_INVALID),        # NULL ring
    ((1, 12, 0, 4, 0, 8, 3, 4, 8, 0), E_INVALID),        # NULL acc
    ((1, 80, 0, 4, 0, 8, 3, 4, 65, 1), E_UNSUPPORTED),   # more than 64 lags
])
def test_refusals_need_no_device(args, code):
    lib = _lib.load()
    r, ring_rows, first_row, n_rows, n_hist, n, d, m, n_lags, a = args
    bogus = 4096
    assert lib.gsss_target_autocov(bogus if r else None, ring_rows, first_row, n_rows, n_hist, n, d, m, n_lags,
                                   bogus if a else None, 0, None) == code
    assert lib.gsss_last_error()


def test_no_rows_is_a_no_op():
    lib = _lib.load()
    assert lib.gsss_target_autocov(4096, 12, 3, 0, 2, 8, 3, 4, 8, 4096, 0, None) == 0
    assert lib.gsss_target_autocov(None, 0, 0, 0, 0, 8, 1, 4, 8, None, 0, None) == 0


def test_autocov_kernels_do_not_spill():
    """The four builds of the lag kernel (8 or 16 lags per group of wavefronts, 1, 2 or 4 groups) and the fold kernel keep their
    sums and their delay line in registers: no scratch."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_autocov.hip")
    assert sum("autocov_kernel" in k for k in ru) == 4 and len(ru) == 5, sorted(ru)
    for name, r in ru.items():
        assert r["scratch"] == 0, (name, r)


def _series(M, m, n, d, seed, offset=3.0, rho=0.8):
    """(n, d, M m): AR(1) series far from zero, so that the end terms of the estimator carry weight."""
    g = np.random.default_rng(seed)
    e = g.standard_normal((n, d, M * m))
    x = np.empty_like(e)
    x[0] = e[0]
    for r in range(1, n):
        x[r] = rho * x[r - 1] + np.sqrt(1 - rho * rho) * e[r]
    return x + offset + 0.2 * g.standard_normal((1, d, M * m))


def _sums(x, m, L):
    """The accumulators (M, d, L + 1, 3) of stored series x (n, d, M m), in longdouble."""
    n, d, N = x.shape
    xl = x.astype(np.longdouble).reshape(n, d, N // m, m)
    acc = np.zeros((N // m, d, L + 1, 3), dtype=np.longdouble)
    for lag in range(L + 1):
        lead, trail = xl[lag:], xl[:n - lag]
        acc[:, :, lag, 0] = (lead * trail).sum((0, 3)).T
        acc[:, :, lag, 1] = lead.sum((0, 3)).T
        acc[:, :, lag, 2] = trail.sum((0, 3)).T
    return acc


def _direct_acf(x, m, L):
    """The pooled-centred direct estimator from the stored series themselves (no lagged sums), in longdouble: (M, d, L + 1)."""
    n, d, N = x.shape
    xl = x.astype(np.longdouble).reshape(n, d, N // m, m)
    z = xl - xl.mean((0, 3), keepdims=True)
    cov = np.stack([(z[lag:] * z[:n - lag]).mean((0, 3)).T for lag in range(L + 1)], -1)
    return cov / cov[..., :1]


@pytest.mark.parametrize("M, m, n, d, L", [(4, 5, 57, 3, 12), (3, 1, 40, 2, 7), (2, 16, 66, 1, 64)])
def test_from_target_autocov_against_longdouble(M, m, n, d, L):
    x = _series(M, m, n, d, seed=n + L)
    acc = _sums(x, m, L)
    out = diagnostics.from_target_autocov(torch.from_numpy(acc.astype(np.float64)), m, n)
    want = _direct_acf(x, m, L)
    assert tuple(out["acf"].shape) == (M, d, L + 1) and tuple(out["iat"].shape) == (M, d)
    # The quotient of two covariances, each a difference of terms of size E[x^2]: a few roundings of E[x^2] / cov_0 each, and
    # the accumulators were rounded to double once.
    tol = 64 * 2.0 ** -52 * float((x * x).mean() / x.var(0).min())
    assert np.max(np.abs(out["acf"].numpy() - want)) <= tol
    iat = diagnostics.iat_from_acf(torch.from_numpy(want.astype(np.float64)))
    assert torch.allclose(out["iat"], iat, rtol=1e-9, atol=0)
    assert torch.allclose(out["ess_within"], m * n / iat, rtol=1e-9, atol=0)
    assert torch.equal(out["iat_truncated"], ~diagnostics.pair_sum_went_negative(out["acf"]))
    # n per target instead of one number
    per = diagnostics.from_target_autocov(torch.from_numpy(acc.astype(np.float64)), m, torch.full((M,), float(n)))
    assert torch.equal(per["acf"], out["acf"]) and torch.equal(per["ess_within"], out["ess_within"])


def test_one_chain_per_target_is_diagnostics_acf():
    M, n, d, L = 6, 57, 2, 12
    x = _series(M, 1, n, d, seed=9)
    out = diagnostics.from_target_autocov(torch.from_numpy(_sums(x, 1, L).astype(np.float64)), 1, n)
    series = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 1, 0)))          # (M, d, n)
    want = diagnostics.acf(series, n_max=L + 1)
    tol = 64 * 2.0 ** -52 * float((x * x).mean() / x.var(0).min())
    assert float((out["acf"] - want).abs().max()) <= tol
    assert torch.allclose(out["iat"], diagnostics.iat_from_acf(want), rtol=1e-9, atol=0)


def test_arguments_are_checked():
    acc = torch.zeros((2, 3, 9, 3), dtype=torch.float64)
    with pytest.raises(ValueError):
        diagnostics.from_target_autocov(acc, 4, 8)                                  # n <= L
    with pytest.raises(ValueError):
        diagnostics.from_target_autocov(acc[..., :2], 4, 50)
    with pytest.raises(ValueError):
        diagnostics.target_autocov(torch.zeros((4, 3, 8), dtype=torch.float64), 4, 8)   # not a device tensor
