"""Per-target moments without a GPU: the row counts and refusals of gsss_target_moments (no device is touched), the register
budget of its kernels, and from_target_moments against numpy longdouble on CPU tensors."""
import numpy as np
import pytest
import torch

from geosss_amd import _lib, diagnostics

E_INVALID, E_UNSUPPORTED = -1, -2


def test_moments_rows():
    lib = _lib.load()
    assert lib.gsss_moments_rows(3, 0) == 1 + 3 + 6
    assert lib.gsss_moments_rows(16, 0) == 1 + 16 + 136
    assert lib.gsss_moments_rows(50, _lib.MOMENTS_DIAG) == 1 + 50 + 50
    assert lib.gsss_moments_rows(17, 0) < 0
    assert lib.gsss_moments_rows(1, 0) < 0 and lib.gsss_moments_rows(1, _lib.MOMENTS_DIAG) < 0


def test_abi_version_is_unchanged():
    assert _lib.load().gsss_abi_version() == 10 == _lib.ABI_VERSION


# (samples, n_rows, n_chains, d, chain_rows, m, flags, acc) -> code; pointers: 1 = some non-NULL address that is never read
@pytest.mark.parametrize("args, code", [
    ((1, 4, 8, 1, 0, 4, 0, 1), E_INVALID),            # d < 2
    ((1, 4, 8, 3, 0, 0, 0, 1), E_INVALID),            # m < 1
    ((1, 4, 8, 3, 0, 3, 0, 1), E_INVALID),            # n_chains % m
    ((0, 4, 8, 3, 0, 4, 0, 1), E_INVALID),            # NULL samples
    ((1, 4, 8, 3, 0, 4, 0, 0), E_INVALID),            # NULL acc
    ((1, -1, 8, 3, 0, 4, 0, 1), E_INVALID),           # negative row count
    ((1, 4, 8, 3, 3, 4, 0, 1), E_INVALID),            # 0 < samples_chain_rows < n_rows
    ((1, 4, 8, 17, 0, 4, 0, 1), E_UNSUPPORTED),       # the full triangle at d > 16
])
def test_refusals_need_no_device(args, code):
    lib = _lib.load()
    s, n_rows, n, d, chain_rows, m, flags, a = args
    bogus = 4096
    assert lib.gsss_target_moments(bogus if s else None, n_rows, n, d, chain_rows, m, flags, bogus if a else None, None, 0,
                                   None) == code
    assert lib.gsss_last_error()


def test_no_rows_is_a_no_op():
    assert _lib.load().gsss_target_moments(4096, 0, 8, 3, 0, 4, 0, 4096, None, 0, None) == 0


def test_moments_kernels_do_not_spill():
    """Every kernel of the unit keeps its sums in registers: no scratch at any D it instantiates (d = 2 .. 16 with the full
    triangle and with the diagonal, the any-d diagonal kernel, the two fold kernels)."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_moments.hip")
    assert sum("moments_kernel" in k for k in ru) == 30 and len(ru) == 33, sorted(ru)
    for name, r in ru.items():
        assert r["scratch"] == 0, (name, r)


def _synthetic(M=5, m=7, R=11, d=4, seed=3):
    g = np.random.default_rng(seed)
    x = g.standard_normal((R, d, M * m))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x += 0.3 * g.standard_normal((1, d, M * m))      # chains that disagree, so that R-hat is not 1
    T = d * (d + 1) // 2
    acc = np.zeros((M, 1 + d + T))
    xt = x.reshape(R, d, M, m)
    acc[:, 0] = m * R
    acc[:, 1:1 + d] = xt.sum((0, 3)).T
    iu = np.triu_indices(d)
    acc[:, 1 + d:] = np.einsum("ritc,rjtc->tij", xt, xt)[:, iu[0], iu[1]]
    return x, acc, x.sum(0)


def _close(got, want, tol=1e-12):
    want = np.asarray(want, dtype=np.float64)
    assert np.max(np.abs(got.numpy() - want)) <= tol * np.max(np.abs(want)), (got, want)


def test_from_target_moments_against_longdouble():
    M, m, R, d = 5, 7, 11, 4
    x, acc, cs = _synthetic(M, m, R, d)
    out = diagnostics.from_target_moments(torch.from_numpy(acc), d, chain_sum=torch.from_numpy(cs), chains_per_target=m)
    xl = x.astype(np.longdouble).reshape(R, d, M, m)
    mean = xl.mean((0, 3)).T                                              # (M, d)
    sm = np.einsum("ritc,rjtc->tij", xl, xl) / (m * R)
    _close(out["n"], np.full(M, m * R), 0.0)
    _close(out["mean"], mean)
    _close(out["second_moment"], sm)
    _close(out["cov"], sm - mean[:, :, None] * mean[:, None, :])
    _close(out["resultant_length"], np.sqrt((mean ** 2).sum(1)))
    cm = xl.mean(0)                                                       # (d, M, m) chain means
    between = cm.var(-1, ddof=1).T
    w_unbiased = xl.var(0, ddof=1).mean(-1).T                             # mean of the chains' unbiased variances
    var_plus = (R - 1) / R * w_unbiased + between
    _close(out["between"], between)
    _close(out["within"], xl.var(0).mean(-1).T)
    _close(out["rhat"], np.sqrt(var_plus / w_unbiased))
    _close(out["ess_between"], (xl.var(0).mean(-1).T + between) / between)
    # the diagonal form gives the same per-coordinate quantities
    acc_d = np.concatenate([acc[:, :1 + d], np.stack([acc[:, 1 + d + i] for i in np.cumsum([0] + list(range(d, 1, -1)))], 1)], 1)
    out_d = diagnostics.from_target_moments(torch.from_numpy(acc_d), d, chain_sum=torch.from_numpy(cs), chains_per_target=m,
                                            second_moment=False)
    assert torch.equal(out_d["rhat"], out["rhat"]) and "second_moment" not in out_d
    _close(out_d["second_moment_diag"], np.einsum("tii->ti", sm))


def test_ess_between_is_ess_between_chains():
    M, m, R, d = 5, 7, 11, 4
    x, acc, cs = _synthetic(M, m, R, d)
    out = diagnostics.from_target_moments(torch.from_numpy(acc), d, chain_sum=torch.from_numpy(cs), chains_per_target=m)
    t, j = 2, 1
    series = x[:, j, t * m:(t + 1) * m]                                   # (R, m)
    want = diagnostics.ess_between_chains(series.mean(0), np.full(m, R), series.var(0))["ess_per_chain"]
    assert abs(float(out["ess_between"][t, j]) - want) <= 1e-12 * want


def test_target_moments_checks_its_arguments():
    with pytest.raises(ValueError):
        diagnostics.target_moments(torch.zeros((2, 3, 8), dtype=torch.float64), 4)  # not a device tensor
    with pytest.raises(ValueError):
        diagnostics._moments_form(17, True)
    assert diagnostics._moments_form(17, None) == (False, 1 + 34) and diagnostics._moments_form(5, None) == (True, 1 + 5 + 15)
