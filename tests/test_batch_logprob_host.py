"""The batch log_prob path without a GPU: the four entry points are exported and bound, their refusals need no device, the
register budget of batch_logprob_kernel against logprob_kernel's, the log-density summaries of TargetMoments.stats() against
numpy longdouble on CPU tensors, and the tie rule of the best draw."""
import re

import numpy as np
import pytest
import torch

from geosss_amd import _lib, diagnostics

E_INVALID, E_UNSUPPORTED = -1, -2
NEW = ["gsss_batch_logprob", "gsss_batch_gradient", "gsss_batch_logprob_draws", "gsss_scalar_moments"]
BOGUS = 4096  # some non-NULL address that is never read


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.gsss_abi_version() == 10 == _lib.ABI_VERSION


@pytest.mark.parametrize("fn", ["gsss_batch_logprob", "gsss_batch_gradient"])
@pytest.mark.parametrize("n", [5, 0, -1])
def test_null_handle_is_refused(fn, n):
    lib = _lib.load()
    assert getattr(lib, fn)(None, BOGUS, n, BOGUS, None) == E_INVALID
    assert lib.gsss_last_error()


@pytest.mark.parametrize("args", [(4, 8, 0), (0, 0, 0), (-1, 8, 0), (4, -8, 0), (4, 8, -1)])
def test_draws_null_handle_is_refused(args):
    lib = _lib.load()
    assert lib.gsss_batch_logprob_draws(None, BOGUS, *args, BOGUS, None) == E_INVALID
    assert lib.gsss_last_error()


# (values, n_rows, n_chains, m, acc) -> code
@pytest.mark.parametrize("args, code", [
    ((1, 4, 8, 0, 1), E_INVALID),             # m < 1
    ((1, 4, 8, 3, 1), E_INVALID),             # n_chains % m
    ((1, 4, -8, 4, 1), E_INVALID),            # negative chains
    ((1, -1, 8, 4, 1), E_INVALID),            # negative rows
    ((0, 4, 8, 4, 1), E_INVALID),             # NULL values
    ((1, 4, 8, 4, 0), E_INVALID),             # NULL acc
])
def test_scalar_moments_refusals_need_no_device(args, code):
    lib = _lib.load()
    v, n_rows, n, m, a = args
    assert lib.gsss_scalar_moments(BOGUS if v else None, n_rows, n, m, BOGUS if a else None, None, 0, None) == code
    assert lib.gsss_last_error()


def test_scalar_moments_of_nothing_is_a_no_op():
    lib = _lib.load()
    assert lib.gsss_scalar_moments(BOGUS, 0, 8, 4, BOGUS, None, 0, None) == 0
    assert lib.gsss_scalar_moments(None, 4, 0, 4, None, None, 0, None) == 0


def test_target_moments_still_refuses_one_coordinate():
    assert _lib.load().gsss_target_moments(BOGUS, 4, 8, 1, 0, 4, _lib.MOMENTS_DIAG, BOGUS, None, 0, None) == E_INVALID


def _key(name, kernel):
    """The template arguments <V, TT, GRAD> of a mangled kernel name."""
    m = re.search(kernel + r"I(.+?Lb[01]E)E", name)
    return m.group(1) if m else None


def test_batch_kernels_keep_the_register_budget_of_logprob_kernel():
    """15 layouts x {VmfMixture, Bingham} x {value, gradient}; no instantiation uses more scratch than the logprob_kernel of the
    same (V, TT, GRAD) in the single-target units, and none where that one uses none."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_batch_logprob.hip")
    assert len(ru) == 60 and all("batch_logprob_kernel" in k for k in ru), sorted(ru)
    parent = {}
    for unit in ("gsss_target_vmfmixture.hip", "gsss_target_bingham.hip"):
        for name, r in build.resource_usage(unit).items():
            if "14logprob_kernel" in name:
                parent[_key(name, "14logprob_kernel")] = r
    assert len(parent) == 60 and None not in parent
    for name, r in ru.items():
        p = parent[_key(name, "20batch_logprob_kernel")]
        print(f"{name}: vgprs {r['vgprs']} ({p['vgprs']}), scratch {r['scratch']} ({p['scratch']})")
        assert r["scratch"] <= p["scratch"], (name, r, p)


def _synthetic(M=5, m=7, R=11, seed=4):
    """A log-density-like trace (R, M m) whose chains disagree, so that R-hat is not 1."""
    g = np.random.default_rng(seed)
    return -3.0 + g.standard_normal((R, M * m)) + 0.3 * g.standard_normal((1, M * m))


def _close(got, want, tol=1e-12):
    want = np.asarray(want, dtype=np.float64)
    assert np.max(np.abs(got.numpy() - want)) <= tol * np.max(np.abs(want)), (got, want)


def test_lp_stats_against_longdouble():
    M, m, R, d = 5, 7, 11, 3
    v = _synthetic(M, m, R)
    vt = v.reshape(R, M, m)
    lp_acc = np.stack([np.full(M, float(m * R)), vt.sum((0, 2)), (vt * vt).sum((0, 2))], 1)
    # coordinates for the part of stats() that was there before: any unit vectors
    g = np.random.default_rng(1)
    x = g.standard_normal((R, d, M * m))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    xt = x.reshape(R, d, M, m)
    iu = np.triu_indices(d)
    acc = np.concatenate([np.full((M, 1), float(m * R)), xt.sum((0, 3)).T, np.einsum("ritc,rjtc->tij", xt, xt)[:, iu[0], iu[1]]], 1)
    best, row, chain = diagnostics.best_draw(torch.from_numpy(v), m)
    tm = diagnostics.TargetMoments(torch.from_numpy(acc), torch.from_numpy(x.sum(0)), d, m, True, lp_acc=torch.from_numpy(lp_acc),
                                   lp_chain_sum=torch.from_numpy(v.sum(0)), lp_best=best,
                                   x_best=torch.from_numpy(x)[row, :, chain])
    st = tm.stats()
    vl = v.astype(np.longdouble).reshape(R, M, m)
    cm = vl.mean(0)                                         # (M, m) chain means
    between = cm.var(-1, ddof=1)
    within = vl.var(0).mean(-1)
    w_unbiased = vl.var(0, ddof=1).mean(-1)
    _close(st["lp_mean"], vl.mean((0, 2)))
    _close(st["lp_var"], vl.transpose(1, 0, 2).reshape(M, -1).var(-1))
    _close(st["lp_rhat"], np.sqrt(((R - 1) / R * w_unbiased + between) / w_unbiased))
    _close(st["lp_ess_between"], (within + between) / between)
    assert float(st["lp_rhat"].min()) > 1.0
    assert np.array_equal(st["lp_best"].numpy(), v.reshape(R, M, m).max((0, 2)))
    for t in range(M):
        assert np.array_equal(st["x_best"][t].numpy(), x[int(row[t]), :, int(chain[t])])
        assert v[int(row[t]), int(chain[t])] == float(best[t]) and t * m <= int(chain[t]) < (t + 1) * m
    # the coordinates' entries are the ones stats() had, and a summary without the trace has no lp_ entry
    plain = diagnostics.TargetMoments(tm.acc, tm.chain_sum, d, m, True).stats()
    assert not any(k.startswith("lp_") or k == "x_best" for k in plain)
    assert set(st) - set(plain) == {"lp_mean", "lp_var", "lp_rhat", "lp_ess_between", "lp_best", "x_best"}
    assert all(torch.equal(st[k], plain[k]) for k in plain)


def test_best_draw_takes_the_first_occurrence():
    """Ties go to the earliest row, then to the lowest chain; a later window replaces the best only if strictly better."""
    M, m, R = 3, 4, 5
    v = np.random.default_rng(2).uniform(-9.0, -1.0, (R, M * m))
    top = 0.5
    v[3, 1] = v[1, 2] = v[1, 3] = top        # target 0: rows 1 and 3 tie, and two chains within row 1
    v[4, 4] = v[4, 7] = top                  # target 1: two chains of the last row
    v[0, 11] = v[2, 8] = top                 # target 2: a high chain in row 0 against a low chain in row 2
    best, row, chain = diagnostics.best_draw(torch.from_numpy(v), m)
    assert best.tolist() == [top] * 3 and row.tolist() == [1, 4, 0] and chain.tolist() == [2, 4, 11]
    # without ties it is the plain argmax
    w = np.random.default_rng(3).standard_normal((R, M * m))
    best, row, chain = diagnostics.best_draw(torch.from_numpy(w), m)
    flat = w.reshape(R, M, m).transpose(1, 0, 2).reshape(M, R * m)
    assert np.array_equal(row.numpy(), flat.argmax(1) // m) and np.array_equal(chain.numpy(), np.arange(M) * m + flat.argmax(1) % m)
    # the running update: an equal value in a later window does not move the best draw
    d = 3
    x1, x2 = torch.randn(R, d, M * m, dtype=torch.float64), torch.randn(R, d, M * m, dtype=torch.float64)
    tm = diagnostics.TargetMoments(torch.zeros(M, 1 + d + 6), torch.zeros(d, M * m), d, m, True,
                                   lp_best=torch.full((M,), float("-inf"), dtype=torch.float64),
                                   x_best=torch.zeros(M, d, dtype=torch.float64))
    tm.update_best(torch.from_numpy(v), x1)
    assert tm.lp_best.tolist() == [top] * 3 and torch.equal(tm.x_best[0], x1[1, :, 2])
    v2 = v.copy()
    v2[0, 5] = top + 1.0                     # only target 1 improves
    tm.update_best(torch.from_numpy(v2), x2)
    assert tm.lp_best.tolist() == [top, top + 1.0, top]
    assert torch.equal(tm.x_best[0], x1[1, :, 2]) and torch.equal(tm.x_best[1], x2[0, :, 5]) and torch.equal(tm.x_best[2], x1[0, :, 11])
