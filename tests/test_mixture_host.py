"""MixtureModel with components other than von Mises-Fisher (distributions.py:209-227): flattening, weights, packing
and the device cache key -- host side only, no GPU."""
import numpy as np
import pytest

import geosss_amd as gs
from geosss_amd import _lib


def _bingham(d, seed):
    return gs.random_bingham(d=d, vmax=10.0, vmin=0.0, seed=seed)


def test_bingham_mixture_is_a_target():
    """The README example: two Bingham girdles as one target, packed as a GSSS_MIXTURE of two Bingham components."""
    mix = gs.MixtureModel([_bingham(5, 1), _bingham(5, 2)])
    kind, d, k, _, arrays, extra = mix._pack()
    assert (kind, d, k, arrays) == (_lib.MIXTURE, 5, 2, ())
    assert [c[0] for c in extra["components"]] == [_lib.BINGHAM, _lib.BINGHAM]
    assert np.allclose(extra["log_weights"], np.log(0.5))
    assert np.array_equal(extra["components"][1][4][2], mix.pdfs[1].A)


def test_nested_mixture_is_flattened_with_weight_products():
    v1, v2 = gs.VonMisesFisher([5.0, 0.0, 0.0]), gs.VonMisesFisher([0.0, 5.0, 0.0])
    B = gs.Bingham(np.diag([1.0, 0.0, -1.0]))
    mix = gs.MixtureModel([gs.MixtureModel([v1, v2], [1.0, 3.0]), B], [0.4, 0.6])
    terms = mix._terms()
    assert [p for p, _ in terms] == [v1, v2, B]
    assert np.allclose([w for _, w in terms], [0.1, 0.3, 0.6])
    kind, d, k, _, _, extra = mix._pack()
    assert (kind, d, k) == (_lib.MIXTURE, 3, 2)
    vm, bg = extra["components"]
    assert vm[0] == _lib.VMF_MIXTURE and vm[2] == 2 and bg[0] == _lib.BINGHAM
    # the vMF terms' weights sit in their logc, the component itself has log w = 0
    assert np.allclose(vm[4][1], [v1._log_const() + np.log(0.1), v2._log_const() + np.log(0.3)])
    assert np.allclose(extra["log_weights"], [0.0, np.log(0.6)])


def test_dimensionless_uniform_takes_the_siblings_dimension():
    mix = gs.MixtureModel([gs.VonMisesFisher([0.0, 0.0, 20.0]), gs.Uniform()], [0.9, 0.1])
    assert mix.d == 3
    _, _, _, _, _, extra = mix._pack()
    u = extra["components"][1]
    assert u[0] == _lib.BINGHAM and u[1] == 3 and not np.any(u[4][2])
    with pytest.raises(TypeError):
        gs.MixtureModel([gs.Uniform(), gs.Uniform()])._pack()  # no dimension anywhere


def test_all_vmf_mixture_packs_as_before():
    mus = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
    w = [0.2, 0.5, 0.3]
    mix = gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], w)
    kind, d, k, kappa, (mu, logc, A, knots) = mix._pack()
    assert (kind, d, k, kappa, A, knots) == (_lib.VMF_MIXTURE, 3, 3, 0.0, None, None)
    assert np.array_equal(mu, mus)
    want = np.array([gs.VonMisesFisher(m)._log_const() for m in mus]) + np.log(np.array(w) / np.sum(w))
    assert np.array_equal(logc, want)


def test_editing_a_component_changes_the_device_key():
    mix = gs.MixtureModel([_bingham(4, 3), gs.BinghamFisher(np.eye(4), np.ones(4))])
    key = gs.Distribution._device_key(mix._pack())
    assert gs.Distribution._device_key(mix._pack()) == key
    mix.pdfs[1].A = mix.pdfs[1].A * 2.0
    assert gs.Distribution._device_key(mix._pack()) != key
    key2 = gs.Distribution._device_key(mix._pack())
    mix.pdfs[1].b = mix.pdfs[1].b + 1.0
    assert gs.Distribution._device_key(mix._pack()) != key2


def test_refused_components():
    mus = [[3.0, 0.0, 0.0], [0.0, 3.0, 0.0]]
    C = np.eye(3)
    for bad in (gs.ACG(C), gs.MultivariateNormal(np.zeros(3), C)):
        with pytest.raises(TypeError):
            gs.MixtureModel([gs.VonMisesFisher(mus[0]), bad])
    with pytest.raises(TypeError):
        gs.MixtureModel([gs.MarginalVonMisesFisher(0, mus[0]), gs.Bingham(C)])
    with pytest.raises(TypeError):
        gs.MixtureModel([gs.MarginalVonMisesFisher(0, m) for m in mus])._pack()
    with pytest.raises(ValueError):
        gs.MixtureModel([gs.VonMisesFisher(mus[0]), _bingham(4, 1)])


def test_stats_modes_of_the_terms():
    v = gs.VonMisesFisher([0.0, 4.0, 0.0])
    B = gs.Bingham(np.diag([0.0, 0.0, 3.0]))
    curve = gs.CurvedVonMisesFisher(gs.SlerpCurve(np.eye(3)), 10.0)
    modes = gs.MixtureModel([v, B, gs.Uniform(), curve])._modes()
    assert len(modes) == 2
    assert np.array_equal(modes[0], v.mu) and np.allclose(np.abs(modes[1]), [0.0, 0.0, 1.0])
