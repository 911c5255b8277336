"""The host side of exact mode through the C ABI: the table of built-in families names the kernel a handle runs (gsss_kernel_name),
GSSS_MIXTURE takes the common run and MH launch path with LDS offsets that do not depend on how a launch is cut, and a launch
whose parameters do not fit a workgroup's LDS in a forced layout is refused by one rule, before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from user_sources import ACG_NO_GRADIENT

pytestmark = pytest.mark.gpu

OK, E_UNSUPPORTED = 0, -2
LANE3 = 2  # the id of "lane3" among the vector layouts (gsss_run_args.variant)
K_BIG = 9000  # on S^2 in lane3: 9000 (3 + 1) 8 = 288 000 B of rows, a workgroup's LDS is 163 840 B


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


@pytest.fixture(scope="module")
def lib(gs):
    return gs._lib.load()


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


class Handles:
    """Targets created through the C ABI; the parameter arrays stay alive until the handles are destroyed."""

    def __init__(self, gs, lib):
        self.L, self.lib, self.keep, self.handles = gs._lib, lib, [], []

    def vmf_desc(self, d, k, kappa=4.0, seed=0):
        mu, logc = kappa * unit_rows(k, d, seed), np.full(k, -np.log(k))
        self.keep += [mu, logc]
        return self.L.TargetDesc(kind=self.L.VMF_MIXTURE, d=d, k=k, mu=mu.ctypes.data, logc=logc.ctypes.data)

    def create(self, desc):
        out = C.c_void_p()
        assert self.lib.gsss_target_create(C.byref(desc), 0, C.byref(out)) == OK, self.lib.gsss_last_error()
        self.handles.append(out)
        return out

    def matrix(self, kind, d):
        A = np.diag(np.arange(1.0, d + 1.0)) + 0.25  # symmetric, positive definite, not diagonal
        self.keep.append(A)
        return self.create(self.L.TargetDesc(kind=kind, d=d, A=A.ctypes.data))

    def curve(self, d, k):
        knots = unit_rows(k, d, 5)
        self.keep.append(knots)
        return self.create(self.L.TargetDesc(kind=self.L.CURVE_VMF, d=d, k=k, knots=knots.ctypes.data, kappa=50.0))

    def mixture(self, descs):
        arr = (self.L.TargetDesc * len(descs))(*descs)
        logw = np.log(np.full(len(descs), 1.0 / len(descs)))
        out = C.c_void_p()
        assert self.lib.gsss_target_create_mixture(arr, len(descs), logw.ctypes.data, 0, C.byref(out)) == OK, self.lib.gsss_last_error()
        self.handles.append(out)
        return out

    def close(self):
        for h in self.handles:
            self.lib.gsss_target_destroy(h)


@pytest.fixture()
def make(gs, lib):
    h = Handles(gs, lib)
    yield h
    import torch
    torch.cuda.synchronize()
    h.close()


def run(gs, lib, handle, state, sampler, n_steps, step_offset=0, variant=0, stepsize=None, n_accept=None):
    a = gs._lib.RunArgs(state_dev=state.data_ptr(), n_chains=state.shape[1], n_steps=n_steps, thin=1, seed=11, step_offset=step_offset,
                        sampler=sampler, mode=gs._lib.MODE_EXACT, max_tries=1000, variant=variant)
    if stepsize is not None:
        a.stepsize_dev, a.n_accept_dev = stepsize.data_ptr(), n_accept.data_ptr()
    rc = lib.gsss_run(handle, C.byref(a), None)
    err = lib.gsss_last_error().decode()
    assert lib.gsss_stream_synchronize(0, None) == OK
    return rc, err


def start(d, n):
    import torch
    return torch.from_numpy(np.ascontiguousarray(unit_rows(n, d, 3).T)).cuda()


def test_kernel_names_through_the_family_table(gs, lib, make, tmp_path):
    L = gs._lib
    user = gs.DeviceDistribution(3, ACG_NO_GRADIENT, np.eye(3), cache_dir=str(tmp_path))
    cases = [(make.create(make.vmf_desc(3, 2)), "run_kernel<lane3, VmfMixture>"),
             (make.matrix(L.BINGHAM, 5), "run_kernel<lane5, Bingham>"),
             (make.matrix(L.ACG, 4), "run_kernel<lane4, Acg>"),
             (make.curve(6, 3), "run_kernel<lane6, CurveVmf>"),
             (make.mixture([make.vmf_desc(7, 1, seed=1), make.vmf_desc(7, 1, seed=2)]), "run_kernel<coop4x4, Mixture>"),
             (user._device_target(0).handle, "run_kernel<lane3, UserTarget>")]
    for handle, name in cases:
        assert lib.gsss_kernel_name(handle, L.MODE_EXACT, 0, 0).decode() == name


@pytest.mark.parametrize("sampler", ["SHRINK", "RWMH"])
def test_mixture_launch_equals_the_same_launch_cut_in_two(gs, lib, make, sampler):
    """8 chains x 2 steps of a two-term GSSS_MIXTURE at d = 7 (coop4x4: slots, scratch rows, the draws' reserve, then the rows)
    against one step twice, bit for bit."""
    import torch
    handle = make.mixture([make.vmf_desc(7, 1, seed=1), make.vmf_desc(7, 1, seed=2)])
    code = getattr(gs._lib, sampler)
    got = []
    for cuts in ((2,), (1, 1)):
        state = start(7, 8)
        mh = dict(stepsize=torch.full((8,), 0.5, dtype=torch.float64, device="cuda"),
                  n_accept=torch.zeros(8, dtype=torch.int64, device="cuda")) if sampler == "RWMH" else {}
        done = 0
        for n in cuts:
            rc, err = run(gs, lib, handle, state, code, n, step_offset=done, **mh)
            assert rc == OK, err
            done += n
        got.append([state.cpu()] + [t.cpu() for t in mh.values()])
    assert not torch.equal(got[0][0], start(7, 8).cpu())
    for whole, cut in zip(*got):
        assert torch.equal(whole, cut)


@pytest.mark.parametrize("kind", ["vmf", "mixture"])
def test_rows_beyond_the_lds_are_refused_in_a_forced_layout(gs, lib, make, kind):
    """K = 9000 on S^2 (and a GSSS_MIXTURE of two such components): refused in lane3 by the one LDS rule, the state untouched;
    with no layout forced the same handle runs in coop64x4, its rows read from global memory."""
    import torch
    L = gs._lib
    if kind == "vmf":
        handle = make.create(make.vmf_desc(3, K_BIG))
    else:
        handle = make.mixture([make.vmf_desc(3, K_BIG, seed=1), make.vmf_desc(3, K_BIG, seed=2)])
    assert lib.gsss_variant_name(handle, L.MODE_EXACT, 0) == b"coop64x4"
    for sampler in (L.SHRINK, L.RWMH):
        state = start(3, 4)
        before = state.clone()
        mh = dict(stepsize=torch.full((4,), 0.5, dtype=torch.float64, device="cuda"),
                  n_accept=torch.zeros(4, dtype=torch.int64, device="cuda")) if sampler == L.RWMH else {}
        rc, err = run(gs, lib, handle, state, sampler, 1, variant=LANE3, **mh)
        assert rc == E_UNSUPPORTED
        assert "B of LDS" in err
        assert torch.equal(state, before)
        rc, err = run(gs, lib, handle, state, sampler, 1, variant=0, **mh)
        assert rc == OK, err
        assert torch.isfinite(state).all()
