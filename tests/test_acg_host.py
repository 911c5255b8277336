"""The angular central Gaussian target without a device: the longdouble restatement of tests/acg_cases.py against the
reference's recorded values, the margins of the reference chains the GPU tests replay, construction and refusals of
gs.AngularCentralGaussian and of the C ABI's kind 7, rand.sample_acg, the fast-mode kernel selection on a host build of
gsss_fast_select.h, and the register budget of the fast kernels against Bingham's all-double ones of the same build."""
import concurrent.futures as cf
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import acg_cases as ac
from conftest import ROOT, golden

SRC = os.path.join(ROOT, "tests", "cpp", "acg_select_host.cpp")
HDR = os.path.join(ROOT, "geosss_amd", "csrc", "gsss_fast_select.h")
OUT = os.path.join(ROOT, "tests", "_build", "libacg_select_host.so")
GSSS_OK, GSSS_E_INVALID, GSSS_E_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def gs():
    import geosss_amd
    return geosss_amd


# ------------------------------------------------------------------------------------------ the reference of the GPU tests
def test_longdouble_restatement_against_the_reference_values():
    """acg_cases.log_prob on Lambda = C^-1 against the reference's own ACG(C).log_prob (tests/golden/helpers_kat.npz, the
    fixture test_helpers.py reads): 1e-12 of the value's scale."""
    z = golden("helpers_kat.npz")
    L = np.linalg.inv(z["mvn_C"])
    got = ac.log_prob(0.5 * (L + L.T), z["mvn_Y"])
    want = z["acg_log_prob"]
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"longdouble ACG against the reference's recorded values: {float(err.max()):.1e}")
    assert len(want) >= 4 and float(err.max()) < 1e-12


def test_gradient_restatement_is_the_derivative_of_log_prob():
    """The longdouble gradient against central differences of the longdouble log_prob (step 1e-6 in longdouble: truncation
    ~1e-12 relative, rounding ~1e-13)."""
    L = ac.precision(7)
    X = ac.points(7)[:9] * 0.998
    _, g = ac.log_prob_and_gradient(L, X)
    h = np.longdouble(1e-6)
    Ll = L.astype(np.longdouble)

    def lp(P):
        q = np.sum((P @ Ll) * P, axis=1)
        return -(np.longdouble(7) / 2) * np.log(q)

    for j in range(7):
        e = np.zeros(7, dtype=np.longdouble)
        e[j] = h
        fd = (lp(X.astype(np.longdouble) + e) - lp(X.astype(np.longdouble) - e)) / (2 * h)
        assert float(np.max(np.abs(fd - g[:, j]))) < 1e-9 * float(np.max(np.abs(g)))


@pytest.mark.parametrize("sampler", ac.SAMPLERS)
@pytest.mark.parametrize("d", sorted(set(ac.CHAIN_DIMS + ac.FAST_DIMS)))
def test_chain_margins(d, sampler):
    """Every reference chain the GPU tests replay decides each try by more than MIN_MARGIN, and accepts within max_tries
    (slice_chain raises otherwise)."""
    ref = ac.reference_chain(d, sampler)
    print(f"d={d} {sampler}: margin {ref['margin']:.1e}, {ref['tries'].mean() / ac.N_STEPS:.1f} tries per step, "
          f"at most {int(ref['tries'].max())} per chain")
    assert ref["margin"] > ac.MIN_MARGIN
    assert ref["states"].shape == (ac.N_STEPS, ac.N_CHAINS, d) and np.all(np.isfinite(ref["states"]))
    assert np.all(ref["tries"] >= ac.N_STEPS) and int(ref["tries"].max()) < ac.N_STEPS * ac.MAX_TRIES
    assert np.max(np.abs(np.linalg.norm(ref["states"], axis=2) - 1.0)) < 1e-12


# ------------------------------------------------------------------------------------------ the Python class
def test_construction(gs):
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    lam = np.array([0.5, 2.0, 3.0, 8.0])
    L = (Q * lam) @ Q.T
    pdf = gs.AngularCentralGaussian(L)
    assert pdf.d == 4 and np.array_equal(pdf.precision, pdf.precision.T) and np.allclose(pdf.precision, L, rtol=0, atol=1e-14)
    assert abs(abs(pdf.mode @ Q[:, 0]) - 1.0) < 1e-12 and abs(np.linalg.norm(pdf.mode) - 1.0) < 1e-12
    assert abs(pdf.max_log_prob - (-2.0 * np.log(0.5))) < 1e-12
    # max_log_prob is the density at the mode
    assert abs(float(ac.log_prob(pdf.precision, pdf.mode)[0]) - pdf.max_log_prob) < 1e-12
    C = np.linalg.inv(L)
    again = gs.AngularCentralGaussian.from_covariance(C)
    assert np.allclose(again.precision, pdf.precision, rtol=1e-12, atol=1e-13)
    host = pdf.host()
    assert isinstance(host, gs.ACG) and not isinstance(pdf, gs.ACG)
    X = rng.standard_normal((6, 4))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    want = ac.log_prob(pdf.precision, X)
    assert float(np.max(np.abs(host.log_prob(X) - want))) < 1e-12
    kind, d, k, kappa, arrays = pdf._pack()[:5]
    assert (kind, d, k, kappa) == (7, 4, 0, 0.0) and gs._lib.ACG == 7
    assert arrays[0] is None and arrays[1] is None and arrays[3] is None and np.array_equal(arrays[2], pdf.precision)
    assert gs.AngularCentralGaussian.__name__ in gs.__all__ and "sample_acg" in gs.__all__


def test_constructor_refusals(gs):
    with pytest.raises(ValueError, match="symmetric"):
        gs.AngularCentralGaussian([[2.0, 0.5, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="positive definite"):
        gs.AngularCentralGaussian(np.diag([1.0, -1.0, 2.0]))
    with pytest.raises(ValueError, match="positive definite"):
        gs.AngularCentralGaussian(np.diag([1.0, 0.0, 2.0]))
    with pytest.raises(ValueError, match="positive definite"):
        gs.AngularCentralGaussian([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(ValueError, match="square"):
        gs.AngularCentralGaussian(np.ones((3, 4)))
    with pytest.raises(ValueError, match="finite"):
        gs.AngularCentralGaussian(np.diag([1.0, np.nan, 2.0]))
    with pytest.raises(ValueError):
        gs.AngularCentralGaussian.from_covariance(np.ones((2, 3)))


def test_mixture_and_batch_refuse_by_name(gs):
    pdf = gs.AngularCentralGaussian(np.diag([1.0, 2.0, 3.0]))
    with pytest.raises(TypeError, match="AngularCentralGaussian is not a mixture component"):
        gs.MixtureModel([gs.VonMisesFisher([3.0, 0.0, 0.0]), pdf])
    with pytest.raises(TypeError, match="AngularCentralGaussian is not built as a batch member"):
        gs.TargetBatch([pdf, pdf])
    with pytest.raises(TypeError, match="AngularCentralGaussian is not built as a batch member"):
        gs.TargetBatch([gs.Bingham(np.eye(3)), pdf])


def test_host_side_acg_still_refuses(gs):
    with pytest.raises(TypeError, match="host-side"):
        gs.ACG(np.eye(4))._pack()
    with pytest.raises(TypeError, match="host-side"):
        gs.AngularCentralGaussian(np.eye(4)).host()._pack()


def test_sample_acg(gs):
    pdf = gs.AngularCentralGaussian(ac.precision(5))
    a = gs.rand.sample_acg(pdf, 1000, seed=3)
    assert a.shape == (1000, 5) and np.max(np.abs(np.linalg.norm(a, axis=1) - 1.0)) < 1e-14
    assert np.array_equal(a, gs.sample_acg(pdf, 1000, seed=3)) and not np.array_equal(a, gs.sample_acg(pdf, 1000, seed=4))
    assert np.allclose(a, gs.sample_acg(pdf.host(), 1000, seed=3), rtol=0, atol=1e-12)  # (the overlay's C^-1 is Lambda to rounding)
    with pytest.raises(TypeError):
        gs.sample_acg(gs.Bingham(np.eye(3)), 10)
    # the law: E[x x^T] of x = y / |y|, y ~ N(0, diag(4, 1, 1 / 4)), has the eigenvalues' order and trace one
    diag = gs.AngularCentralGaussian(np.diag([0.25, 1.0, 4.0]))
    x = gs.sample_acg(diag, 200_000, seed=1)
    m = (x[:, :, None] * x[:, None, :]).mean(0)
    assert abs(np.trace(m) - 1.0) < 1e-12 and m[0, 0] > m[1, 1] + 0.05 and m[1, 1] > m[2, 2] + 0.05
    assert np.max(np.abs(m - np.diag(np.diag(m)))) < 5.0 / np.sqrt(200_000)


# ------------------------------------------------------------------------------------------ the C ABI, before any device
def _desc(gs, L, kind=7):
    L = np.ascontiguousarray(L, dtype=np.float64)
    return gs._lib.TargetDesc(kind, len(L), 0, 0, None, None, L.ctypes.data_as(C.c_void_p), None, 0.0), L


def test_pack_target_refusals(gs):
    """gsss_target_create checks Lambda before it touches a device: the refusals need none."""
    lib = gs._lib.load()
    assert lib.gsss_abi_version() == 10
    h = C.c_void_p()
    cases = [(np.array([[2.0, 0.5, 0.0], [0.25, 2.0, 0.0], [0.0, 0.0, 1.0]]), "not symmetric"),
             (np.diag([1.0, -1.0, 2.0]), "not positive definite"),
             (np.diag([1.0, 0.0, 2.0]), "not positive definite"),
             (np.array([[1.0, 2.0], [2.0, 1.0]]), "not positive definite"),
             (np.diag([1.0, np.inf, 2.0]), "not positive definite"),
             (np.diag([1.0, np.nan, 2.0]), "not positive definite")]
    for L, msg in cases:
        desc, keep = _desc(gs, L)
        assert lib.gsss_target_create(C.byref(desc), 0, C.byref(h)) == GSSS_E_INVALID, L
        assert msg in lib.gsss_last_error().decode() and not h.value, lib.gsss_last_error()
    desc = gs._lib.TargetDesc(7, 3, 0, 0, None, None, None, None, 0.0)
    assert lib.gsss_target_create(C.byref(desc), 0, C.byref(h)) == GSSS_E_INVALID
    assert "needs A" in lib.gsss_last_error().decode()
    # a good Lambda passes the checks; what comes back then depends on the device alone
    desc, keep = _desc(gs, ac.precision(6))
    rc = lib.gsss_target_create(C.byref(desc), 0, C.byref(h))
    assert rc != GSSS_E_INVALID and rc != GSSS_E_UNSUPPORTED, lib.gsss_last_error()
    if rc == GSSS_OK:
        lib.gsss_target_destroy(h)


def test_mixture_batch_and_plan_refuse_kind_7(gs):
    lib = gs._lib.load()
    h = C.c_void_p()
    desc, keep = _desc(gs, np.diag([1.0, 2.0, 3.0]))
    descs = (gs._lib.TargetDesc * 2)(desc, desc)
    logw = np.log(np.array([0.5, 0.5]))
    assert lib.gsss_target_create_mixture(descs, 2, logw.ctypes.data_as(C.c_void_p), 0, C.byref(h)) < 0
    assert "kind 7" in lib.gsss_last_error().decode()
    assert lib.gsss_target_create_batch(descs, 2, 4, 0, C.byref(h)) < 0
    assert "kind 7" in lib.gsss_last_error().decode()
    assert lib.gsss_batch_plan(7, 3, 0, 0, 4, 64, None, None, None, None) == GSSS_E_UNSUPPORTED
    assert "kind 7" in lib.gsss_last_error().decode()


# ------------------------------------------------------------------------------------------ kernel selection on the host
@pytest.fixture(scope="module")
def select():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    lib.t_acg_select.argtypes = [C.c_int] * 9 + [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def run(kind, d, k=0, screen=1, spread=0, numpy=0, replay=0, stats=0, batch=0):
        buf, lane, family = C.create_string_buffer(200), C.c_int(0), C.c_int(0)
        rc = lib.t_acg_select(kind, d, k, screen, spread, numpy, replay, stats, batch, buf, len(buf), C.byref(lane), C.byref(family))
        return rc, buf.value.decode(), bool(lane.value)

    return run


def test_selection(select):
    """Kind 7 at d = 3 .. 10: the all-double lane kernel of FastAcg<D> wherever Bingham's all-double pick (screen = 0) serves
    -- fast_kernel on every stream, its one-wavefront form for a spread ensemble on a generated stream -- whatever `screen` and
    the diagonal flag say; nothing at d = 2, d = 11 and beyond, and no batch."""
    n = 0
    for d in range(3, 11):
        for spread in (0, 1):
            for numpy in (0, 1):
                for replay in (0, 1):
                    for stats in (0, 1):
                        rc_b, name_b, lane_b = select(2, d, screen=0, spread=spread, numpy=numpy, replay=replay, stats=stats)
                        assert rc_b == GSSS_OK and lane_b and f"FastBingham<{d}>" in name_b
                        for screen in (0, 1, 2):
                            for k in (0, 1):
                                rc, name, lane = select(7, d, k=k, screen=screen, spread=spread, numpy=numpy, replay=replay, stats=stats)
                                assert rc == GSSS_OK and lane
                                assert name == name_b.replace("FastBingham", "FastAcg"), (d, spread, numpy, replay, name, name_b)
                                n += 1
                        if not spread or replay:
                            assert name_b == f"fast_kernel<{d}, FastBingham<{d}>>"
        assert select(7, d)[1] == f"fast_kernel<{d}, FastAcg<{d}>>"
        assert select(7, d, spread=1)[1] == f"wave_kernel<{d}, FastAcg<{d}>>"
        assert select(7, d, batch=1)[0] == GSSS_E_UNSUPPORTED
    assert n == 8 * 16 * 6
    for d in (2, 11, 12, 16, 17, 64, 300):
        for spread in (0, 1):
            for screen in (0, 1):
                rc, name, lane = select(7, d, screen=screen, spread=spread)
                assert rc == GSSS_E_UNSUPPORTED and name == "" and not lane, (d, name)


def test_selection_header_needs_no_hip():
    out = subprocess.run(["g++", "-std=c++17", "-M", SRC], check=True, capture_output=True, text=True).stdout
    assert "gsss_fast_select.h" in out and "hip_runtime" not in out and "/hip/" not in out, out


# ------------------------------------------------------------------------------------------ the threshold's exponential
def test_exp_fast_k_equals_exp_fast():
    """fm::exp_fast_k (the constants in scalar registers on the device) is exp_fast operation for operation: the same bits on a
    host build of gsss_math.h over [-800, 800] and beyond the clamp, at the points where n = round(x / ln 2) changes, at +-0,
    +-inf and NaN -- a later edit of one copy alone fails here."""
    src = os.path.join(ROOT, "tests", "cpp", "acg_math_host.cpp")
    hdr = os.path.join(ROOT, "geosss_amd", "csrc", "gsss_math.h")
    out = os.path.join(ROOT, "tests", "_build", "libacg_math_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", out, src])
    lib = C.CDLL(out)
    rng = np.random.default_rng(7)
    half = (np.arange(-1200, 1200) + 0.5) * np.log(2.0)
    x = np.concatenate([rng.uniform(-800.0, 800.0, 400_000), rng.uniform(0.0, 15.0, 200_000), np.linspace(-900.0, 900.0, 100_001),
                        half, np.nextafter(half, np.inf), np.nextafter(half, -np.inf),
                        np.array([0.0, -0.0, 1e-300, -1e-300, 709.78, 709.79, -745.2, 800.0, -800.0, 1e6, -1e6, np.inf, -np.inf, np.nan])])
    a, b = np.empty_like(x), np.empty_like(x)
    lib.t_exp_pair(x.ctypes.data_as(C.c_void_p), C.c_long(len(x)), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    fin = np.isfinite(x) & (np.abs(x) < 700)
    assert np.max(np.abs(b[fin] / np.exp(x[fin]) - 1.0)) < 1e-15 and np.isnan(b[-1]) and b[-3] == np.inf and b[-2] == 0.0


# ------------------------------------------------------------------------------------------ register budget
def _demangled(usage):
    names = subprocess.run(["c++filt"], input="\n".join(usage), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.replace("void gsss::", "").split("(")[0]: v for n, v in zip(names, usage.values())}


def test_register_budget():
    """Every build of the ACG fast kernels (fast_kernel on the Philox, replayed and numpy streams, with and without running
    statistics; its one-wavefront form wave_kernel) needs no scratch and holds at least as many wavefronts per SIMD as the same
    build of Bingham's all-double kernel of the same D, compiled with the same flags."""
    from geosss_amd import build
    with cf.ThreadPoolExecutor(2) as ex:
        acg, bing = [_demangled(u) for u in ex.map(build.resource_usage, ["gsss_fast_acg.hip", "gsss_fast_bingham.hip"])]
    assert len(acg) == 8 * (5 + 4) and all("FastAcg<" in k for k in acg), sorted(acg)
    bad = []
    for name, u in sorted(acg.items()):
        twin = bing[name.replace("FastAcg", "FastBingham")]
        print(f"{name}: {u['vgprs']} VGPRs, {u['scratch']} B scratch, {u['occupancy']} waves/SIMD (Bingham: {twin['vgprs']}, {twin['occupancy']})")
        if u["scratch"] != 0 or u["occupancy"] < twin["occupancy"]:
            bad.append((name, u, twin))
    assert not bad, bad
