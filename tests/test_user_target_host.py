"""CPU checks of user-defined targets (DeviceDistribution): code generation, the module cache, a real hipcc compile of a module for
gfx950, compiler diagnostics, and the C ABI's refusals of a module that does not match the library."""
import ctypes as C
import os

import numpy as np
import pytest

from user_sources import ACG, ACG_NO_GRADIENT, BINGHAM


def test_cache_key_follows_source_layout_and_digest():
    from geosss_amd import usertarget as ut
    base = dict(lib_path="/x/libgsss_hip.so", hipcc="hipcc 1", flags=["-O3"])
    k = ut.cache_key(ACG, 4, "d" * 64, **base)
    assert k == ut.cache_key(ACG, 4, "d" * 64, **base)
    assert k != ut.cache_key(ACG + " ", 4, "d" * 64, **base)
    assert k != ut.cache_key(ACG, 5, "d" * 64, **base)
    assert k != ut.cache_key(ACG, 4, "e" * 64, **base)
    assert k != ut.cache_key(ACG, 4, "d" * 64, **dict(base, hipcc="hipcc 2"))
    assert k != ut.cache_key(ACG, 4, "d" * 64, **dict(base, flags=["-O2"]))


def test_layout_of_d():
    """The module is built per layout, not per d: dimensions that share a layout share a module."""
    from geosss_amd import _lib, usertarget as ut
    lib = _lib.load()
    assert lib.gsss_exact_layout(3) == 2 and lib.gsss_exact_layout(10) == 7           # lane3, lane10
    assert lib.gsss_exact_layout(11) == lib.gsss_exact_layout(16) == 8                 # coop4x4
    assert lib.gsss_exact_layout(50) == 10                                             # coop16x4
    assert lib.gsss_exact_layout(1) < 0 and lib.gsss_exact_layout(100000) < 0
    kw = dict(lib_path="/x", hipcc="h")
    digest = "0" * 64
    assert ut.cache_key(ACG, lib.gsss_exact_layout(11), digest, **kw) == ut.cache_key(ACG, lib.gsss_exact_layout(16), digest, **kw)
    assert ut.cache_key(ACG, lib.gsss_exact_layout(5), digest, **kw) != ut.cache_key(ACG, lib.gsss_exact_layout(6), digest, **kw)


def test_gradient_detection_and_generated_header():
    from geosss_amd import usertarget as ut
    assert ut.has_gradient(ACG) and ut.has_gradient(BINGHAM)
    assert not ut.has_gradient(ACG_NO_GRADIENT)
    assert not ut.has_gradient(ACG_NO_GRADIENT + "\n// gsss_user_gradient(x) is not given\n")
    h = ut.generated_header(ACG)
    assert ACG in h and '#line 1 "user_source"' in h


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    import time
    import geosss_amd as gs
    from geosss_amd import usertarget as ut
    cache = str(tmp_path_factory.mktemp("gsss_user_cache"))
    t0 = time.perf_counter()
    pdf = gs.DeviceDistribution(5, ACG, np.eye(5), cache_dir=cache)
    print(f"one user module (layout {pdf.module.vec_id}, with gradient) compiled in {time.perf_counter() - t0:.1f} s")
    return gs, ut, cache, pdf


def test_module_compiles_for_gfx950_and_exports_its_table(compiled):
    gs, ut, cache, pdf = compiled
    assert pdf.module.compiled and os.path.dirname(pdf.module.path) == cache
    assert os.path.basename(pdf.module.path).startswith("user_") and pdf.module.path.endswith(".so")
    assert [f for f in os.listdir(cache) if f.startswith("build_")] == []                 # the build folder is gone
    assert hasattr(C.CDLL(pdf.module.path), ut.ENTRY) and pdf.module.table
    with open(pdf.module.path, "rb") as f:
        assert b"amdgcn-amd-amdhsa--gfx950" in f.read()                                   # device code for gfx950
    assert pdf.d == 5 and pdf.has_gradient and pdf.params.shape == (5, 5)


def test_second_construction_reuses_the_cached_module(compiled):
    gs, ut, cache, pdf = compiled
    mtime = os.path.getmtime(pdf.module.path)
    again = gs.DeviceDistribution(5, ACG, 2 * np.eye(5), cache_dir=cache)                 # other parameters: same module
    assert not again.module.compiled and again.module.path == pdf.module.path
    ut._modules.clear()                                                                   # as a fresh process would find it
    fresh = gs.DeviceDistribution(5, ACG, np.eye(5), cache_dir=cache)
    assert not fresh.module.compiled and fresh.module.path == pdf.module.path
    assert os.path.getmtime(pdf.module.path) == mtime


def test_cache_dir_from_environment(monkeypatch, tmp_path):
    from geosss_amd import usertarget as ut
    monkeypatch.setenv("GEOSSS_AMD_CACHE", str(tmp_path))
    assert ut.default_cache_dir() == str(tmp_path)
    monkeypatch.delenv("GEOSSS_AMD_CACHE")
    assert ut.default_cache_dir() == os.path.join(os.path.expanduser("~"), ".cache", "geosss_amd")


def test_compiler_error_is_a_value_error_with_hipccs_message(tmp_path):
    import geosss_amd as gs
    bad = "__device__ double gsss_user_log_prob(const double *x, int d, const double *p) {\n    return x[0] +;\n}\n"
    with pytest.raises(ValueError, match=r"(?s)hipcc rejected.*user_source:2:.*error"):
        gs.DeviceDistribution(3, bad, cache_dir=str(tmp_path))
    assert [f for f in os.listdir(tmp_path) if f.endswith(".so") or f.startswith("build_")] == []
    with pytest.raises(ValueError, match="must define"):
        gs.DeviceDistribution(3, "__device__ double f(double x) { return x; }", cache_dir=str(tmp_path))


def test_mixture_of_a_device_distribution_is_refused(compiled):
    gs, ut, cache, pdf = compiled
    with pytest.raises(TypeError, match="DeviceDistribution is not a mixture component"):
        gs.MixtureModel([pdf, gs.VonMisesFisher(np.array([0, 0, 0, 0, 10.0]))])


def test_gradient_and_hmc_need_the_gradient_source(tmp_path):
    import geosss_amd as gs
    pdf = gs.DeviceDistribution(5, ACG_NO_GRADIENT, np.eye(5), cache_dir=str(tmp_path))
    assert not pdf.has_gradient
    with pytest.raises(ValueError, match="no gsss_user_gradient"):
        pdf.gradient(np.eye(5)[0])
    with pytest.raises(ValueError, match="no gsss_user_gradient"):
        gs.SphericalHMC(pdf, np.eye(5)[0], 1)


class _FakeTable(C.Structure):  # gsss::UserModuleTable (gsss_user_target.h)
    _fields_ = [("module_abi", C.c_int32), ("gsss_abi", C.c_int32), ("vec_id", C.c_int32), ("has_gradient", C.c_int32),
                ("digest", C.c_char_p), ("run", C.c_void_p), ("logprob", C.c_void_p), ("mh", C.c_void_p)]


def test_library_refuses_a_module_that_does_not_match(compiled):
    """gsss_target_create_user checks the module's ABI, kernel-source digest and layout before anything else (no device needed)."""
    gs, ut, cache, pdf = compiled
    lib = gs._lib.load()
    h = C.c_void_p()
    p = np.eye(6).ravel()
    rc = lib.gsss_target_create_user(C.c_void_p(pdf.module.table), 6, p.ctypes.data_as(C.c_void_p), p.size, 0, C.byref(h))
    assert rc == -2 and b"layout" in lib.gsss_last_error()                                # a d = 5 module, d = 6 asked for
    digest = lib.gsss_source_digest()
    for fields, what in (((2, 10, 4, 1, digest), b"ABI"), ((1, 9, 4, 1, digest), b"ABI"), ((1, 10, 4, 1, b"0" * 64), b"kernel sources")):
        t = _FakeTable(*fields)
        rc = lib.gsss_target_create_user(C.byref(t), 5, p.ctypes.data_as(C.c_void_p), 25, 0, C.byref(h))
        assert rc == -2 and what in lib.gsss_last_error(), lib.gsss_last_error()
    assert lib.gsss_target_create_user(None, 5, None, 0, 0, C.byref(h)) == -1


def test_builtin_refusals_are_unchanged():
    import geosss_amd as gs
    with pytest.raises(TypeError):
        gs.ACG(np.eye(4))._pack()

    class Mine(gs.Distribution):
        d = 3

    with pytest.raises(TypeError, match="no device parameter block"):
        Mine()._pack()
