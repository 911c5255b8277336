"""The host's rule for the lane kernels' Philox counter words (counter_words, geosss_amd/csrc/gsss_counter_words.h) without a
device: a host build of the header against the counter's definition -- chain = chain_offset + c, step = step_offset + s, words
(step low, chain low, chain high 16 | step high 16 << 16) -- at the boundaries of the 2^32 blocks; and the bound on the
kept rows that the kernels address in 32-bit factors."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "counter_words_host.cpp")
HDR = os.path.join(ROOT, "geosss_amd", "csrc", "gsss_counter_words.h")
OUT = os.path.join(ROOT, "tests", "_build", "libcounter_words_host.so")
B = 2**32


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    lib.t_counter_words.argtypes = [C.c_uint64, C.c_int64, C.c_uint64, C.c_int64, C.POINTER(C.c_uint32)]
    lib.t_kept_rows_fit32.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    return lib


def _words(lib, chain_offset, n_chains, step_offset, n_steps):
    w = (C.c_uint32 * 3)()
    ok = lib.t_counter_words(chain_offset, n_chains, step_offset, n_steps, w)
    return ok, tuple(w)


def _counter(chain, step):
    """(word 1, word 2, word 3) of a draw of (chain id, step id)"""
    return step % B, chain % B, ((chain >> 32) & 0xFFFF) | (((step >> 32) & 0xFFFF) << 16)


# chain_offset, n_chains, step_offset, n_steps, inside one block of either kind
CASES = [
    (0, 1, 0, 0, True),
    (0, 10**6, 0, 1000, True),                        # the bench's launch
    (0, B, 0, 1, True),                               # chains 0 .. 2^32 - 1
    (0, B + 1, 0, 1, False),                          # ... and chain 2^32
    (B - 200, 200, 0, 1, True),                       # the last chain is 2^32 - 1
    (B - 200, 201, 0, 1, False),
    (B - 200, 512, 3, 24, False),
    (B, 312, 3, 24, True),
    (5 * B + 7, 512, 3 * B, 12, True),                # non-zero high words
    (5 * B + 7, B - 7, 0, 1, True),
    (5 * B + 7, B - 6, 0, 1, False),
    (77, 512, B - 8, 7, True),                        # step ids up to 2^32 - 1 (the step count reaches n_steps)
    (77, 512, B - 8, 8, False),                       # ... a chain that has made its steps stands at 2^32
    (77, 512, B - 8, 16, False),
    (77, 512, B, 8, True),
    (77, 512, 0xFFFF * B + 5, 2**31 - 1, True),
    (2**48 - 512, 512, 0, 1, True),                   # the end of the 48-bit counter space
    (0, 0, 0, 5, False),                              # an empty launch draws nothing
]


@pytest.mark.parametrize("chain_offset,n_chains,step_offset,n_steps,inside", CASES)
def test_flag_and_words(lib, chain_offset, n_chains, step_offset, n_steps, inside):
    ok, (chain_lo, step_lo, c3) = _words(lib, chain_offset, n_chains, step_offset, n_steps)
    assert bool(ok) == inside
    # the flag's own definition: the high words of the first and the last id agree
    if n_chains >= 1:
        same = (chain_offset >> 32 == (chain_offset + n_chains - 1) >> 32) and (step_offset >> 32 == (step_offset + n_steps) >> 32)
        assert same == inside
    if ok:  # 32-bit sums give the counter of the launch's first and last chain at its first and last step count
        for c in (0, n_chains - 1):
            for s in (0, n_steps):
                assert ((step_lo + s) % B, (chain_lo + c) % B, c3) == _counter(chain_offset + c, step_offset + s)
                assert step_lo + s < B and chain_lo + c < B


def test_kept_rows_bound(lib):
    """keep_rows d (the chain-major row stride) and rows d of a launch stay below 2^31"""
    fit = lib.t_kept_rows_fit32
    assert fit(0, 1000, 100, 3) == 1 and fit(10, 1000, 100, 3) == 1
    assert fit((2**31 - 1) // 3, 10, 1, 3) == 1 and fit((2**31 - 1) // 3 + 1, 10, 1, 3) == 0
    assert fit(2**31 // 16 - 1, 10, 1, 16) == 1 and fit(2**31 // 16, 10, 1, 16) == 0
    assert fit(0, 2**31 - 1, 16, 16) == 1 and fit(0, 2**31 - 1, 15, 16) == 0
    assert fit(2**40, 10, 1, 3) == 0 and fit(2**62, 10, 1, 16) == 0


def test_host_build_pulls_in_no_hip():
    out = subprocess.run(["g++", "-std=c++17", "-M", SRC], check=True, capture_output=True, text=True).stdout
    assert "gsss_counter_words.h" in out and "hip_runtime" not in out and "/hip/" not in out, out
