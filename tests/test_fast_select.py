"""Which kernel a GSSS_MODE_FAST launch runs (geosss_amd/csrc/gsss_fast_select.h) against the record of the library that chose
by probing its launchers (tests/golden/fast_kernel_names.json, written by tools/record_fast_kernel_names.py from the commit the
file names).  The CPU test replays every recorded row on a host build of the header -- no library, no device; the GPU test walks
the same grid through the C ABI of the library under test."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_fast_kernel_names as rec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fast_kernel_names.json")
SRC = os.path.join(ROOT, "tests", "cpp", "fast_select_host.cpp")
HDR = os.path.join(ROOT, "geosss_amd", "csrc", "gsss_fast_select.h")
OUT = os.path.join(ROOT, "tests", "_build", "libfast_select_host.so")


@pytest.fixture(scope="module")
def select():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    lib.t_fast_select.argtypes = [C.c_int] * 4 + [C.c_double] + [C.c_int] * 8 + [C.c_char_p, C.c_int, C.POINTER(C.c_int)]

    def run(row, screen, spread):
        buf, lane = C.create_string_buffer(200), C.c_int(0)
        rc = lib.t_fast_select(row["kind"], row["d"], row["k"], row["mix_curve"], row["scale"], screen, spread, 0, 0, 0,
                               row["batch"], row["curve_tail"], row["curve_l2"], buf, len(buf), C.byref(lane))
        return rc, buf.value.decode(), bool(lane.value)

    return run


def test_header_needs_no_hip():
    """The selection compiles with the host compiler alone: no HIP header, directly or through an include."""
    out = subprocess.run(["g++", "-std=c++17", "-M", SRC], check=True, capture_output=True, text=True).stdout
    assert "gsss_fast_select.h" in out and "hip_runtime" not in out and "/hip/" not in out, out


def test_select_equals_the_record(select):
    record = rec.load_record(GOLDEN)
    rows = record["rows"]
    assert len(rows) > 2000 and record["variants"] == [0, 100, 101] and record["placements"] == [0, 1, 2]
    bad = []
    for row in rows:
        # gsss_mode_supported / gsss_variant_name: all-double, packed (a batch: screened -- every batch shape has both)
        rc, _, lane = select(row, 1 if row["batch"] else 0, 0)
        got = {"supported": rc == 0, "variant_name": ("fast-lane" if lane else "fast-coop") if rc == 0 else "", "names": []}
        for variant in record["variants"]:
            screen = {0: 1, 100: 0, 101: 2}[variant]
            got["names"].append([select(row, screen, 1 if placement == 2 else 0)[1] for placement in record["placements"]])
        want = {key: row[key] for key in got}
        if got != want:
            bad.append((row, got))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; first: {bad[0]}"


@pytest.mark.gpu
def test_library_equals_the_record():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_fast_kernel_names.py"), "--check", GOLDEN],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
