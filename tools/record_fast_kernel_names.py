#!/usr/bin/env python3
"""Which kernel does a GSSS_MODE_FAST launch run, shape by shape?  Walks a grid of targets through the C ABI only
(gsss_mode_supported, gsss_variant_name, gsss_kernel_name for variant {0, 100, 101} x placement {0, 1, 2}) and writes, or checks,
tests/golden/fast_kernel_names.json:

    GSSS_HIP_LIB=<library of the commit to record> python tools/record_fast_kernel_names.py --out tests/golden/fast_kernel_names.json
    python tools/record_fast_kernel_names.py --check tests/golden/fast_kernel_names.json

The grid straddles every boundary of the selection (geosss_amd/csrc/gsss_fast_select.h).  GSSS_CURVE_TAIL is walked unset and
=0; GSSS_CURVE_L2=1 is read once per process, so its rows come from a child process.  Every row holds the inputs of the
selection beside the answers (tests/test_fast_select.py replays them on a host build of the header, without the library).
Needs a device: creating a target uploads its parameters."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from geosss_amd import _lib  # noqa: E402

VARIANTS = (0, _lib.VARIANT_FAST_DOUBLE, _lib.VARIANT_FAST_VERIFY)
PLACEMENTS = (0, 1, 2)

VMF_D = list(range(3, 18)) + [32, 33, 64, 65, 128, 129, 256, 257]
VMF_K = [1, 3, 4, 5, 6, 10, 11, 16, 17]
VMF_SCALE = [80.0, 4000.0, 4001.0]
BINGHAM_D = list(range(3, 18)) + [32, 33, 64, 65, 126, 127, 128, 129]
BINGHAM_FORMS = ["diagonal", "dense", "diagonal+b"]
CURVE_D = list(range(3, 26)) + [32, 33, 36, 37, 40, 41, 48, 49, 52, 53, 56, 57, 64, 65, 96, 97, 104, 105, 112, 113, 128, 129, 192,
                                193, 208, 209, 256, 257, 512, 513]
CURVE_KNOTS = [2, 10, 11, 16, 17, 18]
MIX_D = [3, 16, 17]
MIX_TERMS = [2, 8, 9]
BATCH_D = list(range(3, 18))


def _ptr(a):
    return a.ctypes.data


class Shape:
    """One target of the grid: its descriptors (kept alive with their arrays) and the inputs of the selection."""

    def __init__(self, kind, d, k, scale=0.0, batch=False, mix_curve=False, note=""):
        self.ask = {"kind": kind, "d": d, "k": k, "scale": scale, "batch": batch, "mix_curve": mix_curve, "note": note}
        self.descs, self.keep, self.log_w = [], [], None


def vmf_desc(shape, d, k, scale):
    mu = np.zeros((k, d))
    mu[:, 0] = 1.0
    mu[0, 0] = scale  # max |mu| is exactly `scale`
    logc = np.zeros(k)
    shape.keep += [mu, logc]
    return _lib.TargetDesc(kind=_lib.VMF_MIXTURE, d=d, k=k, mu=_ptr(mu), logc=_ptr(logc))


def bingham_desc(shape, d, form):
    A = np.diag(np.arange(1.0, d + 1.0))
    if form == "dense":
        A[0, 1] = A[1, 0] = 0.5
    shape.keep.append(A)
    desc = _lib.TargetDesc(kind=_lib.BINGHAM, d=d, k=0, A=_ptr(A))
    if form == "diagonal+b":
        b = np.ones(d)
        shape.keep.append(b)
        desc.mu = _ptr(b)
    return desc


BINGHAM_FLAGS = {"diagonal": 1, "dense": 0, "diagonal+b": 3}


def curve_desc(shape, d, knots):
    t = np.linspace(0.0, 1.0, knots)
    pts = np.zeros((knots, d))
    pts[:, 0], pts[:, 1] = np.cos(t), np.sin(t)
    shape.keep.append(pts)
    return _lib.TargetDesc(kind=_lib.CURVE_VMF, d=d, k=knots, knots=_ptr(pts), kappa=300.0)


def grid(l2_only=False):
    shapes = []
    for d in CURVE_D:
        for knots in CURVE_KNOTS:
            s = Shape(_lib.CURVE_VMF, d, knots)
            s.descs = [curve_desc(s, d, knots)]
            shapes.append(s)
    if l2_only:  # the switch only moves curves
        return shapes
    for d in VMF_D:
        for k in VMF_K:
            for scale in VMF_SCALE:
                s = Shape(_lib.VMF_MIXTURE, d, k, scale)
                s.descs = [vmf_desc(s, d, k, scale)]
                shapes.append(s)
    for d in BINGHAM_D:
        for form in BINGHAM_FORMS:
            s = Shape(_lib.BINGHAM, d, BINGHAM_FLAGS[form], note=form)
            s.descs = [bingham_desc(s, d, form)]
            shapes.append(s)
    for d in MIX_D:  # a vMF mixture of terms - 1 components and a Bingham term
        for terms in MIX_TERMS:
            s = Shape(_lib.MIXTURE, d, terms, scale=80.0)
            s.descs = [vmf_desc(s, d, terms - 1, 80.0), bingham_desc(s, d, "dense")]
            s.log_w = np.log(np.array([0.5, 0.5]))
            shapes.append(s)
    s = Shape(_lib.MIXTURE, 3, 2, scale=80.0, mix_curve=True, note="a curve component")
    s.descs = [vmf_desc(s, 3, 1, 80.0), curve_desc(s, 3, 10)]
    s.log_w = np.log(np.array([0.5, 0.5]))
    shapes.append(s)
    for d in BATCH_D:  # batches of two members
        for k in VMF_K:
            for scale in VMF_SCALE:
                s = Shape(_lib.VMF_MIXTURE, d, k, scale, batch=True)
                s.descs = [vmf_desc(s, d, k, 1.0), vmf_desc(s, d, k, scale)]
                shapes.append(s)
        for form in BINGHAM_FORMS:
            s = Shape(_lib.BINGHAM, d, BINGHAM_FLAGS[form], batch=True, note=form)
            s.descs = [bingham_desc(s, d, form), bingham_desc(s, d, form)]
            shapes.append(s)
        s = Shape(_lib.BINGHAM, d, 0, batch=True, note="one dense member")
        s.descs = [bingham_desc(s, d, "diagonal"), bingham_desc(s, d, "dense")]
        shapes.append(s)
    return shapes


def create(lib, shape):
    """The target's handle, or None where the library refuses to create it (recorded as unsupported)."""
    h = C.c_void_p()
    arr = (_lib.TargetDesc * len(shape.descs))(*shape.descs)
    if shape.ask["batch"]:
        rc = lib.gsss_target_create_batch(arr, len(shape.descs), 256, 0, C.byref(h))
    elif shape.ask["kind"] == _lib.MIXTURE:
        rc = lib.gsss_target_create_mixture(arr, len(shape.descs), _ptr(shape.log_w), 0, C.byref(h))
    else:
        rc = lib.gsss_target_create(C.byref(arr[0]), 0, C.byref(h))
    return h if rc == 0 else None


def walk(lib, curve_tail, curve_l2):
    """Rows of the grid under one setting of the environment switches (curve_tail: None = unset)."""
    if curve_tail is None:
        os.environ.pop("GSSS_CURVE_TAIL", None)
    else:
        os.environ["GSSS_CURVE_TAIL"] = str(curve_tail)
    rows = []
    for shape in grid(l2_only=curve_l2):
        if curve_tail is not None and shape.ask["kind"] != _lib.CURVE_VMF:
            continue  # the switch only moves curves
        row = dict(shape.ask, curve_tail=1 if curve_tail is None else curve_tail, curve_l2=curve_l2)
        h = create(lib, shape)
        row["created"] = h is not None
        if h is None:
            row.update(supported=False, variant_name="", names=[[""] * len(PLACEMENTS)] * len(VARIANTS))
        else:
            row["supported"] = bool(lib.gsss_mode_supported(h, _lib.MODE_FAST))
            vn = {lib.gsss_variant_name(h, _lib.MODE_FAST, v).decode() for v in VARIANTS}
            assert len(vn) == 1, vn
            row["variant_name"] = vn.pop()
            row["names"] = [[lib.gsss_kernel_name(h, _lib.MODE_FAST, v, p).decode() for p in PLACEMENTS] for v in VARIANTS]
            lib.gsss_target_destroy(h)
        rows.append(row)
    os.environ.pop("GSSS_CURVE_TAIL", None)
    return rows


def record():
    """Every row: this process walks GSSS_CURVE_TAIL unset and =0, a child with GSSS_CURVE_L2=1 the curves once more."""
    lib = _lib.load()
    _lib.require_device()
    if os.environ.get("GSSS_CURVE_L2") == "1":
        return walk(lib, None, True)
    rows = walk(lib, None, False) + walk(lib, 0, False)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows"], env=dict(os.environ, GSSS_CURVE_L2="1"),
                           check=True, capture_output=True, text=True, timeout=600)
    return rows + json.loads(child.stdout)


GROUP_KEYS = ("kind", "k", "scale", "batch", "mix_curve", "curve_tail", "curve_l2", "note")


def write_record(path, rows, recorded_from):
    """The file keeps every kernel name and every distinct answer (supported, variant name, the names per variant and placement)
    once; the rows are grouped by everything but d, a group holding its (d, answer) pairs."""
    kernels = sorted({n for r in rows for per_variant in r["names"] for n in per_variant})
    answers, groups = [], {}
    for r in rows:
        ans = [int(r["supported"]), r["variant_name"], [[kernels.index(n) for n in per_variant] for per_variant in r["names"]]]
        if ans not in answers:
            answers.append(ans)
        groups.setdefault(tuple(r[key] for key in GROUP_KEYS), []).append([r["d"], answers.index(ans)])
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"recorded_from":%s,\n"variants":%s,"placements":%s,"group_keys":%s,\n"kernels":[\n' %
                (json.dumps(recorded_from), dump(list(VARIANTS)), dump(list(PLACEMENTS)), dump(list(GROUP_KEYS))))
        f.write(",\n".join(",".join(dump(k) for k in kernels[i:i + 3]) for i in range(0, len(kernels), 3)))
        f.write('],\n"answers":[\n')
        f.write(",\n".join(",".join(dump(a) for a in answers[i:i + 4]) for i in range(0, len(answers), 4)))
        f.write('],\n"groups":[\n')
        f.write(",\n".join(dump([list(key), pairs]) for key, pairs in groups.items()))
        f.write("]}\n")


def load_record(path):
    """The recorded rows spelled out: the inputs of the selection beside `supported`, `variant_name` and `names`."""
    with open(path) as f:
        rec = json.load(f)
    rec["rows"] = []
    for key, pairs in rec["groups"]:
        for d, ans in pairs:
            supported, variant_name, names = rec["answers"][ans]
            rec["rows"].append(dict(zip(rec["group_keys"], key), d=d, supported=bool(supported), variant_name=variant_name,
                                    names=[[rec["kernels"][i] for i in per_variant] for per_variant in names]))
    return rec


def canonical(rows):
    """rows in the record's order and with its fields: what --check compares"""
    keys = GROUP_KEYS + ("d", "supported", "variant_name", "names")
    order = {}
    for r in rows:
        order.setdefault(tuple(r[key] for key in GROUP_KEYS), len(order))
    return sorted(({key: r[key] for key in keys} for r in rows), key=lambda r: order[tuple(r[key] for key in GROUP_KEYS)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the record here")
    ap.add_argument("--check", help="compare the library's answers with this record")
    ap.add_argument("--rows", action="store_true", help="print this process's rows as JSON (the GSSS_CURVE_L2=1 child)")
    ap.add_argument("--recorded-from", default="", help="commit and machine the record is made from (kept in the file)")
    a = ap.parse_args()
    rows = record()
    if a.rows:
        json.dump(rows, sys.stdout)
        return 0
    if a.out:
        write_record(a.out, rows, a.recorded_from)
        print(f"{len(rows)} rows -> {a.out}")
    if a.check:
        want, got = canonical(load_record(a.check)["rows"]), canonical(rows)
        bad = [(w, g) for w, g in zip(want, got) if w != g]
        print(f"{len(got)} rows walked, {len(want)} recorded, {len(bad)} differ")
        for w, g in bad[:20]:
            print("  recorded", json.dumps(w), "\n  got     ", json.dumps(g))
        return 1 if bad or len(want) != len(got) else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
