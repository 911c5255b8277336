"""The cases of the exact-mode batch sweep (tests/batch_layout_cases.py) without a GPU: which layouts they reach, that the CPU
oracle -- the reference of tests/test_hip_target_batch_layouts.py -- runs every one of them to the end within tens of tries, and
that every case constructs: none is skipped, and what DESIGN.md section 5.6c refuses of them (fast mode beyond the lane kernels)
is asserted as that refusal."""
import numpy as np
import pytest

import batch_layout_cases as bc
import geosss_amd as gs
from geosss_amd import _lib

# The layouts a Bingham batch of the sweep runs in.  A dense A of d + 1 rows of DPAD doubles fits the 136 KiB of rows up to
# d = 128 (129 x 128 doubles = 129 KiB in coop16x8), and the sixty-four-lane layouts read it from global memory above: the row
# budget moves no Bingham case of the sweep out of its natural layout, so all fifteen are reached.
BINGHAM_LAYOUTS = ["lane2", "lane3", "lane4", "lane5", "lane6", "lane8", "lane10", "coop4x4", "coop4x8", "coop16x4", "coop16x8",
                   "coop64x4", "coop64x8", "coop64x16", "coop64x32"]
ALL_KEYS = bc.SWEEP + bc.GLOBAL_CASES


def test_sweep_names_every_layout():
    """gsss_exact_layout(d) over the sweep's dimensions, and the row budget restated in batch_layout_cases.layout_of."""
    lib = _lib.load()
    assert [bc.LAYOUTS[lib.gsss_exact_layout(d) - 1] for d in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 32, 33, 64, 65, 128, 129,
                                                                256, 257, 512, 513, 1024, 1025, 2048)] == \
        ["lane2", "lane3", "lane4", "lane5", "lane6", "coop4x4", "lane8", "coop4x4", "lane10", "coop4x4", "coop4x4", "coop4x8", "coop4x8",
         "coop16x4", "coop16x4", "coop16x8", "coop16x8", "coop64x4", "coop64x4", "coop64x8", "coop64x8", "coop64x16", "coop64x16",
         "coop64x32", "coop64x32"]
    for family in bc.VMF_FAMILIES:
        assert {bc.layout_of((family, d)) for d in bc.DIMS} == set(bc.LAYOUTS), family
    for family in ("bingham_diag",):      # (the dense families have the same shape: d + 1 rows)
        assert {bc.layout_of((family, d)) for d in bc.DIMS} == set(BINGHAM_LAYOUTS), family
    assert all(bc.layout_of((family, d)) == bc.natural_layout(d) for family in ("vmf1", "vmf3", "bingham_diag") for d in bc.DIMS)
    # the first and last d of every layout
    by_layout = {}
    d = 2
    while lib.gsss_exact_layout(d) > 0:
        by_layout.setdefault(lib.gsss_exact_layout(d), []).append(d)
        d += 1
    assert {e for ds in by_layout.values() for e in (ds[0], ds[-1])} <= set(bc.DIMS) and len(by_layout) == len(bc.LAYOUTS)
    # rows in global memory: K = 7000 means leave lane3 for the smallest sixty-four-lane layout
    assert [bc.layout_of(k) for k in bc.GLOBAL_CASES] == ["coop64x4", "coop64x16", "coop64x4", "coop64x8"]
    assert not any(bc.rows_in_lds(k) for k in bc.GLOBAL_CASES)
    assert all(bc.rows_in_lds((f, d)) for f, d in bc.SWEEP if d <= 128 or f in bc.VMF_FAMILIES)
    assert not any(bc.rows_in_lds((f, d)) for f, d in bc.SWEEP if d > 128 and f not in bc.VMF_FAMILIES)


def test_chains_per_target():
    """One full chunk, a ragged one and a workgroup boundary inside every target."""
    assert [bc.chains_per_target(name) for name in ("lane2", "lane10", "coop4x4", "coop4x8", "coop16x4", "coop16x8", "coop64x4", "coop64x32")] == \
        [259, 259, 67, 67, 19, 19, 7, 7]
    assert bc.chains_per_target("lane5", "spread") == 7 and bc.chains_per_target("coop4x4", "spread") == 67
    params = bc.sweep_params()
    assert len(params) == len(set(params)) == 2 * (len(bc.SWEEP) + 7 * len(bc.FAMILIES))      # the seven lane dimensions run spread too
    for key, placement, _ in params:
        per = bc.chains(key, placement) - 3
        assert per in (256, 64, 16, 4) and per * bc.lanes(bc.layout_of(key)) in (256, 4)


@pytest.mark.parametrize("key", ALL_KEYS, ids=bc.case_id)
def test_case_constructs_and_refusals(key):
    """Every case is a TargetBatch of members of one shape that differ; fast mode is refused exactly where section 5.6c says."""
    pdfs = bc.pdfs_of(key)
    M, d = len(pdfs), pdfs[0].d
    assert M == (2 if isinstance(key, str) else 3)
    batch = gs.TargetBatch(pdfs)
    m = bc.chains(key)
    kind, pd, k, _, arrays, extra = batch._pack(chains_per_target=m)
    assert pd == d and arrays == () and extra["chains_per_target"] == m and len(extra["batch"]) == M
    sizes = {tuple(None if a is None else a.shape for a in member[4]) for member in extra["batch"]}
    assert len(sizes) == 1, sizes                                               # an equal stride
    blobs = [b"".join(a.tobytes() for a in member[4] if a is not None) for member in extra["batch"]]
    assert len(set(blobs)) == M, "members coincide"
    if key[0] == "bingham_diag":
        assert all(np.array_equal(p.A, np.diag(np.diag(p.A))) for p in pdfs)
    if key[0] in ("bingham_dense", "binghamfisher") or (isinstance(key, str) and key.startswith("bingham")):
        assert not any(np.array_equal(p.A, np.diag(np.diag(p.A))) for p in pdfs)
    assert (key[0] == "binghamfisher") == all(getattr(p, "b", None) is not None for p in pdfs)
    x0 = bc.x0(key)
    assert x0.shape == (M * m, d) and np.max(np.abs(np.linalg.norm(x0, axis=1) - 1.0)) < 1e-14
    # fast mode: the lane-per-chain kernels of d = 3 .. 16 (mixtures of up to 16 terms, 10 from d = 11 on)
    fast = 3 <= d <= 16 and k <= (16 if d <= 10 else 10)
    if fast:
        plan = batch.launch_plan(m)
        assert plan["grid"] >= 1 and 0.0 < plan["lane_use"] <= 1.0
    else:
        with pytest.raises(ValueError, match="no fast-mode batch kernel"):
            batch.launch_plan(m)


def _reference_params():
    out = [(k, p, s) for k, p, s in bc.sweep_params()]
    return out + [(k, "packed", s) for k in bc.GLOBAL_CASES for s in bc.SAMPLERS]


@pytest.mark.parametrize("key,placement,sampler", _reference_params(), ids=bc.case_id)
def test_oracle_chains_alone(key, placement, sampler):
    """The reference alone: every chain ends without an error bit, on the sphere, within tens of tries a step."""
    pdfs = bc.pdfs_of(key)
    M, m, d = len(pdfs), bc.chains(key, placement), pdfs[0].d
    ref = bc.oracle_chains(key, sampler, placement)
    assert ref["samples"].shape == (M * m, bc.N_STEPS // bc.THIN, d) and ref["state"].shape == (M * m, d)
    assert not ref["err"].any()
    assert np.all(np.isfinite(ref["samples"])) and np.all(np.isfinite(ref["state"]))
    assert np.max(np.abs(np.linalg.norm(ref["state"], axis=1) - 1.0)) < 1e-12
    assert np.array_equal(ref["samples"][:, -1], ref["state"])
    assert np.array_equal(ref["n_tries"], ref["n_reject"] + bc.N_STEPS) and ref["n_tries"].min() >= bc.N_STEPS
    per_step = ref["n_tries"].max() / bc.N_STEPS
    print(f"{bc.case_id(key)} {placement} {sampler}: m = {m}, largest try count of a chain {int(ref['n_tries'].max())} over "
          f"{bc.N_STEPS} steps ({per_step:.1f} a step)")
    assert per_step < 100.0
    # the members' chains differ: a batch that read member 0's rows for every target could not match them
    start = bc.x0(key, placement)
    moved = np.max(np.abs(ref["state"] - start), axis=1)
    assert moved.min() > 1e-6
    wrong = bc.oracle_chains_of_wrong_member(key, sampler) if placement == "packed" else None
    if wrong is not None:
        gap = float(np.max(np.abs(wrong - ref["samples"][m:2 * m])))
        print(f"    member 0 in member 1's place: max |dx| {gap:.2e}")
        assert gap > 1e-3


@pytest.mark.parametrize("sampler", bc.SAMPLERS)
def test_mixed_diagonal_and_dense_case(sampler):
    pdfs, m, x0, ref = bc.mixed_case(sampler)
    diag = [bool(np.array_equal(p.A, np.diag(np.diag(p.A)))) for p in pdfs]
    assert diag == [True, False, True, False] and m == 67 and x0.shape == (4 * 67, 24)
    assert not ref["err"].any() and np.all(np.isfinite(ref["samples"]))
    print(f"mixed d=24 {sampler}: largest try count {int(ref['n_tries'].max())}")


def test_no_case_is_skipped_or_expected_to_fail():
    """Neither this module nor the GPU module marks a case skip or xfail."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("test_target_batch_layouts_host.py", "test_hip_target_batch_layouts.py", "batch_layout_cases.py"):
        text = open(os.path.join(here, name)).read()
        for word in ("pytest.mark." + "skip", "pytest." + "skip", "mark." + "xfail", "pytest." + "xfail", "import" + "orskip"):
            assert word not in text, (name, word)
