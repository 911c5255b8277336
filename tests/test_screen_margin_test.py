"""The single-precision screen's verdict (ScreenVmf::screen, gsss_screen.h) tests dev = fl(sum - 1) against +-margin.  It must be
the real-number test sum < 1 - margin / sum > 1 + margin that the margin was derived for, and it may differ from the older
comparison with fl(1 - margin) / fl(1 + margin) only for a sum one float from where those rounded.  float32 arithmetic here is
IEEE round-to-nearest-even, as v_sub_f32 / v_add_f32 are."""
import numpy as np

F32 = np.float32


def _verdict_dev(s, m):
    dev = (s - F32(1.0)).astype(F32)
    return np.where(dev < -m, -1, np.where(dev > m, 1, 0))


def _verdict_old(s, m):
    lo, hi = (F32(1.0) - m).astype(F32), (F32(1.0) + m).astype(F32)
    return np.where(s < lo, -1, np.where(s > hi, 1, 0))


def _verdict_real(s, m):
    s64, m64 = s.astype(np.float64), m.astype(np.float64)  # 1 -+ m and s - 1 are exact in double for m >= 2^-24
    return np.where(s64 < 1.0 - m64, -1, np.where(s64 > 1.0 + m64, 1, 0))


def _neighbours(x, k=3):
    """the floats around each x, bit pattern by bit pattern ([n, 2k + 1])"""
    return (x.astype(F32).view(np.int32)[:, None] + np.arange(-k, k + 1, dtype=np.int32)).view(F32)


def _cases():
    rng = np.random.default_rng(7)
    # margins as make32 forms them: finite ones in [2^-24, 0.25)
    m = np.exp(rng.uniform(np.log(2.0 ** -24), np.log(0.25), 4000)).astype(F32)
    edges = np.stack([(F32(1.0) - m).astype(F32), (F32(1.0) + m).astype(F32), np.ones_like(m)], 1)  # [n, 3]
    s_edge = _neighbours(edges.ravel()).ravel()
    m_edge = np.repeat(m, 3 * 7)
    s_wide = rng.uniform(0.0, 4.0, 20000).astype(F32)  # the range of a try's sum, and beyond [0.5, 2]
    m_wide = rng.choice(m, s_wide.size)
    return np.concatenate([s_edge, s_wide]), np.concatenate([m_edge, m_wide]).astype(F32)


def test_verdict_is_the_real_number_test():
    s, m = _cases()
    assert np.array_equal(_verdict_dev(s, m), _verdict_real(s, m))


def test_nan_sum_and_infinite_margin_stay_undecided():
    s = np.array([np.nan, 0.0, 0.5, 1.0, 2.0, 30.0, np.inf], F32)
    assert np.all(_verdict_dev(s[:1], np.full(1, F32(0.1))) == 0)
    assert np.all(_verdict_dev(s[1:6], np.full(5, F32(np.inf))) == 0)


def test_differs_from_the_rounded_bounds_only_next_to_them():
    s, m = _cases()
    v, w = _verdict_dev(s, m), _verdict_old(s, m)
    diff = v != w
    assert diff.any(), "the cases reach the edges where fl(1 -+ margin) rounds"
    lo, hi = (F32(1.0) - m).astype(F32), (F32(1.0) + m).astype(F32)
    bits = s.view(np.int32).astype(np.int64)
    ulps = np.minimum(np.abs(bits - lo.view(np.int32)), np.abs(bits - hi.view(np.int32)))
    assert np.all(ulps[diff] <= 1)
