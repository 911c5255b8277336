"""diagnostics.ring_plan, the integer plan of Sampler.summarize's one reused buffer, against the two loops it replaced, restated
here as they stood, and against what the kernels that read the ring rely on.  No device: the plan is integers alone."""
import itertools

from geosss_amd.diagnostics import ring_plan

GRID = [(rest, window, H, seen) for rest, window, H in itertools.product(range(41), range(1, 10), range(6)) for seen in range(H + 1)]


def _two_loops(rest, window, H, seen):
    """summarize's walk before ring_plan: -> (rows, draw 0, windows, rows gathered as the new hist)"""
    rows = H + window
    windows = []
    if not H:
        draw0 = None                              # fold(self._state[None])
        done = 0
        while done < rest:
            w = min(window, rest - done)
            windows.append((0, w, 0))             # fold(advance(.., out=buf[:w]))
            done += w
        return rows, draw0, windows, []
    draw0 = (seen, 1, seen)                       # buf[seen] = state; fold(buf[seen:seen + 1], seen, seen)
    pos, seen, done = seen + 1, seen + 1, 0
    while done < rest:
        pos %= rows
        w = min(window, rest - done, rows - pos)
        windows.append((pos, w, min(H, seen)))    # fold(advance(.., out=buf[pos:pos + w]), pos, min(H, seen))
        pos, seen, done = pos + w, seen + w, done + w
    last = [(pos - min(H, seen) + i) % rows for i in range(min(H, seen))]
    return rows, draw0, windows, last


def test_ring_plan_is_the_two_loops():
    assert len(GRID) == 41 * 9 * 21
    for case in GRID:
        assert ring_plan(*case) == _two_loops(*case), case


def test_window_cut_by_the_rings_end():
    """H = 2, window = 3: a ring of 5 rows; draw 0 at row 0, a window of 3 at rows 1 .. 3, then one row before the end."""
    rows, draw0, windows, keep = ring_plan(10, 3, 2, 0)
    assert rows == 5 and draw0 == (0, 1, 0)
    assert windows == [(1, 3, 1), (4, 1, 2), (0, 3, 2), (3, 2, 2), (0, 1, 2)]
    assert keep == [4, 0]


def test_what_the_kernels_rely_on():
    for rest, window, H, seen in GRID:
        rows, draw0, windows, keep = ring_plan(rest, window, H, seen)
        assert rows == H + window
        assert sum(w for _, w, _ in windows) == rest and all(1 <= w <= window for _, w, _ in windows)
        if not H:
            assert draw0 is None and keep == [] and all(first == 0 and h == 0 for first, _, h in windows)
            continue
        # replay the plan on a ring of draw numbers: the earlier call's draws are -seen .. -1, draw 0, then 1 .. rest
        ring = [None] * rows
        ring[:seen] = range(-seen, 0)
        row, one, h = draw0
        assert (row, one, h) == (seen, 1, seen) and h <= H
        ring[row] = 0
        nxt = 1
        for first, w, h in windows:
            assert 0 <= first and first + w <= rows                       # no window crosses the ring's end
            assert h == min(H, seen + nxt) <= H
            before = [(first - h + i) % rows for i in range(h)]
            assert not set(before) & set(range(first, first + w))         # the history is not what the window overwrites
            assert [ring[r] for r in before] == list(range(nxt - h, nxt))   # .. and holds the h draws before it, oldest first
            ring[first:first + w] = range(nxt, nxt + w)
            nxt += w
        assert nxt == rest + 1                                            # every draw once, in order
        k = min(H, seen + nxt)
        assert [ring[r] for r in keep] == list(range(nxt - k, nxt))       # the last min(H, draws so far) draws, oldest first
