"""The piece plan of the lane kernels' partial round (gsss_piece_plan, piece_plan in gsss_device.h) without a GPU.

C chunks of N steps on R resident workgroups, C > R and C not a multiple of R: the chunks are laid end to end and the line is
cut into R slots of T = ceil(C N / R) steps (McNaughton's wrap-around rule), boundaries moved by less than 32 steps so that no
part of a split chunk is shorter than 32.  A chunk that crosses a boundary runs as two pieces -- its head [0, b) at the start
of the later slot, its tail [b, N) at the end of the earlier one -- and ticket t takes entry t of the table.  What the device
relies on is restated and checked here independently of the library: exact cover, one split per chunk at most, heads before
tails in the table AND in time when workgroups take the entries in order as slots fall free, and a makespan of T + 32."""
import ctypes as C
import heapq

import numpy as np
import pytest

from geosss_amd import _lib

WHOLE, HEAD, TAIL = 0, 1, 2
SHAPES = [(1281, 1280), (1954, 1280), (3907, 768), (2000, 768), (257, 256)]
STEPS = [256, 300, 1000, 4096]


def plan(c, r, n):
    lib = _lib.load()
    count = lib.gsss_piece_plan(c, r, n, None, 0)
    assert count >= 0, lib.gsss_last_error()
    table = np.zeros((max(count, 1), 4), dtype=np.int32)
    assert lib.gsss_piece_plan(c, r, n, table.ctypes.data_as(C.POINTER(C.c_int32)), count) == count
    return table[:count]


def test_exported_and_bound():
    lib = _lib.load()
    assert "gsss_piece_plan" in _lib.SIGNATURES and hasattr(lib, "gsss_piece_plan")
    assert lib.gsss_piece_plan(0, 1280, 1000, None, 0) == -1              # GSSS_E_INVALID
    assert lib.gsss_piece_plan(1954, 0, 1000, None, 0) == -1
    assert lib.gsss_piece_plan(1954, 1280, 0, None, 0) == -1
    buf = (C.c_int32 * 8)()
    assert lib.gsss_piece_plan(1954, 1280, 1000, buf, 2) == -1            # a table that does not fit is not written in part
    assert b"gsss_piece_plan" in lib.gsss_last_error()


@pytest.mark.parametrize("c,r", [(1280, 1280), (2560, 1280), (700, 1280), (1, 256), (768 * 5, 768)])
@pytest.mark.parametrize("n", STEPS)
def test_no_plan_when_the_chunks_fill_whole_rounds(c, r, n):
    assert len(plan(c, r, n)) == 0


@pytest.mark.parametrize("c,r", SHAPES)
def test_no_plan_for_short_launches(c, r):
    for n in (1, 64, 255):
        assert len(plan(c, r, n)) == 0


@pytest.mark.parametrize("c,r", SHAPES)
@pytest.mark.parametrize("n", STEPS)
def test_piece_plan(c, r, n):
    t = plan(c, r, n)
    chunk, begin, length, kind = (t[:, i].astype(np.int64) for i in range(4))
    assert len(t) > c and set(np.unique(kind)) <= {WHOLE, HEAD, TAIL}
    assert np.all((chunk >= 0) & (chunk < c)) and np.all(begin >= 0) and np.all(length > 0) and np.all(begin + length <= n)
    # every (chunk, step) exactly once
    cover = np.zeros((c, n), dtype=np.int8) if c * n <= 1 << 24 else None
    steps_of = np.zeros(c, dtype=np.int64)
    np.add.at(steps_of, chunk, length)
    assert np.all(steps_of == n)
    if cover is not None:
        for ch, b, l in zip(chunk, begin, length):
            cover[ch, b:b + l] += 1
        assert np.all(cover == 1)
    # at most two pieces per chunk: a whole one, or a head [0, b) and a tail [b, n)
    pieces = np.bincount(chunk, minlength=c)
    assert np.all((pieces == 1) | (pieces == 2))
    index_of = {}
    for i, (ch, b, l, k) in enumerate(zip(chunk, begin, length, kind)):
        if pieces[ch] == 1:
            assert (k, b, l) == (WHOLE, 0, n), i
        else:
            assert k in (HEAD, TAIL) and l >= 32, (i, k, l)
            assert (b == 0) if k == HEAD else (b + l == n), i
            index_of[(ch, k)] = i
    split = np.flatnonzero(pieces == 2)
    assert 0 < len(split) < r
    for ch in split:
        head, tail = index_of[(ch, HEAD)], index_of[(ch, TAIL)]
        assert head < tail, ch                                        # a tail waits only for an earlier ticket
        assert length[head] == begin[tail], ch                        # ... and starts where the head stopped
    # workgroups take the entries in order, each on the slot that falls free first: the launch ends within T + 32 steps,
    # and no tail starts before its head has ended
    slot_len = -(-c * n // r)
    free = [0] * r
    heapq.heapify(free)
    start = np.zeros(len(t), dtype=np.int64)
    for i, l in enumerate(length):
        start[i] = heapq.heappop(free)
        heapq.heappush(free, start[i] + l)
    assert max(free) <= slot_len + 32, (max(free), slot_len)
    for ch in split:
        head, tail = index_of[(ch, HEAD)], index_of[(ch, TAIL)]
        assert start[tail] >= start[head] + length[head], (ch, start[head], length[head], start[tail])
