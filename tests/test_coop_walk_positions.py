"""CPU: the running positions of the cooperative walk (csrc/gact_walk_pos.hpp) against the closed forms they replace.

coop_walk_batch used to compute, from scratch at every move,
    p = max(p0 + njs, 0), l = (p * kMagic) >> 16, c = p - l * CW          (lane and column in lane of the walk's column)
    rp = rpos0 + dir * nis, qp = qpos0 + dir * njs                        (positions of the cell's bases in the staged slices)
and now keeps the column relative to the lane a trip of eight moves began in, with one clamp, and takes a base's bit
position from one 24-bit multiply-add.  gact_walk_pos.hpp is plain integer code, so this test compiles it with the host
compiler beside a few lines that drive it the way the kernel does -- walk_trip_begin at a refill, walk_col_left per move,
walk_lane_before for the lane a move reads, walk_trip_end before the next refill -- and compares move by move: CW = 13,
every p0 of the sixteen lanes, every run of column moves down to the clamp and eight moves beyond it, the refill falling
on every place of the run, runs with moves that consume no column in between, and both directions."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

CW, LANES = 13, 16
K_MAGIC = (65536 + CW - 1) // CW
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "darwin-gpu_amd", "csrc")

_SHIM = r"""
#include "gact_walk_pos.hpp"
extern "C" {
// n moves from (l, c); the first trip has `first` moves left, every later one eight.  Per move: the lane and the column in
// lane that the move's fetch uses, and (l, c) as a refill placed right behind this move would get them.
void walk_cols(int l, int c, int first, const int *dj, int n, int *l_use, int *c_use, int *l_refill, int *c_refill)
{
    int left = first, cr, cr_min, l0 = l;
    gact::walk_trip_begin<13>(l, c, cr, cr_min);
    for (int i = 0; i < n; i++) {
        if (left == 0) {
            gact::walk_trip_end<13>(l0, cr, l, c);
            l0 = l;
            gact::walk_trip_begin<13>(l, c, cr, cr_min);
            left = 8;
        }
        gact::walk_col_left(cr, cr_min, dj[i]);
        left--;
        const int before = gact::walk_lane_before(cr);
        l_use[i] = l0 + before;
        c_use[i] = cr + (before & 13);
        gact::walk_trip_end<13>(l0, cr, l_refill[i], c_refill[i]);
    }
}
int walk_pos2(int fix2, int dir2, int n) { return gact::walk_pos2(fix2, dir2, n); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler (the oracle's build needs one too)"
    d = tmp_path_factory.mktemp("walk_pos")
    src, lib = str(d / "shim.cpp"), str(d / "libwalkpos.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + _CSRC, "-o", lib, src])
    L = ctypes.CDLL(lib)
    ip = ctypes.POINTER(ctypes.c_int)
    L.walk_cols.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ip, ip, ip, ip]
    L.walk_cols.restype = None
    L.walk_pos2.argtypes = [ctypes.c_int] * 3
    L.walk_pos2.restype = ctypes.c_int
    return L


def _closed_form(p0, dj):
    njs = -np.cumsum(dj)
    p = np.maximum(p0 + njs, 0)
    l = (p * K_MAGIC) >> 16
    return l, p - l * CW


def _run(shim, p0, first, dj):
    dj = np.ascontiguousarray(dj, dtype=np.int32)
    out = [np.empty(len(dj), dtype=np.int32) for _ in range(4)]
    ip = ctypes.POINTER(ctypes.c_int)
    shim.walk_cols(p0 // CW, p0 % CW, first, dj.ctypes.data_as(ip), len(dj), *[o.ctypes.data_as(ip) for o in out])
    return out


def test_magic_divides():
    p = np.arange(LANES * CW)
    assert np.array_equal((p * K_MAGIC) >> 16, p // CW)


def test_every_column_run_down_to_the_clamp_and_beyond(shim):
    """all moves consume a column: from every p0 the walk crosses every lane boundary below it, reaches p = 0 and stays
    there for eight more moves; the refill falls on every place of the run"""
    checked = 0
    for p0 in range(LANES * CW):
        dj = np.ones(p0 + 8, dtype=np.int32)
        want_l, want_c = _closed_form(p0, dj)
        for first in range(1, 9):
            l_use, c_use, l_ref, c_ref = _run(shim, p0, first, dj)
            for name, got, want in (("l", l_use, want_l), ("c", c_use, want_c), ("l at refill", l_ref, want_l), ("c at refill", c_ref, want_c)):
                assert np.array_equal(got, want), (p0, first, name, int(np.flatnonzero(got != want)[0]))
            checked += len(dj)
    assert checked == 8 * sum(p0 + 8 for p0 in range(LANES * CW))


def test_moves_that_consume_no_column(shim):
    """insertion moves (dj = 0) between the column moves, so that a trip's eight moves hold 0 ... 8 column moves and the lane
    boundary and the clamp fall behind any number of them; a walk that has stopped (dj = 0 for good) stays where it is"""
    rng = np.random.default_rng(1313)
    for p0 in range(LANES * CW):
        for density in (0.2, 0.5, 0.9):
            dj = (rng.random(2 * p0 + 24) < density).astype(np.int32)
            dj[-10:] = 0
            want_l, want_c = _closed_form(p0, dj)
            first = int(rng.integers(1, 9))
            l_use, c_use, l_ref, c_ref = _run(shim, p0, first, dj)
            assert np.array_equal(l_use, want_l) and np.array_equal(c_use, want_c), (p0, density, first)
            assert np.array_equal(l_ref, want_l) and np.array_equal(c_ref, want_c), (p0, density, first)
            assert (l_use[-10:] == l_use[-11]).all() and (c_use[-10:] == c_use[-11]).all()


@pytest.mark.parametrize("direction", (1, -1))
def test_base_positions(shim, direction):
    """walk_pos2 with the segment's LDS byte address folded in, as the kernel calls it: the word it addresses and the bit
    offset it leaves in the low five bits are those of pos0 + dir * n, for every n of a tile and every staged start"""
    n = -np.arange(0, 321)
    for seg_a in (0, 4 * 26, 4 * 9973):
        for pos0 in list(range(16, 32)) + [16 + 319, 31 + 319]:
            if direction > 0 and pos0 < 16 + 319:
                continue                                  # forward slices are walked downwards from their last base
            if direction < 0 and pos0 >= 16 + 319:
                continue
            closed = pos0 + direction * n
            assert (closed >= 0).all()
            got = np.array([shim.walk_pos2(2 * pos0 + 8 * seg_a, 2 * direction, int(x)) for x in n], dtype=np.int64)
            assert np.array_equal((got >> 3) & ~3, seg_a + 4 * (closed >> 4)), (seg_a, pos0)
            assert np.array_equal(got & 31, 2 * (closed & 15)), (seg_a, pos0)
