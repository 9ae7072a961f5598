"""CPU check of the sliced pre-draw lane (csrc/fjsp_predraw.h: the per-lane machine of k_step_ag's PD
wave), compiled for the host through tests/hostsim/predraw_shim.cpp (TEST-ONLY).

The lane draws a table in slices (load, refill, consume) that fall in different steps; the shim
drives it by the schedule the kernel's step loop gives it, both ways (a refill and a consume in
every step; alternating by the step's parity) and from both parities.  For every table size and
every start cursor below, the order words, the final cursor and all 624 words of the work row must
be those of the one-shot draw of a reset on a copy of the same row, and those of hostsim.cpp's
sequential generator (numpy's stream); the same after an interruption at every slice, where a new
episode's mailbox makes the lane start over on the row the reset left.  The steps to readiness
must leave the table ready in time at 16, 32 and 64 envs per workgroup.

How the rows compare: against the same 4-word groups drawn unsliced, (pos, g) and the row are
equal word for word.  A reset regenerates 32 words per batch, so its g runs ahead of the lane's in
the same block: pos is equal, and the rows are equal once the words between the two g are
regenerated; against the sequential generator the block is completed the same way."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests import hostsim_build as HB

NUM_ORDERS = [0, 1, 2, 5, 30, 64]
# (pos, g) of the live row: words [0, g) are current, pos <= g, g a multiple of 4 as every refill
# leaves it.  (0, 0): a fresh block; g = 624: a whole block (numpy's pos < 624); g < pos + 4: where
# a 4-word refill stopped; pos near 624: the table crosses the wrap.
CURSORS = [(0, 0), (1, 4), (1, 624), (3, 4), (3, 624), (226, 228), (226, 624), (227, 228), (228, 232), (228, 624),
           (396, 400), (397, 400), (397, 624), (620, 624), (623, 624), (100, 120), (500, 504), (560, 624), (612, 616)]
# Envs per workgroup -> (alternating slices, steps before a lane's first refill): the wave copies
# one env's row per step from step 1 on, a row is stored a step after its load and its lane
# refills from the step after that, or one later by the parity.
EPW = {16: (1, 16 + 3), 32: (0, 32 + 3), 64: (0, 64 + 3)}
READY_BY = {30: 128, 64: 190}   # steps from the episode's start within which the table is ready


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("predraw"), HB.source("predraw_shim.cpp"), "predraw")
    lib.pd_sweep.restype = None
    lib.pd_sweep.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int64)]
    return lib


def key_of(seed):
    """A whole MT19937 block as numpy holds it after some draws (key, pos < 624)."""
    rs = np.random.RandomState(seed)
    rs.randint(0, 4, size=700)
    return np.ascontiguousarray(rs.get_state()[1], dtype=np.uint32)


def sweep(lib, key, pos, g, num_orders, alternate, interruptions=True):
    out = (ctypes.c_int64 * 4)()
    lib.pd_sweep(key.ctypes.data, pos, g, num_orders, alternate, int(interruptions), out)
    return {"fails": out[0], "first": out[1], "steps": out[2], "points": out[3]}


@pytest.mark.parametrize("alternate", [0, 1])
@pytest.mark.parametrize("num_orders", NUM_ORDERS)
def test_sliced_lane_equals_one_shot_and_sequential(shim, num_orders, alternate):
    key = key_of(11 + num_orders)
    points = 0
    for pos, g in CURSORS:
        r = sweep(shim, key, pos, g, num_orders, alternate)
        assert r["fails"] == 0, (pos, g, r)
        points += r["points"]
    if num_orders:
        assert points > 3 * len(CURSORS)   # every slice of every table was an interruption point


@pytest.mark.parametrize("epw", sorted(EPW))
@pytest.mark.parametrize("num_orders", sorted(READY_BY))
def test_table_ready_in_time(shim, epw, num_orders):
    alternate, before = EPW[epw]
    worst = 0
    for seed in range(40):
        key = key_of(1000 + seed)
        for pos, g in [(0, 0), (3, 624), (397, 400), (560, 624)]:
            r = sweep(shim, key, pos, g, num_orders, alternate, interruptions=False)
            assert r["fails"] == 0
            worst = max(worst, r["steps"])
    print(f"epw {epw} num_orders {num_orders}: ready by step {before + worst}")
    assert before + worst < READY_BY[num_orders], (before, worst)


def test_sweep_under_sanitizers(tmp_path):
    """The same sweep as a stand-alone program under ASan + UBSan (nothing loaded into Python)."""
    exe = HB.build_program(tmp_path, [HB.source("predraw_san_main.cpp")], sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed checks" in r.stdout
