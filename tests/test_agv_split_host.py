"""CPU check of the AGV step's two halves (csrc/fjsp_env.h: agv_pre + agv_fin, the P wave of
k_step_ag), compiled for the host through tests/hostsim/agv_split_shim.cpp (TEST-ONLY).

agv_pre runs before the other agents' posts arrive and agv_fin after them; together they must equal
agv_execute<true> (with the move's target folded into the AGV word) on the state the other agents
left.  (a) sweeps a constructed product of actions, locations, carried trays, list lengths, storage
caps and changes by the other agents; (b) replays random episodes in P's schedule against the
plain step and counts how often agv_fin's two rare paths ran."""
import ctypes

import pytest

from tests import hostsim_build as HB


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("agv_split"), HB.source("agv_split_shim.cpp"), "agvsplit")
    I64P = ctypes.POINTER(ctypes.c_int64)
    lib.agv_sweep.restype = None
    lib.agv_sweep.argtypes = [I64P, ctypes.c_char_p, ctypes.c_int]
    lib.agv_replay.restype = None
    lib.agv_replay.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, I64P, ctypes.c_char_p, ctypes.c_int]
    return lib


def test_constructed_sweep(shim):
    """Every action 0-7 x location x hands (empty, an empty tray, a tray of each type unprocessed /
    processed / packaged) x source and destination list at length 0-3 x storage at / below its cap
    x what the other agents do between the halves (nothing, a push on the source list, a pop on
    the destination queue, both): every state word, every table byte, the result, move_to and
    pend equal agv_execute<true> on the changed state."""
    out = (ctypes.c_int64 * 6)()
    msg = ctypes.create_string_buffer(512)
    shim.agv_sweep(out, msg, len(msg))
    cases, bad, front_new, successor_new, pickups, pushes = out
    assert cases == 8 * 5 * 11 * 4 * 4 * 2 * 4
    assert bad == 0, msg.value.decode()
    # the product reaches both rare paths, and the common ones, by construction
    assert front_new > 0 and successor_new > 0 and pickups > 0 and pushes > 0


@pytest.mark.parametrize("num_orders", [2, 30])
def test_replay_in_p_schedule(shim, num_orders):
    """32 envs x 450 steps of uniform-random actions with auto-reset, stepped as the P wave does
    (AGV of step k -> agv_pre of k+1 -> the machines' actions of k and the pickup of k+1 ->
    agv_fin) against the plain step, every env-step; both rare paths of agv_fin must have run.
    These inputs (seed 11) reach them with the halves as they were before the re-split as well:
    front new / successor new 6 / 5 times at 2 orders, 4 / 8 at 30, the counts this version reaches."""
    want = {2: (6, 5), 30: (4, 8)}[num_orders]
    out = (ctypes.c_int64 * 5)()
    msg = ctypes.create_string_buffer(512)
    shim.agv_replay(32, 450, num_orders, 11, out, msg, len(msg))
    compared, bad, front_new, successor_new, resets = out
    assert compared == 32 * 450
    assert bad == 0, msg.value.decode()
    assert resets >= 32 * 2            # the 201-step truncation at least
    assert front_new > 0 and successor_new > 0, (front_new, successor_new)
    assert (front_new, successor_new) == want
