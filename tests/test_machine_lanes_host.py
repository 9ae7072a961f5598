"""CPU check of the AM wave's lane-group form (csrc/fjsp_env.h: mach_lane_*, k_step_ag's AM wave),
compiled for the host through tests/hostsim/machine_lanes_shim.cpp (TEST-ONLY).

With 16 or 32 envs per workgroup the wave has 4 or 2 lanes per env; lane group g < 2 holds machine
g in machine slot 0 of its own Env and runs machine_execute<0> and the one-machine run phase
(mach_lane_run) on it.  Here the lanes of an env run one after another and must leave every state
word, table byte, result word and post as the sequence machine_execute<0>, machine_execute<1>,
machines_run<true> on one Env does; 1 group is that sequence with the queue fronts' successors
known ahead against the plain one.  The shim counts, on the sequence alone, what the inputs
contain: a pass on nothing fails."""
import ctypes

import pytest

from tests import hostsim_build as HB


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("machine_lanes"), HB.source("machine_lanes_shim.cpp"), "machinelanes")
    I64P = ctypes.POINTER(ctypes.c_int64)
    lib.mlanes_sweep.restype = None
    lib.mlanes_sweep.argtypes = [ctypes.c_int, I64P, ctypes.c_char_p, ctypes.c_int]
    lib.mlanes_replay.restype = None
    lib.mlanes_replay.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, I64P,
                                  ctypes.c_char_p, ctypes.c_int]
    return lib


@pytest.mark.parametrize("groups", [4, 2, 1])
def test_constructed_sweep(shim, groups):
    """Per machine: empty / 1 queued / 3 queued / busy and due now / busy and not due / idle with a
    current tray / that with 2 queued / busy with a product due, another to go and 1 queued; crossed
    with actions 0-2 per machine, an AGV drop onto either queue or none, and the machines' trays of
    one order or of two."""
    out = (ctypes.c_int64 * 8)()
    msg = ctypes.create_string_buffer(512)
    shim.mlanes_sweep(groups, out, msg, len(msg))
    cases, bad, both_start, start_signal, both_signal, both_done, done_same_order, overwrite = out
    assert cases == 8 * 8 * 9 * 3 * 2
    assert bad == 0, msg.value.decode()
    # by construction: both machines act in one step, complete products of one order in one step,
    # and a START is granted onto a machine that still holds a tray (ST_OVERWRITE)
    assert both_start > 0 and start_signal > 0 and both_signal > 0
    assert both_done > 0 and done_same_order > 0 and overwrite > 0


@pytest.mark.parametrize("groups", [4, 2, 1])
@pytest.mark.parametrize("num_orders", [2, 30])
def test_replay(shim, groups, num_orders):
    """32 envs x 450 steps of uniform-random actions with auto-reset in launches of 7 steps: a
    launch's first step and the step after a reset run the pickup and the AGV on group 0 and hand
    machine 1's lists to group 1; every env-step against the plain step."""
    out = (ctypes.c_int64 * 14)()
    msg = ctypes.create_string_buffer(512)
    shim.mlanes_replay(groups, 32, 450, 7, num_orders, 11, out, msg, len(msg))
    (compared, bad, resets, fresh_steps, both_start, start_signal, both_signal, both_done, done_same_order, overwrite,
     handover_changed, starts, signals, dones) = out
    print(dict(resets=resets, fresh_steps=fresh_steps, both_start=both_start, start_signal=start_signal,
               both_signal=both_signal, both_done=both_done, done_same_order=done_same_order, overwrite=overwrite,
               handover_changed=handover_changed, starts=starts, signals=signals, dones=dones))
    assert compared == 32 * 450
    assert bad == 0, msg.value.decode()
    assert resets >= 32 * 2            # the 201-step truncation at least
    # uniform-random play never has both machines act in one step (the constructed sweep has): the
    # inputs hold each machine's START, SIGNAL and product completions
    assert starts > 100 and signals > 0 and dones > 100
    if groups > 1:
        assert fresh_steps >= 32 * (450 // 7)
        assert handover_changed > 0    # a fresh step's AGV changed machine 1's lists before the hand-over
