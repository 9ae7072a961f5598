"""CPU check of the pickup station run ahead of the AGV's previous step (csrc/fjsp_env.h:
pickup_execute on the words before that AGV, then pickup_compose; the E3 wave of k_step_ag),
compiled for the host through tests/hostsim/pickup_ahead_shim.cpp (TEST-ONLY).

The speculative pickup followed by pickup_compose must equal pickup_execute on the words the AGV
left; on a sensitive lane the pickup run again on those words must.  (a) sweeps a constructed
product; (b) replays random episodes in the kernel's schedule against the plain step and counts how
often the AGV's pop met a pickup run ahead of it."""
import ctypes

import pytest

from tests import hostsim_build as HB


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("pickup_ahead"), HB.source("pickup_ahead_shim.cpp"), "pickupahead")
    I64P = ctypes.POINTER(ctypes.c_int64)
    lib.pickup_sweep.restype = None
    lib.pickup_sweep.argtypes = [I64P, ctypes.c_char_p, ctypes.c_int]
    lib.pickup_replay.restype = None
    lib.pickup_replay.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, I64P,
                                  ctypes.c_char_p, ctypes.c_int]
    return lib


def test_constructed_sweep(shim):
    """Pickup action 0-2 x current order (none, mid-order, its last product next) x tray (none,
    partly filled, one below tray_cap) x pool 0-2 x L_PREADY at length 0-3 x the AGV's delta (none,
    a pop, a pool refill, both) x orders left or not: every state word, every table byte over a
    stale fill, the result word and the status bits equal the plain order (the AGV, then the
    pickup).  `sensitive` is set only where the two orders differ, and `unlink` exactly where the
    pop and the push met on a list of one."""
    out = (ctypes.c_int64 * 6)()
    msg = ctypes.create_string_buffer(512)
    shim.pickup_sweep(out, msg, len(msg))
    cases, bad, sensitive, pop_push_1, pop_push_n, sensitive_agree = out
    assert cases == 3 * 3 * 3 * 3 * 4 * 4 * 2
    assert bad == 0, msg.value.decode()
    assert sensitive > 0 and pop_push_1 > 0 and pop_push_n > 0, (sensitive, pop_push_1, pop_push_n)
    assert sensitive_agree == 0


@pytest.mark.parametrize("num_orders,pool0", [(2, 1000), (30, 1000), (30, 3)])
def test_replay_in_the_kernel_schedule(shim, num_orders, pool0):
    """32 envs x 450 steps of uniform-random actions with auto-reset, stepped as the kernel does
    (speculative pickup of step k+2 -> agv_pre of k+1 -> the rest of step k -> compose -> agv_fin)
    against the plain step, every env-step.  The AGV must have popped L_PREADY, a pickup run ahead
    must have pushed in the same step, and at least once onto a list of one."""
    out = (ctypes.c_int64 * 7)()
    msg = ctypes.create_string_buffer(512)
    shim.pickup_replay(32, 450, num_orders, pool0, 11, out, msg, len(msg))
    compared, bad, pops, pop_push, pop_push_1, sensitive, resets = out
    print("pops %d pop+push %d at n=1 %d sensitive %d resets %d" % (pops, pop_push, pop_push_1, sensitive, resets))
    assert compared == 32 * 450
    assert bad == 0, msg.value.decode()
    assert resets >= 64
    assert pops > 0 and pop_push > 0 and pop_push_1 > 0, (pops, pop_push, pop_push_1)
