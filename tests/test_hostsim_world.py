"""CPU check of the comparers every wave replay is judged by (tests/hostsim/world.h: same_live and
same_world, through tests/hostsim/world_shim.cpp, TEST-ONLY).

Two equal worlds after some random steps, the AGV carrying a tray; one bit is flipped in a copy of
the second.  same_live must see every flip in the live part (a state word, an order below
num_orders, a slot's code, link or completion step below slot_next) and none outside it, nor in the
two links it exempts: the carried slot's and the caller's dead_slot.  same_world sees them all."""
import ctypes

import pytest

from tests import hostsim_build as HB

NUM_ORDERS, MAX_ORDERS, MAX_SLOTS, NSTATE, NIL = 5, 64, 255, 30, 255
STATE, ORDERS, SCODE, SNEXT, SCSTEP = range(5)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("world"), HB.source("world_shim.cpp"), "world")
    I32P = ctypes.POINTER(ctypes.c_int32)
    lib.world_prepare.restype = None
    lib.world_prepare.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, I32P]
    lib.world_flip.restype = None
    lib.world_flip.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, I32P]
    info = (ctypes.c_int32 * 3)()
    lib.world_prepare(NUM_ORDERS, 11, 200, info)
    steps, slot_next, carry = info
    assert steps > 0, "the rollout never had the AGV carry a tray"
    assert carry + 3 <= slot_next < MAX_SLOTS

    def flip(table, index, dead_slot=NIL):
        verdict = (ctypes.c_int32 * 2)()
        lib.world_flip(table, index, dead_slot, verdict)
        return bool(verdict[0]), bool(verdict[1])
    return flip, slot_next, carry


def test_equal_worlds_are_equal(world):
    flip, _, _ = world
    assert flip(-1, 0) == (True, True)


def test_every_live_flip_is_seen(world):
    flip, slot_next, carry = world
    for w in range(NSTATE):
        assert flip(STATE, w) == (False, False), w
    for o in range(NUM_ORDERS):
        assert flip(ORDERS, o) == (False, False), o
    for s in range(slot_next):
        assert flip(SCODE, s) == (False, False), s
        assert flip(SCSTEP, s) == (False, False), s
        if s != carry:
            assert flip(SNEXT, s) == (False, False), s


def test_flips_outside_the_live_part_pass_same_live_only(world):
    flip, slot_next, _ = world
    for o in range(NUM_ORDERS, MAX_ORDERS):
        assert flip(ORDERS, o) == (True, False), o
    for s in range(slot_next, MAX_SLOTS):
        for table in (SCODE, SNEXT, SCSTEP):
            assert flip(table, s) == (True, False), (table, s)


def test_the_two_exempt_links(world):
    flip, slot_next, carry = world
    assert flip(SNEXT, carry) == (True, False)
    dead = carry + 1
    assert flip(SNEXT, dead, dead_slot=dead) == (True, False)
    assert flip(SNEXT, dead) == (False, False)                       # exempt only when named
    assert flip(SNEXT, carry + 2, dead_slot=dead) == (False, False)  # and only the slot named
    # the exemptions cover the link alone
    assert flip(SCODE, carry) == (False, False) and flip(SCSTEP, dead, dead_slot=dead) == (False, False)
