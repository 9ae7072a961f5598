"""CPU check of fjsp_env.h's pack_words (the pack words fjsp_step_sched stores), compiled for the
host through tests/hostsim/pack_shim.cpp (TEST-ONLY).

The host build of the state machine replays each run of tests/golden/packaging.npz (the twelve
recorded traces and the scripted station policies, with their configs and order tables): its
result words and flags must be the recording's, and pack_words of the state after each step and
before the reset must equal the words the fixture built from the reference's objects, row for
row; the call must leave the state as it is; every row's sum of the four `completed` fields is the
recorded total_products_packaged."""
import ctypes

import numpy as np
import pytest

from tests import hostsim_build as HB
from tests import packaging_util as PU

ST_DIVERGED, ST_PKG_WAIT, ST_PROD_LOST = 0x1, 0x4, 0x10


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("pack"), HB.source("pack_shim.cpp"), "pack")
    P = ctypes.c_void_p
    lib.pack_replay.restype = None
    lib.pack_replay.argtypes = [P, P, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P,
                                ctypes.POINTER(ctypes.c_int64)]
    return lib


@pytest.mark.parametrize("key", PU.KEYS)
def test_replay_equals_the_reference_objects(shim, key):
    r = PU.run(key)
    T = len(r["actions"])
    arr = lambda x, dt: np.ascontiguousarray(x, dtype=dt)  # noqa: E731
    actions, results = arr(r["actions"], np.uint8), arr(r["results"][:, :, 0], np.uint32)
    term, trunc, orders = arr(r["term"][:, 0], np.uint8), arr(r["trunc"][:, 0], np.uint8), arr(r["orders"], np.uint8)
    cfg = arr(r["cfg"], np.int32)
    pack = np.full((T, 4), 0xDEADBEEF, np.uint32)
    packaged = np.full(T, -1, np.int32)
    out = (ctypes.c_int64 * 5)()
    shim.pack_replay(actions.ctypes.data, results.ctypes.data, term.ctypes.data, trunc.ctypes.data, orders.ctypes.data,
                     orders.shape[0], orders.shape[1], T, cfg.ctypes.data, pack.ctypes.data, packaged.ctypes.data, out)
    assert out[0] == 0 and out[1] == 0, "the host replay left the recording"
    assert out[2] == int((term | trunc).astype(bool).sum()) == orders.shape[0] - 1
    assert out[3] == 0, "pack_words changed the state"
    # no run diverges or waits at a station; the capacity-5 run loses products once both blue
    # stations are full, the scripted heuristic runs flag nothing else
    assert not out[4] & (ST_DIVERGED | ST_PKG_WAIT), hex(out[4])
    if key in PU.SCRIPTED_KEYS:
        assert out[4] == (ST_PROD_LOST if key == "eager_cap5_s0" else 0), hex(out[4])
    want = r["pack"][:, :, 0]
    assert pack.tobytes() == want.tobytes(), np.argwhere(pack != want)[:5]
    assert packaged.tolist() == r["packaged"].tolist()
    runs, pending, completed = PU.schedule.pack_fields(want)
    assert completed.sum(axis=1).tolist() == r["packaged"].tolist()
    assert runs.max() >= 1 and pending.max() >= 1 and completed.max() >= 1   # not a comparison of zeros
