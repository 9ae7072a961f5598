"""CPU check of the step-kernel selector (csrc/fjsp_select.h, compiled for the host through
tests/hostsim/select_shim.cpp, TEST-ONLY): the measured thresholds of fjsp_step_many's kernel
choice, row by row.  The plan's name is what fjsp_last_kernel reports and its variant is what
the launch switches on, so the GPU tests that pin a path by name rest on these rules."""
import ctypes
import itertools

import pytest

from tests import hostsim_build as HB

UNMASKED, MASKED, HEURISTIC = 0, 1, 2   # FJSP_ACTIONS_*
MANY, PIPE, AG = 0, 1, 2                # StepFamily
OPTS = ("fused_lds", "pipeline", "predraw", "agents", "ag_envs", "step_envs", "test_stall")
DEFAULTS = dict(fused_lds=-1, pipeline=1, predraw=1, agents=1, ag_envs=0, step_envs=0, test_stall=0)   # fjsp_create
AG_NAME = "k_step_ag<lds,predraw>"
# every name fjsp_step_many can report
NAMES = {"k_step_many", "k_step_many<lds>", "k_step_many<full>", "k_step_many<lds,full>",
         "k_step_pipe<1emit>", "k_step_pipe<2emit>", "k_step_pipe<lds,1emit>", "k_step_pipe<lds,2emit>",
         "k_step_pipe<lds,2emit,predraw>", AG_NAME}


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("select"), HB.source("select_shim.cpp"), "select")
    lib.sel_step_many.restype = ctypes.c_char_p
    lib.sel_step_many.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)] * 2

    def call(n, K=1024, mode=UNMASKED, autoreset=1, full=0, **opts):
        assert set(opts) <= set(OPTS), opts
        o = (ctypes.c_int * len(OPTS))(*[{**DEFAULTS, **opts}[k] for k in OPTS])
        plan = (ctypes.c_int * 9)()
        name = lib.sel_step_many(n, K, mode, autoreset, full, o, plan).decode()
        keys = ("family", "lds", "full", "nemit", "predraw", "epw", "stall", "grid", "waves")
        return dict(zip(keys, plan), name=name)
    return call


# (n, deviation from: lean outputs, autoreset, UNMASKED, K = 1024, default options), name, grid, waves, ag's epw
ROWS = [
    (1, {}, AG_NAME, 1, 8, 16),
    (4096, {}, AG_NAME, 256, 8, 16),
    (4097, {}, AG_NAME, 129, 8, 32),
    (8192, {}, AG_NAME, 256, 8, 32),
    (8193, {}, AG_NAME, 129, 8, 64),
    (4096, dict(K=63), AG_NAME, 64, 8, 64),
    (4096, dict(K=64), AG_NAME, 256, 8, 16),
    (200, dict(ag_envs=32), AG_NAME, 7, 8, 32),
    (16384, {}, AG_NAME, 256, 8, 64),
    (16385, {}, AG_NAME, 257, 8, 64),
    (32768, {}, AG_NAME, 512, 8, 64),
    (32769, {}, "k_step_pipe<1emit>", 513, 2, None),
    (20000, dict(fused_lds=0), "k_step_pipe<1emit>", 313, 2, None),
    (20000, dict(fused_lds=1), AG_NAME, 313, 8, 64),
    (20000, dict(predraw=0), "k_step_pipe<1emit>", 313, 2, None),
    (20000, dict(autoreset=0), "k_step_pipe<1emit>", 313, 2, None),
    (16448, dict(agents=0), "k_step_pipe<1emit>", 257, 2, None),
    (16448, dict(agents=0, fused_lds=1), "k_step_pipe<lds,1emit>", 257, 2, None),
    (200, dict(agents=0), "k_step_pipe<lds,2emit,predraw>", 4, 4, None),
    (200, dict(mode=MASKED), "k_step_pipe<lds,2emit,predraw>", 4, 4, None),
    (200, dict(mode=HEURISTIC), "k_step_pipe<lds,2emit,predraw>", 4, 4, None),
    (16384, dict(mode=MASKED), "k_step_pipe<lds,2emit,predraw>", 256, 4, None),
    (16385, dict(mode=MASKED), "k_step_pipe<1emit>", 257, 2, None),
    (200, dict(predraw=0), "k_step_pipe<lds,2emit>", 4, 3, None),
    (200, dict(autoreset=0), "k_step_pipe<lds,2emit>", 4, 3, None),
    (200, dict(fused_lds=0), "k_step_pipe<2emit>", 4, 3, None),
    (200, dict(pipeline=0), "k_step_many<lds>", 4, 1, None),
    (200, dict(pipeline=0, fused_lds=0), "k_step_many", 4, 1, None),
    (200, dict(full=1), "k_step_many<lds,full>", 4, 1, None),
    (200, dict(full=1, fused_lds=0), "k_step_many<full>", 4, 1, None),
    (16384, dict(full=1), "k_step_many<lds,full>", 256, 1, None),
    (16385, dict(full=1), "k_step_many<full>", 257, 1, None),
]


@pytest.mark.parametrize("n,dev,name,grid,waves,epw", ROWS, ids=[f"{r[0]}-{r[1]}" for r in ROWS])
def test_selected_kernel(select, n, dev, name, grid, waves, epw):
    p = select(n, **dev)
    assert (p["name"], p["grid"], p["waves"]) == (name, grid, waves)
    assert p["family"] == (AG if name == AG_NAME else PIPE if "pipe" in name else MANY)
    assert p["epw"] == (epw if epw else 64)
    assert not p["stall"]
    # the template arguments are the ones the name spells
    if p["family"] != AG:
        assert p["lds"] == ("lds" in name) and p["full"] == ("full" in name) and p["predraw"] == ("predraw" in name)
    if p["family"] == PIPE:
        assert p["nemit"] == (2 if "2emit" in name else 1) and p["waves"] == 1 + p["nemit"] + p["predraw"]


def test_stall_builds(select):
    """test_stall picks the STALL build of k_step_ag (every epw), the one kernel with bounded
    hand-off waits, of nothing else, and changes no name."""
    for n, dev, name, grid, waves, _ in ROWS:
        p = select(n, test_stall=1, **dev)
        assert (p["name"], p["grid"], p["waves"]) == (name, grid, waves)
        assert p["stall"] == (name == AG_NAME), name
    assert {select(n, test_stall=1)["epw"] for n in (4096, 8192, 16384)} == {16, 32, 64}


def test_every_plan_is_a_known_kernel_that_covers_the_envs(select):
    seen = set()
    for n, K, mode, autoreset, full in itertools.product(
            (1, 64, 200, 4096, 4097, 16384, 16385, 32768, 32769, 65536), (1, 63, 64, 1024),
            (UNMASKED, MASKED, HEURISTIC), (0, 1), (0, 1)):
        for lds, pipe, pg, ag, stall in itertools.product((-1, 0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
            opts = dict(fused_lds=lds, pipeline=pipe, predraw=pg, agents=ag, test_stall=stall)
            p = select(n, K=K, mode=mode, autoreset=autoreset, full=full, **opts)
            case = (n, K, mode, autoreset, full, opts)
            assert p["name"] in NAMES, case
            assert p["grid"] * p["epw"] >= n > (p["grid"] - 1) * p["epw"], case
            assert p["epw"] in (16, 32, 64) and (p["family"] == AG or p["epw"] == 64), case
            if p["family"] == AG:
                assert mode == UNMASKED and not full and pipe and ag, case
            seen.add(p["name"])
    assert seen == NAMES
