"""Self-test of parity_util.status_parity on synthetic status streams: the faults it exists to
catch (a bit set late, never, leaked across a reset, dropped inside an episode) must fail it, and
the legitimate stream around a raise of the reference must pass."""
import numpy as np
import pytest

from tests import parity_util as P


def _rec(status, ended=None):
    status = np.asarray(status, np.uint32).reshape(-1, 1)
    e = np.zeros(len(status), np.uint8) if ended is None else np.asarray(ended, np.uint8)
    return {"status": status, "term": np.zeros_like(e).reshape(-1, 1), "trunc": e.reshape(-1, 1)}


def _run(got, want, got_ended=None, want_ended=None):
    ge = None if got_ended is None else np.asarray(got_ended, bool).reshape(-1, 1)
    return P.status_parity(np.asarray(got, np.uint32).reshape(-1, 1), _rec(want, want_ended), "synthetic", got_ended=ge)


RAISE = [0, 0, 1, 1, 1, 1, 1, 1]            # a bare ST_EXCEPTION: the oracle's env is frozen from step 2
END = [0, 0, 0, 0, 1, 0, 0, 0]              # the kernel's env truncates at step 4 and resets


@pytest.mark.parametrize("with_ended", [False, True])
def test_raise_of_the_reference(with_ended):
    ended = END if with_ended else None
    r = _run([0, 0, 1, 1, 1, 0, 0, 0], RAISE, ended)            # flagged to its episode's end, then clean
    assert r["flagged"] == 6 and r["comparable"] == 2
    for got in ([0] * 8,                                        # never flags
                [0, 0, 0, 1, 1, 0, 0, 0],                       # flags a step late
                [0, 1, 1, 1, 1, 0, 0, 0]):                      # flags a step early
        with pytest.raises(AssertionError):
            _run(got, RAISE, ended)
    with pytest.raises(AssertionError):                         # a one-row call at the raise
        _run([0], [1])
    _run([1], [1])


def test_diverged_dropped_inside_an_episode():
    with pytest.raises(AssertionError):
        _run([0, 0, 1, 0, 0, 0, 0, 0], RAISE, END)
    # PKG_WAIT without a raise: the oracle keeps stepping and resets with the kernel
    want, ended = [0, 0, 4, 4, 4, 0, 0, 0], END
    _run([0, 0, 5, 5, 5, 0, 0, 0], want, ended, ended)
    for got in ([0, 0, 5, 5, 0, 0, 0, 0], [0, 0, 5, 5, 5, 5, 0, 0], [0, 0, 0, 5, 5, 0, 0, 0], [0, 0, 3, 3, 3, 0, 0, 0]):
        with pytest.raises(AssertionError):
            _run(got, want, ended, ended)


def test_reference_behaviour_bits():
    want, ended = [0, 8, 8, 0x18, 0x18, 0, 0x20, 0x20], END
    r = _run(want, want, ended, ended)
    assert r["counts"] == {"TRAY_LOST": 4, "PROD_LOST": 2, "OVERWRITE": 2} and r["excluded"] == 0.0
    for got in ([0, 0, 8, 0x18, 0x18, 0, 0x20, 0x20],           # a step late
                [0, 8, 8, 0x18, 0, 0, 0x20, 0x20],              # dropped on the episode-ending step
                [0, 8, 8, 0x18, 0x18, 0x18, 0x20, 0x20],        # leaked across the reset
                [0, 8, 8, 8, 8, 0, 0x20, 0x20],                 # one bit never set
                [0, 8, 8, 0x18, 0x18, 0, 0x60, 0x60],           # SLOT_OVERFLOW
                [0, 8, 8, 0x18, 0x18, 0, 0x22, 0x20]):          # a stray reason bit without DIVERGED
        with pytest.raises(AssertionError):
            _run(got, want, ended, ended)
