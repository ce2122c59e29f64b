"""CPU-side checks of the fixed-pass window protocol (include/rqp_abi.h, rqp_set_window_passes): the entry point exists
and validates its arguments before touching a device, the new status has its string, and the pass bound helper
matches the documented formula 1 + ceil(floor(max_iter / check_interval) / 3)."""
import math

import pytest

from reluqp import _cabi


def test_library_exports_set_window_passes():
    lib = _cabi.load()
    assert "rqp_set_window_passes" in _cabi.ABI_SYMBOLS
    assert hasattr(lib, "rqp_set_window_passes")


def test_set_window_passes_argument_checks():
    lib = _cabi.load()
    assert lib.rqp_set_window_passes(None, 4) == -1
    assert lib.rqp_set_window_passes(None, 0) == -1
    assert lib.rqp_set_window_passes(None, -3) == -1


def test_status_string():
    assert _cabi.STATUS_STR[5] == "window_passes_exhausted"


@pytest.mark.parametrize("max_iter,check_interval,want", [
    (4000, 25, 55),          # the defaults
    (0, 25, 1),              # no check: only the pass of an instance that enters outside its window
    (24, 25, 1),
    (25, 25, 2),             # one check
    (75, 25, 2),             # three checks: one re-centred window is left after >= 3 moves
    (100, 25, 3),
    (600, 25, 9),
    (500, 10, 18),
])
def test_window_pass_bound(max_iter, check_interval, want):
    from reluqp.reluqpth import window_pass_bound
    assert window_pass_bound(max_iter, check_interval) == want
    assert want == 1 + math.ceil((max_iter // check_interval) / 3)
