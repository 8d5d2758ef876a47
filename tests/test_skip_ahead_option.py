"""PWG_OPT_SKIP_AHEAD through the C ABI, host only: default 1, set / get round trip, refusal of
other values, and that it leaves PWG_OPT_FRAGMENT_AHEAD alone."""

import ctypes

from parallelwavegan_amd import _lib, configs
from parallelwavegan_amd.engine import HostHandle


def test_skip_ahead_option_round_trip_and_validate(built_lib):
    h = HostHandle(configs.generator_params("libritts_v1"))
    v = ctypes.c_longlong(-1)
    _lib.check(built_lib.pwg_get_option(h._h, _lib.PWG_OPT_SKIP_AHEAD, ctypes.byref(v)))
    assert v.value == 1
    for val in (0, 1):
        _lib.check(built_lib.pwg_set_option(h._h, _lib.PWG_OPT_SKIP_AHEAD, val))
        _lib.check(built_lib.pwg_get_option(h._h, _lib.PWG_OPT_SKIP_AHEAD, ctypes.byref(v)))
        assert v.value == val
    for val in (2, -1):
        assert built_lib.pwg_set_option(h._h, _lib.PWG_OPT_SKIP_AHEAD, val) == _lib.PWG_ERR_INVALID
    _lib.check(built_lib.pwg_get_option(h._h, _lib.PWG_OPT_SKIP_AHEAD, ctypes.byref(v)))
    assert v.value == 1  # a refused value changes nothing
    _lib.check(built_lib.pwg_get_option(h._h, _lib.PWG_OPT_FRAGMENT_AHEAD, ctypes.byref(v)))
    assert v.value == 1
    assert built_lib.pwg_get_option(h._h, _lib.PWG_OPT_SKIP_AHEAD, None) == _lib.PWG_ERR_INVALID
