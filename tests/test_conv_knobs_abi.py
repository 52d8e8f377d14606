"""vae2_conv2d_set_tune, every key: its default, the values it accepts and what it does with a
value outside them (refuse with -1 and keep the setting, or store a fixed substitute).  The
expected values below are literals recorded before the if-chain became a table lookup; the
call returns the previous value on success.  Host code only: runs without a GPU."""
import pytest

from helpers import GOLDEN  # noqa: F401  (puts the package on sys.path via conftest)

X = "x"  # the call returns -1 and leaves the value unchanged
BOOL_ON, BOOL_OFF = (1, 3, 8, 12, 21), (2, 11, 13, 14)

# key: (default, in-range value, value below the range, outcome, value above, outcome)
TABLE = {
    0: (512, 768, -5, 0, None, None),  # >= 0: no value above the range
    4: (4, 6, 2, X, 9, X),
    5: (2, 1, 0, 2, 3, 2),
    6: (2, 1, -1, X, 3, X),
    7: (3, 1, -1, X, 4, X),
    9: (3, 1, -1, 3, 4, 3),
    10: (0, 5, -1, 0, 9, 0),
    15: (1, 2, -1, X, 3, X),
    16: (2, 1, 0, X, 3, X),
    17: (1, 2, 0, X, 3, X),
    18: (1024, 2048, 255, X, 8193, X),
    19: (1024, 256, 255, X, 8193, X),
    20: (0, 65536, -1, X, 65537, X),
}
TABLE.update({k: (1, 0, -1, 1, 2, 1) for k in BOOL_ON})
TABLE.update({k: (0, 1, -7, 1, 5, 1) for k in BOOL_OFF})


def _lib():
    from vae2 import _lib
    return _lib.load()


def test_table_covers_every_key():
    assert sorted(TABLE) == list(range(22))


@pytest.mark.parametrize("key", sorted(TABLE))
def test_knob_default_range_and_out_of_range_policy(key):
    lib = _lib()
    default, good, below, below_out, above, above_out = TABLE[key]
    try:
        # the default is what a valid set returns; the in-range value is then stored
        assert lib.vae2_conv2d_set_tune(key, good) == default
        assert lib.vae2_conv2d_set_tune(key, good) == good
        for bad, outcome in ((below, below_out), (above, above_out)):
            if bad is None:
                continue
            rc = lib.vae2_conv2d_set_tune(key, bad)
            if outcome == X:
                assert rc == -1, (key, bad)
                assert lib.vae2_conv2d_set_tune(key, good) == good  # unchanged
            else:
                assert rc == good, (key, bad)  # accepted: the previous value comes back
                assert lib.vae2_conv2d_set_tune(key, good) == outcome, (key, bad)
    finally:
        lib.vae2_conv2d_set_tune(key, default)
    assert lib.vae2_conv2d_set_tune(key, default) == default


@pytest.mark.parametrize("key", [22, 23, -1])
def test_unknown_key_is_refused(key):
    lib = _lib()
    for value in (0, 1):
        assert lib.vae2_conv2d_set_tune(key, value) == -1
