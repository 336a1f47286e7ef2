"""Session.holdout / poismf_hip_session_holdout and poismf_hip_holdout_mark (include/poismf_hip.h section 2f) without a GPU: the header, the
export list, the build unit, the wrapper's refusals before any library call and the threshold it derives from frac."""
import ctypes
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_session_update_cpu import DIMA, stub_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("poismf_hip_session_holdout", "poismf_hip_holdout_mark")


@pytest.mark.parametrize("name", NAMES)
def test_the_entry_points_are_declared_exported_and_built(name):
    build.build()
    with open(os.path.join(ROOT, "include", "poismf_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"POISMF_HIP_API\s+int\s+" + name + r"\s*\(", text)
    assert text.index(" * 2e. ") < text.index(" * 2f. ") < text.index("POISMF_HIP_API int " + name)
    assert name in api.EXPORTED_SYMBOLS
    assert build.UNITS["session_holdout"] == ("session_holdout.hip", []) and "philox.hpp" in build._deps("session_holdout.hip")
    for flavour in (False, True, "r"):
        assert hasattr(ctypes.CDLL(build.lib_path(flavour)), name), flavour


class Recorder:
    """every attribute is a function that records its arguments and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


def recording_session():
    s = stub_session(True)
    s.lib = Recorder()
    return s


@pytest.mark.parametrize("kw", [dict(), dict(frac=-0.1), dict(frac=1.5), dict(frac=float("nan")), dict(n_out=-1), dict(n_out=1.5),
                                dict(n_out=1, min_keep=-1), dict(n_out=1, users=[1, 2, 1]), dict(n_out=1, users=[DIMA]),
                                dict(n_out=1, seed=2 ** 64)], ids=str)
def test_holdout_refuses_before_any_library_call(kw):
    s = recording_session()
    with pytest.raises(ValueError):
        s.holdout(**kw)
    assert s.lib.calls == []


@pytest.mark.parametrize("frac, thresh", [(0, 0), (0.5, 2 ** 31), (1, 2 ** 32), (None, 2 ** 32)])
def test_the_threshold_of_a_fraction(frac, thresh):
    s = recording_session()
    T = s.holdout(n_out=3 if frac is None else None, frac=frac, min_keep=2, seed=2 ** 63 + 5, users=[4, 0])
    assert T.shape == (2, s.dimB) and T.nnz == 0
    (name, args), = s.lib.calls            # the counting call; it found nothing held out, so no second call follows
    assert name == NAMES[0] and args[2:8] == (2, 3 if frac is None else 2 ** 64 - 1, thresh, 2, 2 ** 63 + 5, 0)
    assert args[9] is None and args[10] is None
