"""CPU-side checks of the batched re-rank (include/poismf_hip.h section 1s): the header's constant and symbols, the testing aids (no
HIP call), the Python argument checks before any library call, and the same cases as return code 2 of the C entry point with
nothing written."""
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("poismf_hip_order_include", "poismf_hip_session_order_include", "poismf_hip_order_include_scratch_bytes",
         "poismf_hip_order_include_run", "poismf_hip_order_include_wave_row")
NUSERS, NITEMS, K = 6, 70000, 3
LONG = 65536 + 1      # one above POISMF_HIP_ORDER_MAX_ROW (test_header_constant_and_symbols pins the constant)

# (users, include as (indptr, indices)): every one invalid
BAD = {
    "unsorted-row": ([0, 1], ([0, 2, 4], [1, 2, 9, 7])),
    "item-out-of-range": ([0, 1], ([0, 1, 2], [3, NITEMS])),
    "overlong-row": ([0, 1], ([0, LONG, LONG + 1], np.r_[np.arange(LONG), 5])),
    "user-out-of-range": ([0, NUSERS], ([0, 1, 2], [3, 4])),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_header_constant_and_symbols():
    text = open(os.path.join(ROOT, "include", "poismf_hip.h")).read()
    m = re.search(r"^#define\s+POISMF_HIP_ORDER_MAX_ROW\s+(\d+)", text, re.M)
    assert m and int(m.group(1)) == api.ORDER_MAX_ROW == 65536
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS and re.search(r"\b" + n + r"\(", text)


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_libraries_export_the_symbols_and_the_aids_answer(flavour):
    lib = api.load_library(flavour)
    for n in NAMES:
        assert getattr(lib, n) is not None
    run, wave = int(lib.poismf_hip_order_include_run()), int(lib.poismf_hip_order_include_wave_row())
    assert run >= 2048 and run & (run - 1) == 0 and 64 <= wave < run
    for args in [(1, 0, 1, 1), (4096, 4096 * 1000, 10 ** 5, 50), (10 ** 6, 10 ** 8, 10 ** 5, 50), (10 ** 9, 10 ** 11, 2 ** 31 - 1, 512)]:
        assert 0 < int(lib.poismf_hip_order_include_scratch_bytes(*args)) <= 256 << 20, args
    assert int(lib.poismf_hip_order_include_scratch_bytes(64, 6400, 1000, 50)) < (8 << 20)   # a small call does not pay for a large one


class _NoDeviceSession(api.Session):
    """the Python half of a session, never connected to a device: any library call would fail on the missing handle"""

    def __init__(self):
        self.lib = self.h = None
        self.use_float = True
        self.dimA, self.dimB, self.k = NUSERS, NITEMS, K
        self.shardA, self.shardB = (0, NUSERS), (0, NITEMS)


@pytest.mark.parametrize("case", sorted(BAD))
def test_wrappers_raise_before_any_library_call(case):
    users, incl = BAD[case]
    model = api.PoisMF(k=K, use_float=False)
    model.A, model.B, model.nusers, model.nitems, model.is_fitted = np.ones((NUSERS, K)), np.ones((NITEMS, K)), NUSERS, NITEMS, True
    with pytest.raises(ValueError):
        model.order_candidates(users, incl)
    with pytest.raises(ValueError):
        _NoDeviceSession().order_candidates(users, incl, output_score=True)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, incl = BAD[case]
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64
    A, B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    u, ip, ii = (np.asarray(a, np.int64).astype(it) for a in (users, incl[0], incl[1]))
    out, sc, cnt = np.full(len(ii), 12345, it), np.full(len(ii), -7.0, dt), np.full(len(u), 99, it)
    p = api._ptr
    rc = api.load_library(flavour).poismf_hip_order_include(p(A), p(B), K, NUSERS, NITEMS, p(u), len(u), p(ip), p(ii), None, None, p(out), p(sc),
                                                            p(cnt))
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0) and np.all(cnt == 99)
