"""CPU-side checks of the sampled ranks in one pass (include/poismf_hip.h section 1u): the Python argument checks before any library
call, the library's own refusals (return code 2 comes before any device work, so they need no device) and the scratch bound."""
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_sample_negatives_cpu import NITEMS, NUSERS, K, _NoDeviceSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST = ([0, 1, 3], [4, 2, 7])          # user 0 holds out item 4, user 1 items 2 and 7
# keyword arguments of rank_sampled(users=[0, 1], ...): every one invalid
BAD = {
    "m-zero": dict(test=TEST, m=0),
    "m-above-limit": dict(test=TEST, m=4097),
    "no-held-out-list": dict(test=None, m=3),
    "unsorted-held-out-row": dict(test=([0, 1, 3], [4, 7, 2]), m=3),
    "held-out-item-out-of-range": dict(test=([0, 1, 3], [4, 2, NITEMS]), m=3),
    "unsorted-exclusion-row": dict(test=TEST, m=3, exclude=([0, 2, 4], [1, 2, 9, 7])),
    "all-zero-weights": dict(test=TEST, m=3, item_weight=np.zeros(NITEMS)),
    "nan-weight": dict(test=TEST, m=3, item_weight=np.r_[np.nan, np.ones(NITEMS - 1)]),
    "user-out-of-range": dict(test=TEST, m=3, users=[0, NUSERS]),
    "seed-out-of-range": dict(test=TEST, m=3, seed=2 ** 64),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


@pytest.mark.parametrize("case", sorted(BAD))
def test_wrappers_raise_before_any_library_call(case):
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    for call in (lambda **kw: api.rank_sampled(A, B, **kw), _NoDeviceSession().rank_sampled):
        with pytest.raises(ValueError):
            call(**{"users": [0, 1], **BAD[case]})


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_library_refuses_with_2_before_any_device_work(flavour):
    lib = api.load_library(flavour)
    dt = np.float32 if flavour else np.float64
    A, B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    u, tp, ti, out = np.array([0, 1], np.uint64), np.array(TEST[0], np.uint64), np.array(TEST[1], np.uint64), np.zeros(3, np.uint32)
    p = api._ptr

    def rc(k=K, dimA=NUSERS, dimB=NITEMS, users=u, tp=tp, ti=ti, m=3, weight=None):
        return lib.poismf_hip_rank_sampled(p(A), p(B), k, dimA, dimB, p(users), 2, p(tp), p(ti), m, 7, None, None, weight, p(out), p(out), None, None)

    assert rc(m=0) == rc(m=api.NEG_MAX_M + 1) == rc(dimB=2 ** 24 + 1) == rc(k=(512 if flavour else 256) + 1) == 2
    assert rc(users=np.array([0, NUSERS], np.uint64)) == rc(ti=np.array([4, 7, 2], np.uint64)) == rc(tp=np.array([0, 2, 1], np.uint64)) == 2
    assert rc(weight=p(np.zeros(NITEMS, np.uint32))) == 2
    assert lib.poismf_hip_rank_sampled(p(A), p(B), K, NUSERS, NITEMS, p(u), 2, None, p(ti), 3, 7, None, None, None, p(out), p(out), None, None) == 2
    text = open(os.path.join(ROOT, "include", "poismf_hip.h")).read()
    for n in ("poismf_hip_rank_sampled", "poismf_hip_session_rank_sampled", "poismf_hip_rank_sampled_scratch_bytes"):
        assert n in api.EXPORTED_SYMBOLS and re.search(r"\b" + n + r"\(", text) and getattr(lib, n) is not None


def test_scratch_stays_under_the_budget_and_the_unit_is_built():
    lib = api.load_library(False)
    # (n_users, n_test_cells, m, dimB, k, weighted): the extremes of each, alone and together
    for args in [(1, 0, 1, 1, 1, 0), (10 ** 6, 10 ** 7, 4096, 10 ** 5, 50, 0), (10 ** 9, 10 ** 12, 4096, 2 ** 24, 256, 1), (1, 65536, 1, 2 ** 24, 256, 1)]:
        assert 0 < int(lib.poismf_hip_rank_sampled_scratch_bytes(*args)) <= 256 << 20, args
    assert int(lib.poismf_hip_rank_sampled_scratch_bytes(64, 640, 4096, 1000, 50, 0)) < (1 << 20)   # a small call does not pay for a large one
    assert build.UNITS["rank_sampled"] == ("rank_sampled.hip", [])
