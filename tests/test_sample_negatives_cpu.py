"""CPU-side checks of the negative sampler (include/poismf_hip.h section 1t): the generator against the published Philox4x32-10
known-answer vectors, the Python argument checks before any library call, and the scratch bound.  No device."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUSERS, NITEMS, K = 4, 50, 3
F = 0xFFFFFFFF
KAT = [   # counter, key -> output (Random123's kat_vectors, philox4x32 10 rounds)
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((F, F, F, F), (F, F), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
# keyword arguments of sample_negatives(users=[0, 1], ...): every one invalid
BAD = {
    "m-zero": dict(m=0),
    "m-above-limit": dict(m=4097),
    "unsorted-exclusion-row": dict(m=3, exclude=([0, 2, 4], [1, 2, 9, 7])),
    "negative-weight": dict(m=3, item_weight=np.r_[-1.0, np.ones(NITEMS - 1)]),
    "nan-weight": dict(m=3, item_weight=np.r_[np.nan, np.ones(NITEMS - 1)]),
    "infinite-weight": dict(m=3, item_weight=np.r_[np.inf, np.ones(NITEMS - 1)]),
    "all-zero-weights": dict(m=3, item_weight=np.zeros(NITEMS)),
    "all-zero-integer-weights": dict(m=3, item_weight=np.zeros(NITEMS, np.int64)),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


class _NoDeviceSession(api.Session):
    """the Python half of a session, never connected to a device: any library call would fail on the missing handle"""

    def __init__(self):
        self.lib = self.h = None
        self.use_float = True
        self.dimA, self.dimB, self.k = NUSERS, NITEMS, K
        self.shardA, self.shardB = (0, NUSERS), (0, NITEMS)


def _model(nitems=NITEMS):
    model = api.PoisMF(k=K, use_float=False)
    model.A, model.B, model.nusers, model.nitems, model.is_fitted = np.ones((NUSERS, K)), np.ones((1, K)), NUSERS, nitems, True
    return model


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_philox_known_answers_symbols_and_constant(flavour):
    lib = api.load_library(flavour)
    for ctr, key, want in KAT:
        out = np.zeros(4, np.uint32)
        lib.poismf_hip_philox4x32(api._ptr(np.array(ctr, np.uint32)), api._ptr(np.array(key, np.uint32)), api._ptr(out))
        assert tuple(int(x) for x in out) == want
    text = open(os.path.join(ROOT, "include", "poismf_hip.h")).read()
    assert int(re.search(r"^#define\s+POISMF_HIP_NEG_MAX_M\s+(\d+)", text, re.M).group(1)) == api.NEG_MAX_M == 4096
    for n in ("poismf_hip_sample_negatives", "poismf_hip_session_sample_negatives", "poismf_hip_sample_negatives_scratch_bytes",
              "poismf_hip_philox4x32"):
        assert n in api.EXPORTED_SYMBOLS and re.search(r"\b" + n + r"\(", text) and getattr(lib, n) is not None


@pytest.mark.parametrize("case", sorted(BAD))
def test_wrappers_raise_before_any_library_call(case):
    for call in (lambda **kw: api.sample_negatives(NITEMS, **kw), _model().sample_negatives, _NoDeviceSession().sample_negatives):
        with pytest.raises(ValueError):
            call(users=[0, 1], **BAD[case])


def test_too_many_items_and_negatives_with_include_raise():
    with pytest.raises(ValueError):
        api.sample_negatives(2 ** 24 + 1, [0], 3)
    with pytest.raises(ValueError):
        _model(2 ** 24 + 1).sample_negatives([0], 3)
    X = sp.csr_matrix(([1.0], ([0], [1])), shape=(NUSERS, NITEMS))
    for target in (_model(), _NoDeviceSession()):
        with pytest.raises(ValueError, match="negatives"):
            target.eval_ranking(X, negatives=5, include=X)


def test_scratch_stays_under_the_budget():
    lib = api.load_library(False)
    for args in [(1, 1, 1, 0), (10 ** 6, 4096, 10 ** 5, 0), (10 ** 6, 4096, 2 ** 24, 1), (10 ** 9, 1, 2 ** 24, 1)]:
        assert 0 < int(lib.poismf_hip_sample_negatives_scratch_bytes(*args)) <= 256 << 20, args
    assert int(lib.poismf_hip_sample_negatives_scratch_bytes(64, 100, 1000, 0)) < (1 << 20)   # a small call does not pay for a large one
