"""The planner without a device (include/poismf_hip.h, poismf_hip_debug_plan): which launch -- engine, instance, waves, team -- every row of a
half gets, read from the plan text against the sorted row lengths.  Three properties, for both libraries, the three solvers and k across every
slot count the engines distinguish:

  cover       the launches of a call tile its rows exactly once, in sorted order; rows without nonzeros are rows of the shortest class (16)
              like any other, as finish_half_collect bins them;
  capacity    the instance a launch names holds the launch's longest row (constants read from plan.hpp / row_eval.hpp, formulas here);
  invariance  the part of a launch's name that fixes a row's arithmetic -- its signature -- is a function of the row's length alone: the same
              whichever rows share the row's segment, bin, launch or call.

CPU only: the library is cross-compiled, never run on a device here."""
import functools
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not all(os.path.exists(build.lib_path(f)) for f in (False, True)), reason="the HIP libraries are not built")


def _const(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", text) or re.search(r"#define\s+" + name + r"\s+(\d+)", text)
    return int(m.group(1))


_PLAN = open(os.path.join(ROOT, "poismf_amd", "csrc", "plan.hpp")).read()
_ROW = open(os.path.join(ROOT, "poismf_amd", "csrc", "row_eval.hpp")).read()
WAVE = _const(open(os.path.join(ROOT, "poismf_amd", "csrc", "wave_ops.hpp")).read(), "WAVE")
REG_JG = WAVE // _const(_PLAN, "PMF_REG_G")                                           # nonzeros per tile step
REG_SIZES = [int(x) for x in re.findall(r"X\((\d+)\)", re.search(r"#define PMF_REG_SIZES\(X\)(.*)", _PLAN).group(1))]
LONG_ROW_NNZ, LONG_NW, GT_M = _const(_PLAN, "LONG_ROW_NNZ"), _const(_PLAN, "LONG_NW"), _const(_ROW, "GT_M")
TEAM_NW, TEAM_M_MAX = _const(_ROW, "TEAM_NW"), _const(_ROW, "TEAM_M_MAX")

SPECIAL = [4095, 4096, 4097, 8191, 8192, 8193, 20000, 150000]
LENGTHS = np.array(list(range(0, 2201)) + SPECIAL, dtype=np.uint32)
KS = [1, 7, 20, 33, 50, 64, 100, 200]
DIMF = 24000

_NAME = re.compile(r"half_sweep_(?P<kern>reg|regw|team|lane|lane_team|giant|)_?kernel<(?P<type>float|double),(?P<method>pg|cg|tncg|eval)(?:,(?P<rest>.*))?>$")


@functools.lru_cache(maxsize=None)
def parse(name):
    """a launch name as a dict: engine, and the numbers of its instance"""
    m = _NAME.match(name)
    assert m, name
    d = dict(kern=m.group("kern"), type=m.group("type"), method=m.group("method"))
    rest = m.group("rest") or ""
    for key, val in re.findall(r"\b(KS|V|A|S|NW|M|TX)=(\d+)", rest):
        d[key] = int(val)
    lm = re.search(r"\bL=(\d+)(?:\+(\d+))?", rest)
    if lm:
        d["L"], d["LP"] = int(lm.group(1)), int(lm.group(2) or 0)
    d["small"] = "2/SIMD" in rest
    gm = re.search(r"(resident|streamed) cap=(\d+)", rest)
    if gm:
        d["mode"], d["cap"] = gm.group(1), int(gm.group(2))
    d["engine"] = {"reg": "Reg", "regw": "RegW", "team": "RegTeam", "lane": "Lane", "lane_team": "LaneTeam", "giant": "Giant",
                   "": "LdsLong" if d.get("NW", 1) > 1 else "Lds"}[d["kern"]]
    return d


def rides(method, use_float):
    """plan_half's `ride`: a small bin may join the launch of a larger register instance (the claim: the same bits across instances).
    False for TNCG on floats, where S is then part of a row's signature."""
    return not (method == "tncg" and use_float)


@functools.lru_cache(maxsize=None)
def signature(name, ride):
    """what in a launch's name fixes the arithmetic of its rows"""
    d = parse(name)
    e = d["engine"]
    if e in ("Reg", "RegW"):
        return (e, d.get("NW", 1)) + (() if ride else (d["S"],))
    if e == "RegTeam":
        return (e, d["NW"], d["M"], d["S"])
    if e in ("Lane", "LaneTeam"):
        return (e, d["KS"], d["V"], d.get("A", 0), d["L"], d["LP"], d["NW"], d["small"], d.get("TX", 0), d.get("M", 0))
    if e == "Giant":
        return (e, d["NW"], d["M"], d["cap"])
    return (e, d["NW"], d["mode"], d["cap"])


def capacity(d):
    """nonzeros of one row the named instance holds (None: a streamed kernel, any length)"""
    e = d["engine"]
    if e == "Reg":
        return d["S"] * REG_JG
    if e == "RegW":
        return d["NW"] * d["S"] * REG_JG
    if e == "RegTeam":
        return d["M"] * d["NW"] * d["S"] * REG_JG
    if e == "Lane":
        return d["NW"] * (WAVE * (d["V"] + d["A"] + d["L"]) + d["LP"])
    if e == "LaneTeam":
        return d["M"] * d["NW"] * (WAVE * (d["V"] + d["L"]) + d["LP"])
    if e == "Lds" and d["mode"] == "resident":
        return d["cap"]
    return None


def wave_share(nnz, waves):
    """reg_eval.hpp, my_share: the share of a row one of `waves` waves (NW x M) keeps, whole tile steps"""
    per = -(-nnz // waves)
    return -(-per // REG_JG) * REG_JG


class Call:
    """One half-sweep call: the rows it runs in the order the plan lists them (per segment, longest first), and each launch's rows."""

    def __init__(self, lens, cfg, nseg=1, seg=-1):
        lens = np.asarray(lens, dtype=np.uint32)
        self.plan = api.debug_plan(lens, cfg["k"], DIMF, cfg["method"], cfg["use_float"], nseg=nseg, seg=seg, maxupd=cfg["maxupd"],
                                   w_mult=cfg["w_mult"], num_cu=cfg["num_cu"])
        n = len(lens)
        parts = [np.sort(lens[n * j // nseg:n * (j + 1) // nseg])[::-1] for j in (range(nseg) if seg < 0 else [seg])]
        rows = np.concatenate(parts)
        counts = np.array([c for _, c in self.plan], dtype=np.int64)
        assert (counts > 0).all(), self.plan
        assert counts.sum() == len(rows), (counts.sum(), len(rows), cfg, nseg, seg)     # cover: every called row exactly once
        self.per_launch = np.split(rows, np.cumsum(counts)[:-1])                  # ... in the order of the sort

    def launches(self):
        """(name, the distinct lengths of its rows, longest first) per launch; a launch's rows are one segment's, in sorted order"""
        for (name, _), r in zip(self.plan, self.per_launch):
            assert (r[1:] <= r[:-1]).all(), f"{name}: its rows are not a run of one segment's sorted order"
            yield name, np.unique(r)[::-1]


_SIG = {}


def check_signatures(call, base, ride, what, seen=None):
    """every row of `call` has the signature `base` (an array indexed by length, of indices into _SIG) gives its length"""
    for name, lens in call.launches():
        sig = signature(name, ride)
        bad = lens[base[lens] != _SIG.setdefault(sig, len(_SIG))]
        if len(bad):
            was = [s for s, i in _SIG.items() if i == base[bad[0]]][0]
            raise AssertionError(f"{what}: rows of {bad.min()} .. {bad.max()} nonzeros run as {sig}; a row of {bad[0]} planned with one segment of every length: {was}")
        d = parse(name)
        if seen is not None and d["engine"] in ("Reg", "RegW"):
            seen.setdefault((d["engine"], d.get("NW", 1), d["S"]), np.zeros(len(base), bool))[lens] = True


def baseline(cfg, ride):
    base = np.full(int(LENGTHS.max()) + 1, -1, dtype=np.int64)
    for name, lens in Call(LENGTHS, cfg).launches():
        assert (base[lens] == -1).all()
        base[lens] = _SIG.setdefault(signature(name, ride), len(_SIG))
    return base


def configs():
    for use_float in (False, True):
        for method in ("pg", "cg", "tncg"):
            for k in KS:
                for num_cu in (256, 8):
                    for maxupd in ((1, 10) if method == "pg" else (10,)):
                        for w_mult in ((1.0, 3.0) if method == "pg" else (1.0,)):   # (PG: one update at weight 1 is its single-pass mode)
                            yield dict(use_float=use_float, method=method, k=k, num_cu=num_cu, maxupd=maxupd, w_mult=w_mult)


def cfg_id(c):
    return f"{'f32' if c['use_float'] else 'f64'}-{c['method']}-k{c['k']}-cu{c['num_cu']}-upd{c['maxupd']}-w{c['w_mult']:g}"


CONFIGS = list(configs())


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_launches_cover_the_rows_and_hold_them(cfg):
    wide = cfg["k"] == 200 and not cfg["use_float"]   # a factor row of 1.6 KB: eight private tiles of even 16 nonzeros do not fit a CU's LDS, and
    #                                                   plan_half keeps such rows on the one-wave streamed kernel whatever their length, on purpose
    for nseg, seg in ((1, -1), (3, -1), (3, 1)):
        call = Call(LENGTHS, cfg, nseg, seg)                             # (cover: asserted by Call and launches())
        for name, lens in call.launches():
            longest = int(lens[0])
            d = parse(name)
            assert d["type"] == ("float" if cfg["use_float"] else "double") and d["method"] == cfg["method"]
            if 0 in lens:   # rows without nonzeros: with the rows of the shortest class
                assert 1 in lens and 16 in lens, (name, lens)
            cap = capacity(d)
            assert cap is None or cap >= longest, (name, longest)
            if d["engine"] in ("Reg", "RegW", "RegTeam"):
                waves = d.get("NW", 1) * d.get("M", 1)
                assert d["S"] * REG_JG in REG_SIZES and d.get("NW", 1) in (1, 2, 4, 8), name
                assert max(wave_share(n, waves) for n in lens.tolist()) <= d["S"] * REG_JG, name
            if d["engine"] == "RegTeam":
                assert d["NW"] == TEAM_NW and 2 <= d["M"] <= TEAM_M_MAX, name
            if d["engine"] == "LaneTeam":
                assert d["M"] >= 2 and 2 * d["M"] <= cfg["num_cu"] and longest <= LONG_ROW_NNZ, name
            if d["engine"] == "Giant":
                assert d["M"] == GT_M and d["NW"] == LONG_NW and 2 * GT_M <= cfg["num_cu"] and cfg["method"] == "tncg", name
            if longest > LONG_ROW_NNZ and not wide:                        # rows above LONG_ROW_NNZ nonzeros: never one wave
                assert d["engine"] in ("Giant", "LdsLong") and d["NW"] == LONG_NW, (name, longest)
            if cfg["method"] == "tncg" and d["engine"] == "Lds" and not wide:
                assert d["mode"] == "resident", name                       # TNCG's streamed rows: always the eight-wave kernel


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_a_rows_signature_depends_on_its_length_alone(cfg):
    """Before a call over several segments ran them as passes of their own (plan_call), their bins were planned together and the 32nd team launch
    of a call was refused: on that planner this test failed for TNCG fp64 k = 100 from four segments and for CG fp64 k = 33, 50, 64 at eight, e.g.
        4 segments in one call: rows of 385 .. 1088 nonzeros run as ('LdsLong', 8, 'streamed', 16); a row of 1088 planned with one segment of
        every length: ('LaneTeam', 50, 1, 0, 0, 32, 4, False, 0, 3)
        8 segments in one call: rows of 1921 .. 1984 nonzeros run as ('Lds', 1, 'streamed', 48); a row of 1984 planned with one segment of
        every length: ('RegTeam', 4, 4, 32)"""
    ride = rides(cfg["method"], cfg["use_float"])
    base = baseline(cfg, ride)
    seen = {}   # register instance (engine, NW, S) -> the lengths seen on it
    # every segment holds every length: all segments in one call, and one by one
    for nseg in (1, 2, 4, 5, 8, 13):
        lens = np.tile(LENGTHS, nseg)
        check_signatures(Call(lens, cfg, nseg, -1), base, ride, f"{nseg} segments in one call", seen)
        for j in range(nseg):
            check_signatures(Call(lens, cfg, nseg, j), base, ride, f"segment {j} of {nseg}")
    # every row in a segment of its own
    check_signatures(Call(LENGTHS, cfg, len(LENGTHS), -1), base, ride, "a row alone in its segment", seen)
    for n in (0, 1, 160, 161, 1088, 1089, 8192, 8193, 150000):
        check_signatures(Call([n], cfg), base, ride, "a row alone in its half", seen)
    # random company
    for seed in range(20):
        rng = np.random.default_rng(seed)
        check_signatures(Call(LENGTHS[rng.random(len(LENGTHS)) < rng.uniform(0.05, 0.95)], cfg), base, ride, f"random subset {seed}", seen)
    # 5000 more rows in one class: that bin is then worth a register launch of its own (plan_half: 4096 / 2048 rows), and the shorter
    # bins ride with IT
    for cls in list(range(16, 257, 16)) + list(range(320, 1345, 64)):
        check_signatures(Call(np.concatenate([LENGTHS, np.full(5000, cls - 3, np.uint32)]), cfg), base, ride, f"5000 filler rows of {cls - 3} nonzeros", seen)
    # the register instances a length was seen on: one where S is part of the signature; elsewhere instances that differ in S alone -- the pairs
    # that must agree in bits on the device (tests/test_gpu_invariance.py runs such pairs)
    for (e, nw) in sorted({inst[:2] for inst in seen}):
        steps = sorted(S for e2, nw2, S in seen if (e2, nw2) == (e, nw))
        shared = [(a, b) for a in steps for b in steps if a < b and (seen[e, nw, a] & seen[e, nw, b]).any()]
        assert ride or not shared, (e, nw, shared)
        if shared:
            print(f"{cfg_id(cfg)}: {e} NW={nw}: lengths seen on two instances, (S, S'): {shared}")
    for a in seen:   # and never on two register engines or wave counts
        for b in seen:
            assert a[:2] == b[:2] or not (seen[a] & seen[b]).any(), (a, b)


# ---- the cases of tests/test_gpu_invariance.py: what they claim about the plan, held to the planner here -------------------------------------
def _gpu_cases():
    from tests import test_gpu_invariance as G
    return G


def _shape(name):
    """a launch's engine and instance shape: its signature without the register tile's steps and the LDS tile's capacity"""
    d = parse(name)
    return (d["engine"], d["NW"], d["mode"]) if d["engine"] in ("Lds", "LdsLong") else signature(name, True)


@pytest.mark.parametrize("case", list(_gpu_cases().CASES))
def test_the_gpu_cases_reach_every_engine_and_shape_of_their_k(case):
    G = _gpu_cases()
    method, use_float, k, maxupd, want = G.CASES[case]
    cfg = dict(use_float=use_float, method=method, k=k, num_cu=256, maxupd=maxupd, w_mult=1.0)
    names = [name for name, _ in api.debug_plan(G.case_lengths() + [0], k, G.DIMB, method, use_float, maxupd=maxupd)]
    for frag in want:
        assert any(frag in name for name in names), (frag, names)
    # every engine and instance shape the planner has for rows of 0 .. 2200, 4095 .. 8193, 20000 and 150000 nonzeros at this k
    reachable = {_shape(name) for name, _ in Call(LENGTHS, cfg).plan}
    assert {_shape(name) for name in names} == reachable, reachable ^ {_shape(name) for name in names}
    if not rides(method, use_float):   # S is part of the signature: every tile size
        assert {signature(n, False) for n in names} == {signature(n, False) for n, _ in Call(LENGTHS, cfg).plan}


def test_the_gpu_cases_reach_every_engine():
    G = _gpu_cases()
    engines = set()
    for method, use_float, k, maxupd, _ in G.CASES.values():
        engines |= {parse(name)["engine"] for name, _ in api.debug_plan(G.case_lengths(), k, G.DIMB, method, use_float, maxupd=maxupd)}
    declared = set(re.findall(r"^\s+(\w+),\s+//", re.search(r"enum class Engine \{(.*?)\};", _PLAN, re.S).group(1), re.M))
    assert engines == declared and len(declared) == 8, engines ^ declared
