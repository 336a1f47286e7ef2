"""What the planner names, the dispatcher has -- and nothing more.  The instances of the row kernels are written down once, in the tables of
plan.hpp (PMF_LANE_INSTANCES_F64 / _F32, PMF_TEAM_SHAPES, LANE_TEAM_SHAPE); planner and dispatcher both read them.  Two checks over the matrix of
tests/test_plan_cpu.py (its CONFIGS, and the same for the evaluation-only kernels; its LENGTHS; one segment and three), each under the default
settings, with lane_full_width and with reg_quad_off:

  (a) poismf_hip_debug_plan_missing -- the dispatcher itself, asked to find the kernel of every planned launch without launching it -- lists nothing;
  (b) per precision and solver, the lane shapes and the team shapes the plans name are exactly the rows of the tables: no stray, no dead row.

CPU only: the library is cross-compiled, never run on a device here."""
import contextlib
import os
import re

import pytest

from poismf_amd import api, build
from tests.test_plan_cpu import _PLAN, CONFIGS, DIMF, LENGTHS, parse

pytestmark = pytest.mark.skipif(not all(os.path.exists(build.lib_path(f)) for f in (False, True)), reason="the HIP libraries are not built")

SETTINGS = ("default", "lane_full_width", "reg_quad_off")
ALL_CONFIGS = CONFIGS + [dict(c, method="eval") for c in CONFIGS if c["method"] == "cg"]   # (planned like CG, kernels in a unit of their own)
FOR = {"LANE_PG": {"pg"}, "LANE_CG": {"cg", "eval"}, "LANE_CG_TNCG": {"cg", "eval", "tncg"}}   # plan.hpp, the solvers of a table row


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


@contextlib.contextmanager
def setting(name):
    """the process-wide planning switches, in both libraries; restored on the way out"""
    switch = {"default": None, "lane_full_width": api.lane_full_width, "reg_quad_off": api.reg_quad_off}[name]
    was = {}
    try:
        for use_float in (False, True):
            if switch is not None:
                was[use_float] = switch(use_float, True)
        yield
    finally:
        for use_float, prev in was.items():
            switch(use_float, prev)


def plans(cfg, **kw):
    for nseg in (1, 3):
        yield from api.debug_plan(LENGTHS, cfg["k"], DIMF, cfg["method"], cfg["use_float"], nseg=nseg, maxupd=cfg["maxupd"], w_mult=cfg["w_mult"],
                                  num_cu=cfg["num_cu"], **kw)


@pytest.mark.parametrize("name", SETTINGS)
def test_every_planned_launch_has_a_kernel_instance(name):
    with setting(name):
        for cfg in ALL_CONFIGS:
            missing = list(plans(cfg, missing=True))
            assert missing == [], (name, cfg, missing)


def _table(macro):
    body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*)", _PLAN).group(1)
    return [(f, tuple(int(v) for v in nums.split(",")[1:])) for f, nums in re.findall(r"X\((LANE_\w+)((?:,\s*\d+){9})\)", body)]


def _ints(pattern):
    return tuple(int(v) for v in re.search(pattern, _PLAN).group(1).replace(" ", "").split(","))


@pytest.fixture(scope="module")
def named():
    """(use_float, method) -> the lane shapes (KS, LV, LA, LL, NW, SMALL, LP, TX, KU), team shapes (M, S) and lane-team shapes the plans name"""
    out = {}
    for name in SETTINGS:
        with setting(name):
            for cfg in ALL_CONFIGS:
                lane, team, lane_team = out.setdefault((cfg["use_float"], cfg["method"]), (set(), set(), set()))
                for item, _ in plans(cfg, widths=True):
                    ku = re.search(r"\[KU=(\d+)\]$", item)
                    d = parse(item[:ku.start()] if ku else item)
                    if d["engine"] == "Lane":
                        lane.add((d["KS"], d["V"], d["A"], d["L"], d["NW"], int(d["small"]), d["LP"], d.get("TX", 0), int(ku.group(1)) if ku else 0))
                    elif d["engine"] == "RegTeam":
                        team.add((d["M"], d["S"]))
                    elif d["engine"] == "LaneTeam":
                        lane_team.add((d["KS"], d["V"], d["L"], d["NW"], d["LP"]))
    return out


@pytest.mark.parametrize("use_float", (False, True), ids=("f64", "f32"))
def test_the_tables_hold_what_the_plans_name_and_nothing_else(named, use_float):
    rows = _table("PMF_LANE_INSTANCES_F32" if use_float else "PMF_LANE_INSTANCES_F64")
    assert len(rows) == len(set(rows)) and rows, rows
    teams = {tuple(int(v) for v in t) for t in re.findall(r"X\((\d+), (\d+)\)", re.search(r"#define PMF_TEAM_SHAPES\(X\)(.*)", _PLAN).group(1))}
    lv, la, ll, nw, small, lp = _ints(r"LANE_TEAM_SHAPE = \{([\d, ]+)\}")
    lane_team = (int(re.search(r"LANE_TEAM_KS = (\d+)", _PLAN).group(1)), lv, ll, nw, lp)
    assert teams and la == 0 and small == 0
    for method in ("pg", "cg", "tncg", "eval"):
        got_lane, got_team, got_lane_team = named[use_float, method]
        want = {shape for f, shape in rows if method in FOR[f]}
        assert got_lane == want, (method, "named, no table row:", got_lane - want, "table row no plan names:", want - got_lane)
        # register teams: CG on doubles (and the evaluation-only kernels in its place); lane teams: TNCG on doubles
        assert got_team == (teams if not use_float and method in ("cg", "eval") else set()), (method, got_team ^ teams)
        assert got_lane_team == ({lane_team} if not use_float and method == "tncg" else set()), (method, got_lane_team)
