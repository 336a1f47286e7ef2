"""poismf_amd/build.py's unit table against csrc/ itself: every source is compiled, every header reaches an object's digest, a unit's
dependency list is the include closure of its file (derived, not a hand list that drifts), and the -DPMF_TIMING build swaps the four
solver units for one.  CPU only: reads the sources, runs no compiler."""
import os
import re

from poismf_amd import build

SOLVER_UNITS = {"poismf_hip_tncg", "poismf_hip_cg", "poismf_hip_pg", "poismf_hip_eval"}


def _csrc(suffix):
    return {name for name in os.listdir(build.CSRC) if name.endswith(suffix)}


def _closure(source):
    """the test's own scan: `source` and every csrc/ file it reaches through #include "name" lines"""
    todo, seen = [source], set()
    while todo:
        name = todo.pop()
        if name in seen or name not in os.listdir(build.CSRC):   # (system headers and ../../include/poismf_hip.h are not csrc/ files)
            continue
        seen.add(name)
        with open(os.path.join(build.CSRC, name)) as fh:
            todo += re.findall(r'#\s*include\s+"([^"]+)"', fh.read())
    return seen


def test_every_hip_file_is_the_compiled_file_of_a_unit():
    assert _csrc(".hip") == {source for source, _ in build.UNITS.values()}


def test_every_header_is_in_some_unit_s_dependency_list():
    reached = {name for source, _ in build.UNITS.values() for name in build._deps(source)}
    assert _csrc(".hpp") - reached == set()


def test_a_unit_s_dependency_list_is_its_include_closure():
    for unit, (source, _) in build.UNITS.items():
        deps = build._deps(source)
        assert deps[0] == source, unit                      # (the first is the one compiled)
        assert len(deps) == len(set(deps)), (unit, deps)
        assert set(deps) == _closure(source), unit
    assert "session.hpp" in build._deps("planner.hip") and "session.hpp" not in build._deps("poismf_hip.hip")


def test_the_timing_build_swaps_the_solver_units_for_one(monkeypatch):
    monkeypatch.delenv("POISMF_HIP_EXTRA_FLAGS", raising=False)
    default = dict(build._units())
    assert default == build.UNITS and SOLVER_UNITS <= set(default)
    monkeypatch.setenv("POISMF_HIP_EXTRA_FLAGS", "-DPMF_TIMING")
    timing = dict(build._units())
    assert set(default) - set(timing) == SOLVER_UNITS
    assert set(timing) - set(default) == {"poismf_hip_all"}
    assert timing["poismf_hip_all"] == ("poismf_hip.hip", [])
    assert all(timing[u] == default[u] for u in set(timing) & set(default))
