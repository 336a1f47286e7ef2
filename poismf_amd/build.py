"""Builds the HIP shared libraries in-tree (poismf_amd/libpoismf_hip_{d,f}.so) with hipcc for gfx950.

    python -m poismf_amd.build [--force] [-v]

Twenty-nine translation units per precision -- the host side in nine (session.hip the session object, planner.hip the planner,
half_sweep.hip issuing a half-sweep, drivers.hip run_poismf / factors_multiple, multi_device.hip the in-process multi-device driver,
session_update.hip the merge of new counts into a resident session and the half-sweep over listed rows, session_remove.hip the removal of counts, cells and whole rows from a resident session, session_grow.hip new rows joining a resident session, session_scale.hip the scaling of every resident count and the removal of what fades -- the four on session_merge.hpp; they share session.hpp), one per inner solver and one for the evaluation-only kernels (the row kernels of PG, CG and TNCG are the bulk
of the compile time; poismf_hip.hip is compiled once for each with -DPMF_TU=...), the rocPRIM-based COO conversion (coo_convert.hip),
the serving kernels (serve.hip), the likelihood (llk.hip), the batched top-N (topn_batch.hip), the batched ranks (rank_batch.hip), the
batched top-N over include lists (topn_include.hip) and over lists shared between users (topn_shared.hip) and the batched ranks among
include lists (rank_include.hip) and among lists shared between users (rank_shared.hip), the deep batched top-N (topn_deep.hip, with
tb_deep.hpp) and the batched top-N with per-group quotas (topn_quota.hip, with tb_quota.hpp) and with per-item score weights (topn_weighted.hip) and with per-(user, item) score factors (topn_adjust.hip: a dense pass on tb_select.hpp, a sparse one on tb_gather.hpp and a merge) and the diversified top-N (topn_diverse.hip: the deep core's chunk loop and an MMR kernel behind it; the eleven share tb_tile.hpp and tb_batch.hpp, topn_batch / topn_shared / topn_quota / topn_weighted / topn_adjust the selection of tb_select.hpp, the three rank units tb_rank.hpp, the two include units, topn_diverse and topn_adjust tb_gather.hpp) and the
new rows against a resident B (fold_in.hip: the guest of a session, on session.hpp and tb_batch.hpp) and the list-wise evaluation
(list_eval.hip, on tb_gather.hpp and tb_batch.hpp) -- are compiled to object files
side by side and linked.  What an object depends on is derived from its file's #include "..." lines (_deps), never listed by hand.
Every object and library carries a `.stamp` with the digest of its command line and sources: an object is rebuilt exactly when that
digest changes (a different POISMF_HIP_EXTRA_FLAGS rebuilds everything it reaches; file times play no part).  A full build takes ~11.5 minutes on 8 cores
(692 s and 717 s; 690 s before the host side was split into five units); after an edit of drivers.hip alone ~50 s (52 s; 57 s for the one host
file before), most of it the three links and the ISA guard.
"""
import fcntl
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HEADER = os.path.join(os.path.dirname(HERE), "include", "poismf_hip.h")
# unit -> (the file compiled, extra flags).  poismf_hip.hip is compiled four times: one translation unit per inner solver
# (its row kernels are the bulk of the compile time); the host side is five files around session.hpp.
UNITS = {
    "session": ("session.hip", []),
    "planner": ("planner.hip", []),
    "half_sweep": ("half_sweep.hip", []),
    "drivers": ("drivers.hip", []),
    "multi_device": ("multi_device.hip", []),
    "session_update": ("session_update.hip", []),
    "session_remove": ("session_remove.hip", []),
    "session_grow": ("session_grow.hip", []),
    "session_scale": ("session_scale.hip", []),
    "poismf_hip_tncg": ("poismf_hip.hip", ["-DPMF_TU=1"]),
    "poismf_hip_cg": ("poismf_hip.hip", ["-DPMF_TU=2"]),
    "poismf_hip_pg": ("poismf_hip.hip", ["-DPMF_TU=3"]),
    "poismf_hip_eval": ("poismf_hip.hip", ["-DPMF_TU=4"]),   # evaluation-only kernels behind poismf_hip_debug_row_eval (testing aid)
    "coo_convert": ("coo_convert.hip", []),
    "serve": ("serve.hip", []),
    "llk": ("llk.hip", []),
    "topn_batch": ("topn_batch.hip", []),
    "rank_batch": ("rank_batch.hip", []),
    "topn_include": ("topn_include.hip", []),
    "topn_shared": ("topn_shared.hip", []),
    "rank_include": ("rank_include.hip", []),
    "rank_shared": ("rank_shared.hip", []),
    "topn_deep": ("topn_deep.hip", []),
    "topn_quota": ("topn_quota.hip", []),
    "topn_weighted": ("topn_weighted.hip", []),
    "topn_diverse": ("topn_diverse.hip", []),
    "topn_adjust": ("topn_adjust.hip", []),
    "fold_in": ("fold_in.hip", []),
    "list_eval": ("list_eval.hip", []),
}
_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"/]+)"', re.M)   # (the includes inside csrc/ are flat quoted names)


def _deps(source):
    """What an object compiled from csrc/`source` is built from: the file and, transitively, every csrc/ header it includes by
    quoted name (the first is the one compiled).  Derived, so that no header can be forgotten and leave a stale object."""
    seen = [source]
    for name in seen:
        with open(os.path.join(CSRC, name)) as fh:
            seen += [inc for inc in dict.fromkeys(_INCLUDE.findall(fh.read())) if inc not in seen and os.path.exists(os.path.join(CSRC, inc))]
    return seen


# flavour -> flags: the reference builds its core twice for Python (ref: setup.py:225-243) and once for R with int indices
# (ref: src/poismf.h:75-89); the R flavour differs on the host side only and links the double flavour's row kernels
FLAVOURS = {"d": [], "f": ["-DUSE_FLOAT"], "r": ["-D_FOR_R"]}
_KERNEL_UNITS = ("poismf_hip_tncg", "poismf_hip_cg", "poismf_hip_pg", "poismf_hip_all")


def _flavour(use_float):
    return use_float if isinstance(use_float, str) else ("f" if use_float else "d")


def lib_path(use_float):
    """use_float: False / True (the two Python flavours) or a flavour name "d" / "f" / "r" """
    return os.path.join(HERE, f"libpoismf_hip_{_flavour(use_float)}.so")


def _obj_path(unit, flavour):
    flavour = _flavour(flavour)
    if flavour == "r" and unit in _KERNEL_UNITS:
        flavour = "d"
    return os.path.join(CSRC, f"{unit}_{flavour}.o")


def _digest(parts, files):
    """sha256 over strings and file contents"""
    h = hashlib.sha256(repr(parts).encode())
    for path in files:
        with open(path, "rb") as fh:
            h.update(os.path.basename(path).encode() + b"\0" + fh.read())
    return h.hexdigest()


def _fresh(out, digest):
    """`out` exists and was produced from exactly the inputs `digest` stands for (sources AND flags: a changed
    POISMF_HIP_EXTRA_FLAGS rebuilds, file times play no part)"""
    try:
        return os.path.exists(out) and open(out + ".stamp").read().strip() == digest
    except OSError:
        return False


def _mark(out, digest):
    with open(out + ".stamp", "w") as fh:
        fh.write(digest + "\n")


STAMP = os.path.join(HERE, ".build_stamp")   # hash of the sources + flags the in-tree libraries were built from


def _units():
    """The -DPMF_TIMING development build keeps its phase timers in one device-side array, so it stays one translation unit."""
    if "-DPMF_TIMING" in os.environ.get("POISMF_HIP_EXTRA_FLAGS", "").split():
        return {**{u: v for u, v in UNITS.items() if "-DPMF_TU=" not in " ".join(v[1])}, "poismf_hip_all": ("poismf_hip.hip", [])}
    return UNITS


def _flags():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function", "-Wno-unused-const-variable",
             "-Wno-pass-failed"]
    return flags + os.environ.get("POISMF_HIP_EXTRA_FLAGS", "").split()   # development: e.g. -DPMF_REG_G=8, -DPMF_TIMING


def _source_hash():
    names = sorted({f for source, _ in _units().values() for f in _deps(source)})
    return _digest([_flags(), sorted((u, f) for u, (_, f) in _units().items())], [os.path.join(CSRC, f) for f in names] + [HEADER])


def up_to_date():
    """The libraries exist and were built from exactly the sources + flags that are here now.  Object files do not
    travel with a snapshot of the tree (and file times do not survive one), so this is what decides whether a process
    on another machine -- or N ranks of one job at once -- may skip the compiler."""
    try:
        return all(os.path.exists(lib_path(f)) for f in FLAVOURS) and open(STAMP).read().strip() == _source_hash()
    except OSError:
        return False


def build(force=False, verbose=False):
    if not force and up_to_date():
        return lib_path(False), lib_path(True)
    with open(os.path.join(HERE, ".build_lock"), "w") as lock:   # one builder at a time (ranks of a multi-GPU job)
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and up_to_date():
            return lib_path(False), lib_path(True)
        # (the hash of what is being built, taken BEFORE the compilers read it: a source edited while they run must not be
        # recorded as built -- it was, once, and the next build() then skipped a stale library)
        building = _source_hash()
        out = _build_locked(force, verbose)
        with open(STAMP, "w") as fh:
            fh.write(building + "\n")
        return out


def _build_locked(force, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _flags()
    if verbose:
        flags.append("-Rpass-analysis=kernel-resource-usage")
    compiles = []
    digests = {}
    for flavour, fl_flags in FLAVOURS.items():
        for unit, (source, unit_flags) in _units().items():
            deps = [os.path.join(CSRC, f) for f in _deps(source)] + [HEADER]
            obj = _obj_path(unit, flavour)
            if obj in digests:
                continue   # the R flavour's row kernels are the double flavour's objects
            cmd = [hipcc] + fl_flags + flags + unit_flags + ["-c", os.path.join(CSRC, source), "-o", obj]
            digests[obj] = _digest(cmd, deps)
            if force or not _fresh(obj, digests[obj]):
                if verbose:
                    print(" ".join(cmd))
                if os.path.exists(obj + ".stamp"):
                    os.remove(obj + ".stamp")
                compiles.append((cmd, obj, subprocess.Popen(cmd)))   # all stale objects compile side by side
    failed = None
    for cmd, obj, p in compiles:
        if p.wait() != 0:
            failed = failed or subprocess.CalledProcessError(p.returncode, cmd)
        else:
            _mark(obj, digests[obj])
    if failed:
        raise failed
    for flavour in FLAVOURS:
        out = lib_path(flavour)
        objs = [_obj_path(u, flavour) for u in _units()]
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
        digest = _digest(cmd + [digests[o] for o in objs], [])
        if force or not _fresh(out, digest):
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            isa_guard(out)           # (before the library is marked as built: a violated invariant leaves it stale)
            _mark(out, digest)
    return lib_path(False), lib_path(True)


def isa_guard(lib):
    """scripts/isa_guard.py on a freshly linked library: the lane-team kernels must reach their cross-CU exchange through a call of the
    out-of-line team_sum_call, and that function must not spill while EXEC may be narrowed.  Raises on a violation;
    says so and goes on where llvm-objdump is missing.  POISMF_HIP_NO_ISA_GUARD=1 skips it (development builds of variants)."""
    if os.environ.get("POISMF_HIP_NO_ISA_GUARD") or "-DPMF_LANE_ONLY" in os.environ.get("POISMF_HIP_EXTRA_FLAGS", ""):
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmf_isa_guard", os.path.join(os.path.dirname(HERE), "scripts", "isa_guard.py"))
    guard = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(guard)
    if not os.path.exists(guard.OBJDUMP):
        print(f"poismf_amd.build: no {guard.OBJDUMP}: ISA guard skipped for {os.path.basename(lib)}", file=sys.stderr)
        return
    lines = []
    if not guard.check_library(lib, lines.append):
        raise RuntimeError("ISA guard violated in " + lib + ":\n" + "\n".join(l for l in lines if ": info: " not in l))


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose="-v" in sys.argv)
