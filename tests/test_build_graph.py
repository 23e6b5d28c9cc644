"""The library's build graph: every module of intent-mpc_amd/csrc is its own translation unit, so an
edit to a peripheral module must not recompile the solver's unit (impc_qp.hip, minutes), and an edit
to the solver's kernel must recompile nothing else.  Asked of make itself with its what-if option
(`make -n -W file`), on the built tree; nothing is built or modified."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intent-mpc_amd", "csrc")
SOLVER = "impc_qp.hip"
MODULES = ["select.hip", "fanout.hip", "predict.hip", "detect.hip", "mpc_build.hip", "reftraj.hip", "comm.hip",
           "replan_state.hip", "replan_run.hip", "cluster.hip"]


def make(*args):
    return subprocess.run(["make", "-C", ROOT, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def built():
    # the dependencies of a unit are what the compiler reported when it was built: the question only
    # means something where this checkout's own build is complete and current
    if make("-q", "lib").returncode != 0:
        pytest.skip("the library is not up to date in this tree (make -q lib)")


def compiled(touched):
    """the csrc files `make lib` would compile if `touched` had just been modified"""
    r = make("-n", "-W", os.path.join(CSRC, touched), "lib")
    assert r.returncode == 0, r.stderr
    units = set()
    for line in r.stdout.splitlines():
        words = line.split()
        if "-c" in words:
            units.update(os.path.basename(w) for w in words if w.startswith(CSRC + os.sep))
    return units


@pytest.mark.parametrize("touched", MODULES + ["cluster.hpp", "detect_gate.hpp", "plan_exec.hpp"])
def test_module_edit_leaves_the_solver_unit(built, touched):
    units = compiled(touched)
    assert SOLVER not in units, units
    if touched.endswith(".hip"):
        assert touched in units, units  # the what-if reached make: the module itself is recompiled


def test_kernel_edit_rebuilds_the_solver_unit_only(built):
    units = compiled("mpc_wave.hpp")
    assert SOLVER in units, units
    assert not units & set(MODULES), units
