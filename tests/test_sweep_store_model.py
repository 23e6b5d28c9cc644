"""The early stores of the unrolled stage sweeps' capture registers (csrc/sweep_mfma_map.hpp cap_final /
cap_step, used by mpc_wave.hpp sweep_run), checked on the host: tests/native/sweep_store_model.cpp models
the registers' writes per step under the keep masks for sweeps of 19 steps and of 1, 2, 16, 17 and 18 (the
register boundaries) and asserts that each register is final after the step named and that the stores
issued there write every stage's eight elements once, with the value of the step that owns the stage."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "build", "sweep_store_model")


def test_early_stores_cover_every_stage_once():
    assert os.path.exists(EXE), "run make harness (build()) first"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout
