"""The lane and block maps of the stage recursions on the FP64 matrix instruction
(csrc/sweep_mfma_map.hpp), checked on the host: tests/native/sweep_mfma_model.cpp models the instruction
with the operand layout measured on gfx950 and runs both sweeps against a plain double loop."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "build", "sweep_mfma_model")


def test_model_matches_plain_loop():
    assert os.path.exists(EXE), "run make harness (build()) first"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout
