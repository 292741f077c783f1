"""The C++ shim's RandomNumberGenerator (shim/bundle_adjuster_hip.h) against a real std::mt19937, and RansacParameters::rng
mapping the batch front ends onto theia_hip_ransac_estimate_streams (shim/rng_streams_test.cc)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "shim", "_build", "rng_streams_test")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "shim")])
    assert os.path.exists(EXE)


def test_shim_generator_state_matches_std_mt19937():
    _build()
    r = subprocess.run([EXE, "--host-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok generator state against std::mt19937" in r.stdout


@pytest.mark.gpu
def test_shim_estimates_on_a_shared_generator():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok relative pose on a shared generator" in r.stdout, r.stdout
