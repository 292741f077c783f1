"""The shim's GetCovarianceForViews / GetCovarianceForTracks on a problem with variable cameras and variable tracks
(shim/covariance_full_test.cc): the blocks equal the ones theia_hip_ba_covariance_full returns through the C-ABI."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "shim", "_build", "covariance_full_test")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "shim")])
    assert os.path.exists(EXE)


def test_program_builds_and_links_against_the_c_abi():
    _build()
    out = subprocess.check_output(["ldd", EXE]).decode()
    assert "libtheia_hip.so" in out and "not found" not in out.split("libtheia_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_shim_returns_the_coupled_blocks():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok coupled covariances" in r.stdout, r.stdout
