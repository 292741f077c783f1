"""CPU: host_for (csrc/host_team.h), the one parallel-for of the library's host-side loops, as a stand-alone program."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_for_runs_every_part_exactly_once(tmp_path):
    """tests/host_for_check.cpp: a few hundred regions of 1, 3, 64 and 1000 parts with caps 1, 2 and 6 on the team, a region
    entered from a second thread while the team is held (the fallback to threads of its own), and regions in a fork child
    after the parent has used the team; exit status 0 = every part of every region ran exactly once."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "host_for_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "pytheiasfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_for_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], timeout=60, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
