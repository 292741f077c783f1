"""CPU: the host algorithms of the RANSAC driver (csrc/ransac_rng.h: generator, sample streams of a round, acceptance replay)
as a stand-alone program."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ransac_host_algorithms(tmp_path):
    """tests/ransac_host_check.cpp: Mt19937 against std::mt19937 and the std:: distributions bit for bit (seeds 0, 42, 5489,
    0xffffffff, 2000 draws each); the round function against a restatement of RandomSampler on the real engine, the PROSAC
    and EXHAUSTIVE rules and the streams accounting for every K of a round (also across a regeneration and in P4Pfr mode);
    the replay function on three hand-written problems against constants derived from sample_consensus_estimator.h:330-394.
    The header compiles with no HIP on the include path; exit status 0 = everything agrees."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "ransac_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pytheiasfm_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "ransac_host_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], timeout=60, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
