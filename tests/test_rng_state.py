"""CPU: the caller-owned generator state of the streams entry point (theia_rng_state, include/theia_hip.h) and its host-only
functions, against the real libstdc++ (stored draws, and a freshly compiled std::mt19937 when g++ is present), numpy's
MT19937 state, and the Python restatement tests/numpy_routes.LibstdcxxStream."""
import ctypes as C
import json
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ransac
from tests import numpy_routes as nr

HERE = os.path.dirname(os.path.abspath(__file__))


def _L():
    return ransac._sig()


def _seeded(seed):
    st = capi.RngState()
    capi.check(_L().theia_hip_rng_seed(C.byref(st), seed))
    return st


def _rand_int(st, lo, hi, n=1):
    out = np.zeros(max(n, 1), dtype=np.int32)
    capi.check(_L().theia_hip_rng_rand_int(C.byref(st), lo, hi, n, capi.ptr(out, C.c_int32)))
    return out[:n]


def _rand_double(st, lo, hi, n=1):
    out = np.zeros(max(n, 1))
    capi.check(_L().theia_hip_rng_rand_double(C.byref(st), lo, hi, n, capi.ptr(out, C.c_double)))
    return out[:n]


def _snapshot(st):
    return bytes(memoryview(st))


def test_layout():
    assert C.sizeof(capi.RngState) == 624 * 4 + 4 + 4 + 8
    assert capi.RngState.pos.offset == 2496 and capi.RngState.dls_calls.offset == 2504
    assert C.sizeof(capi.RansacStreams) == 3 * 8


def test_seed_matches_std_mt19937_seeding():
    st = _seeded(5489)
    rs = np.random.RandomState(5489)
    key, pos = rs.get_state(legacy=True)[1:3]
    assert np.array_equal(np.array(st.mt[:], dtype=np.uint32), key) and st.pos == pos == 624
    # Seed() resets mt and pos only: the P4Pfr flag and the DLS count stay
    st.p4pfr_static_seeded = 1; st.dls_calls = 17
    _rand_int(st, 0, 9, 5)
    capi.check(_L().theia_hip_rng_seed(C.byref(st), 5489))
    assert np.array_equal(np.array(st.mt[:], dtype=np.uint32), key) and st.pos == 624
    assert st.p4pfr_static_seeded == 1 and st.dls_calls == 17


def test_rand_int_matches_libstdcxx_golden():
    g = json.load(open(os.path.join(HERE, "golden", "mt19937_randint.json")))
    ri = np.array(g["randint"], dtype=np.int64)
    for seed in np.unique(ri[:, 0]):
        rows = ri[ri[:, 0] == seed]
        st = _seeded(int(seed))
        got = [int(_rand_int(st, int(lo), int(hi))[0]) for _, lo, hi, _ in rows]
        assert got == rows[:, 3].tolist()
    # the RandomSampler streams of the same file: the partial shuffle on one continuing state
    for c in g["sampler"]:
        st = _seeded(c["seed"])
        idx = list(range(c["N"]))
        out = []
        for _ in range(64):
            for i in range(c["m"]):
                j = int(_rand_int(st, i, c["N"] - 1)[0])
                idx[i], idx[j] = idx[j], idx[i]
                out.append(idx[i])
        assert out == c["samples"]


def test_rand_double_matches_libstdcxx_golden():
    g = json.load(open(os.path.join(HERE, "golden", "mt19937_randdouble.json")))
    rows = g["randdouble"]
    for seed in sorted({r[0] for r in rows}):
        st = _seeded(seed)
        for _, lo, hi, v in (r for r in rows if r[0] == seed):
            assert _rand_double(st, lo, hi)[0] == v
    # RandInt and RandDouble interleaved on one generator: RandInt(i, n - 1) for i < 4, then three RandDouble
    for key, first_call in (("interleaved", False), ("interleaved_first_call", True)):
        c = g[key]
        st = _seeded(c["seed"])
        for it, row in enumerate(c["rounds"]):
            assert [int(_rand_int(st, i, c["n"] - 1)[0]) for i in range(4)] == row[:4]
            if first_call and it == 0:
                capi.check(_L().theia_hip_rng_seed(C.byref(st), 42))
            assert _rand_double(st, -0.5, 0.5, 3).tolist() == row[4:]


def test_discard_equals_drawing():
    for words in (0, 1, 623, 624, 625, 5000):
        a, b = _seeded(11), _seeded(11)
        capi.check(_L().theia_hip_rng_discard(C.byref(a), words))
        s = nr.LibstdcxxStream(11)
        for _ in range(words):
            s.next()
        key, pos = s.rs.get_state(legacy=True)[1:3]
        assert np.array_equal(np.array(a.mt[:], dtype=np.uint32), key) and a.pos == pos
        _rand_int(b, -2 ** 31, 2 ** 31 - 1, words)   # the full range takes exactly one word per draw
        assert _snapshot(a) == _snapshot(b)


@pytest.mark.parametrize("case", range(6))
def test_mid_stream_states_round_trip_with_numpy(case):
    r = np.random.default_rng(100 + case)
    seed = int(r.integers(0, 2 ** 32))
    g = ransac.RandomNumberGenerator(seed)
    s = nr.LibstdcxxStream(seed)
    for _ in range(int(r.integers(0, 1500))):       # mixed draws, Lemire rejections included (wide ranges)
        if r.random() < 0.5:
            lo = int(r.integers(-10, 10)); hi = lo + int(r.choice([1, 7, 1999, 2 ** 31 - 20]))
            assert g.RandInt(lo, hi) == s.rand_int(lo, hi)
        else:
            assert g.RandDouble(-0.5, 2.0) == s.rand_double(-0.5, 2.0)
    # our state -> numpy: equal keys and pos, and the next draws agree
    name, key, pos, has_gauss, cached = g.get_state()
    ref = s.rs.get_state(legacy=True)
    assert name == "MT19937" and np.array_equal(key, ref[1]) and pos == ref[2]
    t = nr.LibstdcxxStream(0)
    t.rs.set_state(g.get_state())
    assert [t.rand_int(0, 999) for _ in range(700)] == [g.RandInt(0, 999) for _ in range(700)]
    # numpy -> our state, after numpy moved on by itself
    s.rs.bytes(4 * int(r.integers(1, 900)))
    g.set_state(s.rs)
    assert [g.RandDouble(-1.0, 1.0) for _ in range(400)] == [s.rand_double(-1.0, 1.0) for _ in range(400)]


def test_generators_of_one_thread_share_state_threads_do_not():
    a = ransac.RandomNumberGenerator(3)
    b = ransac.RandomNumberGenerator()      # clock-seeded constructor: re-seeds the shared generator ...
    b.Seed(3)                               # ... which Seed() puts back
    s = nr.LibstdcxxStream(3)
    assert [a.RandInt(0, 99), b.RandInt(0, 99), a.RandInt(0, 99)] == [s.rand_int(0, 99) for _ in range(3)]
    other = {}

    def worker():
        g = ransac.RandomNumberGenerator.thread_state()
        other["fresh"] = (np.array(g.mt[:], dtype=np.uint32), g.pos)   # a new thread's generator: std::mt19937 default-constructed
        ransac.RandomNumberGenerator(77).RandInt(0, 9)

    th = threading.Thread(target=worker)
    th.start(); th.join()
    key, pos = np.random.RandomState(5489).get_state(legacy=True)[1:3]
    assert np.array_equal(other["fresh"][0], key) and other["fresh"][1] == pos
    assert a.RandInt(0, 99) == s.rand_int(0, 99)   # untouched by the other thread


def test_argument_errors_leave_state_untouched():
    L = _L()
    st = _seeded(9)
    _rand_int(st, 0, 9, 3)
    before = _snapshot(st)
    out = np.zeros(4, dtype=np.int32); outd = np.zeros(4)
    assert L.theia_hip_rng_rand_int(C.byref(st), 5, 4, 4, capi.ptr(out, C.c_int32)) != 0          # lo > hi
    assert L.theia_hip_rng_rand_int(C.byref(st), 0, 4, -1, capi.ptr(out, C.c_int32)) != 0         # n < 0
    assert L.theia_hip_rng_rand_int(C.byref(st), 0, 4, 4, None) != 0                              # no output
    assert L.theia_hip_rng_rand_double(C.byref(st), 1.0, 0.0, 4, capi.ptr(outd, C.c_double)) != 0
    assert L.theia_hip_rng_rand_double(C.byref(st), float("nan"), 1.0, 4, capi.ptr(outd, C.c_double)) != 0
    assert _snapshot(st) == before
    assert L.theia_hip_rng_seed(None, 1) != 0 and L.theia_hip_rng_discard(None, 3) != 0
    for bad in (-1, 625):
        st.pos = bad
        bad_bytes = _snapshot(st)
        assert L.theia_hip_rng_rand_int(C.byref(st), 0, 4, 4, capi.ptr(out, C.c_int32)) != 0
        assert L.theia_hip_rng_rand_double(C.byref(st), 0.0, 1.0, 4, capi.ptr(outd, C.c_double)) != 0
        assert L.theia_hip_rng_discard(C.byref(st), 10) != 0
        assert _snapshot(st) == bad_bytes
    with pytest.raises(capi.TheiaHipError):
        ransac.RandomNumberGenerator(1).set_state(("MT19937", np.zeros(624, dtype=np.uint32), 700, 0, 0.0))


def test_streams_entry_argument_errors_write_nothing():
    """Checked before any device work: a stream id out of range, pos outside [0, 624], NULL states, seeds given."""
    data = np.random.default_rng(0).standard_normal((60, 4))
    offsets = np.array([0, 20, 40, 60], dtype=np.int64)
    rp = ransac.RansacParameters(); rp.error_thresh = 1e-4; rp.min_iterations = rp.max_iterations = 8

    def attempt(states, sop, seeds=None):
        before = [_snapshot(s) for s in states]
        with pytest.raises(capi.TheiaHipError):
            ransac.estimate_batch(ransac.EST_RELATIVE_POSE, data, offsets, rp, streams=(states, sop), seeds=seeds) if seeds is None else \
                _raw_with_seeds(states, data, offsets, rp)
        assert [_snapshot(s) for s in states] == before

    states = ransac.rng_states(2, [1, 2])
    attempt(states, [0, 2, 1])
    attempt(states, [0, -1, 1])
    bad = ransac.rng_states(2, [1, 2]); bad[1].pos = 625
    attempt(bad, [0, 1, 0])
    bad[1].pos = -3
    attempt(bad, None)
    attempt(states, None, seeds=[1, 2, 3])
    # NULL states / no streams at all
    L = _L()
    b = capi.RansacBatch(); b.estimator = ransac.EST_RELATIVE_POSE; b.num_problems = 3
    b.offsets = capi.ptr(offsets, C.c_int64); b.data = capi.ptr(np.ascontiguousarray(data), C.c_double)
    sv = capi.RansacStreams(); sv.num_streams = 1
    r = capi.RansacResult()
    assert L.theia_hip_ransac_estimate_streams(C.byref(b), C.byref(rp.to_c()), C.byref(sv), C.byref(r)) != 0
    assert L.theia_hip_ransac_estimate_streams(C.byref(b), C.byref(rp.to_c()), None, C.byref(r)) != 0


def _raw_with_seeds(states, data, offsets, rp):
    """The streams call with batch->seeds set (the Python wrapper refuses the combination itself)."""
    L = _L()
    seeds = np.array([1, 2, 3], dtype=np.uint32)
    b = capi.RansacBatch(); b.estimator = ransac.EST_RELATIVE_POSE; b.num_problems = 3
    b.offsets = capi.ptr(offsets, C.c_int64); b.data = capi.ptr(np.ascontiguousarray(data), C.c_double)
    b.seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint32))
    sv = capi.RansacStreams(); sv.num_streams = len(states); sv.states = C.cast(states, C.POINTER(capi.RngState))
    P = 3
    arrs = [np.zeros(P, dtype=np.int32), np.zeros((P, capi.THEIA_RANSAC_MODEL_STRIDE)), np.zeros(P, dtype=np.int32),
            np.zeros(60, dtype=np.uint8), np.zeros(P, dtype=np.int32), np.zeros(P)]
    r = capi.RansacResult()
    r.success = capi.ptr(arrs[0], C.c_int32); r.models = capi.ptr(arrs[1], C.c_double); r.num_inliers = capi.ptr(arrs[2], C.c_int32)
    r.inlier_mask = capi.ptr(arrs[3], C.c_uint8); r.num_iterations = capi.ptr(arrs[4], C.c_int32); r.confidence = capi.ptr(arrs[5], C.c_double)
    capi.check(L.theia_hip_ransac_estimate_streams(C.byref(b), C.byref(rp.to_c()), C.byref(sv), C.byref(r)))


_CXX = r"""
#include <iostream>
#include <random>
#include <sstream>
int main(int argc, char** argv) {
  std::mt19937 g(std::stoul(argv[1]));
  const int k = std::stoi(argv[2]);
  for (int i = 0; i < k; ++i) { std::uniform_int_distribution<int> d(0, 2000000000); (void)d(g); }
  std::cout << g << "\n";
  std::string line; std::getline(std::cin, line);   // a state written by the library: load it, draw three RandInt(0, 999)
  std::istringstream in(line); std::mt19937 h; in >> h;
  for (int i = 0; i < 3; ++i) { std::uniform_int_distribution<int> d(0, 999); std::cout << d(h) << (i < 2 ? " " : "\n"); }
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ for a real std::mt19937")
def test_state_matches_std_mt19937_operator_stream(tmp_path):
    src = tmp_path / "mt_state.cpp"; exe = tmp_path / "mt_state"
    src.write_text(_CXX)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", str(exe), str(src)])
    for seed, k in ((1, 0), (65, 5), (4242, 623), (7, 624), (99, 3001)):
        st = _seeded(seed)
        _rand_int(st, 0, 2000000000, k)
        mine = " ".join(str(v) for v in st.mt[:]) + f" {st.pos}"
        # hand the library's state to std::mt19937 after three more words were skipped, and compare the draws
        nxt = _seeded(seed); _rand_int(nxt, 0, 2000000000, k)
        capi.check(_L().theia_hip_rng_discard(C.byref(nxt), 3))
        line = " ".join(str(v) for v in nxt.mt[:]) + f" {nxt.pos}"
        out = subprocess.run([str(exe), str(seed), str(k)], input=line + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert out[0].strip() == mine
        assert [int(v) for v in out[1].split()] == _rand_int(nxt, 0, 999, 3).tolist()
