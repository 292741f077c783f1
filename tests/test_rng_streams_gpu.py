"""GPU: theia_hip_ransac_estimate_streams -- Estimate() calls that continue one generator per reference thread (include/theia_hip.h).
One problem per stream is the seeded batch; chains are checked against the same problems run one call at a time with the
caller carrying the state, against the Python libstdc++ stream (tests/numpy_routes.LibstdcxxStream) advanced by exactly the
samples the reference takes, and against numpy estimators replaying the loop on that stream."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ransac, synth
from tests import numpy_routes as nr

pytestmark = pytest.mark.gpu

P4PFR_LIMITS = [2000.0, 100.0, -1e-5, -1e-9]
SAMPLE = ransac._SAMPLE_SIZE


def _key(st):
    return np.array(st.mt[:], dtype=np.uint32), int(st.pos)


def _same_state(st, stream):
    key, pos = stream.rs.get_state(legacy=True)[1:3]
    k2, p2 = _key(st)
    return np.array_equal(key, k2) and pos == p2


def _problems(est, rng):
    """Three small problems of estimator `est` (data, offsets, estimator_params, error threshold)."""
    kinds = {0: ("relative", (2e-3) ** 2), 1: ("relative", (2e-3) ** 2), 2: ("absolute", (4e-3) ** 2), 3: ("absolute", (4e-3) ** 2),
             4: ("absolute", (4e-3) ** 2), 5: ("fundamental", 4.0), 6: ("homography", 16.0), 7: ("plane", 0.004),
             8: ("known_orientation", (2e-3) ** 2), 9: ("uncalibrated", 4.0)}
    ep = None
    if est in kinds:
        kind, thr = kinds[est]
        data, offsets, _ = synth.synth_ransac_v1(3, 150, kind, seed=0x57AE0000 + est, inlier_lo=0.5, inlier_hi=0.8)
        if est == 9:
            ep = np.array([1.0, 1e9])
        return data, offsets, ep, thr
    rows = []
    if est == 10:
        data, offsets, truth = synth.synth_ransac_v1(3, 150, "absolute", seed=0x57AE000A, inlier_lo=0.5, inlier_hi=0.7)
        rows = [ransac.RotateCorrespondences(data[offsets[i]:offsets[i + 1]], synth.matrix_to_angle_axis(truth["R"][i])) for i in range(3)]
        thr = (4e-3) ** 2
    elif est == 11:
        from tests import tri_scenes
        for t in range(3):
            cams, feats = tri_scenes.scene(18 + 3 * t, 4, 500 + t, intrinsics=synth.PINHOLE_INTR, spread=0.1, noise=0.3)
            rows.append(ransac.triangulation_observations(cams, feats))
        thr = 4.0
    elif est == 12:
        from tests import radhom_scenes as rh
        f1, f2 = 1200.0, 1300.0
        for pair in range(3):
            n = 120 + 20 * pair
            k1, k2 = -rng.uniform(0.5, 3.0) * 1e-7, -rng.uniform(0.5, 3.0) * 1e-7
            pts = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), np.full(n, 4.0 + 0.2 * pair)])
            R = synth.angle_axis_to_matrix(rng.uniform(-0.15, 0.15, (1, 3)))[0]
            r = rh.rows(pts, R, rng.uniform(-0.5, 0.5, 3), f1, f2, k1, k2, 0.3, rng)
            out = rng.uniform(size=n) < 0.25
            r[out, 2:4] = rng.uniform(-600, 600, (int(out.sum()), 2)); r[out, 6:8] = r[out, 2:4] / f2
            rows.append(r)
        thr = 4.0
    elif est == 13:
        from tests import gdls_scenes as gs
        for r in range(3):
            corr, _ = gs.cameras(4, 60 + 10 * r, seed=70 + r, outlier_frac=0.2, noise=0.5, scale=1.3)
            rows.append(ransac.similarity_correspondence_rows(corr))
        thr = 9.0
    elif est == 14:
        from tests import p4pf_scenes as ps
        for i in range(3):
            rows.append(ps.ransac_scene(rng, 80 + 10 * i, outlier_fraction=0.25)[0])
        thr = 4.0
    elif est == 15:
        from tests import upnp_scenes as us
        for i in range(3):
            q = us.quat_angle_axis(float(rng.uniform(3, 30)), rng.normal(size=3)); t = rng.uniform(-1.5, 1.5, 3)
            rows.append(us.rig_rows(rng, 80 + 10 * i, 2, q, t, outlier_fraction=0.2, pixel_noise=0.3)[0])
        thr = 4.0
    else:
        from tests import p4pfr_scenes as rs
        for i in range(3):
            R = rs.angle_axis(float(rng.uniform(3, 30)), rng.normal(size=3)); t = rng.uniform(-1, 1, 3) * [1.0, 1.0, 0.2]
            rows.append(rs.estimator_scene(rng, R, t, 0.8, 0.5, n=60 + 10 * i))
        thr = 4.0
        ep = np.array(P4PFR_LIMITS + [1.0])
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.concatenate(rows), offsets, ep, thr


def _params(thr, rtype=0, min_it=20, max_it=400, seed=0, use_lo=False):
    p = ransac.RansacParameters(); p.error_thresh = thr; p.failure_probability = 1e-3
    p.min_iterations = min_it; p.max_iterations = max_it; p.seed = seed; p.use_lo = use_lo; p.lo_start_iterations = 5
    pc = p.to_c(); pc.ransac_type = rtype
    return pc


FIELDS = ("success", "models", "num_inliers", "inlier_mask", "num_iterations", "confidence", "num_lo_iterations")


def _assert_same(a, b):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


@pytest.mark.parametrize("est", range(17))
def test_one_problem_per_stream_equals_seeded_batch(est):
    rng = np.random.default_rng(1000 + est)
    data, offsets, ep, thr = _problems(est, rng)
    P = len(offsets) - 1
    pc = _params(thr, seed=300 + est)
    seeded = ransac.estimate_batch(est, data, offsets, pc, ep)
    states = ransac.rng_states(P, [300 + est + i for i in range(P)])
    sep = None if ep is None else ep[:4] if est == 16 else ep      # P4Pfr: the first-call flag comes from the states (0 = not yet)
    res = ransac.estimate_batch(est, data, offsets, pc, sep, streams=(states, np.arange(P)))
    _assert_same(seeded, res)
    assert res["hypotheses_evaluated"] == seeded["hypotheses_evaluated"] and res["models_scored"] == seeded["models_scored"]
    assert (seeded["num_iterations"] > 0).all()
    for i in range(P):
        if est in (3, 13):
            assert states[i].dls_calls == seeded["num_iterations"][i]
        assert states[i].p4pfr_static_seeded == (1 if est == 16 else 0)
    if est not in (3, 13, 16):   # RandomSampler: m RandInt per iteration on a fresh permutation
        for i in range(P):
            s = nr.LibstdcxxStream(300 + est + i)
            _ransac_stream_replay(s, int(offsets[i + 1] - offsets[i]), SAMPLE[est], int(seeded["num_iterations"][i]), 0)
            assert _same_state(states[i], s), i


def _ransac_stream_replay(stream, n, m, iters, rtype):
    """The reference's draws for one Estimate() call on a continuing stream: RandomSampler (a fresh index permutation per call)
    or PROSAC (its sample counter restarting per call); Lemire rejections are counted by LibstdcxxStream itself."""
    if rtype == 1:
        return stream.prosac_samples(n, m, iters)
    idx = list(range(n))
    out = []
    for _ in range(iters):
        for i in range(m):
            j = stream.rand_int(i, n - 1)
            idx[i], idx[j] = idx[j], idx[i]
        out.append(idx[:m])
    return np.array(out, dtype=np.int64).reshape(iters, m)


@pytest.mark.parametrize("leg", ["five_point", "plane", "known_orientation"])
def test_chain_against_numpy_replay_on_one_continuing_stream(leg):
    est, kind, thr = {"five_point": (0, "relative", (2e-3) ** 2), "plane": (7, "plane", 0.004),
                      "known_orientation": (8, "known_orientation", (2e-3) ** 2)}[leg]
    P, N, HY, seed = 5, 200, 60, 4242
    data, offsets, _ = synth.synth_ransac_v1(P, N, kind, seed=0x57AE1000 + est, inlier_lo=0.5, inlier_hi=0.8)
    state = ransac.rng_states(1, [seed])
    res = ransac.estimate_batch(est, data, offsets, _params(thr, min_it=HY, max_it=HY), streams=(state, None))
    stream = nr.LibstdcxxStream(seed)
    m = SAMPLE[est]
    for i in range(P):
        d = data[offsets[i]:offsets[i + 1]]
        samples = _ransac_stream_replay(stream, len(d), m, HY, 0)
        if leg == "five_point":
            x1, x2 = d[:, :2], d[:, 2:4]; x1h = np.c_[x1, np.ones(len(d))]; x2h = np.c_[x2, np.ones(len(d))]
            fit = lambda it, idx: nr.relative_pose_models(x1[idx], x2[idx], nr.five_point)
            err = lambda mdl: nr.relative_pose_errors(mdl, x1h, x2h)
        elif leg == "plane":
            fit = lambda it, idx: nr.plane_from_points(d[idx])
            err = lambda mdl: nr.plane_errors(mdl, d)
        else:
            x1, x2 = d[:, :2], d[:, 2:4]; x1h = np.c_[x1, np.ones(len(d))]; x2h = np.c_[x2, np.ones(len(d))]
            fit = lambda it, idx: nr.two_point_position(x1[idx], x2[idx])
            err = lambda pos: nr.known_orientation_errors(pos, x1h, x2h)
        mask = nr.ransac_replay(samples, fit, err, thr, len(d))
        assert res["num_iterations"][i] == HY
        assert np.array_equal(mask, res["inlier_mask"][offsets[i]:offsets[i + 1]].astype(bool)), f"problem {i}"
    assert _same_state(state[0], stream)


@pytest.mark.parametrize("rtype", [0, 1, 2])
@pytest.mark.parametrize("use_lo", [False, True])
@pytest.mark.parametrize("est,kind,thr", [(2, "absolute", (4e-3) ** 2), (0, "relative", (2e-3) ** 2)])
def test_adaptive_chain_equals_calls_one_by_one(est, kind, thr, rtype, use_lo):
    P, seed = 5, 77 + rtype
    data, offsets, _ = synth.synth_ransac_v1(P, 300, kind, seed=0x57AE2000 + 16 * est + rtype, inlier_lo=0.3, inlier_hi=0.9)
    pc = _params(thr, rtype, min_it=5, max_it=3000, use_lo=use_lo)
    chain = ransac.rng_states(1, [seed])
    res = ransac.estimate_batch(est, data, offsets, pc, streams=(chain, None))
    one = ransac.rng_states(1, [seed])[0]
    stream = nr.LibstdcxxStream(seed)
    for i in range(P):
        sl = slice(offsets[i], offsets[i + 1])
        r1 = ransac.estimate_batch(est, data[sl], np.array([0, sl.stop - sl.start], dtype=np.int64), pc, streams=(one, None))
        for f in FIELDS:
            if f == "inlier_mask":
                assert np.array_equal(r1[f], res[f][sl])
            else:
                assert np.array_equal(r1[f][0], res[f][i], equal_nan=True), (f, i)
        _ransac_stream_replay(stream, sl.stop - sl.start, SAMPLE[est], int(res["num_iterations"][i]), rtype)
        assert _same_state(one, stream), f"after problem {i}"
    assert len(set(res["num_iterations"].tolist())) > 1          # adaptive: the problems stop at different iterations
    assert bytes(memoryview(chain[0])) == bytes(memoryview(one))
    assert _same_state(chain[0], stream)


def test_p4pfr_static_reseed_and_dls_call_count():
    from tests import p4pfr_scenes as rs
    rng = np.random.default_rng(5)
    rows = []
    for i in range(3):
        R = rs.angle_axis(float(rng.uniform(3, 30)), rng.normal(size=3)); t = rng.uniform(-1, 1, 3) * [1.0, 1.0, 0.2]
        rows.append(rs.estimator_scene(rng, R, t, 0.8, 0.5, n=50 + 10 * i))
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    data = np.concatenate(rows)
    pc = _params(4.0, min_it=30, max_it=30)
    for seeded_before in (0, 1):
        st = ransac.rng_states(1, [65])
        st[0].p4pfr_static_seeded = seeded_before
        res = ransac.estimate_batch(16, data, offsets, pc, np.array(P4PFR_LIMITS), streams=(st, None))
        assert st[0].p4pfr_static_seeded == 1
        s = nr.LibstdcxxStream(65)
        for i in range(3):
            s.p4pfr_rounds(int(offsets[i + 1] - offsets[i]), 30, first_call=(i == 0 and not seeded_before))
        assert _same_state(st[0], s)
        # the first problem equals the seeded entry point with the matching first-call flag
        ref = ransac.estimate_batch(16, data[:offsets[1]], offsets[:2], pc, np.array(P4PFR_LIMITS + [1.0 - seeded_before]), seeds=[65])
        assert np.array_equal(ref["inlier_mask"], res["inlier_mask"][:offsets[1]]) and np.array_equal(ref["models"][0], res["models"][0])

    # DLS: call k of a problem uses the Macaulay terms of dls_calls + k; a chain advances dls_calls by num_iterations
    data, offsets, _ = synth.synth_ransac_v1(3, 150, "absolute", seed=0x57AE3000, inlier_lo=0.4, inlier_hi=0.8)
    pc = _params((4e-3) ** 2, min_it=10, max_it=500)
    st = ransac.rng_states(1, [9]); st[0].dls_calls = 5
    res = ransac.estimate_batch(3, data, offsets, pc, streams=(st, None))
    nit = res["num_iterations"]
    assert st[0].dls_calls == 5 + int(nit.sum())
    s = nr.LibstdcxxStream(9)
    for i in range(2):
        _ransac_stream_replay(s, int(offsets[i + 1] - offsets[i]), 3, int(nit[i]), 0)
    single = capi.RngState()
    single.mt[:] = [int(v) for v in s.rs.get_state(legacy=True)[1]]
    single.pos = int(s.rs.get_state(legacy=True)[2]); single.dls_calls = 5 + int(nit[0] + nit[1])
    sl = slice(offsets[2], offsets[3])
    r2 = ransac.estimate_batch(3, data[sl], np.array([0, sl.stop - sl.start], dtype=np.int64), pc, streams=(single, None))
    assert r2["num_iterations"][0] == nit[2]
    assert np.array_equal(r2["inlier_mask"], res["inlier_mask"][sl]) and np.array_equal(r2["models"][0], res["models"][2])
    assert bytes(memoryview(single)) == bytes(memoryview(st[0]))
    # a chain whose DLS count starts elsewhere takes other terms: the count is part of the stream
    st2 = ransac.rng_states(1, [9]); st2[0].dls_calls = 0
    r0 = ransac.estimate_batch(3, data, offsets, pc, streams=(st2, None))
    assert st2[0].dls_calls == int(r0["num_iterations"].sum())


def test_interleaved_streams_equal_each_stream_alone():
    P = 6
    data, offsets, _ = synth.synth_ransac_v1(P, 250, "relative", seed=0x57AE4000, inlier_lo=0.3, inlier_hi=0.9)
    pc = _params((2e-3) ** 2, min_it=5, max_it=2000)
    sop = np.array([0, 1, 0, 1, 1, 0])
    both = ransac.rng_states(2, [11, 12])
    res = ransac.estimate_batch(0, data, offsets, pc, streams=(both, sop))
    for k, seed in ((0, 11), (1, 12)):
        sel = np.flatnonzero(sop == k)
        sub = np.concatenate([data[offsets[i]:offsets[i + 1]] for i in sel])
        off = np.concatenate([[0], np.cumsum([offsets[i + 1] - offsets[i] for i in sel])]).astype(np.int64)
        alone = ransac.rng_states(1, [seed])
        r = ransac.estimate_batch(0, sub, off, pc, streams=(alone, None))
        for j, i in enumerate(sel):
            assert np.array_equal(r["inlier_mask"][off[j]:off[j + 1]], res["inlier_mask"][offsets[i]:offsets[i + 1]])
            for f in ("success", "models", "num_inliers", "num_iterations", "confidence"):
                assert np.array_equal(r[f][j], res[f][i]), (f, i)
        assert bytes(memoryview(alone[0])) == bytes(memoryview(both[k]))


def test_undersized_problem_leaves_its_stream_untouched():
    data, offsets, _ = synth.synth_ransac_v1(2, 200, "relative", seed=0x57AE5000)
    tiny = np.random.default_rng(1).standard_normal((3, 4)) * 0.1
    with_tiny = np.concatenate([data[:offsets[1]], tiny, data[offsets[1]:]])
    off3 = np.array([0, offsets[1], offsets[1] + 3, offsets[2] + 3], dtype=np.int64)
    pc = _params((2e-3) ** 2, min_it=10, max_it=500)
    a = ransac.rng_states(1, [3]); b = ransac.rng_states(1, [3])
    ra = ransac.estimate_batch(0, with_tiny, off3, pc, streams=(a, None))
    rb = ransac.estimate_batch(0, data, offsets, pc, streams=(b, None))
    assert list(ra["success"]) == [1, 0, 1] and ra["num_iterations"][1] == 0 and not ra["inlier_mask"][off3[1]:off3[2]].any()
    assert np.array_equal(ra["models"][[0, 2]], rb["models"])
    assert bytes(memoryview(a[0])) == bytes(memoryview(b[0]))


def test_estimate_wrappers_continue_the_thread_generator():
    data, offsets, _ = synth.synth_ransac_v1(3, 200, "relative", seed=0x57AE6000)
    p = ransac.RansacParameters(); p.error_thresh = (2e-3) ** 2; p.min_iterations = 10; p.failure_probability = 1e-3
    p.rng = ransac.RandomNumberGenerator(21)
    got = [ransac.EstimateRelativePose(p, ransac.RansacType.RANSAC, data[offsets[i]:offsets[i + 1]]) for i in range(3)]
    after = _key(ransac.RandomNumberGenerator.thread_state())
    st = ransac.rng_states(1, [21])
    res = ransac.estimate_batch(0, data, offsets, _params((2e-3) ** 2, min_it=10, max_it=2 ** 31 - 1), streams=(st, None))
    for i, (ok, pose, summ) in enumerate(got):
        assert ok and summ.num_iterations == res["num_iterations"][i]
        assert summ.inliers == np.flatnonzero(res["inlier_mask"][offsets[i]:offsets[i + 1]]).tolist()
        assert np.array_equal(pose.essential_matrix.ravel(), res["models"][i][:9])
    k, pos = _key(st[0])
    assert np.array_equal(after[0], k) and after[1] == pos
    # rng = None keeps the seeded behaviour: every call starts from RandomNumberGenerator(seed)
    p.rng = None; p.seed = 21
    ok, pose, summ = ransac.EstimateRelativePose(p, ransac.RansacType.RANSAC, data[offsets[1]:offsets[2]])
    ref = ransac.estimate_batch(0, data[offsets[1]:offsets[2]], np.array([0, offsets[2] - offsets[1]]), _params((2e-3) ** 2, min_it=10, max_it=2 ** 31 - 1, seed=21))
    assert summ.inliers == np.flatnonzero(ref["inlier_mask"]).tolist()


def test_two_view_info_with_options_rng():
    """EstimateTwoViewInfo with options.rng: successive calls continue the thread's generator (ransac_options.rng =
    options.rng); the first call after Seed(s) is the seeded call."""
    from pytheiasfm_amd import twoview
    data, offsets, _ = synth.synth_ransac_v1(2, 300, "fundamental", seed=0x57AE7000, inlier_lo=0.5, inlier_hi=0.8)
    pr = twoview.CameraIntrinsicsPrior(); pr.image_width = 1000; pr.image_height = 800
    pr.focal_length.is_set = True; pr.focal_length.value = [1000.0]
    pr.principal_point.is_set = True; pr.principal_point.value = [500.0, 400.0]
    o = twoview.EstimateTwoViewInfoOptions(); o.max_sampson_error_pixels = 2.0
    o.rng = ransac.RandomNumberGenerator(8)
    first = twoview.EstimateTwoViewInfo(o, pr, pr, data[:offsets[1]])
    second = twoview.EstimateTwoViewInfo(o, pr, pr, data[offsets[1]:])
    after = _key(ransac.RandomNumberGenerator.thread_state())
    o.rng = None; o.seed = 8
    seeded = twoview.EstimateTwoViewInfoBatch(o, [pr, pr], [pr, pr], [data[:offsets[1]], data[offsets[1]:]])
    assert first[0] and first[2] == seeded[0][2] and np.array_equal(first[1].position_2, seeded[0][1].position_2)
    # the same two estimates as one chained batch of the normalised pairs
    norm = np.concatenate([twoview.NormalizeFeatures(pr, pr, data[:offsets[1]]), twoview.NormalizeFeatures(pr, pr, data[offsets[1]:])])
    t = twoview.ComputeResolutionScaledThreshold(2.0, 1000, 800)
    chain = ransac.rng_states(1, [8])
    r = ransac.estimate_batch(0, norm, offsets, twoview._ransac_params(o, t * t / 1e6), streams=(chain, None))
    assert second[2] == np.flatnonzero(r["inlier_mask"][offsets[1]:]).tolist()
    assert second[1].num_verified_matches == int(r["num_inliers"][1])
    k, pos = _key(chain[0])
    assert np.array_equal(after[0], k) and after[1] == pos
