"""CPU: the numpy restatements of tests/alignment_ref.py on known answers, FindCommonViewsByName, the refusals of
pytheiasfm_amd/alignment.py that fire before the library is called, and the ABI additions of the reconstruction-alignment
entry points.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, alignment, ransac, sfm
from tests import alignment_ref as ar
from tests import alignment_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("angle", [0.0, 1.0, np.pi - 5e-4])
def test_planted_similarity_is_recovered_from_exact_data(angle):
    rng = np.random.default_rng(2)
    R, t, s = sc.planted_similarity(rng, angle)
    left = rng.uniform(-5, 5, (50, 3))
    u = ar.umeyama(left, s * left @ R.T + t)
    assert u["status"] == ar.OK and not u["reflected"]
    assert np.abs(u["R"] - R).max() < 1e-12 and np.abs(u["t"] - t).max() < 1e-11 and abs(u["s"] / s - 1) < 1e-12
    assert np.abs(ar.similarity_apply(u["R"], u["t"], u["s"], left) - (s * left @ R.T + t)).max() < 1e-11


def test_planted_reflection_takes_the_negative_branch():
    rng = np.random.default_rng(3)
    R, t, s = sc.planted_similarity(rng, 0.7)
    left = rng.uniform(-5, 5, (40, 3))
    u = ar.umeyama(left, s * left @ (R @ np.diag([1.0, 1.0, -1.0])).T + t)
    assert u["status"] == ar.OK and u["reflected"]
    assert abs(np.linalg.det(u["R"]) - 1.0) < 1e-12          # still a rotation
    sv = u["sv"]
    sigma = ((left - left.mean(0)) ** 2).sum(1).mean()
    assert abs(u["s"] - (sv[0] + sv[1] - sv[2]) / sigma) < 1e-12 * u["s"]


def test_collinear_and_coplanar_points_give_the_identity():
    b = sc.umeyama_batch()
    for p, kind in enumerate(sc.UMEYAMA_KINDS):
        u = ar.umeyama(b["left"][p], b["right"][p])
        if kind in ("point", "collinear", "coplanar"):
            assert u["status"] == ar.DEGENERATE and np.array_equal(u["R"], np.eye(3)) and not u["t"].any() and u["s"] == 1.0
    # the rule is on ABSOLUTE singular values: a well-shaped cloud of small extent is "degenerate" too
    rng = np.random.default_rng(4)
    left = rng.uniform(-1, 1, (30, 3))
    assert ar.umeyama(left, left)["status"] == ar.OK
    assert ar.umeyama(1e-5 * left, 1e-5 * left)["status"] == ar.DEGENERATE


def test_a_weight_of_zero_removes_its_point():
    rng = np.random.default_rng(5)
    R, t, s = sc.planted_similarity(rng)
    left = rng.uniform(-5, 5, (20, 3))
    right = s * left @ R.T + t
    right[3] += 100.0; right[11] -= 50.0
    w = rng.uniform(0.5, 2.0, 20); w[[3, 11]] = 0.0
    keep = w > 0
    a, b = ar.umeyama(left, right, w), ar.umeyama(left[keep], right[keep], w[keep])
    assert np.abs(a["R"] - b["R"]).max() < 1e-13 and np.abs(a["t"] - b["t"]).max() < 1e-12 and abs(a["s"] - b["s"]) < 1e-13
    assert np.abs(a["R"] - R).max() < 1e-12


def test_camera_alignment_restatement():
    rng = np.random.default_rng(6)
    rows, inl, (R, t, s) = sc.camera_problem(rng, noise=0.0)
    idx = np.flatnonzero(inl)[:4]
    model = ar.camera_alignment_fit(rows[idx])
    e = ar.camera_alignment_errors(model, rows)
    assert (e[inl] < 1e-20).all() and (e[~inl] > 1.0).all()     # displaced by a unit or more per axis


def test_transform_restatement_orders_and_masks():
    rng = np.random.default_rng(7)
    R, t, s = sc.planted_similarity(rng, 2.0)
    cams = np.hstack([rng.uniform(-5, 5, (6, 3)), rng.uniform(-1, 1, (6, 3))]); pts = np.hstack([rng.uniform(-5, 5, (9, 3)), rng.uniform(0.5, 2, (9, 1))])
    cm = np.array([1, 1, 0, 1, 0, 1], dtype=bool); pm = np.arange(9) % 3 != 0
    co, orient, po = ar.transform(cams, cm, pts, pm, R, t, s)
    assert co[~cm].tobytes() == cams[~cm].tobytes() and po[~pm].tobytes() == pts[~pm].tobytes()
    assert (po[pm, 3] == 1.0).all()
    h = pts[pm, :3] / pts[pm, 3:4]
    assert np.abs(po[pm, :3] - (s * h @ R.T + t)).max() < 1e-13
    x = h[0]
    assert po[pm][0, 1] == s * ((R[1, 0] * x[0] + R[1, 1] * x[1]) + R[1, 2] * x[2]) + t[1]       # the stated order, to the bit
    Rc = np.asarray(ar.rotation_ld(cams[:, 3:6]), dtype=np.float64)
    assert np.abs(np.asarray(orient, dtype=np.float64)[cm] - Rc[cm] @ R.T).max() < 1e-15


# ------------------------------------------------------------------------------------------------ the mirror, before the library
def _rec(names, n=None):
    r = sfm.Reconstruction()
    n = len(names) if n is None else n
    r.cam_ext = np.zeros((n, 6)); r.view_estimated = np.ones(n, dtype=bool)
    r.view_names = names
    return r


def test_find_common_views_by_name():
    a = _rec(["c.jpg", "a.jpg", "x.jpg", "b.jpg"]); b = _rec(["b.jpg", "q.jpg", "c.jpg"])
    assert alignment.FindCommonViewsByName(a, b) == ["c.jpg", "b.jpg"]        # the stated order: reconstruction1's views
    assert alignment.FindCommonViewsByName(b, a) == ["b.jpg", "c.jpg"]
    assert alignment.FindCommonViewsByName(a, _rec(["z.jpg"])) == []
    assert sfm.Reconstruction().view_names is None


def _raises_invalid(fn, *args):
    with pytest.raises(capi.TheiaHipError) as e:
        fn(*args)
    assert e.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT


def test_mirror_refusals_before_the_library(monkeypatch):
    monkeypatch.setattr(capi, "lib", lambda: pytest.fail("the library must not be called"))
    named, unnamed = _rec(["a", "b", "c", "d", "e"]), _rec(None, 5)
    for fn in (alignment.FindCommonViewsByName, alignment.AlignReconstructions):
        _raises_invalid(fn, named, unnamed)
        _raises_invalid(fn, unnamed, named)
    _raises_invalid(alignment.AlignReconstructionsRobust, 0.05, named, unnamed)
    _raises_invalid(alignment.FindCommonViewsByName, named, _rec(["a", "b"], 3))           # one name per view
    _raises_invalid(alignment.AlignReconstructions, named, _rec(["p", "q"]))               # nothing in common
    _raises_invalid(alignment.AlignReconstructionsRobust, 0.05, named, _rec(["a", "b", "c"]))   # fewer than the sample of 4
    pts = np.zeros((4, 3))
    _raises_invalid(alignment.AlignPointCloudsUmeyama, pts, np.zeros((5, 3)))               # CHECK_EQ(left.size(), right.size())
    _raises_invalid(alignment.AlignPointCloudsUmeyamaWithWeights, pts, pts, np.ones(3))    # CHECK_EQ(left.size(), weights.size())
    _raises_invalid(alignment.AlignPointCloudsUmeyama, np.zeros((4, 2)), pts)
    _raises_invalid(alignment.AlignPointCloudsUmeyamaBatch, [pts, pts], [pts])
    _raises_invalid(alignment.TransformReconstruction, named, np.eye(4), np.zeros(3), 1.0)
    _raises_invalid(alignment.TransformReconstruction4, named, np.eye(3))
    assert alignment.AlignPointCloudsUmeyamaBatch([], []) == []
    _raises_invalid(alignment.AlignRotations, np.zeros((3, 3)), np.zeros((2, 3)))           # CHECK_EQ of the two sizes
    _raises_invalid(alignment.AlignOrientations, {1: np.zeros(3), 2: np.zeros(3)}, {1: np.zeros(3)})   # FindOrDie
    _raises_invalid(alignment.AlignOrientations, {}, {1: np.zeros(3)})


# ------------------------------------------------------------------------------------------------ the ABI additions
def _header():
    src = open(os.path.join(ROOT, "include", "theia_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_constants_equal_the_header():
    src = _header()
    value = lambda name: int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, src).group(1))
    assert value("THEIA_EST_CAMERA_ALIGNMENT") == 17 == capi.THEIA_EST_CAMERA_ALIGNMENT == ransac.EST_CAMERA_ALIGNMENT
    assert value("THEIA_ALIGN_OK") == capi.THEIA_ALIGN_OK == ar.OK
    assert value("THEIA_ALIGN_DEGENERATE") == capi.THEIA_ALIGN_DEGENERATE == ar.DEGENERATE
    assert int(re.search(r"#define\s+THEIA_ALIGN_WAVE_MAX_POINTS\s+(\d+)", src).group(1)) == capi.THEIA_ALIGN_WAVE_MAX_POINTS
    assert ransac._SAMPLE_SIZE[ransac.EST_CAMERA_ALIGNMENT] == 4
    # the estimator ids stay dense: the new one follows the last
    ids = sorted(int(v) for v in re.findall(r"\bTHEIA_EST_\w+\s*=\s*(\d+)", src))
    assert ids == list(range(18))


def test_struct_sizes_match_the_header():
    # theia_align_rotations_summary: six int32, five doubles, no padding
    assert ctypes.sizeof(capi.AlignRotationsSummary) == 6 * 4 + 5 * 8
    body = re.search(r"typedef struct theia_align_rotations_summary \{(.*?)\} theia_align_rotations_summary;", _header(), re.S).group(1)
    names = [n.strip() for decl in body.split(";") for n in decl.replace("int32_t", "").replace("double", "").split(",") if n.strip()]
    assert names == [n for n, _ in capi.AlignRotationsSummary._fields_]
    kinds = [("int32_t" if "int32_t" in decl else "double") for decl in body.split(";") for n in decl.split(",") if n.strip()]
    assert kinds == ["int32_t" if t is ctypes.c_int32 else "double" for _, t in capi.AlignRotationsSummary._fields_]
    # the termination codes the summary reports are the NONLINEAR rotation stage's
    src = _header()
    for name, v in (("GRADIENT_TOLERANCE", capi.ROTATION_TERM_GRADIENT_TOLERANCE), ("FUNCTION_TOLERANCE", capi.ROTATION_TERM_FUNCTION_TOLERANCE),
                    ("PARAMETER_TOLERANCE", capi.ROTATION_TERM_PARAMETER_TOLERANCE), ("MAX_ITERATIONS", capi.ROTATION_TERM_MAX_ITERATIONS),
                    ("FAILURE", capi.ROTATION_TERM_FAILURE), ("MIN_RADIUS", capi.ROTATION_TERM_MIN_RADIUS)):
        assert int(re.search(r"THEIA_ROTATION_TERM_%s\s*=\s*(\d+)" % name, src).group(1)) == v


def test_entry_points_are_exported_with_their_signatures():
    lib = capi.lib()
    for name in ("theia_hip_align_point_clouds", "theia_hip_transform_reconstruction", "theia_hip_align_rotations"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(lib.theia_hip_align_rotations.argtypes) == 7
    assert len(lib.theia_hip_align_point_clouds.argtypes) == 10
    assert len(lib.theia_hip_transform_reconstruction.argtypes) == 10
    assert lib.theia_hip_transform_reconstruction.argtypes[8] is ctypes.c_double      # scale travels by value
    for name in ("AlignPointCloudsUmeyama", "AlignPointCloudsUmeyamaWithWeights", "AlignReconstructions",
                 "AlignReconstructionsRobust", "TransformReconstruction", "TransformReconstruction4", "FindCommonViewsByName",
                 "AlignRotations", "AlignOrientations"):
        import pytheiasfm_amd
        assert getattr(pytheiasfm_amd, name) is getattr(alignment, name)
