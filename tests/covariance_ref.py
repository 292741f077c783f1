"""Reference values of theia_hip_ba_covariance_full, in numpy, independent of csrc/: the dense Jacobian J of a flat BA
problem from the oracle's Jets (free columns only), the blocks of inv(J'J), and the same blocks through the Schur form

    cov_c = [S^-1]_cc,  S = U - W V^-1 W',
    cov_p = V_p^-1 + V_p^-1 (sum over observations a, b of p: W_ap' [S^-1]_ab W_bp) V_p^-1,  W_ap = J_cam,a' J_pt,a

with H = J'J = [U W; W' V], cameras and free intrinsics first.  Also the scenes the CPU and GPU tests share."""
import numpy as np

from pytheiasfm_amd import synth
from tests import oracle_lib as ol

PINHOLE_FOCAL_RADIAL = [0, 5, 6]      # free parameters of a pinhole group under FOCAL_LENGTH | RADIAL_DISTORTION (0x01 | 0x10)


class Layout:
    """Column ranges of the free parameters in J: cam[c] = (first column, [extrinsics indices]), grp[g] = (first column,
    [intrinsics indices]), pt[q] = first column; the camera and intrinsics columns come first (ncam of them)."""

    def __init__(self, p, pd, free_intr):
        nc, npts = p.cam_ext.shape[0], p.points.shape[0]
        cam_const = np.zeros(nc, np.uint8) if p.cam_const is None else p.cam_const
        pt_const = np.zeros(npts, np.uint8) if p.point_const is None else p.point_const
        seen_c = np.zeros(nc, bool); seen_c[p.obs_cam] = True
        seen_p = np.zeros(npts, bool); seen_p[p.obs_pt] = True
        self.pd, self.cam, self.grp, self.pt = pd, {}, {}, {}
        n = 0
        if free_intr:
            ng = p.intrinsics.shape[0]
            grp_const = np.zeros(ng, np.uint8) if p.group_const is None else p.group_const
            for g in range(ng):
                if not grp_const[g] and seen_c[p.cam_group == g].any():
                    self.grp[g] = (n, list(free_intr)); n += len(free_intr)
        for c in range(nc):
            idx = [q for q in range(6) if not ((cam_const[c] & 1 and q < 3) or (cam_const[c] & 2 and q >= 3))]
            if idx and seen_c[c]:
                self.cam[c] = (n, idx); n += len(idx)
        self.ncam = n
        for q in range(npts):
            if not pt_const[q] and seen_p[q]:
                self.pt[q] = n; n += pd
        self.ncol = n


def dense_jacobian(p, oo, free_intr=None):
    """(J [2 * nobs][ncol], Layout) at the state of p: loss-corrected, unscaled, tangent-space Jets of the oracle."""
    pd = 3 if oo.use_homogeneous_point_parametrization else 4
    if free_intr:
        ok, _, _, jc, jp, ji = ol.evaluate_ex(p, oo)
    else:
        ok, _, _, jc, jp = ol.evaluate(p, oo)
        ji = None
    assert ok == 1
    lay = Layout(p, pd, free_intr)
    nobs = p.obs_uv.shape[0]
    J = np.zeros((2 * nobs, lay.ncol))
    for i in range(nobs):
        c, q = int(p.obs_cam[i]), int(p.obs_pt[i])
        if c in lay.cam:
            o, idx = lay.cam[c]
            J[2 * i:2 * i + 2, o:o + len(idx)] = jc[i][:, idx]
        g = int(p.cam_group[c])
        if g in lay.grp:
            o, idx = lay.grp[g]
            J[2 * i:2 * i + 2, o:o + len(idx)] = ji[i][:, idx]
        if q in lay.pt:
            J[2 * i:2 * i + 2, lay.pt[q]:lay.pt[q] + pd] = jp[i]
    return J, lay


def _pad_cam(block, idx):
    out = np.zeros((6, 6))
    out[np.ix_(idx, idx)] = block
    return out


def blocks_from_dense_inverse(J, lay):
    """({camera: 6 x 6, zero rows / columns at frozen parameters}, {point: d x d}, cond(J'J)) from numpy's dense inverse."""
    H = J.T @ J
    C = np.linalg.inv(H)
    cams = {c: _pad_cam(C[o:o + len(idx), o:o + len(idx)], idx) for c, (o, idx) in lay.cam.items()}
    pts = {q: C[o:o + lay.pd, o:o + lay.pd] for q, o in lay.pt.items()}
    return cams, pts, np.linalg.cond(H)


def blocks_from_schur_form(J, lay):
    """The same blocks through the reduced camera system; also {point: V_p^-1} (what a shortcut without coupling returns)."""
    nc, pd = lay.ncam, lay.pd
    Jc = J[:, :nc]
    U = Jc.T @ Jc
    Vinv, W = {}, {}
    S = U.copy()
    for q, o in lay.pt.items():
        Jp = J[:, o:o + pd]
        Vinv[q] = np.linalg.inv(Jp.T @ Jp)
        W[q] = Jc.T @ Jp                       # = sum over the observations a of q of W_aq, each in its camera's rows
        S -= W[q] @ Vinv[q] @ W[q].T
    Sinv = np.linalg.inv(S)
    cams = {c: _pad_cam(Sinv[o:o + len(idx), o:o + len(idx)], idx) for c, (o, idx) in lay.cam.items()}
    pts = {q: Vinv[q] + Vinv[q] @ (W[q].T @ Sinv @ W[q]) @ Vinv[q] for q in lay.pt}
    return cams, pts, Vinv


def rel_block(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------ scenes
def oracle_options(**kw):
    oo = ol.default_options()
    for k, v in kw.items():
        setattr(oo, k, v)
    return oo


def options(**kw):
    """(device options, oracle options) with the same fields set."""
    from pytheiasfm_amd import ba
    o = ba.default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o, oracle_options(**kw)


def scene_basic(nv=6, nt=40):
    return synth.synth_ba_v1(nv, nt, fix_gauge=True, num_groups=2)


def scene_tile_edge():
    """12 free cameras: n = 72 crosses a 64-tile edge of the factorisation."""
    return synth.synth_ba_v1(14, 80, fix_gauge=True, num_groups=2, seed=0xC0700002)


def scene_robust():
    """Mixed camera models and per-observation sqrt information (Huber loss in the options)."""
    p = synth.synth_ba_v1(8, 60, fix_gauge=True, mixed_models=True, seed=0xC0700003, pixel_noise=1.0)
    rng = np.random.default_rng(3)
    p.obs_sqrt_info = np.ascontiguousarray(rng.uniform(0.5, 2.0, size=p.obs_uv.shape))
    return p


def scene_intrinsics():
    return synth.synth_ba_v1(9, 120, fix_gauge=True, num_groups=2, seed=0xC0700004)


def scene_long_tracks():
    """70 views; 60 short tracks of 8 .. 36 observations, every ninth view of the ring (wide baselines: cond(J'J) stays
    under 1e6; the longer ones span several LDS tiles of k_cov_points); three tracks seen by every view (more than 64
    observations: the long-track path of the linearisation and the pair-tile loop)."""
    from pytheiasfm_amd._capi import FlatProblem
    p, cam_gt, _ = synth.synth_ba_v1(70, 60, fix_gauge=True, num_groups=2, seed=0xC0700005, return_truth=True)
    rng = np.random.default_rng(5)
    X = np.ones((63, 4))
    X[:60, :3] = rng.uniform(-3.0, 3.0, (60, 3))
    X[60:, :3] = [[2.8, 0.3, -2.0], [-1.5, 2.6, 2.2], [-1.4, -2.7, 0.4]]
    oc, op = [], []
    for t in range(60):
        n = 8 + 7 * (t % 5)
        oc += [(7 * t + 9 * j) % 70 for j in range(n)]; op += [t] * n
    for t in range(60, 63):
        oc += list(range(70)); op += [t] * 70
    oc, op = np.array(oc, np.int32), np.array(op, np.int32)
    uv, ok = synth.project(synth.CAM_PINHOLE, p.intrinsics[p.cam_group[oc]], cam_gt[oc], X[op])
    assert ok.all() and (uv[:, 0] > 0).all() and (uv[:, 0] < 1920).all() and (uv[:, 1] > 0).all() and (uv[:, 1] < 1080).all()
    uv = uv + 0.5 * rng.standard_normal(uv.shape)
    X0 = X.copy(); X0[:, :3] += 0.02 * rng.standard_normal((63, 3))
    return FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, X0, uv, oc, op, cam_const=p.cam_const)


def scene_partial_constant():
    """Camera 0 constant, camera 1 with a frozen position (the classic gauge fix), one constant point."""
    p = synth.synth_ba_v1(6, 40, num_groups=2, seed=0xC0700006)
    cc = np.zeros(6, np.uint8); cc[0] = 3; cc[1] = 1
    pc = np.zeros(40, np.uint8); pc[5] = 1
    from pytheiasfm_amd._capi import FlatProblem
    return FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, p.points, p.obs_uv, p.obs_cam, p.obs_pt,
                       cam_const=cc, point_const=pc)


def scene_mirror():
    """BundleAdjustPartialReconstruction with four of ten views free: the flat problem the mirror function solves."""
    from pytheiasfm_amd import sfm
    p = synth.synth_ba_v1(10, 120, seed=0xC0700009, num_groups=2)
    return sfm._flatten(sfm.Reconstruction.from_flat(p), [2, 3, 4, 5], list(range(120)))


HUBER = dict(loss_function_type=1, robust_loss_width=1.5)
FOCAL_RADIAL = dict(intrinsics_to_optimize=0x01 | 0x10)
# name -> (builder, option fields, free intrinsics of the reference's J)
GPU_SCENES = {
    "basic": (scene_basic, {}, None),
    "tile_edge": (scene_tile_edge, {}, None),
    "robust": (scene_robust, HUBER, None),
    "intrinsics": (scene_intrinsics, FOCAL_RADIAL, PINHOLE_FOCAL_RADIAL),
    "long_tracks": (scene_long_tracks, {}, None),
    "partial_constant": (scene_partial_constant, {}, None),
    "mirror": (scene_mirror, {}, None),
}
