"""Scenes of the incremental-step tests (tests/test_incremental_step.py, tests/test_incremental_step_gpu.py)."""
import numpy as np

from pytheiasfm_amd import sfm, synth


class Sweep:
    """Observations and flags of an underconstrained-sweep scene, with the answer worked out by hand."""

    def __init__(self, tracks_of_view, num_tracks, expected=None, view_estimated=None, track_estimated=None):
        self.num_views, self.num_tracks = len(tracks_of_view), num_tracks
        self.obs_view = np.array([v for v, ts in enumerate(tracks_of_view) for _ in ts], dtype=np.int32)
        self.obs_track = np.array([t for ts in tracks_of_view for t in ts], dtype=np.int32)
        self.view_estimated = np.ones(self.num_views, np.uint8) if view_estimated is None else np.array(view_estimated, np.uint8)
        self.track_estimated = np.ones(num_tracks, np.uint8) if track_estimated is None else np.array(track_estimated, np.uint8)
        # (views removed, tracks removed, rounds, view flags after, track flags after)
        self.expected = expected


def stopping_scene():
    """View 0 sees exactly three estimated tracks 0, 1, 2, and no other view sees track 0.  Views 1 and 2 are well
    constrained.  Round 1: the view pass removes nothing (3, 5, 3 tracks), the track pass removes track 0 (one view), and
    `views == 0` ends the loop: view 0 STAYS estimated with two tracks.  A fixed-point loop would go on and remove view 0,
    then tracks 1 and 2."""
    return Sweep([[0, 1, 2], [1, 2, 3, 4, 5], [3, 4, 5]], 6,
                 expected=(0, 1, 1, [1, 1, 1], [0, 1, 1, 1, 1, 1]))


def cascade_scene():
    """Views 0, 1: a stable core on tracks 0..3.  View 2 sees tracks 4, 5 only; view 3 sees 4, 5, 6; view 4 sees 6, 0, 1.
    Round 1: view 2 goes (2 tracks), then tracks 4, 5 (view 3 alone).  Round 2: view 3 goes (track 6 alone), then track 6
    (view 4 alone).  Round 3: view 4 goes (tracks 0, 1), no track goes (0 and 1 keep views 0, 1): the loop ends."""
    return Sweep([[0, 1, 2, 3], [0, 1, 2, 3], [4, 5], [4, 5, 6], [6, 0, 1]], 7,
                 expected=(3, 3, 3, [1, 1, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0]))


def nothing_scene():
    return Sweep([[0, 1, 2, 3], [0, 1, 2, 3]], 4, expected=(0, 0, 1, [1, 1], [1, 1, 1, 1]))


def everything_scene():
    """Two views on two tracks: both views go (2 < 3), then both tracks (no view left); round 2 finds nothing."""
    return Sweep([[0, 1], [0, 1]], 2, expected=(2, 2, 2, [0, 0], [0, 0]))


def random_sweep(num_views=300, num_tracks=2000, seed=7, track_fraction=0.5):
    """About 5 observations per track in distinct views, random flags.  With half the tracks estimated no view is
    underconstrained (one round, tracks only); with an eighth the removals cascade over several rounds."""
    rng = np.random.default_rng(seed)
    ov, ot = [], []
    for t in range(num_tracks):
        views = rng.choice(num_views, size=int(rng.integers(1, 10)), replace=False)
        ov.extend(views.tolist()); ot.extend([t] * len(views))
    order = rng.permutation(len(ov))
    s = Sweep([[]] * num_views, num_tracks)
    s.obs_view = np.array(ov, dtype=np.int32)[order]
    s.obs_track = np.array(ot, dtype=np.int32)[order]
    s.view_estimated = (rng.random(num_views) < 0.8).astype(np.uint8)
    s.track_estimated = (rng.random(num_tracks) < track_fraction).astype(np.uint8)
    return s


IMAGE_SIZE = (1920, 1080)   # synth_ba_v1 keeps every observation inside it


def localization_scene(seed=0x10CA1, num_views=6, num_tracks=200, num_groups=1, pixel_noise=0.3, unestimated_view=2):
    """synth.synth_ba_v1's ring of pinhole cameras without lens distortion, at the true cameras and points, observations =
    exact projections + noise; one view unestimated, image sizes set.  Returns the sfm.Reconstruction."""
    p, cam_gt, pts = synth.synth_ba_v1(num_views, num_tracks, seed=seed, num_groups=num_groups, return_truth=True)
    p.intrinsics[:, 5:7] = 0.0
    p.cam_ext[:] = cam_gt
    p.points[:] = pts
    uv, ok = synth.project(synth.CAM_PINHOLE, p.intrinsics[p.cam_group[p.obs_cam]], cam_gt[p.obs_cam], pts[p.obs_pt])
    assert ok.all()
    noise = np.random.default_rng(seed).normal(size=uv.shape) * pixel_noise
    p.obs_uv = np.ascontiguousarray(uv + noise)
    r = sfm.Reconstruction.from_flat(p)
    r.view_image_size = np.tile(np.array(IMAGE_SIZE, dtype=np.int32), (num_views, 1))
    r.view_focal_prior_set = np.zeros(num_views, dtype=bool)
    if unestimated_view is not None:
        r.view_estimated[unestimated_view] = False
    return r


def copy_reconstruction(r):
    import copy
    q = copy.copy(r)
    for name, value in vars(r).items():
        if isinstance(value, np.ndarray):
            setattr(q, name, value.copy())
    q.view_priors = dict(r.view_priors)
    return q
