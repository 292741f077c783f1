"""numpy restatement of the two view-graph filters of the global pipeline, written from the reference's description:

FilterViewPairsFromRelativeTranslation (sfm/filter_view_pairs_from_relative_translation.cc, Wilson & Snavely's 1DSfM):
  rotate      t_e = AngleAxisRotatePoint(-orientation[first], position_2)                         (:67-84)
  statistics  mean = sum / E, variance = sum (t - mean)^2 / (E - 1), summed in pair order         (:178-195)
  axes        (RandGaussian(mean_x, var_x), RandGaussian(mean_y, var_y), RandGaussian(mean_z, var_z)).normalized(),
              drawn in the order x, y, z -- the variance handed over as the standard deviation    (:212-217)
  project     p_e = (t0 a0 + t1 a1) + t2 a2                                                        (:163-175)
  order       the pair runs first -> second when p_e > 0, else second -> first, with weight |p_e|; one view is taken
              per step: a source (no live incoming pair) if there is one, else the largest
              (outgoing + 1.0) / (incoming + 1.0); its neighbours' weights are decremented         (:86-160)
  weight      over the iterations in order: += |p_e| where the order difference contradicts p_e's sign   (:236-259)
  removed     weight > tolerance * num_iterations                                                  (:296-305)

Where the reference's outcome depends on the iteration order of its hash maps, the rules are: the
lowest view index among the sources (rule="lowest"; rule="random" picks among them with `pick`, to show that the choice
does not change which pairs are judged), the lowest view index among equal scores, a view's initial weights summed
over its pairs in pair order.  Every arg-max step records the relative gap between the best and the second-best score,
and every pair how far its weight sits from the threshold: an equality test against another implementation of these
rules only means something when neither is a near tie.

FilterViewPairsFromOrientation (sfm/filter_view_pairs_from_orientation.cc:46-103): a pair stays when
|MultiplyRotations(-rotation_2, MultiplyRotations(r_second, -r_first))|^2 <= DegToRad(max degrees)^2."""
import math

import numpy as np

from tests.rotation_averaging_ref import multiply_rotations

DBL_EPSILON = np.finfo(np.float64).eps


def rotate_translations(orientations, pairs, position_2):
    """ceres::AngleAxisRotatePoint(-orientation[first], position_2) per pair."""
    aa = -np.asarray(orientations, dtype=np.float64).reshape(-1, 3)[np.asarray(pairs).reshape(-1, 2)[:, 0]]
    pt = np.asarray(position_2, dtype=np.float64).reshape(-1, 3)
    theta2 = (aa[:, 0] * aa[:, 0] + aa[:, 1] * aa[:, 1]) + aa[:, 2] * aa[:, 2]
    big = theta2 > DBL_EPSILON
    theta = np.sqrt(np.where(big, theta2, 1.0))
    c, s = np.cos(theta), np.sin(theta)
    w = aa * (1.0 / theta)[:, None]
    cr = np.stack([w[:, 1] * pt[:, 2] - w[:, 2] * pt[:, 1], w[:, 2] * pt[:, 0] - w[:, 0] * pt[:, 2],
                   w[:, 0] * pt[:, 1] - w[:, 1] * pt[:, 0]], 1)
    tmp = ((w[:, 0] * pt[:, 0] + w[:, 1] * pt[:, 1]) + w[:, 2] * pt[:, 2]) * (1.0 - c)
    out = (pt * c[:, None] + cr * s[:, None]) + w * tmp[:, None]
    small = np.stack([aa[:, 1] * pt[:, 2] - aa[:, 2] * pt[:, 1], aa[:, 2] * pt[:, 0] - aa[:, 0] * pt[:, 2],
                      aa[:, 0] * pt[:, 1] - aa[:, 1] * pt[:, 0]], 1)
    return np.where(big[:, None], out, pt + small)


def mean_variance(rotated):
    """ComputeMeanVariance, summed in pair order (cumsum adds one term after the other).  With one pair the variance is
    0 / 0, as in the reference."""
    t = np.asarray(rotated, dtype=np.float64).reshape(-1, 3)
    E = t.shape[0]
    mean = np.cumsum(t, axis=0)[-1] / float(E)
    d = t - mean
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.cumsum(d * d, axis=0)[-1] / float(E - 1)
    return mean, var


def draw_axes(mean, var, num_iterations, gauss):
    """gauss(mean, std_dev) -> one RandGaussian draw.  Three per iteration in the order x, y, z; Eigen's normalized():
    v / sqrt(|v|^2) when |v|^2 > 0, with |v|^2 = (x^2 + y^2) + z^2."""
    axes = np.empty((num_iterations, 3))
    for it in range(num_iterations):
        v = np.array([gauss(float(mean[k]), float(var[k])) for k in range(3)])
        z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        axes[it] = v / math.sqrt(z) if z > 0.0 else v
    return axes


def project(rotated, axis):
    t = np.asarray(rotated, dtype=np.float64).reshape(-1, 3)
    return (t[:, 0] * axis[0] + t[:, 1] * axis[1]) + t[:, 2] * axis[2]


class Adjacency:
    """One undirected CSR in pair order: per view its neighbours, the pair behind each slot and whether the view is the
    pair's second view."""

    def __init__(self, n_views, pairs):
        p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        E = p.shape[0]
        owner = np.concatenate([p[:, 0], p[:, 1]])
        pair = np.concatenate([np.arange(E), np.arange(E)])
        second = np.concatenate([np.zeros(E, bool), np.ones(E, bool)])
        o = np.lexsort((pair, owner))                   # per owner, in pair order
        self.pair, self.second = pair[o], second[o]
        self.view = np.where(self.second, p[self.pair, 0], p[self.pair, 1])
        self.off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n_views))])
        self.n, self.pairs = int(n_views), p


def order_views(adj, proj, rule="lowest", pick=None):
    """OrderTranslationsFromProjections.  Returns (order [n] with -1 for a view no pair names, the smallest relative gap
    between the best and second-best score over the arg-max steps (inf without one), source steps, arg-max steps)."""
    n, p = adj.n, adj.pairs
    proj = np.asarray(proj, dtype=np.float64)
    w = np.abs(proj)
    fwd = proj > 0.0
    src = np.where(fwd, p[:, 0], p[:, 1])
    dst = np.where(fwd, p[:, 1], p[:, 0])
    in_w, out_w = np.zeros(n), np.zeros(n)
    np.add.at(in_w, dst, w)                             # unbuffered: one addition after the other, in pair order
    np.add.at(out_w, src, w)
    indeg = np.bincount(dst, minlength=n)
    alive = np.diff(adj.off) > 0
    named = int(alive.sum())
    order = -np.ones(n, dtype=np.int64)
    slot_p, slot_w = proj[adj.pair], w[adj.pair]
    min_gap, n_source = np.inf, 0
    for step in range(named):
        sources = alive & (indeg == 0)
        if sources.any():
            v = int(np.argmax(sources)) if rule == "lowest" else int(pick(np.flatnonzero(sources)))
            n_source += 1
        else:
            score = np.where(alive, (out_w + 1.0) / (in_w + 1.0), -np.inf)
            v = int(np.argmax(score))                   # the first of equal maxima: the lowest view index
            if named - step > 1:
                best = score[v]
                score[v] = -np.inf
                min_gap = min(min_gap, (best - score.max()) / best)
        order[v] = step
        alive[v] = False
        k0, k1 = adj.off[v], adj.off[v + 1]
        u = adj.view[k0:k1]
        live = alive[u]
        outgoing = (slot_p[k0:k1] > 0.0) != adj.second[k0:k1]      # from v to u
        a, b = live & outgoing, live & ~outgoing
        in_w[u[a]] -= slot_w[k0:k1][a]                  # pairs are unique: no view twice in u
        indeg[u[a]] -= 1
        out_w[u[b]] -= slot_w[k0:k1][b]
    return order, min_gap, n_source, named - n_source


def filter_translations(n_views, pairs, orientations, position_2, num_iterations=48, tolerance=0.08, axes=None, gauss=None,
                        rotated=None, rule="lowest", pick=None):
    """The whole filter.  axes: [num_iterations][3] used as given, else drawn through gauss.  rotated: the rotated
    translations to go on from (else computed here).  Returns a dict: removed, bad_weight, order [it][n], axes, rotated,
    min_gap (arg-max steps), threshold_margin (smallest relative distance of a weight from the threshold), source_steps,
    argmax_steps."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    E = p.shape[0]
    t = rotate_translations(orientations, p, position_2) if rotated is None else np.asarray(rotated, dtype=np.float64)
    if E < 2:   # the variance is 0 / 0: NaN axes, no comparison holds, nothing is removed
        return dict(removed=np.zeros(E, bool), bad_weight=np.zeros(E), order=-np.ones((num_iterations, n_views), np.int64),
                    axes=np.full((num_iterations, 3), np.nan), rotated=t, min_gap=np.inf, threshold_margin=np.inf,
                    source_steps=0, argmax_steps=0)
    if axes is None:
        mean, var = mean_variance(t)
        axes = draw_axes(mean, var, num_iterations, gauss)
    axes = np.asarray(axes, dtype=np.float64).reshape(num_iterations, 3)
    adj = Adjacency(n_views, p)
    weight = np.zeros(E)
    orders = np.empty((num_iterations, n_views), dtype=np.int64)
    min_gap, ns, na = np.inf, 0, 0
    for it in range(num_iterations):
        pr = project(t, axes[it])
        order, gap, s, a = order_views(adj, pr, rule, pick)
        orders[it] = order
        min_gap, ns, na = min(min_gap, gap), ns + s, na + a
        diff = order[p[:, 1]] - order[p[:, 0]]
        bad = ((diff < 0) & (pr > 0.0)) | ((diff > 0) & (pr < 0.0))
        weight = np.where(bad, weight + np.abs(pr), weight)
    threshold = tolerance * num_iterations
    margin = float(np.min(np.abs(weight - threshold)) / threshold) if threshold > 0.0 else np.inf
    return dict(removed=weight > threshold, bad_weight=weight, order=orders, axes=axes, rotated=t, min_gap=min_gap,
                threshold_margin=margin, source_steps=ns, argmax_steps=na)


def filter_orientations(pairs, orientations, rotation_2, max_degrees, has_orientation=None):
    """Returns (removed [E], the smallest relative distance of a squared residual from the squared threshold)."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    aa = np.asarray(orientations, dtype=np.float64).reshape(-1, 3)
    rel = np.asarray(rotation_2, dtype=np.float64).reshape(-1, 3)
    composed = multiply_rotations(aa[p[:, 1]], -aa[p[:, 0]])
    loop = multiply_rotations(-rel, composed)
    sq = (loop[:, 0] * loop[:, 0] + loop[:, 1] * loop[:, 1]) + loop[:, 2] * loop[:, 2]
    rad = max_degrees * (math.pi / 180.0)
    sq_max = rad * rad
    removed = ~(sq <= sq_max)
    known = np.ones(p.shape[0], bool)
    if has_orientation is not None:
        h = np.asarray(has_orientation, dtype=bool)
        known = h[p[:, 0]] & h[p[:, 1]]
        removed = removed | ~known
    margin = float(np.min(np.abs(sq[known] - sq_max)) / sq_max) if known.any() and sq_max > 0.0 else np.inf
    return removed, margin
