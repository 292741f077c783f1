"""Sequential restatement, in plain numpy, of the brute-force matcher's arithmetic and pair rule (DESIGN.md 3.6m;
matching/brute_force_feature_matcher.cc:48-115, feature_matcher_utils.cc:48-70) for the tests of csrc/brute_force_matcher.hip.

Arithmetic, every operation fixed: dot(i, j) = fmaf chain over k ascending from +0.0f (one accumulator), nrm(i) = the same chain over
d[i, k] * d[i, k], t = nrm1(i) + nrm2(j) (one float rounding), d = max(fmaf(-2, dot, t), 0).  The two nearest per query under
(distance, candidate index) ascending.  Ratio test: (double)d0 < (double)((float)ratio * (float)ratio) * (double)d1."""
import numpy as np

F32, F64 = np.float32, np.float64


def fmaf32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding, elementwise.  The product of two float32 is exact in float64 (48 bits); the sum with c
    is taken by TwoSum, rounded to odd in float64 (if the error term is non-zero and the sum's last mantissa bit is even, one ulp
    towards the error) and only then rounded to float32: float64 keeps more than 24 + 2 bits, so the two roundings equal one."""
    a = np.asarray(a, dtype=F32); b = np.asarray(b, dtype=F32); c = np.asarray(c, dtype=F32)
    p = a.astype(F64) * b.astype(F64)
    c64 = c.astype(F64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    even = (np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0
    step = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & even & np.isfinite(s), step, s)
    return s.astype(F32)


def naive_fmaf32(a, b, c):
    """What NOT to use: rounds twice (to float64, then to float32)."""
    return F32(F64(a) * F64(b) + F64(c))


def norms(desc):
    desc = np.asarray(desc, dtype=F32)
    acc = np.zeros(len(desc), dtype=F32)
    for k in range(desc.shape[1]):
        acc = fmaf32(desc[:, k], desc[:, k], acc)
    return acc


def distance_matrix(desc1, desc2):
    """d[i, j] as stated above, float32 [n1][n2]."""
    desc1 = np.asarray(desc1, dtype=F32); desc2 = np.asarray(desc2, dtype=F32)
    dot = np.zeros((len(desc1), len(desc2)), dtype=F32)
    for k in range(desc1.shape[1]):
        dot = fmaf32(desc1[:, k][:, None], desc2[:, k][None, :], dot)
    t = (norms(desc1)[:, None] + norms(desc2)[None, :]).astype(F32)
    return np.maximum(fmaf32(F32(-2.0), dot, t), F32(0.0))


def _top2(d):
    """Per row of d: the two smallest under (distance, column) ascending; +inf / -1 where the row has fewer than two columns."""
    n, m = d.shape
    dist = np.full((n, 2), np.inf, dtype=d.dtype); index = np.full((n, 2), -1, dtype=np.int32)
    for i in range(n):
        order = sorted(range(m), key=lambda j: (float(d[i, j]), j))[:2]
        for s, j in enumerate(order):
            dist[i, s] = d[i, j]; index[i, s] = j
    return dist, index


def knn2(desc1, desc2):
    """(fwd_dist [n1][2], fwd_index, rev_dist [n2][2], rev_index): ONE matrix serves both directions -- distance(d2[j], d1[i]) of the
    reference's reverse pass is d[i, j] bit for bit (the product and the sum of the norms commute)."""
    d = distance_matrix(desc1, desc2)
    fd, fi = _top2(d)
    rd, ri = _top2(np.ascontiguousarray(d.T))
    return fd, fi, rd, ri


def _one_direction(dist, index, use_lowes_ratio, sq):
    """The reference's loop over the queries of one direction: [(query, nearest, distance)] of those that pass."""
    out = []
    for i in range(len(dist)):
        if index[i, 0] < 0:          # no candidate (stated deviation: the reference is undefined there)
            continue
        if (not use_lowes_ratio) or float(dist[i, 0]) < sq * float(dist[i, 1]):
            out.append((i, int(index[i, 0]), dist[i, 0]))
    return out


def pair_rule(nn, keep_only_symmetric_matches=True, use_lowes_ratio=True, lowes_ratio=0.8, min_num_feature_matches=30):
    """MatchImagePair on the result of knn2: (ok, [(feature1, feature2, distance)]), in the reference's order of steps."""
    fd, fi, rd, ri = nn
    sq = float(F32(lowes_ratio) * F32(lowes_ratio))      # float product, then widened (:56-57)
    matches = _one_direction(fd, fi, use_lowes_ratio, sq)
    if len(matches) < min_num_feature_matches:           # :82-84
        return False, []
    if keep_only_symmetric_matches:
        reverse = _one_direction(rd, ri, use_lowes_ratio, sq)
        index_map = {}                                   # IntersectMatches: feature2 -> feature1 of the backwards matches
        for f2, f1, _ in reverse:
            assert f2 not in index_map
            index_map[f2] = f1
        matches = [m for m in matches if index_map.get(m[1], -1) == m[0]]
    if len(matches) < min_num_feature_matches:           # :114
        return False, []
    return True, matches


def match_image_pair(desc1, desc2, **options):
    return pair_rule(knn2(desc1, desc2), **options)


def direct_f64_matches(desc1, desc2, **options):
    """The same rule on float64 direct-form distances sum((a - b)^2): what the expansion must agree with where decisions have a margin."""
    a = np.asarray(desc1, dtype=F64); b = np.asarray(desc2, dtype=F64)
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    fd, fi = _top2(d)
    rd, ri = _top2(np.ascontiguousarray(d.T))
    return pair_rule((fd, fi, rd, ri), **options)
