"""Inputs for the tests of the global-descriptor image-pair selection (tests/test_graph_match.py, tests/test_graph_match_gpu.py)."""
import numpy as np

F32 = np.float32

# (one-dimensional descriptors, k, the selected pairs as read off the reference's loop by hand)
READ_OFF = [
    ([0, 1, 3, 7], 1, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]),
    # (1, 2) is absent although 1 and 2 are both ranked with 0: the expanded entry (2, 1) has a > i and is dropped; (0, 3) is there
    ([0, -5, 3, 4], 1, [(0, 1), (0, 2), (0, 3), (2, 3)]),
    # ties go to the lower index
    ([0, 0, 0, 0], 1, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]),
    # two images, k clamped to 1
    ([2, 9], 100, [(0, 1)]),
]
READ_OFF_IDS = ["chain", "dropped-entry", "all-tied", "two-images"]


def read_off_descriptors(case):
    return np.asarray(case[0], dtype=F32).reshape(-1, 1)


def tied_integers(n, dim, seed):
    """Small-integer descriptors with forced duplicate images: many equal distances, every one exact in any order of summation."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-3, 4, size=(n, dim)).astype(F32)
    for _ in range(max(1, n // 4)):
        a = int(rng.integers(0, n))
        b = (a + 1 + int(rng.integers(0, n - 1))) % n         # another image
        g[a] = g[b]
    return g


def hub(n, dim, seed):
    """Image n // 2 sits at the centre and every other image at distance 10 in a random direction: in 128 dimensions the hub is
    the nearest of all (one inverse list of n - 1 entries), in few dimensions it is in most lists and the others tie a lot."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, dim)).astype(F32)
    g = (g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), F32(1e-6)) * F32(10.0)).astype(F32)
    g[n // 2] = 0
    return g


def clustered(n, dim, seed, clusters=4):
    """Real-valued descriptors around a few centres, the shape of pooled descriptors: close together, so the order of the fmaf
    chain shows in the last bits."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, dim))
    g = centres[rng.integers(0, clusters, size=n)] + 0.05 * rng.standard_normal((n, dim))
    return (g + 40.0).astype(F32)


def f64_knn(g, k):
    """The independent route for small-integer descriptors: float64 numpy distances, which are exact integers there, and the
    (distance, index) order as the order of the integers distance * N + index."""
    g64 = np.asarray(g, dtype=np.float64)
    assert np.array_equal(g64, np.round(g64))
    sq = (g64 * g64).sum(1)
    d = sq[:, None] + sq[None, :] - 2.0 * (g64 @ g64.T)      # integers far below 2^53: exact
    n = len(g)
    kk = max(0, min(n - 1, k))
    key = d.astype(np.int64) * n + np.arange(n, dtype=np.int64)[None, :]
    np.fill_diagonal(key, np.iinfo(np.int64).max)
    if kk < n - 1:
        key = np.partition(key, kk, axis=1)[:, :kk]              # the kk smallest of every row, in any order
    key = np.sort(key, axis=1)[:, :kk]
    return (key % n).astype(np.int32), (key // n).astype(F32)
