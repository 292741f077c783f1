"""GPU: K3, the tile-sparse level-scheduled Cholesky of the reduced camera system, called directly on tile structures
chosen to take each branch of the plan builder (theia_hip_tile_sparse_spd_solve[_sharded]), against the long-double
yardsticks of tests/k3_systems.py.  Every case also asserts the path it is named for, so none passes on the dense
fallback by accident."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import ba
from tests import k3_systems as ks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _levels_lt_nt(info, nt):
    return info["dense"] == 0 and info["levels"] < nt


# name -> (n, adjacency, seed, column scaling, check(info, nt))
CASES = {
    "single_1": (1, None, 1, 0, lambda i, nt: i["dense"] == 1),
    "single_37": (37, None, 2, 2, lambda i, nt: i["dense"] == 1),
    "single_64": (64, None, 3, 0, lambda i, nt: i["dense"] == 1),
    "two_100": (100, ks.path(2), 4, 2, lambda i, nt: i["dense"] == 1),
    "path3_short": (130, ks.path(3), 5, 0, lambda i, nt: i["dense"] == 0 and i["levels"] == 2 and i["num_symm_tiles"] > 0),
    "path7": (64 * 7, ks.path(7), 6, 2, lambda i, nt: i["dense"] == 0 and i["levels"] == 3),
    "ring8": (64 * 8 - 9, ks.ring(8), 7, 0, lambda i, nt: i["dense"] == 0 and i["levels"] == 4),
    "star7": (64 * 8, ks.star(8, 3), 8, 4, lambda i, nt: i["dense"] == 0 and i["levels"] == 2),
    "ring19_0": (64 * 19, ks.ring(19), 9, 0, _levels_lt_nt),
    "ring19_5": (64 * 19 - 5, ks.ring(19), 10, 2, _levels_lt_nt),
    "ring19_63": (64 * 19 - 63, ks.ring(19), 11, 4, _levels_lt_nt),
    "ring94_0": (64 * 94, ks.ring(94), 12, 0, _levels_lt_nt),
    "ring94_5": (64 * 94 - 5, ks.ring(94), 13, 2, _levels_lt_nt),
    "ring94_63": (64 * 94 - 63, ks.ring(94), 14, 0, _levels_lt_nt),
    "path40": (64 * 40 - 1, ks.path(40), 15, 0, _levels_lt_nt),
    "band48_w2": (64 * 48, ks.band(48, 2), 16, 2, _levels_lt_nt),
    "band48_w3": (64 * 48 - 30, ks.band(48, 3), 17, 0, _levels_lt_nt),
    "grid8x8": (64 * 64, ks.grid(8, 8), 18, 2, _levels_lt_nt),
    "path60_chords": (64 * 60 - 7, ks.path_with_chords(60, [(3, 41), (17, 58)]), 19, 0, _levels_lt_nt),
    "hub_star30": (64 * 31 - 11, ks.star(31, 0), 20, 2,
                   lambda i, nt: i["dense"] == 0 and i["num_deferred_targets"] > 0 and i["levels"] == 2),
    "intrinsics_ring": (80 + 6 * 1000, ks.intrinsics_ring(95), 21, 0,
                        lambda i, nt: i["dense"] == 0 and i["num_deferred_partials"] > i["num_deferred_targets"] > 0),
    "three_rings_isolated": (64 * 31 - 3, ks.disjoint(ks.ring(10), ks.ring(10), ks.ring(9), ks.path(1), ks.path(1)), 22, 0,
                             _levels_lt_nt),
    "random30_s1": (64 * 30 - 21, ks.random_graph(30, 3, 101), 23, 0, _levels_lt_nt),
    "random30_s2": (64 * 30, ks.random_graph(30, 3, 102), 24, 2, _levels_lt_nt),
    "random30_s3": (64 * 30 - 63, ks.random_graph(30, 3, 103), 25, 0, _levels_lt_nt),
    "random80_s1": (64 * 80 - 40, ks.random_graph(80, 3, 201), 26, 0, _levels_lt_nt),
    "random80_s2": (64 * 80, ks.random_graph(80, 3, 202), 27, 4, _levels_lt_nt),
    "random80_s3": (64 * 80 - 2, ks.random_graph(80, 3, 203), 28, 0, _levels_lt_nt),
    "complete12": (64 * 12 - 6, ks.complete(12), 29, 0, lambda i, nt: i["dense"] == 1),
}
# lda = n + 67, modes 1 and 2
PADDED = ["two_100", "path3_short", "ring19_5", "hub_star30", "intrinsics_ring", "random30_s1", "three_rings_isolated"]
REPORT = {}   # case -> numbers for the record (printed by test_zz_report)


@functools.lru_cache(maxsize=None)
def system(name):
    n, adj, seed, c, _ = CASES[name]
    if adj is None:
        adj = np.zeros((ks.num_tiles(n), ks.num_tiles(n)), np.uint8)
    return ks.make_system(n, adj, seed, cscale=c)


def declared_adj(name):
    return CASES[name][1]


def check_accuracy(s, x, tag=""):
    x_ref, kappa, eta_lapack = s.ref()
    e = ks.eta(s.A, x, s.b)
    f = ks.forward_error(x, x_ref)
    assert e <= ks.eta_bound(s.n), f"{tag}: eta {e:.3e} > bound {ks.eta_bound(s.n):.3e} (LAPACK {eta_lapack:.3e})"
    assert f <= ks.fwd_bound(s.n, kappa), f"{tag}: forward error {f:.3e}, kappa {kappa:.3e}"
    return e, eta_lapack, f / (kappa * ks.U)


def check_schedule(adj, order, level):
    nt = len(order)
    assert sorted(order.tolist()) == list(range(nt))
    pos = np.empty(nt, int); pos[order] = np.arange(nt)
    _, fedges = ks.factor_structure(adj, order)
    for u, v in ks.edges_of(adj) + fedges:
        a, b = (u, v) if pos[u] < pos[v] else (v, u)
        assert level[pos[a]] < level[pos[b]], f"edge {a}-{b}: levels {level[pos[a]]} / {level[pos[b]]}"


@pytest.mark.parametrize("name", list(CASES))
def test_k3_case_mode0(name):
    """lda == n, the rhs as row n: accuracy, the path, the schedule; then the same buffer with NaN everywhere the factor
    must not read (strict upper triangle, lower tiles outside the declared + fill structure) gives the same bits."""
    s = system(name)
    adj = declared_adj(name)
    A0 = np.tril(s.A)
    x, info, order, level = ba.tile_sparse_spd_solve(A0, s.b, adj)
    assert CASES[name][4](info, s.nt), info
    e, el, fk = check_accuracy(s, x, name)
    if adj is not None:
        check_schedule(adj, order, level)
    x2, _, _, _ = ba.tile_sparse_spd_solve(A0, s.b, adj)
    assert np.array_equal(x, x2), "two solves of the same input differ"
    struct = ks.factor_structure(adj if adj is not None else np.ones((s.nt, s.nt), np.uint8), order)[0]
    xp, _, _, _ = ba.tile_sparse_spd_solve(ks.poison(s.A, struct, s.n), s.b, adj)
    assert np.array_equal(x, xp), "the poisoned buffer changed the solution"
    REPORT[name] = dict(n=s.n, nt=s.nt, dense=info["dense"], levels=info["levels"], symm=info["num_symm_tiles"],
                        deferred=info["num_deferred_targets"], partials=info["num_deferred_partials"],
                        eta=e, eta_lapack=el, fwd_over_kappa_u=fk, kappa=s.ref()[1])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", PADDED)
def test_k3_case_padded(name, mode):
    """lda = n + 67: the separate-solution back-substitution (mode 1) and the BA's clear-then-add order on a NaN-filled
    buffer (mode 2: a structure or fill tile missing from the clear list shows up)."""
    s = system(name)
    adj = declared_adj(name)
    lda = s.n + 67
    ref_x, _, order, _ = ba.tile_sparse_spd_solve(np.tril(s.A), s.b, adj)
    struct = ks.factor_structure(adj if adj is not None else np.ones((s.nt, s.nt), np.uint8), order)[0]
    declared = (adj != 0) | np.eye(s.nt, dtype=bool) if adj is not None else np.ones((s.nt, s.nt), bool)
    # mode 1: the fill tiles hold zeros (nobody clears them), everything else NaN; mode 2: only the declared tiles'
    # values reach the device buffer, the rest of the host array is NaN
    Ap = ks.poison(s.A, struct if mode == 1 else np.tril(declared), s.n, lda)
    x, info, _, _ = ba.tile_sparse_spd_solve(Ap, s.b, adj, mode=mode)
    assert CASES[name][4](info, s.nt), info
    check_accuracy(s, x, f"{name} mode {mode}")
    assert np.array_equal(x, ref_x), "lda / mode changed the bits"


def test_three_rings_levels_are_those_of_the_components():
    s = system("three_rings_isolated")
    _, info, order, level = ba.tile_sparse_spd_solve(np.tril(s.A), s.b, declared_adj("three_rings_isolated"))
    alone = []
    for k in (10, 10, 9):
        sk = ks.make_system(64 * k, ks.ring(k), 40 + k)
        alone.append(ba.tile_sparse_spd_solve(np.tril(sk.A), sk.b, ks.ring(k))[1]["levels"])
    assert info["levels"] == max(alone)
    # the isolated tiles are leaves: level 0
    pos = {t: p for p, t in enumerate(order.tolist())}
    assert level[pos[29]] == 0 and level[pos[30]] == 0


# ---------------------------------------------------------------- not positive definite
def _npd(name, which, how="neg"):
    s = system(name)
    adj = declared_adj(name)
    A = s.A.copy()
    _, info, order, level = ba.tile_sparse_spd_solve(np.tril(A), s.b, adj)    # control: succeeds
    t = {"level0": order[0], "top": order[-1], "last": s.nt - 1}.get(which, which)
    j = ks.tile_cols(s.n, t)[len(ks.tile_cols(s.n, t)) // 2]
    if how == "neg":
        A[j, j] = -1.0
    elif how == "schur":
        # pivot made non-positive only by the Schur updates: A[j, j] stays positive
        pos = np.empty(s.nt, int); pos[order] = np.arange(s.nt)
        p = np.concatenate([ks.tile_cols(s.n, u) for u in order])
        L = np.linalg.cholesky(A[np.ix_(p, p)])
        q = int(np.nonzero(p == j)[0][0])
        A[j, j] -= 1.01 * L[q, q] ** 2
        assert A[j, j] > 0.0
    else:
        i = ks.tile_cols(s.n, t)[-1]
        A[i, j] = A[j, i] = np.nan
    with pytest.raises(capi.TheiaHipError) as e:
        ba.tile_sparse_spd_solve(np.tril(A), s.b, adj)
    assert e.value.code == capi.THEIA_HIP_ERR_INTERNAL


@pytest.mark.parametrize("name, which, how", [
    ("ring19_5", "level0", "neg"), ("ring19_5", "top", "neg"), ("ring19_5", "top", "schur"), ("ring19_5", "last", "neg"),
    ("hub_star30", 0, "neg"), ("hub_star30", 0, "schur"), ("intrinsics_ring", 1, "neg"), ("path3_short", "last", "neg"),
    ("random30_s1", "level0", "nan"), ("grid8x8", "top", "schur"), ("two_100", "last", "neg")])
def test_not_positive_definite_is_reported(name, which, how):
    _npd(name, which, how)


# ---------------------------------------------------------------- variants of the same solve
@pytest.mark.parametrize("env, want", [("THEIA_HIP_NO_DEFERRED_BORDER", "no_deferred"), ("THEIA_HIP_DENSE_CHOLESKY", "dense")])
@pytest.mark.parametrize("name", ["hub_star30", "intrinsics_ring"])
def test_hub_cases_under_the_switches(name, env, want, monkeypatch):
    s = system(name)
    monkeypatch.setenv(env, "1")
    x, info, _, _ = ba.tile_sparse_spd_solve(np.tril(s.A), s.b, declared_adj(name))
    if want == "dense":
        assert info["dense"] == 1
    else:
        assert info["dense"] == 0 and info["num_deferred_targets"] == 0
    check_accuracy(s, x, f"{name} {env}")


SPLIT_CASES = ["path3_short", "ring19_5", "hub_star30", "intrinsics_ring", "random30_s2", "grid8x8"]


def test_split_trsm_gives_the_same_bits_as_the_fused_kernel(tmp_path):
    """THEIA_HIP_K3_SPLIT_TRSM (k_sp_potrf + k_sp_trsm) is read once per process: a fresh child process solves the same
    systems; the claim at k_sp_potrf_trsm is that the fused kernel does the same arithmetic, so the same bits."""
    out = tmp_path / "split.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from tests import test_k3_cholesky_gpu as t\n"
            "from pytheiasfm_amd import ba\n"
            "np.savez(%r, **{n: ba.tile_sparse_spd_solve(np.tril(t.system(n).A), t.system(n).b, t.declared_adj(n))[0] for n in %r})\n"
            % (ROOT, str(out), SPLIT_CASES))
    env = dict(os.environ, THEIA_HIP_K3_SPLIT_TRSM="1")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=600, cwd=ROOT)
    split = np.load(out)
    for name in SPLIT_CASES:
        s = system(name)
        x, _, _, _ = ba.tile_sparse_spd_solve(np.tril(s.A), s.b, declared_adj(name))
        check_accuracy(s, split[name], f"{name} split")
        assert np.array_equal(split[name], x), f"{name}: split and fused TRSM differ"


# ---------------------------------------------------------------- the sharded plan
def _contiguous(R, nt):
    return lambda tiles, rng: (tiles[0] * R) // nt


def _mostly_home(R, nt):
    return lambda tiles, rng: (tiles[0] * R) // nt if rng.random() < 0.98 else int(rng.integers(0, R))


def _third_rank_on_borders(nt):
    # ranks 0 / 1 own the halves; rank 2 takes some tracks of the tiles both halves already share
    def f(tiles, rng):
        if len(tiles) == 2 and {(t * 2) // nt for t in tiles} == {0, 1}:
            return 2 if rng.random() < 0.5 else 0
        return (tiles[0] * 2) // nt
    return f


def _two_arcs(nt):
    return lambda tiles, rng: (tiles[0] // (nt // 4)) % 2


def _shared_hub(R, leaves):
    return lambda tiles, rng: (max(tiles) - 1) * R // leaves if max(tiles) > 0 else int(rng.integers(0, R))


SHARDED = {
    "ring24_2": (64 * 24 - 5, ks.ring(24), 2, _contiguous(2, 24)),
    "ring24_4": (64 * 24, ks.ring(24), 4, _contiguous(4, 24)),
    "ring24_random": (64 * 24 - 33, ks.ring(24), 2, _mostly_home(2, 24)),
    "ring24_no_private": (64 * 24, ks.ring(24), 3, _third_rank_on_borders(24)),
    "ring24_two_arcs": (64 * 24 - 1, ks.ring(24), 2, _two_arcs(24)),
    "shared_hub": (64 * 21 - 9, ks.star(21, 0), 2, _shared_hub(2, 20)),
}


@functools.lru_cache(maxsize=None)
def sharded_system(name):
    n, adj, R, rank_of = SHARDED[name]
    return ks.make_system(n, adj, 300 + len(name), num_ranks=R, rank_of=rank_of)


@pytest.mark.parametrize("name", list(SHARDED))
def test_sharded_plan(name):
    s = sharded_system(name)
    R = s.parts_A.shape[0]
    if name == "ring24_no_private":
        assert not (s.tile_class[2] == 1).any() and (s.tile_class[2] == 0).any()
    if name == "shared_hub":
        assert (s.tile_class[:, 0] == 0).all()
    x, infos = ba.tile_sparse_spd_solve_sharded(np.tril(s.parts_A), s.parts_b, s.adj, s.tile_class)
    assert max(i["split_level"] for i in infos) > 0, infos
    assert all(i["dense"] == 0 for i in infos)
    shared = np.concatenate([ks.tile_cols(s.n, t) for t in range(s.nt) if s.tile_class[0, t] == 0])
    assert len(shared) > 0
    xa = np.empty(s.n)
    for r in range(R):
        assert np.array_equal(x[r][shared], x[0][shared]), f"rank {r}: the shared part differs from rank 0's"
        mine = [ks.tile_cols(s.n, t) for t in range(s.nt) if s.tile_class[r, t] == 1]
        if mine:
            xa[np.concatenate(mine)] = x[r][np.concatenate(mine)]
    xa[shared] = x[0][shared]
    e, el, fk = check_accuracy(s, xa, name)
    x_ref, kappa, _ = s.ref()
    for r in range(R):
        own = np.concatenate([shared] + [ks.tile_cols(s.n, t) for t in range(s.nt) if s.tile_class[r, t] == 1])
        assert np.abs(x[r][own] - x_ref[own]).max() <= ks.fwd_bound(s.n, kappa) * np.abs(x_ref).max()
    REPORT["sharded_" + name] = dict(n=s.n, ranks=R, split_levels=[i["split_level"] for i in infos],
                                     levels=[i["levels"] for i in infos], shared_tiles=infos[0]["num_shared_tiles"],
                                     eta=e, eta_lapack=el, fwd_over_kappa_u=fk)


def test_sharded_not_positive_definite_in_a_shared_tile():
    s = sharded_system("ring24_2")
    t = int(np.nonzero(s.tile_class[0] == 0)[0][0])
    j = ks.tile_cols(s.n, t)[5]
    P = s.parts_A.copy()
    P[0][j, j] = -np.abs(s.A).max()          # the shared diagonal lives on rank 0; negative after the sum
    with pytest.raises(capi.TheiaHipError) as e:
        ba.tile_sparse_spd_solve_sharded(np.tril(P), s.parts_b, s.adj, s.tile_class)
    assert e.value.code == capi.THEIA_HIP_ERR_INTERNAL


def test_zz_report():
    """The numbers per case, for the record (K3_REPORT=path writes them as JSON)."""
    path = os.environ.get("K3_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, default=float)
    for k, v in REPORT.items():
        print(k, v)
