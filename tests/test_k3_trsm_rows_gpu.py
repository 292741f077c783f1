"""GPU: the rows-per-workgroup rule of K3's fused factor + triangular-solve kernel (csrc/sparse_cholesky.hip,
k_sp_potrf_trsm<RB>): a level's off-diagonal tiles are split over 4, 2 or 1 workgroups each -- the finest split that
needs no more rounds of resident workgroups than one workgroup per tile.  An entry's arithmetic does not depend on the
split, so every setting must return the same bits.

THEIA_HIP_K3_TRSM_SLOTS (development, read once per process) replaces the device's number of resident workgroups: the
systems of tests/test_k3_cholesky_gpu.py are solved in fresh child processes with 8 and 40 places (small systems then
take all three splits, asserted below from the schedule the solver reports), with no limit (four workgroups per tile
everywhere: the kernel before the rule) and with the device's own number.  Accuracy: the long-double backward error
and the forward error with the bounds of tests/k3_systems.py, through the helper of tests/test_k3_cholesky_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pytheiasfm_amd import ba
from tests import k3_systems as ks
from tests import test_k3_cholesky_gpu as t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# short last tile as a diagonal tile and as a row (path3_short, ring19_5), the rhs row (h = 1) everywhere, a dense border
# (hub_star30), isolated tiles (three_rings_isolated), wide levels (grid8x8)
NAMES = ["path3_short", "star7", "ring19_5", "hub_star30", "three_rings_isolated", "random30_s2", "grid8x8"]
SETTINGS = {"device": None, "unlimited": str(1 << 28), "slots8": "8", "slots40": "40"}


def splits(adj, order, level, slots):
    """Workgroups per off-diagonal tile the rule gives each level: a level factors `np` diagonal tiles and solves
    sum(below + 1) off-diagonal ones (the + 1: the rhs row)."""
    nt = len(order)
    pos = np.empty(nt, int); pos[np.asarray(order)] = np.arange(nt)
    below = np.zeros(nt, int)
    for first, _ in ks.factor_structure(adj, np.asarray(order))[1]:
        below[pos[first]] += 1
    out = []
    for l in range(int(max(level)) + 1):
        sel = np.asarray(level) == l
        npotrf, ntrsm = int(sel.sum()), int((below[sel] + 1).sum())
        rounds = lambda w: -(-(npotrf + w * ntrsm) // slots)
        out.append(4 if rounds(4) == rounds(1) else (2 if rounds(2) == rounds(1) else 1))
    return out


def solve_all():
    return {n: ba.tile_sparse_spd_solve(np.tril(t.system(n).A), t.system(n).b, t.declared_adj(n))[0] for n in NAMES}


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    d = tmp_path_factory.mktemp("k3rows")
    code = ("import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from tests import test_k3_trsm_rows_gpu as m\n"
            "np.savez(sys.argv[1], **m.solve_all())\n" % ROOT)
    got = {}
    for tag, slots in SETTINGS.items():
        env = {k: v for k, v in os.environ.items() if k != "THEIA_HIP_K3_TRSM_SLOTS"}
        if slots is not None:
            env["THEIA_HIP_K3_TRSM_SLOTS"] = slots
        out = d / (tag + ".npz")
        subprocess.run([sys.executable, "-c", code, str(out)], env=env, check=True, timeout=600, cwd=ROOT)
        got[tag] = dict(np.load(out))
    return got


def test_the_small_settings_take_every_split():
    seen = {8: set(), 40: set()}
    for name in NAMES:
        s = t.system(name)
        _, info, order, level = ba.tile_sparse_spd_solve(np.tril(s.A), s.b, t.declared_adj(name))
        assert info["dense"] == 0
        for slots in seen:
            seen[slots] |= set(splits(t.declared_adj(name), order, level, slots))
    assert seen[8] | seen[40] == {1, 2, 4}, seen
    assert len(seen[8]) > 1 and len(seen[40]) > 1, seen


@pytest.mark.parametrize("name", NAMES)
def test_every_split_gives_the_same_bits(name, children):
    s = t.system(name)
    ref = children["unlimited"][name]
    t.check_accuracy(s, ref, name + " unlimited")
    for tag in SETTINGS:
        assert np.array_equal(children[tag][name], ref), f"{name}: {tag} differs from four workgroups per tile"
