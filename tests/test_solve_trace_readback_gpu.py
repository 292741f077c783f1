"""GPU: the per-iteration trace of theia_hip_ba_run across the edge of its read-back (csrc/ba_handle.h: the first
kTraceHead = 64 entries of the five arrays sit behind the LM state and come back with it; a longer trace copies the rest
after the loop).  A C1-sized solve of 70 iterations -- all tolerances zero and the trust region capped at 1e-2, a damping
of 100 diag(J'J) after the first accepted step, so the cost still falls by ~2 % of what is left per iteration at the cap
instead of converging exactly in two dozen: 71 trace entries -- is run from the same restored start with every capacity
around that edge; whatever a run returns must be the beginning of the longest run's trace, bit for bit.  (The inverse-depth handle has its own loop and trace, csrc/ba_invdepth.hip.)"""
import numpy as np
import pytest

from pytheiasfm_amd import ba, synth

pytestmark = pytest.mark.gpu
K = 64            # kTraceHead
ITERS = 70
FIELDS = ("cost", "gradient_max_norm", "step_norm", "radius", "accepted")


def _options(iters):
    o = ba.default_options()
    o.max_num_iterations = iters
    o.function_tolerance = 0.0; o.gradient_tolerance = 0.0; o.parameter_tolerance = 0.0
    o.use_inner_iterations = 0
    o.max_trust_region_radius = 1e-2
    return o


@pytest.fixture(scope="module")
def handle():
    p = synth.ba_config("C1")
    h = ba.BaHandle(p, _options(ITERS))
    h.reset(p)
    h.snapshot()
    yield h
    h.close()


def _run(h, cap, iters=ITERS):
    h.set_options(_options(iters))
    h.restore()
    return h.run(trace_capacity=cap)


@pytest.fixture(scope="module")
def longest(handle):
    s, tr = _run(handle, 256)
    assert s.num_iterations == ITERS and tr.size == ITERS + 1, (s.num_iterations, tr.size, s.termination_type)
    assert not np.any(tr.gradient_max_norm == -1.0)
    return s, tr


def _same_prefix(tr, ref, n, tag):
    assert tr.size == n, (tag, tr.size, n)
    for f in FIELDS:
        a, b = getattr(tr, f), getattr(ref, f)[:n]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {f} differs from the long run"


@pytest.mark.parametrize("cap", [0, 1, K - 1, K, K + 1, 256])
def test_capacity_cuts_the_same_trace(handle, longest, cap):
    s, tr = _run(handle, cap)
    assert s.num_iterations == ITERS
    assert (s.final_cost, s.num_successful_steps) == (longest[0].final_cost, longest[0].num_successful_steps)
    _same_prefix(tr, longest[1], min(cap, ITERS + 1), f"capacity {cap}")


@pytest.mark.parametrize("chunk", ["1", "3"])
def test_one_iteration_per_read_back(handle, longest, chunk, monkeypatch):
    """THEIA_HIP_LM_CHUNK: the head is read back after every chunk; the last read is the one that counts."""
    monkeypatch.setenv("THEIA_HIP_LM_CHUNK", chunk)
    for cap in (K, K + 1, 256):
        s, tr = _run(handle, cap)
        _same_prefix(tr, longest[1], min(cap, ITERS + 1), f"chunk {chunk} capacity {cap}")


@pytest.mark.parametrize("iters", [1, 3, K - 1, K, K + 1])
def test_accepted_step_at_the_iteration_cap_gets_its_gradient(handle, longest, iters):
    """A solve that ends on an accepted step has no next linearisation to bring the gradient of its last trace entry:
    run() linearises once more and patches that entry (in the head at index <= 63, in the tail at 64 and 65), and the
    read-back must see the patched value, never the -1 placeholder.  It is the gradient at the same point through the
    same kernels as the long run's next iteration, so the same bits."""
    ref = longest[1]
    s, tr = _run(handle, 256, iters)
    assert s.num_iterations == iters
    _same_prefix(tr, ref, iters + 1, f"{iters} iterations")
    assert tr.gradient_max_norm[-1] != -1.0
    if iters <= 3:
        assert tr.accepted[-1] == 1, "the early steps of this solve are accepted: the case must take the pending-gradient path"
