"""A GN step of the ring schedule whose PCGInit1 stores no zeros into delta (csrc/solver.cpp step_gn_one_kernel: the step's first update of delta is told that delta
is zero) against the same plan with THALLO_AB=delta_first_touch=0 (the zero fill of every other schedule), and the coarse timers that share one event record per
stream position (CoarseTimer::stop_start / stop_both)."""
import numpy as np
import pytest

import thallo_amd
from thallo_amd import api, synthetic as syn
from helpers import to_device, copy_params, set_ab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ring_env(monkeypatch):
    monkeypatch.setenv("THALLO_RESIDENT", "0")          # one launch per PCG iteration
    monkeypatch.setenv("THALLO_MARCH", "2")             # the marching kernel (the one that takes any p plane) at these sizes too
    monkeypatch.delenv("THALLO_DELTA_PLANES", raising=False)


@pytest.mark.parametrize("lit", [40, 12])
@pytest.mark.parametrize("W,H", [(130, 66), (256, 192)])
def test_delta_first_touch_is_bitwise_the_zero_fill(torch, monkeypatch, W, H, lit):
    """lIterations 40: the ring of 33 planes is flushed before launch 33, that PCGDeltaUpdate is delta's first reader; lIterations 12: nothing is flushed,
    PCGLinearUpdate is.  Three GN steps: from the second on the plane still holds the step before's delta (40) or whatever the first plan left there (12), so a
    consumer that reads delta instead of starting from 0.0f shows in the unknowns, the costs and the traces.  Same launches either way."""
    p = syn.image_warping(W, H, n_markers=8, mask_disc=0.1)
    _ring_env(monkeypatch)
    runs = []
    for first_touch in (None, "0"):
        set_ab(monkeypatch, delta_first_touch=first_touch)
        dev = to_device(copy_params(p))
        s = api.ThalloSolver((W, H), thallo_amd.energy_file("image_warping"), timing_level=2)
        s.set_solver_parameters(nIterations=3, lIterations=lit)
        params = s.make_params(dev)
        s.init(params)
        costs, traces = [s.current_cost()], []
        while s.step(params):
            costs.append(s.current_cost()); traces.append(s.alpha_beta_trace())
        stats = {k: v["launches"] for k, v in s.kernel_stats().items()}
        s.close()
        runs.append((costs, traces, dev[0].clone(), dev[1].clone(), stats))
    (c1, t1, o1, a1, n1), (c0, t0, o0, a0, n0) = runs
    assert all(np.isfinite(c0)) and len(c0) == 4 and len(t0) == 3 and len(t0[0]) == lit
    assert n0 == n1, (n0, n1)
    assert n1.get("PCGDeltaUpdate", 0) == (3 if lit == 40 else 0) and n1["PCGIteration"] == 3 * lit and n1["PCGLinearUpdate"] == 3 * 2, n1
    assert t0 == t1, [(i, k) for i, (x, y) in enumerate(zip(t0, t1)) for k, (u, v) in enumerate(zip(x, y)) if u != v][:3]
    assert c0 == c1, (c0, c1)
    assert torch.equal(o0, o1) and torch.equal(a0, a1)


def test_coarse_timers_share_event_records(torch, monkeypatch):
    """timingLevel 1: after three GN steps every per-step row of the performance summary counts 3 ("Total" spans Init to the end of the solve: one interval per solve,
    count 1), and the intervals nest -- "Linear Solve" inside "Nonlinear Iteration" inside "Total", the three parts of a step inside the step -- although a start
    behind a start, a stop and the start behind it, and the two stops at a step's end are ONE event record each; timingLevel 0 records nothing."""
    W, H = 130, 66
    p = syn.image_warping(W, H, n_markers=8)
    _ring_env(monkeypatch)
    for level in (1, 0):
        dev = to_device(copy_params(p))
        s = api.ThalloSolver((W, H), thallo_amd.energy_file("image_warping"), timing_level=level)
        s.set_solver_parameters(nIterations=3, lIterations=12)
        params = s.make_params(dev)
        s.init(params)
        steps = 0
        while s.step(params): steps += 1
        ps = s.performance_summary()
        s.close()
        assert steps == 3
        rows = ["nonlinearIteration", "nonlinearSetup", "linearSolve", "nonlinearResolve"]
        if level == 0:
            assert all(v == 0 for row in ps.values() for v in row.values()), ps
            continue
        assert ps["total"]["count"] == 1 and all(ps[r]["count"] == 3 for r in rows), ps
        assert all(ps[r]["minMS"] > 0.0 and ps[r]["minMS"] <= ps[r]["meanMS"] <= ps[r]["maxMS"] for r in rows + ["total"]), ps
        assert ps["linearSolve"]["meanMS"] <= ps["nonlinearIteration"]["meanMS"] and 3 * ps["nonlinearIteration"]["meanMS"] <= ps["total"]["meanMS"], ps
        parts = ps["nonlinearSetup"]["meanMS"] + ps["linearSolve"]["meanMS"] + ps["nonlinearResolve"]["meanMS"]
        assert parts <= ps["nonlinearIteration"]["meanMS"] * (1 + 1e-3), ps      # (the three parts tile the step: shared records leave no gap to count twice)
