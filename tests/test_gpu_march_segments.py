"""GPU: the marching PCG iteration without an A p plane (k_iter_march_rc, energy_image_warping_march_rc.hip) at every shape of its row loop.

The loop is specialised by phase (head, enter, S1, steady trips, an unrolled clamped tail); which instantiations a wave runs depends on the prefetch depth, the
segment's length, whether it ends at the image's last row and the delta mode (tests/march_classes.py restates the arithmetic).  The automatic rows per segment
reach only a few of those shapes, so here R is FORCED (thallo_hip_march_debug_set(0, R)) and swept:

  * bit for bit against the stored-plane marching kernel (energy_image_warping_march.hip: another row loop, the same forced R), every class a whole image can reach;
  * row slabs at depth 4 (R >= 24), ranks sharing the one GPU, both transports;
  * per pixel against a float64 PCG on the oracle's Jacobian -- the forms compared bit for bit share their stencil and sums, so a common error would cancel there.

tests/test_march_classes.py (no GPU) asserts that the lists below leave no reachable class out."""
import ctypes as C
import os

import numpy as np
import pytest

import thallo_amd
from thallo_amd import api, synthetic as syn
from helpers import to_device, to_host, copy_params
import march_classes as mc

pytestmark = pytest.mark.gpu

LIT = mc.SWEEP_LIT

# Bars of the float64 comparison: 4 x the larger of two yardsticks measured on the same inputs -- the CPU oracle's own float32 solve and the LDS-tiled kernel
# (THALLO_MARCH=0), each against the float64 PCG -- worst case over reference_cases() and the slab shapes; DESIGN.md section 5, table "float64 PCG yardsticks".
# Never derived from the marching kernel's output.  Quantities: max |change - change64| / max |change64| per unknown plane after ONE GN step of LIT iterations;
# max_k |alpha_k - alpha64_k| / |alpha64_k|, the same for beta_k.
BAR_OFFSET = 4 * 3.03e-5      # (oracle and tile kernel alike: the rounding of Offset + delta at coordinates up to 372, half an ulp of 3.05e-5 over a change of 0.5)
BAR_ANGLE = 4 * 1.01e-6
BAR_ALPHA = 4 * 3.69e-5       # (oracle; tile kernel 2.42e-5)
BAR_BETA = 4 * 6.89e-5        # (oracle; tile kernel 5.05e-5)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _instance(W, H):
    return syn.image_warping(W, H, n_markers=min(8, max(0, (W - 2) * (H - 2) // 4)), mask_disc=0.1 if min(W, H) > 8 else 0.0)


def _gn_steps(monkeypatch, p, W, H, nit, march, R=0, planes=None):
    """nit GN steps of LIT launches each, one launch per PCG iteration; returns costs, per-step (alpha_k, beta_k), the unknowns (device) and the kernel statistics"""
    L = thallo_amd.lib()
    monkeypatch.setenv("THALLO_RESIDENT", "0")
    monkeypatch.setenv("THALLO_MARCH", march)
    if planes is None: monkeypatch.delenv("THALLO_DELTA_PLANES", raising=False)
    else: monkeypatch.setenv("THALLO_DELTA_PLANES", str(planes))
    L.thallo_hip_march_debug_set(0, R)
    try:
        dev = to_device(copy_params(p))
        s = api.ThalloSolver((W, H), thallo_amd.energy_file("image_warping"))
        s.set_solver_parameters(nIterations=nit, lIterations=LIT)
        params = s.make_params(dev)
        s.init(params)
        costs, traces = [s.current_cost()], []
        while s.step(params):
            costs.append(s.current_cost()); traces.append(s.alpha_beta_trace())
        names = s.kernel_stats()
        s.close()
    finally:
        L.thallo_hip_march_debug_set(0, 0)
    return costs, traces, dev[0], dev[1], names


def test_model_follows_the_library_on_this_device(torch):
    """the automatic rows per segment (the search over workgroups per CU and the fill rule) on this device's CU count, against the model"""
    L = thallo_amd.lib()
    L.thallo_hip_iw_march_rows.restype = C.c_int
    L.thallo_hip_iw_march_rows.argtypes = [C.c_int, C.c_int]
    cus = L.thallo_hip_device_cu_count()
    assert cus > 0
    for W, H in [(2, 1), (124, 64), (126, 130), (372, 5), (640, 480), (1024, 768), (1200, 800), (2048, 256), (2048, 2048), (8192, 2048), (8192, 4096), (16384, 2048), (16384, 11264), (124 * 1024 + 2, 8)]:
        assert L.thallo_hip_iw_march_rows(W, H) == mc.pick_rows(W, H, cus), (W, H, cus)


# ------------------------------------------------------------------ bit for bit against the stored-plane kernel
@pytest.mark.parametrize("W,H,R,planes", mc.sweep_cases())
def test_forced_rows_sweep_is_bitwise_the_stored_plane_kernel(torch, monkeypatch, W, H, R, planes):
    """Costs, every alpha_k / beta_k and both unknown planes after two GN steps, recomputing kernel (THALLO_MARCH=2) against stored-plane kernel (THALLO_MARCH=4) at the
    same forced rows per segment.  The classes this case executes: march_classes.case_classes(W, H, R, planes, LIT)."""
    p = _instance(W, H)
    c0, t0, o0, a0, n0 = _gn_steps(monkeypatch, p, W, H, 2, "2", R, planes)
    c1, t1, o1, a1, n1 = _gn_steps(monkeypatch, p, W, H, 2, "4", R, planes)
    assert all(np.isfinite(c0)) and len(c0) == 3 and len(t0) == 2 and len(t0[0]) == LIT
    assert n0.get("PCGIteration", {}).get("launches") == 2 * LIT == n1.get("PCGIteration", {}).get("launches"), (n0, n1)
    assert t0 == t1, [(i, k) for i, (x, y) in enumerate(zip(t0, t1)) for k, (u, v) in enumerate(zip(x, y)) if u != v][:3]
    assert c0 == c1, (c0, c1)
    if not (torch.equal(o0, o1) and torch.equal(a0, a1)):
        rows = sorted(set(torch.nonzero((o0 != o1).any(-1) | (a0 != a1))[:, 0].tolist()))
        raise AssertionError(f"rows that differ: {rows[:12]}; segments {mc.segments(0, H, R)[-3:]}, depth {mc.depth(R)}")


# ------------------------------------------------------------------ per pixel against a float64 PCG
def _pcg64(orc, W, H, p):
    """ONE GN step of LIT PCG iterations in float64 on the oracle's Jacobian and residual: (delta, [(alpha_k, beta_k)], excluded)"""
    import scipy.sparse as sp
    pr = orc.Problem(orc.IMAGE_WARPING, (W, H), copy_params(p))
    rp, col, val, res = pr.csr()
    n = 3 * W * H
    J = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(len(res), n))
    excl = pr.excluded()
    _, pre = pr.eval_jtf()
    minv = np.where(excl, 0.0, 1.0 / (1.0 + np.sqrt(pre.astype(np.float64))) ** 2)      # guardedInvert, gauss_newton.t:638-648
    r = -(J.T @ res.astype(np.float64)); r[excl] = 0.0
    pk = minv * r
    aN = float(r @ pk)
    delta, ab = np.zeros(n), []
    for _ in range(LIT):
        Ap = J.T @ (J @ pk); Ap[excl] = 0.0
        aD = float(pk @ Ap)
        alpha = aN / aD if aD != 0.0 else 0.0
        delta += alpha * pk; r -= alpha * Ap
        z = minv * r
        bN = float(z @ r)
        beta = bN / aN if aN != 0.0 else 0.0
        pk = z + beta * pk
        ab.append((alpha, beta)); aN = bN
    return delta, np.array(ab), excl


def _deviation(W, H, p, off, ang, trace, ref, rows=None):
    """(Offset, Angle, alpha, beta) deviations of one float32 result from the float64 step; rows = (g0, g1): off / ang hold those rows only"""
    delta, ab, _ = ref
    N = W * H
    g0, g1 = rows if rows else (0, H)
    d_off = delta[:2 * N].reshape(H, W, 2); d_ang = delta[2 * N:].reshape(H, W)
    e_off = np.abs((off.astype(np.float64) - p[0][g0:g1]) - d_off[g0:g1]).max() / np.abs(d_off).max()
    e_ang = np.abs((ang.astype(np.float64) - p[1][g0:g1]) - d_ang[g0:g1]).max() / np.abs(d_ang).max()
    tr = np.array(trace, np.float64)
    assert tr.shape == ab.shape
    return e_off, e_ang, (np.abs(tr[:, 0] - ab[:, 0]) / np.abs(ab[:, 0])).max(), (np.abs(tr[:, 1] - ab[:, 1]) / np.abs(ab[:, 1])).max()


def _yardsticks(orc, monkeypatch, W, H, p, ref):
    """the reference side's own distance from float64: the CPU oracle's float32 solve and the tile kernel"""
    po = copy_params(p)
    _, tr = orc.Problem(orc.IMAGE_WARPING, (W, H), po).solve(nIterations=1, lIterations=LIT, want_trace=True)
    dev_orc = _deviation(W, H, p, po[0], po[1], tr, ref)
    _, t, o, a, _ = _gn_steps(monkeypatch, p, W, H, 1, "0")
    dev_tile = _deviation(W, H, p, to_host(o), to_host(a), t[0], ref)
    return dev_orc, dev_tile


BARS = (BAR_OFFSET, BAR_ANGLE, BAR_ALPHA, BAR_BETA)
_fmt = lambda d: " ".join(f"{x:.3e}" for x in d)


@pytest.mark.parametrize("W,H,R,planes", mc.reference_cases())
def test_forced_rows_against_a_float64_pcg(torch, orc, monkeypatch, W, H, R, planes):
    """One GN step of LIT iterations: the change of both unknown planes per pixel and every alpha_k, beta_k against a float64 PCG on the oracle's Jacobian, within 4 x
    what the reference side itself (CPU oracle in float32, tile kernel) is away from it; masked unknowns bit-untouched.  Every class of the sweep once."""
    p = _instance(W, H)
    ref = _pcg64(orc, W, H, p)
    dev_orc, dev_tile = _yardsticks(orc, monkeypatch, W, H, p, ref)
    _, t, o, a, names = _gn_steps(monkeypatch, p, W, H, 1, "2", R, planes)
    off, ang = to_host(o), to_host(a)
    dev = _deviation(W, H, p, off, ang, t[0], ref)
    print(f"MARCHREF {W}x{H} R={R} planes={planes}: oracle {_fmt(dev_orc)} | tile {_fmt(dev_tile)} | march {_fmt(dev)}")
    assert names.get("PCGIteration", {}).get("launches") == LIT, names
    assert all(y <= b for y, b in zip(dev_orc, BARS)), ("the bars are below the oracle's own deviation: measure again (DESIGN.md section 5)", dev_orc, BARS)
    excl = ref[2]; N = W * H
    assert np.array_equal(off.reshape(-1)[excl[:2 * N]], p[0].reshape(-1)[excl[:2 * N]]) and np.array_equal(ang.reshape(-1)[excl[2 * N:]], p[1].reshape(-1)[excl[2 * N:]])
    assert all(d <= b for d, b in zip(dev, BARS)), (dev, BARS)


# ------------------------------------------------------------------ row slabs at depth 4
def _slab_worker(rank, world, port, W, H, lit, q, device_exchange, rows, counts):
    """test_gpu_distributed._worker, one launch per PCG iteration of the marching kernels with `rows` rows per segment, on an explicit split of the image"""
    import torch  # noqa: F401  (before libThallo.so: the HIP runtime torch ships must be the one that gets loaded)
    import thallo_amd.distributed as D
    from test_gpu_distributed import _worker
    os.environ["THALLO_RESIDENT"] = "0"
    os.environ["THALLO_MARCH"] = "2"
    thallo_amd.lib().thallo_hip_march_debug_set(0, rows)
    D.image_warping_slab_counts = lambda W_, H_, world_: list(counts)
    _worker(rank, world, port, W, H, 1, lit, q, device_exchange)


def _run_slabs(world, W, counts, R, device_exchange):
    import torch.multiprocessing as mp
    from test_gpu_distributed import _collect, _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_slab_worker, args=(r, world, port, W, sum(counts), LIT, q, device_exchange, R, counts)) for r in range(world)]
    for p_ in procs:
        p_.start()
    return sorted(_collect(q, procs, world), key=lambda t: t[0])


@pytest.mark.parametrize("world,W,counts,R", mc.SLAB_CASES)
def test_slabs_at_depth_4_agree_across_transports_and_with_a_float64_pcg(torch, orc, monkeypatch, world, W, counts, R):
    """Row slabs with R >= 24 (what a real multi-GPU slab of a large image gets): ghost-row clamps and the stores of rows row0 / row1 - 1 of A p_k inside tail steps.
    Short and full last segments on ranks with a ghost row below and on the bottom rank; device-side transport (peer stores) and all-gather transport (A p plane).
    No distributed error, the same alpha / beta bits and costs on every rank, the transports bit-identical on the owned unknowns, the owned rows within the
    float64 bars."""
    assert mc.depth(R) == 4 and all(mc.grid(W, *mc.slab_layout(counts, r)[1:], R, deferred=True) <= mc.MAX_PARTIALS for r in range(world))
    H = sum(counts)
    a = _run_slabs(world, W, counts, R, True)
    b = _run_slabs(world, W, counts, R, False)
    p = syn.image_warping(W, H, n_markers=8)          # (the workers' instance)
    ref = _pcg64(orc, W, H, p)
    dev_orc, dev_tile = _yardsticks(orc, monkeypatch, W, H, p, ref)
    assert all(y <= bar for y, bar in zip(dev_orc, BARS)), (dev_orc, BARS)
    g = 0
    for ra, rb in zip(a, b):
        rank, costs, g0, g1, off, ang, info, err, trace, stats = ra
        assert (g0, g1) == (g, g + counts[rank]) == (rb[2], rb[3]); g = g1
        assert info["exchange"] == "p2p-mailbox" and rb[6]["exchange"] == "allgather", (info, rb[6])
        assert err == 0 and rb[7] == 0, (rank, info)
        assert np.isfinite(costs).all() and len(trace) == LIT
        assert stats["PCGIteration"]["launches"] >= LIT and rb[9]["PCGIteration"]["launches"] >= LIT, (stats, rb[9])
        assert trace == a[0][8] == rb[8] and costs == a[0][1] == rb[1]
        assert (off == rb[4]).all() and (ang == rb[5]).all(), f"rank {rank}: the transports differ on rows {sorted(set(np.nonzero((off != rb[4]).any(-1) | (ang != rb[5]))[0] + g0))[:8]}"
        dev = _deviation(W, H, p, off, ang, trace, ref, rows=(g0, g1))
        print(f"MARCHREF slab {W}x{H} counts={counts} R={R} rank {rank}: oracle {_fmt(dev_orc)} | tile {_fmt(dev_tile)} | march {_fmt(dev)}")
        assert all(d <= bar for d, bar in zip(dev, BARS)), (rank, dev, BARS)


# ------------------------------------------------------------------ the slab iteration whose last workgroup is the exchange
def _slab_worker_budget(rank, world, port, W, H, lit, q, rows, counts, cap):
    """_slab_worker on the device-side transport with the marching kernels' workgroup budget forced to `cap` (0: the device's)"""
    import torch  # noqa: F401  (before libThallo.so: the HIP runtime torch ships must be the one that gets loaded)
    thallo_amd.lib().thallo_hip_march_debug_set(6, cap)
    _slab_worker(rank, world, port, W, H, lit, q, True, rows, counts)


def test_launch_end_exchange_of_the_recomputing_kernel_is_bitwise_the_deferred_cross_rank_finish(torch):
    """The recomputing kernel on a slab with the scalar exchange at the END of its launch (tickets, the last workgroup trades the sums) is what a rank runs
    where the deferred cross-rank finish does not fit the device; every other slab test here fits, so a budget of 8 workgroups is forced: the launch of 8 workgroups
    plus the deferred form's 8 extra ones no longer fits, thallo_hip_iw_march_rc_deferred_fits says 0 on every rank.  One GN step on 128 x 32 split 16 + 16 with R = 8
    (two column strips, two row segments per rank), bit for bit against the same run under the device's own budget -- the deferred finish, which leaves one
    PCGScalars launch per GN step behind (the finish of the last iteration) where the launch-end exchange leaves none."""
    import torch.multiprocessing as mp
    from test_gpu_distributed import _collect, _free_port
    world, W, counts, R = 2, 128, (16, 16), 8
    runs = []
    for cap in (0, 8):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_slab_worker_budget, args=(r, world, port, W, sum(counts), LIT, q, R, counts, cap)) for r in range(world)]
        for p_ in procs:
            p_.start()
        runs.append(sorted(_collect(q, procs, world), key=lambda t: t[0]))
    for ra, rb in zip(*runs):
        print(f"SLABFORMS rank {ra[0]}: deferred {sorted(ra[9])} | launch end {sorted(rb[9])}")
        assert ra[6]["exchange"] == "p2p-mailbox" and rb[6]["exchange"] == "p2p-mailbox" and ra[7] == 0 and rb[7] == 0, (ra[6], rb[6])
        assert ra[9]["PCGIteration"]["launches"] >= LIT and rb[9]["PCGIteration"]["launches"] >= LIT
        assert "PCGScalars" in ra[9] and "PCGScalars" not in rb[9], (sorted(ra[9]), sorted(rb[9]))
        assert np.isfinite(ra[1]).all() and len(ra[8]) == LIT
        assert ra[8] == rb[8] and ra[1] == rb[1]
        assert (ra[4] == rb[4]).all() and (ra[5] == rb[5]).all()
