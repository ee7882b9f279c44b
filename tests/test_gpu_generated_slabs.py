"""GPU: row slabs of GENERATED energies (thallo_amd/distributed_generated.py; the front-end's row-slab unit in solver_dist.cpp's flat form).  The box
has one GPU, so the ranks share cuda:0 and talk over gloo, as in test_gpu_distributed.py; the compute path is the real one.  Bundled files run
generated under THALLO_FRONTEND=generate, set in each worker before the library loads."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS_E = os.path.join(ROOT, "tests", "energies")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _problem(name, W, H):
    from thallo_amd import synthetic as syn
    rng = np.random.default_rng(7)
    if name == "laplacian_image":
        return syn.laplacian_image(W, H), [W, H]
    if name == "shape_from_shading":
        return syn.shape_from_shading(W, H), [W, H]
    if name == "image_warping":
        return syn.image_warping(W, H, n_markers=8), [W, H]
    if name == "gradient_paste":
        T = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
        X = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
        M = np.zeros((H, W), np.float32)
        M[:, :3] = 1; M[:, -3:] = 1; M[:2] = 1; M[-2:] = 1; M[H // 2 - 3:H // 2 + 2, W // 3:W // 3 + 6] = 1      # border + an island across a slab boundary
        return [X, T, M], [W, H]
    if name == "conv2d_wide":
        X = rng.uniform(0, 1, (H, W)).astype(np.float32)
        B = rng.uniform(0, 1, (H, W)).astype(np.float32)
        K = rng.uniform(0, 1, (11, 11)).astype(np.float32); K /= K.sum()
        return [X, B, K], [W, H, 11, 11]
    raise ValueError(name)


def _path(name):
    from thallo_amd import api
    return os.path.join(TESTS_E, name + ".t") if name in ("gradient_paste", "conv2d_wide") else api.energy_file(name)


def _worker(rank, world, port, name, W, H, nit, lit, lm, device_exchange, handwritten, q):
    if not handwritten:
        os.environ["THALLO_FRONTEND"] = "generate"          # (before the library loads)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p, dims = _problem(name, W, H)
        extra = {"q_tolerance": 0.05} if lm else {}
        try:
            if handwritten:
                from thallo_amd.distributed_sfs import PlanSfsSlabSolver
                s = PlanSfsSlabSolver(p, W, H, rank, world, lit, lm=lm, device_exchange=device_exchange)
            else:
                from thallo_amd.distributed_generated import PlanGeneratedSlabSolver
                s = PlanGeneratedSlabSolver(_path(name), dims, p, rank, world, lit, lm=lm, device_exchange=device_exchange)
        except (RuntimeError, ValueError) as e:
            q.put((rank, "refused", str(e)))
            return
        costs = s.solve(nit, **extra)
        q.put((rank, costs, s.lay.g0, s.lay.g1, s.owned(), s.solver.distributed_info(), s.solver.energy_name))
        s.solver.close()
    finally:
        dist.destroy_process_group()


def _run(world, name, W, H, nit, lit, lm=False, device_exchange=True, handwritten=False, limit=120.0):
    import queue as _queue
    import time as _time
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, W, H, nit, lit, lm, device_exchange, handwritten, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    res, t0 = [], _time.time()
    while len(res) < world:
        try:
            res.append(q.get(timeout=1.0))
        except _queue.Empty:
            dead = [p_.exitcode for p_ in procs if p_.exitcode not in (None, 0)]
            if dead or _time.time() - t0 > limit:
                for p_ in procs:
                    if p_.is_alive():
                        p_.terminate()
                raise AssertionError(f"ranks failed or hung: exit codes {[p_.exitcode for p_ in procs]}")
    for p_ in procs:
        p_.join(timeout=30)
        assert p_.exitcode == 0
    res.sort(key=lambda t: t[0])
    for r in res:
        assert r[1] != "refused", r
    for r in res:
        assert r[6].startswith("generated") != handwritten, r[6]
        assert r[1] == res[0][1], ("costs differ between ranks", r[1], res[0][1])
    return res


def _whole(name, W, H, nit, lit):
    """the whole-image generated plan on one GPU (no slabs)"""
    import torch
    from thallo_amd import api
    p, dims = _problem(name, W, H)
    dev = [torch.from_numpy(x.copy()).cuda() if isinstance(x, np.ndarray) else x for x in p]
    s = api.ThalloSolver(tuple(dims), _path(name), timing_level=0)
    final, costs = s.solve(dev, profiled=True, nIterations=nit, lIterations=lit)
    X = dev[0].cpu().numpy()
    s.close()
    return costs, X, p


def _laplacian_oracle(orc, W, H, nit, lit):
    from thallo_amd import synthetic as syn
    p = syn.laplacian_image(W, H)
    po = [x.copy() for x in p]
    co, _ = orc.Problem(orc.LAPLACIAN_IMAGE, (W, H), po, fconst=[0.2], iconst=[1]).solve(nIterations=nit, lIterations=lit)
    return co, po[0]


def test_generated_laplacian_slabs_match_oracle_and_both_transports_agree_bitwise(orc):
    """generated laplacian_image, world 3 (g = 1): the oracle's trajectory; the device-side and all-gather transports give the same bits"""
    W, H, nit, lit = 64, 48, 3, 8
    a = _run(3, "laplacian_image", W, H, nit, lit, device_exchange=True)
    b = _run(3, "laplacian_image", W, H, nit, lit, device_exchange=False)
    co, Xo = _laplacian_oracle(orc, W, H, nit, lit)
    for (rank, costs, g0, g1, X, info, _), (_, costs_b, _, _, X_b, info_b, _) in zip(a, b):
        assert info["exchange"] == "p2p-rows" and info_b["exchange"] == "allgather", (info, info_b)
        assert (np.abs(np.array(costs) - co) <= 2e-5 * np.abs(co) + 1e-9).all(), (rank, costs, co)
        assert np.abs(X - Xo[g0:g1]).max() <= 2e-5
        assert costs == costs_b and np.array_equal(X, X_b), rank


def test_generated_laplacian_single_slab_matches_oracle(orc):
    W, H, nit, lit = 64, 48, 3, 8
    (rank, costs, g0, g1, X, info, _), = _run(1, "laplacian_image", W, H, nit, lit)
    co, Xo = _laplacian_oracle(orc, W, H, nit, lit)
    assert (np.abs(np.array(costs) - co) <= 2e-5 * np.abs(co) + 1e-9).all(), (costs, co)
    assert np.abs(X - Xo).max() <= 2e-5


def test_generated_sfs_slabs_gauss_newton_match_oracle_and_the_handwritten_slabs(orc):
    """generated shape_from_shading (g = 2, global pixel coordinates and borders), GN at world 2: the oracle and PlanSfsSlabSolver at the same world"""
    from thallo_amd import synthetic as syn
    W, H, nit, lit = 64, 64, 3, 10
    gen = _run(2, "shape_from_shading", W, H, nit, lit)
    hand = _run(2, "shape_from_shading", W, H, nit, lit, handwritten=True)
    p = syn.shape_from_shading(W, H)
    co, _ = orc.Problem(orc.SFS, (W, H), p).solve(nIterations=nit, lIterations=lit)
    for (rank, costs, g0, g1, X, info, _), (_, costs_h, _, _, X_h, _, _) in zip(gen, hand):
        assert "2 ghost rows" in info["form"], info
        assert (np.abs(np.array(costs) - co) <= 2e-5 * np.abs(co) + 1e-9).all(), (rank, costs, co)
        assert (np.abs(np.array(costs) - np.array(costs_h)) <= 2e-5 * np.abs(np.array(costs_h)) + 1e-9).all(), (rank, costs, costs_h)
        assert np.abs(X - p[16][g0:g1]).max() <= 2e-5
        assert np.abs(X - X_h).max() <= 2e-5


def test_generated_sfs_slabs_levenberg_marquardt_match_oracle_on_both_transports(orc):
    """the LM branch on generated slabs, world 3: the oracle's LM trajectory (the bar and trajectory-length rule of the hand-written slab tests); the
    all-gather transport agrees with the device-side one to 2e-5"""
    from thallo_amd import synthetic as syn
    W, H, nit, lit = 64, 96, 4, 10
    a = _run(3, "shape_from_shading", W, H, nit, lit, lm=True, device_exchange=True)
    b = _run(3, "shape_from_shading", W, H, nit, lit, lm=True, device_exchange=False)
    p = syn.shape_from_shading(W, H)
    co, _ = orc.Problem(orc.SFS, (W, H), p).solve(nIterations=nit, lIterations=lit, use_lm=1, q_tolerance=0.05)
    for (rank, costs, g0, g1, X, info, _), (_, costs_b, _, _, X_b, _, _) in zip(a, b):
        m = min(len(costs), len(co))
        assert m >= 3 and abs(len(costs) - len(co)) <= 1, (costs, co)
        assert (np.abs(np.array(costs[:m]) - co[:m]) <= 2e-4 * np.abs(co[:m])).all(), (rank, costs, co)
        assert np.abs(X - p[16][g0:g1]).max() <= 2e-4
        assert len(costs) == len(costs_b) and np.abs(np.array(costs) - np.array(costs_b)).max() <= 2e-5 * np.abs(np.array(costs_b)).max(), (rank, costs, costs_b)


def test_generated_gradient_paste_slabs_match_the_whole_image_plan():
    """float4 unknowns with Exclude: costs to 1e-5 relative and unknowns to 1e-5 of the whole-image generated plan; excluded pixels are bit-untouched"""
    W, H, nit, lit = 64, 48, 3, 10
    res = _run(2, "gradient_paste", W, H, nit, lit)
    cw, Xw, p = _whole("gradient_paste", W, H, nit, lit)
    M = p[2]
    for rank, costs, g0, g1, X, info, _ in res:
        assert (np.abs(np.array(costs) - np.array(cw)) <= 1e-5 * np.abs(np.array(cw)) + 1e-9).all(), (rank, costs, cw)
        assert np.abs(X - Xw[g0:g1]).max() <= 1e-5 * max(1.0, np.abs(Xw).max())
        ex = M[g0:g1] != 0
        assert ex.any() and np.array_equal(X[ex], p[0][g0:g1][ex]), rank


def test_generated_conv2d_wide_slabs_match_the_whole_image_plan():
    """the 11 x 11 deconvolution, g = 10, world 3 (slab boundaries at rows 16 and 32, inside the InBoundsExpanded(x, y, 5) band): costs to 1e-5 relative and
    unknowns to 1e-5 (relative to their largest magnitude) of the whole-image generated plan"""
    W, H, nit, lit = 64, 48, 2, 6
    res = _run(3, "conv2d_wide", W, H, nit, lit)
    cw, Xw, p = _whole("conv2d_wide", W, H, nit, lit)
    assert [r[2] for r in res] == [0, 16, 32]
    for rank, costs, g0, g1, X, info, _ in res:
        assert "10 ghost rows" in info["form"], info
        assert (np.abs(np.array(costs) - np.array(cw)) <= 1e-5 * np.abs(np.array(cw)) + 1e-9).all(), (rank, costs, cw)
        assert np.abs(X - Xw[g0:g1]).max() <= 1e-5 * max(1.0, np.abs(Xw).max())      # (both sides scatter the wide residual with float atomics: equal to rounding)


def test_generated_image_warping_is_refused_on_every_rank():
    """two unknown arrays (Offset, Angle): no row-slab form; both ranks return the same error, nobody waits on the other"""
    import torch.multiprocessing as mp
    import queue as _queue
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, "image_warping", 64, 48, 2, 4, False, True, False, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = []
    try:
        for _ in range(2):
            res.append(q.get(timeout=90.0))
    except _queue.Empty:
        pass
    for p_ in procs:
        p_.join(timeout=30)
        if p_.is_alive():
            p_.terminate()
    assert len(res) == 2, res
    res.sort(key=lambda t: t[0])
    assert all(r[1] == "refused" for r in res), res
    assert res[0][2] == res[1][2] and "more than one Unknown" in res[0][2], res
