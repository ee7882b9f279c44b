"""The lean head of a marching Gauss-Newton step (csrc/solver.cpp step_gn_one_kernel `lean`): thallo_hip_iw_pcg_init with pre, z and p_prev NULL stores none of the
three, and the step's first launch (the stored-plane marching kernel, mode bit 0) neither loads p_{-1} nor -- with Ap_out NULL -- stores A p_0.

Kernel level, W in {2, 126, 250} x H in {2, 7, 37} with a masked disc and one active pixel cut off from its neighbours (r_0 = -0.0f and M^-1 = 0 there: p_0 must
stay +0.0f, the bare product would be -0.0f) and 35 rows per segment forced through thallo_hip_march_debug_set, so that 37 rows are two segments:
  * the lean init against the full one: r, cs, flags, the alphaN partials and the irregular word bit for bit, the three sentinel planes untouched;
  * the lean first launch (p_in a plane of NaN sentinels, no Ap_out) behind the lean init against the full launch behind the full init: r_0 as copied, p_0 and
    every partial sum bit for bit; the sentinel plane handed in as Ap_in untouched.
Solver level: THALLO_AB=lean_head=0 (every plane kept) against the default, bit for bit after three GN steps."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import shim_kernels as sk
from shim_kernels import F32
import thallo_amd
from thallo_amd import api, synthetic as syn
from helpers import to_device, copy_params, set_ab

pytestmark = pytest.mark.gpu

TAIL = 64
PSLOTS = sk.MAX_PARTIALS + 8
ROWS = 35


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


@pytest.fixture(autouse=True)
def _rows_back(L):
    try:
        yield
    finally:
        L.thallo_hip_march_debug_set(0, 0)


def _host(t):
    return t.cpu().numpy()


def _params(W, H):
    """image_warping with a masked disc in the middle and pixel (0, 0) cut off from its two neighbours: an active pixel without a valid pair and without a
    constraint has J^T F = 0, so r_0 = -0.0f and M^-1 = 0 there -- the signed zero the first launch must turn into p_0 = +0.0f"""
    p = syn.image_warping(W, H, n_markers=min(8, max(0, (W - 2) * (H - 2) // 4)), mask_disc=0.0)
    ys, xs = np.mgrid[0:H, 0:W]
    p[4][(xs - W / 2.0) ** 2 + (ys - H / 2.0) ** 2 < max(0.3 * min(W, H), 0.8) ** 2] = 255.0
    p[4][0, 1] = p[4][1, 0] = 255.0
    p[4][0, 0] = 0.0
    p[3][0, 0] = -1.0                                         # (no constraint on the cut-off pixel)
    assert (p[4] != 0).any() and (p[4] == 0).any(), "the case needs masked and unmasked pixels"
    return p


def _problem(torch, W, H):
    p = _params(W, H)
    tail = lambda a: np.concatenate([np.ascontiguousarray(a, F32).reshape(-1), np.full(TAIL, sk.CANARY, np.uint32).view(F32)])
    # params as image_warping.t lists them: Offset, Angle, UrShape, Constraints, Mask, w_fit, w_reg
    return SimpleNamespace(W=W, H=H, N=W * H, wf=F32(p[5]), wr=F32(p[6]), bufs=[sk.dbuf(torch, tail(a)) for a in p[:5]])


def _init(torch, L, q, lean):
    N = q.N
    o = SimpleNamespace(**{k: sk.canary_buf(torch, 3 * N + TAIL) for k in ("r", "pre", "z", "p_prev")})
    o.cs, o.aN = sk.canary_buf(torch, 2 * N + TAIL), sk.canary_buf(torch, PSLOTS)
    o.flags = sk.dbuf(torch, np.full((N + 3) // 4 * 4 + 64, 0xA5, np.uint8))
    o.irr = sk.dbuf(torch, np.full(16, 0x5A5A5A5A, np.int32))
    off, ang, ur, cons, mask = (b.data_ptr() for b in q.bufs)
    o.rc = L.thallo_hip_iw_pcg_init(q.W, q.H, 0, q.H, off, ang, ur, cons, mask, q.wf, q.wr, o.r.data_ptr(),
                                    None if lean else o.pre.data_ptr(), None if lean else o.z.data_ptr(), None if lean else o.p_prev.data_ptr(), None,
                                    o.cs.data_ptr(), o.flags.data_ptr(), None, o.irr.data_ptr(), o.aN.data_ptr(), None)
    torch.cuda.synchronize()
    assert o.rc > 0, o.rc
    return o


def _first_launch(torch, L, q, o, lean):
    N = q.N
    f = SimpleNamespace(r_out=sk.canary_buf(torch, 3 * N + TAIL), p_out=sk.canary_buf(torch, 3 * N + TAIL), Ap_out=sk.canary_buf(torch, 3 * N + TAIL),
                        Ap_in=sk.canary_buf(torch, 3 * N + TAIL), aD=sk.canary_buf(torch, PSLOTS), s12=sk.canary_buf(torch, 3 * PSLOTS, np.float64))
    aN = sk.dbuf(torch, np.array([1.0], F32))
    a = sk.IwIterT()
    a.W, a.H, a.row0, a.row1 = q.W, q.H, 0, q.H
    a.cs, a.urshape, a.flags, a.irregular = o.cs.data_ptr(), q.bufs[2].data_ptr(), o.flags.data_ptr(), o.irr.data_ptr()
    a.pre = None if lean else o.pre.data_ptr()
    a.w_fit, a.w_reg = q.wf, q.wr
    a.r_in, a.r_out, a.p_in, a.p_out, a.mode = o.r.data_ptr(), f.r_out.data_ptr(), o.p_prev.data_ptr(), f.p_out.data_ptr(), 1      # (lean: p_prev is all sentinels)
    a.Ap_in = f.Ap_in.data_ptr()
    a.Ap_out = None if lean else f.Ap_out.data_ptr()
    a.alphaN_prev = sk.sumt(aN)
    a.alphaD_out, a.s12_out = f.aD.data_ptr(), f.s12.data_ptr()
    f.rc = L.thallo_hip_iw_pcg_iter(sk.IW_ITER_MARCH, C.byref(a), None)
    torch.cuda.synchronize()
    assert f.rc > 0, f.rc
    return f


@pytest.mark.parametrize("H", [2, 7, 37])
@pytest.mark.parametrize("W", [2, 126, 250])
def test_lean_init_and_first_launch_leave_the_full_ones_bits(torch, L, W, H):
    q = _problem(torch, W, H)
    N = q.N
    full, lean = _init(torch, L, q, False), _init(torch, L, q, True)
    assert full.rc == lean.rc
    for k in ("r", "cs", "flags", "aN", "irr"):
        assert sk.same_bytes(_host(getattr(full, k)), _host(getattr(lean, k))), k
    assert _host(full.irr)[0] == 0 and (_host(full.irr)[1:] == 0x5A5A5A5A).all()
    for k in ("pre", "z", "p_prev"):
        assert (_host(getattr(lean, k)).view(np.uint32) == sk.CANARY).all(), f"{k} was written although it was not given"
    assert (_host(full.p_prev)[:3 * N] == 0).all()
    r0 = _host(full.r)[:3 * N]
    assert (np.signbit(r0) & (r0 == 0)).any(), "the case has no r_0 = -0.0f"
    # ---- the first launch
    L.thallo_hip_march_debug_set(0, ROWS)                    # (37 rows: a segment of 35 and one of 2)
    ff, fl = _first_launch(torch, L, q, full, False), _first_launch(torch, L, q, lean, True)
    assert ff.rc == fl.rc
    for k in ("r_out", "p_out", "aD", "s12"):
        assert sk.same_bytes(_host(getattr(ff, k)), _host(getattr(fl, k))), k
    p0 = _host(fl.p_out)[:3 * N]
    assert np.isfinite(p0).all() and not (np.signbit(p0) & (p0 == 0) & (r0 == 0)).any(), "a p_0 = -0.0f where r_0 is a zero"
    assert sk.written_slots(_host(fl.aD)) == fl.rc
    for f in (ff, fl):
        assert (_host(f.Ap_in).view(np.uint32) == sk.CANARY).all(), "Ap_in was touched"
    assert (_host(fl.Ap_out).view(np.uint32) == sk.CANARY).all()
    assert np.isfinite(_host(ff.Ap_out)[:3 * N]).all()
    assert (_host(lean.p_prev).view(np.uint32) == sk.CANARY).all() and sk.same_bytes(_host(lean.r), _host(full.r))


@pytest.mark.parametrize("W,H,lit", [(250, 70, 2), (250, 70, 5), (132, 40, 40), (250, 70, 100)])
def test_lean_head_step_is_bitwise_the_full_head(torch, monkeypatch, W, H, lit):
    p = syn.image_warping(W, H, n_markers=8, mask_disc=0.1)
    monkeypatch.setenv("THALLO_RESIDENT", "0")
    monkeypatch.setenv("THALLO_MARCH", "2")
    monkeypatch.delenv("THALLO_DELTA_PLANES", raising=False)
    runs = []
    for lean in (None, "0"):
        set_ab(monkeypatch, lean_head=lean)
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
    assert all(np.isfinite(c0)) and len(c0) == 4 and len(t0[0]) == lit
    assert n0 == n1, (n0, n1)
    assert t0 == t1, [(i, k) for i, (x, y) in enumerate(zip(t0, t1)) for k, (u, v) in enumerate(zip(x, y)) if u != v][:3]
    assert c0 == c1, (c0, c1)
    assert torch.equal(o0, o1) and torch.equal(a0, a1)
