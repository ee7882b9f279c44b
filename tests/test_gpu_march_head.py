"""GPU: the head of a marching PCG launch.  Both marching kernels request the word pcg_init wrote (`irregular`) first and look at it later; the recomputing
kernel (k_iter_march_rc) has the loads of its first rows -- and of iteration k-1's partial sums -- in flight by then.  What must not have changed:

  * word set: no store to r_out / p_out / delta (or the A p plane), the workgroups' partials and the two scalar words poisoned, the call returns;
  * word cleared: finite outputs, the two kernels bit for bit on r, p, delta, and the words the recomputing kernel leaves behind are the finished sums' bits
    -- on a grid of 8 workgroups and on one of 272 (more partial slots than the four per lane that are requested ahead);
  * a short slab (two ranks, 16 + 16 rows of 128 x 32 at 8 rows per segment): the exchange wave of the deferred cross-rank finish still waits for what it needs --
    all-gather and device-side transport agree bit for bit.

The launches go through thallo_hip_iw_pcg_iter directly, one block per launch, with the rows per segment forced (thallo_hip_march_debug_set(0, R))."""
import ctypes as C

import numpy as np
import pytest

import thallo_amd
from thallo_amd import api, synthetic as syn
from helpers import to_device
import march_classes as mc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.6789          # prefilled into every plane a poisoned launch must not touch


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


class _Problem:
    """image_warping W x H after pcg_init (r_0, p_0 = M^-1 r_0, the alphaN_0 partials, cos / sin, the flags bytes) and the buffers of single launches"""

    def __init__(self, torch, W, H):
        L = thallo_amd.lib()
        self.L, self.torch, self.W, self.H = L, torch, W, H
        self.p = p = syn.image_warping(W, H, n_markers=6)
        N = W * H
        self.n = 3 * N
        self.na = L.thallo_hip_vector_elems(self.n)
        self.dev = dev = to_device(p)
        self.r0, pre, z, self.p0, self.delta0 = [self.vec() for _ in range(5)]
        self.cs = torch.zeros(2 * N, dtype=torch.float32, device="cuda")
        self.flags = torch.zeros(N + 256, dtype=torch.uint8, device="cuda")
        self.aN0 = torch.zeros(1024, dtype=torch.float32, device="cuda")
        self.irregular = torch.zeros(16, dtype=torch.int32, device="cuda")
        vp, fl = C.c_void_p, C.c_float
        self.nb0 = L.thallo_hip_iw_pcg_init(W, H, 0, H, vp(dev[0].data_ptr()), vp(dev[1].data_ptr()), vp(dev[2].data_ptr()), vp(dev[3].data_ptr()),
                                            vp(dev[4].data_ptr()), fl(p[5]), fl(p[6]), vp(self.r0.data_ptr()), vp(pre.data_ptr()), vp(z.data_ptr()),
                                            vp(self.p0.data_ptr()), vp(self.delta0.data_ptr()), vp(self.cs.data_ptr()), vp(self.flags.data_ptr()), None,
                                            vp(self.irregular.data_ptr()), vp(self.aN0.data_ptr()), None)
        assert self.nb0 > 0
        torch.cuda.synchronize()
        assert int(self.irregular[0].item()) == 0

    def vec(self, fill=0.0):
        return self.torch.full((self.na,), fill, dtype=self.torch.float32, device="cuda")

    def launch(self, kernel, mode, r_in, p_in, A_in, out, sums, prev=None, aD_prev=None, bN_prev=None):
        """one launch; out = (r_out, p_out, A_out, delta), sums = (alphaD partials, s12 partials); the deferred form with `prev`, else the two finished words"""
        a = api.IwIterT(W=self.W, H=self.H, row0=0, row1=self.H, cs=self.cs.data_ptr(), flags=self.flags.data_ptr(), irregular=self.irregular.data_ptr(),
                        w_fit=float(self.p[5]), w_reg=float(self.p[6]), r_in=r_in.data_ptr(), r_out=out[0].data_ptr(), p_in=p_in.data_ptr(), p_out=out[1].data_ptr(),
                        Ap_in=A_in.data_ptr() if A_in is not None else None, Ap_out=out[2].data_ptr(), delta=out[3].data_ptr(), mode=mode,
                        alphaN_prev=api.SumT(self.aN0.data_ptr(), self.nb0), alphaD_out=sums[0].data_ptr(), s12_out=sums[1].data_ptr())
        if prev is not None:
            a.prev = C.pointer(prev)
        elif aD_prev is not None:
            a.alphaD_prev, a.betaN_prev = api.SumT(aD_prev, 1), api.SumT(bN_prev, 1)
        nb = self.L.thallo_hip_iw_pcg_iter(kernel, C.byref(a), None)
        self.torch.cuda.synchronize()           # ("the call returns": a launch that faulted or hung would not get past this)
        return nb

    def sums(self, fill=0.0):
        return (self.torch.full((1024,), fill, dtype=self.torch.float32, device="cuda"), self.torch.full((3 * 1024,), fill, dtype=self.torch.float64, device="cuda"))


def _same_bits(torch, a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _first_iteration(P):
    """iteration 0 of a GN step on the stored-plane kernel (plain form: partials only) and the two words thallo_hip_iw_pcg_iter_finish makes of them"""
    torch = P.torch
    out = (P.vec(), P.vec(), P.vec(), P.delta0.clone())
    sums = P.sums()
    nb = P.launch(api.IW_ITER_MARCH, 1, P.r0, P.p0, None, out, sums)
    assert nb > 0, nb
    words = torch.zeros(16, dtype=torch.float32, device="cuda")
    vp = C.c_void_p
    assert P.L.thallo_hip_iw_pcg_iter_finish(vp(sums[0].data_ptr()), vp(sums[1].data_ptr()), nb, api.SumT(P.aN0.data_ptr(), P.nb0),
                                             vp(words.data_ptr()), vp(words.data_ptr() + 4), None) == 0
    torch.cuda.synchronize()
    return out, sums, nb, words


@pytest.fixture(scope="module")
def forced_rows():
    """rows per wave segment forced for the calls of a test, automatic again behind it"""
    L = thallo_amd.lib()

    def force(R):
        L.thallo_hip_march_debug_set(0, R)
    yield force
    L.thallo_hip_march_debug_set(0, 0)


@pytest.mark.parametrize("W,H,R", [(128, 32, 8), (2048, 64, 1)])
def test_word_cleared_the_two_kernels_agree_bit_for_bit(torch, forced_rows, W, H, R):
    """iteration 1 of a GN step: the recomputing kernel in the deferred form (it adds up iteration 0's partials itself -- requested behind its first rows' loads --
    and leaves the two words behind) against the stored-plane kernel started from the finished words.  128 x 32 at R = 8: 8 workgroups (the poison test's shape);
    2048 x 64 at R = 1: 17 strips x 16 bands = 272 workgroups, so a lane adds four slots requested ahead and one more from the loop."""
    forced_rows(R)
    try:
        grid = mc.grid(W, 0, H, R)
        assert grid == (8 if W == 128 else 272)
        P = _Problem(torch, W, H)
        out0, sums0, nb, words = _first_iteration(P)
        assert nb == grid
        r1, p1, A1, d0 = out0
        assert all(bool(torch.isfinite(t).all()) for t in (r1, p1, A1, words[:2]))
        # recomputing kernel, deferred form (mode 0: delta += alpha_0 p_0 in the launch)
        left = torch.zeros(16, dtype=torch.float32, device="cuda")
        prev = api.PrevT(sums0[0].data_ptr(), sums0[1].data_ptr(), nb, left.data_ptr(), left.data_ptr() + 4)
        out_rc, sums_rc = (P.vec(), P.vec(), P.vec(), d0.clone()), P.sums()
        assert P.launch(api.IW_ITER_MARCH_RC, 0, r1, p1, None, out_rc, sums_rc, prev=prev) == grid
        # stored-plane kernel from the finished words
        out_sp, sums_sp = (P.vec(), P.vec(), P.vec(), d0.clone()), P.sums()
        assert P.launch(api.IW_ITER_MARCH, 0, r1, p1, A1, out_sp, sums_sp, aD_prev=words.data_ptr(), bN_prev=words.data_ptr() + 4) == grid
        print(f"MARCHHEAD {W}x{H} R={R}: finished words {words[:2].tolist()} | left behind by the recomputing kernel {left[:2].tolist()}")
        for name, x, y in (("r", out_rc[0], out_sp[0]), ("p", out_rc[1], out_sp[1]), ("delta", out_rc[3], out_sp[3])):
            assert bool(torch.isfinite(x).all()), name
            assert _same_bits(torch, x, y), (name, int((x != y).sum().item()))
        assert not torch.equal(out_rc[0], r1) and not torch.equal(out_rc[3], d0)          # (the launch did run an iteration)
        # the words the recomputing kernel's first wave left behind: the bits of the finished sums
        assert _same_bits(torch, left[:2], words[:2]), (left[:2].tolist(), words[:2].tolist())
        # the iteration's own sums: finite, and one partial set per workgroup in both kernels
        assert bool(torch.isfinite(sums_rc[0][:grid]).all()) and bool(torch.isfinite(sums_rc[1][:3 * grid]).all())
        assert bool(torch.isfinite(sums_sp[0][:grid]).all()) and bool(torch.isfinite(sums_sp[1][:3 * grid]).all())
    finally:
        forced_rows(0)


@pytest.mark.parametrize("kernel", ["stored-plane", "recomputing"])
def test_word_set_nothing_is_stored_and_the_scalars_are_poisoned(torch, forced_rows, kernel):
    """irregular[0] = 1 on 128 x 32 at 8 rows per segment: r_out, p_out, delta and the A p plane keep a sentinel bit for bit (the rows the recomputing kernel has in
    flight by the time it looks at the word land in registers nobody reads), every workgroup's alphaD partial and the two scalar words are NaN, the call returns.
    The stored-plane kernel is run as a GN step's first iteration (no words in that form: partials only) and as iteration 1 in the deferred form."""
    W, H, R = 128, 32, 8
    forced_rows(R)
    try:
        P = _Problem(torch, W, H)
        out0, sums0, nb, words = _first_iteration(P)
        assert nb == 8
        r1, p1, A1, d0 = out0
        P.irregular[0] = 1
        torch.cuda.synchronize()
        k = api.IW_ITER_MARCH if kernel == "stored-plane" else api.IW_ITER_MARCH_RC
        runs = [(0, r1, p1, A1, True)] + ([(1, P.r0, P.p0, None, False)] if kernel == "stored-plane" else [])
        for mode, r_in, p_in, A_in, deferred in runs:
            out = tuple(P.vec(SENTINEL) for _ in range(4))
            sums = P.sums()
            left = torch.zeros(16, dtype=torch.float32, device="cuda")
            prev = api.PrevT(sums0[0].data_ptr(), sums0[1].data_ptr(), nb, left.data_ptr(), left.data_ptr() + 4) if deferred else None
            got = P.launch(k, mode, r_in, p_in, A_in, out, sums, prev=prev)
            assert got == nb, got
            want = P.vec(SENTINEL)
            for name, t in zip(("r_out", "p_out", "Ap_out", "delta"), out):
                assert _same_bits(torch, t, want), (kernel, mode, name, int((t != want).sum().item()))
            assert bool(torch.isnan(sums[0][:nb]).all()), (kernel, mode, sums[0][:nb].tolist())
            assert bool((sums[0][nb:] == 0).all()) and bool((sums[1] == 0).all())
            if deferred:
                assert bool(torch.isnan(left[:2]).all()), (kernel, mode, left[:2].tolist())
            assert bool((left[2:] == 0).all())
    finally:
        forced_rows(0)


def test_short_slab_agrees_across_transports(torch):
    """One GN step on 128 x 32 split 16 + 16 between two ranks at 8 rows per segment (depth 2, two segments per rank, a ghost row towards the other rank): costs,
    every alpha_k / beta_k and the owned unknowns bit for bit between the all-gather transport (the slab form that stores rows of A p) and the device-side transport
    (peer stores; the launch's extra workgroups carry the exchange wave of the deferred cross-rank finish, which must still come behind everything it waits for)."""
    from test_gpu_march_segments import _run_slabs, LIT
    world, W, counts, R = 2, 128, (16, 16), 8
    a = _run_slabs(world, W, counts, R, True)
    b = _run_slabs(world, W, counts, R, False)
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
