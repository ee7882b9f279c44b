"""tests/iw_reference.py checked on the CPU before any kernel is compared with it: its two derivations of J^T J p, J^T F and the diagonal against each other, its
Jacobian against central differences of its own residual function, everything against the float32 oracle on every case, its flags / counts against a brute-force
loop, and the case list itself: every neighbour count with and without the fit bit occurs, the exact cases are exact, no owned pixel is left out of a comparison."""
import numpy as np
import pytest

import iw_reference as iw
import shim_kernels as sk
from shim_kernels import F32

ALL = list(iw.CASES)
# the oracle computes in float32 in an order of its own: the longest chain counted for the kernels (2 T + 16 roundings into an Angle entry of J^T J p, T = 1 for a
# correctly rounded libm) plus the additions of its own accumulation (at most 8 more per unknown: four residuals seen from both ends)
K_ORACLE = 2 * 1 + 16 + 8


@pytest.mark.parametrize("name", ALL)
def test_two_derivations_agree(name):
    """residual by residual with array shifts against J^T (J p) with J assembled from the residual function: to float64 rounding of the terms' magnitudes"""
    R = iw.ref(name)
    J = R.jacobian()
    st = R.stencil()
    p = np.random.default_rng(11).standard_normal(3 * R.N)
    Ap, S = st.apply(p)
    assert (np.abs(Ap) <= S * (1 + 1e-12)).all()
    assert np.abs(Ap - J.T @ (J @ p)).max() <= 64 * 2.0 ** -53 * max(S.max(), 1e-300)
    r, Sr, diag = R.jtf()
    assert np.abs(r + J.T @ R.residuals(R.x0())).max() <= 64 * 2.0 ** -53 * max(Sr.max(), 1e-300)
    assert np.abs(diag - np.asarray(J.multiply(J).sum(0)).ravel()).max() <= 64 * 2.0 ** -53 * max(diag.max(), 1e-300)
    assert (np.abs(r) <= Sr * (1 + 1e-12)).all()
    if iw.case(name).grid:                                        # the unit grid: u_i - u_j = -d, and the diagonal is a function of the flags byte
        Ag, Sg = R.stencil(grid=True).apply(p)
        assert np.array_equal(Ag, Ap) and np.array_equal(Sg, S)
        do, da, act = iw.diag_from_flags(R.flags(), R.wf, R.wr)
        assert np.abs(diag - iw.pack(np.repeat(do[..., None], 2, -1), da)).max() <= 8 * 2.0 ** -53 * max(diag.max(), 1e-300)
    assert (r[R.excluded()] == 0).all() and (Ap[R.excluded()] == 0).all() and (diag[R.excluded()] == 0).all()


@pytest.mark.parametrize("name", ["t1x1", "t2x2", "m2x7", "shear"])
def test_jacobian_is_the_derivative_of_the_residuals(name):
    """central differences with step 1e-5 in float64: truncation ~ h^2 |d3 F| / 6 ~ 1e-10 |u_i - u_j|, rounding ~ 1e-16 |F| / h ~ 1e-9; asserted to 1e-6 of the largest entry"""
    R = iw.ref(name)
    J = R.jacobian().toarray()
    x, h = R.x0(), 1e-5
    fd = np.empty_like(J)
    for k in range(len(x)):
        d = np.zeros_like(x); d[k] = h
        fd[:, k] = (R.residuals(x + d) - R.residuals(x - d)) / (2 * h)
    assert J.shape == (10 * R.N, 3 * R.N)
    assert np.abs(J - fd).max() <= 1e-6 * max(np.abs(J).max(), 1.0)
    if R.N > 1:
        assert np.abs(J[:, 2 * R.N:]).max() > 0.01           # the angle block is there


@pytest.mark.parametrize("name", ALL)
def test_reference_against_the_oracle(orc, name):
    c, R = iw.case(name), iw.ref(name)
    prob = orc.Problem(orc.IMAGE_WARPING, (c.W, c.H), iw.params(c))
    assert np.array_equal(prob.excluded(), R.excluded())
    r, Sr, diag = R.jtf()
    ro, do = prob.eval_jtf()
    assert (np.abs(ro - r) <= sk.tol(K_ORACLE, Sr)).all(), np.abs(ro - r).max()
    assert (np.abs(do - diag) <= sk.tol(K_ORACLE, diag)).all()
    rng = np.random.default_rng(5)
    p = np.where(R.excluded(), 0, rng.integers(-4, 5, 3 * R.N) if c.exact else rng.standard_normal(3 * R.N)).astype(F32)
    Ap, S = R.stencil().apply(p)
    Ao, aD = prob.apply_jtj(p)
    assert (np.abs(Ao - Ap) <= sk.tol(K_ORACLE, S)).all(), (np.abs(Ao - Ap) / np.maximum(sk.tol(K_ORACLE, S), 1e-300)).max()
    assert abs(aD - (p * Ap).sum()) <= sk.tol(K_ORACLE + 3, (np.abs(p) * S).sum()) + sk.tol(64, np.abs(p * Ap).sum())
    cost, Sc = R.cost_pixels()
    assert abs(prob.cost() - cost.sum()) <= sk.tol(2 * K_ORACLE, Sc.sum())
    if c.exact:
        assert prob.cost() == cost.sum() and np.array_equal(ro, r) and np.array_equal(Ao, Ap)


@pytest.mark.parametrize("name", ALL)
def test_flags_counts_and_irregular_counts_by_brute_force(name):
    c, R = iw.case(name), iw.ref(name)
    W, H = c.W, c.H
    want = np.zeros((H, W), np.uint8)
    bad = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if x + 1 < W and (F32(c.urshape[y, x + 1, 0] - c.urshape[y, x, 0]) != 1 or F32(c.urshape[y, x + 1, 1] - c.urshape[y, x, 1]) != 0): bad[y, x] = True
            if y + 1 < H and (F32(c.urshape[y + 1, x, 0] - c.urshape[y, x, 0]) != 0 or F32(c.urshape[y + 1, x, 1] - c.urshape[y, x, 1]) != 1): bad[y, x] = True
            if c.mask[y, x] != 0:
                continue
            n = sum(1 for dx, dy in iw.DIRS if 0 <= x + dx < W and 0 <= y + dy < H and c.mask[y + dy, x + dx] == 0)
            want[y, x] = 1 | (2 if c.cons[y, x, 0] >= 0 and c.cons[y, x, 1] >= 0 else 0) | (n << 2)
    assert np.array_equal(R.flags(), want)
    for row0, row1 in iw.row_ranges(name):
        f = R.flags(row0, row1)
        assert np.array_equal(f[row0:row1], want[row0:row1])
        ghost = np.ones(H, bool); ghost[row0:row1] = False
        assert np.array_equal(f[ghost], want[ghost] & 1)
        assert R.irregular(row0, row1) == int(bad[row0:row1].sum())
    assert (R.irregular() == 0) == c.grid


def test_the_cases_cover_what_they_claim():
    seen, zero_cons, negzero, under_mask, neg_mask = set(), False, False, False, False
    for name in ALL:
        c, R = iw.case(name), iw.ref(name)
        f = R.flags()
        seen |= {(int(b) >> 2, (int(b) >> 1) & 1) for b in np.unique(f[f != 0])}
        zero_cons |= bool(((c.cons[..., 0] == 0) & (c.cons[..., 1] == 0) & ~np.signbit(c.cons[..., 0])).any())
        negzero |= bool((np.signbit(c.cons[..., 0]) & (c.cons[..., 0] == 0) & R.fit).any())
        under_mask |= bool(((c.cons[..., 0] >= 0) & (c.cons[..., 1] >= 0) & ~R.act).any())
        neg_mask |= bool((np.signbit(c.mask) & R.act).any())
        assert (((c.cons >= 0).sum(-1) == 1) & R.act).any() or c.W * c.H < 4          # one component negative: not a constraint
        # no comparison leaves an owned entry out: every row range of the case owns whole rows of the three planes, and the tests compare exactly rows_mask
        for row0, row1 in iw.row_ranges(name):
            assert 0 <= row0 < row1 <= c.H and row0 <= 1 and c.H - row1 <= 1
            assert iw.rows_mask(c.W, c.H, row0, row1).sum() == 3 * c.W * (row1 - row0)
    assert seen == {(n, f) for n in range(5) for f in range(2)}, sorted(seen)
    assert zero_cons and negzero and under_mask and neg_mask
    assert any(not iw.ref(n).act[iw.case(n).H // 2 + 1].any() for n in ALL if iw.case(n).H > 2)              # a fully masked row
    assert not iw.ref("m248x3").act[:, iw.MARCH_USE:2 * iw.MARCH_USE].any()                                   # a fully masked strip
    assert {iw.case(n).W for n in ALL} >= {1, 2, 63, 64, 65, 130, 122, 124, 126, 248, 250}
    assert {iw.case(n).H for n in ALL} >= {1, 2, 15, 16, 17, 33}
    assert any((2 * iw.case(n).W * iw.case(n).H) % 4 for n in ALL)                                            # the launchers' drop to the general path


@pytest.mark.parametrize("name", [n for n in ALL if iw.CASES[n][4]])
def test_the_exact_cases_are_exact(name):
    """angle 0, integer offsets, weights whose squares are powers of two, small-integer planes, scalars that are exact quotients: every product and sum of the
    iteration is a multiple of 2^-6 below 2^18, so float32 computes it without rounding in any order (M^-1 aside: pre_from_flags_f32 has its bits)"""
    c, R = iw.case(name), iw.ref(name)
    P = iw.planes(name, 3)
    aN, aD, bN, aN2, aD2 = iw.exact_scalars()
    alpha, beta, alpha2 = sk.div32(aN, aD, True), sk.div32(bN, aN, True), sk.div32(aN2, aD2, True)
    st = R.stencil(cs=np.stack([np.ones((c.H, c.W)), np.zeros((c.H, c.W))], -1), grid=True)
    pre = np.where(R.excluded(), 0, sk.exact_pre(np.random.default_rng(4), 3 * R.N))
    o = iw.iteration(st, pre, P.r, P.Ap, P.p, P.delta, P.p_old, 4, alpha, beta, alpha2)
    for v in (o.r, o.p, o.delta, o.Ap, R.jtf()[0]):
        assert np.array_equal(v, v.astype(F32)) and np.array_equal(v * 64, np.rint(v * 64)) and np.abs(v).max() < 2 ** 18
    for terms in (o.alphaD, R.cost_pixels()[0].ravel()):
        assert np.array_equal(terms * 4096, np.rint(terms * 4096)) and np.abs(terms).sum() < 2 ** 24 / 4096 * 2 ** 10
    mo, ma = iw.pre_from_flags_f32(R.flags(), c.w_fit, c.w_reg)
    mo64, ma64 = iw.pre_from_flags(R.flags(), c.w_fit, c.w_reg)
    assert (np.abs(mo - mo64) <= sk.tol(8, mo64)).all() and (np.abs(ma - ma64) <= sk.tol(8, ma64)).all()


@pytest.mark.parametrize("xguard", [0, 1])
@pytest.mark.parametrize("W,H", iw.LAP_CASES)
def test_laplacian_reference(orc, W, H, xguard):
    X, A, w = iw.lap_inputs(W, H)
    R = iw.LapRef(W, H, X, A, w, xguard)
    J = R.jacobian()
    v = np.random.default_rng(2).standard_normal(W * H)
    Av, S = R.apply(v)
    assert np.abs(Av.ravel() - J.T @ (J @ v)).max() <= 64 * 2.0 ** -53 * S.max()
    F = J @ R.X.ravel() - np.concatenate([R.w * R.A.ravel(), np.zeros(2 * W * H)])
    r, Sr, diag = R.system()
    assert np.abs(r.ravel() + J.T @ F).max() <= 64 * 2.0 ** -53 * Sr.max()
    assert np.abs(diag.ravel() - np.asarray(J.multiply(J).sum(0)).ravel()).max() <= 1e-15 * diag.max()
    assert abs(R.cost_pixels()[0].sum() - 0.5 * (F * F).sum()) <= 1e-13 * R.cost_pixels()[1].sum()
    prob = orc.Problem(orc.LAPLACIAN_IMAGE, (W, H), [X.copy(), A.copy()], fconst=[w], iconst=[xguard])
    ro, do = prob.eval_jtf()                                      # (16: the 12 roundings counted for the kernel's chain and the oracle's own order of additions)
    assert (np.abs(ro - r.ravel()) <= sk.tol(16, Sr.ravel())).all()
    assert (np.abs(do - diag.ravel()) <= sk.tol(8, diag.ravel())).all()
    Ao, _ = prob.apply_jtj(v.astype(F32))
    assert (np.abs(Ao - R.apply(v.astype(F32))[0].ravel()) <= sk.tol(16, R.apply(v.astype(F32))[1].ravel())).all()
    assert abs(prob.cost() - R.cost_pixels()[0].sum()) <= sk.tol(16, R.cost_pixels()[1].sum())


def test_owner_maps():
    blk, per = iw.tile_blocks(130, 33, 0, 33, 9)
    assert per == 1 and blk.min() == 0 and blk.max() == 8 and blk[16, 64] == 4 and blk[32, 129] == 8
    blk, per = iw.tile_blocks(130, 35, 1, 34, 8)                  # 9 tiles on 8 workgroups in 8 groups: group g owns tiles [9 g / 8, 9 (g + 1) / 8)
    assert per == 2 and (blk[0] == -1).all() and (blk[34] == -1).all() and blk[1, 0] == 0 and np.bincount(blk[blk >= 0]).size == 8
    blk, per = iw.tile_blocks(65, 9, 0, 9, 6, 64, 4)
    assert per == 1 and blk[8, 64] == 5
