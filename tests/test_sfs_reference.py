"""tests/sfs_reference.py before any kernel is compared with it: against central differences, against the float32 oracle, and against its own conditions
(margins, coverage, the branch every input family is named for, the slab cut).  No device."""
import numpy as np
import pytest
import scipy.sparse as sp

import sfs_reference as sr
from sfs_reference import F32

# the sizes of tests/test_gpu_sfs_kernels.py (SHAPES there is this list) and the two sizes the whole-solve and slab tests use
SHAPES = sr.SHAPES
EXTRA = [(12, 12), (64, 48), (130, 33)]
ORACLE_SHAPES = [(3, 3), (12, 12), (61, 5), (130, 17)]


def test_shapes_cover_the_widths_and_heights_the_kernels_branch_on():
    assert {w for w, _ in SHAPES} == {1, 2, 3, 4, 59, 60, 61, 62, 64, 65, 124, 125, 126, 130, 250}
    assert {h for _, h in SHAPES} == {1, 2, 3, 5, 15, 16, 17, 33, 9}
    assert max(w for w, _ in SHAPES) <= 250 and max(h for _, h in SHAPES) <= 33


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_margins_coverage_and_branches(family):
    """no |dX| within 1e-5 of the gate, no D in (0, 1e-6), |n|^2 exactly 0 or above 1e-12; in every family except `degenerate` and at every size of at least 12 x 12 at
    least 10 % of the pixels are regularisation-valid, 10 % are not, and 10 % of the inner pixels carry a shading weight; the family's own branch is taken wherever the
    size can hold it"""
    for W, H in SHAPES + EXTRA:
        for only in (None, "p"):
            cs = sr.case(family, W, H, 0, only)
            m = sr.margins(cs)
            assert m.gate > 1e-5 and not (0 < m.d_pos < 1e-6) and m.sq_pos > 1e-12, (cs.name, vars(m))
            assert sr.margins_ok(cs)
            hit = sr.branch_hits(cs, family)
            assert hit is None or hit, cs.name
            if family != "degenerate" and W >= 12 and H >= 12 and only is None:
                assert cs.valid.mean() >= 0.1 and (~cs.valid).mean() >= 0.1, (cs.name, cs.valid.mean())
                assert ((cs.Wt != 0).any(-1) & cs.inner).sum() >= 0.1 * cs.inner.sum(), cs.name
    big = sr.case(family, 250, 33)
    assert sr.branch_hits(big, family)
    if family == "holes":
        D = big.D
        assert (D[:, 59:62] <= 0).any(0).all() and (D[:, 123:126] <= 0).any(0).all() and (D[:, 7:9] <= 0).any(0).all()          # across both strip seams and a pair boundary
        assert all((D[y, :] <= 0).any() for y in (0, 32)) and all((D[:, x] <= 0).any() for x in (0, 249))
        lone = big.pos & ~(sr.shift(D, 1, 0) > 0) & ~(sr.shift(D, -1, 0) > 0) & ~(sr.shift(D, 0, 1) > 0) & ~(sr.shift(D, 0, -1) > 0) & big.inner
        assert lone.any()
    if family == "steps":
        dX = np.abs(big.X[:, 1:].astype(np.float64) - big.X[:, :-1])
        med = np.median(dX, 0)                                                   # (single pixels carry a bump of 0.05)
        assert 0.0101 < med[59] < 0.014 and 0.006 < med[60] < 0.0099 and 0.0101 < med[123] < 0.014 and 0.006 < med[124] < 0.0099


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_jacobian_against_central_differences(family):
    """every column of J on a 9 x 7 image: F(X + t e_i) - F(X - t e_i) over 2 t, with the decisions frozen at X (the reference takes them on the inputs, and t = 1e-6 moves
    no |dX| across the gate: margins).  |n|^2 == 0 pixels are left out: there the function is not differentiable, and the spec's derivative is that of the frozen factor."""
    W, H = 9, 7
    cs = sr.case(family, W, H, 3)
    s = cs.system()
    J = s.J.toarray()
    t = 1e-6
    sq = cs.bi_forward()[1]
    flat = (np.nan_to_num(sq, nan=1.0) == 0)
    # rows whose BI terms touch a flat pixel
    touched = np.zeros((H, W, 6), bool)
    for rk, (ex, ey) in ((1, (1, 0)), (2, (0, 1))):
        touched[..., rk] = flat | sr.shift(flat, ex, ey)
    touched = touched.reshape(-1)
    worst = 0.0
    for i in range(W * H):
        Fs = []
        for sgn in (1.0, -1.0):
            X = cs.X.astype(np.float64).copy(); X.reshape(-1)[i] += sgn * t
            c2 = _frozen(cs, X)
            Fs.append(c2)
        col = (Fs[0] - Fs[1]) / (2 * t)
        err = np.abs(col - J[:, i])[~touched]
        scale = np.abs(J[:, i]).max() + 1.0
        worst = max(worst, float(err.max() / scale))
    assert worst < 1e-5, worst


def _frozen(cs, X64):
    """the residual vector at other (float64) unknowns with the decisions of cs: the formulas restated without any derivative machinery"""
    H, W = cs.H, cs.W
    c, l, u = X64, sr.shift(X64, -1, 0), sr.shift(X64, 0, -1)
    nx = u * (c - l) / cs.fy; ny = l * (c - u) / cs.fx
    nz = nx * (cs.ux - cs.xs) / cs.fx + ny * (cs.uy - cs.ys) / cs.fy - l * u / (cs.fx * cs.fy)
    sq0 = cs.bi_forward()[1]
    pos = np.nan_to_num(sq0, nan=0.0) > 0
    sq = nx * nx + ny * ny + nz * nz
    inv = np.where(pos, 1.0 / np.sqrt(np.where(pos, sq, 1.0)), 1.0)
    n0, n1, n2 = inv * nx, inv * ny, inv * nz
    L = cs.L
    B = L[0] + L[1] * n1 + L[2] * n2 + L[3] * n0 + L[4] * n0 * n1 + L[5] * n1 * n2 + L[6] * (-n0 * n0 - n1 * n1 + 2 * n2 * n2) + L[7] * n2 * n0 + L[8] * (n0 * n0 - n1 * n1)
    Im = cs.Im.astype(np.float64)
    BI = np.where(cs.on, B - (0.5 * Im + 0.25 * (sr.shift(Im, -1, 0) + sr.shift(Im, 0, -1))), 0.0)
    F = np.zeros((H, W, 6))
    F[..., 0] = np.where(cs.pos, cs.wp * (X64 - cs.D), 0.0)
    F[..., 1] = cs.h * (BI - sr.shift(BI, 1, 0)); F[..., 2] = cs.k * (BI - sr.shift(BI, 0, 1))
    for k in range(3):
        P = cs.coef[k] * X64
        F[..., 3 + k] = np.where(cs.valid, cs.ws * (4 * P - sum(sr.shift(P, dx, dy) for dx, dy in sr.NBRS)), 0.0)
    return F.reshape(-1)


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_frozen_restatement_equals_the_reference_residuals(family):
    cs = sr.case(family, 9, 7, 3)
    s = cs.system()
    assert np.abs(_frozen(cs, cs.X.astype(np.float64)) - s.F).max() <= 1e-12 * (np.abs(s.F).max() + 1)


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_forward_and_closed_form_agree(family):
    """the two derivations of G give the same numbers in float64 (to 1e-9 of the magnitude), and every magnitude bounds its value"""
    for W, H in ((9, 7), (61, 5), (130, 17)):
        cs = sr.case(family, W, H)
        (Gf, _), (Gc, _) = cs.bi_forward(), cs.bi_closed()
        for a, b in zip(Gf, Gc):
            assert (a.m >= np.abs(a.v) * (1 - 1e-12)).all() and (b.m >= np.abs(b.v) * (1 - 1e-12)).all()
            assert (np.abs(a.v - b.v) <= 1e-9 * np.maximum(a.m, b.m) + 1e-300).all(), cs.name
        assert Gf[3].k < 200 and Gf[0].k < 400 and Gc[0].k < 400, (Gf[3].k, Gf[0].k, Gc[0].k)


@pytest.mark.parametrize("only", [None, "p", "s", "g"])
@pytest.mark.parametrize("family", sr.FAMILIES)
def test_against_the_oracle(orc, family, only):
    """residuals, cost, J (csr()), eval_jtf and apply_jtj of the float32 oracle on every family: the bound is the reference's own k 2^-24 S with the k of the kernels' chains
    (the oracle runs the same float32 operations in the forward-mode form: k_G from the tree, + 12 for the weight and the row, 2 k_G + 40 for J^T (J p))"""
    for W, H in ORACLE_SHAPES:
        cs = sr.case(family, W, H, 0, only)
        G, _ = cs.bi_forward()
        kG = max(t.k for t in G)
        s = cs.system(Gmag=cs.Gmag())                    # the oracle's float32 planes carry the rounding of the whole BI tree: its magnitudes
        pr = orc.Problem(orc.SFS, (W, H), [a.copy() if isinstance(a, np.ndarray) else a for a in cs.params])
        rowptr, col, val, res = pr.csr()
        Jo = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(len(rowptr) - 1, cs.N))
        assert Jo.shape[0] == 6 * cs.N
        tolF = sr.EPS * (kG + 12) * s.Fabs + 1e-30
        assert (np.abs(res - s.F) <= tolF).all(), (cs.name, np.abs(res - s.F).max())
        assert (np.abs((Jo - s.J).toarray()) <= sr.EPS * (kG + 12) * s.Jabs.toarray() + 1e-30).all(), cs.name
        assert abs(pr.cost() - s.cost) <= (np.abs(s.F) * tolF).sum() + 1e-6 * s.cost + 1e-30
        r, _ = pr.eval_jtf()
        assert (np.abs(r - s.r) <= (2 * kG + 40) * sr.EPS * s.r_abs + 1e-30).all(), (cs.name, (np.abs(r - s.r) / (s.r_abs + 1e-30)).max() / sr.EPS)
        p = np.random.default_rng(5).standard_normal(cs.N).astype(F32)
        Ap, _ = pr.apply_jtj(p)
        want, mag = s.apply(p)
        assert (np.abs(Ap - want) <= (2 * kG + 40) * sr.EPS * mag + 1e-30).all(), (cs.name, (np.abs(Ap - want) / (mag + 1e-30)).max() / sr.EPS)


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_jtj_is_symmetric_and_diag_is_its_diagonal(family):
    for W, H in ((3, 3), (12, 12), (61, 5)):
        s = sr.case(family, W, H).system()
        A = s.jtj()
        assert abs(A - A.T).max() <= 1e-12 * (abs(A).max() + 1e-300)
        assert np.abs(A.diagonal() - s.diag).max() <= 1e-12 * (s.diag.max() + 1e-300)
        assert (s.diag_abs >= s.diag * (1 - 1e-12)).all()
        p = np.random.default_rng(1).standard_normal(s.cs.N)
        want, mag = s.apply(p)
        assert np.abs(A @ p - want).max() <= 1e-10 * (mag.max() + 1e-300) and (mag >= np.abs(want) * (1 - 1e-12)).all()


@pytest.mark.parametrize("family", ["holes", "steps", "masks"])
def test_slab_cut(family):
    """owned rows of a top, a middle and a bottom slab: the reference evaluated on the LOCAL inputs with global coordinates (u_y moved by yoff, the border guard by hand)
    equals the global result there -- which is what the cut promises a kernel's caller"""
    W, H = 130, 33
    cs = sr.case(family, W, H)
    s = cs.system()
    p = np.random.default_rng(2).standard_normal(cs.N)
    want, _ = s.apply(p)
    for g0, g1 in ((0, 11), (11, 18), (13, 14), (19, 33)):
        sl = sr.slab(cs, g0, g1)
        assert sl.H == (g1 - g0) + (2 if g0 > 0 else 0) + (2 if g1 < H else 0) and sl.Hg == H and sl.yoff == g0 - (2 if g0 > 0 else 0)
        assert sl.row1 - sl.row0 == g1 - g0
        lp = list(sl.params); lp[6] = float(F32(lp[6])) - sl.yoff                      # the local image in its own coordinates: u_y moves (and is rounded again: 1e-6)
        lc = sr.Case(lp)
        Gl = lc.G64()
        assert np.abs(Gl[sl.planes] - cs.G64()[sl.lo:sl.hi][sl.planes]).max() <= 1e-6 * (np.abs(Gl).max() + 1e-300)
        assert np.array_equal(lc.fl[sl.planes], cs.fl[sl.lo:sl.hi][sl.planes])
        assert np.array_equal(lc.Wt[sl.planes], cs.Wt[sl.lo:sl.hi][sl.planes])
        # two ghost rows suffice: the local system's r, diag and J^T J p on the owned rows are the global ones
        ls = lc.system()
        own = slice(sl.row0, sl.row1)
        lw, lmag = ls.apply(p.reshape(H, W)[sl.lo:sl.hi])
        for loc, glob, mag in ((ls.r, s.r, ls.r_abs), (ls.diag, s.diag, ls.diag_abs), (lw, want, lmag)):
            loc, glob, mag = loc.reshape(sl.H, W)[own], glob.reshape(H, W)[sl.rows], mag.reshape(sl.H, W)[own]
            assert (np.abs(loc - glob) <= 1e-5 * mag + 1e-300).all(), (family, g0, g1)


def test_packed_dword_fields():
    for family in sr.FAMILIES:
        cs = sr.case(family, 62, 3)
        d = cs.dword
        assert np.array_equal(d & 0xff, cs.fl) and ((d >> 24) == 0).all()
        mr, mc = (d >> 8) & 0xff, (d >> 16) & 0xff
        assert np.array_equal(mr[cs.inner], cs.mR[cs.inner]) and np.array_equal(mc[cs.inner], cs.mC[cs.inner])
        assert not mr[~cs.inner].any() and not mc[~cs.inner].any()
        wg = np.sqrt(cs.hp[2])
        assert np.array_equal(cs.Wt[..., 0], (wg * mr.astype(F32)).astype(F32)) and np.array_equal(cs.Wt[..., 1], (wg * mc.astype(F32)).astype(F32))
