"""CPU: the restatement of the assembled reduced camera matrix (tests/ba_schur_explicit_mirror.py) -- its float64 blocks are the dense Schur complement, its float32
assembly runs the matrix-free mirror's solves, and its structure builder counts what a brute-force walk over the observations counts -- so a failure of
tests/test_gpu_ba_schur_explicit.py is the device's, not the algorithm's.

Measured here (LM 5 x 150, q_tolerance 0.1, function_tolerance 0; iterations per step): (24, 300, 1200) assembled 3, 6, 7, 6, 8 = matrix-free; (48, 1200, 5000) assembled
2, 9, 9, 15, 17 = matrix-free; costs within 4e-7, GN 4 x 10 within 6e-7.  Block mirror: 52 and 69 in total."""
import numpy as np
import pytest

from thallo_amd import synthetic as syn

from ba_schur_mirror import BaSchurMirror, SchurLists, dense_reduced_solve, with_extras
from ba_schur_explicit_mirror import BaSchurExplicitMirror, SchurStructure, blocks64, brute_force_counts, hand_made, jb_of

LM = dict(q_tolerance=0.1, function_tolerance=0.0)
TABLE = [((24, 300, 1200), 12, 52), ((48, 1200, 5000), 16, 69)]      # ..., the block mirror's LM 5 x 150 iterations in total


def instance(dims, band):
    return syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)


@pytest.mark.parametrize("dims,band,_", TABLE)
@pytest.mark.parametrize("lm", [False, True])
def test_float64_assembled_s_is_the_dense_schur_complement(dims, band, _, lm):
    """S assembled block by block in float64 from Jb (W_q W_q'^T summed over the term lists, no dense J) against dense_reduced_solve's S of the first GN / LM system: <= 1e-9 of
    max |S|, test_ba_schur_mirror.py's bar for the reduced solve; and the blocks nobody stores are zero in the dense S"""
    m = BaSchurMirror(dims, instance(dims, band))
    C = dims[0]
    J = m.linearise()[0]
    if lm:
        A, b = m.first_lm_system()
        shift = np.asarray(A.diagonal() - (J.T @ J).diagonal())
    else:
        A, b, shift = (J.T @ J), np.zeros(m.n), None
    _, S, _ = dense_reduced_solve(A, b, 9 * C)
    Jb, oc, op = jb_of(J, C)
    L = SchurLists(oc, op, C, dims[1])
    st = SchurStructure(L)
    _, blocks = blocks64(Jb[L.cam_obs], L, st, shift, np.zeros(dims[1], bool))
    got = st.bsr(blocks).toarray()
    err = np.abs(got - S).max() / np.abs(S).max()
    stored = st.bsr(np.ones_like(blocks)).toarray() != 0
    print("assembled float64 S vs dense", dims, "LM" if lm else "GN", err, "blocks", st.nblk, "terms", st.nterms)
    assert err <= 1e-9
    assert np.abs(S[~stored]).max(initial=0.0) <= 1e-9 * np.abs(S).max()


@pytest.mark.parametrize("dims,band,block_total", TABLE)
def test_assembled_mirror_runs_the_matrix_free_mirrors_solves(dims, band, block_total):
    """LM 5 x 150 and GN 4 x 10 with the float32-assembled S against the matrix-free mirror: costs per step within 1e-5 (the floor of the bar tests/test_gpu_ba_schur.py
    places between device and mirror, max(1e-5, 3 err_jacobi)); LM iterations in total no more than the block mirror's"""
    p = instance(dims, band)
    ce, ie = BaSchurExplicitMirror(dims, p).lm_solve(5, 150, **LM)
    cm, im = BaSchurMirror(dims, p).lm_solve(5, 150, **LM)
    print("LM", dims, "assembled", ie, sum(ie), ce, "matrix-free", im, sum(im), cm)
    ge, gm = BaSchurExplicitMirror(dims, p).gn_solve(4, 10), BaSchurMirror(dims, p).gn_solve(4, 10)
    print("GN 4x10", dims, "assembled", ge, "matrix-free", gm)
    assert len(ce) == len(cm) and len(ie) == 5
    assert np.abs(np.array(ce) / np.array(cm) - 1).max() <= 1e-5
    assert np.abs(np.array(ge) / np.array(gm) - 1).max() <= 1e-5
    assert sum(ie) <= block_total, (ie, block_total)


def test_structure_builder_against_a_brute_force_count():
    """blocks and terms of the builder against a walk over all pairs of observations, on the kernel tests' shapes, on (72, 500, 2500, band 72) and on a hand-made instance
    with repeated (camera, point) pairs; in both point orders"""
    cases = []
    for dims, band, want in (((5, 72, 330), 5, (15, 930)), ((3, 160, 480), 3, (6, 960)), ((72, 500, 2500), 72, None)):
        p = instance(dims, band)
        cases.append((dims, p[3], p[4], dims[0], dims[1], want))
    oc, op, C, P = hand_made()
    cases.append(("hand-made", oc, op, C, P, None))
    for name, oc, op, C, P, want in cases:
        nlower, nterms, nblk, per_row = brute_force_counts(oc, op, C)
        for renumber in (False, True):
            L = SchurLists(oc, op, C, P, renumber)
            st = SchurStructure(L)
            print("structure", name, "renumbered" if renumber else "caller's order", "lower blocks", st.nlower, "terms", st.nterms, "stored", st.nblk,
                  "blocks per row", int(np.diff(st.row_ptr).min()), "-", int(np.diff(st.row_ptr).max()), "terms per block <=", int(np.diff(st.term_ptr).max()))
            assert (st.nlower, st.nterms, st.nblk) == (nlower, nterms, nblk) and (np.diff(st.row_ptr) == per_row).all()
            if want: assert (st.nlower, st.nterms) == want
            # the lists themselves: ascending terms of the right cameras and one point; ascending columns; a block and its transpose in each other's rows
            cam, pt = L.q_cam[st.terms], L.q_pt[st.terms]
            assert (pt[:, 0] == pt[:, 1]).all()
            blk = np.repeat(np.arange(st.nlower), np.diff(st.term_ptr))
            assert (cam[:, 0] == st.row[blk]).all() and (cam[:, 1] == st.colj[blk]).all()
            k = (blk * L.O + st.terms[:, 0]) * L.O + st.terms[:, 1]
            assert (np.diff(k) > 0).all()
            for c in range(C): assert (np.diff(st.col[st.row_ptr[c]:st.row_ptr[c + 1]]) > 0).all()
            assert (st.block_row[st.lower[:, 0]] == st.row).all() and (st.col[st.lower[:, 0]] == st.colj).all()
            assert (st.block_row[st.lower[:, 1]] == st.colj).all() and (st.col[st.lower[:, 1]] == st.row).all()
            assert ((st.lower[:, 2] >= 0) == (st.row == st.colj)).all() and sorted(st.lower[st.lower[:, 2] >= 0, 2]) == list(range(C))
        if name == (3, 160, 480): assert (np.diff(st.term_ptr) == 160).all()
        if name == (72, 500, 2500):
            full = np.diff(st.row_ptr)[8:-8]
            assert full.min() <= 64 < full.max() and 49 <= full.min() and np.diff(st.row_ptr).max() <= 69
        if name == "hand-made":      # (camera 3, point 0) three times: 9 terms in block (3, 3) from that point alone; (camera 1, point 2) twice: 4
            assert st.nterms > sum(n * (n + 1) // 2 for n in np.bincount(op))


def test_with_extras_structure():
    """the kernel tests' instances with their extras: the camera nothing observes has a row of one block, its diagonal, without a term"""
    p, d3 = with_extras(instance((5, 72, 330), 5))
    st = SchurStructure(SchurLists(p[3], p[4], d3[0], d3[1]))
    assert st.row_ptr[-1] - st.row_ptr[-2] == 1 and st.col[-1] == d3[0] - 1
    assert st.term_ptr[-1] == st.term_ptr[-2] and st.lower[-1, 2] == d3[0] - 1
    assert st.nterms == 930 + 1
