"""tests/generated_reference.py against itself, on the CPU: the complex-step Jacobian against central differences, the rows test_gpu_frontend.py writes out for scipy
(graph2d.t, flow_sample.t), and the MUTATION CHECK that gives the tolerances of tests/test_gpu_generated_kernels.py their meaning: every mutant of the reference --
the kind of error a whole solve does not see -- must move at least one element of r, diag or Ap by at least ten times the bound the GPU test allows at that element.

Mutants (each where the energy has the construct):
  drop      one partial dropped at a border instance (the last instance of the last residual with a non-zero row);
  flip      the sign of one off-centre partial (the largest entry behind the first of a row with at least two);
  leak      a guarded load returning its clamped neighbour instead of 0 (conv2d_wide.t: the window at a pixel of the border band; flow_sample.t: the samples of the
            pixel that looks off the left edge; for the difference stencils the clamped neighbour is the pixel itself and the mutant is the identity);
  diag2     one residual's contribution to diag doubled;
  exclude   the Exclude mask ignored at one unknown;
  redirect  one Sparse-map entry redirected to the neighbouring owner."""
import numpy as np
import pytest
import scipy.sparse as sps

import generated_reference as gr

CASES = [(gr.gradient_paste, (14, 11)), (gr.gradient_paste, (1, 9)), (gr.gradient_paste, (9, 1)), (gr.gradient_paste, (67, 3)), (gr.weighted_laplacian, (40, 28)),
         (gr.weighted_laplacian, (14, 9)), (gr.weighted_laplacian, (2, 2)), (gr.volume_arap, ()), (gr.flow_sample, (28, 20)), (gr.flow_sample, (3, 2)), (gr.cotan_smooth, ()),
         (gr.robust_plane, ()), (gr.embedded_nodes, ()), (gr.graph2d, ()), (gr.two_domains, (100, 37)), (gr.two_domains, (64, 5)), (gr.two_domains, (7, 30)), (gr.two_domains, (300, 260)), (gr.conv2d_wide, ()),
         (gr.row_gain, (100, 37)), (gr.row_gain, (64, 5)), (gr.row_gain, (7, 30)), (gr.conv1d, ()), (gr.layer_sample, (28, 20)), (gr.layer_sample, (3, 2)), (gr.lp_smooth, (33,)), (gr.lp_smooth, (2,)),
         (gr.sparse_exclude, ()), (gr.arap_mesh, ()), (gr.bundle_adjustment, ()), (gr.shape_from_shading, (2, 5)), (gr.shape_from_shading, (5, 2)), (gr.shape_from_shading, (33, 7)),
         (gr.image_warping, (19, 13)), (gr.image_warping, (65, 6)), (gr.shape_from_shading, (19, 13)), (gr.shape_from_shading, (65, 6))]
ident = lambda c: c[0].__name__ + "".join(f"-{a}" for a in c[1])


@pytest.mark.parametrize("case", [c for c in CASES if c[0] not in (gr.flow_sample, gr.shape_from_shading, gr.lp_smooth, gr.arap_mesh, gr.bundle_adjustment)], ids=ident)
def test_complex_step_jacobian_equals_central_differences(case):
    """(the bundled shape_from_shading, arap_mesh_deformation and bundle_adjustment take their J from sfs_reference.py, graph_reference.py and ba_reference.py, which their own
    CPU tests hold to differences; lp_smooth's L_p holds a factor constant that a difference of F moves; flow_sample.t is not here: the partials of a SampledImage are samples of its derivative images, not the slope of the bilinear patch -- its J is compared with
    the scipy rows below)"""
    R = gr.reference(case[0], *case[1])
    e = R.energy
    rng = np.random.default_rng(1)
    cols = rng.choice(np.flatnonzero(e.free), min(40, int(e.free.sum())), replace=False)
    J = R.J.tocsc()
    for j in cols:
        h = 1e-5 * max(1.0, abs(e.x0[j]))
        xp, xm = e.x0.copy(), e.x0.copy(); xp[j] += h; xm[j] -= h
        fd = (e.F(xp) - e.F(xm)) / (2 * h)
        col = np.asarray(J[:, j].todense()).ravel()
        assert np.abs(fd - col).max() <= 1e-6 * max(1.0, np.abs(col).max()), (e.name, j)
    assert R.J[:, ~e.free].nnz == 0


def test_graph2d_rows_equal_the_scipy_rows():
    R = gr.reference(gr.graph2d)
    e = R.energy
    wf, x0, data, mask, right, down = e.params
    W, H = e.dims
    n = W * H; pix = np.arange(n).reshape(H, W); yy, xx = np.mgrid[0:H, 0:W]
    rows = [sps.diags((wf * mask).ravel()), 0.5 * (sps.identity(n) - sps.csr_matrix((np.ones(n), (pix.ravel(), (yy * W + right).ravel())), shape=(n, n))),
            sps.identity(n) - sps.csr_matrix((np.ones(n), (pix.ravel(), (down * W + xx).ravel())), shape=(n, n))]
    J = sps.vstack(rows).tocsr()
    b = np.concatenate([(wf * mask * data).ravel(), np.zeros(2 * n)])
    assert abs(J - R.J).max() <= 1e-15
    assert np.abs((J @ x0.ravel() - b) - R.Fx).max() <= 1e-14
    assert np.abs(-(J.T @ (J @ x0.ravel() - b)) - R.r).max() <= 1e-12


def test_flow_sample_rows_equal_the_scipy_rows():
    R = gr.reference(gr.flow_sample, 28, 20)
    e = R.energy
    wf, wr, flow0, src, dst, ddx, ddy = e.params
    W, H = e.dims
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    n = H * W; pix = np.arange(n).reshape(H, W)
    px, py = xx + flow0[..., 0], yy + flow0[..., 1]
    rows, cols, vals = [], [], []
    for c in range(2):
        gx, gy = gr.bilinear(ddx[..., c], px, py), gr.bilinear(ddy[..., c], px, py)
        for comp, g in ((0, gx), (1, gy)):
            rows.append(c * n + pix.ravel()); cols.append(2 * pix.ravel() + comp); vals.append(-wf * g.ravel())
    base = 2 * n
    for k, (dxo, dyo) in enumerate(((1, 0), (0, 1))):
        ok = np.zeros((H, W), bool); ok[:H - dyo, :W - dxo] = True
        nb = np.roll(pix, (-dyo, -dxo), (0, 1))
        for comp in range(2):
            rr = base + k * 2 * n + 2 * pix[ok] + comp
            rows += [rr, rr]; cols += [2 * pix[ok] + comp, 2 * nb[ok] + comp]; vals += [np.full(rr.size, float(wr)), np.full(rr.size, -float(wr))]
    J = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 2 * n))
    assert abs(J - R.J).max() <= 1e-14


# ------------------------------------------------------------------ the mutation check
def k_for(e):
    return gr.k_eval(e)


def with_J(R, J, Fx=None, diag_extra=None):
    return gr.Reference(R.energy, J=J.tocsc(), Fx=R.Fx if Fx is None else Fx, diag_extra=diag_extra)


def mutants(case, R):
    e = R.energy
    Jr = R.J.tocsr(); lens = np.diff(Jr.indptr)
    out = {}
    live = np.flatnonzero((lens >= 1) & (np.abs(R.Fx) > 1e-3))
    i = live[-1]                                                           # drop: the last live instance
    J = Jr.tolil(copy=True); J[i, Jr.indices[Jr.indptr[i]]] = 0.0
    out["drop"] = with_J(R, J.tocsr())
    two = np.flatnonzero((lens >= 2) & (np.abs(R.Fx) > 1e-3))
    if two.size:
        i = two[len(two) // 2]
        ent = slice(Jr.indptr[i] + 1, Jr.indptr[i + 1])                       # not the first entry; of the others the largest (a partial that is nearly 0 flips nothing)
        j = Jr.indices[ent][np.argmax(np.abs(Jr.data[ent]))]
        J = Jr.tolil(copy=True); J[i, j] = -Jr[i, j]
        out["flip"] = with_J(R, J.tocsr())
    i = live[len(live) // 3]
    row = Jr[i].toarray().ravel()
    out["diag2"] = with_J(R, Jr, diag_extra=row * row)
    if not e.free.all():
        j = np.flatnonzero(~e.free)[len(np.flatnonzero(~e.free)) // 2]
        free = e.free.copy(); free[j] = True
        e2 = case[0](*case[1]); e2.free = free
        M = gr.Reference(e2)
        if M.J[:, j].nnz: out["exclude"] = M          # (image_warping: every residual that reads a masked pixel is switched off by the same mask -- the mutant is the identity)
    if e.index_slots:
        E = e.params[e.index_slots[0]].size
        slot = 2 if case[0] is gr.cotan_smooth else 1 if case[0] in (gr.arap_mesh, gr.bundle_adjustment) else 0           # (cotan_smooth: an apex -- redirecting v0 onto v1 would make the triangle degenerate, the cotangent infinite)
        out["redirect"] = gr.Reference(case[0](*case[1], redirect=(slot, E // 2)))
        assert np.isfinite(out["redirect"].r).all()
    if case[0] is gr.conv2d_wide:
        out["leak"] = gr.Reference(gr.conv2d_wide(*case[1], leak_at=(2, 7)))
    if case[0] is gr.flow_sample:                    # pixel (0, 0) samples off the left edge (flow -0.25, 0)
        out["leak"] = gr.Reference(gr.flow_sample(*case[1], leak_at=(0, 0)))
    return out


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_every_mutant_moves_an_element_by_ten_times_the_bound(case):
    R = gr.reference(case[0], *case[1])
    e = R.energy
    k = k_for(e)
    if k is None:
        pytest.fail(f"{e.name}: no recorded k_eval (generated_reference.K_EVAL_MEASURED): the GPU test cannot hold it, so nothing here has a bound to check")
    P = gr.probe_vectors(e.n, 1)
    checked = []
    for name, M in mutants(case, R).items():
        hit = lambda got, want, bound: ((np.abs(got - want) >= 10 * bound) & (got != want)).any()
        assert hit(M.r, R.r, R.bound_r(k["r"])) or hit(M.diag, R.diag, R.bound_diag(k["diag"])) or any(hit(M.Ap(p), R.Ap(p), R.bound_Ap(k["Ap"], p, True)) for p in P.values()), \
            (e.name, name, "slips under ten times the bound")
        checked.append(name)
    assert {"drop", "diag2"} <= set(checked)
