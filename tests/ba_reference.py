"""Bundle adjustment in plain numpy, float64, no device: the reference of tests/test_gpu_ba_kernels.py (validated on the CPU by tests/test_ba_reference.py).

Written from include/thallo_hip.h (E4: the unknowns' flat layout [cameras 9 c + k | points 9 C + 3 p + k], the index lists, the block of an observation
Jb[24 q ..] = { d r0 / d cam[9], d r0 / d pt[3], d r1 / d cam[9], d r1 / d pt[3] }; the LM single-reduction block: N, S1, S2, U, T1, T2, q_{k+1}) and from the energy itself,
examples/bundle_adjustment/bundle_adjustment.t with AngleAxisRotatePoint of lib.t:514-555 -- not from the kernels.

  * residual_and_jacobian: the residual's expression over forward-mode duals, a dual being one numpy array [13, O] (the value, then the 12 partials);
    the same function on float32 arrays is the float32 restatement that sets the bars of the closed form;
  * jt_f / jtj_diag / apply: J^T F, diag J^T J, (J^T J + CtC) p of a GIVEN block array (the device's own stored bits), as sparse gathers (np.add.at), never a dense matrix;
  * sums3 / sumsq / lm_q1: the sums of the single-reduction PCG and LM forms, term by term;
  * incidence(): index lists with prescribed observation counts per camera and per point, in the caller's point order or the plan's renumbered one."""
from types import SimpleNamespace

import numpy as np

THETA2_CUT = 1e-8            # lib.t:517


# ------------------------------------------------------------------ duals: a[0] the value, a[1:13] the partials
def _const(like, c):
    r = np.zeros_like(like); r[0] = c
    return r


def _mul(a, b):
    r = np.empty_like(a)
    r[0] = a[0] * b[0]; r[1:] = a[1:] * b[0] + a[0] * b[1:]
    return r


def _div(a, b):
    r = np.empty_like(a)
    r[0] = a[0] / b[0]; r[1:] = (a[1:] * b[0] - a[0] * b[1:]) / (b[0] * b[0])
    return r


def _sqrt(a):
    r = np.empty_like(a)
    r[0] = np.sqrt(a[0]); r[1:] = a[1:] / (r[0] + r[0])
    return r


def _sin(a):
    r = np.empty_like(a)
    r[0] = np.sin(a[0]); r[1:] = a[1:] * np.cos(a[0])
    return r


def _cos(a):
    r = np.empty_like(a)
    r[0] = np.cos(a[0]); r[1:] = -(a[1:] * np.sin(a[0]))
    return r


def _cross(a, b):
    return [_mul(a[1], b[2]) - _mul(a[2], b[1]), _mul(a[2], b[0]) - _mul(a[0], b[2]), _mul(a[0], b[1]) - _mul(a[1], b[0])]


def _dot(a, b):
    return _mul(a[0], b[0]) + _mul(a[1], b[1]) + _mul(a[2], b[2])


def check_rotation_branches(cams):
    """every camera's float64 |w|^2 is exactly 0 or at least 1 % away from the cut of lib.t:517: a float32 evaluation then takes the same branch"""
    w = np.asarray(cams, np.float64)[:, 0:3]
    t2 = (w * w).sum(axis=1)
    assert ((t2 == 0) | (np.abs(t2 - THETA2_CUT) >= 0.01 * THETA2_CUT)).all(), "a camera's |w|^2 is within 1 % of the branch cut 1e-8"
    return t2 > THETA2_CUT


def residual_and_jacobian(cams, pts, obs, q_cam, q_pt, dtype=np.float64, branch=None):
    """F[O, 2] and J[O, 2, 12] of the observations (camera q_cam[q], point q_pt[q], observed obs[q]): residual = observed - predicted, columns 0..8 the camera's
    (w, t, f, l1, l2), 9..11 the point's.  dtype = np.float32: the same arithmetic in float32 (the restatement whose error against float64 sets the kernels' bars).
    branch (per camera, True = Rodrigues' formula): holds the rotation branch instead of choosing it -- for difference quotients, whose steps must not cross the cut."""
    large = (check_rotation_branches(cams) if branch is None else np.asarray(branch, bool))[q_cam]
    cam = np.asarray(cams)[q_cam].astype(dtype); X = np.asarray(pts)[q_pt].astype(dtype); ob = np.asarray(obs).astype(dtype)
    O_ = cam.shape[0]
    var = []
    for k in range(12):
        v = np.zeros((13, O_), dtype)
        v[0] = cam[:, k] if k < 9 else X[:, k - 9]; v[1 + k] = 1
        var.append(v)
    one = _const(var[0], 1)
    aa, t, f, l1, l2, pt = var[0:3], var[3:6], var[6], var[7], var[8], var[9:12]
    with np.errstate(all="ignore"):            # (the branch not taken may divide by zero: select() drops it)
        theta2 = _dot(aa, aa)
        theta = _sqrt(theta2)
        ct, st = _cos(theta), _sin(theta)
        ti = _div(one, theta)
        w = [_mul(a, ti) for a in aa]
        wxp = _cross(w, pt)
        tmp = _mul(_dot(w, pt), one - ct)
        big = [_mul(pt[i], ct) + _mul(wxp[i], st) + _mul(w[i], tmp) for i in range(3)]
        axp = _cross(aa, pt)
        small = [pt[i] + axp[i] for i in range(3)]
    p = [np.where(large[None, :], big[i], small[i]) + t[i] for i in range(3)]
    c = [-_div(p[0], p[2]), -_div(p[1], p[2])]
    r2 = _mul(c[0], c[0]) + _mul(c[1], c[1])
    dist = one + _mul(r2, l1 + _mul(l2, r2))
    res = [_const(one, ob[:, i]) - _mul(_mul(c[i], f), dist) for i in range(2)]
    F = np.stack([res[0][0], res[1][0]], axis=1)
    J = np.stack([res[0][1:].T, res[1][1:].T], axis=1)
    assert F.dtype == dtype and J.dtype == dtype
    return F, J


# ------------------------------------------------------------------ operators on a given block array
def columns(inc):
    """[O, 12]: the flat index of each of a block row's 12 columns"""
    return np.concatenate([9 * inc.q_cam[:, None] + np.arange(9), 9 * inc.C + 3 * inc.q_pt[:, None] + np.arange(3)], axis=1)


def row_counts(inc):
    """observations behind each unknown's row of J^T"""
    return np.concatenate([np.repeat(np.diff(inc.cam_ptr), 9), np.repeat(np.diff(inc.pt_ptr), 3)])


def _blocks(Jb):
    return np.asarray(Jb, np.float64).reshape(-1, 2, 12)


def jt_f(Jb, F, inc):
    """J^T F and sum |J F| per row"""
    J, F = _blocks(Jb), np.asarray(F, np.float64).reshape(-1, 2)
    t = J * F[:, :, None]
    col = np.broadcast_to(columns(inc)[:, None, :], t.shape)
    g, mag = np.zeros(inc.n), np.zeros(inc.n)
    np.add.at(g, col, t); np.add.at(mag, col, np.abs(t))
    return g, mag


def jtj_diag(Jb, inc):
    J = _blocks(Jb)
    d = np.zeros(inc.n)
    np.add.at(d, np.broadcast_to(columns(inc)[:, None, :], J.shape), J * J)
    return d


def apply(Jb, inc, p, ctc=None):
    """(J^T J + CtC) p; the row majorant M_i = sum_q sum_r |J_qri| sum_k |J_qrk p_k| (+ |ctc_i p_i|); the observation count of the row"""
    J, p = _blocks(Jb), np.asarray(p, np.float64)
    col = columns(inc)
    t = J * p[col][:, None, :]
    Jp, aJp = t.sum(axis=2), np.abs(t).sum(axis=2)
    colb = np.broadcast_to(col[:, None, :], J.shape)
    Ap, M = np.zeros(inc.n), np.zeros(inc.n)
    np.add.at(Ap, colb, J * Jp[:, :, None]); np.add.at(M, colb, np.abs(J) * aJp[:, :, None])
    if ctc is not None:
        c = np.asarray(ctc, np.float64)
        Ap += c * p; M += np.abs(c * p)
    return Ap, M, row_counts(inc)


def sums3(pre, r, Ap):
    """[n, 3]: the terms of N = r.M^-1 r, S1 = r.M^-1 Ap, S2 = Ap.M^-1 Ap"""
    m, r, a = (np.asarray(x, np.float64) for x in (pre, r, Ap))
    return np.stack([m * r * r, m * r * a, m * a * a], axis=1)


def sumsq(delta, r, b, p, Ap):
    """[n, 3]: the terms of U = delta.(r + b), T1 = p.(r + b), T2 = delta.Ap"""
    d, r, b, p, a = (np.asarray(x, np.float64) for x in (delta, r, b, p, Ap))
    return np.stack([d * (r + b), p * (r + b), d * a], axis=1)


def lm_q1(U, T1, T2, alpha, alphaD):
    """q_{k+1} = 0.5 [U + alpha (T1 - T2) - alpha^2 alphaD]; returns the value and the sum of its terms' magnitudes"""
    a, ad = float(alpha), float(alphaD)
    with np.errstate(all="ignore"):
        return 0.5 * (U + a * (T1 - T2) - a * a * ad), 0.5 * (abs(U) + abs(a * T1) + abs(a * T2) + abs(a * a * ad))


# ------------------------------------------------------------------ index lists
def incidence(cam_counts, pt_counts, seed=0, plan_order=False):
    """Index lists of an instance whose camera c sees cam_counts[c] observations and whose point j is seen pt_counts[j] times (equal totals).  The caller's observation
    order is a random permutation of any camera order.  plan_order False: the lists in the caller's point ids (a camera's observations in the caller's order, a point's too);
    True: the plan's -- points renumbered by first observing camera (pt_new2old[new] = the caller's id; unobserved points last), a camera's observations by new point id,
    a point's by place in camera order.  q = place of an observation in camera-sorted order; cam_obs[q] its id in the caller's order.
    A camera takes a run of point stubs that are laid out layer by layer, so a run that crosses a layer boundary can hold a point twice: a camera may observe a point more
    than once (it must, where its count exceeds the number of points of a layer -- EDGE's camera with 193 observations over 192 observed points).  No real scene does;
    the lists' format allows it, the kernels and these references treat each observation on its own, and duplicate_pairs() counts them."""
    cam_counts, pt_counts = np.asarray(cam_counts, np.int64), np.asarray(pt_counts, np.int64)
    C_, P_, O_ = cam_counts.size, pt_counts.size, int(cam_counts.sum())
    assert O_ == pt_counts.sum() and O_ > 1
    rng = np.random.default_rng(seed)
    # point stubs layer by layer (every point's first observation, then every second one, ...), shuffled inside a layer: a camera takes a run of them
    stubs = np.concatenate([rng.permutation(np.flatnonzero(pt_counts > k)) for k in range(int(pt_counts.max()))])
    perm = rng.permutation(O_)
    while (perm == np.arange(O_)).all() or (np.diff(np.repeat(np.arange(C_), cam_counts)[perm]) >= 0).all(): perm = rng.permutation(O_)
    oToC, oToP = np.repeat(np.arange(C_), cam_counts)[perm], stubs[perm]
    new2old = np.arange(P_)
    if plan_order:
        first = np.full(P_, C_); np.minimum.at(first, oToP, oToC)
        new2old = np.argsort(first, kind="stable"); old2new = np.empty(P_, np.int64); old2new[new2old] = np.arange(P_)
        oToP = old2new[oToP]
    cam_obs = np.lexsort((np.arange(O_), oToP, oToC)) if plan_order else np.argsort(oToC, kind="stable")
    place = np.empty(O_, np.int64); place[cam_obs] = np.arange(O_)
    q_cam, q_pt = oToC[cam_obs], oToP[cam_obs]
    pt_pos = np.argsort(q_pt, kind="stable") if plan_order else place[np.argsort(oToP, kind="stable")]
    return SimpleNamespace(C=C_, P=P_, O=O_, n=9 * C_ + 3 * P_, cam_ptr=np.concatenate([[0], np.cumsum(np.bincount(oToC, minlength=C_))]), cam_obs=cam_obs, q_cam=q_cam,
                           q_pt=q_pt, pt_ptr=np.concatenate([[0], np.cumsum(np.bincount(oToP, minlength=P_))]), pt_pos=pt_pos, oToC=oToC, oToP=oToP, pt_new2old=new2old)


def duplicate_pairs(inc):
    """observations whose (camera, point) pair an earlier observation has too"""
    return inc.O - np.unique(inc.oToC * inc.P + inc.oToP).size


# ------------------------------------------------------------------ the EDGE instance's counts, a scene for the lists
EDGE_CAMS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 193, 0]


def edge_pt_counts(total):
    """point counts that cover {0, 1, 2, 3, 4, 5, 7, 8, 9}, add up to `total`, and end with a point nothing observes"""
    base = [1, 2, 3, 4, 5, 7, 8, 9, 0]
    rest = total - sum(base)
    assert rest >= 0
    fill = [4] * (rest // 4) + ([rest % 4] if rest % 4 else [])
    return np.array(base[:-1] + fill + [0])


SPECIAL_W2 = (2e-8, 2e-8, 0.5e-8, 0.5e-8, 0.0)      # |w|^2 of a scene's special cameras: on both sides of the cut, and no rotation at all


def scene(inc, seed=0, special=0, noise=1.0, distortion=1.0):
    """float32 cameras [C, 9], points [P, 3] (in the lists' point ids) and observations [O, 2] (the caller's order) for the lists of incidence(): ordinary rotations
    (|w| ~ 0.3); cameras special .. special + 4 have |w|^2 = SPECIAL_W2 (special None: none have); t_z around -6 and |X_k| <= 1, so the depth stays in [-8.3, -3.7]; focal length 400..900;
    l1, l2 of both signs (times `distortion`); observed = predicted (float64) + `noise` pixels."""
    rng = np.random.default_rng(seed)
    C_, P_ = inc.C, inc.P
    cams = np.zeros((C_, 9))
    cams[:, 0:3] = 0.3 * rng.standard_normal((C_, 3))
    if special is not None:
        for c, w2 in enumerate(SPECIAL_W2):
            d = rng.standard_normal(3)
            cams[special + c, 0:3] = d / np.linalg.norm(d) * np.sqrt(w2)
    cams[:, 3:5] = 0.5 * rng.standard_normal((C_, 2)); cams[:, 5] = -6.0 + rng.uniform(-0.5, 0.5, C_)
    cams[:, 6] = rng.uniform(400.0, 900.0, C_)
    cams[:, 7] = distortion * 0.05 * rng.standard_normal(C_); cams[:, 8] = distortion * 0.01 * rng.standard_normal(C_)
    pts = rng.uniform(-1.0, 1.0, (P_, 3))
    cams, pts = cams.astype(np.float32), pts.astype(np.float32)
    F, _ = residual_and_jacobian(cams, pts, np.zeros((inc.O, 2)), inc.oToC, inc.oToP)
    obs = (-F + noise * rng.standard_normal((inc.O, 2))).astype(np.float32)
    return cams, pts, obs
