"""Bundle adjustment's kernels (csrc/energy_ba.hip) one by one against float64 (tests/ba_reference.py, validated on the CPU by tests/test_ba_reference.py).

Instances (u = 2^-24):
  EDGE       11 cameras that see [0, 1, 2, 63, 64, 65, 127, 128, 129, 193, 0] observations -- both sides of the camera kernel's trips of 2 x 64 -- and points that are seen
             {0, 1, 2, 3, 4, 5, 7, 8, 9} times -- both sides of the point kernel's trips of 4; the last point is unobserved.  Cameras 3 .. 7 have |w|^2 = 2e-8, 2e-8, 0.5e-8,
             0.5e-8 and 0 (both rotation branches next to the cut, and no rotation).  In the caller's point order and in the plan's renumbered one.  39 of its 772
             observations repeat a (camera, point) pair (ba_reference.incidence: the 193-observation camera must); every observation is treated on its own.
  CAMSTRIDE  1801 cameras (> 4 x 448: every camera launch strides), 2 - 3 observations each, camera 1795 sees 130; 600 points.
  PTSTRIDE   131 100 points (> 512 x 256: every point launch strides), 1 - 2 observations each; 8 cameras.
Every device buffer is followed by canary words, every output starts as the canary, every input is compared with its bytes afterwards.

Every bar is (i) counted roundings, derived where it is used, (ii) 4 x the same statistic of the float32 restatement of the reference, computed on the CPU in the
test (the `4 e32` convention of tests/test_gpu_block_precond.py), or (iii) an exact / bitwise comparison.  Each test prints its largest error / bar before it asserts.

Launch shapes restated from include/thallo_hip.h and csrc/ba_blocks.hpp's comments: 256 threads; a camera launch has min(ceil(C / 4), 448) workgroups, one wave per
camera, camera c in workgroup (c / 4) mod that; a point launch min(ceil(P / 256), 512), point j in workgroup (j / 256) mod that; the slots of the camera launch first.
The chain of float additions behind a partial is therefore c = max(ceil(C / (4 cam groups)), 3 ceil(P / (256 point groups))) + 6 butterfly levels + 4 waves.

Measured on an MI355X (largest error / bar of each test; also in DESIGN.md "Bundle adjustment's kernels one by one"):
  a. compute_j      scaled errors of the float32 restatement (CPU) | the closed form | the duals (both on the device), per column group and for F; each bar is 4 x the first
                    cameras 3, 4 (near the cut)  rotation 3.73e-3 | 3.73e-3 | 3.73e-3, translation 2.2e-7 | 1.8e-7 | 1.7e-7, f, l1, l2 1.37e-4 | 1.37e-4 | 1.37e-4,
                                                 point 2.4e-7 | 1.7e-7 | 2.0e-7, F 4.23e-6 | 4.23e-6 | 4.23e-6 (plan's order: 5.49e-5 | 5.48e-5 | 5.48e-5)
                    the other cameras            rotation 5.0e-7 | 3.0e-7 | 6.3e-7, translation 1.9e-7 | 2.2e-7 | 1.8e-7, f, l1, l2 1.2e-5 | 9.3e-6 | 1.2e-5,
                                                 point 2.3e-7 | 2.6e-7 | 2.1e-7, F 1.80e-6 | 3.14e-6 | 1.80e-6
                      ... in the plan's order    rotation 3.9e-7 | 3.2e-7 | 5.2e-7, f, l1, l2 5.5e-6 | 9.3e-6 | 5.4e-6, F 1.15e-6 | 4.52e-6 | 1.15e-6
                    largest error / bar: 0.25 (near the cut), 0.44 (others, caller's order), 0.98 (others, plan's order: the closed form's F)
  b. rebuilt block  0 differing entries of 18 528 (EDGE, both orders) and of 111 096 (CAMSTRIDE); Huber and Cauchy: 0 differing from w x plain and from the stored robust Jb
  d. pcg_init       r 0.19, diag 0.49, pre 0.85, r . z partials 0.026
  e. apply / reset  Ap rows 0.24 (CAMSTRIDE, decades, LM), reset rows 0.54 (EDGE, a CtC-only row), p . Ap partials 0.18, (pre r) . r partials 0.074, {N, S1, S2} per slot 0.18
  f. finishes       alphaD words bit for bit, betaN and Q1 0 ulp apart, {U, T1, T2} per slot 0.028
  g. cost           per slot 0.15, sum 0.026
The 43 cases take 4 s."""
from types import SimpleNamespace

import numpy as np
import pytest

import ba_reference as br
import shim_kernels as sk
from shim_kernels import EPS, F32, FIN_TICKET_WORDS, FinT, INVALID, NO_FIN, div32, ref_lm_zeta, ref_scalars_finish, sum_partials, written_slots

pytestmark = pytest.mark.gpu

TAIL = 64                      # canary words behind every device buffer
EPS64 = 2.0 ** -53
PSLOTS = sk.MAX_PARTIALS + 8
GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7), slice(7, 8), slice(8, 9), slice(9, 12))      # rotation, translation, f, l1, l2, point


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


class Buf:
    """A device buffer: the payload `a` (or, a None: `words` elements of `dtype`, every 32-bit word the canary -- an output), then TAIL canary words."""

    def __init__(self, torch, a=None, words=None, dtype=F32):
        self.torch, self.dtype = torch, np.dtype(dtype)
        if a is None: body = np.full(words * self.dtype.itemsize // 4, sk.CANARY, np.uint32)
        else: body = np.ascontiguousarray(a, dtype).view(np.uint32).ravel()
        self.nw = body.size
        self.h0 = np.concatenate([body, np.full(TAIL, sk.CANARY, np.uint32)])
        self.t = torch.from_numpy(self.h0.view(np.int32).copy()).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def words(self):
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[self.nw:] == sk.CANARY).all(), "the canary behind a buffer changed"
        return h[:self.nw]

    def get(self):
        return self.words().view(self.dtype).copy()

    def unchanged(self):
        return self.t.cpu().numpy().tobytes() == self.h0.tobytes()


def out(torch, words, dtype=F32):
    return Buf(torch, None, words, dtype)


def cam_groups(C_): return min((C_ + 3) // 4, 448)
def pt_groups(P_): return max(1, min((P_ + 255) // 256, 512))


class Inst:
    """One instance on the device behind thallo_hip_ba_point_order + thallo_hip_ba_compute_j + thallo_hip_ba_pack_point_blocks, with the device's own Jb and F on the host."""

    def __init__(self, torch, L, name, inc, seed, special):
        self.torch, self.L, self.name, self.inc = torch, L, name, inc
        self.C, self.P, self.O, self.n = inc.C, inc.P, inc.O, inc.n
        self.cams, self.pts, self.obs = br.scene(inc, seed=seed, special=special)
        i32 = lambda a: Buf(torch, a, dtype=np.int32)
        self.d = d = SimpleNamespace(cam_ptr=i32(inc.cam_ptr), cam_obs=i32(inc.cam_obs), q_cam=i32(inc.q_cam), q_pt=i32(inc.q_pt), pt_ptr=i32(inc.pt_ptr), pt_pos=i32(inc.pt_pos),
                                     cams=Buf(torch, self.cams), pts=Buf(torch, self.pts), obs=Buf(torch, self.obs), q_ptk=out(torch, self.O, np.int32),
                                     Jb=out(torch, 24 * self.O), F=out(torch, 2 * self.O), JP=out(torch, 6 * self.O))
        self.inputs = [d.cam_ptr, d.cam_obs, d.q_cam, d.q_pt, d.pt_ptr, d.pt_pos, d.cams, d.pts, d.obs]
        assert L.thallo_hip_ba_point_order(self.O, d.pt_pos.ptr, d.q_ptk.ptr, None) == 0
        assert L.thallo_hip_ba_compute_j(self.O, d.cams.ptr, d.pts.ptr, d.obs.ptr, d.cam_obs.ptr, d.q_cam.ptr, d.q_pt.ptr, d.Jb.ptr, d.F.ptr, None) == 0
        assert L.thallo_hip_ba_pack_point_blocks(self.O, d.Jb.ptr, d.q_ptk.ptr, d.JP.ptr, None) == 0
        torch.cuda.synchronize()
        self.Jb, self.F = d.Jb.get().reshape(self.O, 24), d.F.get().reshape(self.O, 2)
        assert np.isfinite(self.Jb).all() and np.isfinite(self.F).all()
        self.inputs += [d.q_ptk, d.Jb, d.F, d.JP]
        for b in self.inputs[-4:]: b.h0 = np.concatenate([b.words(), b.h0[b.nw:]])         # from here on they are inputs
        self.cb, self.pg = cam_groups(self.C), pt_groups(self.P)
        self.grid = self.cb + self.pg
        assert L.thallo_hip_ba_apply2_camera_slots(self.C, self.P) == self.cb
        self.slot = np.concatenate([np.repeat((np.arange(self.C) // 4) % self.cb, 9), np.repeat(self.cb + (np.arange(self.P) // 256) % self.pg, 3)])
        self.chain_c = -(-self.C // (4 * self.cb)) + 6 + 4
        self.chain_p = 3 * -(-self.P // (256 * self.pg)) + 6 + 4
        self._init = None

    def lists(self, JpC):
        d = self.d
        return (self.C, self.P, d.cam_ptr.ptr, d.q_pt.ptr, d.pt_pos.ptr, d.pt_ptr.ptr, d.cams.ptr, d.pts.ptr, d.JP.ptr, JpC.ptr)

    def inputs_unchanged(self):
        return all(b.unchanged() for b in self.inputs)

    def vec(self, a):
        return Buf(self.torch, np.asarray(a, F32))

    def group_sums(self, terms):
        """float64 sums of per-unknown terms over the camera unknowns and over the point unknowns"""
        t = np.asarray(terms, np.float64)
        return t[:9 * self.C].sum(), t[9 * self.C:].sum()

    def init(self):
        """thallo_hip_ba_pcg_init, once"""
        if self._init is None:
            t, d, n = self.torch, self.d, self.n
            o = SimpleNamespace(**{k: out(t, n) for k in ("r", "pre", "z", "p_prev", "delta", "diag")}, part=out(t, PSLOTS))
            o.ret = self.L.thallo_hip_ba_pcg_init(self.C, self.P, d.cam_ptr.ptr, d.q_pt.ptr, d.pt_ptr.ptr, d.pt_pos.ptr, d.q_cam.ptr, d.Jb.ptr, d.F.ptr, o.r.ptr, o.pre.ptr,
                                                  o.z.ptr, o.p_prev.ptr, o.delta.ptr, o.diag.ptr, o.part.ptr, None)
            t.cuda.synchronize()
            self._init = o
        return self._init


def _counts(name):
    rng = np.random.default_rng(7)
    if name == "EDGE":
        return br.EDGE_CAMS, br.edge_pt_counts(sum(br.EDGE_CAMS))
    if name == "CAMSTRIDE":
        cc = rng.integers(2, 4, 1801); cc[1795] = 130
        O_ = int(cc.sum())
        pc = np.full(600, O_ // 600); pc[:O_ % 600] += 1
        return cc, pc
    pc = rng.integers(1, 3, 131100)
    O_ = int(pc.sum())
    cc = np.full(8, O_ // 8); cc[:O_ % 8] += 1
    return cc, pc


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(name, plan_order=False):
        key = (name, plan_order)
        if key not in cache:
            cc, pc = _counts(name)
            inc = br.incidence(cc, pc, seed=11, plan_order=plan_order)
            cache[key] = Inst(torch, L, name, inc, seed=13, special=3 if name == "EDGE" else None)
        return cache[key]
    return get


ALL = [("EDGE", False), ("EDGE", True), ("CAMSTRIDE", False), ("PTSTRIDE", False)]


def test_the_instances_are_the_ones_the_kernels_edges_need(instances):
    e = instances("EDGE")
    for plan in (False, True):
        inc = instances("EDGE", plan).inc
        assert list(np.diff(inc.cam_ptr)) == [0, 1, 2, 63, 64, 65, 127, 128, 129, 193, 0] and inc.C % 4 != 0
        assert set(np.diff(inc.pt_ptr)) == {0, 1, 2, 3, 4, 5, 7, 8, 9} and np.diff(inc.pt_ptr)[-1] == 0
        assert not (np.diff(inc.oToC) >= 0).all() and br.duplicate_pairs(inc) == 39 and inc.O == 772
    w2 = (e.cams[:, :3].astype(np.float64) ** 2).sum(axis=1)
    assert np.allclose(w2[3:8], br.SPECIAL_W2, rtol=1e-5, atol=0) and w2[7] == 0 and (w2[[0, 1, 2, 8, 9, 10]] > 1e-4).all()
    assert (e.cams[:, 6] >= 400).all() and (e.cams[:, 6] <= 900).all() and (e.cams[:, 5] < -5).all()
    assert (e.cams[:, 7] > 0).any() and (e.cams[:, 7] < 0).any() and (e.cams[:, 8] > 0).any() and (e.cams[:, 8] < 0).any()
    c = instances("CAMSTRIDE").inc
    cnt = np.diff(c.cam_ptr)
    assert c.C == 1801 > 4 * 448 and cnt[1795] == 130 and set(np.delete(cnt, 1795)) == {2, 3} and c.P == 600
    p = instances("PTSTRIDE").inc
    assert p.P == 131100 > 512 * 256 and set(np.diff(p.pt_ptr)) == {1, 2} and p.C == 8


# ------------------------------------------------------------------ a. compute_j
NAMES = ("rotation", "translation", "f", "l1", "l2", "point", "F")
NEAR_CUT = (3, 4)              # EDGE's cameras with |w|^2 = 2e-8: Rodrigues' formula where float32 rounds cos to 1 and 1 - cos to 0


def scaled_stats(F, J, F64, J64, obs):
    """the largest scaled errors, one per column group of the blocks (per observation and residual row the scale is the group's largest |ref|) and one for the residuals
    (scale |observed| + |predicted|): seven figures, in the order of NAMES"""
    F, J = np.asarray(F, np.float64), np.asarray(J, np.float64)
    s7 = []
    with np.errstate(all="ignore"):
        for g in GROUPS:
            e, s = np.abs(J[:, :, g] - J64[:, :, g]).max(axis=2), np.abs(J64[:, :, g]).max(axis=2)
            s7.append(float(np.where(s > 0, e / s, np.where(e > 0, np.inf, 0.0)).max()))
    s7.append(float((np.abs(F - F64) / (np.abs(obs) + np.abs(obs - F64))).max()))
    return np.array(s7)


@pytest.mark.parametrize("plan_order", [False, True])
def test_compute_j_against_float64(torch, L, instances, plan_order):
    """F and all 24 entries of every block of thallo_hip_ba_compute_j (the closed form) and of thallo_hip_ba_compute_j_ad (the duals) against the float64 duals of
    tests/ba_reference.py, at EDGE.  Statistic: the largest scaled error (scaled_stats), taken per column group and for F, and with the two cameras next to the cut on
    Rodrigues' side apart from the rest -- there float32 loses 1 - cos altogether (3.7e-3 of the rotation columns, for any float32 evaluation), and pooled with the others
    that figure would be everybody's bar.  2 x 7 bars, each 4 x the same statistic of the float32 restatement over the same observations -- the factor covers another order
    of the arithmetic (the closed form), fma contraction and the device's sincosf.  F[q] is compared with the reference of observation cam_obs[q], whose observed value
    carries its own pixel of noise: a residual in another place misses its bar (1e-5 .. 2e-4 of |observed| + |predicted|) by orders of magnitude."""
    B = instances("EDGE", plan_order)
    inc = B.inc
    obs_q = B.obs[inc.cam_obs].astype(np.float64)
    F64, J64 = br.residual_and_jacobian(B.cams, B.pts, obs_q, inc.q_cam, inc.q_pt)
    F32_, J32_ = br.residual_and_jacobian(B.cams, B.pts, obs_q, inc.q_cam, inc.q_pt, dtype=np.float32)
    Jad, Fad = out(torch, 24 * B.O), out(torch, 2 * B.O)
    d = B.d
    assert L.thallo_hip_ba_compute_j_ad(B.O, d.cams.ptr, d.pts.ptr, d.obs.ptr, d.cam_obs.ptr, d.q_cam.ptr, d.q_pt.ptr, Jad.ptr, Fad.ptr, None) == 0
    torch.cuda.synchronize()
    forms = {"closed form": (B.F, B.Jb.reshape(-1, 2, 12)), "duals": (Fad.get().reshape(-1, 2), Jad.get().reshape(-1, 2, 12))}
    near = np.isin(inc.q_cam, NEAR_CUT)
    assert near.sum() == 63 + 64 and (~near).sum() == B.O - 127
    worst = []
    for label, m in (("near-cut", near), ("others", ~near)):
        e32 = scaled_stats(F32_[m], J32_[m], F64[m], J64[m], obs_q[m])
        assert (e32 > 0).all() and (e32 < 1e-2).all()
        print("compute_j EDGE", "plan" if plan_order else "caller", label, "e32        ", " ".join("%s %.2e" % x for x in zip(NAMES, e32)))
        for k, (Fd, Jd) in forms.items():
            got = scaled_stats(Fd[m], Jd[m], F64[m], J64[m], obs_q[m])
            print("compute_j EDGE", "plan" if plan_order else "caller", label, "%-11s" % k, " ".join("%s %.2e" % x for x in zip(NAMES, got)), "largest / bar", (got / (4 * e32)).max())
            worst.append((label, k, got, e32))
    for label, k, got, e32 in worst:
        assert (got <= 4 * e32).all(), (label, k, [n for n, ok in zip(NAMES, got <= 4 * e32) if not ok], got, e32)
    assert B.inputs_unchanged()


# ------------------------------------------------------------------ b. the rebuilt block is the stored block
def rebuilt_blocks(torch, L, B, w=None):
    """the 24 entries per observation that the camera launch of J^T (J p) works with, read through J p: p = 1 at unknown k of every camera (point) and 0 elsewhere makes
    J p of observation q exactly (b[k], b[12 + k]) ((b[9 + k], b[21 + k])) -- one non-zero product, times exactly 1, added to zeros"""
    got = np.full((B.O, 24), np.nan, F32)
    for k in range(12):
        p = np.zeros(B.n, F32)
        if k < 9: p[k:9 * B.C:9] = 1
        else: p[9 * B.C + k - 9::3] = 1
        pd, Ap, JpC, part = B.vec(p), out(torch, B.n), out(torch, 2 * B.O), out(torch, PSLOTS)
        if w is None: ret = L.thallo_hip_ba_apply_jtj2(*B.lists(JpC), pd.ptr, Ap.ptr, part.ptr, None, None, None, None, None)
        else: ret = L.thallo_hip_ba_apply_jtj2_fin_robust(*B.lists(JpC), pd.ptr, Ap.ptr, part.ptr, None, None, None, None, NO_FIN, w.ptr, None)
        torch.cuda.synchronize()
        assert ret == B.grid and pd.unchanged()
        j = JpC.get().reshape(B.O, 2)
        got[:, k], got[:, 12 + k] = j[:, 0], j[:, 1]
    return got


@pytest.mark.parametrize("name,plan_order", ALL[:3])
def test_the_rebuilt_block_is_the_stored_block_bit_for_bit(torch, L, instances, name, plan_order):
    """DESIGN.md and thallo_hip.h promise that the operator the camera launch applies -- rebuilt per observation from cameras and points -- is the Jb that
    thallo_hip_ba_compute_j stored and that PCGInit1, the block diagonal, JP and the Schur kernels read.  All 24 entries of every observation, as float32 values (0 == -0)."""
    B = instances(name, plan_order)
    got = rebuilt_blocks(torch, L, B)
    bad = np.argwhere(got != B.Jb)
    print("rebuilt == stored", name, plan_order, "differing entries", len(bad), "of", got.size, "cameras", sorted(set(B.inc.q_cam[bad[:, 0]])) if len(bad) else [])
    assert len(bad) == 0, (bad[:10], got[got != B.Jb][:10], B.Jb[got != B.Jb][:10])
    assert B.inputs_unchanged()


@pytest.mark.parametrize("kind", [1, 2])
def test_the_rebuilt_robust_block_is_the_weight_times_the_plain_one(torch, L, instances, kind):
    """thallo_hip_ba_compute_j_robust's w (Huber, Cauchy at a scale of 1 pixel against 1 pixel of noise: inliers and outliers) handed to thallo_hip_ba_apply_jtj2_fin_robust:
    the rebuilt entries are float32(w x plain entry) -- and so the robust Jb that compute_j_robust stored."""
    B = instances("EDGE")
    d = B.d
    Jr, Fr, w = out(torch, 24 * B.O), out(torch, 2 * B.O), out(torch, B.O)
    assert L.thallo_hip_ba_compute_j_robust(B.O, d.cams.ptr, d.pts.ptr, d.obs.ptr, d.cam_obs.ptr, d.q_cam.ptr, d.q_pt.ptr, kind, 1.0, Jr.ptr, Fr.ptr, w.ptr, None) == 0
    torch.cuda.synchronize()
    wh = w.get()
    w.h0 = np.concatenate([w.words(), w.h0[w.nw:]])
    assert (wh > 0).all() and (wh <= 1).all() and (wh < 1).any() and (kind == 2 or (wh == 1).any())
    got = rebuilt_blocks(torch, L, B, w)
    want = (wh[:, None] * B.Jb).astype(F32)
    print("robust rebuilt", kind, "differing from w x plain", int((got != want).sum()), "from the stored robust Jb", int((got != Jr.get().reshape(B.O, 24)).sum()))
    assert (got == want).all() and (got == Jr.get().reshape(B.O, 24)).all()
    assert w.unchanged() and B.inputs_unchanged()


# ------------------------------------------------------------------ c. point_order, pack_point_blocks
@pytest.mark.parametrize("name,plan_order", ALL)
def test_point_order_and_pack_point_blocks(torch, L, instances, name, plan_order):
    B = instances(name, plan_order)
    q_ptk = B.d.q_ptk.get()
    assert (q_ptk[B.inc.pt_pos] == np.arange(B.O)).all()
    JP = B.d.JP.words().reshape(B.O, 6)
    Jw = B.Jb.view(np.uint32)[B.inc.pt_pos]
    assert (JP == Jw[:, [9, 10, 11, 21, 22, 23]]).all()
    o = out(torch, 8)
    for args in ((0, B.d.pt_pos.ptr, o.ptr), (B.O, None, o.ptr), (B.O, B.d.pt_pos.ptr, None)):
        assert L.thallo_hip_ba_point_order(*args, None) == INVALID
    for args in ((0, B.d.Jb.ptr, B.d.q_ptk.ptr, o.ptr), (B.O, None, B.d.q_ptk.ptr, o.ptr), (B.O, B.d.Jb.ptr, None, o.ptr), (B.O, B.d.Jb.ptr, B.d.q_ptk.ptr, None)):
        assert L.thallo_hip_ba_pack_point_blocks(*args, None) == INVALID
    torch.cuda.synchronize()
    assert o.unchanged() and B.inputs_unchanged()


# ------------------------------------------------------------------ d. pcg_init
@pytest.mark.parametrize("name,plan_order", ALL)
def test_pcg_init_against_float64_of_the_devices_own_blocks(torch, L, instances, name, plan_order):
    """thallo_hip_ba_pcg_init from the device's own Jb and F bits; n_i = observations behind row i.
    r = -J^T F within (2 n_i + 8) u sum |J F|: 2 n_i products and at most 2 n_i additions (a lane's chain and the 6 butterfly levels are among them or add zeros), with room.
    diag within (2 n_i + 2) u diag_i likewise (its terms are positive: sum |terms| = diag).  pre within 5 u of 1 / (1 + sqrt(diag))^2 of the device's diag bits (sqrt, the
    addition, the square, the division: with t = sqrt(diag) the count is [2 t / (1 + t) + 4] u < 6 u in the worst case -- all four errors at their bound with one sign; the bar is
    held at the tighter 5 u).  z == float32(pre r) of the device's own words.  p_prev = delta = 0 in [0, n);
    nothing behind n.  Unobserved camera / point: diag = 0, pre = 1, r = z = 0.  Partials: the return value = written slots = camera + point workgroups; their sum within
    (c + 1) u sum |r z| of the float64 dot of the device's r and z -- c the chain of the file's docstring, + 1 for the product."""
    B = instances(name, plan_order)
    o = B.init()
    r, pre, z, diag = (getattr(o, k).get() for k in ("r", "pre", "z", "diag"))          # (.get() asserts the canary behind n)
    cnt = br.row_counts(B.inc)
    g, mag = br.jt_f(B.Jb, B.F, B.inc)
    d64 = br.jtj_diag(B.Jb, B.inc)
    bar_r, bar_d = (2 * cnt + 8) * EPS * mag, (2 * cnt + 2) * EPS * d64
    ok = cnt > 0
    print("pcg_init", name, plan_order, "r err / bar", (np.abs(r + g)[ok] / bar_r[ok]).max(), "diag err / bar", (np.abs(diag - d64)[ok] / bar_d[ok]).max())
    assert (np.abs(r + g) <= bar_r).all() and (np.abs(diag - d64) <= bar_d).all()
    want_pre = sk.guarded_invert(diag)
    print("   pre err / bar", (np.abs(pre - want_pre) / (5 * EPS * want_pre)).max())
    assert (np.abs(pre - want_pre) <= 5 * EPS * want_pre).all()
    assert sk.same_bytes(z, pre * r)
    assert not o.p_prev.get().any() and not o.delta.get().any()
    un = ~ok
    assert un.any() == (name == "EDGE") and (name != "EDGE" or (un[-3:].all() and un[0:9].all() and un[90:99].all()))
    assert (diag[un] == 0).all() and (pre[un] == 1).all() and (r[un] == 0).all() and (z[un] == 0).all()
    ph = o.part.get()
    assert o.ret == B.grid == written_slots(ph[:, None])
    terms = r.astype(np.float64) * z.astype(np.float64)
    c = max(B.chain_c, B.chain_p)
    err = abs(ph[:B.grid].astype(np.float64).sum() - terms.sum())
    print("   r.z err / bar", err / ((c + 1) * EPS * np.abs(terms).sum()))
    assert err <= (c + 1) * EPS * np.abs(terms).sum()
    assert B.inputs_unchanged()


# ------------------------------------------------------------------ e. apply_jtj2, _lm, lm_reset_residual
def vectors(B, kind, seed):
    rng = np.random.default_rng(seed)
    n = B.n
    gen = (lambda: rng.standard_normal(n).astype(F32)) if kind == "random" else (lambda: (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F32))
    return SimpleNamespace(p=gen(), delta=gen(), r=gen(), b=gen(), pre=rng.uniform(0.1, 1.0, n).astype(F32),
                           ctc=(rng.uniform(0.5, 2.0, n) * 10.0 ** rng.integers(0, 5, n)).astype(F32))


def check_partials(B, what, ph, terms, extra):
    """slots [0, camera slots) add up to the camera part, the others to the point part, each within (its chain + extra) u sum |terms|"""
    t = np.asarray(terms, np.float64)
    wc, wp = B.group_sums(t); mc, mp = B.group_sums(np.abs(t))
    ec, ep = abs(ph[:B.cb].astype(np.float64).sum() - wc), abs(ph[B.cb:B.grid].astype(np.float64).sum() - wp)
    bc, bp = (B.chain_c + extra) * EPS * mc, (B.chain_p + extra) * EPS * mp
    print("  ", what, "partials err / bar: cameras", ec / bc if bc else 0.0, "points", ep / bp if bp else 0.0)
    assert ec <= bc and ep <= bp


def check_slot_sums(B, what, got, terms):
    """double sums per slot within (terms + 8) 2^-53 sum |terms|: a product of float data is exact in double but for its last factor (one rounding; U, T1: the sum r + b
    another), and T terms added in any order pass through at most T - 1 inexact additions (adding a zero is exact)"""
    got = np.asarray(got, np.float64).reshape(-1, 3)[:B.grid]
    cnt = np.bincount(B.slot, minlength=B.grid)
    worst = 0.0
    for j in range(3):
        want = np.bincount(B.slot, weights=terms[:, j], minlength=B.grid); mag = np.bincount(B.slot, weights=np.abs(terms[:, j]), minlength=B.grid)
        bar = (cnt + 8) * EPS64 * mag
        err = np.abs(got[:, j] - want)
        with np.errstate(all="ignore"): worst = max(worst, float(np.nanmax(np.where(bar > 0, err / bar, 0.0))))
        assert (err <= bar).all(), (what, j, np.argmax(err - bar))
    print("  ", what, "per-slot err / bar", worst)


def check_rows(what, got, ref, bar):
    with np.errstate(all="ignore"): ratio = np.where(bar > 0, np.abs(got - ref) / bar, np.where(got == ref, 0.0, np.inf))
    i = int(np.argmax(ratio))
    print("  ", what, "row err / bar", float(ratio[i]), "at row", i)
    assert (np.abs(got - ref) <= bar).all(), (what, i, got[i], ref[i], bar[i])


@pytest.mark.parametrize("kind", ["random", "decades"])
@pytest.mark.parametrize("name,plan_order", ALL)
def test_apply_and_reset_against_float64_of_the_devices_own_blocks(torch, L, instances, name, plan_order, kind):
    """thallo_hip_ba_apply_jtj2 (alone, and with r / pre / s3_out), thallo_hip_ba_apply_jtj2_lm and thallo_hip_ba_lm_reset_residual; p standard normal, and p with
    components of magnitude 1e-3 .. 1e3.  Reference: ba_reference.apply on the device's stored Jb (the rebuilt block is that block: test b).
    Ap per row: |Ap_i - ref_i| <= 1.01 (2 n_i + 24) u M_i, M_i = sum_q sum_r |J_qri| sum_k |J_qrk p_k| (+ |ctc_i p_i|): 12 products and 11 additions in J p, one product per
    term, at most 2 n_i additions + 6 butterfly levels, the CtC term; 1.01 for the second-order terms.  Reset: r = b - A delta within that + u |b_i|.
    Partials (p . Ap; the reset's (pre r) . r): camera slots and point slots each within (chain + 1) u (+ 2 for the reset's two products) of the float64 sums from the
    device's own Ap (r).  N, S1, S2 per slot: check_slot_sums.  The forms that share arguments give the same Ap bits.  A set gate word: nothing is written, same return."""
    B = instances(name, plan_order)
    v = vectors(B, kind, 23)
    d = SimpleNamespace(**{k: B.vec(getattr(v, k)) for k in ("p", "delta", "r", "b", "pre", "ctc")})
    Ap0, M0, cnt = br.apply(B.Jb, B.inc, v.p)
    k1 = 1.01 * (2 * cnt + 24) * EPS

    def run(form, gate=None):
        o = SimpleNamespace(Ap=out(torch, B.n), JpC=out(torch, 2 * B.O), part=out(torch, PSLOTS), s3=out(torch, 3 * PSLOTS, np.float64), r=out(torch, B.n))
        g = None if gate is None else gate.ptr
        if form == "plain": o.ret = L.thallo_hip_ba_apply_jtj2(*B.lists(o.JpC), d.p.ptr, o.Ap.ptr, o.part.ptr, None, None, None, g, None)
        elif form == "sums": o.ret = L.thallo_hip_ba_apply_jtj2(*B.lists(o.JpC), d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, o.s3.ptr, g, None)
        elif form == "lm": o.ret = L.thallo_hip_ba_apply_jtj2_lm(*B.lists(o.JpC), d.p.ptr, d.ctc.ptr, o.Ap.ptr, o.part.ptr, g, None)
        else: o.ret = L.thallo_hip_ba_lm_reset_residual(*B.lists(o.JpC), d.delta.ptr, d.ctc.ptr, d.b.ptr, d.pre.ptr, o.r.ptr, o.part.ptr, g, None)
        torch.cuda.synchronize()
        return o

    print("apply", name, plan_order, kind)
    plain = run("plain")
    Ap = plain.Ap.get()
    check_rows("apply_jtj2 Ap", Ap, Ap0, k1 * M0)
    ph = plain.part.get()
    assert plain.ret == B.grid == written_slots(ph[:, None]) and plain.s3.unchanged() and plain.r.unchanged()
    check_partials(B, "p.Ap", ph, v.p.astype(np.float64) * Ap, 1)
    assert np.isfinite(plain.JpC.get()).all()

    sums = run("sums")
    assert sums.ret == B.grid and sk.same_bytes(sums.Ap.get(), Ap) and sk.same_bytes(sums.part.get(), ph)
    s3 = sums.s3.get()
    assert written_slots(s3.reshape(-1, 3)) == B.grid
    check_slot_sums(B, "{N, S1, S2}", s3, br.sums3(v.pre, v.r, Ap))

    lm = run("lm")
    Al = lm.Ap.get()
    c64, p64 = v.ctc.astype(np.float64), v.p.astype(np.float64)
    check_rows("apply_jtj2_lm Ap", Al, Ap0 + c64 * p64, k1 * (M0 + np.abs(c64 * p64)))
    pl = lm.part.get()
    assert lm.ret == B.grid == written_slots(pl[:, None])
    check_partials(B, "p.(A + CtC)p", pl, p64 * Al, 1)

    rs = run("reset")
    Ad, Md, _ = br.apply(B.Jb, B.inc, v.delta, v.ctc)
    rr = rs.r.get()
    b64 = v.b.astype(np.float64)
    check_rows("lm_reset_residual r", rr, b64 - Ad, k1 * Md + EPS * np.abs(b64))
    pr = rs.part.get()
    assert rs.ret == B.grid == written_slots(pr[:, None]) and rs.Ap.unchanged()
    check_partials(B, "(pre r).r", pr, v.pre.astype(np.float64) * rr * rr, 2)

    gate = Buf(torch, np.array([1], np.uint32), dtype=np.uint32)
    for form in ("plain", "sums", "lm", "reset"):
        o = run(form, gate)
        assert o.ret == B.grid and all(b.unchanged() for b in (o.Ap, o.JpC, o.part, o.s3, o.r)), form
    assert gate.unchanged() and all(b.unchanged() for b in vars(d).values()) and B.inputs_unchanged()


def test_the_argument_combinations_that_are_refused(torch, L, instances):
    """what ba_apply2 and its entry points reject returns -hipErrorInvalidValue and writes nothing"""
    B = instances("EDGE")
    v = vectors(B, "random", 5)
    d = SimpleNamespace(**{k: B.vec(getattr(v, k)) for k in ("p", "delta", "r", "b", "pre", "ctc")})
    o = SimpleNamespace(Ap=out(torch, B.n), JpC=out(torch, 2 * B.O), part=out(torch, PSLOTS), s3=out(torch, 3 * PSLOTS, np.float64), q3=out(torch, 3 * PSLOTS, np.float64),
                        r=out(torch, B.n), words=out(torch, 2), state=out(torch, 8))
    tickets = Buf(torch, np.zeros(FIN_TICKET_WORDS, np.uint32), dtype=np.uint32)
    aN = Buf(torch, np.array([1.0], F32))
    lists = B.lists(o.JpC)
    fin = FinT(sk.api.SumT(aN.ptr, 1), tickets.ptr, o.words.ptr, o.words.ptr + 4)
    A, P = L.thallo_hip_ba_apply_jtj2, L.thallo_hip_ba_apply_jtj2_fin
    rets = []
    for i in range(2, 10):          # a missing list, the cameras, the points, JP or JpC
        a = list(lists); a[i] = None
        rets.append(A(*a, d.p.ptr, o.Ap.ptr, o.part.ptr, None, None, None, None, None))
    rets += [A(*lists, None, o.Ap.ptr, o.part.ptr, None, None, None, None, None), A(*lists, d.p.ptr, None, o.part.ptr, None, None, None, None, None),
             A(*lists, d.p.ptr, o.Ap.ptr, None, None, None, None, None, None),
             A(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, None, d.pre.ptr, o.s3.ptr, None, None), A(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, None, o.s3.ptr, None, None),
             P(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, None, None, None, None, fin, None),                                  # tickets without the sums
             P(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, o.s3.ptr, o.state.ptr, fin, None),              # tickets and a gate
             P(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, o.s3.ptr, None, FinT(fin.alphaN, tickets.ptr, None, o.words.ptr), None),
             P(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, o.s3.ptr, None, FinT(fin.alphaN, tickets.ptr, o.words.ptr, None), None),
             P(*lists, d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, o.s3.ptr, None, FinT(sk.api.SumT(None, 0), tickets.ptr, o.words.ptr, o.words.ptr + 4), None),
             L.thallo_hip_ba_apply_jtj2_lm(*lists, d.p.ptr, None, o.Ap.ptr, o.part.ptr, None, None)]
    R = L.thallo_hip_ba_lm_reset_residual
    full = [d.delta.ptr, d.ctc.ptr, d.b.ptr, d.pre.ptr, o.r.ptr, o.part.ptr]
    for i in range(6):
        a = list(full); a[i] = None
        rets.append(R(*lists, *a, None, None))
    Q = L.thallo_hip_ba_pcg_apply_lm
    full = [d.p.ptr, d.ctc.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, d.delta.ptr, d.b.ptr, o.s3.ptr, o.q3.ptr]
    for i in (1, 6, 7, 8, 9):
        a = list(full); a[i] = None
        rets.append(Q(*lists, *a, fin, o.state.ptr, 0, 0.1, 0, 0, None))
    rets += [Q(*lists, *full, fin, None, 0, 0.1, 0, 0, None), Q(*lists, *full, fin, o.state.ptr, 0, 0.1, 8, 0, None), Q(*lists, *full, fin, o.state.ptr, 0, 0.1, 0, -1, None),
             Q(*lists, *full, fin, o.state.ptr, 0, 0.1, 0, 8, None)]
    torch.cuda.synchronize()
    assert rets == [INVALID] * len(rets), rets
    assert all(b.unchanged() for b in list(vars(o).values()) + list(vars(d).values()) + [tickets, aN]) and B.inputs_unchanged()


# ------------------------------------------------------------------ f. the finishes
@pytest.mark.parametrize("name", ["EDGE", "CAMSTRIDE"])
def test_apply_jtj2_fin_finishes_the_iterations_scalars(torch, L, instances, name):
    """thallo_hip_ba_apply_jtj2_fin with tickets: the point launch's last workgroup adds up the slots of both launches (3 + 1 at EDGE, 448 + 3 at CAMSTRIDE: the point
    launch's slot offset matters at both).  alphaD_word == sum_partials of the slots bit for bit; betaN_word within 1 ulp of ref_scalars_finish (a double expression the
    compiler may contract; its condition number is asserted); the tickets are zero again and nothing is written behind the two words.  Ap, the partials and the sums are
    the plain form's bits."""
    B = instances(name)
    v = vectors(B, "random", 31)
    d = SimpleNamespace(**{k: B.vec(getattr(v, k)) for k in ("p", "r", "pre")})
    aNv = F32((v.pre.astype(np.float64) * v.r * v.r).sum())
    aN = Buf(torch, np.array([aNv], F32))
    res = []
    for with_fin in (False, True):
        o = SimpleNamespace(Ap=out(torch, B.n), JpC=out(torch, 2 * B.O), part=out(torch, PSLOTS), s3=out(torch, 3 * PSLOTS, np.float64), words=out(torch, 2),
                            tickets=Buf(torch, np.zeros(FIN_TICKET_WORDS, np.uint32), dtype=np.uint32))
        fin = FinT(sk.api.SumT(aN.ptr, 1), o.tickets.ptr, o.words.ptr, o.words.ptr + 4) if with_fin else NO_FIN
        assert L.thallo_hip_ba_apply_jtj2_fin(*B.lists(o.JpC), d.p.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, o.s3.ptr, None, fin, None) == B.grid
        torch.cuda.synchronize()
        res.append(o)
    a, b = res
    assert a.words.unchanged() and b.tickets.unchanged()
    for k in ("Ap", "part", "s3", "JpC"): assert sk.same_bytes(getattr(a, k).words(), getattr(b, k).words()), k
    ph, s3, w = b.part.get(), b.s3.get(), b.words.get()
    assert written_slots(ph[:, None]) == B.grid and B.cb > 1 and B.pg >= 1
    adw, alpha, bnw, mag = ref_scalars_finish(ph[:B.grid], s3[:3 * B.grid], aNv)
    print("apply_jtj2_fin", name, "alphaD", w[0], adw, "betaN", w[1], bnw, "ulps", sk.ulp_apart(w[1], bnw))
    assert sk.same_bytes(w[0:1], adw)
    assert float(bnw) > 0 and mag / float(bnw) < 2.0 ** 20
    assert sk.ulp_apart(w[1], bnw) <= 1
    assert aN.unchanged() and all(x.unchanged() for x in vars(d).values()) and B.inputs_unchanged()


def lm_launch(torch, L, B, d, aN, state0, k, tol, q_in, q_out, tickets=True):
    o = SimpleNamespace(Ap=out(torch, B.n), JpC=out(torch, 2 * B.O), part=out(torch, PSLOTS), s3=out(torch, 3 * PSLOTS, np.float64), q3=out(torch, 3 * PSLOTS, np.float64),
                        words=out(torch, 2), tickets=Buf(torch, np.zeros(FIN_TICKET_WORDS, np.uint32), dtype=np.uint32), state=Buf(torch, state0))
    fin = FinT(sk.api.SumT(aN.ptr, 1), o.tickets.ptr if tickets else None, o.words.ptr, o.words.ptr + 4)
    o.ret = L.thallo_hip_ba_pcg_apply_lm(*B.lists(o.JpC), d.p.ptr, d.ctc.ptr, o.Ap.ptr, o.part.ptr, d.r.ptr, d.pre.ptr, d.delta.ptr, d.b.ptr, o.s3.ptr, o.q3.ptr, fin,
                                         o.state.ptr, k, tol, q_in, q_out, None)
    torch.cuda.synchronize()
    return o


def lm_state(Q0, frozen, its, decoy, q_in):
    s = np.zeros(8, F32)
    s[[0, 3, 4, 5, 6, 7]] = decoy; s[q_in] = Q0
    s.view(np.uint32)[1] = frozen; s.view(np.int32)[2] = its
    return s


@pytest.mark.parametrize("words", [(0, 0), (0, 6), (6, 0)])
@pytest.mark.parametrize("case", ["continue", "stop", "frozen", "zero"])
def test_pcg_apply_lm_sums_finish_and_zeta_test(torch, L, instances, case, words):
    """thallo_hip_ba_pcg_apply_lm at EDGE, k = 4, q_tolerance = 1.  First with fin.tickets = NULL: partials only, the state untouched; {U, T1, T2} per slot against sumsq on
    the device's Ap (check_slot_sums), Ap and {N, S1, S2} the bits of thallo_hip_ba_apply_jtj2_lm and of the sums form.  From the device's own partials, in the documented
    order: alphaD = sum_partials, alpha = alphaN / alphaD unguarded in float32, Q1 = float32(0.5 [U + alpha (T1 - T2) - alpha^2 alphaD]).  Then the in-kernel finish, with
    Q0 in state[q_in] and a decoy in every other free word so that reading the wrong word flips the verdict: continue (Q0 = Q1 / 2: zeta = 2.5): state[q_out] = Q1 to
    1 ulp, nothing else changes; stop (Q0 = Q1: zeta = 0 < 1): frozen = 1, iterations = 5; frozen before: both launches do nothing; zero (alphaN = 0, delta = 0:
    Q0 = Q1 = 0, zeta = 0 / 0): stop.  Then (q_in != q_out) thallo_hip_pcg_update_lm_fin on the deferred run's partials: the same alphaD, betaN and state words bitwise."""
    B = instances("EDGE")
    q_in, q_out = words
    k, tol = 4, 1.0
    v = vectors(B, "random", 41)
    if case == "zero": v.delta[:] = 0
    d = SimpleNamespace(**{key: B.vec(getattr(v, key)) for key in ("p", "delta", "r", "b", "pre", "ctc")})
    aNv = F32(0.0) if case == "zero" else F32((v.pre.astype(np.float64) * v.r * v.r).sum())
    aN = Buf(torch, np.array([aNv], F32))
    s_any = lm_state(1.0, 0, 0, 2.0, q_in)
    de = lm_launch(torch, L, B, d, aN, s_any, k, tol, q_in, q_out, tickets=False)
    assert de.ret == B.grid and de.state.unchanged() and de.words.unchanged() and de.tickets.unchanged()
    ph, s3, q3, Ap = de.part.get(), de.s3.get(), de.q3.get(), de.Ap.get()
    assert written_slots(ph[:, None]) == written_slots(s3.reshape(-1, 3)) == written_slots(q3.reshape(-1, 3)) == B.grid
    check_slot_sums(B, "{N, S1, S2}", s3, br.sums3(v.pre, v.r, Ap))
    check_slot_sums(B, "{U, T1, T2}", q3, br.sumsq(v.delta, v.r, v.b, v.p, Ap))
    lmo = SimpleNamespace(Ap=out(torch, B.n), JpC=out(torch, 2 * B.O), part=out(torch, PSLOTS))
    assert L.thallo_hip_ba_apply_jtj2_lm(*B.lists(lmo.JpC), d.p.ptr, d.ctc.ptr, lmo.Ap.ptr, lmo.part.ptr, None, None) == B.grid
    torch.cuda.synchronize()
    assert sk.same_bytes(lmo.Ap.get(), Ap) and sk.same_bytes(lmo.part.get(), ph)
    adw = sum_partials(ph[:B.grid]); alpha = div32(aNv, adw, False)
    U, T1, T2 = (sk.sum_partials_f64(q3.reshape(-1, 3)[:B.grid, j]) for j in range(3))
    Q1, qmag = br.lm_q1(U, T1, T2, alpha, adw)
    _, _, bnw, bmag = ref_scalars_finish(ph[:B.grid], s3[:3 * B.grid], aNv, guard=False)
    if case == "zero": assert Q1 == 0 and float(alpha) == 0
    else: assert np.isfinite(Q1) and Q1 != 0 and qmag / abs(Q1) < 2.0 ** 20 and float(bnw) > 0 and bmag / float(bnw) < 2.0 ** 20
    Q0, decoy = {"continue": (0.5 * Q1, Q1), "stop": (Q1, 0.5 * Q1), "frozen": (0.5 * Q1, Q1), "zero": (0.0, 0.0)}[case]
    s0 = lm_state(Q0, 1 if case == "frozen" else 0, 2 if case == "frozen" else 0, decoy, q_in)
    o = lm_launch(torch, L, B, d, aN, s0, k, tol, q_in, q_out)
    assert o.ret == B.grid and o.tickets.unchanged()
    sh = o.state.get()
    if q_in != q_out:          # the deferred finish on the partials of the run without tickets (its loop alternates the words: equal ones are refused)
        n = B.n
        dv = [sk.DVec(torch, n, x) for x in (v.r, Ap, v.pre, v.p, None, v.delta)]
        w2, st2 = out(torch, 2), Buf(torch, s0)
        assert L.thallo_hip_pcg_update_lm_fin(*(x.ptr for x in dv), n, sk.api.SumT(aN.ptr, 1), de.part.ptr, de.s3.ptr, de.q3.ptr, B.grid, w2.ptr, w2.ptr + 4, st2.ptr,
                                              k, tol, q_in, q_out, None) == 0
        torch.cuda.synchronize()
        assert sk.same_bytes(st2.get(), sh) and sk.same_bytes(w2.words(), o.words.words()) and all(x.canary_ok() for x in dv)
    if case == "frozen":
        assert o.state.unchanged() and all(b.unchanged() for b in (o.Ap, o.JpC, o.part, o.s3, o.q3, o.words))
        return
    for key in ("Ap", "part", "s3", "q3", "JpC"): assert sk.same_bytes(getattr(o, key).words(), getattr(de, key).words()), key
    w = o.words.get()
    assert sk.same_bytes(w[0:1], adw) and sk.ulp_apart(w[1], bnw) <= 1
    new = ref_lm_zeta((float(F32(Q0)), 0, 0), float(F32(Q1)), k, tol)
    want = s0.copy()
    if case == "continue":
        assert new[1] == 0
        want[q_out] = sh[q_out]
        print("pcg_apply_lm", case, words, "Q1", sh[q_out], Q1, "ulps", sk.ulp_apart(sh[q_out], F32(Q1)))
        assert sk.same_bytes(sh, want) and sk.ulp_apart(sh[q_out], F32(Q1)) <= 1
    else:
        assert new[1:] == (1, k + 1)
        want.view(np.uint32)[1] = 1; want.view(np.int32)[2] = k + 1
        assert sk.same_bytes(sh, want), (sh, want)
    assert aN.unchanged() and all(x.unchanged() for x in vars(d).values()) and B.inputs_unchanged()


# ------------------------------------------------------------------ g. ba_cost
@pytest.mark.parametrize("name,plan_order", ALL)
def test_cost_against_float64_of_the_devices_own_residuals(torch, L, instances, name, plan_order):
    """thallo_hip_ba_cost, with oToC / oToP in the caller's observation order: ceil(O / 256) slots (at most 1024), observation o in slot (o / 256) mod that; each slot and
    their sum against sum 1/2 (F0^2 + F1^2) of thallo_hip_ba_compute_j's own F bits (the same float32 expression of the residual; F[q] is observation cam_obs[q]) within
    (c + 4) u sum terms: c = the observations a lane visits + 6 butterfly levels + 4 waves additions; the two squares, their sum and the accumulation's first."""
    B = instances(name, plan_order)
    oc, op, part = Buf(torch, B.inc.oToC, dtype=np.int32), Buf(torch, B.inc.oToP, dtype=np.int32), out(torch, PSLOTS)
    nb = L.thallo_hip_ba_cost(B.C, B.P, B.O, B.d.cams.ptr, B.d.pts.ptr, B.d.obs.ptr, oc.ptr, op.ptr, part.ptr, None)
    torch.cuda.synchronize()
    grid = (B.O + 255) // 256
    assert grid <= 1024 and (name == "EDGE" or grid > 1)
    ph = part.get()
    assert nb == grid == written_slots(ph[:, None])
    place = np.empty(B.O, np.int64); place[B.inc.cam_obs] = np.arange(B.O)
    terms = 0.5 * (B.F.astype(np.float64) ** 2).sum(axis=1)[place]
    slot = (np.arange(B.O) // 256) % grid
    want = np.bincount(slot, weights=terms, minlength=grid)
    c = -(-B.O // (256 * grid)) + 6 + 4
    err = np.abs(ph[:grid].astype(np.float64) - want)
    print("cost", name, plan_order, "per-slot err / bar", (err / ((c + 4) * EPS * want)).max(), "sum err / bar", abs(ph[:grid].astype(np.float64).sum() - terms.sum()) / ((c + 4) * EPS * terms.sum()))
    assert (err <= (c + 4) * EPS * want).all()
    assert abs(ph[:grid].astype(np.float64).sum() - terms.sum()) <= (c + 4) * EPS * terms.sum()
    assert oc.unchanged() and op.unchanged() and B.inputs_unchanged()
