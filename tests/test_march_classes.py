"""CPU: the model of the marching kernel's loop classes (tests/march_classes.py) follows the library, and the forced-R sweep of
tests/test_gpu_march_segments.py leaves no class out that a launch can reach.  No GPU compute here."""
import ctypes as C

import pytest

import thallo_amd
import march_classes as mc

# every shape the GPU suite fed to the marching kernel at its AUTOMATIC rows per segment before the forced-R sweep existed (test_gpu_parity.py: cost trajectory,
# without-the-A-p-plane, ring of p planes, resident-is-bitwise-the-marching-kernel, the large sizes)
SHAPES_BEFORE = [(64, 64), (96, 80), (70, 33), (256, 256), (130, 3), (252, 41), (2048, 2048), (1024, 768), (130, 7), (124, 64), (250, 2), (126, 130), (2, 1), (372, 5),
                 (8192, 4096), (16384, 11264), (512, 512), (2048, 256), (2048, 512), (1024, 1024), (1200, 800), (640, 480)]


@pytest.fixture(scope="module")
def L():
    from thallo_amd.build import build_library
    build_library()
    lib = thallo_amd.lib()
    lib.thallo_hip_iw_march_rows.restype = C.c_int
    lib.thallo_hip_iw_march_rows.argtypes = [C.c_int, C.c_int]
    return lib


@pytest.mark.parametrize("cap", [8, 32, 112, 256, 304, 1024])
def test_model_follows_the_librarys_rows_per_segment(L, cap):
    """thallo_hip_iw_march_rows under a forced workgroup budget (debug knob 6: host logic only) against the model, over widths of one to many strips and heights
    from one row up; a forced R is returned as it is"""
    shapes = [(2, 1), (124, 64), (126, 130), (250, 2), (372, 5), (1024, 768), (2048, 256), (2048, 2048), (1200, 800), (8192, 4096), (16384, 11264), (124 * 256 + 2, 64)]
    try:
        L.thallo_hip_march_debug_set(6, cap)
        for W, H in shapes:
            assert L.thallo_hip_iw_march_rows(W, H) == mc.pick_rows(W, H, 0, forced_cap=cap), (W, H, cap)
        L.thallo_hip_march_debug_set(0, 27)
        assert L.thallo_hip_iw_march_rows(2048, 2048) == mc.pick_rows(2048, 2048, 0, forced_rows=27, forced_cap=cap) == 27
    finally:
        L.thallo_hip_march_debug_set(0, 0)
        L.thallo_hip_march_debug_set(6, 0)


def test_the_iteration_block_mirror_has_the_librarys_size(L):
    """api.IwIterT mirrors thallo_iw_iter_t field by field; a field added on one side only changes the size on that side"""
    from thallo_amd import api
    assert C.sizeof(api.IwIterT) == L.thallo_hip_iw_iter_size()


def test_depth_n_pairs_of_the_automatic_geometry_on_256_cus():
    """what the automatic rows per segment reach on a 256-CU device: the table the forced-R sweep was written against"""
    pairs = mc.depth_n_pairs(SHAPES_BEFORE, cus=256)
    assert sorted(n for d, n in pairs if d == 2) == [1, 2, 3, 4, 5, 7, 8, 9, 10]
    assert sorted(n for d, n in pairs if d == 4) == [18, 35, 334, 342, 383, 403]


def test_phase_arithmetic_takes_every_row_once():
    """head (4 steps) + 4 K + T = n + 4 and T <= DEPTH + 5 (asserted inside phases) for every segment up to 60 rows, both depths, every mode, every position"""
    for DEPTH in (2, 4):
        for DMODE in (0, 1, 2):
            for n in range(1, 61):
                for below in (0, 1, 2, 50):
                    for ya in (0, 1, 9):
                        mc.phases(ya, ya + n, ya + n + below, DEPTH, DMODE)


def test_the_sweep_covers_every_reachable_class():
    """A condition, not a measurement: every (DEPTH, DMODE, ends at the image's last row, K clipped at 3, T) that a whole-image launch with segments of up to 40 rows
    can execute is executed by a case of the bit-for-bit sweep and by a case of the float64 comparison."""
    want = mc.reachable_whole()
    have = set()
    for W, H, R, planes in mc.sweep_cases():
        assert W % 2 == 0 and W <= 372 and H <= 120 and mc.grid(W, 0, H, R) <= mc.MAX_PARTIALS
        have |= mc.case_classes(W, H, R, planes, mc.SWEEP_LIT)
    missing = sorted(want - have)
    print("classes reachable:", len(want), "executed by the sweep:", len(have & want), "missing:", missing)
    assert not missing, missing
    # the phase arithmetic alone, any segment length at any place (DMODE 0 and 2 taken together: they share the arithmetic, not the code): 154 classes
    free = {(d, dm == 1, b, min(ph["K"], mc.K_CLIP), ph["T"]) for d in (2, 4) for dm in (0, 1) for b in (0, 1) for n in range(1, 41)
            for ph in [mc.phases(10, 10 + n, 10 + n + (0 if b else 50), d, dm)]}
    assert len(free) == 154
    # the ninth tail step (T = DEPTH + 5) and T = 7 at depth 2: what no test executed before
    assert any(c[0] == 4 and c[4] == 9 for c in have) and any(c[0] == 2 and c[4] == 7 for c in have)
    # every width under every delta schedule at both depths
    assert {(W, planes, mc.depth(R)) for W, H, R, planes in mc.sweep_cases()} == {(W, pl, d) for W in mc.SWEEP_WIDTHS for pl in mc.SWEEP_PLANES for d in (2, 4)}
    ref = set()
    for W, H, R, planes in mc.reference_cases():
        ref |= mc.case_classes(W, H, R, planes, mc.SWEEP_LIT)
    assert ref == want


def test_the_slab_cases_run_depth_4_with_short_and_full_last_segments():
    """the classes only a slab reaches -- a SHORT segment above a ghost row -- : every (K, T) of them at depth 4 is the last segment of an interior rank of a slab case
    (the delta mode is the transport's schedule); short and full last segments both above a ghost row and on the bottom rank"""
    only = {(c[0], c[3], c[4]) for c in mc.reachable_slab_only()}
    got, lasts = set(), set()
    for world, W, counts, R in mc.SLAB_CASES:
        assert 2 <= world <= 3 and len(counts) == world and W % 4 == 0 and mc.depth(R) == 4
        got |= {(c[0], c[3], c[4]) for c in mc.slab_classes(counts, R) if not c[2]}
        for rank in range(world):
            Hl, row0, row1 = mc.slab_layout(counts, rank)
            assert mc.grid(W, row0, row1, R, deferred=True) <= mc.MAX_PARTIALS
            ya, yb = mc.segments(row0, row1, R)[-1]
            lasts.add((rank < world - 1, yb - ya == R))
    assert lasts == {(True, True), (True, False), (False, True), (False, False)}      # (ghost row below?, full last segment?)
    print("slab-only (DEPTH, K, T):", len(only), "executed by the slab cases:", len(only & got), "missing:", sorted(only - got))
    assert not {c for c in only if c[0] == 4} - got
    assert any(c[0] == 4 and c[4] == 9 and c[2] for _, _, counts, R in mc.SLAB_CASES for c in mc.slab_classes(counts, R))      # the ninth tail step on a bottom rank
