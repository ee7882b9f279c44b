"""CPU: where the marching kernels put every wave of a launch.  The kernels compute the placement in front of their first load with 32-bit arithmetic and a
multiplier the host hands over (march_place_at, thallo_amd/csrc/iw_march.hpp); thallo_hip_iw_march_place runs that same code on the host.  Here it is compared
with a restatement of the formula the kernels used before -- 64-bit products and divisions by the run-time group count and strip count -- for every workgroup and
wave of every grid, and the placements of a launch must cover every (strip, segment) exactly once.  No GPU compute here."""
import ctypes as C

import numpy as np
import pytest

import thallo_amd
import march_classes as mc

WIDTHS = (2, 126, 250, 2048, 16384)
ROWS = (2, 7, 35, 2048)
RS = (1, 8, 35)                     # rows per wave segment, as the tests' knob forces them
GRIDS = (8, 16, 256, 1024)
INVALID = -1                        # -hipErrorInvalidValue


@pytest.fixture(scope="module")
def L():
    from thallo_amd.build import build_library
    build_library()
    lib = thallo_amd.lib()
    lib.thallo_hip_iw_march_place.restype = C.c_int
    lib.thallo_hip_iw_march_place.argtypes = [C.c_int] * 5 + [C.c_void_p]
    return lib


def place(L, W, row0, row1, R, grid):
    out = np.full((max(grid, 1), mc.WAVES, 3), -7, dtype=np.int32)
    rc = L.thallo_hip_iw_march_place(W, row0, row1, R, grid, out.ctypes.data)
    return rc, out


def place_before(W, row0, row1, R, grid):
    """march_place as it stood: G groups of workgroups (8 where the grid is a multiple of 8, else 1), group grp owns the ids [total grp / G, total (grp + 1) / G),
    id -> (strip = id % nstrips, band = id / nstrips), wave w of the band's workgroup takes segment 4 band + w; Python integers, so nothing overflows"""
    nstrips = (W + mc.MARCH_USE - 1) // mc.MARCH_USE
    nseg = (row1 - row0 + R - 1) // R
    total = nstrips * ((nseg + mc.WAVES - 1) // mc.WAVES)
    G = 8 if grid % 8 == 0 else 1
    out = np.zeros((grid, mc.WAVES, 3), dtype=np.int64)
    for b in range(grid):
        grp, l = b % G, b // G
        lo, hi = total * grp // G, total * (grp + 1) // G
        ident = lo + l
        if ident < hi:
            for w in range(mc.WAVES):
                seg = (ident // nstrips) * mc.WAVES + w
                ya = row0 + seg * R
                out[b, w] = (ident % nstrips, min(ya, row1), min(ya + R, row1))
    return total, out


def geometries():
    out = [(W, 0, rows, R) for W in WIDTHS for rows in ROWS for R in RS]
    # row slabs: a ghost row above the owned rows (row0 = 1), as the multi-GPU launches place them
    out += [(128, 1, 17, 8), (252, 1, 38, 24), (2048, 1, 513, 35), (2, 1, 2, 1)]
    return out


@pytest.mark.parametrize("W,row0,row1,R", geometries())
def test_placement_is_the_formula_it_replaces_on_every_grid(L, W, row0, row1, R):
    """every (workgroup, wave) of grids of 8, 16, 256 and 1024 workgroups, of the launch's own grid and of that grid with the deferred cross-rank finish's eight
    extra workgroups; what no launcher can run -- more (strip, band) ids than partial slots -- is refused instead of being placed with arithmetic that is too narrow"""
    total = place_before(W, row0, row1, R, 8)[0]
    own = mc.grid(W, row0, row1, R)
    if total > mc.MAX_PARTIALS:
        assert own > mc.MAX_PARTIALS                         # (the launchers refuse the grid)
        for grid in GRIDS:
            assert place(L, W, row0, row1, R, grid)[0] == INVALID
        return
    nstrips = (W + mc.MARCH_USE - 1) // mc.MARCH_USE
    segs = mc.segments(row0, row1, R)
    for grid in sorted(set(GRIDS) | {own, own + 8}):
        if grid > mc.MAX_PARTIALS:
            assert place(L, W, row0, row1, R, grid)[0] == INVALID
            continue
        rc, got = place(L, W, row0, row1, R, grid)
        assert rc == 0, (grid, rc)
        _, want = place_before(W, row0, row1, R, grid)
        assert np.array_equal(got.astype(np.int64), want), (grid, np.argwhere(got != want)[:4])
        # a grid of at least the launch's own places every (strip, segment) exactly once; a smaller one places no (strip, segment) twice
        work = got[got[:, :, 1] < got[:, :, 2]]
        placed = sorted((int(s), int(ya), int(yb)) for s, ya, yb in work)
        assert len(set(placed)) == len(placed)
        if grid >= own:
            assert placed == sorted((s, ya, yb) for s in range(nstrips) for ya, yb in segs), grid


def test_a_grid_no_launcher_makes_is_refused(L):
    """every launcher rounds its grid up to a multiple of 8 workgroups (the XCD count), so the kernels no longer carry the one-group branch of the old formula: the
    host mirror says so instead of placing such a grid differently from the kernels"""
    for grid in (0, 1, 7, 12, 257, 1025, 1032):
        assert place(L, 2048, 0, 2048, 35, grid)[0] == INVALID, grid
    assert L.thallo_hip_iw_march_place(2048, 0, 2048, 35, 256, None) == INVALID
    for W, row0, row1, R in ((3, 0, 8, 4), (0, 0, 8, 4), (64, 4, 4, 4), (64, -1, 4, 4), (64, 0, 8, 0)):
        assert place(L, W, row0, row1, R, 8)[0] == INVALID, (W, row0, row1, R)


def test_the_launchers_grids_are_multiples_of_eight():
    """... which is what makes the one-group branch unreachable: the model of the launch geometry (tests/march_classes.py, pinned to the sources' constants and to the
    library by tests/test_march_classes.py) over the shapes of this file and of the sweep"""
    for W, row0, row1, R in geometries():
        assert mc.grid(W, row0, row1, R) % 8 == 0 and mc.grid(W, row0, row1, R, deferred=True) % 8 == 0
    for W, H, R, _ in mc.sweep_cases():
        assert mc.grid(W, 0, H, R) % 8 == 0


def test_the_strip_multiplier_divides_exactly_over_its_whole_range():
    """id / nstrips == (id * (2^s / nstrips + 1)) >> s, s = MARCH_PLACE_SHIFT, for every id and strip count the partial slots allow, inside 32 bits (the bound
    iw_march.hpp states)"""
    shift = mc._const("iw_march.hpp", "MARCH_PLACE_SHIFT")
    ids = np.arange(mc.MAX_PARTIALS, dtype=np.uint64)
    for n in range(1, mc.MAX_PARTIALS + 1):
        magic = np.uint64((1 << shift) // n + 1)
        prod = ids * magic
        assert int(prod.max()) < 1 << 32
        assert np.array_equal(prod >> np.uint64(shift), ids // np.uint64(n)), n
