"""A plain-Python model of what one launch of k_iter_march_rc (thallo_amd/csrc/energy_image_warping_march_rc.hip) executes.

The kernel's row loop is specialised by phase: a head, two "enter" and two "S1" steps, a steady loop of unclamped four-step trips and an unrolled, clamped
tail of up to DEPTH + 5 steps.  Which of these a wave runs is decided on the host (rows per segment R -> prefetch depth, segment bounds) and by a few lines
of integer arithmetic at the top of the kernel.  This module restates both, so that the tests can say which *classes* of the loop a list of shapes executes:

    class = (DEPTH, DMODE, the segment ends at the image's last row, steady trips K clipped at 3, tail steps T)

It restates march_rows_per_segment (device_common.hpp), march_pick_rows / make_march_geo / march_place's segment bounds (iw_march.hpp), the DEPTH rule of
launch_march_rc and t_first / t_last / t_lim / t_safe / K / T of the kernel.  tests/test_march_classes.py pins it to the library (thallo_hip_iw_march_rows) and
to the constants in the sources; tests/test_gpu_march_segments.py builds its parameter lists from it.  No GPU, no numpy."""
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thallo_amd", "csrc")


def _const(fname, name):
    """`constexpr int NAME = value;` / `#define NAME value` of a source file: the model follows the sources' constants instead of copying them"""
    txt = open(os.path.join(_CSRC, fname)).read()
    m = re.search(r"(?:constexpr\s+int\s+%s\s*=|#define\s+%s)\s*(\d+)" % (name, name), txt)
    assert m, (fname, name)
    return int(m.group(1))


MARCH_USE = _const("iw_march.hpp", "MARCH_USE")                  # output pixels per wave row
WAVES = _const("iw_march.hpp", "MARCH_NT") // 64                 # segments (waves) per workgroup
WG_PER_CU = _const("iw_march.hpp", "MARCH_WG_PER_CU")
MAX_PARTIALS = _const("device_common.hpp", "THALLO_MAX_PARTIALS")
DEEP_ROWS = _const("energy_image_warping_march_rc.hip", "MARCH_RC_DEEP_ROWS")
K_CLIP = 3                                                       # steady trips are told apart up to "three or more"


def depth(R):
    """rows of prefetch (launch_march_rc, RC_BY_DEPTH)"""
    return 4 if R >= DEEP_ROWS else 2


def rows_per_segment(rows, nstrips, cap, rmin=4):
    """march_rows_per_segment"""
    cap = min(cap, MAX_PARTIALS)
    cap -= cap % 8
    cap = max(cap, 8)
    for R in range(rmin, max(rows, rmin) + 1):
        nseg = (rows + R - 1) // R
        total = nstrips * ((nseg + WAVES - 1) // WAVES)
        if (total + 7) // 8 * 8 <= cap:
            return R
    return 0


def pick_rows(W, rows, cus, forced_rows=0, forced_cap=0):
    """march_pick_rows on a device of `cus` compute units; forced_rows / forced_cap: thallo_hip_march_debug_set(0, .) / (6, .)"""
    if forced_rows > 0:
        return forced_rows
    nstrips = (W + MARCH_USE - 1) // MARCH_USE
    if forced_cap > 0:
        return rows_per_segment(rows, nstrips, forced_cap)
    best_R, best_fill = 0, -1.0
    for m in range(WG_PER_CU, 5):
        R = rows_per_segment(rows, nstrips, cus * m)
        if R <= 0:
            break
        nseg = (rows + R - 1) // R
        total = nstrips * ((nseg + WAVES - 1) // WAVES)
        fill = total / float(((total + cus - 1) // cus) * cus)
        if best_R == 0 or fill > best_fill + 1e-9:
            best_R, best_fill = R, fill
        if fill >= (0.75 if m == WG_PER_CU else 0.9):
            break
    return best_R


def grid(W, row0, row1, R, deferred=False):
    """workgroups of the launch (make_march_geo + launch_march_rc); must stay <= MAX_PARTIALS"""
    nstrips = (W + MARCH_USE - 1) // MARCH_USE
    nseg = (row1 - row0 + R - 1) // R
    total = nstrips * ((nseg + WAVES - 1) // WAVES)
    return (total + 7) // 8 * 8 + (8 if deferred else 0)


def segments(row0, row1, R):
    """[ya, yb) of every wave that has rows (march_place; the same for every strip)"""
    return [(ya, min(ya + R, row1)) for ya in range(row0, row1, R)]


def phases(ya, yb, H, DEPTH, DMODE):
    """the kernel's phase arithmetic for one segment: rows taken t_first .. t_last, K steady trips of four unclamped steps, T clamped tail steps"""
    t_first, t_last = ya - 2, yb + 1
    t_lim = min(t_last, H - 1)
    if DMODE != 1 and yb < t_lim:
        t_lim = yb
    t_safe = t_lim - DEPTH
    t, K = ya + 2, 0
    while t + 3 <= t_safe:
        t += 4
        K += 1
    T = t_last - t + 1
    assert 0 <= T <= DEPTH + 5, (ya, yb, H, DEPTH, DMODE, T)      # the tail is unrolled DEPTH + 5 times: a longer one would drop rows
    assert 4 + 4 * K + T == (yb - ya) + 4                           # every row ya-2 .. yb+1 is taken exactly once
    return {"t_first": t_first, "t_last": t_last, "t_lim": t_lim, "t_safe": t_safe, "K": K, "T": T}


def segment_class(ya, yb, H, R, DMODE):
    ph = phases(ya, yb, H, depth(R), DMODE)
    return (depth(R), DMODE, yb == H, min(ph["K"], K_CLIP), ph["T"])


def launch_classes(W, H, row0, row1, R, DMODE):
    """the classes one launch executes (W does not enter: every strip runs the same segments)"""
    return {segment_class(ya, yb, H, R, DMODE) for ya, yb in segments(row0, row1, R)}


def delta_modes(planes, lit):
    """DMODE of the launches k = 1 .. lit-1 of a GN step (k = 0 is the stored-plane kernel) under THALLO_DELTA_PLANES=planes: 0 -> delta every iteration
    (DMODE 0); 1 -> every other one (THALLO_IW_STEP1_MODE: odd k none = DMODE 1, even k two terms = DMODE 2); a ring of >= 2 planes -> none in the loop"""
    if planes == 0:
        return {0} if lit > 1 else set()
    if planes == 1:
        return {1 if k & 1 else 2 for k in range(1, lit)}
    return {1} if lit > 1 else set()


def case_classes(W, H, R, planes, lit):
    out = set()
    for dm in delta_modes(planes, lit):
        out |= launch_classes(W, H, 0, H, R, dm)
    return out


def depth_n_pairs(shapes, cus=256):
    """(DEPTH, n) of every segment of whole-image launches at the automatic rows per segment"""
    out = set()
    for W, H in shapes:
        if W % 2 or W < 2:
            continue
        R = pick_rows(W, H, cus)
        if R > 0:
            out |= {(depth(R), yb - ya) for ya, yb in segments(0, H, R)}
    return out


def reachable_whole(n_max=40):
    """every class a WHOLE-image launch can execute with segments of up to n_max rows: the last segment (any length 1 .. R, ends at the image's last row) and
    the ones above it (always R rows; one or more rows of the image below them -- one row when the last segment is a single row)"""
    out = set()
    for R in range(1, n_max + 1):
        for dm in (0, 1, 2):
            for n in range(1, R + 1):
                out.add(segment_class(R, R + n, R + n, R, dm))          # last segment of H = R + n
            out.add(segment_class(0, R, R + 1, R, dm))                  # full segment, one row below
            out.add(segment_class(0, R, 2 * R, R, dm))                  # full segment, R rows below
            out.add(segment_class(0, R, R, R, dm))                      # the whole image in one segment
    return out


def reachable_slab_only(n_max=40):
    """classes only a row slab reaches: a SHORT segment that does not end at the (local) image's last row -- the last segment of a rank that has a ghost row below"""
    whole, out = reachable_whole(n_max), set()
    for R in range(1, n_max + 1):
        for dm in (0, 1, 2):
            for n in range(1, R + 1):
                out.add(segment_class(1, 1 + n, 2 + n, R, dm))
    return out - whole


# ---------------------------------------------------------------- the sweep of tests/test_gpu_march_segments.py
SWEEP_LIT = 5            # PCG iterations per GN step: launches k = 1 .. 4 run the kernel under test -- both parities of the every-other-iteration delta schedule, a wrapped ring of 3
SWEEP_WIDTHS = (124, 250, 2, 372, 64)           # one strip exactly / three strips, the last one 2 pixels / the narrowest image / three strips exactly / half a strip
SWEEP_PLANES = (0, 1, 3)                        # THALLO_DELTA_PLANES: DMODE 0 / DMODE 1 and 2 alternating / a ring of three p planes (DMODE 1)
DEEP_FULL_R = 24                                # the smallest R of the sweep that runs at depth 4


def sweep_heights():
    """(R, H): R = 1 .. DEEP_ROWS - 1 (depth 2) and R = 24, 25, 26, 27, 35, 40 (depth 4: every R mod 4, the benchmark's 35), each with a last segment of EVERY
    length (H = R + n, n = 1 .. R), the image in one segment (H = R), a one-row last segment under two full ones (2 R + 1) and three segments (3 R - 1); depth 4
    also with less than one segment (H < R: one short segment under the deep prefetch; 13 rows take the ninth tail step).  A case costs milliseconds."""
    out = []
    assert depth(DEEP_FULL_R) == 4 and depth(DEEP_ROWS - 1) == 2, "MARCH_RC_DEEP_ROWS moved: choose the swept R again"
    for R in list(range(1, DEEP_ROWS)) + [DEEP_FULL_R, 25, 26, 27, 35, 40]:
        hs = {R + n for n in range(1, R + 1)} | {R, 2 * R + 1, 3 * R - 1}
        if R >= DEEP_ROWS:
            hs |= {R - 1, 7, 13}
        out += [(R, H) for H in sorted(hs)]
    return out


def sweep_cases():
    """(W, H, R, planes) of the bit-for-bit sweep: every height of sweep_heights() under every delta schedule, the widths dealt round robin (so that every
    width meets every schedule and both depths).  A case whose forced grid would not fit the partial slots is a mistake in this list, not something to skip."""
    cases, i = [], 0
    for R, H in sweep_heights():
        for planes in SWEEP_PLANES:
            W = SWEEP_WIDTHS[i % len(SWEEP_WIDTHS)]
            i += 1
            assert grid(W, 0, H, R) <= MAX_PARTIALS, (W, H, R)
            cases.append((W, H, R, planes))                             # (3 schedules, 5 widths: every pairing comes round)
    return cases


def reference_cases():
    """the subset the float64 PCG is run on: greedily, cases of the sweep (at least half a strip wide) until every class has been executed once"""
    want, have, out = reachable_whole(), set(), []
    for case in sweep_cases():
        W, H, R, planes = case
        got = case_classes(W, H, R, planes, SWEEP_LIT)
        if W >= 64 and got - have:
            have |= got
            out.append(case)
    assert have == want, sorted(want - have)
    return out


# ---------------------------------------------------------------- row slabs at depth 4 (ranks sharing the one GPU)
# (world, W, rows per rank, R): short and full last segments on ranks with a ghost row below (interior) and on the bottom rank
SLAB_CASES = [
    (2, 128, (29, 48), 24),          # rank 0: 24 + 5 rows above a ghost row;   rank 1: two full segments down to the image's last row
    (2, 252, (48, 37), 24),          # rank 0: two full segments, ghost below;  rank 1: 24 + 13 (the ninth tail step on the bottom rank); two strips
    (3, 128, (25, 33, 50), 24),      # ranks 0, 1: last segments of 1 and 9 rows above a ghost row;  rank 2: 24 + 24 + 2
    (3, 64, (27, 54, 30), 27),       # R = 27: ranks 0, 1 one / two full segments above a ghost row;  rank 2: 27 + 3
    # ... and the other short last segments above a ghost row that give a (K, T) of their own (n = 1 .. 16 at R = 24; longer ones repeat a whole image's classes)
    (3, 64, (26, 34, 31), 24), (3, 128, (27, 35, 41), 24), (3, 64, (28, 36, 29), 24), (3, 128, (30, 37, 47), 24),
    (3, 64, (31, 38, 28), 24), (3, 128, (32, 39, 35), 24), (3, 64, (40, 24, 45), 24),
]


def slab_layout(counts, rank):
    """(local H, row0, row1) of a rank: its rows plus one ghost row towards each neighbour (thallo_amd.distributed.SlabLayout)"""
    top, bot = (1 if rank > 0 else 0), (1 if rank < len(counts) - 1 else 0)
    return counts[rank] + top + bot, top, top + counts[rank]


def slab_classes(counts, R, dmodes=(0, 1, 2)):
    """classes of a slab run's launches, for every delta mode (which of them a run executes is the transport's schedule)"""
    out = set()
    for rank in range(len(counts)):
        Hl, row0, row1 = slab_layout(counts, rank)
        for dm in dmodes:
            out |= launch_classes(0, Hl, row0, row1, R, dm)
    return out
