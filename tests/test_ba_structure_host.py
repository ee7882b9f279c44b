"""CPU: the host code every Schur plan of bundle adjustment rests on (thallo_amd/csrc/ba_structure.cpp: the incidence lists, the symbolic structure of the reduced camera
matrix, the greedy aggregates, the member lists, the byte count) against its Python restatements, entry by entry and with no tolerance, under AddressSanitizer + UBSan.
tools/ba_structure_check.cpp links that one file, reads an instance from stdin and prints every array by name.  The mirrors the device tests trust -- SchurLists,
SchurStructure, greedy_aggregates, member_lists -- are thereby the C++'s restatement by test, not by reading; any sanitizer report (an index past a list, a signed overflow,
a leak) fails the test."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from thallo_amd import synthetic as syn

from ba_schur_mirror import SchurLists, with_extras
from ba_schur_explicit_mirror import SchurStructure, hand_made
from ba_two_level_mirror import default_k, greedy_aggregates, member_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"5x72x330": ((5, 72, 330), 5), "3x160x480": ((3, 160, 480), 3), "24x300x1200": ((24, 300, 1200), 12), "72x500x2500": ((72, 500, 2500), 72)}
INSTANCES = [*SHAPES, "5x72x330+extras", "hand-made"]


@functools.lru_cache(maxsize=None)
def instance(name):
    """-> (oToC, oToP, C, P)"""
    if name == "hand-made": return hand_made()
    dims, band = SHAPES[name.split("+")[0]]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    if name.endswith("+extras"): p, dims = with_extras(p)
    return np.asarray(p[3]), np.asarray(p[4]), dims[0], dims[1]


@functools.lru_cache(maxsize=None)
def mirrors(name, renumber):
    oc, op, C, P = instance(name)
    L = SchurLists(oc, op, C, P, renumber)
    return L, SchurStructure(L)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("ba_structure") / "ba_structure_check")
    src = [os.path.join(ROOT, "tools", "ba_structure_check.cpp"), os.path.join(ROOT, "thallo_amd", "csrc", "ba_structure.cpp")]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *src, "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and ("sanitize" in cc.stderr or "asan" in cc.stderr or "ubsan" in cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + cc.stderr[-300:])
    assert cc.returncode == 0, cc.stderr[-2000:]
    return exe


def run(exe, oc, op, C, P, renumber, k, given):
    text = " ".join(map(str, [C, P, len(oc), int(renumber), k, *oc.tolist(), *op.tolist(), *given.tolist()]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=60)
    tail = (r.stdout[-500:] + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[1] == "=": out[f[0]] = int(f[2])
        else:
            assert int(f[1]) == len(f) - 2, f[0]
            out[f[0]] = np.array(f[2:], np.int64)
    return out


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("renumber", [False, True], ids=["callers-order", "renumbered"])
@pytest.mark.parametrize("name", INSTANCES)
def test_host_structure_is_the_mirrors(checker, name, renumber, k):
    oc, op, C, P = instance(name)
    L, st = mirrors(name, renumber)
    given = (np.arange(C) * 7 + 3) % min(C, 3)      # a caller's array: dense ids, not in camera order
    got = run(checker, oc, op, C, P, renumber, k, given)

    def same(key, want):
        want = np.asarray(want, np.int64).ravel()
        assert got[key].shape == want.shape and (got[key] == want).all(), (name, renumber, k, key)

    assert got["perm"] == int(renumber and P > 1)
    for key in ("cam_ptr", "cam_obs", "q_cam", "q_pt", "pt_ptr", "pt_pos"): same(key, getattr(L, key))
    same("new2old", L.new2old if renumber else [])
    assert (got["nterms"], got["nlower"], got["nblk"]) == (st.nterms, st.nlower, st.nblk)
    for key in ("row_ptr", "col", "lower", "term_ptr", "terms"): same(key, getattr(st, key))
    same("keys", st.row * C + st.colj)
    assert got["structure_bytes"] == st.bytes(len(oc))
    agg, mem_ptr, mem = greedy_aggregates(st, k)
    same("agg", agg); same("mem_ptr", mem_ptr); same("mem", mem)
    gp, gm = member_lists(given)
    same("given_agg", given); same("given_mem_ptr", gp); same("given_mem", gm)
    assert got["default_cameras_per_aggregate"] == default_k(C)
