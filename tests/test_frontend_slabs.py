"""Row slabs of generated energies, host side: which `.t` files have a row-slab form, how many ghost rows their stencil needs
(ThalloX_FrontendSlabGhostRows), and the front-end's row-slab translation unit (ThalloX_FrontendTextDims, what = 2) -- it compiles for gfx950 and
leaves the plan's own unit (what = 1) alone."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGIES = os.path.join(ROOT, "thallo_amd", "energies")
TESTS_E = os.path.join(ROOT, "tests", "energies")


def _lib():
    from thallo_amd import api
    L = api.lib()
    L.ThalloX_FrontendSlabGhostRows.argtypes = [C.c_char_p, C.c_void_p]
    L.ThalloX_FrontendSlabGhostRows.restype = C.c_int
    L.ThalloX_FrontendTextDims.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    L.ThalloX_FrontendTextDims.restype = C.c_int
    return L


def _ghost(path, dims):
    from thallo_amd import api
    L = _lib()
    d = (C.c_uint * len(dims))(*dims)
    g = L.ThalloX_FrontendSlabGhostRows(str(path).encode(), d)
    return g, (api.last_error() if g < 0 else "")


def _text(path, what, dims):
    from thallo_amd import api
    L = _lib()
    d = (C.c_uint * len(dims))(*dims)
    buf = C.create_string_buffer(1 << 23)
    n = L.ThalloX_FrontendTextDims(str(path).encode(), what, d, buf, len(buf))
    assert 0 <= n < len(buf), api.last_error()
    return buf.value.decode()


ELIGIBLE = [(os.path.join(ENERGIES, "laplacian_image.t"), [64, 48], 1),
            (os.path.join(TESTS_E, "gradient_paste.t"), [64, 48], 1),
            (os.path.join(ENERGIES, "shape_from_shading.t"), [64, 48], 2),
            (os.path.join(TESTS_E, "conv2d_wide.t"), [64, 48, 11, 11], 10)]


@pytest.mark.parametrize("path,dims,g", ELIGIBLE, ids=lambda v: os.path.basename(v) if isinstance(v, str) else None)
def test_ghost_rows_of_eligible_energies(path, dims, g):
    """g = the largest row span of one residual's data accesses; shape_from_shading: B_I reads X rows {-1, 0}, shading_v reads B_I at {0, +1} -> 2 (the
    hand-written plugin's radius); the 11 x 11 deconvolution: 10"""
    assert _ghost(path, dims) == (g, "")


def test_ghost_rows_of_a_central_second_difference_in_y(tmp_path):
    f = tmp_path / "d2y.t"
    f.write_text('W, H = Dims("W", "H")\nInputs { X = Unknown(float, {W, H}, 0), A = Array(float, {W, H}, 1) }\nx, y = W(), H()\n'
                 'r = Residuals { fit = X(x, y) - A(x, y), d2 = Select(InBounds(x, y - 1) * InBounds(x, y + 1), X(x, y - 1) - 2 * X(x, y) + X(x, y + 1), 0) }\n')
    assert _ghost(f, [32, 16]) == (2, "")


@pytest.mark.parametrize("path,dims,construct", [
    (os.path.join(ENERGIES, "image_warping.t"), [64, 48], "more than one Unknown"),
    (os.path.join(TESTS_E, "flow_sample.t"), [64, 48], "SampledImage"),
    (os.path.join(TESTS_E, "graph2d.t"), [64, 48], "Sparse"),
    (os.path.join(TESTS_E, "row_gain.t"), [64, 48], "1-D domain"),
    (os.path.join(TESTS_E, "volume_arap.t"), [8, 8, 8], "more than one Unknown"),
    (os.path.join(ENERGIES, "laplacian_graph.t"), [64, 64], "Sparse"),
], ids=lambda v: os.path.basename(v) if isinstance(v, str) and v.endswith(".t") else None)
def test_files_without_a_row_slab_form_say_why(path, dims, construct):
    g, why = _ghost(path, dims)
    assert g == -1 and "no row-slab form" in why and construct in why, why
    assert _lib().ThalloX_FrontendTextDims(path.encode(), 2, (C.c_uint * len(dims))(*dims), C.create_string_buffer(16), 16) == -1


def test_a_three_d_unknown_and_a_materialize_line_are_refused(tmp_path):
    f = tmp_path / "vol.t"
    f.write_text('W, H, D = Dims("W", "H", "D")\nInputs { X = Unknown(float, {W, H, D}, 0), A = Array(float, {W, H, D}, 1) }\nx, y, z = W(), H(), D()\n'
                 'r = Residuals { fit = X(x, y, z) - A(x, y, z) }\n')
    g, why = _ghost(f, [8, 8, 8])
    assert g == -1 and "3-D" in why, why
    m = tmp_path / "mat.t"
    m.write_text('W, H = Dims("W", "H")\nInputs { X = Unknown(float, {W, H}, 0), A = Array(float, {W, H}, 1) }\nx, y = W(), H()\n'
                 'r = Residuals { fit = X(x, y) - A(x, y) }\nr.fit.J:set_materialize(true)\n')
    g, why = _ghost(m, [8, 8])
    assert g == -1 and "materialize" in why, why


@pytest.mark.parametrize("path,dims,g", ELIGIBLE, ids=lambda v: os.path.basename(v) if isinstance(v, str) else None)
def test_the_slab_unit_is_a_second_unit(path, dims, g):
    """what = 2 is the row-slab unit: owned-row loops and the four slab words behind the dimensions; what = 1 does not change with it"""
    one, two = _text(path, 1, dims), _text(path, 2, dims)
    assert one != two
    assert f"#define NDIM {len(dims) + 4}" in two and f"#define NDIM {len(dims)}\n" in one
    assert "jtjgrp_0" in two or "jtj_s0" in two


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
@pytest.mark.parametrize("path,dims,g", ELIGIBLE, ids=lambda v: os.path.basename(v) if isinstance(v, str) else None)
def test_slab_units_compile_for_gfx950(tmp_path, path, dims, g):
    """the what = 2 unit of every eligible energy compiles for gfx950 (as test_generated_kernels_compile_for_gfx950 does for what = 1)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / (os.path.basename(path) + ".slab.hip")
    src.write_text(_text(path, 2, dims))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-munsafe-fp-atomics", "-c", str(src), "-o", str(tmp_path / "k.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_python_slab_ghost_rows():
    from thallo_amd import api
    assert api.slab_ghost_rows(os.path.join(ENERGIES, "shape_from_shading.t"), [64, 48]) == 2
    with pytest.raises(ValueError, match="more than one Unknown"):
        api.slab_ghost_rows(os.path.join(ENERGIES, "image_warping.t"), [64, 48])
