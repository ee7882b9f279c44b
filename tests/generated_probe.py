"""What the tests of the generated kernels share on the device side (test_gpu_generated_kernels.py, test_gpu_prelude_functions.py): padded vectors with a NaN canary,
one open probe of a generated plugin (thallo_hip_genprobe_*, csrc/dsl_plugin.cpp), the library's switches for the length of a case."""
import ctypes as C
import os

import numpy as np

import shim_kernels as sk

CANARY = {4: sk.CANARY, 8: 0x7FF8BEEF7FF8BEEF}          # per element size: a quiet NaN as a float / as a double


class Vec:
    """thallo_hip_vector_elems(n) + 256 elements of 4 or 8 bytes: payload (None: the canary everywhere), the canary behind it"""

    def __init__(self, torch, L, n, size, payload=None):
        self.n, self.elems, self.size = n, int(L.thallo_hip_vector_elems(n)), size
        self.dt = np.float32 if size == 4 else np.float64
        h = np.full(self.elems + 256, CANARY[size], np.uint32 if size == 4 else np.uint64).view(self.dt)
        if payload is not None:
            h[:self.elems] = 0; h[:n] = np.asarray(payload, self.dt)
        self.h0 = h.copy()
        self.t = torch.from_numpy(h).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy()

    def body(self):
        return self.host()[:self.n].astype(np.float64)

    def check(self, padding_zero=True, ones_to_ceil4=False):
        """the canary behind the vector is intact; the padding [n, elems) is 0 -- or untouched where padding_zero is False; ones_to_ceil4: M^-1 of the empty diagonal, 1,
        up to the next multiple of four (PCGInit1_Finish works on float4)"""
        h = self.host()
        assert h[self.elems:].tobytes() == self.h0[self.elems:].tobytes(), "the canary behind a vector changed"
        pad = h[self.n:self.elems]
        w = pad.view(np.uint32 if self.size == 4 else np.uint64)
        ok = w == 0
        if not padding_zero: ok |= w == CANARY[self.size]
        if ones_to_ceil4: ok[:sk.ceil4(self.n) - self.n] |= pad[:sk.ceil4(self.n) - self.n] == 1
        assert ok.all(), "the padding behind the last unknown is not 0"


class Handle:
    """one open probe: the plugin of (file, dims, autoschedule, precision) under the switches that were in force when it was opened"""

    def __init__(self, L, path, dims, auto, dbl):
        d = (C.c_uint * len(dims))(*dims)
        self.h = L.thallo_hip_genprobe_open(path.encode(), d, auto, int(dbl))
        import thallo_amd
        assert self.h, thallo_amd.last_error()
        self.L = L

    def kernels(self, what):
        """names of the generated kernels: 0 launched since open, 1 held by the plugin, 2 launched since the last call with 2"""
        return {n for n in self.L.thallo_hip_genprobe_kernels(self.h, what).decode().split(";") if n}

    def close(self):
        if self.h:
            self.L.thallo_hip_genprobe_close(self.h); self.h = None


class Switches:
    """THALLO_AB / THALLO_DENSE_JTJ_MAX for the length of one case: the library reads them when a plugin is made and when its instance lists are built"""

    def __init__(self, ab="", dense_max=None):
        self.want = {"THALLO_AB": ab or None, "THALLO_DENSE_JTJ_MAX": dense_max, "THALLO_FRONTEND": None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.want}
        for k, v in self.want.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
