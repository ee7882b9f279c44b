"""GPU: time the recomputing marching kernel's SLAB form (k_iter_march_rc<..., SLAB = 1>: a rank's row slab with one ghost row towards each neighbour, the exchanged
rows of A p in a plane -- what the all-gather transport launches) back to back, through thallo_hip_iw_pcg_iter.  THALLO_LIB selects the build, so two builds can be
compared launch for launch (profiles/march_head/README.md: the slab instantiations' 20-byte private segment).

    python tools/march_slab_time.py [W rows R reps]      one JSON line: microseconds per launch (HIP events around `reps` launches, best and median of 7 windows)"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thallo_amd
from thallo_amd import api, synthetic as syn

W, rows, R, reps = (int(x) for x in (sys.argv[1:5] + ["2048", "256", "0", "200"][len(sys.argv) - 1:]))
H = rows + 2                                         # the local image: the owned rows and a ghost row above and below
L = thallo_amd.lib()
p = syn.image_warping(W, H)
N = W * H
na = L.thallo_hip_vector_elems(3 * N)
dev = [torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x for x in p]
f = lambda: torch.zeros(na, dtype=torch.float32, device="cuda")
r0, pre, z, p0, delta, A0, r1, p1, A1 = [f() for _ in range(9)]
cs = torch.zeros(2 * N, dtype=torch.float32, device="cuda")
flags = torch.zeros(N + 256, dtype=torch.uint8, device="cuda")
parts = torch.zeros(4 * 1024, dtype=torch.float32, device="cuda")
s12 = torch.zeros(3 * 1024, dtype=torch.float64, device="cuda")
irregular = torch.zeros(16, dtype=torch.int32, device="cuda")
scal = torch.tensor([1.0, 2.0, 0.3], dtype=torch.float32, device="cuda")          # alphaN, alphaD, betaN of "iteration k-1": alpha 0.5, beta 0.3
vp, fl = C.c_void_p, C.c_float
assert L.thallo_hip_iw_pcg_init(W, H, 0, H, vp(dev[0].data_ptr()), vp(dev[1].data_ptr()), vp(dev[2].data_ptr()), vp(dev[3].data_ptr()), vp(dev[4].data_ptr()),
                                fl(p[5]), fl(p[6]), vp(r0.data_ptr()), vp(pre.data_ptr()), vp(z.data_ptr()), vp(p0.data_ptr()), vp(delta.data_ptr()),
                                vp(cs.data_ptr()), vp(flags.data_ptr()), None, vp(irregular.data_ptr()), vp(parts.data_ptr()), None) > 0
S = lambda i: api.SumT(scal.data_ptr() + 4 * i, 1)
L.thallo_hip_march_debug_set(0, R)
a = api.IwIterT(W=W, H=H, row0=1, row1=H - 1, cs=cs.data_ptr(), flags=flags.data_ptr(), irregular=irregular.data_ptr(), w_fit=float(p[5]), w_reg=float(p[6]),
                r_in=r0.data_ptr(), r_out=r1.data_ptr(), Ap_in=A0.data_ptr(), Ap_out=A1.data_ptr(), p_in=p0.data_ptr(), p_out=p1.data_ptr(), delta=delta.data_ptr(),
                mode=2, alphaN_prev=S(0), alphaD_prev=S(1), betaN_prev=S(2), alphaD_out=parts.data_ptr() + 4096, s12_out=s12.data_ptr())
launch = lambda: L.thallo_hip_iw_pcg_iter(api.IW_ITER_MARCH_RC, C.byref(a), None)
nb = launch()
assert nb > 0, nb
for _ in range(50):
    launch()
torch.cuda.synchronize()
t = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    t.append(e0.elapsed_time(e1) * 1000.0 / reps)
L.thallo_hip_march_debug_set(0, 0)
print(json.dumps({"W": W, "owned_rows": rows, "forced_R": R, "workgroups": nb, "reps": reps, "us_per_launch_min": round(min(t), 3), "us_per_launch_median": round(statistics.median(t), 3),
                  "windows": [round(x, 3) for x in t]}))
