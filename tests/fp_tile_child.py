"""Child process of test_fp128_tile_1024x4.py: LFGPU_FP_TILE1024 is read once per process, so the specialised and the generic
K1 tile kernels each get a process of their own.  Usage: fp_tile_child.py <cases.npz> <out.npz>; every case of the input
(rows x n elements, row stride ld, direction) is transformed in place and written back under the same key."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import gpu_util as G

cases = np.load(sys.argv[1])
out = {}
for key in cases.files:
    _, logn, rows, ld, forward = key.split("_")
    n, rows, ld = 1 << int(logn), int(rows), int(ld)
    d = G.to_dev(cases[key])
    G.gpu().fp128_fft(d.data_ptr(), rows, n, ld=ld, forward=forward == "f")
    out[key] = G.from_dev(d, np.uint64, cases[key].shape)
np.savez(sys.argv[2], **out)
