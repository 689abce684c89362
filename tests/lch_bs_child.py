"""Child process of test_lch_bs_variants.py: LFGPU_LCH_BS, LFGPU_RS_TOWER and the LFGPU_BS_* switches of the bit-sliced
GF(2^128) path (csrc/lch_bs.hip, csrc/rs.hip) are read once per process, so every setting gets a process of its own on the
same inputs.  Usage: lch_bs_child.py <cases.npz> <out.npz> [prefix]; every case of the input (only the keys that start
with `prefix`, when given) is transformed in place and the whole buffer written back under the same key:
  fft_<k>_<l>_<coset>_<rows>_<f|i>   rows x ld elements through gf2128_lch14_fft (f: FFT, i: IFFT)
  rs_<k>_<n>_<m>_<nrow>              nrow x ld elements through gf2128_rs_encode_rows
The row stride ld is the second dimension of the array."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import gpu_util as G

cases = np.load(sys.argv[1])
prefix = sys.argv[3] if len(sys.argv) > 3 else ""
out = {}
for key in cases.files:
    if not key.startswith(prefix):
        continue
    a = cases[key]
    ld = a.shape[1]
    f = key.split("_")
    d = G.to_dev(a)
    if f[0] == "fft":
        k, l, coset, rows = (int(x) for x in f[1:5])
        G.gpu().gf2128_lch14_fft(d.data_ptr(), rows, l, coset=coset, ld=ld, inverse=f[5] == "i", subfield_log_bits=k)
    else:
        k, n, m, nrow = (int(x) for x in f[1:5])
        G.gpu().gf2128_rs_encode_rows(d.data_ptr(), nrow, n, m, ld=ld, subfield_log_bits=k)
    out[key] = G.from_dev(d, np.uint64, a.shape)
    del d
np.savez(sys.argv[2], **out)
print("OK", len(out))
