"""K13 (the copy rounds of the sumcheck over nc copies, csrc/sumcheck.hip evaluations_c_kernel) at a workload-like size:
one synthetic layer of nw = 2^14 wires in nc = 256 copies with nh ~ 10^5 HQUAD terms, both fields.  Reports the time of the
FIRST copy round's evaluations_c launch (lfgpu_sumcheck_evaluations_c: memset + kernel + read-back of the 12 accumulator
words) against its algorithmic bytes nh * 2 * nc * 16 B, the same launch with nc halved (the time should follow the copy
count), the row bind that follows it, and one whole lfgpu_sumcheck_layer_copies.  One JSON line per field.

usage: python tools/bench_sumcheck_copies.py [--nh 100000] [--logw 14] [--nc 256] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


def rand_elts(rng, n, field):
    a = rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
    if field == 6:
        a[:, 1] &= np.uint64(0x7FFFFFFFFFFFFFFF)  # below p = 2^128 - 2^108 + 1
    return a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)  # (the entry points return after their read-back)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nh", type=int, default=100000)
    ap.add_argument("--logw", type=int, default=14)
    ap.add_argument("--nc", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    pkg = load_package()
    gpu = pkg.LfGpu(0)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    nw, nc, nh = 1 << a.logw, a.nc, a.nh
    for field, name in ((pkg.FIELD_FP128, "fp128"), (pkg.FIELD_GF2_128, "gf2_128")):
        rng = np.random.default_rng(field)
        dW = dev(rand_elts(rng, nw * nc, field))
        dEQ = dev(rand_elts(rng, nc, field))
        dhc = dev(rng.integers(0, nw, size=(nh, 2), dtype=np.uint32))
        dvc = dev(rand_elts(rng, nh, field))
        dOut = torch.empty(nw * (nc // 2) * 16, dtype=torch.uint8, device="cuda")
        res = dict(field=name, nh=nh, nw=nw, nc=nc)
        for n0 in (nc, nc // 2):  # (the halved run reads the same buffer as [nw][nc / 2])
            med, best = timed(lambda: gpu.sumcheck_evaluations_c(field, nh, dhc.data_ptr(), dvc.data_ptr(), n0, nw, dW.data_ptr(), dEQ.data_ptr()),
                              a.reps)
            alg = nh * 2 * n0 * 16
            key = "evaluations_c" if n0 == nc else "evaluations_c_half_nc"
            res[key] = dict(n0=n0, median_ms=round(med * 1e3, 4), best_ms=round(best * 1e3, 4), algorithmic_bytes=alg,
                            gbytes_per_s=round(alg / med / 1e9, 1), hbm_fraction=round(alg / med / HBM_BYTES_PER_S, 4),
                            field_products_per_s=round(nh * (n0 // 2) * 7 / med / 1e9, 2))
        res["time_ratio_nc_over_half"] = round(res["evaluations_c"]["median_ms"] / res["evaluations_c_half_nc"]["median_ms"], 3)
        r = (3, 5)
        med, best = timed(lambda: (gpu.dense_bind_rows(field, nc, nw, r, dW.data_ptr(), dOut.data_ptr()), torch.cuda.synchronize()), a.reps)
        res["dense_bind_rows"] = dict(median_ms=round(med * 1e3, 4), bytes=nw * (nc + nc // 2) * 16,
                                      hbm_fraction=round(nw * (nc + nc // 2) * 16 / med / HBM_BYTES_PER_S, 4))
        # one whole layer: the nh terms as a quad over 2^10 outputs (hand pairs mostly distinct, so bind_g keeps ~nh terms)
        logv, logc = 10, max(1, (nc - 1).bit_length())
        h = rng.integers(0, nw, size=(nh, 2), dtype=np.uint32)
        h0, h1 = np.minimum(h[:, 0], h[:, 1]), np.maximum(h[:, 0], h[:, 1])
        g = rng.integers(0, 1 << logv, size=nh, dtype=np.uint32)

        def morton(x, y):
            m = np.zeros(len(x), dtype=np.uint64)
            for i in range(24):
                m |= ((x.astype(np.uint64) >> np.uint64(i)) & np.uint64(1)) << np.uint64(2 * i)
                m |= ((y.astype(np.uint64) >> np.uint64(i)) & np.uint64(1)) << np.uint64(2 * i + 1)
            return m

        key2 = np.stack([morton(h0, h1), g.astype(np.uint64)], axis=1)
        _, idx = np.unique(key2, axis=0, return_index=True)
        idx = idx[np.lexsort((g[idx], morton(h0[idx], h1[idx])))]
        kvec = rand_elts(rng, 9, field)
        q = pkg.Quad(gpu, field, g[idx], h0[idx], h1[idx], rng.integers(1, 9, size=len(idx), dtype=np.uint32), kvec, 1 << logv)
        Q, G0 = rand_elts(rng, logc, field), rand_elts(rng, logv, field)
        chal = [tuple(int(x) for x in e) for e in rand_elts(rng, logc + 2 * a.logw, field)]
        layer_ms = []
        for _ in range(3):
            dW2 = dW.clone()
            k = [0]

            def nxt(*_):
                k[0] += 1
                return chal[k[0] - 1]

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.sumcheck_layer_copies(logc, nc, Q, logv, G0, G0, (7, 0), (9, 0), a.logw, nw, dW2.data_ptr(), [(1, 0), (2, 0)], nxt, nxt)
            layer_ms.append((time.perf_counter() - t0) * 1e3)
        q.close()
        res["layer_copies_ms"] = [round(x, 3) for x in layer_ms]
        print(json.dumps(res))
    gpu.close()


if __name__ == "__main__":
    main()
