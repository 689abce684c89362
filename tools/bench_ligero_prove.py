"""Wall time of lfgpu_ligero_prove / lfgpu_ligero_verify on the shape of tests/golden/ligero_test_vector.bin (GF2_128, nw 1000,
nq 50, 1000 terms, nl 15, block_enc 4096): median and range of 7 calls after one warm-up (profiles/ligero_prove/README.md)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
import ligero_fixture as lf  # noqa: E402


def main():
    pkg = ge.load_package()
    gpu = pkg.LfGpu(0)
    v = lf.load()
    p = pkg.ligero_param(pkg.FIELD_GF2_128, v["nw"], v["nq"], 4, v["nreq"], 4096)
    pr = pkg.LigeroProver(gpu, pkg.FIELD_GF2_128, p)
    root = pr.commit(v["W"], v["subfield_boundary"], v["lqc"], lf.LcgRng(100).bytes)
    ll = pkg.llterm_array([(c, w, k) for (c, w, k) in v["llterm"]])
    tp, tv = [], []
    for i in range(8):
        ts = pkg.FsTranscript(b"test")
        ts.write_bytes(root)
        t0 = time.perf_counter()
        proof = pr.prove(ts, v["nl"], ll, v["hash_of_statement"], v["lqc"])
        t1 = time.perf_counter()
        ts.close()
        ts = pkg.FsTranscript(b"test")
        ts.write_bytes(root)
        t2 = time.perf_counter()
        ok, why = pkg.ligero_verify(gpu, pkg.FIELD_GF2_128, p, root, proof, ts, v["nl"], ll, v["hash_of_statement"], v["b"], v["lqc"])
        t3 = time.perf_counter()
        ts.close()
        assert proof == v["proof"] and ok, why
        if i:
            tp.append((t1 - t0) * 1e3)
            tv.append((t3 - t2) * 1e3)
    for name, t in (("prove", sorted(tp)), ("verify", sorted(tv))):
        print("lfgpu_ligero_%s: median %.3f ms (min %.3f, max %.3f) over %d calls" % (name, t[len(t) // 2], t[0], t[-1], len(t)))
    pr.close()
    gpu.close()


if __name__ == "__main__":
    main()
