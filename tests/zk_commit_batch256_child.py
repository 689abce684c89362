"""Child process of test_zk_commit_batch256.py: LFGPU_COMMIT_BATCH256 and LFGPU_CB_CHUNK are read once per process, so every
setting gets its own.  Commits B statements of a case with ZkBatch256.commit, proves them with ZkBatch256.prove and prints one
JSON line {"roots": [hex], "wires": [sha256 hex], "after": [hex]}; the parent compares it with the single path's bytes.
Usage: zk_commit_batch256_child.py <case> <B>"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_util as G
import ligero_fixture as lf
from test_zk_prove_batch256 import load, seeds

case, B = sys.argv[1], int(sys.argv[2])
raw, W, par = load(case)
pkg, gpu = G.pkg, G.gpu()
circ = pkg.Circuit(gpu, raw)
provers = [pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
batch = pkg.ZkBatch256(gpu, circ, B)
for rep in range(2):  # twice: the second run reuses the pooled buffers and the pinned staging memory
    tss = [pkg.FsTranscript(seeds(par, b)[1]) for b in range(B)]
    roots = batch.commit(provers, [W] * B, [lf.LcgRng(seeds(par, b)[0]).bytes for b in range(B)], tss)
    assert batch.prove(provers, [W] * B, tss) == [True] * B, "prove failed"
    out = dict(roots=[r.hex() for r in roots], wires=[hashlib.sha256(zk.wire()).hexdigest() for zk in provers], after=[ts.bytes(32).hex() for ts in tss])
    for ts in tss:
        ts.close()
    if rep:
        assert out == first, "the second pass differs from the first"
    first = out
print(json.dumps(out))
