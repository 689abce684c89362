"""Child process of test_zk_prove_batch_ligero.py: LFGPU_LIGERO_PROVE_BATCH and LFGPU_LP_CHUNK are read once per process, so
every setting gets its own.  Runs check_batch of test_zk_prove_batch.py (every statement against lfgpu_zk_prove, the fixture's
wire SHA-256, the transcript's end state and zk_verify) and then prints one JSON line with the timings of a batch of the same
size: {"prove": [ms per member], "constraints": [...], "ligero_prove": [...]}.
Usage: zk_prove_batch_ligero_child.py <case> <B>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gpu_util as G
from test_zk_prove_batch import check_batch, commit_all, load

case, B = sys.argv[1], int(sys.argv[2])
check_batch(case, B)
raw, W, par = load(case)
gpu = G.gpu()
circ = G.pkg.Circuit(gpu, raw)
provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
batch = G.pkg.ZkBatch(gpu, circ, B)
tss, _ = commit_all(provers, [W] * B, par)
assert batch.prove(provers, [W] * B, tss) == [True] * B
t = [zk.timings() for zk in provers]
print(json.dumps({k: [x[k] for x in t] for k in ("prove", "constraints", "ligero_prove")}))
