"""Child process of test_zk_prove_batch256.py: LFGPU_LIGERO_PROVE_BATCH256 is read once per process, so every setting gets its
own.  Commits B provers of an Fp256Base case with the seeds of test_zk_prove_batch256.py, proves them with one
lfgpu_zk_prove_batch256 and prints one JSON line: {"switch": the setting, "sha256": [per statement], "constraints": [ms per
member], "ligero_prove": [...]}.  The parent compares the settings with each other and with the fixture.
Usage: zk_prove_batch256_child.py <case> <B>"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gpu_util as G
from test_zk_prove_batch256 import SWITCH, commit_all, load

case, B = sys.argv[1], int(sys.argv[2])
raw, W, par = load(case)
gpu = G.gpu()
circ = G.pkg.Circuit(gpu, raw)
provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
batch = G.pkg.ZkBatch256(gpu, circ, B)
tss, _ = commit_all(provers, [W] * B, par)
assert batch.prove(provers, [W] * B, tss) == [True] * B
t = [zk.timings() for zk in provers]
res = {"switch": os.environ.get(SWITCH, ""), "sha256": [hashlib.sha256(zk.wire()).hexdigest() for zk in provers]}
res.update({k: [x[k] for x in t] for k in ("constraints", "ligero_prove")})
print(json.dumps(res))
