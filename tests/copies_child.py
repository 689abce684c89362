"""child process of tests/test_sumcheck_copies_gpu.py: the synthetic chain of copies_chain.py on the GPU under the
LFGPU_SC_MODE of the environment (read once per process); prints every value the prover handed out as one JSON line.
usage: copies_child.py <field id> <nc>[:<logc>] [<nc>[:<logc>] ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import copies_chain as cc  # noqa: E402
import gpu_util as G  # noqa: E402

field = int(sys.argv[1])
res = {}
for a in sys.argv[2:]:
    nc, logc = (int(x) for x in a.split(":")) if ":" in a else (int(a), None)
    res[a] = cc.run_gpu(cc.make_chain(field, nc, logc), G.pkg, G.gpu(), G.to_dev)
print("RESULT " + json.dumps(res))
