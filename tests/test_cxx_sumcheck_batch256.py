"""examples/sumcheck_layer_batch256.cc: the Fp256Base sumcheck layer from plain C++.  Its check mode runs B statements through
lfgpu_sumcheck_layer256 one after the other and through one lfgpu_sumcheck_layer_batch256, and exits non-zero unless every
evaluation, wc_out, g_out and bound_quad agree byte for byte and the wires are untouched."""
import json
import subprocess

import pytest

from test_sumcheck_batch256_abi import build_example

# (logv, logw, terms, nv, nw): `tiny` and `small` of tests/test_sumcheck_layer_batch256.py
SHAPES = {"tiny": (2, 3, 8, 3, 5), "small": (5, 6, 300, 0, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["tiny", "small"])
def test_cxx_batch_equals_sequential(shape):
    exe = build_example()
    out = subprocess.run([exe] + [str(x) for x in SHAPES[shape]] + ["3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["B"] == 3 and res["result"] == "identical"
    logv, logw, terms, nv, nw = SHAPES[shape]
    assert (res["logv"], res["logw"], res["nv"], res["nw"]) == (logv, logw, nv or 1 << logv, nw or 1 << logw)
    assert 0 < res["terms"] <= terms
