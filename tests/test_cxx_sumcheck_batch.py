"""examples/sumcheck_layer_batch.cc: lfgpu_sumcheck_layer_batch from plain C++.  Its check mode runs B statements through
lfgpu_sumcheck_layer one after the other and through one batched call, and exits non-zero unless every evaluation, wc_out,
g_out and bound_quad agree byte for byte."""
import json
import subprocess

import pytest

from test_sumcheck_batch_abi import build_example

# (logv, logw, terms, nv, nw): `tiny` and `cross` of tests/test_sumcheck_layer_batch.py
SHAPES = {"tiny": (2, 3, 8, 3, 5), "cross": (11, 15, 20000, 1025, (1 << 14) + 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["gf", "fp"])
@pytest.mark.parametrize("shape", ["tiny", "cross"])
def test_cxx_batch_equals_sequential(field, shape):
    exe = build_example()
    out = subprocess.run([exe, field] + [str(x) for x in SHAPES[shape]] + ["3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["B"] == 3 and res["batch_equals_sequential"] is True
    assert (res["logv"], res["logw"], res["nv"], res["nw"]) == SHAPES[shape][:2] + SHAPES[shape][3:]
    assert 0 < res["terms"] <= SHAPES[shape][2]
