"""The order of frees that include/lfgpu_zk.h permits: a prover and a batch may be freed AFTER their circuit (their scrubbing
destructors go by the byte sizes recorded at allocation, not by the circuit handle); the context outlives all three.

Once over Fp128 and once over Fp256Base on the synthetic `funnel` fixture of tests/golden: circuit, one prover, one batch of 2;
commit and prove singly; free the circuit FIRST, then the batch, then the prover, each free returning LFGPU_OK; a fresh circuit
and prover on the same context then emit the same wire bytes, which are the fixture's reference bytes.

This pins the permitted order and that the context is left in working order.  It cannot by itself show that no destructor reads
the freed circuit: that is a property of the driver layer's source (csrc/zk_driver.h: no destructor dereferences the handle)."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

LFGPU_OK = 0


def _prove_once(G, gpu, circ, W, par, with_batch):
    """-> (prover, batch or None, wire bytes); neither is closed"""
    import ligero_fixture as lf
    zk = G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"])
    batch = None
    if with_batch:
        batch = (G.pkg.ZkBatch256 if circ.info.field == G.pkg.FIELD_P256 else G.pkg.ZkBatch)(gpu, circ, 2)
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(par["rng_seed"]).bytes, ts)
    assert zk.prove(W, ts) is True
    ts.close()
    return zk, batch, zk.wire()


@pytest.mark.parametrize("width", ["fp128", "p256"])
def test_prover_and_batch_outlive_their_circuit(width):
    import gpu_util as G
    if width == "p256":
        from test_zk_prove_batch256 import load
    else:
        from test_zk_prove_batch import load
    raw, W, par = load("funnel")
    gpu = G.gpu()
    L = gpu.L
    circ = G.pkg.Circuit(gpu, raw)
    assert (circ.info.field == G.pkg.FIELD_P256) == (width == "p256")
    zk, batch, wire = _prove_once(G, gpu, circ, W, par, with_batch=True)
    assert hashlib.sha256(wire).hexdigest() == par["sha"], "the reference's proof bytes"
    # the circuit first, then the batch, then the prover (the mirror objects forget their handles: nothing is freed twice)
    free_batch = L.lfgpu_zk_batch256_free if width == "p256" else L.lfgpu_zk_batch_free
    for obj, free in ((circ, L.lfgpu_circuit_free), (batch, free_batch), (zk, L.lfgpu_zk_prover_free)):
        h, obj.h = obj.h, None
        assert free(h) == LFGPU_OK
    circ2 = G.pkg.Circuit(gpu, raw)
    zk2, _, wire2 = _prove_once(G, gpu, circ2, W, par, with_batch=False)
    assert wire2 == wire
    zk2.close()
    circ2.close()
