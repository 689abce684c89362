"""verifier_constraints above LF_GH_BATCH_MAX (csrc/ctx.h: 96 layers).  Up to that many layers the 16-byte verifier enqueues
every layer's bind_gh_all sum and finalizes the constraints after one read-back; above it, it synchronises per layer.  The
deferred side is what every 16-byte fixture runs: the "nl" entries of tests/golden/*.json go up to 21 (mdoc.json).  The
per-layer branch of the shared build_constraints (csrc/zk_proto.h) is run here only: a synthetic Fp128 circuit of 97 layers,
proved and verified by the library."""
import numpy as np
import pytest

NL = 97  # LF_GH_BATCH_MAX + 1
NW = 6   # wires per layer (logw = 3; the narrow layers of the synth_fp128 "funnel" fixture have this shape)


def lfc1_chain():
    """LFC1 bytes (lib/proto/circuit_writer.h:39-114) of NL layers over Fp128: every layer copies its inputs, V[i] = W[0] * W[i]
    with W[0] = 1; the output layer has the two outputs W[0] * W[1] and W[1] * W[2], zero when W[1] = 0"""
    num = lambda v: int(v).to_bytes(3, "little")
    out = bytearray([1]) + b"".join(num(v) for v in (6, 2, 1, 1, 1, NW, NL, 1))  # fid, nv, nc, npub, sfb, ninputs, nl, nconst
    out += (1).to_bytes(16, "little")  # the constant 1

    def layer(terms):
        b, prev = bytearray(num(3) + num(NW) + num(len(terms))), (0, 0, 0)
        for t in terms:  # deltas with the sign in the LSB, then the constant's index
            for a, p in zip(t, prev):
                b += num(abs(a - p) << 1 | (a < p))
            b += num(0)
            prev = t
        return b
    out += layer([(0, 0, 1), (1, 1, 2)])
    for _ in range(NL - 1):
        out += layer([(i, 0, i) for i in range(NW)])
    return bytes(out + bytes(range(32)))


@pytest.mark.gpu
def test_verify_above_the_gh_batch_limit():
    import gpu_util as G
    import ligero_fixture as lf
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, lfc1_chain())
    assert (circ.info.field, circ.info.nl, circ.info.ninputs, circ.info.nv) == (G.pkg.FIELD_FP128, NL, NW, 2)
    one = (1 << 128) % (2**128 - 2**108 + 1)  # Montgomery image of 1
    vals = [one, 0] + [(one * k) % (2**128 - 2**108 + 1) for k in (5, 7, 11, 13)]
    W = np.array([[v & (2**64 - 1), v >> 64] for v in vals], dtype=np.uint64)
    rate, nreq = 4, 6
    zk = G.pkg.ZkProver(gpu, circ, rate, nreq)
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(3).bytes, ts)
    assert zk.prove(W, ts) is True
    wire = zk.wire()
    ts.close()

    def verify(proof):
        tv = G.pkg.FsTranscript(b"test")
        try:
            return G.pkg.zk_verify(gpu, circ, proof, W[:1], tv, rate, nreq)
        finally:
            tv.close()
    assert verify(wire) == (True, "ok")
    bad = bytearray(wire)
    bad[32 + 50 * (4 * 3 + 2) * 16 + 4 * 3 * 16] ^= 1  # the low byte of wc[0] of layer 50
    assert verify(bytes(bad))[0] is False
    zk.close()
    circ.close()
