"""What the synthetic-circuit suites of the two 16-byte fields share (test_zk_fp128_synth.py, test_zk_gf_synth.py): the
reader of the reference's LFC1 wire format, and GF2_128<4>'s 16-bit subfield on the host."""
import numpy as np


def read_lfc1_16(raw):
    """the reference's LFC1 wire format (lib/proto/circuit_writer.h:39-85) with 16-byte constants ->
    dict(fid, nv, nc, npub_in, subfield_boundary, ninputs, nl, nconst, layers=[{logw, nw, g, h0, h1, vi}])"""
    b = np.frombuffer(raw, dtype=np.uint8)
    assert b[0] == 1
    pos = 1

    def num():
        nonlocal pos
        v = int(b[pos]) | int(b[pos + 1]) << 8 | int(b[pos + 2]) << 16
        pos += 3
        return v

    fid, nv, nc, npub, sfb, nin, nl, nk = (num() for _ in range(8))
    pos += 16 * nk
    layers = []
    for _ in range(nl):
        logw, nw, nq = num(), num(), num()
        t = b[pos:pos + 12 * nq].reshape(nq, 4, 3).astype(np.int64)
        pos += 12 * nq
        v = t[:, :, 0] | (t[:, :, 1] << 8) | (t[:, :, 2] << 16)
        idx = np.cumsum((v[:, :3] >> 1) * (1 - 2 * (v[:, :3] & 1)), axis=0)  # deltas, LSB = sign
        layers.append(dict(logw=logw, nw=nw, g=idx[:, 0], h0=idx[:, 1], h1=idx[:, 2], vi=v[:, 3]))
    assert pos + 32 == len(b)
    return dict(fid=fid, nv=nv, nc=nc, npub_in=npub, subfield_boundary=sfb, ninputs=nin, nl=nl, nconst=nk, layers=layers)


def elt_int(row):
    """uint64[2] element image -> int"""
    return int(row[0]) | int(row[1]) << 64


class GfSubfield:
    """GF2_128<4>'s subfield GF(2^16) as a GF(2) vector space (lib/gf2k/gf2_128.h:112-116, 150-160, 201-204): the basis
    beta_i = g^i of the CPU oracle's context (pinned to the reference by test_oracle_golden.py), of_scalar and in_subfield
    by elimination on 128-bit integers"""

    def __init__(self):
        import oracle_lib as ol
        c = ol.gf_ctx(4)
        self.beta = [elt_int(ol.arr(c.beta[i])) for i in range(16)]
        self.ech = []  # (pivot bit, vector), a vector's pivot is clear in every later one
        for v in self.beta:
            for pb, r in self.ech:
                if v >> pb & 1:
                    v ^= r
            assert v
            self.ech.append((v.bit_length() - 1, v))

    def of_scalar(self, u):
        e = 0
        for i in range(16):
            if u >> i & 1:
                e ^= self.beta[i]
        return e

    def contains(self, e):
        for pb, r in self.ech:
            if e >> pb & 1:
                e ^= r
        return e == 0
