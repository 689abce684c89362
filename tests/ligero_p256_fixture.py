"""Parser for tests/golden/ligero_p256_vector.bin -- a Ligero known-answer vector over Fp256Base, written once by a scratch
program (not kept) around the reference's own classes:

  LigeroProver<Fp256Base, ReedSolomonFactory<Fp256Base, FFTExtConvolutionFactory<Fp256Base, Fp2<Fp256Base>>>> with the root of
  unity of order 2^31 in the quadratic extension (lib/circuits/mdoc/mdoc_zk.cc:82-88), LigeroVerifier of the same types accepting
  the proof, and ZkProof<Fp256Base>::write_com_proof (lib/zk/zk_proof.h:137-185) for the proof bytes.

Statement: the one of the reference's test_ligero_verifier_failures (lib/ligero/ligero_test.cc:160-203) --
LigeroParam(nw 300, nq 30, rateinv 4, nreq 18) (the searching constructor: block_enc 512, block 85, w 67, 11 rows, 343 leaves),
nl 7, lqc[i] = (3 i, 3 i + 1, 3 i + 2) with W[z] = W[x] W[y], one linear term per wire with c = w % nl, b = A W,
hash_of_llterm = de ad be ef 0..., transcript "test".  In the place of SecureRandomEngine and random() stands ONE engine, the
fixtures' LCG (ligero_fixture.LcgRng) with seed 100: it first yields W[0], k[0], W[1], k[1], ... (RandomEngine::elt: 32 bytes an
attempt, rejected when >= p), then the quadratic wires are overwritten, and the same engine goes on to serve commit.

Layout: that of ligero_test_vector.bin (ligero_fixture.py) with 32-byte elements (Montgomery images, 4 x u64 little-endian)."""
import os
import struct

import numpy as np

from ligero_fixture import GOLD, LcgRng

P256_P = 2**256 - 2**224 + 2**192 + 2**96 - 1
SEED = 100


def load():
    d = open(os.path.join(GOLD, "ligero_p256_vector.bin"), "rb").read()
    off = 0

    def u64():
        nonlocal off
        (v,) = struct.unpack_from("<Q", d, off)
        off += 8
        return v

    def elts(n):
        nonlocal off
        a = np.frombuffer(d, dtype=np.uint64, count=4 * n, offset=off).reshape(n, 4).copy()
        off += 32 * n
        return a

    v = {}
    v["nw"], v["nq"], v["nreq"], v["nl"], v["subfield_boundary"] = u64(), u64(), u64(), u64(), u64()
    v["W"] = elts(v["nw"])
    v["A"] = elts(v["nw"])
    v["lqc"] = [(u64(), u64(), u64()) for _ in range(v["nq"])]
    nll = u64()
    ll = []
    for _ in range(nll):
        c, w = u64(), u64()
        ll.append((c, w, elts(1)[0]))
    v["llterm"] = ll
    v["b"] = elts(v["nl"])
    v["hash_of_statement"] = d[off:off + 32]
    off += 32
    v["root"] = d[off:off + 32]
    off += 32
    plen = u64()
    v["proof"] = d[off:off + plen]
    off += plen
    assert off == len(d)
    return v


def commit_engine(v):
    """the LCG in the state in which the generator handed it to LigeroProver::commit: the draws of W and k replayed (and checked
    against the file where the quadratic constraints have not overwritten W)"""
    eng = LcgRng(SEED)
    z = {q[2] for q in v["lqc"]}
    for i in range(v["nw"]):
        for name in ("W", "A"):
            while True:
                x = int.from_bytes(eng.bytes(32), "little")
                if x < P256_P:
                    break
            m = (x << 256) % P256_P
            got = sum(int(v[name][i][j]) << (64 * j) for j in range(4))
            assert got == m or (name == "W" and i in z), (name, i)
    return eng
