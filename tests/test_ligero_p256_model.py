"""Ligero over Fp256Base without a device: the reference's known-answer vector (tests/ligero_p256_fixture.py) rebuilt from
lfgpu_ligero_layout_rows(P256) (host only), the oracle's Reed-Solomon extension and column commitment, and the Python model of
the prover (tests/ligero_p256_model.py).  This pins the model against the real reference before test_ligero_p256_gpu.py leans
on it."""
import pytest

import __graft_entry__ as ge
import ligero_p256_fixture as lf
import ligero_p256_model as lm
from fs_transcript import Transcript


@pytest.fixture(scope="module")
def rebuilt():
    pkg = ge.load_package()
    pkg.load_library()
    v = lf.load()
    p = pkg.ligero_param(pkg.FIELD_P256, v["nw"], v["nq"], 4, v["nreq"], 0)
    T, nonces = lm.tableau(pkg, p, v["W"], v["lqc"], lf.commit_engine(v).bytes)
    return dict(pkg=pkg, v=v, p=p, T=T, nonces=nonces)


def test_layout_param(rebuilt):
    p = rebuilt["p"]
    assert (p.block_enc, p.block, p.w, p.dblock, p.nrow, p.block_ext) == (512, 85, 67, 169, 11, 343)


def test_root_from_host_layout_and_oracle(rebuilt):
    r = rebuilt
    assert lm.root_of(r["p"], r["T"], r["nonces"]) == r["v"]["root"]
    assert lm.Model(r["p"], r["T"], r["nonces"], r["v"]["lqc"]).root() == r["v"]["root"]


def test_model_proof_bytes(rebuilt):
    r = rebuilt
    v = r["v"]
    m = lm.Model(r["p"], r["T"], r["nonces"], v["lqc"])
    ts = Transcript(b"test")
    ts.write_bytes(v["root"])
    terms = [(c, w, lm.a2i(k)) for (c, w, k) in v["llterm"]]
    got = m.prove(ts, v["nl"], terms, v["hash_of_statement"])
    assert len(got) == len(v["proof"]) == 20332
    assert got == v["proof"]
    # b = A W, as the generator computed it
    b = [0] * v["nl"]
    W = lm.ints(v["W"])
    for (c, w, k) in terms:
        b[c] = (b[c] + lm.mul(k, W[w])) % lm.P
    assert b == lm.ints(v["b"])
