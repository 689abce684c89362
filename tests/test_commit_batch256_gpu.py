"""lfgpu_column_commit_batch256 and lfgpu_ligero_commit_batch256: the commits of B statements of one shape over Fp256Base through
one chain of dispatches, byte for byte against the unchanged single-statement entry points in the same process.

Column commit: every root and the WHOLE Merkle heap of every statement against lfgpu_column_commit(field = P256) on that
statement alone, and for one shape against the oracle's P-256 column hash.  Ligero commit: roots, the complete tableau and an
opening (columns, nonces, Merkle path) against lfgpu_ligero_commit(P256) with the same witnesses and RandomEngine seeds, at the
tableau shapes of the `funnel` and `wide` fixtures of tests/golden/synth_p256.json."""
import numpy as np
import pytest

import ligero_fixture as lf
import ligero_p256_model as lm
import oracle_lib as ol
from oracle_lib import P
from test_commit_batch_gpu import _d2h, _lqc, _open_idx
from test_zk_p256_synth import records

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- lfgpu_column_commit_batch256
def _rand_tableau(rng, n):
    """n uniform canonical elements (values below p) as (n, 4) words"""
    return lm.elts(lm.rand_ints(rng, n))


# (1, 1): the root is the leaf; (3, 2): one node; (21, 173): funnel's, not a power of two; (2, 1025): one node on level 10 of the
# top kernel; (20, 3187): odd's, the level kernel on level 11
SHAPES = [(1, 1, 1), (1, 1, 3), (1, 1, 64), (3, 2, 1), (3, 2, 3), (3, 2, 64), (21, 173, 1), (21, 173, 3), (21, 173, 64), (2, 1025, 3), (20, 3187, 3)]


@pytest.mark.parametrize("nrow,ncols,B", SHAPES, ids=["%dx%d-B%d" % s for s in SHAPES])
def test_column_commit_batch256_equals_single(nrow, ncols, B):
    import torch

    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    col0 = 5
    ld = col0 + ncols + 3
    rng = np.random.default_rng(1000 * ncols + 10 * nrow + B)
    base = _rand_tableau(rng, nrow * ld).reshape(nrow, ld, 4)
    Ts = [np.ascontiguousarray(np.roll(base, b, axis=1)) for b in range(B)]  # statement b: the rows rotated by b columns (and nonces of its own)
    nonces = rng.integers(0, 256, size=(B, ncols, 32), dtype=np.uint8)
    dTs = [G.to_dev(T) for T in Ts]
    dN = G.to_dev(nonces)
    dLs = [torch.full((2 * ncols * 32,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(B)]
    roots = gpu.column_commit_batch256(nrow, ld, col0, ncols, [t.data_ptr() for t in dTs], dN.data_ptr(), [t.data_ptr() for t in dLs])
    assert len(roots) == B and len(set(roots)) == B
    for b in range(B):
        heap = G.from_dev(dLs[b], np.uint8, (2 * ncols, 32))
        assert (heap[0] == 0x5A).all(), "slot 0 of heap %d was written" % b
        assert (G.from_dev(dTs[b], np.uint64, (nrow, ld, 4)) == Ts[b]).all(), "tableau %d was written" % b
        dL1 = torch.full((2 * ncols * 32,), 0x5A, dtype=torch.uint8, device="cuda")
        dN1 = G.to_dev(nonces[b])
        root1 = gpu.column_commit(pkg.FIELD_P256, nrow, ld, col0, ncols, dTs[b].data_ptr(), dN1.data_ptr(), dL1.data_ptr())
        assert roots[b] == root1, b
        assert (heap[1:] == G.from_dev(dL1, np.uint8, (2 * ncols, 32))[1:]).all(), "heap %d vs lfgpu_column_commit" % b


def test_column_commit_batch256_equals_the_oracle():
    """funnel's shape against the oracle's column hash and tree, the way test_column_commit_p256 checks the single call"""
    import torch

    import gpu_util as G
    gpu = G.gpu()
    o = ol.oracle()
    nrow, ncols, B, col0 = 21, 173, 3, 5
    ld = col0 + ncols + 3
    rng = np.random.default_rng(77)
    Ts = [_rand_tableau(rng, nrow * ld).reshape(nrow, ld, 4) for _ in range(B)]
    nonces = rng.integers(0, 256, size=(B, ncols, 32), dtype=np.uint8)
    dTs = [G.to_dev(T) for T in Ts]
    dN = G.to_dev(nonces)
    dLs = [torch.zeros(2 * ncols * 32, dtype=torch.uint8, device="cuda") for _ in range(B)]
    roots = gpu.column_commit_batch256(nrow, ld, col0, ncols, [t.data_ptr() for t in dTs], dN.data_ptr(), [t.data_ptr() for t in dLs])
    for b in range(B):
        want_root = np.zeros(32, dtype=np.uint8)
        lay = np.zeros((2 * ncols, 32), dtype=np.uint8)
        o.lfo_column_commit32(nrow, ld, col0, ncols, P(Ts[b]), P(np.ascontiguousarray(nonces[b])), P(want_root), P(lay))
        assert roots[b] == want_root.tobytes(), b
        assert (G.from_dev(dLs[b], np.uint8, (2 * ncols, 32))[1:] == lay[1:]).all(), b


def test_column_commit_batch256_argument_errors():
    import torch

    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ok = dict(nrow=1, ld=8, col0=2, ncols=4, nb=2)
    for bad in (dict(nb=0), dict(nb=pkg.SC_BATCH_MAX + 1), dict(ncols=0), dict(col0=5)):
        a = dict(ok)
        a.update(bad)
        with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
            gpu.column_commit_batch256(a["nrow"], a["ld"], a["col0"], a["ncols"], [d.data_ptr()] * a["nb"], d.data_ptr(), [d.data_ptr()] * a["nb"])
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        gpu.column_commit_batch256(1, 8, 2, 4, [d.data_ptr(), None], d.data_ptr(), [d.data_ptr()] * 2)


# ---------------------------------------------------------------- lfgpu_ligero_commit_batch256
def _param(pkg, case):
    """the fixture's LigeroParam, rebuilt from its arguments and checked against its recorded layout"""
    lp = records()[case]["ligero_param"]
    p = pkg.ligero_param(pkg.FIELD_P256, lp["nw"], lp["nq"], lp["rateinv"], lp["nreq"], lp["block_enc"])
    assert (p.nrow, p.block, p.dblock, p.block_enc, p.block_ext) == (lp["nrow"], lp["block"], lp["dblock"], lp["block_enc"], lp["block_ext"])
    return p, lp["nw"], lp["nq"]


def _witness(nw, lqc, seed):
    """random, with W[z] = W[x] W[y] for every triple"""
    W = lm.rand_ints(np.random.default_rng(seed), nw)
    for x, y, z in lqc:
        W[z] = lm.mul(W[x], W[y])
    return lm.elts(W)


def _snapshot(gpu, pr, p):
    """(complete tableau, opened columns, nonces, Merkle path) of a committed prover"""
    T = _d2h(gpu, pr.tableau_ptr(), p.nrow * p.block_enc * 32).tobytes()
    req, nonces, path = pr.open(_open_idx(p))
    return T, req.tobytes(), nonces.tobytes(), path


def _single(gpu, pkg, p, W, lqc, rng_bytes):
    pr = pkg.LigeroProver(gpu, pkg.FIELD_P256, p)
    root = pr.commit(W, 0, lqc, rng_bytes)
    snap = _snapshot(gpu, pr, p)
    pr.close()
    return root, snap


def _check(p, Ws, lqc, seeds, gpu=None):
    """the batch against per-statement lfgpu_ligero_commit(P256) with the same seeds -> the roots"""
    import gpu_util as G
    pkg = G.pkg
    gpu = gpu or G.gpu()
    B = len(Ws)
    want = [_single(gpu, pkg, p, Ws[b], lqc, lf.LcgRng(seeds[b]).bytes) for b in range(B)]
    roots, provers = pkg.LigeroProver.commit_batch256(gpu, p, Ws, lqc, [lf.LcgRng(s).bytes for s in seeds])
    for b in range(B):
        assert roots[b] == want[b][0], "root %d" % b
        T, req, nonces, path = _snapshot(gpu, provers[b], p)
        assert T == want[b][1][0], "tableau %d" % b
        assert (req, nonces, path) == want[b][1][1:], "opening %d" % b
    for pr in provers:
        pr.close()
    return roots


@pytest.mark.parametrize("case", ["funnel", "wide"])
def test_ligero_commit_batch256_equals_single(case):
    import gpu_util as G
    p, nw, nq = _param(G.pkg, case)
    lqc = _lqc(nw, nq, 31)
    Ws = [_witness(nw, lqc, 500 + b) for b in range(3)]
    roots = _check(p, Ws, lqc, [900 + 13 * b for b in range(3)])
    assert len(set(roots)) == 3


def test_one_engine_shared_by_all_statements_draws_in_index_order():
    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    p, nw, nq = _param(pkg, "funnel")
    lqc = _lqc(nw, nq, 31)
    Ws = [_witness(nw, lqc, 700 + b) for b in range(3)]
    eng = lf.LcgRng(4242)
    want = [_single(gpu, pkg, p, Ws[b], lqc, eng.bytes) for b in range(3)]
    eng = lf.LcgRng(4242)
    roots, provers = pkg.LigeroProver.commit_batch256(gpu, p, Ws, lqc, [eng.bytes] * 3)
    for b in range(3):
        assert roots[b] == want[b][0], b
        assert _snapshot(gpu, provers[b], p) == want[b][1], b
        provers[b].close()
    assert len(set(roots)) == 3


def test_exact_rng_calls_with_an_engine_that_answers_every_call_alike():
    """lfgpu_set_rng_exact_calls(1) and the reference's TestRng ({2, 0, 0, ...} for EVERY call): the batch draws with the single
    path's call pattern"""
    import gpu_util as G
    pkg = G.pkg
    gpu = pkg.LfGpu(0)
    try:
        gpu.set_rng_exact_calls(True)

        def two(n):
            return b"\x02" + bytes(n - 1) if n else b""

        p, nw, nq = _param(pkg, "funnel")
        lqc = _lqc(nw, nq, 31)
        Ws = [_witness(nw, lqc, 300 + b) for b in range(2)]
        want = [_single(gpu, pkg, p, W, lqc, two) for W in Ws]
        roots, provers = pkg.LigeroProver.commit_batch256(gpu, p, Ws, lqc, [two, two])
        for b in range(2):
            assert roots[b] == want[b][0], b
            assert _snapshot(gpu, provers[b], p) == want[b][1], b
            provers[b].close()
    finally:
        gpu.close()
