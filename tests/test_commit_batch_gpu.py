"""lfgpu_column_commit_batch and lfgpu_ligero_commit_batch: the commits of B statements of one shape through one chain of
dispatches, byte for byte against the unchanged single-statement entry points in the same process.

Column commit: every root and the WHOLE Merkle heap of every statement against lfgpu_column_commit on that statement alone
and against a SHA-256 tree computed here with hashlib.  Ligero commit: roots, the complete tableau and an opening (columns,
nonces, Merkle path) against lfgpu_ligero_commit with the same RandomEngine seeds; statement 0 of the fixture shape carries
the fixture's seed, so its root is also the reference's own commitment."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import ligero_fixture as lf
import oracle_lib as ol
from oracle_lib import FP, GF, arr, elt

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ASSERT = 1, 5


def _d2h(gpu, ptr, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    gpu._ck(gpu.L.lfgpu_memcpy_d2h(gpu.h, C.c_void_p(out.ctypes.data), C.c_void_p(ptr), nbytes))
    return out


# ---------------------------------------------------------------- lfgpu_column_commit_batch
def _canon_bytes(pkg, field, col):
    """the 16-byte to_bytes_field images of a column (Fp128: out of Montgomery form)"""
    if field == GF:
        return np.ascontiguousarray(col).tobytes()
    rinv = pow(1 << 128, -1, pkg.FP128_P)
    return b"".join((((int(e[0]) | int(e[1]) << 64) * rinv) % pkg.FP128_P).to_bytes(16, "little") for e in col)


def _hashlib_heap(pkg, field, T, col0, ncols, nonces):
    heap = [b""] * (2 * ncols)
    for j in range(ncols):
        heap[ncols + j] = hashlib.sha256(nonces[j].tobytes() + _canon_bytes(pkg, field, T[:, col0 + j])).digest()
    for i in range(ncols - 1, 0, -1):
        heap[i] = hashlib.sha256(heap[2 * i] + heap[2 * i + 1]).digest()
    return heap


# 1: root = leaf; 2: one node; 3: odd; 1025: one node on level 10 of the top kernel; 2049: the first node that needs the level
# kernel; 2733: the reference vector's leaf count
@pytest.mark.parametrize("ncols", [1, 2, 3, 1025, 2049, 2733])
@pytest.mark.parametrize("nrow", [1, 5])
@pytest.mark.parametrize("field", [GF, FP])
def test_column_commit_batch_equals_single_and_hashlib(field, nrow, ncols):
    import torch

    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    B, col0 = 3, 5
    ld = col0 + ncols + 3
    rng = np.random.default_rng(1000 * ncols + 10 * nrow + field)
    Ts = [ol.rand_elts(rng, nrow * ld, field).reshape(nrow, ld, 2) for _ in range(B)]
    nonces = rng.integers(0, 256, size=(B, ncols, 32), dtype=np.uint8)
    dTs = [G.to_dev(T) for T in Ts]
    dN = G.to_dev(nonces)
    dLs = [torch.full((2 * ncols * 32,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(B)]
    roots = gpu.column_commit_batch(field, nrow, ld, col0, ncols, [t.data_ptr() for t in dTs], dN.data_ptr(), [t.data_ptr() for t in dLs])
    assert len(roots) == B and len(set(roots)) == B
    for b in range(B):
        heap = G.from_dev(dLs[b], np.uint8, (2 * ncols, 32))
        assert (heap[0] == 0x5A).all(), "slot 0 of heap %d was written" % b
        assert (G.from_dev(dTs[b], np.uint64, (nrow, ld, 2)) == Ts[b]).all(), "tableau %d was written" % b
        dL1 = torch.full((2 * ncols * 32,), 0x5A, dtype=torch.uint8, device="cuda")
        dN1 = G.to_dev(nonces[b])
        root1 = gpu.column_commit(field, nrow, ld, col0, ncols, dTs[b].data_ptr(), dN1.data_ptr(), dL1.data_ptr())
        assert roots[b] == root1, b
        assert (heap[1:] == G.from_dev(dL1, np.uint8, (2 * ncols, 32))[1:]).all(), "heap %d vs lfgpu_column_commit" % b
        want = _hashlib_heap(pkg, field, Ts[b], col0, ncols, nonces[b])
        assert roots[b] == want[1], b
        assert heap[1:].tobytes() == b"".join(want[1:]), "heap %d vs hashlib" % b


def test_column_commit_batch_argument_errors():
    import torch

    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ok = dict(field=GF, nrow=1, ld=8, col0=2, ncols=4, nb=2)
    for bad in (dict(nb=0), dict(nb=pkg.SC_BATCH_MAX + 1), dict(ncols=0), dict(col0=5), dict(field=99)):
        a = dict(ok)
        a.update(bad)
        with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
            gpu.column_commit_batch(a["field"], a["nrow"], a["ld"], a["col0"], a["ncols"], [d.data_ptr()] * a["nb"], d.data_ptr(), [d.data_ptr()] * a["nb"])
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 3:"):
        gpu.column_commit_batch(pkg.FIELD_P256, 1, 8, 2, 4, [d.data_ptr()] * 2, d.data_ptr(), [d.data_ptr()] * 2)
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        gpu.column_commit_batch(GF, 1, 8, 2, 4, [d.data_ptr(), None], d.data_ptr(), [d.data_ptr()] * 2)


# ---------------------------------------------------------------- lfgpu_ligero_commit_batch
def _lqc(nw, nq, seed):
    """nq triples (x, y, z): x, y in the first half of the witness, the z distinct in the second half"""
    rng = np.random.default_rng(seed)
    zs = rng.choice(np.arange(nw // 2, nw), size=nq, replace=False)
    return [(int(rng.integers(0, nw // 2)), int(rng.integers(0, nw // 2)), int(zs[i])) for i in range(nq)]


def _witness(field, nw, lqc, seed):
    """random, with W[z] = W[x] W[y] (the oracle's product) for every triple"""
    o = ol.oracle()
    W = ol.rand_elts(np.random.default_rng(seed), nw, field)
    for x, y, z in lqc:
        W[z] = arr(o.lfo_mul(field, elt(W[x]), elt(W[y])))
    return W


def _subfield_prefix(W, n, lqc, seed):
    """GF(2^128): W[:n] replaced by elements of the 16-bit subfield -- what a commit with subfield_boundary = n demands of its
    witness (LigeroProver::commit, ligero_prover.h:63-66) -- and the products of the triples recomputed"""
    from synth_fixture import GfSubfield
    o, sub = ol.oracle(), GfSubfield()
    W = W.copy()
    for i, u in enumerate(np.random.default_rng(seed).integers(1, 1 << 16, size=n)):
        e = sub.of_scalar(int(u))
        W[i] = (e & (2**64 - 1), e >> 64)
    for x, y, z in lqc:
        assert z >= n
        W[z] = arr(o.lfo_mul(GF, elt(W[x]), elt(W[y])))
    return W


def _open_idx(p):
    return sorted(int(i) for i in np.random.default_rng(p.block_ext).choice(p.block_ext, size=p.nreq, replace=False))


def _snapshot(gpu, pr, p):
    """(complete tableau, opened columns, nonces, Merkle path) of a committed prover"""
    T = _d2h(gpu, pr.tableau_ptr(), p.nrow * p.block_enc * 16).tobytes()
    req, nonces, path = pr.open(_open_idx(p))
    return T, req.tobytes(), nonces.tobytes(), path


def _single(gpu, pkg, field, p, W, sfb, lqc, rng_bytes):
    pr = pkg.LigeroProver(gpu, field, p)
    root = pr.commit(W, sfb, lqc, rng_bytes)
    snap = _snapshot(gpu, pr, p)
    pr.close()
    return root, snap


def _check(field, p, Ws, sfb, lqc, seeds, gpu=None):
    """the batch against per-statement lfgpu_ligero_commit with the same seeds -> the roots"""
    import gpu_util as G
    pkg = G.pkg
    gpu = gpu or G.gpu()
    B = len(Ws)
    want = [_single(gpu, pkg, field, p, Ws[b], sfb, lqc, lf.LcgRng(seeds[b]).bytes) for b in range(B)]
    roots, provers = pkg.LigeroProver.commit_batch(gpu, field, p, Ws, sfb, lqc, [lf.LcgRng(s).bytes for s in seeds])
    for b in range(B):
        assert roots[b] == want[b][0], "root %d" % b
        T, req, nonces, path = _snapshot(gpu, provers[b], p)
        assert T == want[b][1][0], "tableau %d" % b
        assert (req, nonces, path) == want[b][1][1:], "opening %d" % b
    for pr in provers:
        pr.close()
    return roots


def test_reference_fixture_statement_in_a_batch_of_three():
    """LigeroParam(1000, 50, 4, 36, 4096), LCG seed 100 in slot 0: its root is the reference's own commitment"""
    import gpu_util as G
    v = lf.load()
    p = G.pkg.ligero_param(GF, v["nw"], v["nq"], 4, v["nreq"], 4096)
    assert (p.block, p.dblock, p.nrow, p.block_ext) == (682, 1363, 8, 2733)
    roots = _check(GF, p, [v["W"]] * 3, v["subfield_boundary"], v["lqc"], [100, 101, 7919])
    assert roots[0] == v["root"]
    assert len(set(roots)) == 3


@pytest.mark.parametrize("nq", [7, 0])
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("field", [GF, FP])
def test_small_odd_shape(field, B, nq):
    """block 10, dblock 19, 45 leaves, 12 rows (9 without quadratic rows): rows shorter than a wave, an odd leaf count, a
    non-power-of-two block"""
    import gpu_util as G
    p = G.pkg.ligero_param(field, 40, nq, 4, 3, 64)
    assert (p.block, p.dblock, p.block_ext, p.nrow) == (10, 19, 45, 12 if nq else 9)
    lqc = _lqc(40, nq, 31)
    Ws = [_witness(field, 40, lqc, 500 + b) for b in range(B)]
    roots = _check(field, p, Ws, 0, lqc, [900 + 13 * b for b in range(B)])
    assert len(set(roots)) == B


def test_gf_rows_longer_than_the_lds_kernel_take_the_per_statement_encoder():
    """block 5461 > 2^12: the per-statement RS fallback inside the batched call; 21847 leaves: the batched level kernel runs on
    levels 13, 12 and 11"""
    import gpu_util as G
    p = G.pkg.ligero_param(GF, 100, 0, 4, 3, 32768)
    assert (p.block, p.nrow, p.block_ext) == (5461, 4, 21847)
    Ws = [_witness(GF, 100, [], 40 + b) for b in range(2)]
    _check(GF, p, Ws, 0, [], [11, 12])


def test_fp128_two_pass_fft_plan_inside_the_batched_convolution():
    import gpu_util as G
    p = G.pkg.ligero_param(FP, 3000, 0, 4, 3, 16384)
    assert (p.block, p.nrow) == (2730, 5)
    Ws = [_witness(FP, 3000, [], 60 + b) for b in range(2)]
    _check(FP, p, Ws, 0, [], [21, 22])


@pytest.mark.parametrize("field", [GF, FP])
def test_one_engine_shared_by_all_statements_draws_in_index_order(field):
    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    p = pkg.ligero_param(field, 40, 7, 4, 3, 64)
    lqc = _lqc(40, 7, 31)
    Ws = [_witness(field, 40, lqc, 700 + b) for b in range(3)]
    eng = lf.LcgRng(4242)
    want = [_single(gpu, pkg, field, p, Ws[b], 0, lqc, eng.bytes) for b in range(3)]
    eng = lf.LcgRng(4242)
    roots, provers = pkg.LigeroProver.commit_batch(gpu, field, p, Ws, 0, lqc, [eng.bytes] * 3)
    for b in range(3):
        assert roots[b] == want[b][0], b
        assert _snapshot(gpu, provers[b], p) == want[b][1], b
        provers[b].close()
    assert len(set(roots)) == 3


@pytest.mark.parametrize("field", [GF, FP])
def test_violated_quadratic_constraint_fails_the_whole_call(field):
    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    p = pkg.ligero_param(field, 40, 7, 4, 3, 64)
    lqc = _lqc(40, 7, 31)
    Ws = [_witness(field, 40, lqc, 800 + b) for b in range(3)]
    bad = Ws[1].copy()
    bad[lqc[3][2], 0] ^= np.uint64(1)
    n = 3
    def engine(seed):
        e = lf.LcgRng(seed)

        def cb(_user, buf, k):
            C.memmove(buf, e.bytes(k), k)
        return pkg.RNG_FN(cb)

    cbs = [engine(50 + b) for b in range(n)]
    lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
    hw = [Ws[0], bad, Ws[2]]
    roots = (C.c_uint8 * (32 * n))()
    out = (C.c_void_p * n)(1, 1, 1)
    rc = gpu.L.lfgpu_ligero_commit_batch(gpu.h, field, 4, C.byref(p), n, (C.c_void_p * n)(*[w.ctypes.data for w in hw]), 0, C.c_void_p(lq.ctypes.data),
                                         (pkg.RNG_FN * n)(*cbs), None, roots, out)
    assert rc == ERR_ASSERT and [out[b] for b in range(n)] == [None] * n
    # an lqc index out of range is an argument error of the whole call
    lq2 = lq.copy()
    lq2[3 * 5 + 1] = 40
    rc = gpu.L.lfgpu_ligero_commit_batch(gpu.h, field, 4, C.byref(p), n, (C.c_void_p * n)(*[w.ctypes.data for w in Ws]), 0, C.c_void_p(lq2.ctypes.data),
                                         (pkg.RNG_FN * n)(*cbs), None, roots, out)
    assert rc == ERR_ARG and [out[b] for b in range(n)] == [None] * n
    for nb in (0, pkg.SC_BATCH_MAX + 1):
        assert gpu.L.lfgpu_ligero_commit_batch(gpu.h, field, 4, C.byref(p), nb, (C.c_void_p * 65)(*([Ws[0].ctypes.data] * 65)), 0, C.c_void_p(lq.ctypes.data),
                                               (pkg.RNG_FN * 65)(*([cbs[0]] * 65)), None, (C.c_uint8 * (32 * 65))(), (C.c_void_p * 65)()) == ERR_ARG
    # a following good call on the same context gives the right roots
    _check(field, p, Ws, 0, lqc, [61, 62, 63])


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

        for field in (GF, FP):
            p = pkg.ligero_param(field, 40, 7, 4, 3, 64)
            lqc = _lqc(40, 7, 31)
            Ws = [_witness(field, 40, lqc, 300 + b) for b in range(2)]
            if field == GF:  # below the boundary of 17 (two subfield-only rows of w = 7 and a mixed one) the witness is subfield-valued
                Ws = [_subfield_prefix(W, 17, lqc, 310 + b) for b, W in enumerate(Ws)]
            want = [_single(gpu, pkg, field, p, W, 17, lqc, two) for W in Ws]
            roots, provers = pkg.LigeroProver.commit_batch(gpu, field, p, Ws, 17, lqc, [two, two])
            for b in range(2):
                assert roots[b] == want[b][0], (field, b)
                assert _snapshot(gpu, provers[b], p) == want[b][1], (field, b)
                provers[b].close()
    finally:
        gpu.close()
