"""lfgpu_ligero_prove_batch256 and lfgpu_ligero_open_batch256: the low-degree, dot and quadratic proofs and the openings of B
provers from lfgpu_ligero_commit(FIELD_P256) through one chain of dispatches.

Everything is compared byte for byte, with two sources of expected values: the single-statement entry points on the same
provers in the same process (lfgpu_ligero_low_degree_proof, lfgpu_ligero_dot_proof on the dense A that the batch builds from
scale * dense + the sparse terms, lfgpu_ligero_quadratic_proof, lfgpu_ligero_open), and the Python model of
tests/ligero_p256_model.py on the CPU over the same tableaux (pinned against the reference's known-answer vector by
test_ligero_p256_model.py).

The shape (asserted below, so that a changed parameter search cannot thin the test): block 85 and dblock 169, no multiples of
the 64 columns of a workgroup; nwqrow 15 and 9: every one of the four row slices has work and one more row than another, and an
ODD row count, so the Reed-Solomon extension of a chain pairs the last A row of one statement with the first of the next; two
quadratic triples, and a second parameter set with none.

What this ABI cannot reach and the test therefore does not try: a sharded or slab prover and a prover without a commitment over
Fp256Base (lfgpu_ligero_prover_from_slab and the sharded commit refuse the field)."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of the chunking test
    sys.path.insert(0, ROOT)

import numpy as np
import pytest

import ligero_p256_model as lm

pytestmark = pytest.mark.gpu

ERR_ARG = 1
NW, NREQ, BE, B = 650, 12, 512, 5
NQS = (100, 0)


# ---------------------------------------------------------------- statements
def param(pkg, nq):
    p = pkg.ligero_param(pkg.FIELD_P256, NW, nq, 4, NREQ, BE)
    assert p.block % 64 != 0 and p.dblock % 64 != 0 and p.block > 64 and p.dblock > 128
    assert p.nwqrow >= 5 and p.nwqrow % 4 != 0 and p.nwqrow % 2 == 1
    assert (p.nqtriples >= 2) if nq else (p.nqtriples == 0)
    assert NW % p.w != 0
    return p


class Statements:
    """B committed device provers and the model over the same tableaux: random witnesses with nq quadratic constraints"""

    def __init__(self, G, nq, seed, gpu=None, nb=B):
        pkg = G.pkg
        self.G, self.gpu = G, gpu or G.gpu()
        self.p = p = param(pkg, nq)
        rng = np.random.default_rng(seed)
        self.lqc = []
        zs = rng.choice(np.arange(NW // 2, NW), size=nq, replace=False) if nq else []
        for i in range(nq):
            self.lqc.append((int(rng.integers(0, NW // 2)), int(rng.integers(0, NW // 2)), int(zs[i])))
        self.provers, self.models = [], []
        for b in range(nb):
            W = lm.rand_ints(rng, NW)
            for (x, y, z) in self.lqc:
                W[z] = lm.mul(W[x], W[y])
            Wa = lm.elts(W)

            def engine(b=b):
                eng = np.random.default_rng(seed + 1 + b)
                return lambda n: bytes(eng.integers(0, 256, size=n, dtype=np.uint8))

            T, nonces = lm.tableau(pkg, p, Wa, self.lqc, engine())
            self.models.append(lm.Model(p, T, nonces, self.lqc))
            pr = pkg.LigeroProver(self.gpu, pkg.FIELD_P256, p)
            assert pr.commit(Wa, 0, self.lqc, engine()) == self.models[-1].root(), b
            self.provers.append(pr)

    def close(self):
        for pr in self.provers:
            pr.close()


def sparse_lists(rng, p):
    """statement 0: no sparse term; statement 1: every flat position; the rest: random strictly increasing subsets of differing lengths"""
    nflat = p.nwqrow * p.w
    idxs, vals = [], []
    for b in range(B):
        if b == 0:
            i = np.zeros(0, dtype=np.uint64)
        elif b == 1:
            i = np.arange(nflat, dtype=np.uint64)
        else:
            i = np.unique(np.concatenate([rng.choice(nflat, size=40 + 97 * b, replace=False), [0, nflat - 1] if b == 2 else []])).astype(np.uint64)
        idxs.append(i)
        vals.append(lm.rand_ints(rng, len(i)))
    return idxs, vals


def prove_inputs(p, ndense, seed):
    rng = np.random.default_rng(seed)
    idxs, vals = sparse_lists(rng, p)
    return dict(u_ldt=[lm.rand_ints(rng, p.nwqrow) for _ in range(B)], u_quad=[lm.rand_ints(rng, p.nqtriples) for _ in range(B)],
                scales=lm.rand_ints(rng, B), dense=[lm.rand_ints(rng, max(1, ndense)) for _ in range(B)], ndense=ndense, idxs=idxs, vals=vals)


def matrix_of(p, inp, b):
    """inner_product_vector as the ZK path builds it: scale * dense over the first ndense flat positions, then the sparse terms"""
    A = [0] * (p.nwqrow * p.w)
    for t in range(inp["ndense"]):
        A[t] = lm.mul(inp["scales"][b], inp["dense"][b][t])
    for i, v in zip(inp["idxs"][b], inp["vals"][b]):
        A[int(i)] = (A[int(i)] + v) % lm.P
    return A


def batch_proofs(pkg, gpu, p, provers, inp, dense_ptrs):
    """dense_ptrs: one device address per statement"""
    y = pkg.LigeroProver.prove_batch256(
        gpu, provers, np.stack([lm.elts(u) for u in inp["u_ldt"]]), dense_ptrs if inp["ndense"] else None, inp["ndense"], lm.elts(inp["scales"]), inp["idxs"],
        [lm.elts(v) if len(v) else np.zeros((0, 4), dtype=np.uint64) for v in inp["vals"]],
        np.stack([lm.elts(u) for u in inp["u_quad"]]) if p.nqtriples else np.zeros((0, 4), dtype=np.uint64))
    return [tuple(a[b].tobytes() for a in y) for b in range(len(provers))]


def check_prove(st, ndense, seed):
    G, p = st.G, st.p
    inp = prove_inputs(p, ndense, seed)
    d_dense = [G.to_dev(lm.elts(inp["dense"][b])) for b in range(B)]  # device buffers of the test's own, one per statement
    got = batch_proofs(G.pkg, st.gpu, p, st.provers, inp, [t.data_ptr() for t in d_dense])
    names = ("y_ldt", "y_dot", "y_quad_0", "y_quad_2")
    for b, (pr, m) in enumerate(zip(st.provers, st.models)):
        A = matrix_of(p, inp, b)
        y0, y2 = pr.quadratic_proof(lm.elts(inp["u_quad"][b]) if p.nqtriples else np.zeros((0, 4), dtype=np.uint64))
        single = (pr.low_degree_proof(lm.elts(inp["u_ldt"][b])).tobytes(), pr.dot_proof(lm.elts(A)).tobytes(), y0.tobytes(), y2.tobytes())
        q0, q2 = m.quadratic(inp["u_quad"][b])
        model = tuple(lm.elts(y).tobytes() if len(y) else b"" for y in (m.low_degree(inp["u_ldt"][b]), m.dot(A), q0, q2))
        for name, g, s, w in zip(names, got[b], single, model):
            assert g == s, "%s of statement %d vs the single call (ndense %d)" % (name, b, ndense)
            assert g == w, "%s of statement %d vs the model (ndense %d)" % (name, b, ndense)
    assert len(set(got)) == B  # the statements differ
    return inp, d_dense, got


def open_sets(p, seed):
    """statement 0: the first and the last column; 1: a neighbour pair (2 j, 2 j + 1), twice; 2: nreq consecutive leaves; the rest
    random; every list in a shuffled order"""
    rng = np.random.default_rng(seed)
    n, k = p.block_ext, p.nreq
    out = []
    for b in range(B):
        if b == 2:
            s = list(range(n // 2, n // 2 + k))
        else:
            s = [0, n - 1] if b == 0 else [10, 11, n - 3, n - 2] if b == 1 else []
            rest = [int(x) for x in rng.permutation(n) if int(x) not in s]
            s = (s + rest)[:k]
        rng.shuffle(s)
        out.append([int(x) for x in s])
    return out


def check_open(st, seed):
    pkg, p = st.G.pkg, st.p
    sets = open_sets(p, seed)
    got = pkg.LigeroProver.open_batch256(st.gpu, st.provers, sets)
    for b, (pr, m) in enumerate(zip(st.provers, st.models)):
        req, nonces, path = pr.open(sets[b])
        assert got[b][0].tobytes() == req.tobytes(), "req %d" % b
        assert got[b][1].tobytes() == nonces.tobytes(), "nonces %d" % b
        assert got[b][2] == path, "path %d" % b
        mreq, mnon, mpath = m.open(sets[b])
        assert got[b][0].tobytes() == np.stack([lm.elts(r) for r in mreq]).tobytes(), "req %d vs the model" % b
        assert [bytes(x) for x in got[b][1]] == mnon and got[b][2] == mpath, "nonces / path %d vs the model" % b
    npath = [len(g[2]) for g in got]
    assert len(set(npath)) > 1, npath  # the path lengths differ between the statements and come back per statement
    # path_cap exact: the longest path fits; one short: refused before anything is written
    exact = pkg.LigeroProver.open_batch256(st.gpu, st.provers, sets, path_cap=max(npath))
    assert [g[2] for g in exact] == [g[2] for g in got]
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        pkg.LigeroProver.open_batch256(st.gpu, st.provers, sets, path_cap=max(npath) - 1)
    return sets


def check_shape(G, nq, seed):
    st = Statements(G, nq, seed)
    p = st.p
    for nd in (NW, 0, p.nwqrow * p.w):  # a dense block that ends inside a row, none, all of A
        check_prove(st, nd, seed + nd)
    check_open(st, seed)
    st.close()


@pytest.mark.parametrize("nq", NQS)
def test_batch_equals_single_calls_and_model(nq):
    import gpu_util as G
    check_shape(G, nq, 7000 + nq)


# ---------------------------------------------------------------- where the index list and the offset table land in the uploaded block
@pytest.fixture(scope="module")
def four_statements():
    import gpu_util as G
    st = Statements(G, NQS[0], 7800, nb=4)
    yield st
    st.close()


@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("nb", [3, 4])
def test_packed_lists_at_every_residue_of_the_sparse_total(four_statements, nb, r):
    """The chain's uploaded block holds u_ldt | u_quad | scale | val [tot] | idx [tot] (u64) | off [nb + 1] (u64) in 32-byte elements,
    so the index list ends, and the offset table begins, on an element boundary only where tot is a multiple of 4.  Sparse lists of
    lengths (0, 1, r[, 2]): tot = 1 .. 6 takes every residue, one statement has no term, and nb + 1 is even and odd.  No dense block;
    the one-term list sits on the last flat position.  y_dot against the single call on the same prover, byte for byte."""
    st = four_statements
    p, provers = st.p, st.provers[:nb]
    nflat = p.nwqrow * p.w
    lens = (0, 1, r, 2)[:nb]
    rng = np.random.default_rng(7810 + 10 * nb + r)
    inp = dict(u_ldt=[lm.rand_ints(rng, p.nwqrow) for _ in range(nb)], u_quad=[lm.rand_ints(rng, p.nqtriples) for _ in range(nb)], scales=lm.rand_ints(rng, nb),
               ndense=0, idxs=[np.array([nflat - 1], dtype=np.uint64) if b == 1 else np.arange(n, dtype=np.uint64) for b, n in enumerate(lens)],
               vals=[lm.rand_ints(rng, n) for n in lens])
    got = batch_proofs(st.G.pkg, st.gpu, p, provers, inp, None)
    for b, pr in enumerate(provers):
        assert got[b][1] == pr.dot_proof(lm.elts(matrix_of(p, inp, b))).tobytes(), "y_dot of statement %d (lengths %s)" % (b, lens)


# ---------------------------------------------------------------- chunking (the environment is read once per process)
def test_chunks_of_two_statements_give_the_same_bytes():
    env = {k: v for k, v in os.environ.items() if k != "LFGPU_LP_CHUNK"}
    env["LFGPU_LP_CHUNK"] = "2"
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-500:] + r.stderr[-2000:]


def _child():
    """B = 5: chains of 2, 2 and 1 statements against the single calls and the model"""
    import gpu_util as G
    check_shape(G, NQS[0], 7300)
    print("OK")


# ---------------------------------------------------------------- argument errors
def test_argument_errors_touch_nothing():
    import torch

    import gpu_util as G
    import ligero_fixture as lf16
    from test_commit_batch_gpu import _lqc, _witness
    pkg, gpu = G.pkg, G.gpu()
    st = Statements(G, NQS[0], 7500)
    p = st.p
    inp, d_dense, before = check_prove(st, NW, 7501)
    sets = open_sets(p, 7502)
    opened = pkg.LigeroProver.open_batch256(gpu, st.provers, sets)
    dd = [t.data_ptr() for t in d_dense]
    # provers that do not belong into this batch: another context, a 16-byte field, another lfgpu_ligero_param
    gpu2 = pkg.LfGpu(0)
    foreign = Statements(G, NQS[0], 7600, gpu=gpu2, nb=2)
    other_param = Statements(G, NQS[1], 7700, nb=2)
    p16 = pkg.ligero_param(pkg.FIELD_FP128, 40, 7, 4, 3, 64)
    lqc16 = _lqc(40, 7, 31)
    _, fp128 = pkg.LigeroProver.commit_batch(gpu, pkg.FIELD_FP128, p16, [_witness(pkg.FIELD_FP128, 40, lqc16, 1)], 0, lqc16, [lf16.LcgRng(9).bytes])
    null = pkg.LigeroProver(gpu, pkg.FIELD_P256, p)  # never committed: a NULL handle
    good = st.provers

    def prove(provers, inp=inp, dd=dd):
        return batch_proofs(pkg, gpu, p, provers, inp, dd)

    def refused(fn, what):
        try:
            fn()
        except pkg.LfGpuError as e:
            assert "lfgpu error 1:" in str(e), (what, str(e))  # LFGPU_ERR_ARG
        else:
            pytest.fail(what + ": the call was not refused")

    for what, bad in (("NULL entry", null), ("another context", foreign.provers[1]), ("a 16-byte field", fp128[0]), ("another lfgpu_ligero_param", other_param.provers[1]),
                      ("the same prover twice", good[0])):
        provers = [good[0], bad] + good[2:]
        refused(lambda: prove(provers), what)
        refused(lambda: pkg.LigeroProver.open_batch256(gpu, provers, sets), what)
    # nb out of 1 .. LFGPU_SC_BATCH_MAX (raw: the wrappers size their arrays by the list)
    L = gpu.L
    n = pkg.SC_BATCH_MAX + 1
    hs = (C.c_void_p * n)(*[good[0].h.value] * n)
    buf = np.zeros(n * (p.dblock + p.nrow * p.nreq + 64) * 32, dtype=np.uint8)
    vp = C.c_void_p(buf.ctypes.data)
    nsp, npath, idx = (C.c_size_t * n)(), (C.c_size_t * n)(), (C.c_size_t * (n * p.nreq))(*list(range(p.nreq)) * n)
    for nb in (0, n):
        assert L.lfgpu_ligero_prove_batch256(gpu.h, hs, nb, vp, None, 0, None, None, None, nsp, vp, vp, vp, vp, vp) == ERR_ARG, nb
        assert L.lfgpu_ligero_open_batch256(gpu.h, hs, nb, idx, vp, vp, vp, p.nreq * p.mc_pathlen + 1, npath) == ERR_ARG, nb
    assert not buf.any(), "a refused call wrote to an output buffer"
    # sparse lists: not strictly increasing (a repeated index, a descending pair), out of range
    i2 = inp["idxs"][2]
    for what, bad in (("repeated", np.concatenate([i2[:2], i2[1:]])), ("descending", i2[::-1].copy()),
                      ("out of range", np.concatenate([i2[:-1], [p.nwqrow * p.w]]).astype(np.uint64))):
        bad_inp = dict(inp, idxs=inp["idxs"][:2] + [bad] + inp["idxs"][3:], vals=inp["vals"][:2] + [lm.rand_ints(np.random.default_rng(1), len(bad))] + inp["vals"][3:])
        refused(lambda: prove(good, bad_inp), what)
    # opened indices: out of range, given twice within a statement
    for what, s in (("out of range", sets[1][:-1] + [p.block_ext]), ("given twice", sets[1][:-1] + [sets[1][0]])):
        refused(lambda: pkg.LigeroProver.open_batch256(gpu, good, [sets[0], s] + sets[2:]), what)
    # a dense block inside the scratch the call is about to use
    sc, nbytes = C.c_void_p(), C.c_size_t()
    gpu._ck(L.lfgpu_scratch_info(gpu.h, 2, C.byref(sc), C.byref(nbytes)))
    assert sc.value and nbytes.value >= NW * 32
    refused(lambda: prove(good, inp, [dd[0], sc.value + nbytes.value - NW * 32] + dd[2:]), "dense block in scratch")
    torch.cuda.synchronize()
    # the provers answer as before, and the batch works
    assert prove(good) == before
    again = pkg.LigeroProver.open_batch256(gpu, good, sets)
    for a, b in zip(again, opened):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    for pr in fp128:
        pr.close()
    for s in (st, foreign, other_param):
        s.close()
    gpu2.close()


if __name__ == "__main__":
    _child()
