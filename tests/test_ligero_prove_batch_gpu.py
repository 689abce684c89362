"""lfgpu_ligero_prove_batch and lfgpu_ligero_open_batch: the low-degree, dot (sparse form) and quadratic proofs and the
openings of B committed provers of one LigeroParam through one chain of dispatches, byte for byte against the unchanged
single-statement entry points (lfgpu_ligero_low_degree_proof, _dot_proof_sparse, _quadratic_proof, _open) on the same provers
in the same process.  Those are pinned against the oracle by test_gpu_parity.py.

The shapes are the ones test_commit_batch_gpu.py asserts; the provers come from LigeroProver.commit_batch."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of the chunking test
    sys.path.insert(0, ROOT)

import numpy as np
import pytest

import ligero_fixture as lf
import oracle_lib as ol
from oracle_lib import FP, GF
from test_commit_batch_gpu import _lqc, _witness

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 1, 3
PAT = 0xA5


# ---------------------------------------------------------------- inputs
def commit(field, p, B, lqc, seed, Ws=None, gpu=None):
    import gpu_util as G
    gpu = gpu or G.gpu()
    Ws = Ws or [_witness(field, p.nw, lqc, seed + b) for b in range(B)]
    _, provers = G.pkg.LigeroProver.commit_batch(gpu, field, p, Ws, 0, lqc, [lf.LcgRng(seed + 100 + b).bytes for b in range(B)])
    return provers


def sparse_lists(rng, field, p, B):
    """statement 0: no sparse term; statement 1: flat indices 0 and nwqrow * w - 1 among others; every length differs"""
    nflat = p.nwqrow * p.w
    idxs, vals = [], []
    for b in range(B):
        if b == 0:
            i = np.zeros(0, dtype=np.uint64)
        else:
            n = min(nflat, 2 + (5 * b) % 23)
            i = rng.choice(nflat, size=n, replace=False)
            if b == 1:
                i = np.concatenate([i, [0, nflat - 1]])
            i = np.unique(i).astype(np.uint64)
        idxs.append(i)
        vals.append(ol.rand_elts(rng, len(i), field).reshape(-1, 2))
    return idxs, vals


def prove_inputs(field, p, B, ndense, seed):
    rng = np.random.default_rng(seed)
    u_ldt = ol.rand_elts(rng, B * p.nwqrow, field).reshape(B, p.nwqrow, 2)
    u_quad = ol.rand_elts(rng, B * max(1, p.nqtriples), field).reshape(B, -1, 2)[:, :p.nqtriples]
    scales = ol.rand_elts(rng, B, field).reshape(B, 2)
    dense = ol.rand_elts(rng, B * max(1, ndense), field).reshape(B, -1, 2)
    idxs, vals = sparse_lists(rng, field, p, B)
    return dict(u_ldt=u_ldt, u_quad=u_quad, scales=scales, dense=dense, ndense=ndense, idxs=idxs, vals=vals)


def open_sets(p, B, seed):
    """statement 0: leaves 0 and block_ext - 1; 1: two adjacent leaves; 2: nreq consecutive leaves of one subtree; the rest random;
    every list in a shuffled order"""
    rng = np.random.default_rng(seed)
    n, k = p.block_ext, p.nreq
    out = []
    for b in range(B):
        if b == 2:
            span = 1 << (k - 1).bit_length()
            first = (n // 2 // span) * span
            s = list(range(first, first + k))
        else:
            s = [0, n - 1] if b == 0 else [n // 2, n // 2 + 1] if b == 1 else []
            rest = [int(x) for x in rng.permutation(n) if int(x) not in s]
            s = (s + rest)[:k]
        rng.shuffle(s)
        out.append([int(x) for x in s])
    return out


# ---------------------------------------------------------------- batch against single
def single_proofs(provers, inp, d_dense):
    want = []
    for b, pr in enumerate(provers):
        y_ldt = pr.low_degree_proof(inp["u_ldt"][b])
        y_dot = pr.dot_proof_sparse(d_dense[b].data_ptr() if inp["ndense"] else None, inp["ndense"], inp["scales"][b], inp["idxs"][b], inp["vals"][b])
        y0, y2 = pr.quadratic_proof(inp["u_quad"][b])
        want.append((y_ldt.tobytes(), y_dot.tobytes(), y0.tobytes(), y2.tobytes()))
    return want


def batch_proofs(gpu, provers, inp, d_dense):
    import gpu_util as G
    y = G.pkg.LigeroProver.prove_batch(gpu, provers, inp["u_ldt"], [t.data_ptr() for t in d_dense] if inp["ndense"] else None, inp["ndense"], inp["scales"],
                                       inp["idxs"], inp["vals"], inp["u_quad"])
    return [tuple(a[b].tobytes() for a in y) for b in range(len(provers))]


def check_prove(gpu, field, p, provers, ndense, seed):
    import gpu_util as G
    inp = prove_inputs(field, p, len(provers), ndense, seed)
    d_dense = [G.to_dev(inp["dense"][b]) for b in range(len(provers))]  # device buffers of the test's own, one per statement
    want = single_proofs(provers, inp, d_dense)
    got = batch_proofs(gpu, provers, inp, d_dense)
    for b in range(len(provers)):
        for name, g, w in zip(("y_ldt", "y_dot", "y_quad_0", "y_quad_2"), got[b], want[b]):
            assert g == w, "%s of statement %d (ndense %d)" % (name, b, ndense)
    assert len(set(got)) == len(provers)  # the statements differ


def check_open(gpu, p, provers, seed):
    import gpu_util as G
    sets = open_sets(p, len(provers), seed)
    got = G.pkg.LigeroProver.open_batch(gpu, provers, sets)
    for b, pr in enumerate(provers):
        req, nonces, path = pr.open(sets[b])
        assert got[b][0].tobytes() == req.tobytes(), "req %d" % b
        assert got[b][1].tobytes() == nonces.tobytes(), "nonces %d" % b
        assert got[b][2] == path, "path %d" % b
    return [len(g[2]) for g in got]


def check_shape(field, p, B, lqc, seed, ndenses, gpu=None):
    import gpu_util as G
    gpu = gpu or G.gpu()
    provers = commit(field, p, B, lqc, seed, gpu=gpu)
    for nd in ndenses:
        check_prove(gpu, field, p, provers, nd, seed + nd)
    npath = check_open(gpu, p, provers, seed)
    for pr in provers:
        pr.close()
    return npath


@pytest.mark.parametrize("nq", [7, 0])
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("field", [GF, FP])
def test_small_odd_shape(field, B, nq):
    """block 10, dblock 19, 45 leaves, 12 rows (9 without quadratic rows): rows shorter than a wave, a non-power-of-two block, no
    quadratic triple; ndense 0, 40 (no multiple of w = 7) and nwqrow * w"""
    import gpu_util as G
    p = G.pkg.ligero_param(field, 40, nq, 4, 3, 64)
    assert (p.block, p.dblock, p.block_ext, p.nrow) == (10, 19, 45, 12 if nq else 9)
    assert 40 % p.w != 0 and 40 < p.nwqrow * p.w
    npath = check_shape(field, p, B, _lqc(40, nq, 31), 2000 + B, [0, 40, p.nwqrow * p.w])
    assert len(set(npath)) > 1, npath  # the path lengths differ between the statements and come back per statement


def test_reference_fixture_shape():
    """LigeroParam(1000, 50, 4, 36, 4096): block 682, dblock 1363 (22 column tiles of 64, the last one ragged), 2733 leaves"""
    import gpu_util as G
    v = lf.load()
    p = G.pkg.ligero_param(GF, v["nw"], v["nq"], 4, v["nreq"], 4096)
    assert (p.block, p.dblock, p.nrow, p.block_ext) == (682, 1363, 8, 2733)
    gpu = G.gpu()
    _, provers = G.pkg.LigeroProver.commit_batch(gpu, GF, p, [v["W"]] * 3, v["subfield_boundary"], v["lqc"], [lf.LcgRng(s).bytes for s in (100, 101, 7919)])
    check_prove(gpu, GF, p, provers, 1001, 77)
    npath = check_open(gpu, p, provers, 78)
    assert len(set(npath)) > 1, npath
    for pr in provers:
        pr.close()


def test_gf_rows_longer_than_the_lds_kernel_take_the_per_statement_encoder():
    """block 5461 > 2^12: the per-statement RS fallback inside the batched dot proof"""
    import gpu_util as G
    p = G.pkg.ligero_param(GF, 100, 0, 4, 3, 32768)
    assert (p.block, p.nrow, p.block_ext) == (5461, 4, 21847)
    check_shape(GF, p, 2, [], 3100, [101])


def test_fp128_two_pass_fft_plan_inside_the_batched_extension():
    import gpu_util as G
    p = G.pkg.ligero_param(FP, 3000, 0, 4, 3, 16384)
    assert (p.block, p.nrow) == (2730, 5)
    check_shape(FP, p, 2, [], 3200, [1501])


# ---------------------------------------------------------------- where the index list and the offset table land in the uploaded block
@pytest.fixture(scope="module")
def small_provers():
    """four provers of the 40-element shape per field, committed once for the module"""
    import gpu_util as G
    made = {}

    def get(field):
        if field not in made:
            p = G.pkg.ligero_param(field, 40, 7, 4, 3, 64)
            made[field] = p, commit(field, p, 4, _lqc(40, 7, 31), 6000 + field)
        return made[field]

    yield get
    for _, provers in made.values():
        for pr in provers:
            pr.close()


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("field", [GF, FP])
def test_packed_lists_at_every_residue_of_the_sparse_total(small_provers, field, B, r):
    """The chain's uploaded block holds u_ldt | u_quad | scale | val [tot] | idx [tot] (u64) | off [B + 1] (u64) in 16-byte elements,
    so the index list ends, and the offset table begins, on an element boundary only for an even tot.  Sparse lists of lengths
    (0, 1, r[, 2]): tot = 1 .. 4 takes both residues, one statement has no term, and B + 1 is even and odd.  No dense block; the
    one-term list sits on the last flat position.  y_dot against the single call on the same prover, byte for byte."""
    import gpu_util as G
    p, provers = small_provers(field)
    provers = provers[:B]
    nflat = p.nwqrow * p.w
    lens = (0, 1, r, 2)[:B]
    inp = prove_inputs(field, p, B, 0, 6100 + 10 * B + r)
    inp["idxs"] = [np.array([nflat - 1], dtype=np.uint64) if b == 1 else np.arange(n, dtype=np.uint64) for b, n in enumerate(lens)]
    inp["vals"] = [ol.rand_elts(np.random.default_rng(6200 + b), n, field).reshape(-1, 2) for b, n in enumerate(lens)]
    got = batch_proofs(G.gpu(), provers, inp, [])
    for b, pr in enumerate(provers):
        want = pr.dot_proof_sparse(None, 0, inp["scales"][b], inp["idxs"][b], inp["vals"][b])
        assert got[b][1] == want.tobytes(), "y_dot of statement %d (lengths %s)" % (b, lens)


# ---------------------------------------------------------------- chunking (the environment is read once per process)
@pytest.mark.parametrize("field", [GF, FP])
def test_chunks_of_two_statements_give_the_same_bytes(field):
    env = {k: v for k, v in os.environ.items() if k != "LFGPU_LP_CHUNK"}
    env["LFGPU_LP_CHUNK"] = "2"
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), str(field)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-500:] + r.stderr[-2000:]


def _child(field):
    """B = 5 on the 40-element shape: chains of 2, 2 and 1 statements against the single calls"""
    import gpu_util as G
    p = G.pkg.ligero_param(field, 40, 7, 4, 3, 64)
    check_shape(field, p, 5, _lqc(40, 7, 31), 4000, [0, 40, p.nwqrow * p.w])
    print("OK")


# ---------------------------------------------------------------- argument errors
def _handles(provers):
    return [pr.h.value if pr is not None else None for pr in provers]


class _Raw:
    """the two entry points through ctypes with output buffers of the test's own, filled with a pattern"""

    def __init__(self, gpu, p, n):
        self.gpu, self.p, self.n = gpu, p, n
        self.cap = p.nreq * p.mc_pathlen + 1
        sizes = dict(y_ldt=p.block * 16, y_dot=p.dblock * 16, y_q0=p.r * 16, y_q2=(p.dblock - p.block) * 16, req=p.nrow * p.nreq * 16, nonces=p.nreq * 32,
                     path=self.cap * 32, npath=8)
        self.out = {k: np.full(n * v, PAT, dtype=np.uint8) for k, v in sizes.items()}

    def untouched(self):
        return all((a == PAT).all() for a in self.out.values())

    def prove(self, handles, inp, d_dense, nb=None, idxs=None):
        n = len(handles)
        idxs = inp["idxs"] if idxs is None else idxs
        ix = [np.ascontiguousarray(i, dtype=np.uint64) for i in idxs]
        vl = [np.ascontiguousarray(v, dtype=np.uint64) for v in inp["vals"]]
        u, uq, sc = (np.ascontiguousarray(inp[k]) for k in ("u_ldt", "u_quad", "scales"))
        o = self.out
        return self.gpu.L.lfgpu_ligero_prove_batch(
            self.gpu.h, (C.c_void_p * n)(*handles), n if nb is None else nb, C.c_void_p(u.ctypes.data), (C.c_void_p * n)(*d_dense), inp["ndense"],
            C.c_void_p(sc.ctypes.data), (C.c_void_p * n)(*[i.ctypes.data if i.size else None for i in ix]),
            (C.c_void_p * n)(*[v.ctypes.data if v.size else None for v in vl]), (C.c_size_t * n)(*[len(i) for i in ix]), C.c_void_p(uq.ctypes.data),
            C.c_void_p(o["y_ldt"].ctypes.data), C.c_void_p(o["y_dot"].ctypes.data), C.c_void_p(o["y_q0"].ctypes.data), C.c_void_p(o["y_q2"].ctypes.data))

    def open(self, handles, sets, nb=None):
        n = len(handles)
        flat = [j for s in sets for j in s]
        o = self.out
        return self.gpu.L.lfgpu_ligero_open_batch(self.gpu.h, (C.c_void_p * n)(*handles), n if nb is None else nb, (C.c_size_t * len(flat))(*flat),
                                                  C.c_void_p(o["req"].ctypes.data), C.c_void_p(o["nonces"].ctypes.data), C.c_void_p(o["path"].ctypes.data),
                                                  self.cap, C.cast(C.c_void_p(o["npath"].ctypes.data), C.POINTER(C.c_size_t)))


def test_argument_errors_touch_nothing():
    import torch

    import gpu_util as G
    pkg, gpu = G.pkg, G.gpu()
    field, B = GF, 3
    p = pkg.ligero_param(field, 40, 7, 4, 3, 64)
    lqc = _lqc(40, 7, 31)
    provers = commit(field, p, B, lqc, 5000)
    inp = prove_inputs(field, p, B, 40, 5001)
    d_dense = [G.to_dev(inp["dense"][b]) for b in range(B)]
    dd = [t.data_ptr() for t in d_dense]
    sets = open_sets(p, B, 5002)
    before = single_proofs(provers, inp, d_dense), [pr.open(s) for pr, s in zip(provers, sets)]
    # provers that do not belong into this batch
    gpu2 = pkg.LfGpu(0)
    foreign = commit(field, p, 1, lqc, 5100, gpu=gpu2)[0]
    other_field = commit(FP, pkg.ligero_param(FP, 40, 7, 4, 3, 64), 1, lqc, 5200)[0]
    other_param = commit(field, pkg.ligero_param(field, 40, 7, 4, 4, 64), 1, lqc, 5300)[0]
    slab_h = C.c_void_p()
    gpu._ck(gpu.L.lfgpu_ligero_prover_from_slab(gpu.h, field, 4, C.byref(p), 1, p.nrow, C.c_void_p(provers[2].tableau_ptr() + p.block_enc * 16), None, None,
                                                 C.byref(slab_h)))
    raw = _Raw(gpu, p, pkg.SC_BATCH_MAX + 1)
    h = _handles(provers)
    bad_provers = [("NULL entry", [h[0], None, h[2]]), ("another context", [h[0], foreign.h.value, h[2]]), ("another field", [h[0], other_field.h.value, h[2]]),
                   ("another lfgpu_ligero_param", [h[0], other_param.h.value, h[2]]), ("the same prover twice", [h[0], h[1], h[0]])]
    for what, hs in bad_provers:
        assert raw.prove(hs, inp, dd) == ERR_ARG, what
        assert raw.open(hs, sets) == ERR_ARG, what
    for nb in (0, pkg.SC_BATCH_MAX + 1):
        big = [h[0]] * (pkg.SC_BATCH_MAX + 1)
        inp_big = prove_inputs(field, p, pkg.SC_BATCH_MAX + 1, 40, 5003)
        assert raw.prove(big, inp_big, [dd[0]] * len(big), nb=nb) == ERR_ARG, nb
        assert raw.open(big, open_sets(p, len(big), 5004), nb=nb) == ERR_ARG, nb
    # sparse lists: not strictly increasing (a repeated index, a descending pair), out of range
    i1 = inp["idxs"][1]
    for what, bad in (("repeated", np.concatenate([i1[:2], i1[1:]])), ("descending", i1[::-1].copy()),
                      ("out of range", np.concatenate([i1[:-1], [p.nwqrow * p.w]]).astype(np.uint64))):
        idxs = [inp["idxs"][0], bad, inp["idxs"][2]]
        vals = dict(inp, vals=[inp["vals"][0], ol.rand_elts(np.random.default_rng(1), len(bad), field).reshape(-1, 2), inp["vals"][2]])
        assert raw.prove(h, vals, dd, idxs=idxs) == ERR_ARG, what
    # opened indices: out of range, given twice within a statement
    for what, s in (("out of range", [0, 1, p.block_ext]), ("given twice", [7, 9, 7])):
        assert raw.open(h, [sets[0], s, sets[2]]) == ERR_ARG, what
    # a dense block inside the scratch the call is about to use
    sc, nbytes = C.c_void_p(), C.c_size_t()
    gpu._ck(gpu.L.lfgpu_scratch_info(gpu.h, 2, C.byref(sc), C.byref(nbytes)))
    assert sc.value and nbytes.value >= 40 * 16
    assert raw.prove(h, inp, [dd[0], sc.value + nbytes.value - 40 * 16, dd[2]]) == ERR_ARG
    # a slab prover is refused as unsupported
    assert raw.prove([h[0], slab_h.value, h[2]], inp, dd) == ERR_UNSUPPORTED
    assert raw.open([h[0], slab_h.value, h[2]], sets) == ERR_UNSUPPORTED
    assert raw.untouched(), "a refused call wrote to an output buffer"
    torch.cuda.synchronize()
    # the provers answer the single calls as before, and the batch works
    after = single_proofs(provers, inp, d_dense), [pr.open(s) for pr, s in zip(provers, sets)]
    assert after[0] == before[0]
    for a, b in zip(after[1], before[1]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert batch_proofs(gpu, provers, inp, d_dense) == before[0]
    gpu.L.lfgpu_ligero_free(slab_h)
    for pr in provers + [foreign, other_field, other_param]:
        pr.close()
    gpu2.close()


if __name__ == "__main__":
    _child(int(sys.argv[1]))
