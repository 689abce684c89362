"""The device instructions of the Fp128, F64 and GF(2^128) arithmetic (csrc/fields.h, the __HIP_DEVICE_COMPILE__ path) on every carry
path, every row compared.  The host compilation of that header is different code, and uniform operands reach the rare links of the
chains with probability about 2^-32 each; tests/golden/fields_carry_pairs.json is a set of operand pairs that reaches every reachable
link of fp_add, fp_sub, fp_mul, f64_add, f64_sub and f64_mul at least four times and notices the loss of any one of them
(tests/fields_limb_model.py, tests/test_fields_limb_model.py).  Here those pairs, the squared edge lists, structured-limb and uniform
rows go through

  tests/fields_arith_check.hip, a stand-alone program around fields.h          against Python integers, all rows, all 13 outputs,
  the same program compiled with -DLF_FP_REDC2 (fp_mul's two-step REDC)          Fp128 products of the same records,
  field_binop(FIELD_FP128 | FIELD_GF2_128, add | sub | mul)                      against Python integers, all rows,
  f64_2_fft of n = 2 and n = 4, both directions, on rows of F64 carry pairs      against the oracle's lfo_f64_2_fftb / fftf,

the last two because the same inline assembly sits there under the library's own register allocation.  Bit-exact."""
import os
import subprocess

import numpy as np
import pytest

import fields_limb_model as L
import oracle_lib as ol
from oracle_lib import FP, GF, P, elt
from test_fields_limb_model import f64x2_mul_exact, f64x2_records
from test_fp_tile_arith import ROOT, _hipcc

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "tests", "fields_arith_check.hip")
NOUT = 13
N = 1 << 17  # rows per field
SPECIAL = np.array(L.SPECIAL, dtype=np.uint32)
(FP_ADD, FP_SUB, FP_MUL, FP_FROM_MONT, FP_REDUCE, F64_ADD, F64_SUB, F64_MUL, X2_ADD, X2_SUB, X2_MUL, X2_MUL_REAL, GF_MUL) = range(NOUT)


# ---- records: (n, 4) uint64 = (a.lo, a.hi, b.lo, b.hi)
def _rows(pairs, bits):
    """[(a, b)] of `bits`-bit integers -> uint64[n, 2 * bits / 64]"""
    nb = bits // 8
    return np.frombuffer(b"".join(a.to_bytes(nb, "little") + b.to_bytes(nb, "little") for a, b in pairs), dtype=np.uint64).reshape(len(pairs), -1).copy()


def _ints(a):
    """uint64[n, 2] -> Python integers"""
    return [l | (h << 64) for l, h in zip(a[:, 0].tolist(), a[:, 1].tolist())]


def _every_lane(rows):
    """an odd number of rows, 64 times over: every lane position 0..63 of a wave meets every row"""
    if len(rows) % 2 == 0:
        rows = np.concatenate([rows, rows[:1]])
    return np.tile(rows, (64, 1))


def _limbs(rng, n, nl, structured):
    w = rng.integers(0, 2**32, size=(n, nl), dtype=np.uint32)
    if structured:
        w = np.where(rng.random((n, nl)) < 0.85, SPECIAL[rng.integers(0, len(SPECIAL), size=(n, nl))], w)
    return np.ascontiguousarray(w).view(np.uint64)


def fp_elements(rng, n, structured):
    """n canonical Fp128 elements as uint64[n, 2]; structured: each 32-bit limb one of SPECIAL with probability 0.85, else uniform"""
    out = np.zeros((0, 2), dtype=np.uint64)
    while len(out) < n:
        a = _limbs(rng, n - len(out) + 16, 4, structured)
        ok = (a[:, 1] < np.uint64(L.P >> 64)) | ((a[:, 1] == np.uint64(L.P >> 64)) & (a[:, 0] == 0))
        out = np.concatenate([out, a[ok]])
    return out[:n]


def f64_elements(rng, n, structured):
    out = np.zeros(0, dtype=np.uint64)
    while len(out) < n:
        a = _limbs(rng, n - len(out) + 16, 2, structured).reshape(-1)
        out = np.concatenate([out, a[a < np.uint64(L.P64)]])
    return out[:n]


def fp_records():
    """the committed pairs in both operand orders at every lane position, the squared edge list, then structured-limb and uniform
    pairs shuffled together: rare-path and common-path lanes share waves"""
    pairs = L.load_pairs("fp128")
    front = np.concatenate([_every_lane(_rows(pairs + [(b, a) for a, b in pairs], 128)), _rows([(a, b) for a in L.EDGES["fp128"] for b in L.EDGES["fp128"]], 128)])
    rng = np.random.default_rng(20261021)
    n = N - len(front)
    half = n // 2
    back = np.concatenate([np.concatenate([fp_elements(rng, half, True), fp_elements(rng, n - half, False)]),
                           np.concatenate([fp_elements(rng, half, True), fp_elements(rng, n - half, False)])], axis=1)
    rec = np.concatenate([front, back[rng.permutation(n)]])
    assert rec.shape == (N, 4)
    return rec


def f64_records():
    """four words below p a row: neighbouring committed F64 pairs as (re, im), so that a.lo, b.lo and a.hi, b.hi are committed pairs
    and (a, b) is an F64_2 pair; then the squared edge list and structured-limb and uniform words"""
    ps = L.load_pairs("f64")
    ps = ps + [(b, a) for a, b in ps]
    x2 = [(a[0] | (a[1] << 64), b[0] | (b[1] << 64)) for a, b in f64x2_records(ps + ps[:1])]
    e = [(a, b) for a in L.F64_EDGES for b in L.F64_EDGES]
    x2e = [(e[i][0] | (e[i - 1][0] << 64), e[i][1] | (e[i - 1][1] << 64)) for i in range(len(e))]
    front = np.concatenate([_every_lane(_rows(x2, 128)), _rows(x2e, 128)])
    rng = np.random.default_rng(20261022)
    n = N - len(front)
    half = n // 2
    back = np.stack([np.concatenate([f64_elements(rng, half, True), f64_elements(rng, n - half, False)]) for _ in range(4)], axis=1)
    rec = np.concatenate([front, back[rng.permutation(n)]])
    assert rec.shape == (N, 4) and (rec < np.uint64(L.P64)).all()
    return rec


def gf_records():
    """any words: tests/fields_limb_model.py's records (every word in every position, full holes, every fold shift:
    tests/test_fields_limb_model.py) at every lane position, then uniform rows"""
    front = _every_lane(_rows(L.gf_records(), 128))
    rng = np.random.default_rng(20261023)
    rec = np.concatenate([front, rng.integers(0, 2**64, size=(N - len(front), 4), dtype=np.uint64)])
    assert rec.shape == (N, 4)
    return rec


def reduce_records():
    """fp_reduce_limbs takes four u64 limb accumulators: the extreme words of test_fp_reduce_limbs_matches_big_integers and uniform ones"""
    m = 2**64 - 1
    ext = [0, 1, m, 2**32, 2**32 - 1, 2**63, 0xFFFFF00000000000, 0xFFFFF, 1 << 20, (1 << 20) - 1]
    cases = []
    for a in ext:
        for b in ext:
            cases += [[a, b, ext[(a + b) % len(ext)], ext[(a ^ b) % len(ext)]], [b, 0, 0, a], [m, m, a, b]]
    cases += [[a, b, c, d] for a in (0, m, 2**32 - 1) for b in (0, m, 2**32) for c in (0, m, 1) for d in (0, m, 0xFFFFF00000000000, 2**32 - 1)]
    rng = np.random.default_rng(20261024)
    return np.concatenate([_every_lane(np.array(cases, dtype=np.uint64)), rng.integers(0, 2**64, size=(4096, 4), dtype=np.uint64)])


_cache = {}


def records(kind):
    if kind not in _cache:
        _cache[kind] = {"fp128": fp_records, "f64": f64_records, "gf": gf_records, "reduce": reduce_records}[kind]()
    return _cache[kind]


# ---- the stand-alone program
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """fields_arith_check compiled twice, with fp_mul's default one-step REDC and with -DLF_FP_REDC2"""
    d = tmp_path_factory.mktemp("fields_arith_check")
    out = {"redc1": str(d / "fields_arith_check"), "redc2": str(d / "fields_arith_check_redc2")}
    base = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17"]
    procs = [subprocess.Popen(base + flags + ["-o", out[k], CHECK]) for k, flags in (("redc1", []), ("redc2", ["-DLF_FP_REDC2"]))]
    assert [p.wait(timeout=600) for p in procs] == [0, 0]
    return out


def run(exe, rec, tmp_path):
    """one child process, one launch -> uint64[n, NOUT, 2]"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(rec).tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return np.fromfile(fout, dtype=np.uint64).reshape(len(rec), NOUT, 2)


def compare(name, got, want, rec, model=None):
    """every row; a failure names the first row and, where there is a model, the events the pair reaches"""
    assert len(got) == len(want) == len(rec)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    if bad:
        i = bad[0]
        a, b = _ints(rec[i:i + 1, 0:2])[0], _ints(rec[i:i + 1, 2:4])[0]
        ev = set()
        if model:
            model(ev)(a, b)
        pytest.fail("%s: %d of %d rows differ; the first is row %d, a = %#x, b = %#x: got %#x, want %#x; the pair reaches %s"
                    % (name, len(bad), len(want), i, a, b, got[i], want[i], sorted(ev)))


def _fp_model(op):
    return lambda ev: (lambda a, b: L.MODELS[op](a, b, ev=ev))


def _f64_model(op):
    return lambda ev: (lambda a, b: [L.MODELS[op](a & L.M64, b & L.M64, ev=ev), L.MODELS[op](a >> 64, b >> 64, ev=ev)])


@pytest.mark.parametrize("redc", ["redc1", "redc2"])
def test_fp128_every_row(exes, tmp_path, redc):
    """fp_add, fp_sub, fp_mul and fp_from_mont on the Fp128 records.  Under -DLF_FP_REDC2 the products go through the two-step REDC
    (no model of that branch: results only); the sums and differences are the same code again"""
    rec = records("fp128")
    out = run(exes[redc], rec, tmp_path)
    A, B = _ints(rec[:, 0:2]), _ints(rec[:, 2:4])
    assert max(A) < L.P and max(B) < L.P
    print("rows", len(rec))
    compare("fp_mul " + redc, _ints(out[:, FP_MUL]), [a * b * L.R_INV % L.P for a, b in zip(A, B)], rec, _fp_model("mul"))
    compare("fp_from_mont " + redc, _ints(out[:, FP_FROM_MONT]), [a * L.R_INV % L.P for a in A], rec, lambda ev: (lambda a, b: L.fp_mul_model(a, 1, ev=ev)))
    compare("fp_add", _ints(out[:, FP_ADD]), [(a + b) % L.P for a, b in zip(A, B)], rec, _fp_model("add"))
    compare("fp_sub", _ints(out[:, FP_SUB]), [(a - b) % L.P for a, b in zip(A, B)], rec, _fp_model("sub"))


def test_f64_and_f64x2_every_row(exes, tmp_path):
    rec = records("f64")
    out = run(exes["redc1"], rec, tmp_path)
    w = [rec[:, k].tolist() for k in range(4)]  # a.lo, a.hi, b.lo, b.hi
    p, ri = L.P64, L.R64_INV
    print("rows", len(rec))

    def both(o):
        return _ints(out[:, o])

    def pack(lo, hi):
        return [x | (y << 64) for x, y in zip(lo, hi)]

    add = pack([(x + y) % p for x, y in zip(w[0], w[2])], [(x + y) % p for x, y in zip(w[1], w[3])])
    sub = pack([(x - y) % p for x, y in zip(w[0], w[2])], [(x - y) % p for x, y in zip(w[1], w[3])])
    compare("f64_add", both(F64_ADD), add, rec, _f64_model("f64add"))
    compare("f64_sub", both(F64_SUB), sub, rec, _f64_model("f64sub"))
    compare("f64_mul", both(F64_MUL), pack([x * y * ri % p for x, y in zip(w[0], w[2])], [x * y * ri % p for x, y in zip(w[1], w[3])]), rec, _f64_model("f64mul"))
    compare("f64x2_add", both(X2_ADD), add, rec)
    compare("f64x2_sub", both(X2_SUB), sub, rec)
    compare("f64x2_mul", both(X2_MUL), pack(*zip(*[f64x2_mul_exact((a0, a1), (b0, b1)) for a0, a1, b0, b1 in zip(*w)])), rec)
    compare("f64x2_mul_real", both(X2_MUL_REAL), pack([x * y * ri % p for x, y in zip(w[0], w[2])], [x * y * ri % p for x, y in zip(w[1], w[2])]), rec)


def test_gf_mul_every_row(exes, tmp_path):
    rec = records("gf")
    out = run(exes["redc1"], rec, tmp_path)
    A, B = _ints(rec[:, 0:2]), _ints(rec[:, 2:4])
    print("rows", len(rec))
    compare("gf_mul", _ints(out[:, GF_MUL]), [L.gf_mul_exact(a, b) for a, b in zip(A, B)], rec)


def test_fp_reduce_limbs_every_row(exes, tmp_path):
    """its device build adds the three residues with the assembly fp_add"""
    rec = records("reduce")
    out = run(exes["redc1"], rec, tmp_path)
    want = [sum(v << (32 * k) for k, v in enumerate(r)) % L.P for r in rec.tolist()]
    compare("fp_reduce_limbs", _ints(out[:, FP_REDUCE]), want, rec)


# ---- through the ABI: the kernel the library itself compiles
@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


@pytest.mark.parametrize("field", [FP, GF])
def test_field_binop_every_row(G, field):
    import torch
    rec = records("fp128" if field == FP else "gf")
    n = len(rec)
    a, b = np.ascontiguousarray(rec[:, 0:2]), np.ascontiguousarray(rec[:, 2:4])
    A, B = _ints(a), _ints(b)
    da, db = G.to_dev(a), G.to_dev(b)
    dout = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    if field == FP:
        ops = ((0, "add", L.EXACT["add"], _fp_model("add")), (1, "sub", L.EXACT["sub"], _fp_model("sub")), (2, "mul", L.EXACT["mul"], _fp_model("mul")))
    else:
        ops = ((0, "add", lambda x, y: x ^ y, None), (1, "sub", lambda x, y: x ^ y, None), (2, "mul", L.gf_mul_exact, None))
    for op, name, exact, model in ops:
        dout.zero_()
        G.gpu().field_binop(field, op, n, da.data_ptr(), db.data_ptr(), dout.data_ptr())
        got = _ints(G.from_dev(dout, np.uint64, (n, 2)))
        compare("field_binop %s %s" % ("FP" if field == FP else "GF", name), got, [exact(x, y) for x, y in zip(A, B)], rec, model)


# ---- F64_2 end to end: the n = 2 butterfly is an add and a sub of caller-chosen operands
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("forward", [False, True])
def test_f64_2_fft_on_carry_pairs(G, n, forward):
    """rows of F64 carry pairs as (re, im) of neighbouring elements: x0 = a, x1 = b for n = 2; for n = 4 the pairs (a, b), (a', b') of
    two records as (x0, x1, x2, x3) in both interleavings, whichever elements the first butterflies join"""
    from test_gpu_parity import _f64_2_roots
    o = ol.oracle()
    w = _f64_2_roots(o)["times_i"]
    ps = L.load_pairs("f64")
    x2 = _rows([(a[0] | (a[1] << 64), b[0] | (b[1] << 64)) for a, b in f64x2_records(ps + [(b, a) for a, b in ps])], 128).reshape(-1, 2, 2)  # [record, a | b, re | im]
    if n == 2:
        rows = x2
    else:
        m = len(x2) // 2
        u, v = x2[:m], x2[m:2 * m]
        rows = np.concatenate([np.concatenate([u, v], axis=1), np.stack([u[:, 0], v[:, 0], u[:, 1], v[:, 1]], axis=1)])
    rows = np.ascontiguousarray(rows)
    assert rows.shape[1:] == (n, 2) and len(rows) > 600
    want = rows.copy()
    for r in range(len(want)):
        (o.lfo_f64_2_fftf if forward else o.lfo_f64_2_fftb)(P(want[r]), n, elt(w), 1 << 32)
    d = G.to_dev(rows)
    G.gpu().f64_2_fft(d.data_ptr(), len(rows), n, forward=forward, omega=(int(w[0]), int(w[1])))
    got = G.from_dev(d, np.uint64, rows.shape)
    assert (got == want).all(), ("rows", sorted(set(np.argwhere(got != want)[:, 0].tolist()))[:10])
    if n == 2 and not forward:
        # what the reference computed is the add and the sub of the committed pairs
        i = 0
        assert [int(x) for x in want[i].reshape(-1)] == [(int(rows[i, 0, k]) + s * int(rows[i, 1, k])) % L.P64 for s in (1, -1) for k in (0, 1)]
