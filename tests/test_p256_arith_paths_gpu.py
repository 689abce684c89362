"""The device instructions of the Fp256Base arithmetic (csrc/fp256.h, the __HIP_DEVICE_COMPILE__ path) on every carry path, every row
compared.  The host compilation of that header is different code, and uniform 256-bit operands reach the rare links of the chains
with probability about 2^-32 each; tests/golden/p256_carry_pairs.json is a set of operand pairs that reaches every reachable link
of fp256_mul, fp256_add and fp256_sub at least four times and notices the loss of any one of them (tests/p256_limb_model.py,
tests/test_p256_limb_model.py).  Here those pairs, structured-limb and uniform ones go through

  field_binop(FIELD_P256, add | sub | mul)                          against Python integers, all rows,
  fp256_rs_encode_rows                                              against lfo_p256_rs_interpolate,
  Quad.sumcheck_layer256, sumcheck_layer_batch256, eval_quad_batch256   against tests/p256_layer_model.py,

the last two because the same inline assembly sits there under other register pressure, and their tests feed it uniform data only.
Bit-exact, canonical operands only."""
import numpy as np
import pytest

import oracle_lib as ol
import p256_layer_model as M
import p256_limb_model as L
from oracle_lib import FP, P
from test_sumcheck_layer_random import _morton, make_layer_vec

pytestmark = pytest.mark.gpu

P256 = 1  # LFGPU_FIELD_P256
SPECIAL = np.array(L.SPECIAL, dtype=np.uint32)
P_WORDS = [(L.P >> (64 * k)) & (2**64 - 1) for k in range(4)]
PM1 = [(L.P - 1 >> (64 * k)) & (2**64 - 1) for k in range(4)]
STRIDE = 67
N_RANDOM = 1 << 16  # structured-limb pairs, and as many uniform ones


def below_p(a):
    """uint64[n, 4] little-endian words -> bool[n]: the value is below p"""
    lt = np.zeros(len(a), dtype=bool)
    eq = np.ones(len(a), dtype=bool)
    for k in (3, 2, 1, 0):
        w = np.uint64(P_WORDS[k])
        lt |= eq & (a[:, k] < w)
        eq &= a[:, k] == w
    return lt


def _draw(rng, n, structured):
    if not structured:
        return rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    w = rng.integers(0, 2**32, size=(n, 8), dtype=np.uint32)
    pick = rng.random((n, 8)) < 0.9
    w = np.where(pick, SPECIAL[rng.integers(0, len(SPECIAL), size=(n, 8))], w)
    return np.ascontiguousarray(w).view(np.uint64)


def elements(rng, n, structured=True):
    """n canonical elements as uint64[n, 4].  structured: each 32-bit limb one of SPECIAL with probability 0.9, else uniform"""
    out = np.zeros((0, 4), dtype=np.uint64)
    while len(out) < n:
        a = _draw(rng, n - len(out) + 16, structured)
        out = np.concatenate([out, a[below_p(a)]])
    return np.ascontiguousarray(out[:n])


def words(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(len(ints), 4).copy()


def ints(a):
    raw = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def binop_rows():
    """-> (a, b) as uint64[n, 4] and the row ranges by name.  Front: the committed pairs in both operand orders, packed, then the edge
    pairs of test_p256_binops that are canonical.  Then structured-limb and uniform pairs, shuffled together, with the committed pairs
    once more at every STRIDE-th row: rare-path and common-path lanes share waves."""
    pairs = L.load_pairs()
    both = pairs + [(b, a) for a, b in pairs]
    e = [[0, 0, 0, 0], [1, 0, 0, 0], PM1, [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF00000000], [0, 0, 0, 1], [0xFFFFFFFFFFFFFFFF, 0, 0, 0],
         [0, 1 << 32, 0, 0], [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF]]
    e = [v for v in ints(np.array(e, dtype=np.uint64)) if v < L.P]
    edge = [(x, y) for x in e for y in e]
    front = words([a for a, _ in both + edge]), words([b for _, b in both + edge])
    rng = np.random.default_rng(20261021)
    ra = np.concatenate([elements(rng, N_RANDOM), elements(rng, N_RANDOM, structured=False)])
    rb = np.concatenate([elements(rng, N_RANDOM), elements(rng, N_RANDOM, structured=False)])
    perm = rng.permutation(len(ra))
    ra, rb = ra[perm], rb[perm]
    nback = len(ra) + len(both)
    assert STRIDE * len(both) <= nback
    at = np.zeros(nback, dtype=bool)
    at[STRIDE * np.arange(len(both))] = True
    back = [np.zeros((nback, 4), dtype=np.uint64) for _ in range(2)]
    for dst, committed, rnd in zip(back, front, (ra, rb)):
        dst[at] = committed[:len(both)]
        dst[~at] = rnd
    a, b = np.concatenate([front[0], back[0]]), np.concatenate([front[1], back[1]])
    assert below_p(a).all() and below_p(b).all()
    return a, b, dict(committed=len(both), edge=len(edge), scattered=len(both), random=len(ra))


def test_field_binop_every_row(G):
    import torch
    a, b, parts = binop_rows()
    n = len(a)
    A, B = ints(a), ints(b)
    print("rows per op", n, parts)
    da, db = G.to_dev(a), G.to_dev(b)
    dout = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    for op, name in ((0, "add"), (1, "sub"), (2, "mul")):
        G.gpu().field_binop(P256, op, n, da.data_ptr(), db.data_ptr(), dout.data_ptr())
        got = ints(G.from_dev(dout, np.uint64, (n, 4)))
        exact = L.EXACT[name]
        bad = [i for i in range(n) if got[i] != exact(A[i], B[i])]
        if bad:
            i = bad[0]
            ev = set()
            L.MODELS[name](A[i], B[i], ev=ev)
            pytest.fail("%s: %d of %d rows differ; the first is row %d, a = %#x, b = %#x: got %#x, want %#x; the pair reaches %s"
                        % (name, len(bad), n, i, A[i], B[i], got[i], exact(A[i], B[i]), sorted(ev)))


RS_KINDS = ("structured", "all p - 1", "zero", "one-hot")


@pytest.mark.parametrize("n,m,nrow,ld", [(1, 2, 1, 2), (3, 8, 2, 8), (21, 128, 4, 130), (100, 257, 3, 257)])
def test_rs_encode_rows_structured(G, n, m, nrow, ld):
    """every kind of row at every shape: as many calls of nrow rows as it takes to go through RS_KINDS"""
    o = ol.oracle()
    rng = np.random.default_rng(1000 * n + m)
    for call in range(-(-len(RS_KINDS) // nrow)):
        T = elements(rng, nrow * ld).reshape(nrow, ld, 4)
        for r in range(nrow):
            kind = RS_KINDS[(call * nrow + r) % len(RS_KINDS)]
            if kind == "all p - 1":
                T[r, :n] = PM1
            elif kind == "zero":
                T[r, :n] = 0
            elif kind == "one-hot":
                hot = T[r, n // 2].copy()
                T[r, :n] = 0
                T[r, n // 2] = hot if hot.any() else PM1
        want = T.copy()
        for r in range(nrow):
            row = np.ascontiguousarray(want[r, :m])
            o.lfo_p256_rs_interpolate(n, m, P(row))
            want[r, :m] = row
        d = G.to_dev(T)
        G.gpu().fp256_rs_encode_rows(d.data_ptr(), nrow, n, m, ld=ld)
        got = G.from_dev(d, np.uint64, T.shape)
        assert (got == want).all(), ("call", call, "rows", sorted(set(np.argwhere(got != want)[:, 0].tolist())))


# ---- the sumcheck layer and eval_quad on structured-limb elements
B = 3
LAYERS = ("tiny", "small", "fan", "star", "diag")
_layers = {}


def _tup(e):
    return tuple(int(x) for x in e)


def _canonical(g, h0, h1, nv, logv, logw, rng):
    """a layer from distinct (g, h0 <= h1) terms, in canonical order: by the Morton code of the hands, then by the output"""
    assert len(set(zip(g.tolist(), h0.tolist(), h1.tolist()))) == len(g) and (h0 <= h1).all()
    order = np.lexsort((g, _morton(h0, h1)))
    g, h0, h1 = (np.ascontiguousarray(x[order], dtype=np.uint32) for x in (g, h0, h1))
    return dict(g=g, h0=h0, h1=h1, vi=rng.integers(1, 9, size=len(g), dtype=np.uint32), nv=nv, nw=1 << logw, logv=logv, logw=logw, n=len(g))


def _pick(rng, n, *dims):
    """n distinct index tuples below dims"""
    flat = rng.permutation(int(np.prod(dims)))[:n]
    return np.unravel_index(flat, dims)


def make_layer(name):
    """tiny and small: the shapes of test_sumcheck_layer_batch256.py.  fan, star, diag: 300 terms over 64 wires that make_layer_vec
    cannot produce -- fan: one output (logv = 0), every term accumulates into it; star: h0 = 0 in every term, one long run for the
    scatter; diag: h0 = h1 in every term"""
    rng = np.random.default_rng(sum(name.encode()))
    if name in ("tiny", "small"):
        logv, logw, nterms, *shape = {"tiny": (2, 3, 8, 3, 5), "small": (5, 6, 300)}[name]
        Lr = make_layer_vec(rng, FP, logv, logw, nterms, *([9] + shape if shape else []))
        del Lr["W"], Lr["kvec"]
    elif name == "fan":
        tri = np.array([(a, b) for a in range(64) for b in range(a, 64)], dtype=np.int64)
        tri = tri[rng.permutation(len(tri))[:300]]
        Lr = _canonical(np.zeros(300, dtype=np.int64), tri[:, 0], tri[:, 1], 1, 0, 6, rng)
    elif name == "star":
        g, h1 = _pick(rng, 300, 8, 64)
        Lr = _canonical(g, np.zeros(300, dtype=np.int64), h1, 8, 3, 6, rng)
    else:
        g, h = _pick(rng, 300, 8, 64)
        Lr = _canonical(g, h, h, 8, 3, 6, rng)
    return Lr, rng


def layer(name):
    """the layer, B statements of structured-limb elements over it (statement 1's wires are all p - 1) and the model's results"""
    if name not in _layers:
        Lr, rng = make_layer(name)
        logv, logw, nw = Lr["logv"], Lr["logw"], Lr["nw"]
        Lr["kvec"] = elements(rng, 9)
        Lr["kvec"][0] = 0
        assert Lr["kvec"][1:].any(axis=1).all()  # no assert-zero term: vi >= 1
        st = []
        for b in range(B):
            W = elements(rng, nw)
            if b == 1:
                W[:] = PM1
            e = elements(rng, 4 + 2 * logw)
            st.append(dict(W=W, G0=elements(rng, max(1, logv)), G1=elements(rng, max(1, logv)), alpha=_tup(e[0]), beta=_tup(e[1]),
                           wc_in=[_tup(e[2]), _tup(e[3])], chal=[_tup(x) for x in e[4:]]))
        want = [M.layer(M.P256, Lr, Lr["kvec"], s["W"], logv, s["G0"], s["G1"], s["alpha"], s["beta"], s["wc_in"], s["chal"])[:3] for s in st]
        wantV = [M.eval_quad(M.P256, Lr, Lr["kvec"], s["W"]) for s in st]
        _layers[name] = (Lr, st, want, wantV)
    return _layers[name]


def test_the_three_new_layers_are_what_they_say():
    fan, star, diag = (layer(n)[0] for n in ("fan", "star", "diag"))
    for Lr in (fan, star, diag):
        assert Lr["n"] == 300 and Lr["logw"] == 6 and Lr["nw"] == 64
        key = list(zip(_morton(Lr["h0"], Lr["h1"]).tolist(), Lr["g"].tolist()))
        assert key == sorted(set(key)) and (Lr["h0"] <= Lr["h1"]).all()  # canonical order, no term twice
    assert fan["logv"] == 0 and fan["nv"] == 1 and not fan["g"].any()
    assert not star["h0"].any() and (diag["h0"] == diag["h1"]).all()
    assert set(ints(layer("fan")[1][1]["W"])) == {L.P - 1}


@pytest.mark.parametrize("name", LAYERS)
def test_sumcheck_layer_structured(G, name):
    """sumcheck_layer256 on each statement and sumcheck_layer_batch256 on the three together: evaluations of every round-hand, the
    wire claims and the bound quad equal the model's"""
    Lr, st, want, _ = layer(name)
    logv, logw, nw = Lr["logv"], Lr["logw"], Lr["nw"]
    q = G.pkg.Quad(G.gpu(), P256, Lr["g"], Lr["h0"], Lr["h1"], Lr["vi"], Lr["kvec"], Lr["nv"])
    for b, s in enumerate(st):
        dW = G.to_dev(s["W"])
        got = []

        def cb(hand, rnd, ev):
            got.append(tuple(_tup(e) for e in ev))
            return s["chal"][len(got) - 1]

        wc, _, bq = q.sumcheck_layer256(logv, s["G0"], s["G1"], s["alpha"], s["beta"], logw, nw, dW.data_ptr(), s["wc_in"], cb)
        assert (got, [_tup(w) for w in wc], _tup(bq)) == want[b], "statement %d, sumcheck_layer256" % b
    Wb = np.stack([s["W"] for s in st])
    dW = G.to_dev(Wb)
    G0 = np.concatenate([s["G0"][:logv] for s in st]) if logv else np.zeros((1, 4), dtype=np.uint64)
    G1 = np.concatenate([s["G1"][:logv] for s in st]) if logv else np.zeros((1, 4), dtype=np.uint64)
    gotb, calls = [[] for _ in st], []

    def cbb(hand, rnd, evals):
        calls.append((rnd, hand))
        for b in range(B):
            gotb[b].append(tuple(_tup(e) for e in evals[b]))
        return [s["chal"][len(calls) - 1] for s in st]

    wc, _, bq = q.sumcheck_layer_batch256(logv, G0, G1, [s["alpha"] for s in st], [s["beta"] for s in st], logw, nw, dW.data_ptr(), nw,
                                          [s["wc_in"] for s in st], cbb)
    q.close()
    assert (G.from_dev(dW, np.uint64, Wb.shape) == Wb).all()
    for b in range(B):
        assert (gotb[b], [_tup(w) for w in wc[b]], _tup(bq[b])) == want[b], "statement %d, sumcheck_layer_batch256" % b


@pytest.mark.parametrize("name", LAYERS)
def test_eval_quad_batch_structured(G, name):
    Lr, st, _, wantV = layer(name)
    nw, nv = Lr["nw"], Lr["nv"]
    q = G.pkg.Quad(G.gpu(), P256, Lr["g"], Lr["h0"], Lr["h1"], Lr["vi"], Lr["kvec"], nv)
    dW = G.to_dev(np.stack([s["W"] for s in st]))
    dV = G.to_dev(np.zeros((B, nv, 4), dtype=np.uint64))
    ok = q.eval_quad_batch256(B, nw, dW.data_ptr(), nw, dV.data_ptr(), nv)
    q.close()
    V = G.from_dev(dV, np.uint64, (B, nv, 4))
    for b in range(B):
        assert ok[b] == wantV[b][1] and (V[b] == wantV[b][0]).all(), "statement %d" % b
