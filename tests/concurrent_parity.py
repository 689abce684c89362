"""Lock-step parity harness for throughput mode: K workers in K host threads on ONE device, every result compared byte for byte.

What the rest of the suite pins is the SERIAL path: one context, one proof at a time, against the reference's recorded bytes
(fixtures, synthetic circuits).  This harness adds the link concurrent == serial: every worker first runs its own job list on an
otherwise idle device (the serial pass, which fills `expected`), then all workers run the same lists at once, and the SHA-256 of
every single result has to be the expected one.  Anchor jobs do not go through that link: they replay the fixtures' RandomEngine
and transcript seed, and their expected value is the reference's recorded wire SHA-256, never something computed in this run.

run_lockstep() is the runner and knows nothing about the GPU: a worker is any object with job(j) -> bytes (and, optionally,
describe_mismatch(j, got) -> str for the report).  tests/test_concurrent_parity_harness.py drives it with fake workers.

Workers (each with a context and stream of its own, lfgpu_own_stream, and a handle from lfgpu_circuit_share):
  ZkWorker        commit + prove of one statement per job; seeds unique per (worker, job), so a pad or a challenge of one worker
                  that lands in another's proof changes bytes
  ZkBatchWorker   ZkBatch.commit + ZkBatch.prove of 4 statements per job; expected from ZkProver.commit / prove, run serially
  VerifyWorker    zk_verify of the reference's own proof and of a copy with one bit flipped in section j of the wire
  KernelWorker    the kernel-level ABI on lfgpu_malloc'ed memory, expected from the CPU oracle

As a child process:  python tests/concurrent_parity.py '<JSON spec>'  prints one JSON report line and exits non-zero on any
failure.  The spec: {"workers": [{"kind": "zk" | "batch" | "verify" | "kernel", "stem": <fixture>, "count": n}, ...],
"njobs": jobs per worker, "anchor_every": a (0: no anchors), "env": {LFGPU_* of the case}}.  Every LFGPU_* variable of the
parent is dropped first: the switches are read once per process."""
import ctypes as C
import hashlib
import json
import lzma
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RATE, NREQ = 7, 132  # of every fixture used here
NB = 4  # statements per batch job


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ================================================================ the runner (no GPU knowledge)
def run_lockstep(workers, njobs, expected):
    """All threads wait on one event, then worker i runs job(0) .. job(njobs - 1) in order and compares sha256(result) with
    expected[i][j] after each.  The first mismatch or exception is recorded and sets a stop flag; every thread finishes the
    call it is in and joins, no job is started after the flag is up and nothing is retried.
    -> {"done": jobs finished with the expected result per worker, "started": job() calls per worker,
        "failure": None | {"worker", "job", "kind": "mismatch" | "exception", "detail"}}"""
    n = len(workers)
    njobs = [njobs] * n if isinstance(njobs, int) else list(njobs)
    done, started = [0] * n, [0] * n
    go, stop, lock = threading.Event(), threading.Event(), threading.Lock()
    failure = []

    def fail(i, j, kind, detail):
        with lock:
            if not failure:
                failure.append({"worker": i, "job": j, "kind": kind, "detail": detail})
        stop.set()

    def body(i):
        w = workers[i]
        go.wait()
        for j in range(njobs[i]):
            if stop.is_set():
                return
            started[i] += 1
            try:
                got = w.job(j)
            except BaseException as e:  # noqa: BLE001 -- the report carries it; the thread ends
                fail(i, j, "exception", "%s: %s" % (type(e).__name__, e))
                return
            h = sha(got)
            if h != expected[i][j]:
                detail = "sha256 %s, expected %s" % (h, expected[i][j])
                describe = getattr(w, "describe_mismatch", None)
                if describe is not None:
                    try:
                        detail += "; " + describe(j, got)
                    except Exception as e:  # noqa: BLE001
                        detail += "; (describe_mismatch raised %s: %s)" % (type(e).__name__, e)
                fail(i, j, "mismatch", detail)
                return
            done[i] += 1

    th = [threading.Thread(target=body, args=(i,)) for i in range(n)]
    for t in th:
        t.start()
    go.set()
    for t in th:
        t.join()
    return {"done": done, "started": started, "failure": failure[0] if failure else None}


# ================================================================ where in ZkProof::write a byte lies
def wire_sections(wire, B, logws, p, sub_bytes):
    """[(name, start, end)] of the wire bytes of one proof (csrc/zk_proto.h proof_write): the commitment root, per layer 4 logw
    round values and wc[2], the Ligero vectors (offsets: test_verifier_checks.y_offsets), the nonces, the opened columns in
    run-length-prefixed runs (full-field elements of B bytes and subfield elements of sub_bytes alternate, the first run is a
    full-field one), a 4-byte count and the Merkle path.  B, sub_bytes: 16, 2 over GF(2^128); 16, 16 over Fp128; 32, 32 over
    Fp256Base.  p: anything with LigeroParam's block, dblock, r, nreq, nrow."""
    from test_verifier_checks import y_offsets
    secs = [("commitment", 0, 32)]
    at = 32
    for ly, logw in enumerate(logws):
        secs.append(("sumcheck layer %d" % ly, at, at + B * (4 * logw + 2)))
        at = secs[-1][2]
    o = y_offsets(p, B, base=at)
    secs += [("Ligero y_ldt", o["y_ldt"], o["y_dot"]), ("Ligero y_dot", o["y_dot"], o["y_q0"]), ("Ligero y_quad", o["y_q0"], o["nonces"]),
             ("nonces", o["nonces"], o["req"])]
    at, left, sub = o["req"], p.nrow * p.nreq, False
    while left:
        run = int.from_bytes(wire[at:at + 4], "little")
        assert run <= left and at + 4 <= len(wire), "opened columns do not parse"
        at += 4 + run * (sub_bytes if sub else B)
        left -= run
        sub = not sub
    secs.append(("opened columns", o["req"], at))
    npath = int.from_bytes(wire[at:at + 4], "little")
    assert at + 4 + 32 * npath == len(wire), "Merkle path does not end the wire"
    secs.append(("Merkle path", at, len(wire)))
    return secs


def coarse_sections(secs):
    """the same with the sumcheck layers as one section"""
    sc = [s for s in secs if s[0].startswith("sumcheck layer")]
    return [secs[0], ("sumcheck", sc[0][1], sc[-1][2])] + [s for s in secs[1:] if s not in sc]


def locate(secs, off):
    for name, a, b in secs:
        if a <= off < b:
            return name
    return "past the end"


def first_difference(a, b):
    """the first offset at which two byte strings differ (the shorter length where one is a prefix), None when equal"""
    if a == b:
        return None
    n = min(len(a), len(b))
    lo, hi = 0, n
    if a[:n] == b[:n]:
        return n
    while hi - lo > 1:  # a[:lo] == b[:lo], a[:hi] != b[:hi]
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def describe_wire_difference(got, want, secs, what="the serial run"):
    off = first_difference(got, want)
    if off is None:
        return "equal bytes"
    name = locate(secs, off)
    start = dict((s[0], s[1]) for s in secs).get(name, 0)
    return "first byte that differs from %s: offset %d, in %s (+%d); %d bytes, expected %d" % (what, off, name, off - start, len(got), len(want))


# ================================================================ fixtures
_stems = {}


def load_stem(stem):
    """circuit bytes, witness and the reference's record of one fixture; read once per process"""
    if stem not in _stems:
        import numpy as np
        sig = stem == "mdoc_sig"
        raw = lzma.decompress(open(os.path.join(GOLD, stem + ".lfc1.xz"), "rb").read())
        W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, stem + ".w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 4 if sig else 2).copy()
        if stem.startswith("mdoc"):
            info = json.load(open(os.path.join(GOLD, "mdoc.json")))["sig" if sig else "hash"]
            be = info["block_enc"]
        else:
            info = json.load(open(os.path.join(GOLD, stem + ".json")))
            be = 0
        _stems[stem] = dict(stem=stem, raw=raw, W=W, be=be, info=info, wire_bytes=info["zk_wire_bytes"], wire_sha=info["zk_wire_sha256"])
    return _stems[stem]


def field_bytes(pkg, field):
    """(element bytes, bytes of a subfield element in the opened columns)"""
    return {pkg.FIELD_GF2_128: (16, 2), pkg.FIELD_FP128: (16, 16), pkg.FIELD_P256: (32, 32)}[field]


class _Statement:
    """what the prover-level workers share: a context with its own stream, the shared circuit, the wire layout"""

    def __init__(self, pkg, base, st, index, device):
        self.pkg, self.st, self.index = pkg, st, index
        self.gpu = pkg.LfGpu(device).own_stream()
        self.L = self.gpu.L
        self.circ = base[st["stem"]].share(self.gpu)
        self.B, self.sub_bytes = field_bytes(pkg, self.circ.info.field)
        self.logws = [self.circ.layer(i)["logw"] for i in range(self.circ.info.nl)]
        self.rng_fn = C.cast(self.L.lfgpu_transcript_bytes, pkg.RNG_FN)  # the library's transcript as a C-speed RandomEngine
        self.Wp = C.c_void_p(st["W"].ctypes.data)

    def new_prover(self):
        return self.pkg.ZkProver(self.gpu, self.circ, RATE, NREQ, self.st["be"])

    def prove(self, zk, eng_seed, ts_seed):
        """commit + prove of one statement: engine lfgpu_transcript_bytes over FsTranscript(eng_seed), transcript seed ts_seed"""
        eng, ts = self.pkg.FsTranscript(eng_seed), self.pkg.FsTranscript(ts_seed)
        try:
            ops = ts.ops()
            root, ok = (C.c_uint8 * 32)(), C.c_int()
            self.gpu._ck(self.L.lfgpu_zk_commit(zk.h, self.Wp, self.rng_fn, eng.h, C.byref(ops), root))
            self.gpu._ck(self.L.lfgpu_zk_prove(zk.h, self.Wp, C.byref(ops), C.byref(ok)))
            assert ok.value == 1, "prove failed: " + self.st["stem"]
            return zk.wire()
        finally:
            eng.close()
            ts.close()

    def sections(self, wire, p):
        return wire_sections(wire, self.B, self.logws, p, self.sub_bytes)


class ZkWorker(_Statement):
    kind = "zk"

    def __init__(self, pkg, base, st, index, njobs, anchor_every, device=0):
        super().__init__(pkg, base, st, index, device)
        self.zk = self.new_prover()
        self.njobs, self.anchor_every = njobs, anchor_every
        self.serial_wire = {}

    def is_anchor(self, j):
        return self.anchor_every > 0 and j % self.anchor_every == 0

    def job(self, j):
        if not self.is_anchor(j):
            return self.prove(self.zk, b"eng w%d j%d" % (self.index, j), b"ts w%d j%d" % (self.index, j))
        import ligero_fixture as lf
        ts = self.pkg.FsTranscript(b"test")
        try:
            self.zk.commit(self.st["W"], lf.LcgRng(100).bytes, ts)
            assert self.zk.prove(self.st["W"], ts), "prove failed: " + self.st["stem"]
            return self.zk.wire()
        finally:
            ts.close()

    def serial(self):
        """the job list on an idle device -> expected SHA-256 per job; an anchor's is the reference's, whatever this run gave"""
        exp = []
        for j in range(self.njobs):
            self.serial_wire[j] = w = self.job(j)
            if self.is_anchor(j):
                assert len(w) == self.st["wire_bytes"] and sha(w) == self.st["wire_sha"], \
                    "serial pass: the wire of %s (job %d) is not the reference's" % (self.st["stem"], j)
            exp.append(self.st["wire_sha"] if self.is_anchor(j) else sha(w))
        return exp

    def describe_mismatch(self, j, got):
        want = self.serial_wire[j]
        return describe_wire_difference(got, want, self.sections(want, self.zk.param))

    def close(self):
        self.zk.close()
        self.circ.close()
        self.gpu.close()


class ZkBatchWorker(_Statement):
    kind = "batch"

    def __init__(self, pkg, base, st, index, njobs, anchor_every=0, device=0):
        super().__init__(pkg, base, st, index, device)
        self.njobs = njobs
        self.provers = [self.new_prover() for _ in range(NB)]
        self.batch = pkg.ZkBatch(self.gpu, self.circ, NB)
        self.serial_wire = {}

    def is_anchor(self, j):
        return False

    def seeds(self, j, b):
        return b"eng w%d j%d b%d" % (self.index, j, b), b"ts w%d j%d b%d" % (self.index, j, b)

    def job(self, j):
        pkg, W = self.pkg, self.st["W"]
        engs = [pkg.FsTranscript(self.seeds(j, b)[0]) for b in range(NB)]
        tss = [pkg.FsTranscript(self.seeds(j, b)[1]) for b in range(NB)]
        try:
            self.batch.commit(self.provers, [W] * NB, [e.bytes for e in engs], tss)
            assert self.batch.prove(self.provers, [W] * NB, tss) == [True] * NB, "prove_batch failed: " + self.st["stem"]
            return b"".join(zk.wire() for zk in self.provers)
        finally:
            for t in engs + tss:
                t.close()

    def serial(self):
        """expected: the single-statement path with the same seeds, one statement after the other"""
        exp = []
        for j in range(self.njobs):
            self.serial_wire[j] = [self.prove(self.provers[b], *self.seeds(j, b)) for b in range(NB)]
            exp.append(sha(b"".join(self.serial_wire[j])))
        return exp

    def describe_mismatch(self, j, got):
        at = 0
        for b, want in enumerate(self.serial_wire[j]):
            part = got[at:at + len(want)]
            if part != want:
                return "statement %d of the batch: " % b + describe_wire_difference(part, want, self.sections(want, self.provers[b].param),
                                                                                   "ZkProver.commit / prove")
            at += len(want)
        return "%d bytes after the last statement" % (len(got) - at)

    def close(self):
        self.batch.close()
        for zk in self.provers:
            zk.close()
        self.circ.close()
        self.gpu.close()


class VerifyWorker(_Statement):
    kind = "verify"

    def __init__(self, pkg, base, st, index, njobs, anchor_every=0, device=0):
        super().__init__(pkg, base, st, index, device)
        from test_zk_cxx import wire_from_components
        self.njobs = njobs
        fp = self.circ.info.field == pkg.FIELD_FP128
        p = pkg.ligero_param(self.circ.info.field, st["info"]["zk_nw"], self.circ.info.nl, RATE, NREQ, st["be"])
        comp = lzma.decompress(open(os.path.join(GOLD, st["stem"] + ".zkproof.xz"), "rb").read())
        self.wire = wire_from_components(comp, self.logws, p, fp128=fp)  # the reference's own proof
        assert len(self.wire) == st["wire_bytes"] and sha(self.wire) == st["wire_sha"], "the fixture's proof does not re-serialise: " + st["stem"]
        self.secs = coarse_sections(self.sections(self.wire, p))
        self.pub = st["W"][:self.circ.info.npub_in]
        self.serial_result = {}

    def is_anchor(self, j):
        return False

    def verify(self, wire):
        ts = self.pkg.FsTranscript(b"test")
        try:
            return self.pkg.zk_verify(self.gpu, self.circ, wire, self.pub, ts, RATE, NREQ, self.st["be"])
        finally:
            ts.close()

    def job(self, j):
        name, a, b = self.secs[j % len(self.secs)]
        bad = bytearray(self.wire)
        bad[(a + b) // 2] ^= 0x04
        honest, tampered = self.verify(self.wire), self.verify(bytes(bad))
        assert honest == (True, "ok"), "the reference's proof refused: %r" % (honest,)
        assert tampered[0] is False and tampered[1] != "ok", "a flipped bit in %s accepted: %r" % (name, tampered)
        return repr((honest, tampered)).encode()

    def serial(self):
        exp = []
        for j in range(self.njobs):
            self.serial_result[j] = self.job(j)
            exp.append(sha(self.serial_result[j]))
        return exp

    def describe_mismatch(self, j, got):
        return "section %s: answered %s, on an idle device %s" % (self.secs[j % len(self.secs)][0], got.decode(), self.serial_result[j].decode())

    def close(self):
        self.circ.close()
        self.gpu.close()


# ================================================================ the kernel-level ABI
_cases = None


def kernel_cases(pkg):
    """[(name, input arrays, expected result bytes, run(gpu, device pointers, fetch) -> result bytes)]: the smallest shapes of
    tests/test_gpu_parity.py and tests/test_p256_gpu.py, inputs seeded as there, every expected result from the CPU oracle.
    Computed once per process; read-only afterwards."""
    global _cases
    if _cases is not None:
        return _cases
    import numpy as np

    import oracle_lib as ol
    from oracle_lib import GF, P, elt
    from test_p256_cpu import fill
    o = ol.oracle()
    cases = []

    def in_place(name, a, want, call):
        def run(gpu, d, fetch):
            call(gpu, d[0])
            return fetch(d[0], a).tobytes()
        cases.append((name, [a], want.tobytes(), run))

    for n, rows, forward in ((1 << 10, 2, False), (1 << 13, 3, True)):
        a = np.zeros((rows, n, 2), dtype=np.uint64)
        for r in range(rows):
            o.lfo_fp_bogorng_fill(1234569 + r, n, P(a[r]))
        want = a.copy()
        for r in range(rows):
            (o.lfo_fp_fftf if forward else o.lfo_fp_fftb)(P(want[r]), n, o.lfo_fp_omega32(), 1 << 32)
        in_place("fp128_fft %dx%d %s" % (n, rows, "forward" if forward else "backward"), a, want,
                 lambda gpu, d, rows=rows, n=n, forward=forward: gpu.fp128_fft(d, rows, n, forward=forward))

    n, rows = 1 << 12, 2
    w = np.array([o.lfo_f64_omega32(), 0], dtype=np.uint64)
    a = np.zeros((rows, n, 2), dtype=np.uint64)
    for r in range(rows):
        o.lfo_f64_2_bogorng_fill(1234569 + r, 1, n, P(a[r]))
    want = a.copy()
    for r in range(rows):
        o.lfo_f64_2_fftb(P(want[r]), n, elt(w), 1 << 32)
    in_place("f64_2_fft %dx%d" % (n, rows), a, want, lambda gpu, d, rows=rows, n=n, w=w: gpu.f64_2_fft(d, rows, n, omega=(int(w[0]), int(w[1]))))

    k = 4
    ctx = ol.gf_ctx(k)
    for l, rows, coset, ld, seed in ((10, 3, 0, 1 << 10, 10 * 7 + k), (7, 40, 128, (1 << 7) + 5, 7 * 13 + k + 40)):  # the second: bit-sliced
        a = ol.rand_elts(np.random.default_rng(seed), rows * ld).reshape(rows, ld, 2)
        want = a.copy()
        for r in range(rows):
            row = np.ascontiguousarray(want[r, :1 << l])
            o.lfo_lch14_fft(C.byref(ctx), l, coset, P(row))
            want[r, :1 << l] = row
        in_place("gf2128_lch14_fft l=%d x%d" % (l, rows), a, want,
                 lambda gpu, d, rows=rows, l=l, coset=coset, ld=ld: gpu.gf2128_lch14_fft(d, rows, l, coset=coset, ld=ld))

    n, m, nrow = 21, 128, 8
    ld = m + 3
    T = ol.rand_elts(np.random.default_rng(n * 3 + m), nrow * ld).reshape(nrow, ld, 2)
    want = T.copy()
    for r in range(nrow):
        o.lfo_lch14_rs_interpolate(C.byref(ctx), n, m, P(want[r]))
    in_place("gf2128_rs_encode_rows (21, 128, 8)", T, want, lambda gpu, d, ld=ld: gpu.gf2128_rs_encode_rows(d, 8, 21, 128, ld=ld))

    n, m, nrow = 21, 128, 4
    T = np.zeros((nrow, m, 2), dtype=np.uint64)
    o.lfo_fp_bogorng_fill(5 + n, nrow * m, P(T))
    want = T.copy()
    for r in range(nrow):
        o.lfo_fp_rs_interpolate(n, m, P(want[r]))
    in_place("fp128_rs_encode_rows (21, 128, 4)", T, want, lambda gpu, d: gpu.fp128_rs_encode_rows(d, 4, 21, 128))

    n, m, nrow = 5, 16, 5
    T = fill(7 * n + m, nrow * m).reshape(nrow, m, 4)
    want = T.copy()
    for r in range(nrow):
        o.lfo_p256_rs_interpolate(n, m, P(want[r]))
    in_place("fp256_rs_encode_rows (5, 16, 5)", T, want, lambda gpu, d: gpu.fp256_rs_encode_rows(d, 5, 5, 16))

    def commit(name, field, nrow, ld, col0, ncols, T, rng):
        nonces = rng.integers(0, 256, size=(ncols, 32), dtype=np.uint8)
        layers = np.zeros((2 * ncols, 32), dtype=np.uint8)
        root = np.zeros(32, dtype=np.uint8)
        if field == pkg.FIELD_P256:
            o.lfo_column_commit32(nrow, ld, col0, ncols, P(T), P(nonces), P(root), P(layers))
        else:
            o.lfo_column_commit(field, nrow, ld, col0, ncols, P(T), P(nonces), P(root), P(layers))
        zero = np.zeros_like(layers)

        def run(gpu, d, fetch):
            got = gpu.column_commit(field, nrow, ld, col0, ncols, d[0], d[1], d[2])
            return got + fetch(d[2], zero)[1:].tobytes()
        cases.append((name, [T, nonces, zero], root.tobytes() + layers[1:].tobytes(), run))

    nrow, ld = 2, 8
    rng = np.random.default_rng(nrow * ld)
    commit("column_commit GF (2, 8, 1, 1)", GF, nrow, ld, 1, 1, ol.rand_elts(rng, nrow * ld, GF), rng)
    nrow, ld = 19, 600
    commit("column_commit P-256 (19, 600, 131, 469)", pkg.FIELD_P256, nrow, ld, 131, 469, fill(nrow + ld, nrow * ld).reshape(nrow, ld, 4),
           np.random.default_rng(nrow * 1000 + 469))

    n = 1000
    rng = np.random.default_rng(n)
    leaves = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    layers = np.zeros((2 * n, 32), dtype=np.uint8)
    o.lfo_merkle_build_tree(n, P(leaves), P(layers))
    pos = sorted(set(int(x) for x in rng.integers(0, n, size=7)))
    tree = [False] * (2 * n)  # the compressed opening (merkle_tree.h:122-143) replayed from the oracle's layers
    for p_ in pos:
        tree[p_ + n] = True
    for i in range(n - 1, 0, -1):
        tree[i] = tree[2 * i] or tree[2 * i + 1]
    path = []
    for i in range(n - 1, 0, -1):
        if tree[i]:
            ch = 2 * i + 1 if tree[2 * i] else 2 * i
            if not tree[ch]:
                path.append(bytes(layers[ch]))
    dev = np.zeros((2 * n, 32), dtype=np.uint8)
    dev[n:] = leaves
    cases.append(("merkle_build_tree + merkle_open n=1000", [dev], bytes(layers[1]) + b"".join(path),
                  lambda gpu, d, fetch: gpu.merkle_build_tree(n, d[0]) + b"".join(gpu.merkle_open(n, d[0], pos))))
    _cases = cases
    return cases


class KernelWorker:
    """three passes through kernel_cases(), entered at position `index` so that different kernels overlap; device memory
    of its own (lfgpu_malloc), uploaded again before every call"""
    kind = "kernel"

    def __init__(self, pkg, base, st, index, njobs, anchor_every=0, device=0):
        self.pkg, self.index = pkg, index
        self.cases = kernel_cases(pkg)
        self.njobs = njobs * len(self.cases)  # njobs: passes
        self.gpu = pkg.LfGpu(device).own_stream()
        self.dev = [[self.gpu.malloc(a.nbytes) for a in arrays] for _, arrays, _, _ in self.cases]

    def is_anchor(self, j):
        return False

    def case(self, j):
        return (self.index + j) % len(self.cases)

    def fetch(self, d, like):
        import numpy as np
        out = np.empty_like(like)
        self.gpu.memcpy_d2h(out, d)
        return out

    def job(self, j):
        c = self.case(j)
        _, arrays, _, run = self.cases[c]
        for d, a in zip(self.dev[c], arrays):
            self.gpu.memcpy_h2d(d, a)
        return run(self.gpu, self.dev[c], self.fetch)

    def serial(self):
        """no serial pass: the oracle's results are the expected ones, and the first call of every kernel of a context (the
        tables and scratch buffers it builds) happens under load"""
        return [sha(self.cases[self.case(j)][2]) for j in range(self.njobs)]

    def describe_mismatch(self, j, got):
        name, _, want, _ = self.cases[self.case(j)]
        return "%s: first byte that differs from the oracle at offset %s of %d" % (name, first_difference(got, want), len(want))

    def close(self):
        for ds in self.dev:
            for d in ds:
                self.gpu.free(d)
        self.gpu.close()


KINDS = {"zk": ZkWorker, "batch": ZkBatchWorker, "verify": VerifyWorker, "kernel": KernelWorker}


# ================================================================ the child process
def main(argv):
    spec = json.loads(argv[1])
    for k in list(os.environ):
        if k.startswith("LFGPU_"):
            del os.environ[k]
    os.environ.update(spec.get("env", {}))
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")  # as tools/zk_throughput.py: before the first HIP call
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    pkg = ge.load_package()
    t0 = time.perf_counter()
    report = {"workers": [], "failure": None}
    workers, base = [], {}
    base_gpu = pkg.LfGpu(0)  # uploads the circuits and proves nothing: no stream of its own, no sharer of the device
    try:
        for g in spec["workers"]:
            st = None
            if g["kind"] != "kernel":
                st = load_stem(g["stem"])
                if g["stem"] not in base:
                    base[g["stem"]] = pkg.Circuit(base_gpu, st["raw"])
            for _ in range(g["count"]):
                workers.append(KINDS[g["kind"]](pkg, base, st, len(workers), spec["njobs"], spec.get("anchor_every", 0)))
                report["workers"].append(g["kind"] + ":" + g.get("stem", "abi"))
        assert len(workers) <= 8, "at most 8 threads"
        t1 = time.perf_counter()
        expected = [w.serial() for w in workers]  # every worker in turn, all the others idle
        t2 = time.perf_counter()
    except BaseException as e:  # noqa: BLE001 -- nothing further is started on the GPU
        report["failure"] = {"worker": len(report["workers"]) - 1, "job": None, "kind": "setup or serial pass", "detail": "%s: %s" % (type(e).__name__, e)}
        return finish(report)
    njobs = [w.njobs for w in workers]
    report.update(run_lockstep(workers, njobs, expected))
    t3 = time.perf_counter()
    report.update(njobs=njobs, compared=sum(report["done"]),
                  anchored=sum(1 for w, d in zip(workers, report["done"]) for j in range(d) if w.is_anchor(j)),
                  setup_s=round(t1 - t0, 2), serial_s=round(t2 - t1, 2), concurrent_s=round(t3 - t2, 2))
    if report["failure"] is None and report["done"] != njobs:
        report["failure"] = {"worker": None, "job": None, "kind": "incomplete", "detail": "jobs done %r of %r" % (report["done"], njobs)}
    if report["failure"] is None:
        for w in workers:
            w.close()
        for c in base.values():
            c.close()
        base_gpu.close()
    return finish(report)


def finish(report):
    """after a failure the handles are left as they are: releasing them is GPU work, and a HIP error may be the failure"""
    print(json.dumps(report), flush=True)
    sys.stderr.flush()
    os._exit(0 if report["failure"] is None else 1)


if __name__ == "__main__":
    main(sys.argv)
