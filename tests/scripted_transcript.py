"""A Fiat-Shamir transcript for the test harness whose challenges do not depend on what is written to it.

The library reaches the caller's transcript through function pointers (lfgpu_transcript_ops, include/lfgpu_zk.h), so a test may
serve one of its own.  Under the real SHA/AES transcript every proof byte feeds every later challenge: a flipped element of
y_ldt moves the opened columns and the Merkle check refuses before the low-degree check is asked.  Here a write hook never
reads its payload, only its SHAPE, so a tampered proof is checked under the honest proof's challenges and the check that owns
the tampered section has to be the one that refuses (tests/test_verifier_checks.py).

State of a lineage: (key, pos, epoch).
  write (tag 0 bytes, 1 element, 2 array -- the real transcript's tags):
      key = SHA-256(key || tag || u64 length-or-count || u64 payload bytes), pos = 0, epoch += 1
  gen_bytes(n): the next n bytes of the epoch's stream  SHA-256(key || u64 0) || SHA-256(key || u64 1) || ...
This is the reset-on-write structure of the real transcript (any write re-keys the PRF), so a prover and a verifier that agree
under the real transcript agree under this one.

clone() copies (key, pos, epoch) into a new lineage with its own `user` value (a small integer looked up in a dict); the script
is shared.  ZkProver::prove runs the sumcheck on a clone and then replays the same writes on the original, so a script keyed by
epoch NUMBER applies to both.

The script edits the stream of one epoch; the edits apply in the order given, each offset counted in the stream as the edits
before it left it:
  splice(epoch, at, data)   data is inserted at byte offset `at` (what followed moves back)
  replace(epoch, at, data)  data stands in place of the stream's own bytes at `at`

Every lineage keeps a log of ("w", tag, payload bytes) and ("g", n) events; epochs(user) folds it into one record per epoch, so
that a test finds its epochs from the shapes of the writes and never hard-codes them.

ctypes swallows an exception raised inside a callback: every hook catches its own, keeps the first, and check() raises it."""
import ctypes as C
import hashlib
import struct

from fs_transcript import Transcript as _RefTranscript

ROOT_USER = 1  # the `user` value of the lineage a ScriptedTranscript starts with


class _Lineage:
    def __init__(self, key, pos, epoch):
        self.key, self.pos, self.epoch = key, pos, epoch
        self.first_epoch = epoch
        self.log = []
        self.freed = False
        self._cache = (None, b"")  # (key the bytes belong to, the edited stream's known prefix)


class ScriptedTranscript:
    def __init__(self, seed):
        seed = seed if isinstance(seed, (bytes, bytearray)) else struct.pack("<Q", seed)
        self.lineages = {ROOT_USER: _Lineage(hashlib.sha256(b"scripted transcript" + bytes(seed)).digest(), 0, 0)}
        self._next_user = ROOT_USER + 1
        self.script = {}  # epoch -> [(kind, at, data)]
        self.errors = []
        self._make_hooks()

    # ------------------------------------------------------------ the script
    def splice(self, epoch, at, data):
        self.script.setdefault(epoch, []).append(("splice", at, bytes(data)))
        self._drop_caches()

    def replace(self, epoch, at, data):
        self.script.setdefault(epoch, []).append(("replace", at, bytes(data)))
        self._drop_caches()

    def _drop_caches(self):
        for ln in self.lineages.values():
            ln._cache = (None, b"")

    # ------------------------------------------------------------ the stream of an epoch
    def _stream(self, ln, need):
        """the first `need` bytes (at least) of the current epoch's stream, script applied"""
        key, have = ln._cache
        if key == ln.key and len(have) >= need:
            return have
        edits = self.script.get(ln.epoch, [])
        want = max([2 * need, 64] + [at + len(d) for _, at, d in edits])
        s = bytearray()
        for ctr in range((want + 31) // 32):
            s += hashlib.sha256(ln.key + struct.pack("<Q", ctr)).digest()
        for kind, at, d in edits:
            if kind == "splice":
                s[at:at] = d
            else:
                s[at:at + len(d)] = d
        ln._cache = (ln.key, bytes(s))
        return ln._cache[1]

    # ------------------------------------------------------------ the operations, on a lineage
    def _write(self, user, tag, count, nbytes):
        ln = self._lineage(user)
        ln.key = hashlib.sha256(ln.key + bytes([tag]) + struct.pack("<QQ", count, nbytes)).digest()
        ln.pos = 0
        ln.epoch += 1
        ln.log.append(("w", tag, nbytes))

    def _gen(self, user, n):
        ln = self._lineage(user)
        out = self._stream(ln, ln.pos + n)[ln.pos:ln.pos + n]
        ln.pos += n
        ln.log.append(("g", n))
        return out

    def _clone(self, user):
        src = self._lineage(user)
        new = self._next_user
        self._next_user += 1
        self.lineages[new] = _Lineage(src.key, src.pos, src.epoch)
        return new

    def _free(self, user):
        ln = self._lineage(user)
        if user == ROOT_USER:
            raise ValueError("free_clone of the original transcript")
        ln.freed = True  # the log stays readable

    def _lineage(self, user):
        ln = self.lineages.get(user)
        if ln is None:
            raise KeyError("transcript hook called with an unknown user value %r" % (user,))
        if ln.freed:
            raise ValueError("transcript hook called on a freed clone (user %r)" % (user,))
        return ln

    # ------------------------------------------------------------ the caller's side (the original lineage), as fs_transcript.Transcript
    def write_bytes(self, data):
        self._write(ROOT_USER, 0, len(data), len(data))

    def write_elt(self, e):
        self._write(ROOT_USER, 1, 1, len(e))

    def write_array(self, elts):
        self._write(ROOT_USER, 2, len(elts), sum(len(e) for e in elts))

    def bytes(self, n):
        return self._gen(ROOT_USER, n)

    nat = _RefTranscript.nat  # RandomEngine::nat and choose over self.bytes
    choose = _RefTranscript.choose

    def clone(self):
        """-> the `user` value of a copy of the original lineage"""
        return self._clone(ROOT_USER)

    # ------------------------------------------------------------ the log
    def log(self, user=ROOT_USER):
        return list(self.lineages[user].log)

    def epochs(self, user=ROOT_USER):
        """the lineage's log by epoch: [dict(epoch, write=(tag, payload bytes) or None for the epoch it started in, draws=[n, ...])]"""
        ln = self.lineages[user]
        out = [dict(epoch=ln.first_epoch, write=None, draws=[])]
        for ev in ln.log:
            if ev[0] == "w":
                out.append(dict(epoch=out[-1]["epoch"] + 1, write=(ev[1], ev[2]), draws=[]))
            else:
                out[-1]["draws"].append(ev[1])
        return out

    def clones(self):
        """the `user` values of the clones, in the order they were made"""
        return sorted(u for u in self.lineages if u != ROOT_USER)

    # ------------------------------------------------------------ the hooks
    def _guard(self, fn, on_error=None):
        def hook(*a):
            try:
                return fn(*a)
            except BaseException as e:  # noqa: B036 -- nothing may escape into the C caller
                self.errors.append(e)
                return on_error
        return hook

    def _make_hooks(self):
        vp, sz = C.c_void_p, C.c_size_t

        def gen_bytes(user, out, n):
            C.memset(out, 0, n)  # what the caller sees if the hook fails below
            C.memmove(out, self._gen(user, n), n)

        g = self._guard
        self._fns = dict(
            write_bytes=C.CFUNCTYPE(None, vp, vp, sz)(g(lambda u, _d, n: self._write(u, 0, n, n))),
            write_elt=C.CFUNCTYPE(None, vp, vp)(g(lambda u, _e: self._write(u, 1, 1, 16))),
            write_elt_array=C.CFUNCTYPE(None, vp, vp, sz)(g(lambda u, _e, n: self._write(u, 2, n, 16 * n))),
            gen_bytes=C.CFUNCTYPE(None, vp, vp, sz)(g(gen_bytes)),
            clone=C.CFUNCTYPE(vp, vp)(g(self._clone, on_error=None)),
            free_clone=C.CFUNCTYPE(None, vp)(g(self._free)),
            write_elt_sized=C.CFUNCTYPE(None, vp, vp, sz)(g(lambda u, _e, nb: self._write(u, 1, 1, nb))),
            write_elt_array_sized=C.CFUNCTYPE(None, vp, vp, sz, sz)(g(lambda u, _e, n, nb: self._write(u, 2, n, n * nb))),
        )

    HOOKS = ("write_bytes", "write_elt", "write_elt_array", "gen_bytes", "clone", "free_clone", "write_elt_sized", "write_elt_array_sized")

    def hook(self, name):
        """the ctypes function object behind a hook: calling it goes through the C thunk, as the library's call does"""
        return self._fns[name]

    def ops(self):
        """lfgpu_transcript_ops over the original lineage"""
        from __graft_entry__ import load_package
        return load_package().TranscriptOps(ROOT_USER, *[C.cast(self._fns[n], C.c_void_p) for n in self.HOOKS])

    def check(self):
        """raise the first exception that a hook swallowed"""
        if self.errors:
            raise self.errors[0]
