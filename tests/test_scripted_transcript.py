"""tests/scripted_transcript.py on its own (no GPU, no library): the hooks are called through their ctypes function objects,
the way the library calls them."""
import ctypes as C
import hashlib
import struct

import pytest

from scripted_transcript import ROOT_USER, ScriptedTranscript


def gen(ts, n, user=ROOT_USER):
    buf = C.create_string_buffer(n)
    ts.hook("gen_bytes")(user, C.cast(buf, C.c_void_p), n)
    return buf.raw


def write_bytes(ts, data, user=ROOT_USER):
    buf = C.create_string_buffer(bytes(data), len(data))
    ts.hook("write_bytes")(user, C.cast(buf, C.c_void_p), len(data))


def base_stream(key, n):
    return b"".join(hashlib.sha256(key + struct.pack("<Q", i)).digest() for i in range((n + 31) // 32))[:n]


def test_same_seed_same_bytes():
    a, b, c = ScriptedTranscript(7), ScriptedTranscript(7), ScriptedTranscript(8)
    for ts in (a, b, c):
        write_bytes(ts, b"x" * 32)
    got = [gen(ts, 16) + gen(ts, 1) + gen(ts, 50) for ts in (a, b, c)]
    assert got[0] == got[1] and got[0] != got[2]
    assert len(got[0]) == 67
    # reads of any split are one stream: SHA-256(key || u64 counter) blocks of the lineage's key
    d = ScriptedTranscript(7)
    write_bytes(d, b"y" * 32)
    assert gen(d, 67) == got[0] == base_stream(d.lineages[ROOT_USER].key, 67)
    assert d.bytes(5) == a.bytes(5)  # the Python-side read is the same stream
    for ts in (a, b, c, d):
        ts.check()


def test_a_write_rekeys_by_shape_only():
    def after(*writes):
        ts = ScriptedTranscript(b"seed")
        first = gen(ts, 40)
        for w in writes:
            w(ts)
        out = gen(ts, 40)
        ts.check()
        return first, out

    e16, e32 = C.create_string_buffer(16), C.create_string_buffer(32)
    ptr = lambda b: C.cast(b, C.c_void_p)  # noqa: E731
    first, a = after(lambda ts: write_bytes(ts, b"a" * 20))
    assert a != first  # a write changes the stream, and restarts it
    assert after(lambda ts: write_bytes(ts, b"b" * 20))[1] == a  # another payload of the same length does not
    assert after(lambda ts: write_bytes(ts, b"a" * 21))[1] != a  # another length does
    elt = after(lambda ts: ts.hook("write_elt")(ROOT_USER, ptr(e16)))[1]
    arr1 = after(lambda ts: ts.hook("write_elt_array")(ROOT_USER, ptr(e16), 1))[1]
    sized16 = after(lambda ts: ts.hook("write_elt_sized")(ROOT_USER, ptr(e16), 16))[1]
    sized32 = after(lambda ts: ts.hook("write_elt_sized")(ROOT_USER, ptr(e32), 32))[1]
    arr_sized = after(lambda ts: ts.hook("write_elt_array_sized")(ROOT_USER, ptr(e16), 1, 16))[1]
    bytes16 = after(lambda ts: write_bytes(ts, b"\0" * 16))[1]
    assert len({elt, arr1, bytes16}) == 3  # the tag tells 16 bytes, one element and an array of one apart
    assert sized16 == elt and arr_sized == arr1 and sized32 != elt  # the sized hooks are the same writes at another width
    # the order of two writes matters
    w1, w2 = (lambda ts: write_bytes(ts, b"a" * 3)), (lambda ts: write_bytes(ts, b"a" * 4))
    assert after(w1, w2)[1] != after(w2, w1)[1]


def test_log_and_epochs():
    ts = ScriptedTranscript(1)
    gen(ts, 3)
    write_bytes(ts, b"r" * 32)
    gen(ts, 16)
    gen(ts, 16)
    ts.write_array([b"e" * 16] * 5)
    ts.write_elt(b"e" * 32)
    ts.bytes(2)
    assert ts.log() == [("g", 3), ("w", 0, 32), ("g", 16), ("g", 16), ("w", 2, 80), ("w", 1, 32), ("g", 2)]
    assert ts.epochs() == [dict(epoch=0, write=None, draws=[3]), dict(epoch=1, write=(0, 32), draws=[16, 16]),
                           dict(epoch=2, write=(2, 80), draws=[]), dict(epoch=3, write=(1, 32), draws=[2])]
    ts.check()


def test_clone_is_independent_and_replays():
    ts = ScriptedTranscript(3)
    ts.splice(2, 5, b"SPLICE")
    write_bytes(ts, b"a" * 8)
    head = gen(ts, 7)
    cl = ts.hook("clone")(ROOT_USER)
    assert cl not in (None, 0, ROOT_USER) and ts.clones() == [cl]
    assert ts.hook("clone")(ROOT_USER) not in (None, 0, ROOT_USER, cl)
    # the clone goes on where the original stood (position included) and does not move it
    c1 = gen(ts, 9, cl)
    write_bytes(ts, b"b" * 4, cl)
    c2 = gen(ts, 20, cl)
    o1 = gen(ts, 9)
    assert o1 == c1 and head + o1 == base_stream(ts.lineages[ROOT_USER].key, 16)
    # the same writes replayed on the original give the same challenges, the script (keyed by epoch number) included
    write_bytes(ts, b"c" * 4)
    assert gen(ts, 20) == c2 and c2[5:11] == b"SPLICE"
    assert ts.epochs(cl) == [dict(epoch=1, write=None, draws=[9]), dict(epoch=2, write=(0, 4), draws=[20])]
    ts.hook("free_clone")(cl)
    assert ts.log(cl) == [("g", 9), ("w", 0, 4), ("g", 20)]  # a freed clone's log stays
    ts.check()


@pytest.mark.parametrize("at,n", [(0, 16), (7, 16), (32, 16), (20, 40), (31, 2), (64, 1)])
def test_splice_and_replace_at_block_boundaries(at, n):
    """offsets that are no multiple of 32, and data that spans two (20 + 40: three) SHA blocks"""
    data = bytes(range(100, 100 + n))
    plain = ScriptedTranscript(5)
    write_bytes(plain, b"w")
    base = gen(plain, 200)
    assert base == base_stream(plain.lineages[ROOT_USER].key, 200)
    sp, rp, other = ScriptedTranscript(5), ScriptedTranscript(5), ScriptedTranscript(5)
    sp.splice(1, at, data)
    rp.replace(1, at, data)
    other.splice(2, at, data)  # another epoch's script
    other.replace(0, at, data)
    head = [gen(ts, 4) for ts in (sp, rp, other)]  # epoch 0, unscripted for sp and rp
    assert head[0] == head[1] == gen(ScriptedTranscript(5), 4)
    assert head[2] == (data + b"\0" * 4)[:4] if at == 0 else head[2] == head[0]
    for ts in (sp, rp, other):
        write_bytes(ts, b"w")
    # read in pieces that straddle the edit
    assert gen(sp, at) + gen(sp, 3) + gen(sp, 197 - at) == (base[:at] + data + base[at:])[:200]
    assert gen(rp, at + 1) + gen(rp, 199 - at) == base[:at] + data + base[at + n:]
    assert gen(other, 200) == base
    for ts in (plain, sp, rp, other):
        ts.check()


def test_edits_apply_in_order():
    ts = ScriptedTranscript(9)
    ts.splice(0, 16, b"B" * 16)
    ts.splice(0, 0, b"A" * 16)  # counted in the stream the first splice left: the first now sits at 32
    ts.replace(0, 48, b"C" * 2)
    base = base_stream(ts.lineages[ROOT_USER].key, 100)
    assert gen(ts, 80) == (b"A" * 16 + base[:16] + b"B" * 16 + b"CC" + base[18:])[:80]
    ts.check()


def test_nat_and_choose_read_the_scripted_stream():
    ts = ScriptedTranscript(2)
    ts.replace(0, 0, (0).to_bytes(2, "little") + (298).to_bytes(2, "little"))
    idx = ts.choose(300, 4)
    assert idx[:2] == [0, 299] and len(set(idx)) == 4 and all(0 <= i < 300 for i in idx)
    ts.check()


def test_a_raising_hook_is_reported():
    ts = ScriptedTranscript(4)
    buf = C.create_string_buffer(b"\xaa" * 8, 8)
    ts.hook("gen_bytes")(77, C.cast(buf, C.c_void_p), 8)  # no such lineage: nothing reaches the caller but zeros
    assert buf.raw == b"\0" * 8
    with pytest.raises(KeyError, match="unknown user value"):
        ts.check()
    ts = ScriptedTranscript(4)
    assert ts.hook("clone")(55) is None  # NULL: the library reports it
    with pytest.raises(KeyError):
        ts.check()
    ts = ScriptedTranscript(4)
    cl = ts.hook("clone")(ROOT_USER)
    ts.hook("free_clone")(cl)
    ts.check()
    ts.hook("write_elt")(cl, None)  # use after free
    ts.hook("free_clone")(ROOT_USER)
    with pytest.raises(ValueError, match="freed clone"):
        ts.check()


def test_ops_table():
    ts = ScriptedTranscript(0)
    o = ts.ops()
    assert o.user == ROOT_USER
    for name in ScriptedTranscript.HOOKS:
        assert getattr(o, name) == C.cast(ts.hook(name), C.c_void_p).value != 0
    # through the table, as C would call it
    fn = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)(o.gen_bytes)
    buf = C.create_string_buffer(8)
    fn(o.user, C.cast(buf, C.c_void_p), 8)
    assert buf.raw == base_stream(ts.lineages[ROOT_USER].key, 8)
    ts.check()
