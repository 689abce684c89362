"""The Ligero section of the wire format on the host: zkp::com_proof_read / com_proof_write (csrc/zk_proto.h), the pair that
lfgpu_ligero_prove / lfgpu_ligero_verify and ZkProof::write / read share, compiled without device code
(tests/host_ligero_wire.hip) and run on the reference's own known-answer proof (tests/golden/ligero_test_vector.bin:
LigeroParam(1000, 50, rateinv 4, nreq 36, block_enc 4096) over GF2_128<4>).  No GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import __graft_entry__ as ge
import ligero_fixture as lf
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostligerowire.so")
SRC = os.path.join(HERE, "host_ligero_wire.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
GF = 4
PROOF_LEN = 55768

_state = None


def _setup():
    """(harness, package, vector, LigeroParam of the vector)"""
    global _state
    if _state is None:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        if not os.path.exists(ge.LIB):
            ge.build()
        pkg = ge.load_package()
        pkg.load_library()
        csrc = os.path.join(ol.ROOT, "longfellow-zk_amd", "csrc")
        deps = [SRC, ge.LIB] + [os.path.join(csrc, h) for h in ("zk_proto.h", "hostfield.h", "fp256.h", "fields.h", "ctx.h", "zkint.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC, "-L" + os.path.dirname(ge.LIB),
                                   "-l:" + os.path.basename(ge.LIB), "-Wl,-rpath," + os.path.dirname(ge.LIB)])
        v = lf.load()
        p = pkg.ligero_param(GF, v["nw"], v["nq"], 4, v["nreq"], 4096)
        _state = (C.CDLL(SO), pkg, v, p)
    return _state


def _roundtrip(L, p, data):
    """-> (status, bytes written again, npath, run lengths)"""
    out = C.create_string_buffer(len(data) + 64)
    nbytes, npath, nruns = C.c_size_t(), C.c_size_t(), C.c_size_t()
    runs = (C.c_size_t * 16)()
    rc = L.hlw_roundtrip(C.c_int(GF), C.c_int(4), C.byref(p), bytes(data), C.c_size_t(len(data)), out, C.c_size_t(len(out)), C.byref(nbytes), C.byref(npath),
                         runs, C.c_size_t(16), C.byref(nruns))
    return rc, out.raw[:nbytes.value], npath.value, list(runs[:min(nruns.value, 16)])


def test_vector_layout_by_hand():
    """the committed proof IS the write_com_proof layout: parsed here with struct alone, no code of ours"""
    _, _, v, p = _setup()
    d = v["proof"]
    assert len(d) == PROOF_LEN
    assert (p.block, p.dblock, p.r, p.dblock - p.block, p.nrow) == (682, 1363, 36, 681, 8)
    off = 16 * (682 + 1363 + 36 + 681) + 32 * 36
    runs = []
    for width in (16, 2, 16):
        (n,) = struct.unpack_from("<I", d, off)
        runs.append(n)
        off += 4 + n * width
    assert runs == [108, 36, 144] and sum(runs) == p.nreq * p.nrow
    (npath,) = struct.unpack_from("<I", d, off)
    assert npath == 197
    assert off + 4 + 32 * npath == len(d)


def test_com_proof_read_write_roundtrip():
    L, _, v, p = _setup()
    rc, again, npath, runs = _roundtrip(L, p, v["proof"])
    assert rc == 1
    assert len(again) == PROOF_LEN and again == v["proof"]
    assert runs == [108, 36, 144]
    assert npath == 197


def test_truncated_and_overlong_do_not_parse():
    L, _, v, p = _setup()
    d = v["proof"]
    for bad in (d[:-1], d + b"\x00", d[:-32], d[:16 * 682], b"", d + d):
        assert _roundtrip(L, p, bad)[0] == 0, len(bad)
    # a run length that overshoots the nreq * nrow opened elements
    off = 16 * (682 + 1363 + 36 + 681) + 32 * 36
    assert _roundtrip(L, p, d[:off] + struct.pack("<I", 289) + d[off + 4:])[0] == 0
    # a path shorter than nreq digests
    tail = len(d) - 4 - 32 * 197
    assert _roundtrip(L, p, d[:tail] + struct.pack("<I", 35) + d[tail + 4:tail + 4 + 32 * 35])[0] == 0
