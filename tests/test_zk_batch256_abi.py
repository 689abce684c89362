"""lfgpu_zk_batch256_new / lfgpu_zk_prove_batch256 / lfgpu_zk_batch256_free and lfgpu_ligero_prove_batch256 /
lfgpu_ligero_open_batch256 at the boundary, without a device (the pattern of test_zk_batch_abi.py): the symbols, their
declarations, the Python mirror, the argument checks that need no context, and the C++ example's build."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build, load_package

LIBDIR = os.path.join(ROOT, "longfellow-zk_amd")
LIB = os.path.join(LIBDIR, "liblfgpu.so")
ZK_SYMBOLS = ("lfgpu_zk_batch256_new", "lfgpu_zk_prove_batch256", "lfgpu_zk_batch256_free")
LIGERO_SYMBOLS = ("lfgpu_ligero_prove_batch256", "lfgpu_ligero_open_batch256")
ERR_ARG = 1


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("liblfgpu.so not built and no hipcc")
        build()
    return load_package()


def build_example():
    """examples/zk_prove_batch256.cc -> examples/zk_prove_batch256, by the line in its header"""
    src = os.path.join(ROOT, "examples", "zk_prove_batch256.cc")
    exe = os.path.join(ROOT, "examples", "zk_prove_batch256")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(LIB)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + LIBDIR, "-llfgpu",
                               "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_library_exports_the_five_entry_points(pkg):
    L = C.CDLL(LIB)
    for name in ZK_SYMBOLS + LIGERO_SYMBOLS:
        assert hasattr(L, name), name


def test_headers_declare_them():
    ws = r"\s*"
    zk = open(os.path.join(ROOT, "include", "lfgpu_zk.h")).read()
    assert re.search(r"typedef\s+struct\s+lfgpu_zk_batch256\s+lfgpu_zk_batch256\s*;", zk)
    assert re.search(r"\bint\s+lfgpu_zk_batch256_new\s*\(\s*lfgpu_ctx\s*\*\s*\w*\s*,\s*const\s+lfgpu_circuit\s*\*\s*\w*\s*,\s*size_t\s+nb_max\s*,\s*lfgpu_zk_batch256\s*\*\*\s*out\s*\)", zk)
    assert re.search(r"\bint\s+lfgpu_zk_prove_batch256\s*\(\s*lfgpu_zk_batch256\s*\*\s*\w*\s*,\s*lfgpu_zk_prover\s*\*\s*const\s*\*\s*zk\s*,\s*size_t\s+nb\s*,"
                     r"\s*const\s+void\s*\*\s*const\s*\*\s*h_W\s*,\s*const\s+lfgpu_transcript_ops\s*\*\s*const\s*\*\s*ts\s*,\s*int\s*\*\s*ok", zk)
    assert re.search(r"\bint\s+lfgpu_zk_batch256_free\s*\(\s*lfgpu_zk_batch256\s*\*", zk)
    # the refusal of the 16-byte entry points points at the new names, and the switch of the tail is this field's own
    assert "lfgpu_zk_batch256_new / lfgpu_zk_prove_batch256 below" in zk and "LFGPU_LIGERO_PROVE_BATCH256=0" in zk
    k = open(os.path.join(ROOT, "include", "lfgpu.h")).read()
    args = ws.join([r"lfgpu_ctx\s*\*\s*\w*\s*,", r"lfgpu_ligero_prover\s*\*\s*const\s*\*\s*pr\s*,", r"size_t\s+nb\s*,"])
    assert re.search(r"\bint\s+lfgpu_ligero_prove_batch256\s*\(\s*" + args + r"\s*const\s+void\s*\*\s*h_u_ldt\s*,\s*const\s+void\s*\*\s*const\s*\*\s*d_dense\s*,"
                     r"\s*size_t\s+ndense\s*,\s*const\s+uint64_t\s*\*\s*scale[^,]*,\s*const\s+uint64_t\s*\*\s*const\s*\*\s*h_idx\s*,\s*const\s+void\s*\*\s*const\s*\*\s*h_val\s*,"
                     r"\s*const\s+size_t\s*\*\s*nsparse[^,]*,\s*const\s+void\s*\*\s*h_u_quad\s*,\s*void\s*\*\s*h_y_ldt\s*,\s*void\s*\*\s*h_y_dot\s*,\s*void\s*\*\s*h_y_q0\s*,"
                     r"\s*void\s*\*\s*h_y_q2\s*\)", k)
    assert re.search(r"\bint\s+lfgpu_ligero_open_batch256\s*\(\s*" + args + r"\s*const\s+size_t\s*\*\s*idx[^,]*,\s*void\s*\*\s*h_req\s*,\s*uint8_t\s*\*\s*h_nonces\s*,"
                     r"\s*uint8_t\s*\*\s*h_path\s*,\s*size_t\s+path_cap\s*,\s*size_t\s*\*\s*npath", k)
    assert "lfgpu_ligero_prove_batch256" in k[:k.index("typedef struct lfgpu_ctx")], "the field's summary names the batch entry points"


def test_python_mirror_names_them(pkg):
    for name in ZK_SYMBOLS + LIGERO_SYMBOLS:
        assert name in pkg.ABI_SYMBOLS, name
    L = pkg.load_library()
    assert L.lfgpu_zk_batch256_new.restype is C.c_int and len(L.lfgpu_zk_batch256_new.argtypes) == 4
    assert L.lfgpu_zk_prove_batch256.restype is C.c_int and len(L.lfgpu_zk_prove_batch256.argtypes) == 6
    assert len(L.lfgpu_zk_batch256_free.argtypes) == 1
    assert L.lfgpu_ligero_prove_batch256.restype is C.c_int and len(L.lfgpu_ligero_prove_batch256.argtypes) == 15
    assert L.lfgpu_ligero_open_batch256.restype is C.c_int and len(L.lfgpu_ligero_open_batch256.argtypes) == 9
    # the twins take what the 16-byte calls take
    assert len(L.lfgpu_ligero_prove_batch256.argtypes) == len(L.lfgpu_ligero_prove_batch.argtypes)
    assert len(L.lfgpu_ligero_open_batch256.argtypes) == len(L.lfgpu_ligero_open_batch.argtypes)
    assert callable(getattr(pkg.ZkBatch256, "prove")) and callable(getattr(pkg.ZkBatch256, "close"))
    assert callable(getattr(pkg.LigeroProver, "prove_batch256")) and callable(getattr(pkg.LigeroProver, "open_batch256"))


def test_null_arguments_are_argument_errors_without_a_device(pkg):
    L = pkg.load_library()
    out = C.c_void_p()
    ok = (C.c_int * 2)()
    assert L.lfgpu_zk_batch256_new(None, None, 2, C.byref(out)) == ERR_ARG
    assert out.value is None
    assert L.lfgpu_zk_prove_batch256(None, None, 1, None, None, ok) == ERR_ARG
    assert L.lfgpu_zk_batch256_free(None) == ERR_ARG
    buf = (C.c_uint8 * 64)()
    nsp = (C.c_size_t * 1)(0)
    npath = (C.c_size_t * 1)(0)
    idx = (C.c_size_t * 1)(0)
    assert L.lfgpu_ligero_prove_batch256(None, None, 1, buf, None, 0, None, None, None, nsp, buf, buf, buf, buf, buf) == ERR_ARG
    assert L.lfgpu_ligero_open_batch256(None, None, 1, idx, buf, buf, buf, 1, npath) == ERR_ARG


def test_cxx_example_compiles_and_fails_loudly_without_gpu(pkg):
    exe = build_example()
    import torch
    if torch.cuda.is_available():
        return  # with a device the example runs: tests/test_zk_prove_batch256.py
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "nonexistent.lfc1"), "w.bin", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
