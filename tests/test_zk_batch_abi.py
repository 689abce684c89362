"""lfgpu_zk_batch_new / lfgpu_zk_prove_batch / lfgpu_zk_batch_free and lfgpu_eval_quad_batch at the boundary, without a
device: the symbols, their declarations, the Python mirror, the argument checks that need no context, and the C++ example's
build."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build, load_package

LIBDIR = os.path.join(ROOT, "longfellow-zk_amd")
LIB = os.path.join(LIBDIR, "liblfgpu.so")
SYMBOLS = ("lfgpu_zk_batch_new", "lfgpu_zk_prove_batch", "lfgpu_zk_batch_free", "lfgpu_eval_quad_batch")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("liblfgpu.so not built and no hipcc")
        build()
    return load_package()


def build_example():
    """examples/zk_prove_batch.cc -> examples/zk_prove_batch, as tests/test_cxx_example.py builds zk_flatsha"""
    src = os.path.join(ROOT, "examples", "zk_prove_batch.cc")
    exe = os.path.join(ROOT, "examples", "zk_prove_batch")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(LIB)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + LIBDIR, "-llfgpu",
                               "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_library_exports_the_batch_entry_points(pkg):
    L = C.CDLL(LIB)
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_headers_declare_them():
    zk = open(os.path.join(ROOT, "include", "lfgpu_zk.h")).read()
    assert re.search(r"typedef\s+struct\s+lfgpu_zk_batch\s+lfgpu_zk_batch\s*;", zk)
    assert re.search(r"\bint\s+lfgpu_zk_batch_new\s*\(\s*lfgpu_ctx\s*\*\s*\w*\s*,\s*const\s+lfgpu_circuit\s*\*\s*\w*\s*,\s*size_t\s+nb_max\s*,\s*lfgpu_zk_batch\s*\*\*\s*out\s*\)", zk)
    assert re.search(r"\bint\s+lfgpu_zk_prove_batch\s*\(\s*lfgpu_zk_batch\s*\*\s*\w*\s*,\s*lfgpu_zk_prover\s*\*\s*const\s*\*\s*zk\s*,\s*size_t\s+nb\s*,"
                     r"\s*const\s+void\s*\*\s*const\s*\*\s*h_W\s*,\s*const\s+lfgpu_transcript_ops\s*\*\s*const\s*\*\s*ts\s*,\s*int\s*\*\s*ok", zk)
    assert re.search(r"\bint\s+lfgpu_zk_batch_free\s*\(\s*lfgpu_zk_batch\s*\*", zk)
    # the two documented properties of the timings and of the threading model
    assert "same values for every member" in zk and "single-threaded per call" in zk
    k = open(os.path.join(ROOT, "include", "lfgpu.h")).read()
    assert re.search(r"\bint\s+lfgpu_eval_quad_batch\s*\(\s*lfgpu_quad\s*\*\s*q\s*,\s*size_t\s+nb\s*,\s*size_t\s+nw\s*,\s*const\s+void\s*\*\s*d_W\s*,\s*size_t\s+ldw\s*,"
                     r"\s*void\s*\*\s*d_V\s*,\s*size_t\s+ldv\s*,\s*int\s*\*\s*ok_out", k)


def test_python_mirror_names_them(pkg):
    for name in SYMBOLS:
        assert name in pkg.ABI_SYMBOLS, name
    L = pkg.load_library()
    assert L.lfgpu_zk_batch_new.restype is C.c_int and len(L.lfgpu_zk_batch_new.argtypes) == 4
    assert L.lfgpu_zk_prove_batch.restype is C.c_int and len(L.lfgpu_zk_prove_batch.argtypes) == 6
    assert len(L.lfgpu_zk_batch_free.argtypes) == 1 and len(L.lfgpu_eval_quad_batch.argtypes) == 8
    assert callable(getattr(pkg.ZkBatch, "prove")) and callable(getattr(pkg.ZkBatch, "close"))
    assert callable(getattr(pkg.Quad, "eval_batch"))


def test_null_arguments_are_argument_errors_without_a_device(pkg):
    L = pkg.load_library()
    out = C.c_void_p()
    ok = (C.c_int * 2)()
    assert L.lfgpu_zk_batch_new(None, None, 2, C.byref(out)) == 1  # LFGPU_ERR_ARG
    assert out.value is None
    assert L.lfgpu_zk_prove_batch(None, None, 1, None, None, ok) == 1
    assert L.lfgpu_zk_batch_free(None) == 1
    assert L.lfgpu_eval_quad_batch(None, 2, 4, None, 4, None, 4, ok) == 1


def test_cxx_example_compiles_and_fails_loudly_without_gpu(pkg):
    exe = build_example()
    import torch
    if torch.cuda.is_available():
        return  # with a device the example runs: tests/test_zk_prove_batch.py
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "nonexistent.lfc1"), "w.bin", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
