"""lfgpu_sumcheck_layer_batch (K14, the batch axis of the sumcheck layer) at the boundary, without a device: the symbol, its
declaration, the Python mirror, the argument check that needs no context, and the C++ example's build."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build, load_package

LIBDIR = os.path.join(ROOT, "longfellow-zk_amd")
LIB = os.path.join(LIBDIR, "liblfgpu.so")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("liblfgpu.so not built and no hipcc")
        build()
    return load_package()


def build_example():
    """examples/sumcheck_layer_batch.cc -> examples/sumcheck_layer_batch, as tests/test_cxx_example.py builds zk_flatsha"""
    src = os.path.join(ROOT, "examples", "sumcheck_layer_batch.cc")
    exe = os.path.join(ROOT, "examples", "sumcheck_layer_batch")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(LIB)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + LIBDIR, "-llfgpu",
                               "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_library_exports_the_batched_layer(pkg):
    L = pkg.load_library()
    assert hasattr(L, "lfgpu_sumcheck_layer_batch")


def test_header_declares_it_and_the_cap():
    hdr = open(os.path.join(ROOT, "include", "lfgpu.h")).read()
    assert re.search(r"^#define\s+LFGPU_SC_BATCH_MAX\s+64\b", hdr, re.M)
    assert re.search(r"\bint\s+lfgpu_sumcheck_layer_batch\s*\(\s*lfgpu_quad\s*\*\s*q\s*,\s*size_t\s+nb\s*,", hdr)
    assert re.search(r"typedef\s+void\s*\(\s*\*\s*lfgpu_sc_round_batch_fn\s*\)", hdr)


def test_python_mirror_names_it(pkg):
    assert "lfgpu_sumcheck_layer_batch" in pkg.ABI_SYMBOLS
    L = pkg.load_library()
    fn = L.lfgpu_sumcheck_layer_batch
    assert fn.restype is C.c_int and len(fn.argtypes) == 17 and fn.argtypes[12] is pkg.SC_ROUND_BATCH_FN
    assert pkg.SC_BATCH_MAX == 64
    assert callable(getattr(pkg.Quad, "sumcheck_layer_batch"))


def test_null_quad_is_an_argument_error_without_a_device(pkg):
    L = pkg.load_library()
    z2, z4 = (C.c_uint64 * 2)(), (C.c_uint64 * 4)()
    cb = pkg.SC_ROUND_BATCH_FN(lambda *a: None)
    rc = L.lfgpu_sumcheck_layer_batch(None, 1, 0, None, None, z2, z2, 1, 2, None, 2, z4, cb, None, z4, z4, z2)
    assert rc == 1  # LFGPU_ERR_ARG


def test_cxx_example_compiles_and_fails_loudly_without_gpu(pkg):
    exe = build_example()
    import torch
    if torch.cuda.is_available():
        return  # with a device the example runs: tests/test_cxx_sumcheck_batch.py
    r = subprocess.run([exe, "gf", "2", "3", "8", "3", "5", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
