"""The Fp256Base sumcheck layer (lfgpu_sumcheck_layer256, lfgpu_sumcheck_layer_batch256, lfgpu_eval_quad_batch256) at the
boundary, without a device: the symbols, their declarations, the Python mirror, the argument check that needs no context,
and the C++ example's build."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build, load_package

LIBDIR = os.path.join(ROOT, "longfellow-zk_amd")
LIB = os.path.join(LIBDIR, "liblfgpu.so")
NAMES = ("lfgpu_sumcheck_layer256", "lfgpu_sumcheck_layer_batch256", "lfgpu_eval_quad_batch256")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("liblfgpu.so not built and no hipcc")
        build()
    return load_package()


def build_example():
    """examples/sumcheck_layer_batch256.cc -> examples/sumcheck_layer_batch256, with plain g++ against the header"""
    src = os.path.join(ROOT, "examples", "sumcheck_layer_batch256.cc")
    exe = os.path.join(ROOT, "examples", "sumcheck_layer_batch256")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(LIB)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + LIBDIR, "-llfgpu",
                               "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_library_exports_the_three_entry_points(pkg):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name


def test_header_declares_them_and_the_callbacks():
    hdr = open(os.path.join(ROOT, "include", "lfgpu.h")).read()
    assert re.search(r"\bint\s+lfgpu_sumcheck_layer256\s*\(\s*lfgpu_quad\s*\*\s*q\s*,\s*size_t\s+logv\s*,", hdr)
    assert re.search(r"\bint\s+lfgpu_sumcheck_layer_batch256\s*\(\s*lfgpu_quad\s*\*\s*q\s*,\s*size_t\s+nb\s*,", hdr)
    assert re.search(r"\bint\s+lfgpu_eval_quad_batch256\s*\(\s*lfgpu_quad\s*\*\s*q\s*,\s*size_t\s+nb\s*,", hdr)
    assert re.search(r"typedef\s+void\s*\(\s*\*\s*lfgpu_sc_round256_fn\s*\)", hdr)
    assert re.search(r"typedef\s+void\s*\(\s*\*\s*lfgpu_sc_round_batch256_fn\s*\)", hdr)
    m = re.search(r"^#define\s+LFGPU_P256_BATCH_SMALL_MAX\s+(\d+)\b", hdr, re.M)
    assert m and int(m.group(1)) == load_package().P256_BATCH_SMALL_MAX
    # the wires are left intact, unlike the 16-byte call: the header says so
    assert "LEFT INTACT" in hdr


def test_python_mirror_names_them(pkg):
    for name in NAMES:
        assert name in pkg.ABI_SYMBOLS
    L = pkg.load_library()
    fn = L.lfgpu_sumcheck_layer256
    assert fn.restype is C.c_int and len(fn.argtypes) == 15 and fn.argtypes[10] is pkg.SC_ROUND256_FN
    fn = L.lfgpu_sumcheck_layer_batch256
    assert fn.restype is C.c_int and len(fn.argtypes) == 17 and fn.argtypes[12] is pkg.SC_ROUND_BATCH256_FN
    fn = L.lfgpu_eval_quad_batch256
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    for m in ("sumcheck_layer256", "sumcheck_layer_batch256", "eval_quad_batch256"):
        assert callable(getattr(pkg.Quad, m))


def test_null_quad_is_an_argument_error_without_a_device(pkg):
    L = pkg.load_library()
    z4, z8 = (C.c_uint64 * 4)(), (C.c_uint64 * 8)()
    ok = (C.c_int * 1)()
    assert L.lfgpu_sumcheck_layer256(None, 0, None, None, z4, z4, 1, 2, None, z8, pkg.SC_ROUND256_FN(lambda *a: None), None, z8, z8, z4) == 1  # LFGPU_ERR_ARG
    assert L.lfgpu_sumcheck_layer_batch256(None, 1, 0, None, None, z4, z4, 1, 2, None, 2, z8, pkg.SC_ROUND_BATCH256_FN(lambda *a: None), None, z8, z8, z4) == 1
    assert L.lfgpu_eval_quad_batch256(None, 1, 2, None, 2, None, 1, ok) == 1


def test_cxx_example_compiles_and_fails_loudly_without_gpu(pkg):
    exe = build_example()
    import torch
    if torch.cuda.is_available():
        return  # with a device the example runs: tests/test_cxx_sumcheck_batch256.py
    r = subprocess.run([exe, "2", "3", "8", "3", "5", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
