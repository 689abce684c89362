"""lfgpu_column_commit_batch256 / lfgpu_ligero_commit_batch256 / lfgpu_zk_commit_batch256 at the boundary, without a device (the
pattern of test_zk_batch256_abi.py): the symbols, their declarations, the Python mirror, the argument checks that need no
context, and the C++ example's build."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build, load_package

LIBDIR = os.path.join(ROOT, "longfellow-zk_amd")
LIB = os.path.join(LIBDIR, "liblfgpu.so")
SYMBOLS = ("lfgpu_column_commit_batch256", "lfgpu_ligero_commit_batch256", "lfgpu_zk_commit_batch256")
ERR_ARG = 1


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("liblfgpu.so not built and no hipcc")
        build()
    return load_package()


def build_example():
    """examples/zk_commit_batch256.cc -> examples/zk_commit_batch256, by the line in its header"""
    src = os.path.join(ROOT, "examples", "zk_commit_batch256.cc")
    exe = os.path.join(ROOT, "examples", "zk_commit_batch256")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(LIB)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + LIBDIR, "-llfgpu",
                               "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_library_exports_the_three_entry_points(pkg):
    L = C.CDLL(LIB)
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_headers_declare_them():
    k = open(os.path.join(ROOT, "include", "lfgpu.h")).read()
    assert re.search(r"\bint\s+lfgpu_column_commit_batch256\s*\(\s*lfgpu_ctx\s*\*\s*\w*\s*,\s*size_t\s+nrow\s*,\s*size_t\s+ld\s*,\s*size_t\s+col0\s*,"
                     r"\s*size_t\s+ncols\s*,\s*size_t\s+nb\s*,\s*const\s+void\s*\*\s*const\s*\*\s*d_T\s*,\s*const\s+void\s*\*\s*d_nonces\s*,"
                     r"\s*void\s*\*\s*const\s*\*\s*d_layers\s*,\s*uint8_t\s*\*\s*roots_out", k)
    assert re.search(r"\bint\s+lfgpu_ligero_commit_batch256\s*\(\s*lfgpu_ctx\s*\*\s*\w*\s*,\s*const\s+lfgpu_ligero_param\s*\*\s*p\s*,\s*size_t\s+nb\s*,"
                     r"\s*const\s+void\s*\*\s*const\s*\*\s*h_W\s*,\s*const\s+size_t\s*\*\s*h_lqc\s*,\s*const\s+lfgpu_rng_fn\s*\*\s*rng\s*,"
                     r"\s*void\s*\*\s*const\s*\*\s*rng_user\s*,\s*uint8_t\s*\*\s*roots_out[^,]*,\s*lfgpu_ligero_prover\s*\*\*\s*out", k)
    # the documented properties: the draw order of a shared engine, the per-statement fallback, the switch of its own
    assert "LFGPU_COMMIT_BATCH256=0" in k and "draw order of sequential calls" in k
    summary = k[:k.index("typedef struct lfgpu_ctx")]
    assert "lfgpu_ligero_commit_batch256" in summary and "lfgpu_zk_commit_batch256" in summary, "the field's summary names the batched commit"
    assert "Not batched for this field: the commit" not in k
    zk = open(os.path.join(ROOT, "include", "lfgpu_zk.h")).read()
    assert re.search(r"\bint\s+lfgpu_zk_commit_batch256\s*\(\s*lfgpu_zk_batch256\s*\*\s*\w*\s*,\s*lfgpu_zk_prover\s*\*\s*const\s*\*\s*zk\s*,\s*size_t\s+nb\s*,"
                     r"\s*const\s+void\s*\*\s*const\s*\*\s*h_W\s*,\s*const\s+lfgpu_rng_fn\s*\*\s*rng\s*,\s*void\s*\*\s*const\s*\*\s*rng_user\s*,"
                     r"\s*const\s+lfgpu_transcript_ops\s*\*\s*const\s*\*\s*ts\s*,\s*uint8_t\s*\*\s*roots_out", zk)
    assert "LFGPU_COMMIT_BATCH256=0" in zk and "Not batched for this field: the commit" not in zk


def test_python_mirror_names_them(pkg):
    for name in SYMBOLS:
        assert name in pkg.ABI_SYMBOLS, name
    L = pkg.load_library()
    assert L.lfgpu_column_commit_batch256.restype is C.c_int and len(L.lfgpu_column_commit_batch256.argtypes) == 10
    assert L.lfgpu_ligero_commit_batch256.restype is C.c_int and len(L.lfgpu_ligero_commit_batch256.argtypes) == 9
    assert L.lfgpu_zk_commit_batch256.restype is C.c_int and len(L.lfgpu_zk_commit_batch256.argtypes) == 8
    # the twins take what the 16-byte calls take, less the field (and the subfield arguments the field ignores)
    assert len(L.lfgpu_column_commit_batch256.argtypes) == len(L.lfgpu_column_commit_batch.argtypes) - 1
    assert len(L.lfgpu_ligero_commit_batch256.argtypes) == len(L.lfgpu_ligero_commit_batch.argtypes) - 3
    assert len(L.lfgpu_zk_commit_batch256.argtypes) == len(L.lfgpu_zk_commit_batch.argtypes)
    assert callable(getattr(pkg.LfGpu, "column_commit_batch256")) and callable(getattr(pkg.LigeroProver, "commit_batch256"))
    assert callable(getattr(pkg.ZkBatch256, "commit"))


def test_null_arguments_are_argument_errors_without_a_device(pkg):
    L = pkg.load_library()
    roots = (C.c_uint8 * 64)()
    ptrs = (C.c_void_p * 2)()
    assert L.lfgpu_column_commit_batch256(None, 1, 1, 0, 1, 1, ptrs, roots, ptrs, roots) == ERR_ARG
    assert L.lfgpu_ligero_commit_batch256(None, None, 1, None, None, None, None, roots, ptrs) == ERR_ARG
    assert L.lfgpu_zk_commit_batch256(None, None, 1, None, None, None, None, roots) == ERR_ARG


def test_cxx_example_compiles_and_fails_loudly_without_gpu(pkg):
    exe = build_example()
    import torch
    if torch.cuda.is_available():
        return  # with a device the example runs: tests/test_zk_commit_batch256.py
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "nonexistent.lfc1"), "w.bin", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
