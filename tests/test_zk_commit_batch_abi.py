"""lfgpu_column_commit_batch / lfgpu_ligero_commit_batch / lfgpu_zk_commit_batch at the boundary, without a device: the
symbols, their declarations, the Python mirror, the argument checks that need no context, and the C++ example's build."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build, load_package

LIBDIR = os.path.join(ROOT, "longfellow-zk_amd")
LIB = os.path.join(LIBDIR, "liblfgpu.so")
SYMBOLS = ("lfgpu_column_commit_batch", "lfgpu_ligero_commit_batch", "lfgpu_zk_commit_batch")


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(LIB):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("liblfgpu.so not built and no hipcc")
        build()
    return load_package()


def build_example():
    """examples/zk_commit_batch.cc -> examples/zk_commit_batch, as tests/test_zk_batch_abi.py builds its sibling"""
    src = os.path.join(ROOT, "examples", "zk_commit_batch.cc")
    exe = os.path.join(ROOT, "examples", "zk_commit_batch")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(LIB)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + LIBDIR, "-llfgpu",
                               "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_library_exports_the_commit_batch_entry_points(pkg):
    L = C.CDLL(LIB)
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_headers_declare_them():
    k = open(os.path.join(ROOT, "include", "lfgpu.h")).read()
    assert re.search(r"\bint\s+lfgpu_column_commit_batch\s*\(\s*lfgpu_ctx\s*\*\s*\w*\s*,\s*int\s+field\s*,\s*size_t\s+nrow\s*,\s*size_t\s+ld\s*,\s*size_t\s+col0\s*,"
                     r"\s*size_t\s+ncols\s*,\s*size_t\s+nb\s*,\s*const\s+void\s*\*\s*const\s*\*\s*d_T\s*,\s*const\s+void\s*\*\s*d_nonces\s*,"
                     r"\s*void\s*\*\s*const\s*\*\s*d_layers\s*,\s*uint8_t\s*\*\s*roots_out", k)
    assert re.search(r"\bint\s+lfgpu_ligero_commit_batch\s*\(\s*lfgpu_ctx\s*\*\s*\w*\s*,\s*int\s+field\s*,\s*int\s+subfield_log_bits\s*,"
                     r"\s*const\s+lfgpu_ligero_param\s*\*\s*p\s*,\s*size_t\s+nb\s*,\s*const\s+void\s*\*\s*const\s*\*\s*h_W\s*,\s*size_t\s+subfield_boundary\s*,"
                     r"\s*const\s+size_t\s*\*\s*h_lqc\s*,\s*const\s+lfgpu_rng_fn\s*\*\s*rng\s*,\s*void\s*\*\s*const\s*\*\s*rng_user\s*,\s*uint8_t\s*\*\s*roots_out[^,]*,"
                     r"\s*lfgpu_ligero_prover\s*\*\*\s*out", k)
    # the documented properties: a shared engine draws in index order, the per-statement RS fallback, the A/B switch
    assert "SAME" in k and "index order" in k and "merely unbatched" in k and "LFGPU_COMMIT_BATCH" in k and "LFGPU_CB_CHUNK" in k
    zk = open(os.path.join(ROOT, "include", "lfgpu_zk.h")).read()
    assert re.search(r"\bint\s+lfgpu_zk_commit_batch\s*\(\s*lfgpu_zk_batch\s*\*\s*\w*\s*,\s*lfgpu_zk_prover\s*\*\s*const\s*\*\s*zk\s*,\s*size_t\s+nb\s*,"
                     r"\s*const\s+void\s*\*\s*const\s*\*\s*h_W\s*,\s*const\s+lfgpu_rng_fn\s*\*\s*rng\s*,\s*void\s*\*\s*const\s*\*\s*rng_user\s*,"
                     r"\s*const\s+lfgpu_transcript_ops\s*\*\s*const\s*\*\s*ts\s*,\s*uint8_t\s*\*\s*roots_out", zk)
    assert "the same value for every member" in zk and "LFGPU_COMMIT_BATCH" in zk


def test_python_mirror_names_them(pkg):
    for name in SYMBOLS:
        assert name in pkg.ABI_SYMBOLS, name
    L = pkg.load_library()
    assert L.lfgpu_column_commit_batch.restype is C.c_int and len(L.lfgpu_column_commit_batch.argtypes) == 11
    assert L.lfgpu_ligero_commit_batch.restype is C.c_int and len(L.lfgpu_ligero_commit_batch.argtypes) == 12
    assert L.lfgpu_zk_commit_batch.restype is C.c_int and len(L.lfgpu_zk_commit_batch.argtypes) == 8
    assert callable(getattr(pkg.ZkBatch, "commit")) and callable(getattr(pkg.LigeroProver, "commit_batch"))
    assert callable(getattr(pkg.LfGpu, "column_commit_batch"))


def test_null_arguments_are_argument_errors_without_a_device(pkg):
    L = pkg.load_library()
    roots = (C.c_uint8 * 64)()
    out = (C.c_void_p * 2)()
    assert L.lfgpu_column_commit_batch(None, pkg.FIELD_GF2_128, 1, 4, 0, 4, 2, None, None, None, roots) == 1  # LFGPU_ERR_ARG
    assert L.lfgpu_ligero_commit_batch(None, pkg.FIELD_GF2_128, 4, None, 2, None, 0, None, None, None, roots, out) == 1
    assert out[0] is None and out[1] is None
    assert L.lfgpu_zk_commit_batch(None, None, 2, None, None, None, None, roots) == 1
    assert bytes(roots) == bytes(64)


def test_cxx_example_compiles_and_fails_loudly_without_gpu(pkg):
    exe = build_example()
    import torch
    if torch.cuda.is_available():
        return  # with a device the example runs: tests/test_zk_commit_batch.py
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "nonexistent.lfc1"), "w.bin", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
