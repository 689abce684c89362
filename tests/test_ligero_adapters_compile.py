"""include/lfgpu_zk_adapters.h: lfgpu::GpuLigeroProver / GpuLigeroVerifier instantiate with the reference's own LigeroParam,
LigeroCommitment, LigeroProof, LigeroLinearConstraint, LigeroHash, LigeroQuadraticConstraint, Transcript and RandomEngine
(compile only; build container only, as tests/test_abi_and_adapters.py::test_adapters_instantiate_reference_ligero_prover)."""
import os
import subprocess

import pytest

from __graft_entry__ import ROOT


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir("/root/reference/lib"), reason="reference checkout not present")
def test_ligero_adapters_instantiate_with_reference_types(tmp_path):
    cmd = ["g++", "-std=c++17", "-O0", "-mpclmul", "-DOPENSSL_SUPPRESS_DEPRECATED=1", "-Wno-deprecated-declarations",
           "-Wno-ignored-attributes", "-I/root/reference/lib", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "ligero_adapters_compile_check.cc"), "-o", str(tmp_path / "lacc.o")]
    subprocess.check_call(cmd)
