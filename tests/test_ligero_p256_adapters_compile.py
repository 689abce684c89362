"""include/lfgpu_zk_adapters.h: lfgpu::GpuLigeroProver / GpuLigeroVerifier instantiate over Fp256Base with the reference's own
LigeroParam, LigeroCommitment, LigeroProof, LigeroLinearConstraint, LigeroHash, LigeroQuadraticConstraint, Transcript and
RandomEngine (compile only; build container only, as tests/test_ligero_adapters_compile.py for the 16-byte fields)."""
import os
import subprocess

import pytest

from __graft_entry__ import ROOT


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir("/root/reference/lib"), reason="reference checkout not present")
def test_ligero_adapters_instantiate_with_reference_types_over_p256(tmp_path):
    cmd = ["g++", "-std=c++17", "-O0", "-mpclmul", "-DOPENSSL_SUPPRESS_DEPRECATED=1", "-Wno-deprecated-declarations",
           "-Wno-ignored-attributes", "-I/root/reference/lib", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "ligero_p256_adapters_compile_check.cc"), "-o", str(tmp_path / "lp256acc.o")]
    subprocess.check_call(cmd)
