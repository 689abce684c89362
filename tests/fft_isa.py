"""The gfx950 assembly of csrc/fft.hip, for the tests that pin what K1's tile kernels compile to: one `hipcc -S` per process,
and the parsing those tests share.  Kernels are named by their mangled names."""
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT = os.path.join(ROOT, "longfellow-zk_amd", "csrc", "fft.hip")

SCC_READ = re.compile(r"(s_cbranch_scc[01]|s_addc_u32|s_subb_u32|s_cselect_b(32|64)|s_cmov_b(32|64)|s_cmovk_i32)$")
SCC_WRITE = re.compile(r"(s_cmp\w*|s_bitcmp\w*|s_add_[iu]32|s_addc_u32|s_sub_[iu]32|s_subb_u32|s_(and|or|xor|andn2|orn2|nand|nor|xnor|not)_\w+|"
                       r"s_lshl\w*|s_lshr\w*|s_ashr\w*|s_bfe_\w+|s_min_\w+|s_max_\w+|s_abs\w*|s_bcnt\w*|s_quadmask\w*|s_wqm\w*)$")

# desc: the integer fields of the kernel descriptor (.amdhsa_<field>); lines: the body, stripped; ops: its instructions' opcodes
Kernel = collections.namedtuple("Kernel", "desc lines ops")


def hipcc():
    h = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(h):
        pytest.skip("no hipcc")
    return h


@functools.lru_cache(maxsize=None)
def _asm():
    with tempfile.TemporaryDirectory(prefix="fft_isa_") as d:
        out = os.path.join(d, "fft.s")
        subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-S",
                               "--cuda-device-only", "-o", out, FFT])
        with open(out) as f:
            return f.read()


def _is_instruction(l):
    return l and not l.startswith((";", ".")) and not l.endswith(":")


@functools.lru_cache(maxsize=None)
def kernel(name):
    s = _asm()
    desc = s.split(".amdhsa_kernel " + name + "\n", 1)[1].split(".end_amdhsa_kernel", 1)[0]
    body = s.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
    lines = [l.strip() for l in body.splitlines()]
    return Kernel({k: int(v) for k, v in re.findall(r"^\s*\.amdhsa_(\w+) (\d+)\s*$", desc, re.M)}, lines,
                  [l.split()[0] for l in lines if _is_instruction(l)])


def valu(name):
    """VALU instructions in the kernel's body (the tiles are fully unrolled: static = dynamic count)"""
    return sum(op.startswith("v_") for op in kernel(name).ops)


def assert_no_scratch_within_128_vgprs(name):
    """no scratch, and at most 128 VGPRs: 4 waves per SIMD, two 512-thread workgroups per CU"""
    desc = kernel(name).desc
    assert desc["private_segment_fixed_size"] == 0, name
    assert desc["next_free_vgpr"] <= 128, name


def assert_scc_clean(name):
    """The SALU instructions inside the arithmetic's asm write SCC: no SCC reader of the compiler's may follow one of them
    without an SCC write of its own in between (the asm statements declare the clobber)."""
    in_asm, last = False, None
    for l in kernel(name).lines:
        if l.startswith(";;#ASMSTART") or l.startswith(";;#ASMEND"):
            in_asm = l.startswith(";;#ASMSTART")
        elif l.endswith(":"):
            last = None
        elif _is_instruction(l):
            op = l.split()[0]
            if SCC_READ.match(op):
                assert last != "asm", (name, l)
            if SCC_WRITE.match(op):
                last = "asm" if in_asm else "c"


def vm_stream(name):
    """(the kernel's global loads and s_waitcnt instructions in program order, the indices of the loads among them)"""
    ins = [l for l in kernel(name).lines if l.startswith(("global_load", "s_waitcnt"))]
    return ins, [i for i, l in enumerate(ins) if l.startswith("global_load")]


def _vmcnt_wait(l):
    return l.startswith("s_waitcnt") and "vmcnt" in l


def dwordx4_loads_before_first_vmcnt_wait(name):
    ins, _ = vm_stream(name)
    first_wait = next(i for i, l in enumerate(ins) if _vmcnt_wait(l))
    return sum(l.startswith("global_load_dwordx4") for l in ins[:first_wait])


def assert_global_loads(name, n):
    """exactly n global loads, every one a dwordx4"""
    ins, loads = vm_stream(name)
    assert len(loads) == n and all(ins[i].startswith("global_load_dwordx4") for i in loads), (name, ins)


def assert_no_vmcnt_wait_among_loads(name, last=None):
    """no wait on vector memory between the first and the last of the kernel's global loads (of its final `last` ones, if given)"""
    ins, loads = vm_stream(name)
    if last is not None:
        loads = loads[-last:]
    assert not any(_vmcnt_wait(l) for l in ins[loads[0]:loads[-1]]), (name, ins)
