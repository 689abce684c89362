"""longfellow-zk_amd -- MI355X-native prover hot path for longfellow-zk.

Host-side mirror (Python/ctypes) of the C ABI in include/lfgpu.h.  The compute
lives in hand-written HIP kernels (csrc/*.hip, built into liblfgpu.so by
__graft_entry__.build()).  There is NO CPU fallback: if the library is missing
or the GPU is absent every call raises.

The directory name contains a hyphen, so import it through
``__graft_entry__.load_package()`` (importlib) rather than ``import``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFGPU_LIB") or os.path.join(_HERE, "liblfgpu.so")  # LFGPU_LIB: an instrumented build of the same sources

FIELD_GF2_128 = 4  # FieldID, reference lib/proto/circuit_io.h:24-36
FIELD_FP128 = 6
FIELD_P256 = 1  # Fp256Base, 32-byte elements

# 2^32-order root of unity of Fp128 (reference lib/algebra/fp_p128.h:48-56), canonical value
FP128_OMEGA32 = 164956748514267535023998284330560247862
FP128_P = 2**128 - 2**108 + 1
# F64 = Fp<1>, p = 2^64 - 2^32 + 1, and its root of unity of order 2^32 (reference lib/algebra/fft_test.cc:208-213)
F64_P = 2**64 - 2**32 + 1
F64_OMEGA32 = 2752994695033296049

ABI_SYMBOLS = [
    "lfgpu_init", "lfgpu_shutdown", "lfgpu_last_error", "lfgpu_set_stream", "lfgpu_own_stream", "lfgpu_set_rng_exact_calls", "lfgpu_sync", "lfgpu_malloc",
    "lfgpu_free", "lfgpu_memcpy_h2d", "lfgpu_memcpy_d2h", "lfgpu_fp128_fft", "lfgpu_f64_2_fft", "lfgpu_gf2128_lch14_fft",
    "lfgpu_gf2128_rs_encode_rows", "lfgpu_gf2128_rs_encode_tableau", "lfgpu_fp128_rs_encode_rows", "lfgpu_fp256_rs_encode_rows", "lfgpu_column_commit", "lfgpu_column_leaves", "lfgpu_merkle_build_tree",
    "lfgpu_merkle_open", "lfgpu_sumcheck_partials", "lfgpu_qw_scatter", "lfgpu_dense_bind", "lfgpu_hquad_bind_h",
    "lfgpu_rows_axpy", "lfgpu_gather_columns", "lfgpu_field_binop", "lfgpu_fp128_fft_host", "lfgpu_f64_2_fft_host", "lfgpu_gf2128_lch14_fft_host",
    "lfgpu_gf2128_rs_encode_rows_host", "lfgpu_fp128_rs_encode_rows_host", "lfgpu_fp256_rs_encode_rows_host", "lfgpu_column_commit_host",
    "lfgpu_ligero_param_init", "lfgpu_ligero_commit", "lfgpu_ligero_commit_sharded", "lfgpu_ligero_row_shard", "lfgpu_ligero_layout_rows_sharded", "lfgpu_comm_selftest", "lfgpu_ligero_layout_rows", "lfgpu_ligero_encode_rows", "lfgpu_ligero_prover_from_slab", "lfgpu_ligero_low_degree_proof", "lfgpu_ligero_dot_proof",
    "lfgpu_ligero_inner_product_rows", "lfgpu_ligero_dot_proof_sparse",
    "lfgpu_ligero_quadratic_proof", "lfgpu_ligero_open", "lfgpu_ligero_tableau", "lfgpu_ligero_free",
    "lfgpu_quad_upload", "lfgpu_quad_free", "lfgpu_eval_quad", "lfgpu_quad_bind_g", "lfgpu_sumcheck_layer", "lfgpu_raw_eq2", "lfgpu_quad_bind_gh_all",
    "lfgpu_eval_quad_copies", "lfgpu_sumcheck_evaluations_c", "lfgpu_dense_bind_rows", "lfgpu_eqs", "lfgpu_sumcheck_layer_copies",
    "lfgpu_sumcheck_layer_batch", "lfgpu_eval_quad_batch",
    "lfgpu_sumcheck_layer256", "lfgpu_sumcheck_layer_batch256", "lfgpu_eval_quad_batch256",
    # include/lfgpu_zk.h
    "lfgpu_transcript_new", "lfgpu_transcript_free", "lfgpu_transcript_get_ops", "lfgpu_transcript_write_bytes",
    "lfgpu_transcript_write_elt", "lfgpu_transcript_write_elt_array", "lfgpu_transcript_bytes", "lfgpu_transcript_write_elt_sized", "lfgpu_transcript_write_elt_array_sized", "lfgpu_sha256",
    "lfgpu_aes256_ecb_block", "lfgpu_host_gf2128_mul", "lfgpu_crypto_hw", "lfgpu_circuit_from_lfc1", "lfgpu_circuit_share", "lfgpu_circuit_get_info", "lfgpu_circuit_layer_info",
    "lfgpu_circuit_free", "lfgpu_zk_prover_new", "lfgpu_zk_prover_set_comm", "lfgpu_zk_prover_param", "lfgpu_zk_commit", "lfgpu_zk_prove",
    "lfgpu_zk_proof_write", "lfgpu_zk_timings", "lfgpu_zk_prover_free", "lfgpu_zk_verify", "lfgpu_zk_verify_committed",
    "lfgpu_zk_batch_new", "lfgpu_zk_prove_batch", "lfgpu_zk_batch_free",
    "lfgpu_column_commit_batch", "lfgpu_ligero_commit_batch", "lfgpu_zk_commit_batch",
    "lfgpu_ligero_prove", "lfgpu_ligero_verify",
    "lfgpu_zk_batch256_new", "lfgpu_zk_prove_batch256", "lfgpu_zk_batch256_free", "lfgpu_ligero_prove_batch256", "lfgpu_ligero_open_batch256",
    "lfgpu_column_commit_batch256", "lfgpu_ligero_commit_batch256", "lfgpu_zk_commit_batch256",
]


class LigeroParam(C.Structure):
    """lfgpu_ligero_param == LigeroParam (reference lib/ligero/ligero_param.h:117-307)"""
    _fields_ = [(n, C.c_size_t) for n in (
        "nw", "nq", "rateinv", "nreq", "block_enc", "block", "dblock", "block_ext", "r", "w", "nwrow", "nqtriples",
        "nwqrow", "nrow", "mc_pathlen", "ildt", "idot", "iquad", "iw", "iq")]


RNG_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)  # RandomEngine::bytes
# round callback of lfgpu_sumcheck_layer: (user, hand, round, evals[3][2], challenge_out[2])
SC_ROUND_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
# copy-round callback of lfgpu_sumcheck_layer_copies: (user, round, evals[4][2], challenge_out[2])
SC_ROUND_C_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
# round callback of lfgpu_sumcheck_layer_batch: (user, hand, round, nb, evals[nb][3][2], challenge_out[nb][2])
SC_ROUND_BATCH_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
SC_BATCH_MAX = 64  # LFGPU_SC_BATCH_MAX
# the same two callbacks over Fp256Base (4-word elements): evals[3][4] -> challenge_out[4]; evals[nb][3][4] -> challenge_out[nb][4]
SC_ROUND256_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
SC_ROUND_BATCH256_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
P256_BATCH_SMALL_MAX = 2048  # LFGPU_P256_BATCH_SMALL_MAX: the hand-off bound of lfgpu_sumcheck_layer_batch256's one-launch step


class TranscriptOps(C.Structure):
    """lfgpu_transcript_ops (include/lfgpu_zk.h): the caller's Fiat-Shamir transcript behind function pointers"""
    _fields_ = [("user", C.c_void_p), ("write_bytes", C.c_void_p), ("write_elt", C.c_void_p),
                ("write_elt_array", C.c_void_p), ("gen_bytes", C.c_void_p), ("clone", C.c_void_p), ("free_clone", C.c_void_p),
                ("write_elt_sized", C.c_void_p), ("write_elt_array_sized", C.c_void_p)]  # 32-byte elements (Fp256Base)


class LigeroLlterm(C.Structure):
    """lfgpu_ligero_llterm == LigeroLinearConstraint (reference lib/ligero/ligero_param.h): A[c][w] += k"""
    _fields_ = [("c", C.c_size_t), ("w", C.c_size_t), ("k", C.c_uint64 * 2)]


LLTERM_DTYPE = [("c", "<u8"), ("w", "<u8"), ("k", "<u8", (2,))]  # the same record as a numpy dtype


def llterm_array(llterm):
    """a list of (c, w, k) -- k a pair of uint64 words, the Elt image -- or an array of LLTERM_DTYPE -> a contiguous array of
    lfgpu_ligero_llterm records"""
    import numpy as np
    if isinstance(llterm, np.ndarray) and llterm.dtype == np.dtype(LLTERM_DTYPE):
        return np.ascontiguousarray(llterm)
    a = np.zeros(len(llterm), dtype=LLTERM_DTYPE)
    for i, (c, w, k) in enumerate(llterm):
        a[i] = (c, w, (int(k[0]), int(k[1])))
    return a


class LigeroLlterm256(C.Structure):
    """lfgpu_ligero_llterm256: the same term over Fp256Base, k a 32-byte Montgomery image"""
    _fields_ = [("c", C.c_size_t), ("w", C.c_size_t), ("k", C.c_uint64 * 4)]


LLTERM256_DTYPE = [("c", "<u8"), ("w", "<u8"), ("k", "<u8", (4,))]


def llterm256_array(llterm):
    """llterm_array for Fp256Base: (c, w, k) with k four uint64 words, or an array of LLTERM256_DTYPE"""
    import numpy as np
    if isinstance(llterm, np.ndarray) and llterm.dtype == np.dtype(LLTERM256_DTYPE):
        return np.ascontiguousarray(llterm)
    a = np.zeros(len(llterm), dtype=LLTERM256_DTYPE)
    for i, (c, w, k) in enumerate(llterm):
        a[i] = (c, w, tuple(int(x) for x in k))
    return a


def elt_words(field):
    """uint64 words of one host element: 4 for Fp256Base, 2 for the 16-byte fields"""
    return 4 if field == FIELD_P256 else 2


class CircuitInfo(C.Structure):
    """lfgpu_circuit_info"""
    _fields_ = [("field", C.c_int)] + [(n, C.c_size_t) for n in (
        "nv", "nc", "npub_in", "subfield_boundary", "ninputs", "nl", "logv", "nterms")] + [("id", C.c_uint8 * 32)]


class LfGpuError(RuntimeError):
    pass


_lib = None


def load_library():
    """dlopen liblfgpu.so and declare the ABI.  Raises (never falls back) when missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LfGpuError("%s not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime (libamdhip64 under torch/lib).  When torch shares the process -- device
    # tensors, streams, torch.distributed -- that runtime must be the one already loaded when liblfgpu.so is opened;
    # loading the system runtime first and torch's afterwards leaves the process with two runtimes and lfgpu_init
    # fails.  Stand-alone use (examples/zk_flatsha.cc) needs no torch and binds the system runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, u64, ci = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int
    pu64 = C.POINTER(C.c_uint64)
    sig = {
        "lfgpu_init": [ci, C.POINTER(vp)], "lfgpu_shutdown": [vp], "lfgpu_set_stream": [vp, vp], "lfgpu_own_stream": [vp], "lfgpu_set_rng_exact_calls": [vp, ci], "lfgpu_sync": [vp],
        "lfgpu_malloc": [vp, sz, C.POINTER(vp)], "lfgpu_free": [vp, vp], "lfgpu_scratch_info": [vp, ci, C.POINTER(vp), C.POINTER(sz)],
        "lfgpu_memcpy_h2d": [vp, vp, vp, sz], "lfgpu_memcpy_d2h": [vp, vp, vp, sz],
        "lfgpu_fp128_fft": [vp, ci, sz, sz, pu64, u64, vp, sz],
        "lfgpu_f64_2_fft": [vp, ci, sz, sz, pu64, u64, vp, sz],
        "lfgpu_gf2128_lch14_fft": [vp, ci, ci, sz, C.c_uint, u64, vp, sz],
        "lfgpu_gf2128_rs_encode_rows": [vp, ci, sz, sz, sz, vp, sz],
        "lfgpu_gf2128_rs_encode_tableau": [vp, ci, sz, sz, sz, sz, sz, sz, vp, sz],
        "lfgpu_fp128_rs_encode_rows": [vp, sz, sz, sz, pu64, u64, vp, sz],
        "lfgpu_fp256_rs_encode_rows": [vp, sz, sz, sz, vp, sz],
        "lfgpu_column_commit": [vp, ci, sz, sz, sz, sz, vp, vp, vp, vp],
        "lfgpu_column_leaves": [vp, ci, sz, sz, sz, sz, vp, vp, vp],
        "lfgpu_merkle_build_tree": [vp, sz, vp, vp],
        "lfgpu_merkle_open": [vp, sz, vp, vp, sz, vp, sz, C.POINTER(sz)],
        "lfgpu_sumcheck_partials": [vp, ci, sz, vp, vp, pu64, pu64],
        "lfgpu_qw_scatter": [vp, ci, sz, vp, vp, ci, vp, sz, vp],
        "lfgpu_dense_bind": [vp, ci, sz, pu64, vp, vp],
        "lfgpu_hquad_bind_h": [vp, ci, sz, vp, vp, pu64, ci, vp, vp, C.POINTER(sz)],
        "lfgpu_rows_axpy": [vp, ci, sz, sz, vp, vp, vp, sz],
        "lfgpu_field_binop": [vp, ci, ci, sz, vp, vp, vp],
        "lfgpu_gather_columns": [vp, sz, sz, sz, vp, vp, sz, vp],
        "lfgpu_fp128_fft_host": [vp, ci, sz, pu64, u64, vp],
        "lfgpu_f64_2_fft_host": [vp, ci, sz, pu64, u64, vp],
        "lfgpu_gf2128_lch14_fft_host": [vp, ci, ci, C.c_uint, u64, vp],
        "lfgpu_gf2128_rs_encode_rows_host": [vp, ci, sz, sz, sz, vp, sz],
        "lfgpu_fp128_rs_encode_rows_host": [vp, sz, sz, sz, pu64, u64, vp, sz],
        "lfgpu_fp256_rs_encode_rows_host": [vp, sz, sz, sz, vp, sz],
        "lfgpu_column_commit_host": [vp, ci, sz, sz, sz, sz, vp, vp, vp, vp],
        "lfgpu_ligero_param_init": [C.POINTER(LigeroParam), ci, ci, sz, sz, sz, sz, sz],
        "lfgpu_ligero_commit": [vp, ci, ci, C.POINTER(LigeroParam), vp, sz, vp, RNG_FN, vp, vp, C.POINTER(vp)],
        "lfgpu_ligero_layout_rows": [ci, ci, C.POINTER(LigeroParam), vp, sz, vp, RNG_FN, vp, sz, sz, vp, vp],
        "lfgpu_ligero_commit_sharded": [vp, ci, ci, C.POINTER(LigeroParam), vp, sz, vp, RNG_FN, vp, vp, vp, C.POINTER(vp)],
        "lfgpu_ligero_row_shard": [C.POINTER(LigeroParam), ci, ci, C.POINTER(sz), C.POINTER(sz)],
        "lfgpu_ligero_layout_rows_sharded": [ci, ci, C.POINTER(LigeroParam), vp, sz, vp, RNG_FN, vp, vp, vp, vp],
        "lfgpu_comm_selftest": [vp],
        "lfgpu_zk_prover_set_comm": [vp, vp, sz],
        "lfgpu_ligero_encode_rows": [vp, ci, ci, C.POINTER(LigeroParam), sz, sz, vp, vp],
        "lfgpu_ligero_prover_from_slab": [vp, ci, ci, C.POINTER(LigeroParam), sz, sz, vp, vp, vp, C.POINTER(vp)],
        "lfgpu_ligero_low_degree_proof": [vp, vp, vp],
        "lfgpu_ligero_dot_proof": [vp, vp, vp],
        "lfgpu_ligero_inner_product_rows": [vp, ci, sz, sz, sz, sz, vp, sz, vp, vp, vp, sz, vp],
        "lfgpu_ligero_dot_proof_sparse": [vp, vp, sz, vp, vp, vp, sz, vp],
        "lfgpu_ligero_quadratic_proof": [vp, vp, vp, vp],
        "lfgpu_ligero_open": [vp, vp, vp, vp, vp, sz, C.POINTER(sz)],
        "lfgpu_ligero_tableau": [vp, C.POINTER(vp)],
        "lfgpu_ligero_free": [vp],
        "lfgpu_quad_upload": [vp, ci, sz, vp, vp, vp, vp, sz, vp, sz, C.POINTER(vp)],
        "lfgpu_quad_free": [vp],
        "lfgpu_eval_quad": [vp, sz, vp, vp, C.POINTER(ci)],
        "lfgpu_quad_bind_g": [vp, sz, vp, vp, pu64, pu64, vp, vp, C.POINTER(sz)],
        "lfgpu_sumcheck_layer": [vp, sz, vp, vp, pu64, pu64, sz, sz, vp, pu64, SC_ROUND_FN, vp, pu64, pu64, pu64],
        "lfgpu_raw_eq2": [vp, ci, sz, sz, vp, vp, pu64, vp],
        "lfgpu_quad_bind_gh_all": [vp, sz, vp, vp, pu64, pu64, sz, sz, vp, vp, pu64],
        "lfgpu_eval_quad_copies": [vp, sz, sz, vp, vp, C.POINTER(ci)],
        "lfgpu_sumcheck_evaluations_c": [vp, ci, sz, vp, vp, sz, sz, vp, vp, pu64],
        "lfgpu_dense_bind_rows": [vp, ci, sz, sz, pu64, vp, vp],
        "lfgpu_eqs": [vp, ci, sz, sz, vp, vp],
        "lfgpu_sumcheck_layer_copies": [vp, sz, sz, vp, sz, vp, vp, pu64, pu64, sz, sz, vp, pu64, SC_ROUND_C_FN, SC_ROUND_FN, vp, pu64, pu64, pu64, pu64],
        "lfgpu_sumcheck_layer_batch": [vp, sz, sz, vp, vp, pu64, pu64, sz, sz, vp, sz, pu64, SC_ROUND_BATCH_FN, vp, pu64, pu64, pu64],
        "lfgpu_sumcheck_layer256": [vp, sz, vp, vp, pu64, pu64, sz, sz, vp, pu64, SC_ROUND256_FN, vp, pu64, pu64, pu64],
        "lfgpu_sumcheck_layer_batch256": [vp, sz, sz, vp, vp, pu64, pu64, sz, sz, vp, sz, pu64, SC_ROUND_BATCH256_FN, vp, pu64, pu64, pu64],
        "lfgpu_eval_quad_batch256": [vp, sz, sz, vp, sz, vp, sz, C.POINTER(ci)],
        "lfgpu_circuit_from_lfc1": [vp, vp, sz, C.POINTER(vp)],
        "lfgpu_circuit_share": [vp, vp, C.POINTER(vp)],
        "lfgpu_circuit_get_info": [vp, C.POINTER(CircuitInfo)],
        "lfgpu_circuit_layer_info": [vp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)],
        "lfgpu_circuit_free": [vp],
        "lfgpu_zk_prover_new": [vp, vp, sz, sz, sz, C.POINTER(vp)],
        "lfgpu_zk_prover_param": [vp, C.POINTER(LigeroParam)],
        "lfgpu_zk_commit": [vp, vp, RNG_FN, vp, C.POINTER(TranscriptOps), vp],
        "lfgpu_zk_prove": [vp, vp, C.POINTER(TranscriptOps), C.POINTER(ci)],
        "lfgpu_zk_proof_write": [vp, vp, sz, C.POINTER(sz)],
        "lfgpu_zk_timings": [vp, C.POINTER(C.c_double)],
        "lfgpu_zk_prover_free": [vp],
        "lfgpu_zk_verify": [vp, vp, sz, sz, sz, vp, sz, vp, C.POINTER(TranscriptOps), C.POINTER(ci), C.POINTER(C.c_char_p)],
        "lfgpu_zk_verify_committed": [vp, vp, sz, sz, sz, vp, sz, vp, C.POINTER(TranscriptOps), C.POINTER(ci), C.POINTER(C.c_char_p)],
        "lfgpu_crypto_hw": [ci],
        "lfgpu_eval_quad_batch": [vp, sz, sz, vp, sz, vp, sz, C.POINTER(ci)],
        "lfgpu_zk_batch_new": [vp, vp, sz, C.POINTER(vp)],
        "lfgpu_zk_prove_batch": [vp, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(C.POINTER(TranscriptOps)), C.POINTER(ci)],
        "lfgpu_zk_batch_free": [vp],
        "lfgpu_column_commit_batch": [vp, ci, sz, sz, sz, sz, sz, C.POINTER(vp), vp, C.POINTER(vp), vp],
        "lfgpu_ligero_commit_batch": [vp, ci, ci, C.POINTER(LigeroParam), sz, C.POINTER(vp), sz, vp, C.POINTER(RNG_FN), C.POINTER(vp), vp, C.POINTER(vp)],
        "lfgpu_ligero_prove_batch": [vp, C.POINTER(vp), sz, vp, C.POINTER(vp), sz, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), vp, vp, vp, vp, vp],
        "lfgpu_ligero_open_batch": [vp, C.POINTER(vp), sz, C.POINTER(sz), vp, vp, vp, sz, C.POINTER(sz)],
        "lfgpu_zk_batch256_new": [vp, vp, sz, C.POINTER(vp)],
        "lfgpu_zk_prove_batch256": [vp, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(C.POINTER(TranscriptOps)), C.POINTER(ci)],
        "lfgpu_zk_batch256_free": [vp],
        "lfgpu_ligero_prove_batch256": [vp, C.POINTER(vp), sz, vp, C.POINTER(vp), sz, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), vp, vp, vp, vp, vp],
        "lfgpu_ligero_open_batch256": [vp, C.POINTER(vp), sz, C.POINTER(sz), vp, vp, vp, sz, C.POINTER(sz)],
        "lfgpu_zk_commit_batch": [vp, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(RNG_FN), C.POINTER(vp), C.POINTER(C.POINTER(TranscriptOps)), vp],
        "lfgpu_column_commit_batch256": [vp, sz, sz, sz, sz, sz, C.POINTER(vp), vp, C.POINTER(vp), vp],
        "lfgpu_ligero_commit_batch256": [vp, C.POINTER(LigeroParam), sz, C.POINTER(vp), vp, C.POINTER(RNG_FN), C.POINTER(vp), vp, C.POINTER(vp)],
        "lfgpu_zk_commit_batch256": [vp, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(RNG_FN), C.POINTER(vp), C.POINTER(C.POINTER(TranscriptOps)), vp],
        "lfgpu_ligero_prove": [vp, C.POINTER(TranscriptOps), sz, sz, vp, vp, vp, vp, sz, C.POINTER(sz)],
        "lfgpu_ligero_verify": [vp, ci, ci, C.POINTER(LigeroParam), vp, vp, sz, C.POINTER(TranscriptOps), sz, sz, vp, vp, vp, vp, C.POINTER(ci),
                                C.POINTER(C.c_char_p)],
        "lfgpu_ligero_prove256": [vp, C.POINTER(TranscriptOps), sz, sz, vp, vp, vp, vp, sz, C.POINTER(sz)],
        "lfgpu_ligero_verify256": [vp, C.POINTER(LigeroParam), vp, vp, sz, C.POINTER(TranscriptOps), sz, sz, vp, vp, vp, vp, C.POINTER(ci),
                                   C.POINTER(C.c_char_p)],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ci, args
    L.lfgpu_last_error.restype, L.lfgpu_last_error.argtypes = C.c_char_p, [vp]
    L.lfgpu_transcript_new.restype, L.lfgpu_transcript_new.argtypes = vp, [vp, sz]
    for name, args in (("lfgpu_transcript_free", [vp]), ("lfgpu_transcript_get_ops", [vp, C.POINTER(TranscriptOps)]),
                       ("lfgpu_transcript_write_bytes", [vp, vp, sz]), ("lfgpu_transcript_write_elt", [vp, vp]),
                       ("lfgpu_transcript_write_elt_array", [vp, vp, sz]), ("lfgpu_transcript_bytes", [vp, vp, sz]),
                       ("lfgpu_transcript_write_elt_sized", [vp, vp, sz]), ("lfgpu_transcript_write_elt_array_sized", [vp, vp, sz, sz]),
                       ("lfgpu_sha256", [vp, sz, vp]), ("lfgpu_aes256_ecb_block", [vp, vp, vp]),
                       ("lfgpu_host_gf2128_mul", [pu64, pu64, pu64])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = None, args
    _lib = L
    return L


def _u64x2(v):
    """int (canonical 128-bit image) or sequence of two u64 -> (c_uint64 * 2)"""
    if isinstance(v, int):
        v = (v & (2**64 - 1), v >> 64)
    return (C.c_uint64 * 2)(int(v[0]), int(v[1]))


def _u64x4(v):
    """int (canonical 256-bit image) or sequence of four u64 -> (c_uint64 * 4)"""
    if isinstance(v, int):
        v = tuple((v >> (64 * k)) & (2**64 - 1) for k in range(4))
    return (C.c_uint64 * 4)(*[int(x) for x in v])


def fp128_to_montgomery(x):
    return (x * (1 << 128)) % FP128_P


def fp128_from_montgomery(x):
    return (x * pow(1 << 128, -1, FP128_P)) % FP128_P


def f64_to_montgomery(x):
    return (x * (1 << 64)) % F64_P


def f64_from_montgomery(x):
    return (x * pow(1 << 64, -1, F64_P)) % F64_P


def _f64_2_omega(omega):
    """None = the reference's root of order 2^32 (real); else (re, im) Montgomery images"""
    if omega is None:
        omega = (f64_to_montgomery(F64_OMEGA32), 0)
    return (C.c_uint64 * 2)(int(omega[0]), int(omega[1]))


class LfGpu:
    """One context per process / GPU (lfgpu_ctx).  Pointer arguments are raw device
    addresses (e.g. torch.Tensor.data_ptr()); strides are in 16-byte elements."""

    def __init__(self, device=0, stream=None):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.lfgpu_init(int(device), C.byref(h))
        if rc != 0:
            raise LfGpuError("lfgpu_init(device=%d) failed with code %d (no usable MI355X?)" % (device, rc))
        self.h = h
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "h", None):
            self.L.lfgpu_shutdown(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise LfGpuError("lfgpu error %d: %s" % (rc, self.L.lfgpu_last_error(self.h).decode()))

    def set_stream(self, stream):
        self._ck(self.L.lfgpu_set_stream(self.h, C.c_void_p(int(stream))))

    def own_stream(self):
        """a non-blocking stream of the context's own: K contexts in K host threads then run concurrently on one device"""
        self._ck(self.L.lfgpu_own_stream(self.h))
        return self

    def set_rng_exact_calls(self, exact=True):
        """one RandomEngine call per element / nonce, as the reference draws (for engines that are not byte streams)"""
        self._ck(self.L.lfgpu_set_rng_exact_calls(self.h, 1 if exact else 0))

    def sync(self):
        self._ck(self.L.lfgpu_sync(self.h))

    # --- device memory without torch: for callers whose threads each drive a context and stream of their own
    def malloc(self, nbytes):
        d = C.c_void_p()
        self._ck(self.L.lfgpu_malloc(self.h, nbytes, C.byref(d)))
        return d.value

    def free(self, d_ptr):
        self._ck(self.L.lfgpu_free(self.h, C.c_void_p(d_ptr)))

    def memcpy_h2d(self, d_ptr, a):
        """a: a contiguous numpy array; copied on the context's stream, complete on return"""
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("memcpy_h2d: contiguous array needed")
        self._ck(self.L.lfgpu_memcpy_h2d(self.h, C.c_void_p(d_ptr), C.c_void_p(a.ctypes.data), a.nbytes))

    def memcpy_d2h(self, a, d_ptr):
        """fills the contiguous numpy array a; ordered behind the context's earlier calls, complete on return"""
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("memcpy_d2h: contiguous array needed")
        self._ck(self.L.lfgpu_memcpy_d2h(self.h, C.c_void_p(a.ctypes.data), C.c_void_p(d_ptr), a.nbytes))

    # --- K1 FFT<Fp128>::fftb / fftf (reference lib/algebra/fft.h:185-201)
    def fp128_fft(self, d_ptr, rows, n, ld=None, forward=False, omega=None, omega_order=1 << 32):
        omega = _u64x2(fp128_to_montgomery(FP128_OMEGA32) if omega is None else omega)
        self._ck(self.L.lfgpu_fp128_fft(self.h, 1 if forward else 0, rows, n, omega, omega_order, C.c_void_p(d_ptr),
                                        n if ld is None else ld))

    # --- K1 over F64_2 = Fp2<Fp<1>> (reference lib/algebra/fft_test.cc:205-229); omega = (re, im) in Montgomery form
    def f64_2_fft(self, d_ptr, rows, n, ld=None, forward=False, omega=None, omega_order=1 << 32):
        omega = _f64_2_omega(omega)
        self._ck(self.L.lfgpu_f64_2_fft(self.h, 1 if forward else 0, rows, n, omega, omega_order, C.c_void_p(d_ptr),
                                        n if ld is None else ld))

    # --- K2 LCH14::FFT / IFFT (reference lib/gf2k/lch14.h:106-144)
    def gf2128_lch14_fft(self, d_ptr, rows, l, coset=0, ld=None, inverse=False, subfield_log_bits=4):
        self._ck(self.L.lfgpu_gf2128_lch14_fft(self.h, subfield_log_bits, 1 if inverse else 0, rows, l, coset,
                                               C.c_void_p(d_ptr), (1 << l) if ld is None else ld))

    # --- K3 LCH14ReedSolomon::interpolate over rows (reference lib/gf2k/lch14_reed_solomon.h:49-103)
    def gf2128_rs_encode_rows(self, d_ptr, nrow, n, m, ld=None, subfield_log_bits=4):
        self._ck(self.L.lfgpu_gf2128_rs_encode_rows(self.h, subfield_log_bits, nrow, n, m, C.c_void_p(d_ptr),
                                                    m if ld is None else ld))

    def gf2128_rs_encode_tableau(self, d_ptr, nrow, n1, n2, lo2, hi2, m, ld=None, subfield_log_bits=4):
        """all rows of a Ligero tableau in one launch: rows [lo2, hi2) have n2 valid values, the others n1"""
        self._ck(self.L.lfgpu_gf2128_rs_encode_tableau(self.h, subfield_log_bits, nrow, n1, n2, lo2, hi2, m, C.c_void_p(d_ptr),
                                                       m if ld is None else ld))

    # --- K4 ReedSolomon::interpolate over rows (reference lib/algebra/reed_solomon.h:93-110)
    def fp128_rs_encode_rows(self, d_ptr, nrow, n, m, ld=None, omega=None, omega_order=1 << 32):
        omega = _u64x2(fp128_to_montgomery(FP128_OMEGA32) if omega is None else omega)
        self._ck(self.L.lfgpu_fp128_rs_encode_rows(self.h, nrow, n, m, omega, omega_order, C.c_void_p(d_ptr),
                                                   m if ld is None else ld))

    # --- ReedSolomon<Fp256Base, FFTExtConvolution>::interpolate over rows of 32-byte elements (BASELINE config 5)
    def fp256_rs_encode_rows(self, d_ptr, nrow, n, m, ld=None):
        self._ck(self.L.lfgpu_fp256_rs_encode_rows(self.h, nrow, n, m, C.c_void_p(d_ptr), m if ld is None else ld))

    # --- inner_product_vector + layout_Aext on the device (reference lib/ligero/ligero_param.h:382-430)
    def ligero_inner_product_rows(self, field, w, r, ld, nrows, d_dense, ndense, scale, idx, val, d_rows):
        """rows[i][r + j] = scale * dense[i*w + j] (flat positions < ndense), then rows[pos(idx)] += val; the first
        r + w columns of all nrows rows are cleared first.  idx: strictly increasing flat indices (host)."""
        import numpy as np
        sc = np.ascontiguousarray(scale, dtype=np.uint64)
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        val = np.ascontiguousarray(val, dtype=np.uint64)
        self._ck(self.L.lfgpu_ligero_inner_product_rows(self.h, field, w, r, ld, nrows, C.c_void_p(d_dense), ndense,
                                                        C.c_void_p(sc.ctypes.data), C.c_void_p(idx.ctypes.data),
                                                        C.c_void_p(val.ctypes.data), len(idx), C.c_void_p(d_rows)))

    # --- K5+K6 MerkleCommitment::commit (reference lib/merkle/merkle_commitment.h:50-64)
    def column_commit(self, field, nrow, ld, col0, ncols, d_T, d_nonces, d_layers):
        root = (C.c_uint8 * 32)()
        self._ck(self.L.lfgpu_column_commit(self.h, field, nrow, ld, col0, ncols, C.c_void_p(d_T),
                                            C.c_void_p(d_nonces), C.c_void_p(d_layers), root))
        return bytes(root)

    def column_commit_batch(self, field, nrow, ld, col0, ncols, d_Ts, d_nonces, d_layers):
        """lfgpu_column_commit for len(d_Ts) tableaux of one shape in one chain: d_Ts / d_layers are lists of device pointers,
        d_nonces one contiguous [nb][ncols][32] device array -> [root] per statement"""
        nb = len(d_Ts)
        if len(d_layers) != nb:
            raise ValueError("column_commit_batch: one heap per tableau")
        n = max(1, nb)
        roots = (C.c_uint8 * (32 * n))()
        self._ck(self.L.lfgpu_column_commit_batch(self.h, field, nrow, ld, col0, ncols, nb, (C.c_void_p * n)(*d_Ts), C.c_void_p(d_nonces),
                                                  (C.c_void_p * n)(*d_layers), roots))
        raw = bytes(roots)
        return [raw[32 * b:32 * b + 32] for b in range(nb)]

    def column_commit_batch256(self, nrow, ld, col0, ncols, d_Ts, d_nonces, d_layers):
        """lfgpu_column_commit_batch256: column_commit_batch for tableaux of 32-byte elements (FIELD_P256) -> [root] per statement"""
        nb = len(d_Ts)
        if len(d_layers) != nb:
            raise ValueError("column_commit_batch256: one heap per tableau")
        n = max(1, nb)
        roots = (C.c_uint8 * (32 * n))()
        self._ck(self.L.lfgpu_column_commit_batch256(self.h, nrow, ld, col0, ncols, nb, (C.c_void_p * n)(*d_Ts), C.c_void_p(d_nonces),
                                                     (C.c_void_p * n)(*d_layers), roots))
        raw = bytes(roots)
        return [raw[32 * b:32 * b + 32] for b in range(nb)]

    def merkle_build_tree(self, n, d_layers):
        root = (C.c_uint8 * 32)()
        self._ck(self.L.lfgpu_merkle_build_tree(self.h, n, C.c_void_p(d_layers), root))
        return bytes(root)

    def merkle_open(self, n, d_layers, pos):
        pos_a = (C.c_size_t * len(pos))(*pos)
        cap = max(1, len(pos) * 64)
        buf = (C.c_uint8 * (32 * cap))()
        npath = C.c_size_t()
        self._ck(self.L.lfgpu_merkle_open(self.h, n, C.c_void_p(d_layers), pos_a, len(pos), buf, cap, C.byref(npath)))
        raw = bytes(buf)
        return [raw[32 * i:32 * i + 32] for i in range(npath.value)]

    # --- K7 loop of ProverLayers::evaluations (reference lib/sumcheck/prover_layers.h:365-388)
    def sumcheck_partials(self, field, n, d_QW, d_W):
        a0, a2 = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        self._ck(self.L.lfgpu_sumcheck_partials(self.h, field, n, C.c_void_p(d_QW), C.c_void_p(d_W), a0, a2))
        return (a0[0], a0[1]), (a2[0], a2[1])

    # --- K8 QW scatter (reference lib/sumcheck/prover_layers.h:239-243)
    def qw_scatter(self, field, n, d_hc, d_vc, hand, d_Wother, nqw, d_QW):
        self._ck(self.L.lfgpu_qw_scatter(self.h, field, n, C.c_void_p(d_hc), C.c_void_p(d_vc), hand,
                                         C.c_void_p(d_Wother), nqw, C.c_void_p(d_QW)))

    # --- K9 Dense::bind / HQuad::bind_h (reference lib/arrays/dense.h:70-87, lib/sumcheck/hquad.h:90-123)
    def dense_bind(self, field, n0, r, d_in, d_out):
        self._ck(self.L.lfgpu_dense_bind(self.h, field, n0, _u64x2(r), C.c_void_p(d_in), C.c_void_p(d_out)))
        return (n0 + 1) // 2

    def hquad_bind_h(self, field, n, d_hc, d_vc, r, hand, d_hc_out, d_vc_out):
        n_out = C.c_size_t()
        self._ck(self.L.lfgpu_hquad_bind_h(self.h, field, n, C.c_void_p(d_hc), C.c_void_p(d_vc), _u64x2(r), hand,
                                           C.c_void_p(d_hc_out), C.c_void_p(d_vc_out), C.byref(n_out)))
        return n_out.value

    # --- Eqs::raw_eq2 (reference lib/arrays/eqs.h:46-80)
    def raw_eq2(self, field, logn, n, G0, G1, alpha, d_eq):
        """eq[i] = EQ(G0, i) + alpha EQ(G1, i), i < n; G0 / G1: numpy uint64[logn][2] host arrays"""
        import numpy as np
        G0, G1 = np.ascontiguousarray(G0, dtype=np.uint64), np.ascontiguousarray(G1, dtype=np.uint64)
        self._ck(self.L.lfgpu_raw_eq2(self.h, field, logn, n, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data),
                                      _u64x2(alpha), C.c_void_p(d_eq)))

    # --- the copy rounds of a circuit with nc > 1 copies (reference lib/sumcheck/prover_layers.h:196-216,415-496)
    def sumcheck_evaluations_c(self, field, nh, d_hc, d_vc, n0, nrows, d_W, d_eq):
        """the accumulators of ProverLayers::evaluations_c -> [coefs[0], coefs[2], coefs[3]] as (lo, hi) pairs"""
        acc = (C.c_uint64 * 6)()
        self._ck(self.L.lfgpu_sumcheck_evaluations_c(self.h, field, nh, C.c_void_p(d_hc), C.c_void_p(d_vc), n0, nrows,
                                                     C.c_void_p(d_W), C.c_void_p(d_eq), acc))
        return [(acc[2 * k], acc[2 * k + 1]) for k in range(3)]

    def dense_bind_rows(self, field, n0, nrows, r, d_in, d_out):
        """Dense::bind with n1 = nrows, out of place -> the new row length (n0 + 1) // 2"""
        self._ck(self.L.lfgpu_dense_bind_rows(self.h, field, n0, nrows, _u64x2(r), C.c_void_p(d_in), C.c_void_p(d_out)))
        return (n0 + 1) // 2

    def eqs(self, field, logn, n, Q, d_eq):
        """Eqs::filleq: eq[i] = EQ(Q, i), i < n; Q: numpy uint64[logn][2] host array"""
        import numpy as np
        Q = np.ascontiguousarray(Q, dtype=np.uint64)
        self._ck(self.L.lfgpu_eqs(self.h, field, logn, n, C.c_void_p(Q.ctypes.data) if logn else None, C.c_void_p(d_eq)))

    def field_binop(self, field, op, n, d_a, d_b, d_out):
        """element-wise Field::addf/subf/mulf (op 0/1/2)"""
        self._ck(self.L.lfgpu_field_binop(self.h, field, op, n, C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_out)))

    # --- K12 row combinations (reference lib/ligero/ligero_prover.h:281-291,346-351)
    def rows_axpy(self, field, nrows, n, d_y, u_host, d_T, ld):
        self._ck(self.L.lfgpu_rows_axpy(self.h, field, nrows, n, C.c_void_p(d_y), C.c_void_p(u_host.ctypes.data),
                                        C.c_void_p(d_T), ld))

    def gather_columns(self, nrow, ld, col0, d_T, idx, d_req):
        idx_a = (C.c_size_t * len(idx))(*idx)
        self._ck(self.L.lfgpu_gather_columns(self.h, nrow, ld, col0, C.c_void_p(d_T), idx_a, len(idx),
                                             C.c_void_p(d_req)))

    # --- host-buffer conveniences (numpy uint64[...,2] arrays, modified in place)
    def fp128_fft_host(self, a, forward=False, omega=None, omega_order=1 << 32):
        omega = _u64x2(fp128_to_montgomery(FP128_OMEGA32) if omega is None else omega)
        self._ck(self.L.lfgpu_fp128_fft_host(self.h, 1 if forward else 0, a.shape[0], omega, omega_order,
                                             C.c_void_p(a.ctypes.data)))

    def f64_2_fft_host(self, a, forward=False, omega=None, omega_order=1 << 32):
        self._ck(self.L.lfgpu_f64_2_fft_host(self.h, 1 if forward else 0, a.shape[0], _f64_2_omega(omega), omega_order,
                                             C.c_void_p(a.ctypes.data)))

    def gf2128_lch14_fft_host(self, a, l, coset=0, inverse=False, subfield_log_bits=4):
        self._ck(self.L.lfgpu_gf2128_lch14_fft_host(self.h, subfield_log_bits, 1 if inverse else 0, l, coset,
                                                    C.c_void_p(a.ctypes.data)))

    def gf2128_rs_encode_rows_host(self, T, nrow, n, m, ld, subfield_log_bits=4):
        self._ck(self.L.lfgpu_gf2128_rs_encode_rows_host(self.h, subfield_log_bits, nrow, n, m,
                                                         C.c_void_p(T.ctypes.data), ld))

    def column_commit_host(self, field, T, nrow, ld, col0, ncols, nonces, layers=None):
        root = (C.c_uint8 * 32)()
        self._ck(self.L.lfgpu_column_commit_host(self.h, field, nrow, ld, col0, ncols, C.c_void_p(T.ctypes.data),
                                                 C.c_void_p(nonces.ctypes.data),
                                                 C.c_void_p(layers.ctypes.data) if layers is not None else None, root))
        return bytes(root)


def ligero_param(field, nw, nq, rateinv, nreq, block_enc, subfield_log_bits=4):
    """LigeroParam(nw, nq, rateinv, nreq, block_enc) (reference lib/ligero/ligero_param.h:172-178)"""
    p = LigeroParam()
    rc = load_library().lfgpu_ligero_param_init(C.byref(p), field, subfield_log_bits, nw, nq, rateinv, nreq, block_enc)
    if rc != 0:
        raise LfGpuError("LigeroParam layout failed (block_enc too large / too small)")
    return p


def ligero_layout_rows(field, param, W, subfield_boundary, lqc, rng_bytes, row_lo=0, row_hi=None, subfield_log_bits=4):
    """lfgpu_ligero_layout_rows (host only, no device): every RandomEngine draw of LigeroProver::commit in the reference's order
    -> (the un-encoded rows [row_lo, row_hi) as [rows][dblock] elements, the block_ext Merkle nonces).  All three fields;
    FIELD_P256: W and the rows are (n, 4) uint64 arrays of 32-byte Montgomery images."""
    import numpy as np
    L = load_library()
    row_hi = param.nrow if row_hi is None else row_hi

    def cb(_user, buf, n):
        C.memmove(buf, rng_bytes(n), n)

    fn = RNG_FN(cb)
    lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
    W = np.ascontiguousarray(W, dtype=np.uint64)
    rows = np.zeros((max(row_hi - row_lo, 0), param.dblock, elt_words(field)), dtype=np.uint64)
    nonces = np.zeros((param.block_ext, 32), dtype=np.uint8)
    rc = L.lfgpu_ligero_layout_rows(field, subfield_log_bits, C.byref(param), C.c_void_p(W.ctypes.data) if W.size else None, subfield_boundary,
                                    C.c_void_p(lq.ctypes.data) if lq.size else None, fn, None, row_lo, row_hi,
                                    C.c_void_p(rows.ctypes.data) if rows.size else None, C.c_void_p(nonces.ctypes.data))
    if rc != 0:
        raise LfGpuError("lfgpu error %d: lfgpu_ligero_layout_rows" % rc)
    return rows, nonces


class LigeroProver:
    """Mirror of LigeroProver<Field, InterpolatorFactory> (reference lib/ligero/ligero_prover.h:34-359)
    over the C ABI: the tableau lives in HBM; the caller owns the transcript and the RandomEngine.
    `rng_bytes(n) -> bytes` plays RandomEngine::bytes.  Elements are (n, 2) uint64 arrays for GF(2^128) and Fp128 and (n, 4) --
    32-byte Montgomery images -- for FIELD_P256, which commit, low_degree_proof, dot_proof, quadratic_proof, open and prove serve
    (the sharded, slab and sparse forms and commit_batch are for the 16-byte fields; commit_batch256, prove_batch256 and
    open_batch256 are the batch of FIELD_P256 provers)."""

    def __init__(self, gpu, field, param, subfield_log_bits=4):
        self.gpu, self.field, self.p, self.k = gpu, field, param, subfield_log_bits
        self.ew = elt_words(field)
        self.h = None

    def commit(self, W, subfield_boundary, lqc, rng_bytes):
        """returns the 32-byte commitment root (LigeroProver::commit, :58-79, without ts.write)"""
        import numpy as np
        gpu = self.gpu

        def cb(_user, buf, n):
            data = rng_bytes(n)
            C.memmove(buf, data, n)

        self._cb = RNG_FN(cb)
        lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
        W = np.ascontiguousarray(W)
        root = (C.c_uint8 * 32)()
        h = C.c_void_p()
        gpu._ck(gpu.L.lfgpu_ligero_commit(gpu.h, self.field, self.k, C.byref(self.p), C.c_void_p(W.ctypes.data),
                                           subfield_boundary, C.c_void_p(lq.ctypes.data) if lq.size else None,
                                           self._cb, None, root, C.byref(h)))
        self.h = h
        return bytes(root)

    @staticmethod
    def commit_batch(gpu, field, param, Ws, subfield_boundary, lqc, rng_bytes_list, subfield_log_bits=4):
        """lfgpu_ligero_commit_batch: len(Ws) commits of one LigeroParam and one lqc through one chain of dispatches, statement b
        with witness Ws[b] and RandomEngine rng_bytes_list[b] (the same callable may appear more than once: the draws then
        come in index order) -> ([root], [LigeroProver]); the provers are ordinary ones"""
        import numpy as np
        nb = len(Ws)
        if len(rng_bytes_list) != nb:
            raise ValueError("LigeroProver.commit_batch: one RandomEngine per witness")

        def mk(rng_bytes):
            def cb(_user, buf, n):
                C.memmove(buf, rng_bytes(n), n)
            return RNG_FN(cb)

        cbs = [mk(r) for r in rng_bytes_list]
        lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
        Ws = [np.ascontiguousarray(W) for W in Ws]
        n = max(1, nb)
        roots = (C.c_uint8 * (32 * n))()
        hs = (C.c_void_p * n)()
        gpu._ck(gpu.L.lfgpu_ligero_commit_batch(gpu.h, field, subfield_log_bits, C.byref(param), nb, (C.c_void_p * n)(*[W.ctypes.data for W in Ws]),
                                                 subfield_boundary, C.c_void_p(lq.ctypes.data) if lq.size else None, (RNG_FN * n)(*cbs), None, roots, hs))
        raw = bytes(roots)
        provers = []
        for b in range(nb):
            pr = LigeroProver(gpu, field, param, subfield_log_bits)
            pr.h, pr._cb = C.c_void_p(hs[b]), cbs[b]
            provers.append(pr)
        return [raw[32 * b:32 * b + 32] for b in range(nb)], provers

    @staticmethod
    def commit_batch256(gpu, param, Ws, lqc, rng_bytes_list):
        """lfgpu_ligero_commit_batch256: commit_batch over FIELD_P256 (Ws[b]: (nw, 4) Montgomery images) -> ([root], [LigeroProver]);
        the provers are of the kind commit(FIELD_P256) returns"""
        import numpy as np
        nb = len(Ws)
        if len(rng_bytes_list) != nb:
            raise ValueError("LigeroProver.commit_batch256: one RandomEngine per witness")

        def mk(rng_bytes):
            def cb(_user, buf, n):
                C.memmove(buf, rng_bytes(n), n)
            return RNG_FN(cb)

        cbs = [mk(r) for r in rng_bytes_list]
        lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
        Ws = [np.ascontiguousarray(W) for W in Ws]
        n = max(1, nb)
        roots = (C.c_uint8 * (32 * n))()
        hs = (C.c_void_p * n)()
        gpu._ck(gpu.L.lfgpu_ligero_commit_batch256(gpu.h, C.byref(param), nb, (C.c_void_p * n)(*[W.ctypes.data for W in Ws]),
                                                    C.c_void_p(lq.ctypes.data) if lq.size else None, (RNG_FN * n)(*cbs), None, roots, hs))
        raw = bytes(roots)
        provers = []
        for b in range(nb):
            pr = LigeroProver(gpu, FIELD_P256, param)
            pr.h, pr._cb = C.c_void_p(hs[b]), cbs[b]
            provers.append(pr)
        return [raw[32 * b:32 * b + 32] for b in range(nb)], provers

    @staticmethod
    def prove_batch(gpu, provers, u_ldt, d_dense, ndense, scales, idxs, vals, u_quad, _ew=2):
        """lfgpu_ligero_prove_batch: the low-degree, dot (sparse form) and quadratic proofs of len(provers) committed provers of
        one LigeroParam in one chain of dispatches.  u_ldt: [nb][nwqrow] elements; d_dense: one device pointer per statement (or
        None when ndense == 0); scales: [nb] elements; idxs[b] / vals[b]: statement b's sparse list (may be empty); u_quad:
        [nb][nqtriples] elements -> (y_ldt [nb][block], y_dot [nb][dblock], y_q0 [nb][r], y_q2 [nb][dblock - block])"""
        import numpy as np
        nb = len(provers)
        p = provers[0].p if nb else LigeroParam()
        n = max(1, nb)
        u = np.ascontiguousarray(u_ldt, dtype=np.uint64)
        uq = np.ascontiguousarray(u_quad, dtype=np.uint64)
        sc = np.ascontiguousarray(scales, dtype=np.uint64)
        ix = [np.ascontiguousarray(i, dtype=np.uint64) for i in idxs]
        vl = [np.ascontiguousarray(v, dtype=np.uint64) for v in vals]
        if len(ix) != nb or len(vl) != nb:
            raise ValueError("LigeroProver.prove_batch: one sparse list per prover")
        y_ldt = np.zeros((n, p.block, _ew), dtype=np.uint64)
        y_dot = np.zeros((n, p.dblock, _ew), dtype=np.uint64)
        y_q0 = np.zeros((n, p.r, _ew), dtype=np.uint64)
        y_q2 = np.zeros((n, p.dblock - p.block, _ew), dtype=np.uint64)
        dd = (C.c_void_p * n)(*(d_dense if d_dense is not None else [None] * nb))
        fn = gpu.L.lfgpu_ligero_prove_batch256 if _ew == 4 else gpu.L.lfgpu_ligero_prove_batch
        gpu._ck(fn(
            gpu.h, (C.c_void_p * n)(*[pr.h.value if pr.h else None for pr in provers]), nb, C.c_void_p(u.ctypes.data), dd, ndense,
            C.c_void_p(sc.ctypes.data), (C.c_void_p * n)(*[i.ctypes.data if i.size else None for i in ix]),
            (C.c_void_p * n)(*[v.ctypes.data if v.size else None for v in vl]), (C.c_size_t * n)(*[len(i) for i in ix]),
            C.c_void_p(uq.ctypes.data) if uq.size else None, C.c_void_p(y_ldt.ctypes.data), C.c_void_p(y_dot.ctypes.data), C.c_void_p(y_q0.ctypes.data),
            C.c_void_p(y_q2.ctypes.data)))
        return y_ldt[:nb], y_dot[:nb], y_q0[:nb], y_q2[:nb]

    @staticmethod
    def open_batch(gpu, provers, idxs, path_cap=None, _ew=2):
        """lfgpu_ligero_open_batch: open() of every prover with its own nreq indices idxs[b] in one column gather, one digest gather
        and one read-back -> [(req[nrow][nreq], nonces[nreq], path digests)] per statement.  path_cap: digests of room per
        statement (default: the most a statement can need)"""
        import numpy as np
        nb = len(provers)
        p = provers[0].p if nb else LigeroParam()
        n = max(1, nb)
        flat = [int(j) for i in idxs for j in i]
        if len(flat) != nb * p.nreq:
            raise ValueError("LigeroProver.open_batch: nreq indices per prover")
        req = np.zeros((n, p.nrow, p.nreq, _ew), dtype=np.uint64)
        nonces = np.zeros((n, p.nreq, 32), dtype=np.uint8)
        cap = p.nreq * p.mc_pathlen + 1 if path_cap is None else path_cap
        path = np.zeros((n, max(1, cap), 32), dtype=np.uint8)
        npath = (C.c_size_t * n)()
        fn = gpu.L.lfgpu_ligero_open_batch256 if _ew == 4 else gpu.L.lfgpu_ligero_open_batch
        gpu._ck(fn(gpu.h, (C.c_void_p * n)(*[pr.h.value if pr.h else None for pr in provers]), nb,
                   (C.c_size_t * max(1, len(flat)))(*flat), C.c_void_p(req.ctypes.data), C.c_void_p(nonces.ctypes.data),
                   C.c_void_p(path.ctypes.data), cap, npath))
        return [(req[b], nonces[b], [bytes(path[b, i]) for i in range(npath[b])]) for b in range(nb)]

    @staticmethod
    def prove_batch256(gpu, provers, u_ldt, d_dense, ndense, scales, idxs, vals, u_quad):
        """lfgpu_ligero_prove_batch256: prove_batch for provers committed over FIELD_P256; every element is a row of 4 uint64 (a
        32-byte Montgomery image), d_dense[b] points at 32-byte elements"""
        return LigeroProver.prove_batch(gpu, provers, u_ldt, d_dense, ndense, scales, idxs, vals, u_quad, _ew=4)

    @staticmethod
    def open_batch256(gpu, provers, idxs, path_cap=None):
        """lfgpu_ligero_open_batch256: open_batch for provers committed over FIELD_P256 (req: [nrow][nreq][4])"""
        return LigeroProver.open_batch(gpu, provers, idxs, path_cap, _ew=4)

    def low_degree_proof(self, u_ldt):
        import numpy as np
        y = np.zeros((self.p.block, self.ew), dtype=np.uint64)
        u = np.ascontiguousarray(u_ldt)
        self.gpu._ck(self.gpu.L.lfgpu_ligero_low_degree_proof(self.h, C.c_void_p(u.ctypes.data), C.c_void_p(y.ctypes.data)))
        return y

    def dot_proof(self, A):
        import numpy as np
        y = np.zeros((self.p.dblock, self.ew), dtype=np.uint64)
        A = np.ascontiguousarray(A)
        self.gpu._ck(self.gpu.L.lfgpu_ligero_dot_proof(self.h, C.c_void_p(A.ctypes.data), C.c_void_p(y.ctypes.data)))
        return y

    def dot_proof_sparse(self, d_dense, ndense, scale, idx, val):
        """dot_proof with A built on the device: A[t] = scale * d_dense[t] (device pointer), A[idx] += val."""
        import numpy as np
        y = np.zeros((self.p.dblock, 2), dtype=np.uint64)
        sc = np.ascontiguousarray(scale, dtype=np.uint64)
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        val = np.ascontiguousarray(val, dtype=np.uint64)
        self.gpu._ck(self.gpu.L.lfgpu_ligero_dot_proof_sparse(self.h, C.c_void_p(d_dense), ndense, C.c_void_p(sc.ctypes.data),
                                                              C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), len(idx),
                                                              C.c_void_p(y.ctypes.data)))
        return y

    def quadratic_proof(self, u_quad):
        import numpy as np
        y0 = np.zeros((self.p.r, self.ew), dtype=np.uint64)
        y2 = np.zeros((self.p.dblock - self.p.block, self.ew), dtype=np.uint64)
        u = np.ascontiguousarray(u_quad)
        self.gpu._ck(self.gpu.L.lfgpu_ligero_quadratic_proof(self.h, C.c_void_p(u.ctypes.data) if u.size else None,
                                                             C.c_void_p(y0.ctypes.data), C.c_void_p(y2.ctypes.data)))
        return y0, y2

    def open(self, idx, rows=None):
        """compute_req + MerkleCommitment::open -> (req[nrow][nreq], nonces[nreq], path digests); a slab prover
        (parallel.GpuEngine.slab_prover) returns its own `rows` rows of req"""
        import numpy as np
        p = self.p
        idx_a = (C.c_size_t * p.nreq)(*idx)
        req = np.zeros((p.nrow if rows is None else rows, p.nreq, self.ew), dtype=np.uint64)
        nonces = np.zeros((p.nreq, 32), dtype=np.uint8)
        cap = p.nreq * p.mc_pathlen + 1
        path = np.zeros((cap, 32), dtype=np.uint8)
        npath = C.c_size_t()
        self.gpu._ck(self.gpu.L.lfgpu_ligero_open(self.h, idx_a, C.c_void_p(req.ctypes.data), C.c_void_p(nonces.ctypes.data),
                                                  C.c_void_p(path.ctypes.data), cap, C.byref(npath)))
        return req, nonces, [bytes(path[i]) for i in range(npath.value)]

    def prove(self, ts, nl, llterm, hash_of_llterm, lqc):
        """LigeroProver::prove (:84-146) -> the write_com_proof bytes.  ts: a transcript with .ops() (FsTranscript) that already
        holds the commitment root; llterm: llterm_array's input (FIELD_P256: llterm256_array's, through lfgpu_ligero_prove256),
        any order, duplicates allowed; lqc as at commit."""
        import numpy as np
        gpu = self.gpu
        p256 = self.field == FIELD_P256
        fn = gpu.L.lfgpu_ligero_prove256 if p256 else gpu.L.lfgpu_ligero_prove
        ll = llterm256_array(llterm) if p256 else llterm_array(llterm)
        lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
        ops = ts.ops()
        h = bytes(hash_of_llterm)
        n = C.c_size_t()
        args = (self.h, C.byref(ops) if ops is not None else None, nl, len(ll), C.c_void_p(ll.ctypes.data) if len(ll) else None, h,
                C.c_void_p(lq.ctypes.data) if lq.size else None)
        gpu._ck(fn(*args, None, 0, C.byref(n)))  # proves and reports the size
        buf = C.create_string_buffer(n.value)
        gpu._ck(fn(*args, buf, n.value, C.byref(n)))  # copies the held bytes
        return buf.raw[:n.value]

    def tableau_ptr(self):
        d = C.c_void_p()
        self.gpu._ck(self.gpu.L.lfgpu_ligero_tableau(self.h, C.byref(d)))
        return d.value

    def close(self):
        if self.h:
            self.gpu.L.lfgpu_ligero_free(self.h)
            self.h = None


class Quad:
    """One sumcheck layer resident on the device (mirror of Quad<Field>, reference
    lib/sumcheck/quad.h:55-226): eval (ProverLayers::eval_quad) and bind_g."""

    def __init__(self, gpu, field, g, h0, h1, vi, kvec, nv):
        import numpy as np
        self.gpu, self.field, self.n, self.nv = gpu, field, len(g), nv
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (g, h0, h1, vi)]
        kvec = np.ascontiguousarray(kvec)
        h = C.c_void_p()
        gpu._ck(gpu.L.lfgpu_quad_upload(gpu.h, field, self.n, *[C.c_void_p(a.ctypes.data) for a in arrs], len(kvec),
                                        C.c_void_p(kvec.ctypes.data), nv, C.byref(h)))
        self.h = h

    def eval(self, nw, d_W, d_V):
        ok = C.c_int()
        self.gpu._ck(self.gpu.L.lfgpu_eval_quad(self.h, nw, C.c_void_p(d_W), C.c_void_p(d_V), C.byref(ok)))
        return bool(ok.value)

    def eval_copies(self, nc, nw, d_W, d_V):
        """ProverLayers::eval_quad over nc copies: W[h * nc + c] -> V[g * nc + c]; False if an assert-zero term fails in any copy"""
        ok = C.c_int()
        self.gpu._ck(self.gpu.L.lfgpu_eval_quad_copies(self.h, nc, nw, C.c_void_p(d_W), C.c_void_p(d_V), C.byref(ok)))
        return bool(ok.value)

    def eval_batch(self, nb, nw, d_W, ldw, d_V, ldv):
        """ProverLayers::eval_quad for nb statements in one launch: statement b reads d_W + b * ldw and writes d_V + b * ldv
        (elements) -> [bool] * nb, False where an assert-zero term of that statement fails"""
        ok = (C.c_int * max(1, nb))()
        self.gpu._ck(self.gpu.L.lfgpu_eval_quad_batch(self.h, nb, nw, C.c_void_p(d_W), ldw, C.c_void_p(d_V), ldv, ok))
        return [bool(ok[b]) for b in range(nb)]

    def bind_g(self, logv, G0, G1, alpha, beta, d_hc_out, d_vc_out):
        import numpy as np
        G0, G1 = np.ascontiguousarray(G0), np.ascontiguousarray(G1)
        n_out = C.c_size_t()
        self.gpu._ck(self.gpu.L.lfgpu_quad_bind_g(self.h, logv, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data),
                                                  _u64x2(alpha), _u64x2(beta), C.c_void_p(d_hc_out), C.c_void_p(d_vc_out),
                                                  C.byref(n_out)))
        return n_out.value

    def bind_gh_all(self, logv, G0, G1, alpha, beta, logw, nw, H0, H1):
        """Quad::bind_gh_all (the verifier's combined bind) -> (lo, hi)"""
        import numpy as np
        G0, G1, H0, H1 = (np.ascontiguousarray(a) for a in (G0, G1, H0, H1))
        out = (C.c_uint64 * 2)()
        self.gpu._ck(self.gpu.L.lfgpu_quad_bind_gh_all(self.h, logv, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data),
                                                       _u64x2(alpha), _u64x2(beta), logw, nw, C.c_void_p(H0.ctypes.data),
                                                       C.c_void_p(H1.ctypes.data), out))
        return (out[0], out[1])

    def sumcheck_layer(self, logv, G0, G1, alpha, beta, logw, nw, d_W, wc_in, round_cb):
        """ProverLayers::layer (logc = 0) incl. bind_g; round_cb(hand, round, evals[3]) -> challenge, evals and
        challenge as (lo, hi) pairs.  Returns (wc_out[2], challenges[2][logw], bound_quad)."""
        import numpy as np
        G0, G1 = np.ascontiguousarray(G0), np.ascontiguousarray(G1)

        def cb(_user, hand, rnd, evals, out):
            ev = [(evals[2 * k], evals[2 * k + 1]) for k in range(3)]
            r = round_cb(hand, rnd, ev)
            out[0], out[1] = int(r[0]), int(r[1])

        cfn = SC_ROUND_FN(cb)
        wci = (C.c_uint64 * 4)(int(wc_in[0][0]), int(wc_in[0][1]), int(wc_in[1][0]), int(wc_in[1][1]))
        wco = (C.c_uint64 * 4)()
        gout = (C.c_uint64 * (4 * max(1, logw)))()
        bq = (C.c_uint64 * 2)()
        self.gpu._ck(self.gpu.L.lfgpu_sumcheck_layer(self.h, logv, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data),
                                                     _u64x2(alpha), _u64x2(beta), logw, nw, C.c_void_p(d_W), wci, cfn, None,
                                                     wco, gout, bq))
        ch = [[(gout[(h * logw + r) * 2], gout[(h * logw + r) * 2 + 1]) for r in range(logw)] for h in range(2)]
        return [(wco[0], wco[1]), (wco[2], wco[3])], ch, (bq[0], bq[1])

    def sumcheck_layer_copies(self, logc, nc, Q, logv, G0, G1, alpha, beta, logw, nw, d_W, wc_in, round_c_cb, round_cb):
        """ProverLayers::layer with nc copies incl. the Eqs constructor and bind_g; d_W: [nw][nc] on the device (consumed).
        round_c_cb(round, evals[4]) -> challenge for the logc copy rounds, round_cb(hand, round, evals[3]) -> challenge for
        the hand rounds.  Returns (wc_out[2], q_out[logc], challenges[2][logw], bound_quad)."""
        import numpy as np
        G0, G1 = np.ascontiguousarray(G0), np.ascontiguousarray(G1)
        Q = np.ascontiguousarray(Q, dtype=np.uint64)

        def cbc(_user, rnd, evals, out):
            r = round_c_cb(rnd, [(evals[2 * k], evals[2 * k + 1]) for k in range(4)])
            out[0], out[1] = int(r[0]), int(r[1])

        def cb(_user, hand, rnd, evals, out):
            r = round_cb(hand, rnd, [(evals[2 * k], evals[2 * k + 1]) for k in range(3)])
            out[0], out[1] = int(r[0]), int(r[1])

        cfc, cfn = SC_ROUND_C_FN(cbc), SC_ROUND_FN(cb)
        wci = (C.c_uint64 * 4)(int(wc_in[0][0]), int(wc_in[0][1]), int(wc_in[1][0]), int(wc_in[1][1]))
        wco = (C.c_uint64 * 4)()
        qout = (C.c_uint64 * (2 * max(1, logc)))()
        gout = (C.c_uint64 * (4 * max(1, logw)))()
        bq = (C.c_uint64 * 2)()
        self.gpu._ck(self.gpu.L.lfgpu_sumcheck_layer_copies(self.h, logc, nc, C.c_void_p(Q.ctypes.data) if logc else None, logv,
                                                            C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data), _u64x2(alpha),
                                                            _u64x2(beta), logw, nw, C.c_void_p(d_W), wci, cfc, cfn, None, wco, qout,
                                                            gout, bq))
        ch = [[(gout[(h * logw + r) * 2], gout[(h * logw + r) * 2 + 1]) for r in range(logw)] for h in range(2)]
        return [(wco[0], wco[1]), (wco[2], wco[3])], [(qout[2 * r], qout[2 * r + 1]) for r in range(logc)], ch, (bq[0], bq[1])

    def sumcheck_layer_batch(self, logv, G0, G1, alphas, betas, logw, nw, d_W, ldw, wc_ins, round_cb):
        """ProverLayers::layer (logc = 0) incl. bind_g for B = len(alphas) statements of this quad in lock-step.  G0, G1:
        [B][logv] elements; alphas, betas: B (lo, hi) pairs; d_W: statement b's nw wires at d_W + b * ldw elements (device,
        consumed); wc_ins: B pairs of (lo, hi) pairs.  round_cb(hand, round, evals) is called once per round-hand with
        evals[b] = the 3 evaluations of statement b as (lo, hi) pairs and returns B (lo, hi) challenges.
        Returns (wc_out[B], challenges[B][2][logw], bound_quad[B])."""
        import numpy as np
        B = len(alphas)
        G0, G1 = np.ascontiguousarray(G0, dtype=np.uint64), np.ascontiguousarray(G1, dtype=np.uint64)

        def cb(_user, hand, rnd, nb, evals, out):
            ev = [tuple((evals[6 * b + 2 * k], evals[6 * b + 2 * k + 1]) for k in range(3)) for b in range(nb)]
            rs = round_cb(hand, rnd, ev)
            for b in range(nb):
                out[2 * b], out[2 * b + 1] = int(rs[b][0]), int(rs[b][1])

        cfn = SC_ROUND_BATCH_FN(cb)
        n = max(1, B)
        al = (C.c_uint64 * (2 * n))(*[int(x) for a in alphas for x in _u64x2(a)])
        be = (C.c_uint64 * (2 * n))(*[int(x) for a in betas for x in _u64x2(a)])
        wci = (C.c_uint64 * (4 * n))(*[int(x) for w in wc_ins for e in w for x in e])
        wco = (C.c_uint64 * (4 * n))()
        gout = (C.c_uint64 * (4 * n * max(1, logw)))()
        bq = (C.c_uint64 * (2 * n))()
        self.gpu._ck(self.gpu.L.lfgpu_sumcheck_layer_batch(self.h, B, logv, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data), al, be,
                                                           logw, nw, C.c_void_p(d_W), ldw, wci, cfn, None, wco, gout, bq))
        ch = [[[(gout[((b * 2 + h) * logw + r) * 2], gout[((b * 2 + h) * logw + r) * 2 + 1]) for r in range(logw)] for h in range(2)]
              for b in range(B)]
        return ([[(wco[4 * b], wco[4 * b + 1]), (wco[4 * b + 2], wco[4 * b + 3])] for b in range(B)], ch,
                [(bq[2 * b], bq[2 * b + 1]) for b in range(B)])

    # ---- Fp256Base (field 1): elements are 4-word tuples (Montgomery images, little-endian words)
    def eval_quad_batch256(self, nb, nw, d_W, ldw, d_V, ldv):
        """eval_batch over Fp256Base (32-byte elements) -> [bool] * nb"""
        ok = (C.c_int * max(1, nb))()
        self.gpu._ck(self.gpu.L.lfgpu_eval_quad_batch256(self.h, nb, nw, C.c_void_p(d_W), ldw, C.c_void_p(d_V), ldv, ok))
        return [bool(ok[b]) for b in range(nb)]

    def sumcheck_layer256(self, logv, G0, G1, alpha, beta, logw, nw, d_W, wc_in, round_cb):
        """sumcheck_layer over Fp256Base: G0, G1: [logv][4] words; alpha, beta, the claims, evaluations and challenges are
        4-word tuples.  d_W is left intact.  Returns (wc_out[2], challenges[2][logw], bound_quad)."""
        import numpy as np
        G0, G1 = np.ascontiguousarray(G0, dtype=np.uint64), np.ascontiguousarray(G1, dtype=np.uint64)

        def cb(_user, hand, rnd, evals, out):
            r = round_cb(hand, rnd, [tuple(evals[4 * k + j] for j in range(4)) for k in range(3)])
            for j in range(4):
                out[j] = int(r[j])

        cfn = SC_ROUND256_FN(cb)
        wci = (C.c_uint64 * 8)(*[int(x) for e in wc_in for x in e])
        wco = (C.c_uint64 * 8)()
        gout = (C.c_uint64 * (8 * max(1, logw)))()
        bq = (C.c_uint64 * 4)()
        self.gpu._ck(self.gpu.L.lfgpu_sumcheck_layer256(self.h, logv, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data),
                                                        _u64x4(alpha), _u64x4(beta), logw, nw, C.c_void_p(d_W), wci, cfn, None, wco, gout, bq))
        ch = [[tuple(gout[(h * logw + r) * 4 + j] for j in range(4)) for r in range(logw)] for h in range(2)]
        return [tuple(wco[0:4]), tuple(wco[4:8])], ch, tuple(bq)

    def sumcheck_layer_batch256(self, logv, G0, G1, alphas, betas, logw, nw, d_W, ldw, wc_ins, round_cb):
        """sumcheck_layer_batch over Fp256Base for B = len(alphas) statements: G0, G1: [B][logv][4] words; alphas, betas: B
        4-word tuples; d_W: statement b's nw wires at d_W + b * ldw 32-byte elements (device, left intact); wc_ins: B pairs
        of 4-word tuples.  round_cb(hand, round, evals) gets evals[b] = 3 4-word tuples and returns B 4-word challenges.
        Returns (wc_out[B], challenges[B][2][logw], bound_quad[B])."""
        import numpy as np
        B = len(alphas)
        G0, G1 = np.ascontiguousarray(G0, dtype=np.uint64), np.ascontiguousarray(G1, dtype=np.uint64)

        def cb(_user, hand, rnd, nb, evals, out):
            ev = [tuple(tuple(evals[12 * b + 4 * k + j] for j in range(4)) for k in range(3)) for b in range(nb)]
            rs = round_cb(hand, rnd, ev)
            for b in range(nb):
                for j in range(4):
                    out[4 * b + j] = int(rs[b][j])

        cfn = SC_ROUND_BATCH256_FN(cb)
        n = max(1, B)
        al = (C.c_uint64 * (4 * n))(*[int(x) for a in alphas for x in a])
        be = (C.c_uint64 * (4 * n))(*[int(x) for a in betas for x in a])
        wci = (C.c_uint64 * (8 * n))(*[int(x) for w in wc_ins for e in w for x in e])
        wco = (C.c_uint64 * (8 * n))()
        gout = (C.c_uint64 * (8 * n * max(1, logw)))()
        bq = (C.c_uint64 * (4 * n))()
        self.gpu._ck(self.gpu.L.lfgpu_sumcheck_layer_batch256(self.h, B, logv, C.c_void_p(G0.ctypes.data), C.c_void_p(G1.ctypes.data), al, be,
                                                              logw, nw, C.c_void_p(d_W), ldw, wci, cfn, None, wco, gout, bq))
        ch = [[[tuple(gout[((b * 2 + h) * logw + r) * 4 + j] for j in range(4)) for r in range(logw)] for h in range(2)] for b in range(B)]
        return ([[tuple(wco[8 * b:8 * b + 4]), tuple(wco[8 * b + 4:8 * b + 8])] for b in range(B)], ch,
                [tuple(bq[4 * b:4 * b + 4]) for b in range(B)])

    def close(self):
        if self.h:
            self.gpu.L.lfgpu_quad_free(self.h)
            self.h = None


class FsTranscript:
    """The library's built-in Fiat-Shamir transcript (reference lib/random/transcript.h:33-190); host only."""

    def __init__(self, init=b""):
        self.L = load_library()
        self.h = self.L.lfgpu_transcript_new(bytes(init), len(init))
        if not self.h:
            raise LfGpuError("lfgpu_transcript_new failed")

    def write_bytes(self, data):
        self.L.lfgpu_transcript_write_bytes(self.h, bytes(data), len(data))

    def write_elt(self, e16):
        self.L.lfgpu_transcript_write_elt(self.h, bytes(e16))

    def write_array(self, elts):
        b = b"".join(bytes(e) for e in elts)
        self.L.lfgpu_transcript_write_elt_array(self.h, b, len(elts))

    def write_elt_sized(self, e):
        self.L.lfgpu_transcript_write_elt_sized(self.h, bytes(e), len(e))

    def write_array_sized(self, elts, nbytes):
        b = b"".join(bytes(e) for e in elts)
        self.L.lfgpu_transcript_write_elt_array_sized(self.h, b, len(elts), nbytes)

    def bytes(self, n):
        buf = C.create_string_buffer(n)
        self.L.lfgpu_transcript_bytes(self.h, buf, n)
        return buf.raw

    def ops(self):
        o = TranscriptOps()
        self.L.lfgpu_transcript_get_ops(self.h, C.byref(o))
        return o

    def close(self):
        if self.h:
            self.L.lfgpu_transcript_free(self.h)
            self.h = None


def sha256(data):
    out = C.create_string_buffer(32)
    load_library().lfgpu_sha256(bytes(data), len(data), out)
    return out.raw


def aes256_ecb_block(key, block):
    out = C.create_string_buffer(16)
    load_library().lfgpu_aes256_ecb_block(bytes(key), bytes(block), out)
    return out.raw


class Circuit:
    """A circuit parsed from the reference's LFC1 wire bytes, layers resident on the device (lfgpu_circuit)."""

    def __init__(self, gpu, lfc1_bytes, _shared_from=None):
        self.gpu = gpu
        h = C.c_void_p()
        if _shared_from is not None:
            gpu._ck(gpu.L.lfgpu_circuit_share(gpu.h, _shared_from.h, C.byref(h)))
        else:
            raw = bytes(lfc1_bytes)
            gpu._ck(gpu.L.lfgpu_circuit_from_lfc1(gpu.h, raw, len(raw), C.byref(h)))
        self.h = h
        self.info = CircuitInfo()
        gpu._ck(gpu.L.lfgpu_circuit_get_info(self.h, C.byref(self.info)))

    def share(self, gpu):
        """a handle on the same device-resident circuit for another context of the same device (lfgpu_circuit_share)"""
        return Circuit(gpu, None, _shared_from=self)

    def layer(self, i):
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.gpu._ck(self.gpu.L.lfgpu_circuit_layer_info(self.h, i, C.byref(a), C.byref(b), C.byref(c)))
        return dict(logw=a.value, nw=b.value, nterms=c.value)

    def close(self):
        if self.h:
            self.gpu.L.lfgpu_circuit_free(self.h)
            self.h = None


class ZkProver:
    """Mirror of ZkProver<Field, RSFactory> (reference lib/zk/zk_prover.h:45-149) over include/lfgpu_zk.h: the whole
    host control flow runs in the library's C++; `rng_bytes(n) -> bytes` plays the RandomEngine."""

    def __init__(self, gpu, circuit, rate=7, nreq=132, block_enc=0):
        self.gpu, self.circuit = gpu, circuit
        h = C.c_void_p()
        gpu._ck(gpu.L.lfgpu_zk_prover_new(gpu.h, circuit.h, rate, nreq, block_enc, C.byref(h)))
        self.h = h
        self.param = LigeroParam()
        gpu._ck(gpu.L.lfgpu_zk_prover_param(self.h, C.byref(self.param)))

    def set_comm(self, comm, min_tableau_bytes=0):
        """lfgpu_zk_prover_set_comm: `comm` = parallel.TorchComm (or None); tableaux of at least min_tableau_bytes are
        committed with their rows sharded over the communicator's GPUs, smaller ones replicated"""
        self._comm = comm
        self.gpu._ck(self.gpu.L.lfgpu_zk_prover_set_comm(self.h, C.byref(comm.ops) if comm is not None else None, min_tableau_bytes))

    def commit(self, W, rng_bytes, transcript):
        import numpy as np

        def cb(_user, buf, n):
            C.memmove(buf, rng_bytes(n), n)

        self._cb = RNG_FN(cb)
        W = np.ascontiguousarray(W)
        root = (C.c_uint8 * 32)()
        ops = transcript.ops()
        self.gpu._ck(self.gpu.L.lfgpu_zk_commit(self.h, C.c_void_p(W.ctypes.data), self._cb, None, C.byref(ops), root))
        return bytes(root)

    def prove(self, W, transcript):
        """-> True (proof held by the object; wire() serializes it) or False (witness does not satisfy the circuit)"""
        import numpy as np
        W = np.ascontiguousarray(W)
        ok = C.c_int()
        ops = transcript.ops()
        self.gpu._ck(self.gpu.L.lfgpu_zk_prove(self.h, C.c_void_p(W.ctypes.data), C.byref(ops), C.byref(ok)))
        return bool(ok.value)

    def wire(self):
        """ZkProof::write bytes"""
        n = C.c_size_t()
        self.gpu._ck(self.gpu.L.lfgpu_zk_proof_write(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self.gpu._ck(self.gpu.L.lfgpu_zk_proof_write(self.h, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def timings(self):
        ms = (C.c_double * 6)()
        self.gpu._ck(self.gpu.L.lfgpu_zk_timings(self.h, ms))
        return dict(zip(("commit", "prove", "eval_circuit", "sumcheck", "constraints", "ligero_prove"), list(ms)))

    def close(self):
        if self.h:
            self.gpu.L.lfgpu_zk_prover_free(self.h)
            self.h = None


class ZkBatch:
    """lfgpu_zk_batch: up to nb_max committed ZkProvers of one context and circuit proved in lock-step through one chain of
    dispatches (batched eval_circuit and sumcheck; one EQ launch, one lfgpu_ligero_prove_batch and one
    lfgpu_ligero_open_batch for the Ligero proofs of all statements; LFGPU_LIGERO_PROVE_BATCH=0 runs that tail per statement).
    Every proof is byte-identical to ZkProver.prove's.  GF2_128 and Fp128 circuits."""

    def __init__(self, gpu, circuit, nb_max):
        self.gpu, self.circuit, self.nb_max = gpu, circuit, nb_max
        h = C.c_void_p()
        gpu._ck(gpu.L.lfgpu_zk_batch_new(gpu.h, circuit.h, nb_max, C.byref(h)))
        self.h = h

    def commit(self, provers, Ws, rng_bytes_list, transcripts):
        """lfgpu_zk_commit_batch: ZkProver.commit for every prover through one chain of dispatches (one batched Ligero commit),
        statement b with its own witness, RandomEngine `rng_bytes_list[b](n) -> bytes` and transcript -> [root]"""
        import numpy as np
        nb = len(provers)
        if not (len(Ws) == nb and len(rng_bytes_list) == nb and len(transcripts) == nb):
            raise ValueError("ZkBatch.commit: one witness, one RandomEngine and one transcript per prover")

        def mk(rng_bytes):
            def cb(_user, buf, n):
                C.memmove(buf, rng_bytes(n), n)
            return RNG_FN(cb)

        cbs = [mk(r) for r in rng_bytes_list]
        Ws = [np.ascontiguousarray(W) for W in Ws]
        ops = [t.ops() for t in transcripts]
        n = max(1, nb)
        roots = (C.c_uint8 * (32 * n))()
        self.gpu._ck(self.gpu.L.lfgpu_zk_commit_batch(self.h, (C.c_void_p * n)(*[p.h for p in provers]), nb, (C.c_void_p * n)(*[W.ctypes.data for W in Ws]),
                                                      (RNG_FN * n)(*cbs), None, (C.POINTER(TranscriptOps) * n)(*[C.pointer(o) for o in ops]), roots))
        raw = bytes(roots)
        return [raw[32 * b:32 * b + 32] for b in range(nb)]

    def prove(self, provers, Ws, transcripts):
        """-> [bool] per statement: True = provers[b] holds its proof, False = witness b does not satisfy the circuit"""
        import numpy as np
        nb = len(provers)
        if not (len(Ws) == nb and len(transcripts) == nb):
            raise ValueError("ZkBatch.prove: one witness and one transcript per prover")
        Ws = [np.ascontiguousarray(W) for W in Ws]
        ops = [t.ops() for t in transcripts]
        n = max(1, nb)
        zk = (C.c_void_p * n)(*[p.h for p in provers])
        hw = (C.c_void_p * n)(*[W.ctypes.data for W in Ws])
        tp = (C.POINTER(TranscriptOps) * n)(*[C.pointer(o) for o in ops])
        ok = (C.c_int * n)()
        self.gpu._ck(self.gpu.L.lfgpu_zk_prove_batch(self.h, zk, nb, hw, tp, ok))
        return [bool(ok[b]) for b in range(nb)]

    def close(self):
        if self.h:
            self.gpu.L.lfgpu_zk_batch_free(self.h)
            self.h = None


class ZkBatch256:
    """lfgpu_zk_batch256: ZkBatch for circuits over FIELD_P256 -- up to nb_max committed ZkProvers of one context and one Fp256Base
    circuit proved in lock-step (batched eval_circuit and sumcheck; one EQ launch chain, one lfgpu_ligero_prove_batch256 and one
    lfgpu_ligero_open_batch256 for the Ligero proofs of all statements; LFGPU_LIGERO_PROVE_BATCH256=0 runs that tail per
    statement).  Every proof is byte-identical to ZkProver.prove's.  The provers commit one by one (ZkProver.commit) or all in one
    chain (commit: lfgpu_zk_commit_batch256, one lfgpu_ligero_commit_batch256; LFGPU_COMMIT_BATCH256=0 runs it per statement)."""

    def __init__(self, gpu, circuit, nb_max):
        self.gpu, self.circuit, self.nb_max = gpu, circuit, nb_max
        h = C.c_void_p()
        gpu._ck(gpu.L.lfgpu_zk_batch256_new(gpu.h, circuit.h, nb_max, C.byref(h)))
        self.h = h

    def commit(self, provers, Ws, rng_bytes_list, transcripts):
        """lfgpu_zk_commit_batch256: ZkProver.commit for every prover through one chain of dispatches (one batched Ligero commit),
        statement b with its own witness, RandomEngine `rng_bytes_list[b](n) -> bytes` and transcript -> [root]"""
        import numpy as np
        nb = len(provers)
        if not (len(Ws) == nb and len(rng_bytes_list) == nb and len(transcripts) == nb):
            raise ValueError("ZkBatch256.commit: one witness, one RandomEngine and one transcript per prover")

        def mk(rng_bytes):
            def cb(_user, buf, n):
                C.memmove(buf, rng_bytes(n), n)
            return RNG_FN(cb)

        cbs = [mk(r) for r in rng_bytes_list]
        Ws = [np.ascontiguousarray(W) for W in Ws]
        ops = [t.ops() for t in transcripts]
        n = max(1, nb)
        roots = (C.c_uint8 * (32 * n))()
        self.gpu._ck(self.gpu.L.lfgpu_zk_commit_batch256(self.h, (C.c_void_p * n)(*[p.h for p in provers]), nb, (C.c_void_p * n)(*[W.ctypes.data for W in Ws]),
                                                         (RNG_FN * n)(*cbs), None, (C.POINTER(TranscriptOps) * n)(*[C.pointer(o) for o in ops]), roots))
        raw = bytes(roots)
        return [raw[32 * b:32 * b + 32] for b in range(nb)]

    def prove(self, provers, Ws, transcripts):
        """-> [bool] per statement: True = provers[b] holds its proof, False = witness b does not satisfy the circuit"""
        import numpy as np
        nb = len(provers)
        if not (len(Ws) == nb and len(transcripts) == nb):
            raise ValueError("ZkBatch256.prove: one witness and one transcript per prover")
        Ws = [np.ascontiguousarray(W) for W in Ws]
        ops = [t.ops() for t in transcripts]
        n = max(1, nb)
        zk = (C.c_void_p * n)(*[p.h for p in provers])
        hw = (C.c_void_p * n)(*[W.ctypes.data for W in Ws])
        tp = (C.POINTER(TranscriptOps) * n)(*[C.pointer(o) for o in ops])
        ok = (C.c_int * n)()
        self.gpu._ck(self.gpu.L.lfgpu_zk_prove_batch256(self.h, zk, nb, hw, tp, ok))
        return [bool(ok[b]) for b in range(nb)]

    def close(self):
        if self.h:
            self.gpu.L.lfgpu_zk_batch256_free(self.h)
            self.h = None


def ligero_verify(gpu, field, p, root, proof, ts, nl, llterm, hash_of_llterm, b, lqc, subfield_log_bits=4):
    """LigeroVerifier::verify (reference lib/ligero/ligero_verifier.h:42-123) on the write_com_proof bytes -> (accepted, reason);
    ts: a transcript with .ops() that already holds the commitment root; b: the nl right-hand sides (Elt images)"""
    import numpy as np
    ll = llterm_array(llterm)
    lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
    b = np.ascontiguousarray(b)
    ok, why = C.c_int(), C.c_char_p()
    ops = ts.ops()
    raw = bytes(proof)
    gpu._ck(gpu.L.lfgpu_ligero_verify(gpu.h, field, subfield_log_bits, C.byref(p), bytes(root), raw, len(raw), C.byref(ops), nl, len(ll),
                                       C.c_void_p(ll.ctypes.data) if len(ll) else None, bytes(hash_of_llterm),
                                       C.c_void_p(b.ctypes.data) if b.size else None, C.c_void_p(lq.ctypes.data) if lq.size else None,
                                       C.byref(ok), C.byref(why)))
    return bool(ok.value), (why.value or b"").decode()


def ligero_verify256(gpu, p, root, proof, ts, nl, llterm, hash_of_llterm, b, lqc):
    """ligero_verify over Fp256Base (lfgpu_ligero_verify256): llterm as llterm256_array takes it, b the nl right-hand sides as
    32-byte Montgomery images; ts needs the sized element writes (FsTranscript has them)"""
    import numpy as np
    ll = llterm256_array(llterm)
    lq = np.ascontiguousarray(np.asarray(lqc, dtype=np.uint64).reshape(-1))
    b = np.ascontiguousarray(b)
    ok, why = C.c_int(), C.c_char_p()
    ops = ts.ops()
    raw = bytes(proof)
    gpu._ck(gpu.L.lfgpu_ligero_verify256(gpu.h, C.byref(p), bytes(root), raw, len(raw), C.byref(ops), nl, len(ll),
                                          C.c_void_p(ll.ctypes.data) if len(ll) else None, bytes(hash_of_llterm),
                                          C.c_void_p(b.ctypes.data) if b.size else None, C.c_void_p(lq.ctypes.data) if lq.size else None,
                                          C.byref(ok), C.byref(why)))
    return bool(ok.value), (why.value or b"").decode()


def zk_verify(gpu, circuit, proof, pub, transcript, rate=7, nreq=132, block_enc=0, committed=False):
    """ZkVerifier::recv_commitment + verify over the wire bytes -> (accepted, reason); committed=True: the caller has already
    written the commitment root to the transcript (ZkVerifier::recv_commitment as a separate step, as in run_mdoc_verifier)"""
    import numpy as np
    pub = np.ascontiguousarray(pub)
    ok, why = C.c_int(), C.c_char_p()
    ops = transcript.ops()
    raw = bytes(proof)
    fn = gpu.L.lfgpu_zk_verify_committed if committed else gpu.L.lfgpu_zk_verify
    gpu._ck(fn(gpu.h, circuit.h, rate, nreq, block_enc, raw, len(raw), C.c_void_p(pub.ctypes.data) if pub.size else None,
               C.byref(ops), C.byref(ok), C.byref(why)))
    return bool(ok.value), (why.value or b"").decode()
