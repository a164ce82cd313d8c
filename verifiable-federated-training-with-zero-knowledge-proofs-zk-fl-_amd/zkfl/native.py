"""ctypes binding of libzkfl.so (the C ABI declared in include/zkfl.h).

This is the Python twin of the N-API binding shown in INTEGRATION.md.  The library is built
in-tree (``make`` in the package directory, or ``__graft_entry__.build()``); if it is missing
every call raises ``ZkflError`` — there is no CPU fallback on the proving path.
"""

from __future__ import annotations

import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ZKFL_LIB: an alternative build of the library (A/B experiments); default the in-tree one
LIB_PATH = os.path.abspath(os.environ["ZKFL_LIB"]) if os.environ.get("ZKFL_LIB") else os.path.join(_PKG_DIR, "libzkfl.so")

ZKFL_OK = 0
# one shard's part of a split proof: A' | B1' | B2' | C' | H as XYZZ points (X, Y, ZZ, ZZZ), every
# coordinate std-form 32 B LE (G2: c0, c1); ZZ = 0 is infinity (include/zkfl.h)
PART_BYTES = 768
PART_LAYOUT = {"A": (0, 128), "B1": (128, 256), "B2": (256, 512), "C": (512, 640), "H": (640, 768)}
ERRORS = {
    -1: "ZKFL_E_ARG", -2: "ZKFL_E_FORMAT", -3: "ZKFL_E_PRIME", -4: "ZKFL_E_MISMATCH",
    -5: "ZKFL_E_DEVICE", -6: "ZKFL_E_OOM", -7: "ZKFL_E_CONSTRAINT", -8: "ZKFL_E_KEY",
}

_P = C.c_void_p
_U8P = C.POINTER(C.c_uint8)


class R1csHeader(C.Structure):
    """zkfl_r1cs_header: the counts of a .r1cs (n_terms: every term of its constraints section)."""
    _fields_ = [("n_wires", C.c_uint32), ("n_pub_out", C.c_uint32), ("n_pub_in", C.c_uint32),
                ("n_prv_in", C.c_uint32), ("n_constraints", C.c_uint32), ("n_labels", C.c_uint64),
                ("n_terms", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class R1csReport(C.Structure):
    """zkfl_r1cs_report"""
    _fields_ = [("n_failed", C.c_uint32), ("first", C.c_uint32), ("a", C.c_uint8 * 32), ("b", C.c_uint8 * 32),
                ("c", C.c_uint8 * 32)]


class PtauView(C.Structure):
    """zkfl_ptau_view: the ptau's Lagrange blocks at the circuit's power and its alpha / beta points."""
    _fields_ = [("power", C.c_uint32),
                ("L", C.c_char_p), ("L2", C.c_char_p), ("La", C.c_char_p), ("Lb", C.c_char_p), ("H0", C.c_char_p),
                ("L_len", C.c_size_t), ("L2_len", C.c_size_t), ("La_len", C.c_size_t), ("Lb_len", C.c_size_t),
                ("H0_len", C.c_size_t),
                ("alpha1", C.c_char_p), ("beta1", C.c_char_p), ("beta2", C.c_char_p)]


# zkfl_zkey_check's checks in the order they are reported, and a check's three states
KEY_CHECKS = ("header", "points", "coefficients", "A", "B1", "B2", "IC", "C", "H")
KEY_STATES = ("pass", "fail", "not run")


class ZkeyReport(C.Structure):
    """zkfl_zkey_report"""
    _fields_ = [("status", C.c_uint32 * len(KEY_CHECKS)),
                ("point_section", C.c_uint32), ("point_index", C.c_uint32), ("point_count", C.c_uint32),
                ("coef_matrix", C.c_uint32), ("coef_row", C.c_uint32), ("coef_count", C.c_uint32)]


# zkfl_ptau_check's checks in the order they are reported (their states are KEY_STATES)
PTAU_CHECKS = ("STRUCTURE", "POINTS", "TAU_G1", "TAU_G2", "ALPHA_G1", "BETA_G1", "BETA_G2",
               "L_TAU_G1", "L_TAU_G2", "L_ALPHA_G1", "L_BETA_G1")
PTAU_LAGRANGE_CHECKS = PTAU_CHECKS[7:]


class PtauHeader(C.Structure):
    """zkfl_ptau_header"""
    _fields_ = [("power", C.c_uint32), ("ceremony_power", C.c_uint32), ("prepared", C.c_uint32),
                ("contributions", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PtauReportC(C.Structure):
    """zkfl_ptau_report"""
    _fields_ = [("status", C.c_uint32 * len(PTAU_CHECKS)), ("prepared", C.c_uint32), ("power", C.c_uint32),
                ("point_section", C.c_uint32), ("point_index", C.c_uint32), ("point_count", C.c_uint32),
                ("chunks", C.c_uint32)]


GROUP_QUERIES = ("A", "B1", "B2", "CH")


class GroupsInfo(C.Structure):
    """zkfl_groups_info"""
    _fields_ = [("grouped", C.c_uint32), ("learned", C.c_uint32), ("groups", C.c_uint32), ("non_rep", C.c_uint32),
                ("bases", C.c_uint32 * 4), ("bases_rep", C.c_uint32 * 4), ("builds", C.c_uint32),
                ("last_miss", C.c_uint32), ("build_ms", C.c_double)]


class GroupRowsInfo(C.Structure):
    """zkfl_group_rows_info"""
    _fields_ = [("rows_grouped", C.c_uint32), ("row_classes", C.c_uint32), ("terms", C.c_uint32),
                ("terms_rep", C.c_uint32), ("wire_list", C.c_uint32), ("wires_over_cap", C.c_uint32),
                ("last_dirty", C.c_uint32), ("last_plain", C.c_uint32), ("rows_build_ms", C.c_double)]


class AdmitPhase(C.Structure):
    """zkfl_admit_phase"""
    _fields_ = [("present", _P), ("claimed", _P), ("signals", _P), ("proofs", _P)]


class AdmitRound(C.Structure):
    """zkfl_admit_round"""
    _fields_ = [("n", C.c_size_t), ("dim", C.c_uint32), ("ids", _P), ("round", _P), ("tau_squared", _P),
                ("vkeys", _P * 3), ("balance", AdmitPhase), ("training", AdmitPhase), ("secagg", AdmitPhase),
                ("gradients", _P), ("masked_update", _P), ("weights", _P), ("peer_ptr", _P), ("peer_ids", _P)]


class PrepareRound(C.Structure):
    """zkfl_prepare_round"""
    _fields_ = [("n", C.c_size_t), ("ids", _P), ("samples", C.c_uint32), ("dim", C.c_uint32), ("depth", C.c_uint32),
                ("batch", C.c_uint32), ("precision", C.c_uint32), ("peers", C.c_uint32), ("features", _P),
                ("labels", _P), ("batch_idx", _P), ("weights", _P), ("round", _P), ("tau_squared", C.c_uint64),
                ("peer_ids", _P), ("keys", _P), ("master_keys", _P)]


class PrepareOut(C.Structure):
    """zkfl_prepare_out"""
    _fields_ = [("balance_inputs", _P), ("training_inputs", _P), ("secagg_inputs", _P), ("roots", _P),
                ("gradients", _P), ("masked", _P), ("c1", _P), ("status", _P)]


PREPARE_OK, PREPARE_NORM = 0, 1                                                  # ZKFL_PREPARE_*
PREPARE_MAX_DIM, PREPARE_MAX_PEERS, MERKLE_MAX_DEPTH = 255, 15, 30
PREPARE_OUTPUTS = ("balance_inputs", "training_inputs", "secagg_inputs", "roots", "gradients", "masked", "c1",
                   "status")


def prepare_lengths(samples: int, dim: int, depth: int, batch: int, peers: int) -> dict:
    """The input counts of balance_unified(samples, depth, dim), sgd_verified(batch, dim, depth, .) and
    secure_masked_update(dim, peers)."""
    return {"balance": 5 + samples * dim + samples + 2 * samples * depth,
            "training": 6 + 5 * dim + batch * dim + batch + 2 * batch * depth,
            "secagg": 8 + 2 * dim + 2 * peers}


# ZKFL_ADMIT_*: a client's code per phase (0 = accepted, else the first failing check) and the flags
ADMIT_CODES = {
    0: "OK",
    1: "B_MISSING", 2: "B_SIG_ROOT_D", 3: "B_PROOF",
    16: "T_MISSING", 17: "T_NO_BALANCE", 18: "T_BIND_ROOT_D", 19: "T_SIG_ROOT_D", 20: "T_SIG_ROOT_G",
    21: "T_SIG_ROOT_W", 22: "T_SIG_ROUND", 23: "T_ROUND_STALE", 24: "T_SIG_TAU", 25: "T_ROOT_G_GRADIENT",
    26: "T_ROOT_W_MODEL", 27: "T_PROOF",
    32: "S_MISSING", 33: "S_NO_TRAINING", 34: "S_BIND_ROOT_G", 35: "S_BIND_ROOT_D", 36: "S_BIND_ROOT_W",
    37: "S_SIG_CLIENT_ID", 38: "S_SIG_ROUND", 39: "S_ROUND_STALE", 40: "S_SIG_ROOT_D", 41: "S_SIG_ROOT_G",
    42: "S_SIG_ROOT_W", 43: "S_SIG_ROOT_K", 44: "S_SIG_TAU", 45: "S_SIG_MASKED", 46: "S_SIG_PEERS", 47: "S_PROOF",
}
ADMIT_CHECK_ROUND, ADMIT_CHECK_MODEL, ADMIT_CHECK_PEERS, ADMIT_COMBINED = 1, 2, 4, 8
ADMIT_PHASES = ("balance", "training", "secagg")
ADMIT_FIELDS = {"balance": ("root_D",), "training": ("root_D", "root_G", "root_W", "round"),
                "secagg": ("root_D", "root_G", "root_W", "root_K", "round")}   # the claimed fields, in order
ADMIT_NPUBLIC = {"balance": 5, "training": 6, "secagg": 7}                      # secagg: 7 + dim + peers


# every exported symbol of include/zkfl.h with (restype, argtypes)
SIGNATURES = {
    "zkfl_version": (C.c_int, []),
    "zkfl_build_id": (C.c_char_p, []),
    "zkfl_last_error": (C.c_char_p, []),
    "zkfl_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "zkfl_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "zkfl_ctx_destroy": (C.c_int, [_P]),
    "zkfl_ctx_set_profiling": (C.c_int, [_P, C.c_int]),
    "zkfl_ctx_profile": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "zkfl_ctx_profile_reset": (C.c_int, [_P]),
    "zkfl_ctx_synchronize": (C.c_int, [_P]),
    "zkfl_zkey_load": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(_P)]),
    "zkfl_zkey_load_shard": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "zkfl_zkey_file_open": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "zkfl_zkey_load_file": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "zkfl_zkey_file_close": (C.c_int, [_P]),
    "zkfl_key_shard": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "zkfl_groth16_prove_part_batch": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(_P), C.c_char_p, _U8P]),
    "zkfl_groth16_assemble": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_char_p, C.c_char_p, _U8P]),
    "zkfl_key_free": (C.c_int, [_P]),
    "zkfl_key_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "zkfl_key_ab_shared": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "zkfl_debug_ab_partition": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _U8P]),
    "zkfl_key_set_groups": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_size_t]),
    "zkfl_key_learn_groups": (C.c_int, [_P, _P, _P]),
    "zkfl_key_groups": (C.c_int, [_P, C.POINTER(GroupsInfo)]),
    "zkfl_key_group_rows": (C.c_int, [_P, C.POINTER(GroupRowsInfo)]),
    "zkfl_debug_groups": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                    C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint32)]),
    "zkfl_debug_group_rows": (C.c_int, [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                        C.c_uint32] + [C.POINTER(C.c_uint32)] * 7),
    "zkfl_debug_abc": (C.c_int, [_P, _P, _P, C.c_int, _U8P, C.POINTER(C.c_uint32)]),
    "zkfl_key_set_slots": (C.c_int, [_P, C.c_int]),
    "zkfl_groth16_prove": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t, C.c_char_p, _U8P, _U8P,
                                     C.POINTER(C.c_size_t)]),
    "zkfl_witness_upload": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t, C.POINTER(_P)]),
    "zkfl_witness_free": (C.c_int, [_P]),
    "zkfl_groth16_prove_resident": (C.c_int, [_P, _P, _P, C.c_char_p, _U8P]),
    "zkfl_groth16_prove_batch": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(_P), C.c_char_p, _U8P]),
    "zkfl_debug_prove_parts": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t, _U8P, _U8P]),
    "zkfl_debug_glv_split": (C.c_int, [C.c_char_p, _U8P]),
    "zkfl_debug_g1_glv_mul": (C.c_int, [_P, C.c_size_t, C.c_char_p, C.c_char_p, C.c_char_p, _U8P]),
    "zkfl_debug_asm_ops": (C.c_int, [_P, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]),
    "zkfl_debug_msm_front": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                       C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_size_t), C.c_uint32, C.c_char_p, C.c_size_t, C.c_int, C.c_int,
                                       _U8P, _U8P]),
    "zkfl_debug_wtrace": (C.c_int, [_P, C.c_int, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    "zkfl_msm_g1": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_size_t, _U8P]),
    "zkfl_msm_g2": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_size_t, _U8P]),
    "zkfl_ntt_coset": (C.c_int, [_P, _U8P, C.c_uint32]),
    "zkfl_debug_ntt_coset": (C.c_int, [_P, _U8P, C.c_uint32, C.c_uint32, C.c_size_t, C.c_int]),
    "zkfl_debug_coset_join": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_int, _U8P]),
    "zkfl_setup_g1_gen_mul": (C.c_int, [_P, C.c_char_p, C.c_size_t, _U8P]),
    "zkfl_setup_g2_gen_mul": (C.c_int, [_P, C.c_char_p, C.c_size_t, _U8P]),
    "zkfl_setup_g1_scale": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_size_t, _U8P]),
    "zkfl_setup_g2_scale": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_size_t, _U8P]),
    "zkfl_setup_g1_lagrange": (C.c_int, [_P, C.c_char_p, C.c_uint32, _U8P]),
    "zkfl_setup_g2_lagrange": (C.c_int, [_P, C.c_char_p, C.c_uint32, _U8P]),
    "zkfl_setup_g1_lincomb": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint32), C.c_char_p, _U8P]),
    "zkfl_setup_g2_lincomb": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint32), C.c_char_p, _U8P]),
    "zkfl_groth16_verify": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p]),
    "zkfl_groth16_verify_batch": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p, C.c_size_t,
                                            C.c_char_p, C.POINTER(C.c_int32)]),
    "zkfl_pairing": (C.c_int, [_P, C.c_size_t, C.c_char_p, C.c_char_p, _U8P]),
    "zkfl_debug_miller_loop": (C.c_int, [_P, C.c_size_t, C.c_char_p, C.c_char_p, _U8P]),
    "zkfl_vkey_load": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(_P)]),
    "zkfl_vkey_info": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "zkfl_vkey_free": (C.c_int, [_P]),
    "zkfl_groth16_verify_multi": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_char_p),
                                            C.POINTER(C.c_size_t), C.c_char_p, C.POINTER(C.c_int32), C.c_int]),
    "zkfl_groth16_verify_round": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_char_p),
                                            C.POINTER(C.c_size_t), C.c_char_p, C.c_char_p, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_uint32)]),
    "zkfl_debug_verify_round": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_char_p),
                                          C.POINTER(C.c_size_t), C.c_char_p, C.c_char_p, C.c_size_t, _U8P,
                                          C.POINTER(C.c_int32)]),
    "zkfl_groth16_verify_round_narrow": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_char_p),
                                                   C.POINTER(C.c_size_t), C.c_char_p, C.c_char_p, C.c_uint32,
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    "zkfl_debug_verify_round_groups": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_char_p),
                                                 C.POINTER(C.c_size_t), C.c_char_p, C.c_char_p, C.c_size_t,
                                                 C.c_uint32, C.POINTER(C.c_uint32), _U8P, C.c_size_t,
                                                 C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "zkfl_debug_wave_pairing": (C.c_int,[_P, C.c_size_t, C.c_char_p, C.c_char_p, C.c_int, _U8P]),
    "zkfl_wprog_load": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(_P)]),
    "zkfl_wprog_free": (C.c_int, [_P]),
    "zkfl_wprog_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "zkfl_wtns_size": (C.c_size_t, [_P]),
    "zkfl_witness_compute": (C.c_int, [_P, _P, C.c_size_t, C.c_char_p, _U8P]),
    "zkfl_witness_compute_resident": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_char_p, C.POINTER(_P)]),
    "zkfl_wprog_parse_inputs": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, _U8P, C.c_size_t,
                                          C.POINTER(C.c_size_t)]),
    "zkfl_witness_compute_json": (C.c_int, [_P, _P, C.c_char_p, _U8P]),
    "zkfl_groth16_full_prove_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_char_p, C.c_char_p, _U8P, _U8P]),
    "zkfl_poseidon_params": (C.c_int, [C.c_uint32, _U8P, _U8P, C.POINTER(C.c_uint32)]),
    "zkfl_poseidon_batch": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_char_p, _U8P]),
    "zkfl_vector_hash_batch": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_char_p, _U8P]),
    "zkfl_merkle_build": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_uint32, _U8P]),
    "zkfl_dataset_commit": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, _U8P]),
    "zkfl_groth16_full_prove_json": (C.c_int, [_P, _P, _P, C.c_char_p, C.c_char_p, _U8P, _U8P]),
    "zkfl_groth16_prove_multi": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(_P), C.c_char_p, _U8P]),
    "zkfl_groth16_full_prove_json_batch": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_char_p), C.c_char_p, _U8P,
                                                     _U8P]),
    "zkfl_groth16_full_prove_multi": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_char_p),
                                                C.c_char_p, _U8P, C.POINTER(_U8P)]),
    "zkfl_r1cs_parse": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(R1csHeader)]),
    "zkfl_r1cs_load": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(_P)]),
    "zkfl_r1cs_info": (C.c_int, [_P, C.POINTER(R1csHeader)]),
    "zkfl_r1cs_free": (C.c_int, [_P]),
    "zkfl_r1cs_check": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                  C.POINTER(R1csReport)]),
    "zkfl_r1cs_check_resident": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(_P), C.POINTER(R1csReport)]),
    "zkfl_zkey_check": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t, C.POINTER(PtauView), C.c_char_p, C.c_char_p,
                                  C.POINTER(ZkeyReport)]),
    "zkfl_ptau_parse": (C.c_int, [_P, C.c_size_t, C.POINTER(PtauHeader)]),
    "zkfl_ptau_check": (C.c_int, [_P, _P, C.c_size_t, C.c_char_p, C.c_uint32, C.POINTER(PtauReportC)]),
    # buffers as addresses: the callers hand numpy arrays over (Context.secagg_mask / secagg_aggregate)
    "zkfl_secagg_mask": (C.c_int, [_P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, C.c_uint32]),
    "zkfl_secagg_aggregate": (C.c_int, [_P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                        C.c_uint32]),
    "zkfl_round_admit": (C.c_int, [_P, C.POINTER(AdmitRound), C.c_uint32, _P, _P]),
    "zkfl_debug_admit_static": (C.c_int, [_P, C.POINTER(AdmitRound), C.c_uint32, C.c_uint32, _P]),
    "zkfl_round_prepare": (C.c_int, [_P, C.POINTER(PrepareRound), C.POINTER(PrepareOut)]),
}


class ZkflError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ZkflError(-5, f"{LIB_PATH} not built (run make in the package dir / __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        # an A/B build named by ZKFL_LIB (tools/ab.sh) may predate an entry point: bind what it has
        ab = bool(os.environ.get("ZKFL_LIB"))
        for name, (res, args) in SIGNATURES.items():
            if ab and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != ZKFL_OK:
        raise ZkflError(rc, lib().zkfl_last_error().decode(errors="replace"))


def _frs(values) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def _ints(b: bytes) -> list:
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _levels(flat, depth):
    out, pos = [], 0
    for lvl in range(depth + 1):
        w = 1 << (depth - lvl)
        out.append(flat[pos:pos + w])
        pos += w
    return out


def poseidon_params(t: int):
    """Host only (no device): circomlib's raw constants for width t from the library's own Grain
    LFSR -> (round constants, x points, y points, R_P)."""
    c = _buf(32 * (8 + 70) * t)     # R_P <= 70 for t <= 17
    xy = _buf(64 * t)
    rp = C.c_uint32()
    check(lib().zkfl_poseidon_params(t, c, xy, C.byref(rp)))
    consts = _ints(bytes(c))[:(8 + rp.value) * t]
    pts = _ints(bytes(xy))
    return consts, pts[:t], pts[t:], rp.value


def build_id() -> str:
    """The loaded library's source hash (zkfl_build_id, set by the package Makefile)."""
    return lib().zkfl_build_id().decode()


def source_id(pkg_dir: str = _PKG_DIR) -> str:
    """The same hash recomputed from the sources in this tree: csrc/*.h, *.hip, *.cc sorted by
    name, then include/zkfl.h (the Makefile's ID_SRCS), SHA-256, first 16 hex digits."""
    import glob
    import hashlib
    names = sorted(os.path.relpath(p, pkg_dir) for ext in ("h", "hip", "cc")
                   for p in glob.glob(os.path.join(pkg_dir, "csrc", "*." + ext)))
    h = hashlib.sha256()
    for n in names + [os.path.join("..", "include", "zkfl.h")]:
        with open(os.path.join(pkg_dir, n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def device_count() -> int:
    """HIP devices visible to this process (0 when there is no GPU or no driver)."""
    n = C.c_int(0)
    if lib().zkfl_device_count(C.byref(n)) != ZKFL_OK:
        return 0
    return n.value


def _buf(n):
    return (C.c_uint8 * n)()


def _u64(a):
    """Unsigned 64-bit integers as a contiguous numpy array."""
    import numpy as np
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def _u8(b):
    """bytes, or an array of uint8, as a flat contiguous uint8 array (no copy where it is one)."""
    import numpy as np
    if isinstance(b, (bytes, bytearray, memoryview)):
        return np.frombuffer(b, dtype=np.uint8)
    b = np.ascontiguousarray(b)
    if b.dtype != np.uint8:
        raise ZkflError(-1, f"expected bytes or a uint8 array, got {b.dtype}")
    return b.reshape(-1)


def _addr(a):
    """A numpy array's address for a void* parameter (None for an empty one)."""
    return a.ctypes.data if a is not None and a.size else None


def _proofs(out, n) -> list:
    """n proofs of 256 B out of a call's output buffer."""
    ob = bytes(out)
    return [ob[256 * i:256 * i + 256] for i in range(n)]


def _proofs_publics(out, pubs, n, k) -> list:
    """[(proof, [k public ints])] out of a call's proof buffer and its n x k x 32 B of signals."""
    pb = bytes(pubs)
    return [(p, _ints(pb[32 * k * i:32 * k * (i + 1)])) for i, p in enumerate(_proofs(out, n))]


class _Handle:
    """An object of the C ABI: its handle `h` and `_free`, the name of the call that releases it."""
    _free = None
    h = None

    def close(self):
        if self.h:
            getattr(lib(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Context(_Handle):
    """One device, one HIP stream (one process per GPU for multi-GPU)."""
    _free = "zkfl_ctx_destroy"

    def __init__(self, device: int = 0):
        import weakref
        h = _P()
        check(lib().zkfl_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device
        # keys, programs and resident witnesses made on this context: closed before it, so none
        # outlives the context it points into (a key freed after its context reads freed memory)
        self._deps = weakref.WeakSet()

    def _own(self, obj):
        self._deps.add(obj)
        return obj

    def close(self):
        if self.h:
            for d in list(self._deps):
                d.close()
        super().close()

    # profiling (bench.py roofline)
    def set_profiling(self, on, serialize: bool = False):
        check(lib().zkfl_ctx_set_profiling(self.h, (2 if serialize else 1) if on else 0))

    def profile(self, name: str):
        """-> (total ms, launches, units, median launch ms)"""
        ms, n, u, med = C.c_double(), C.c_uint64(), C.c_double(), C.c_double()
        check(lib().zkfl_ctx_profile(self.h, name.encode(), C.byref(ms), C.byref(n), C.byref(u), C.byref(med)))
        return ms.value, n.value, u.value, med.value

    def profile_reset(self):
        check(lib().zkfl_ctx_profile_reset(self.h))

    def synchronize(self):
        check(lib().zkfl_ctx_synchronize(self.h))

    def check_ptau(self, buf, rnd: bytes | None = None, chunk_points: int = 0) -> "PtauReport":
        """zkfl_ptau_check: is ``buf`` (bytes, or any buffer such as a mapped file) a well-formed
        Powers of Tau with sections 12-15 the Lagrange form of sections 2-5?  rnd: None draws the
        scalars from the OS CSPRNG; bytes (z | gamma[power + 2] | rho[2n - 1], 32 B std each) are for
        tests and forfeit soundness.  chunk_points: points per device pass (0: the library's
        default).  -> PtauReport; unusable arguments or a malformed file raise ZkflError."""
        addr, length, keep = _buffer_address(buf)
        rep = PtauReportC()
        rc = lib().zkfl_ptau_check(self.h, addr, length, rnd, chunk_points, C.byref(rep))
        del keep
        if rc not in (ZKFL_OK, -8):
            check(rc)
        return PtauReport(rc, rep, lib().zkfl_last_error().decode(errors="replace") if rc else "")

    # wave timeline (libraries built with -DZK_WTRACE=1; tools/wtrace.py)
    def wtrace_start(self, cap: int):
        check(lib().zkfl_debug_wtrace(self.h, 1, cap, None, None))

    def wtrace_stop(self, cap: int) -> tuple[bytes, int]:
        """-> (min(count, cap) records of 40 B, count recorded)"""
        buf = C.create_string_buffer(40 * cap)
        n = C.c_uint32(0)
        check(lib().zkfl_debug_wtrace(self.h, 2, cap, buf, C.byref(n)))
        return buf.raw[:40 * min(n.value, cap)], n.value

    def wtrace_free(self):
        check(lib().zkfl_debug_wtrace(self.h, 0, 0, None, None))

    # primitives
    def msm_g1(self, bases: bytes, scalars: bytes) -> bytes:
        n = len(scalars) // 32
        assert len(bases) == 64 * n
        out = _buf(64)
        check(lib().zkfl_msm_g1(self.h, bases, scalars, n, out))
        return bytes(out)

    def g1_glv_mul(self, points: bytes, scalars: bytes, zs: bytes | None = None) -> bytes:
        """The assembly's scalar multiplications (parity hook): k_i P_i, affine std in and out.
        zs: one z per point (32 B std, nonzero): the chains start from (x z^2, y z^3, z^2, z^3)."""
        n = len(scalars) // 32
        assert len(points) == 64 * n and (zs is None or len(zs) == 32 * n)
        out = _buf(64 * n)
        check(lib().zkfl_debug_g1_glv_mul(self.h, n, points, zs, scalars, out))
        return bytes(out)

    ASM_IN, ASM_OUT = 72, 256   # words per case of asm_ops

    def asm_ops(self, policy: int, op: int, cases) -> list:
        """One operation of the assembly's field / point arithmetic on raw limbs (parity hook,
        zkfl_debug_asm_ops; include/zkfl.h lists the operations and layouts).  policy 0: row, 1: quad;
        cases: per case up to eight operands of nine u32 limbs.  -> per case its 256 output words."""
        n = len(cases)
        inp = (C.c_uint32 * (self.ASM_IN * n))()
        for c, ops in enumerate(cases):
            assert len(ops) <= 8
            for k, limbs in enumerate(ops):
                assert len(limbs) == 9
                inp[self.ASM_IN * c + 9 * k:self.ASM_IN * c + 9 * k + 9] = [int(v) for v in limbs]
        out = (C.c_uint32 * (self.ASM_OUT * n))()
        check(lib().zkfl_debug_asm_ops(self.h, policy, op, n, inp, out))
        flat = list(out)
        return [flat[self.ASM_OUT * c:self.ASM_OUT * (c + 1)] for c in range(n)]

    def msm_front(self, sets, b: int, bases_g2: bytes, fast: bool = True, joint: bool = True):
        """The MSM stage of a small key's proof on the caller's sets (parity hook,
        zkfl_debug_msm_front).  sets: 1..4 of (bases, scalars) or (bases, scalars, sidx, extra_start,
        extra) -- mont affine G1 bases, std scalars, sidx a sequence of u32 (one per base) or None;
        bases_g2: one mont affine G2 base per base of set b.  -> ([64 B std affine per set], 128 B)."""
        n1 = len(sets)
        full = [tuple(s) + (None, 0, b"")[len(s) - 2:] for s in sets]
        arr = lambda t, v: (t * n1)(*v)
        maps = [(C.c_uint32 * len(s[2]))(*s[2]) if s[2] is not None else None for s in full]
        for s, m in zip(full, maps):
            assert len(s[0]) % 64 == 0 and len(s[1]) % 32 == 0 and len(s[4]) % 32 == 0
            assert m is None or len(m) == len(s[0]) // 64
        assert len(bases_g2) % 128 == 0
        out1, out2 = _buf(64 * n1), _buf(128)
        check(lib().zkfl_debug_msm_front(
            self.h, n1, arr(C.c_size_t, [len(s[0]) // 64 for s in full]), arr(C.c_char_p, [s[0] for s in full]),
            arr(C.c_char_p, [s[1] for s in full]), arr(C.c_size_t, [len(s[1]) // 32 for s in full]),
            arr(C.POINTER(C.c_uint32), [C.cast(m, C.POINTER(C.c_uint32)) if m is not None else None for m in maps]),
            arr(C.c_uint32, [s[3] for s in full]), arr(C.c_char_p, [s[4] for s in full]),
            arr(C.c_size_t, [len(s[4]) // 32 for s in full]), b, bases_g2, len(bases_g2) // 128, int(fast),
            int(joint), out1, out2))
        o = bytes(out1)
        return [o[64 * i:64 * i + 64] for i in range(n1)], bytes(out2)

    def msm_g2(self, bases: bytes, scalars: bytes) -> bytes:
        n = len(scalars) // 32
        assert len(bases) == 128 * n
        out = _buf(128)
        check(lib().zkfl_msm_g2(self.h, bases, scalars, n, out))
        return bytes(out)

    def ntt_coset(self, data: bytes) -> bytes:
        n = len(data) // 32
        logn = n.bit_length() - 1
        assert 1 << logn == n
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        check(lib().zkfl_ntt_coset(self.h, buf, logn))
        return bytes(buf)

    def debug_ntt_coset(self, data: bytes, logn: int, nvec: int = 1, vstride: int | None = None,
                        col_max: int = -1) -> bytes:
        """The coset transform of nvec vectors of 2^logn elements in one batched call (parity hook,
        zkfl_debug_ntt_coset): vector v starts at element v * vstride (default 2^logn); col_max = 0
        runs the schedule of the domains above 2^20, < 0 the prover's own."""
        n = 1 << logn
        vstride = n if vstride is None else vstride
        assert len(data) == ((nvec - 1) * vstride + n) * 32
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        check(lib().zkfl_debug_ntt_coset(self.h, buf, logn, nvec, vstride, col_max))
        return bytes(buf)

    def debug_coset_join(self, abc: bytes, logn: int, col_max: int = -1) -> bytes:
        """h = a b - c on the odd coset (std form) from abc = a | b | c on the domain, 2^logn elements
        each, by the prover's own transform and join (parity hook, zkfl_debug_coset_join); col_max as
        for debug_ntt_coset."""
        n = 1 << logn
        assert len(abc) == 3 * n * 32
        out = _buf(32 * n)
        check(lib().zkfl_debug_coset_join(self.h, abc, logn, col_max, out))
        return bytes(out)

    def g1_gen_mul(self, scalars: bytes) -> bytes:
        n = len(scalars) // 32
        out = _buf(64 * n if n else 1)
        check(lib().zkfl_setup_g1_gen_mul(self.h, scalars, n, out))
        return bytes(out)[:64 * n]

    def g2_gen_mul(self, scalars: bytes) -> bytes:
        n = len(scalars) // 32
        out = _buf(128 * n if n else 1)
        check(lib().zkfl_setup_g2_gen_mul(self.h, scalars, n, out))
        return bytes(out)[:128 * n]

    # ceremony primitives (zkfl/ptau.py, zkfl/zkey.py::setup_from_ptau / zkey_contribute)
    def _scale(self, fn, size, points: bytes, scalars: bytes) -> bytes:
        n = len(scalars) // 32
        if len(points) != size * n or len(scalars) != 32 * n:
            raise ZkflError(-1, f"scale: {len(points)} B of points for {n} scalars")
        out = _buf(size * n if n else 1)
        check(fn(self.h, points, scalars, n, out))
        return bytes(out)[:size * n]

    def g1_scale(self, points: bytes, scalars: bytes) -> bytes:
        """out[i] = k_i * P_i (mont affine points, std scalars)."""
        return self._scale(lib().zkfl_setup_g1_scale, 64, points, scalars)

    def g2_scale(self, points: bytes, scalars: bytes) -> bytes:
        return self._scale(lib().zkfl_setup_g2_scale, 128, points, scalars)

    def _lagrange(self, fn, size, points: bytes, logn: int) -> bytes:
        if len(points) != size << logn:
            raise ZkflError(-1, f"lagrange: expected {1 << logn} points")
        out = _buf(size << logn)
        check(fn(self.h, points, logn, out))
        return bytes(out)

    def g1_lagrange(self, points: bytes, logn: int) -> bytes:
        """Inverse FFT over G1: [tau^i G] (2^logn points) -> [L_j(tau) G]."""
        return self._lagrange(lib().zkfl_setup_g1_lagrange, 64, points, logn)

    def g2_lagrange(self, points: bytes, logn: int) -> bytes:
        return self._lagrange(lib().zkfl_setup_g2_lagrange, 128, points, logn)

    def _lincomb(self, fn, size, bases: bytes, rowptr, idx, coefs: bytes) -> bytes:
        import numpy as np
        rp = np.ascontiguousarray(rowptr, dtype=np.uint64)
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        n_out = len(rp) - 1
        if len(coefs) != 32 * len(ix) or int(rp[-1]) != len(ix) or len(bases) % size:
            raise ZkflError(-1, "lincomb: inconsistent term arrays")
        out = _buf(size * n_out if n_out else 1)
        check(fn(self.h, bases, len(bases) // size, n_out, rp.ctypes.data_as(C.POINTER(C.c_uint64)),
                 ix.ctypes.data_as(C.POINTER(C.c_uint32)), coefs, out))
        return bytes(out)[:size * n_out]

    def g1_lincomb(self, bases: bytes, rowptr, idx, coefs: bytes) -> bytes:
        """out[r] = sum_{t in row r} coefs[t] * bases[idx[t]] (rowptr: n_out + 1 offsets)."""
        return self._lincomb(lib().zkfl_setup_g1_lincomb, 64, bases, rowptr, idx, coefs)

    def g2_lincomb(self, bases: bytes, rowptr, idx, coefs: bytes) -> bytes:
        return self._lincomb(lib().zkfl_setup_g2_lincomb, 128, bases, rowptr, idx, coefs)

    # verification (snarkjs groth16 verify)
    def verify(self, vk: bytes, public: bytes, proof: bytes) -> bool:
        """vk image (zkfl.groth16.vk_bytes), public signals npub x 32 B std LE, proof 256 B."""
        assert len(proof) == 256 and len(public) % 32 == 0
        rc = lib().zkfl_groth16_verify(self.h, vk, len(vk), public, len(public) // 32, proof)
        if rc < 0:
            check(rc)
        return rc == 1

    def verify_batch(self, vk: bytes, publics: bytes, proofs: bytes, npub: int) -> list:
        n = len(proofs) // 256
        assert len(proofs) == 256 * n and len(publics) == 32 * npub * n
        res = (C.c_int32 * max(1, n))()
        check(lib().zkfl_groth16_verify_batch(self.h, vk, len(vk), n, publics, npub, proofs, res))
        return [bool(res[i]) for i in range(n)]

    def verify_multi(self, jobs, schedule: str = "auto") -> list:
        """jobs: [(VerifyingKey, public bytes, proof bytes)], each proof against its own resident
        key, in one call -> [bool] in job order.  schedule: "auto", "lanes" (one proof per lane,
        grouped by key) or "waves" (one proof per wavefront: the latency of a round)."""
        sched = VERIFY_SCHEDULES.get(schedule, schedule)
        if not isinstance(sched, int):
            raise ValueError(f"schedule must be one of {sorted(VERIFY_SCHEDULES)}")
        n = len(jobs)
        for _, public, proof in jobs:
            assert len(proof) == 256 and len(public) % 32 == 0
        keys = (_P * max(1, n))(*[k.h for k, _, _ in jobs])
        pubs = (C.c_char_p * max(1, n))(*[bytes(p) for _, p, _ in jobs])
        npubs = (C.c_size_t * max(1, n))(*[len(p) // 32 for _, p, _ in jobs])
        res = (C.c_int32 * max(1, n))()
        check(lib().zkfl_groth16_verify_multi(self.h, n, keys, pubs, npubs, b"".join(pr for _, _, pr in jobs),
                                              res, sched))
        return [bool(res[i]) for i in range(n)]

    @staticmethod
    def _round_args(jobs, z):
        n = len(jobs)
        for _, public, proof in jobs:
            assert len(proof) == 256 and len(public) % 32 == 0
        if z is not None:
            z = b"".join(int(v).to_bytes(16, "little") for v in z) if not isinstance(z, (bytes, bytearray)) else bytes(z)
            assert len(z) == 16 * n
        keys = (_P * max(1, n))(*[k.h for k, _, _ in jobs])
        pubs = (C.c_char_p * max(1, n))(*[bytes(p) for _, p, _ in jobs])
        npubs = (C.c_size_t * max(1, n))(*[len(p) // 32 for _, p, _ in jobs])
        return n, keys, pubs, npubs, b"".join(pr for _, _, pr in jobs), z

    def verify_round(self, jobs, z=None):
        """verify_multi's jobs and verdicts by one random combination with one final exponentiation
        (zkfl_groth16_verify_round) -> ([bool] in job order, report dict: keys, screened, combined,
        passed, fallback).  z (n ints below 2^128, or n x 16 B): for tests only, forfeits soundness;
        None draws them from the OS CSPRNG inside the call."""
        n, keys, pubs, npubs, proofs, z = self._round_args(jobs, z)
        res = (C.c_int32 * max(1, n))()
        rep = (C.c_uint32 * len(ROUND_REPORT_FIELDS))()
        check(lib().zkfl_groth16_verify_round(self.h, n, keys, pubs, npubs, proofs, z, res, rep))
        return [bool(res[i]) for i in range(n)], dict(zip(ROUND_REPORT_FIELDS, (int(v) for v in rep)))

    def debug_verify_round(self, jobs, z, chunk: int = 0):
        """The parity hook of verify_round -> (the final-exponentiated combination, 384 B in
        pairing()'s layout; [bool] screened per job).  chunk: proofs per pass (0 = production)."""
        n, keys, pubs, npubs, proofs, z = self._round_args(jobs, z)
        out = _buf(384)
        scr = (C.c_int32 * max(1, n))()
        check(lib().zkfl_debug_verify_round(self.h, n, keys, pubs, npubs, proofs, z, chunk, out, scr))
        return bytes(out)[:384], [bool(scr[i]) for i in range(n)]

    def verify_round_narrow(self, jobs, z=None, group: int = 0):
        """verify_round with a failed round narrowed to its bad groups
        (zkfl_groth16_verify_round_narrow): the passes' jobs, sorted by key, are cut into groups of
        `group`, every group gets a value of its own, and only the jobs of the groups whose value
        is not 1 are re-verified -> ([bool] in job order, report dict: NARROW_REPORT_FIELDS).
        group 0: the production policy (groups of ROUND_GROUP, narrowing from ROUND_NARROW_MIN
        combined jobs on).  z as in verify_round."""
        n, keys, pubs, npubs, proofs, z = self._round_args(jobs, z)
        res = (C.c_int32 * max(1, n))()
        rep = (C.c_uint32 * len(NARROW_REPORT_FIELDS))()
        check(lib().zkfl_groth16_verify_round_narrow(self.h, n, keys, pubs, npubs, proofs, z, group, res, rep))
        return [bool(res[i]) for i in range(n)], dict(zip(NARROW_REPORT_FIELDS, (int(v) for v in rep)))

    def debug_verify_round_groups(self, jobs, z, chunk: int = 0, group: int = 0):
        """The parity hook of verify_round_narrow -> ([job i's group], [every group's
        final-exponentiated value, 384 B in pairing()'s layout], [bool] screened per job)."""
        n, keys, pubs, npubs, proofs, z = self._round_args(jobs, z)
        cap = max(1, n)  # a group holds at least one job
        group_of = (C.c_uint32 * cap)()
        out = _buf(384 * cap)
        scr = (C.c_int32 * cap)()
        ng = C.c_uint32(0)
        check(lib().zkfl_debug_verify_round_groups(self.h, n, keys, pubs, npubs, proofs, z, chunk, group, group_of,
                                                   out, cap, C.byref(ng), scr))
        raw = bytes(out)
        return ([int(group_of[i]) for i in range(n)], [raw[384 * g:384 * (g + 1)] for g in range(ng.value)],
                [bool(scr[i]) for i in range(n)])

    def wave_pairing(self, g1: bytes, g2: bytes, final_exp: bool = True) -> bytes:
        """pairing() computed by the wave verifier's tower, Miller loop and final exponentiation
        (one pair per wavefront): the parity hook of Context.verify_multi's "waves" schedule."""
        n = len(g1) // 64
        assert len(g1) == 64 * n and len(g2) == 128 * n
        out = _buf(384 * n if n else 1)
        check(lib().zkfl_debug_wave_pairing(self.h, n, g1, g2, 1 if final_exp else 0, out))
        return bytes(out)[:384 * n]

    # Poseidon / vectorHash / Merkle trees (the reference's data and server side)
    def poseidon_batch(self, rows) -> list:
        """[[ints] * arity] -> [Poseidon(row)] (circomlibjs poseidon, on the GPU)."""
        if not rows:
            return []
        arity = len(rows[0])
        assert all(len(r) == arity for r in rows)
        out = _buf(32 * len(rows))
        check(lib().zkfl_poseidon_batch(self.h, arity, len(rows), _frs(v for r in rows for v in r), out))
        return _ints(bytes(out))

    def vector_hash_batch(self, vectors) -> list:
        """[[ints] * len] -> [vectorHash(v)] (tests/full_system_simulation.mjs:139-156)."""
        if not vectors:
            return []
        ln = len(vectors[0])
        assert all(len(v) == ln for v in vectors)
        out = _buf(32 * len(vectors))
        check(lib().zkfl_vector_hash_batch(self.h, ln, len(vectors), _frs(x for v in vectors for x in v), out))
        return _ints(bytes(out))

    def merkle_build(self, leaves, depth: int) -> list:
        """buildMerkleTree(leaves, depth) -> the reference's `tree` (list of padded levels of ints)."""
        out = _buf(32 * ((2 << depth) - 1))
        check(lib().zkfl_merkle_build(self.h, _frs(leaves), len(leaves), depth, out))
        return _levels(_ints(bytes(out)), depth)

    def dataset_commit(self, samples, depth: int) -> list:
        """computeDatasetCommitment: leaves = vectorHash(sample) on the device, then the tree."""
        ln = len(samples[0]) if samples else 1
        assert all(len(v) == ln for v in samples)
        flat = self.dataset_commit_raw(_frs(x for v in samples for x in v), len(samples), ln, depth)
        return _levels(_ints(flat), depth)

    def dataset_commit_raw(self, values: bytes, n: int, ln: int, depth: int) -> bytes:
        """Byte form: values n x ln x 32 B std -> the flattened padded tree ((2^(depth+1) - 1) x 32 B)."""
        assert len(values) == 32 * n * ln
        out = _buf(32 * ((2 << depth) - 1))
        check(lib().zkfl_dataset_commit(self.h, values, n, ln, depth, out))
        return bytes(out)

    def poseidon_batch_raw(self, arity: int, rows):
        """Byte form of poseidon_batch: rows = n x arity x 32 B std (bytes or a uint8 array) -> a uint8
        array (n, 32).  For batches too large to go through Python integers."""
        import numpy as np
        rows = _u8(rows)
        n = rows.size // (32 * arity)
        assert rows.size == 32 * arity * n
        out = np.zeros((n, 32), np.uint8)
        if n:
            check(lib().zkfl_poseidon_batch(self.h, arity, n, C.cast(rows.ctypes.data, C.c_char_p),
                                            C.cast(out.ctypes.data, _U8P)))
        return out

    # secure aggregation (csrc/secagg.hip; zkfl/secagg.py holds the list-level interface)
    def secagg_mask(self, ids, peer_ptr, peer_ids, keys, rnd: int, gradients, dim: int, chunk_terms: int = 0):
        """zkfl_secagg_mask: ids (n), peer_ptr (n + 1, CSR) and peer_ids (T) as unsigned 64-bit
        integers; keys (T x 32 B) and gradients (n x dim x 32 B) std-form field elements as bytes or
        uint8 arrays; rnd an integer < r.  -> the masked updates, a uint8 array (n, dim, 32)."""
        import numpy as np
        ids, peer_ptr, peer_ids = _u64(ids), _u64(peer_ptr), _u64(peer_ids)
        keys, gradients = _u8(keys), _u8(gradients)
        n = ids.size
        if peer_ptr.size != n + 1:
            raise ZkflError(-1, f"secagg_mask: peer_ptr holds {peer_ptr.size} entries for {n} clients")
        t = int(peer_ptr[n])
        if t < 1 << 32 and (peer_ids.size != t or keys.size != 32 * t):
            raise ZkflError(-1, f"secagg_mask: peer_ptr counts {t} peers, peer_ids holds {peer_ids.size} "
                                f"and keys {keys.size // 32}")
        if gradients.size != 32 * n * dim:
            raise ZkflError(-1, f"secagg_mask: expected {n} x {dim} gradient values (32 B each)")
        out = np.zeros((n, dim, 32), np.uint8)
        check(lib().zkfl_secagg_mask(self.h, n, dim, _addr(ids), _addr(peer_ptr), _addr(peer_ids), _addr(keys),
                                     int(rnd).to_bytes(32, "little"), _addr(gradients), _addr(out), chunk_terms))
        return out

    def secagg_aggregate(self, member_ptr, masked, pair_ptr, pair_in, pair_out, pair_keys, rnd: int, dim: int,
                         chunk_terms: int = 0, decode: bool = True):
        """zkfl_secagg_aggregate: member_ptr / pair_ptr (n_groups + 1, CSR), pair_in / pair_out (P)
        as unsigned 64-bit integers; masked (M x dim x 32 B, the included members' updates, group after
        group) and pair_keys (P x 32 B) as bytes or uint8 arrays.  -> (sums: uint8 (n_groups, dim, 32),
        signed: int64 (n_groups, dim), out_of_range: bool (n_groups)); the last two None when not
        decode."""
        import numpy as np
        member_ptr, pair_ptr, pair_in, pair_out = _u64(member_ptr), _u64(pair_ptr), _u64(pair_in), _u64(pair_out)
        masked, pair_keys = _u8(masked), _u8(pair_keys)
        g = member_ptr.size - 1
        if g < 0 or pair_ptr.size != g + 1:
            raise ZkflError(-1, "secagg_aggregate: member_ptr and pair_ptr must hold n_groups + 1 entries each")
        m, p = int(member_ptr[g]), int(pair_ptr[g])
        if p < 1 << 32 and (pair_in.size != p or pair_out.size != p or pair_keys.size != 32 * p):
            raise ZkflError(-1, f"secagg_aggregate: pair_ptr counts {p} pairs, the pair arrays hold "
                                f"{pair_in.size}, {pair_out.size} and {pair_keys.size // 32}")
        if m < 1 << 32 and masked.size != 32 * m * dim:
            raise ZkflError(-1, f"secagg_aggregate: expected {m} x {dim} masked values (32 B each)")
        sums = np.zeros((g, dim, 32), np.uint8)
        signed = np.zeros((g, dim), np.int64) if decode else None
        oor = np.zeros(g, np.uint8) if decode else None
        check(lib().zkfl_secagg_aggregate(self.h, g, dim, _addr(member_ptr), _addr(masked), _addr(pair_ptr),
                                          _addr(pair_in), _addr(pair_out), _addr(pair_keys),
                                          int(rnd).to_bytes(32, "little"), _addr(sums),
                                          _addr(signed) if decode else None, _addr(oor) if decode else None,
                                          chunk_terms))
        return sums, signed, (oor.astype(bool) if decode else None)

    # admitting a round (csrc/admit.hip; zkfl/admit.py holds the package-level interface)
    @staticmethod
    def _admit_round(r: dict, flags: int, s_npub: int, proofs: bool):
        """The arrays of a round -> (zkfl_admit_round, what must stay alive during the call).  r: "ids"
        (n), "round", "tau_squared" (integers < r), "dim", "gradients" (int64 n x dim), "masked_update"
        (uint8 n x dim x 32), per phase r[phase] = {"present" (n bytes), "claimed" (uint8 n x fields x 32),
        "signals" (uint8 n x nPublic x 32), "proofs" (uint8 n x 256)}, optional "weights" (dim x 32),
        "peer_ptr" (n + 1) and "peer_ids"."""
        import numpy as np
        ids = _u64(r["ids"])
        n, dim = ids.size, int(r["dim"])
        keep = [ids, int(r["round"]).to_bytes(32, "little"), int(r["tau_squared"]).to_bytes(32, "little")]
        a = AdmitRound()
        a.n, a.dim, a.ids = n, dim, _addr(ids)
        a.round = C.cast(C.c_char_p(keep[1]), _P)
        a.tau_squared = C.cast(C.c_char_p(keep[2]), _P)

        def arr(x, size, what, dtype=np.uint8):
            if x is None:
                return None
            x = _u8(x) if dtype is np.uint8 else np.ascontiguousarray(x, dtype=dtype).reshape(-1)
            if x.size != size:
                raise ZkflError(-1, f"admit: {what} holds {x.size} entries, expected {size}")
            keep.append(x)
            return _addr(x)

        for name in ADMIT_PHASES:
            ph, src = getattr(a, name), r[name]
            npub = ADMIT_NPUBLIC[name] if name != "secagg" else s_npub
            ph.present = arr(src.get("present"), n, f"{name} present")
            ph.claimed = arr(src.get("claimed"), 32 * n * len(ADMIT_FIELDS[name]), f"{name} claimed")
            ph.signals = arr(src.get("signals"), 32 * n * npub, f"{name} signals")
            ph.proofs = arr(src.get("proofs"), 256 * n, f"{name} proofs") if proofs else None
        a.gradients = arr(r.get("gradients"), n * dim, "gradients", np.int64)
        a.masked_update = arr(r.get("masked_update"), 32 * n * dim, "masked_update")
        a.weights = arr(r.get("weights"), 32 * dim, "weights")
        if r.get("peer_ptr") is not None:
            ptr = _u64(r["peer_ptr"])
            if ptr.size != n + 1:
                raise ZkflError(-1, f"admit: peer_ptr holds {ptr.size} entries for {n} clients")
            pid = _u64(r.get("peer_ids", ()))
            if int(ptr[n]) < 1 << 32 and ptr[0] == 0 and pid.size != int(ptr[n]):
                raise ZkflError(-1, f"admit: peer_ptr counts {int(ptr[n])} peers, peer_ids holds {pid.size}")
            keep += [ptr, pid]
            a.peer_ptr, a.peer_ids = ptr.ctypes.data, _addr(pid)
        return a, keep

    def round_admit(self, r: dict, vkeys, flags: int = 7):
        """zkfl_round_admit: r as _admit_round describes, vkeys the three VerifyingKey (balance, training,
        secagg) -> (codes: uint32 array (3, n), phase-major; the verifier's report dict).  flags: ADMIT_*;
        the default turns the three added checks on."""
        import numpy as np
        a, keep = self._admit_round(r, flags, vkeys[2].n_public, True)
        for i, k in enumerate(vkeys):
            a.vkeys[i] = k.h
        codes = np.zeros((3, a.n), np.uint32)
        rep = (C.c_uint32 * len(ROUND_REPORT_FIELDS))()
        check(lib().zkfl_round_admit(self.h, C.byref(a), flags, _addr(codes), C.cast(rep, _P)))
        del keep
        return codes, dict(zip(ROUND_REPORT_FIELDS, (int(v) for v in rep)))

    def debug_admit_static(self, r: dict, secagg_npublic: int, flags: int = 7):
        """zkfl_debug_admit_static: the static codes alone (no keys, no proofs) -> uint32 array (3, n)."""
        import numpy as np
        a, keep = self._admit_round(r, flags, secagg_npublic, False)
        codes = np.zeros((3, a.n), np.uint32)
        check(lib().zkfl_debug_admit_static(self.h, C.byref(a), flags, secagg_npublic, _addr(codes)))
        del keep
        return codes

    # preparing a round (csrc/prepare.hip; zkfl/prepare.py holds the spec-level interface)
    def round_prepare(self, r: dict, want=None) -> dict:
        """zkfl_round_prepare.  r: "ids" (n), "samples", "dim", "depth", "batch", "precision", "peers",
        "features" (int64 n x samples x dim), "labels" (uint8 n x samples), "batch_idx" (uint32 n x batch,
        or None), "weights" (int64 dim), "round" (integer < r), "tau_squared", and with peers > 0
        "peer_ids" (uint64 n x peers), "keys" (uint8 n x peers x 32), "master_keys" (uint8 n x 32).
        want: the names of PREPARE_OUTPUTS to compute (None: all the shape has; the secagg outputs
        only with peers > 0).  -> {name: array}: the input vectors as uint8 (n, n_inputs, 32), "roots"
        uint8 (n, 4, 32) (D, G, W, K), "gradients" int64 (n, dim), "masked" uint8 (n, dim, 32), "c1" and
        "status" uint32 (n)."""
        import numpy as np
        ids = _u64(r["ids"])
        n = ids.size
        S, dim, depth, batch, peers = (int(r[k]) for k in ("samples", "dim", "depth", "batch", "peers"))
        keep = [ids, int(r["round"]).to_bytes(32, "little")]
        a = PrepareRound()
        a.n, a.ids = n, _addr(ids)
        a.samples, a.dim, a.depth, a.batch, a.precision, a.peers = S, dim, depth, batch, int(r["precision"]), peers
        a.round = C.cast(C.c_char_p(keep[1]), _P)
        a.tau_squared = int(r["tau_squared"])

        def arr(x, size, what, dtype):
            if x is None:
                return None
            x = _u8(x) if dtype is np.uint8 else np.ascontiguousarray(x, dtype=dtype).reshape(-1)
            if x.size != size:
                raise ZkflError(-1, f"round_prepare: {what} holds {x.size} entries, expected {size}")
            keep.append(x)
            return x.ctypes.data          # an empty array keeps its (non-null) address: n == 0 stays valid

        a.features = arr(r["features"], n * S * dim, "features", np.int64)
        a.labels = arr(r["labels"], n * S, "labels", np.uint8)
        a.batch_idx = arr(r.get("batch_idx"), n * batch, "batch_idx", np.uint32)
        a.weights = arr(r["weights"], dim, "weights", np.int64)
        a.peer_ids = arr(r.get("peer_ids"), n * peers, "peer_ids", np.uint64)
        a.keys = arr(r.get("keys"), 32 * n * peers, "keys", np.uint8)
        a.master_keys = arr(r.get("master_keys"), 32 * n, "master_keys", np.uint8)
        names = [k for k in PREPARE_OUTPUTS if peers or k not in ("secagg_inputs", "masked")] if want is None else list(want)
        ln = prepare_lengths(S, dim, depth, batch, peers)
        shapes = {"balance_inputs": ((n, ln["balance"], 32), np.uint8), "training_inputs": ((n, ln["training"], 32), np.uint8),
                  "secagg_inputs": ((n, ln["secagg"], 32), np.uint8), "roots": ((n, 4, 32), np.uint8),
                  "gradients": ((n, dim), np.int64), "masked": ((n, dim, 32), np.uint8), "c1": ((n,), np.uint32),
                  "status": ((n,), np.uint32)}
        res, o = {}, PrepareOut()
        for k in names:
            shape, dt = shapes[k]
            res[k] = np.zeros(shape, dt)
            setattr(o, k, res[k].ctypes.data)
        check(lib().zkfl_round_prepare(self.h, C.byref(a), C.byref(o)))
        del keep
        return res

    # multi-key batches (one federated round: several circuits' proofs interleaved on one device)
    def prove_multi(self, jobs, rs: bytes | None = None) -> list:
        """jobs: [(ProvingKey, ResidentWitness)] -> [proof 256 B] (zkfl_groth16_prove_multi)."""
        n = len(jobs)
        keys = (_P * max(1, n))(*[k.h for k, _ in jobs])
        ws = (_P * max(1, n))(*[w.h for _, w in jobs])
        out = _buf(256 * max(1, n))
        check(lib().zkfl_groth16_prove_multi(self.h, n, keys, ws, rs, out))
        return _proofs(out, n)

    def full_prove_multi(self, jobs, rs: bytes | None = None) -> list:
        """jobs: [(ProvingKey, WitnessProgram, input vector bytes)] -> [(proof, [public ints])]
        (zkfl_groth16_full_prove_multi: witness + proof per slot, keys interleaved)."""
        n = len(jobs)
        for k, wp, inp in jobs:
            if len(inp) != 32 * wp.n_inputs:
                raise ZkflError(-1, f"expected {wp.n_inputs} input values (32 B each)")
        keys = (_P * max(1, n))(*[k.h for k, _, _ in jobs])
        progs = (_P * max(1, n))(*[wp.h for _, wp, _ in jobs])
        ins = (C.c_char_p * max(1, n))(*[inp for _, _, inp in jobs])
        pub_bufs = [_buf(32 * max(1, k.n_public)) for k, _, _ in jobs]
        pubs = (_U8P * max(1, n))(*[C.cast(b, _U8P) for b in pub_bufs])
        out = _buf(256 * max(1, n))
        check(lib().zkfl_groth16_full_prove_multi(self.h, n, keys, progs, ins, rs, out, pubs))
        return [(p, _ints(bytes(pub_bufs[i]))[:jobs[i][0].n_public]) for i, p in enumerate(_proofs(out, n))]

    def assemble(self, parts: bytes, n_parts: int, rs: bytes) -> list:
        """Split proofs: parts = n x n_parts x 768 B (proof-major, zkfl_groth16_prove_part_batch's
        layout), rs = n x 64 B -> n proofs of 256 B (zkfl_groth16_assemble)."""
        n = len(rs) // 64
        if len(rs) != 64 * n or len(parts) != PART_BYTES * n * n_parts:
            raise ZkflError(-1, "assemble: parts / rs sizes disagree")
        out = _buf(256 * max(1, n))
        check(lib().zkfl_groth16_assemble(self.h, n, n_parts, parts, rs, out))
        return _proofs(out, n)

    def pairing(self, g1: bytes, g2: bytes, final_exp: bool = True) -> bytes:
        """e(P_i, Q_i) for n pairs (std affine); 384 B std Fq12 each (toObject order)."""
        n = len(g1) // 64
        assert len(g1) == 64 * n and len(g2) == 128 * n
        out = _buf(384 * n if n else 1)
        fn = lib().zkfl_pairing if final_exp else lib().zkfl_debug_miller_loop
        check(fn(self.h, n, g1, g2, out))
        return bytes(out)[:384 * n]


VERIFY_SCHEDULES = {"auto": 0, "lanes": 1, "waves": 2}  # ZKFL_VERIFY_*
ROUND_REPORT_FIELDS = ("keys", "screened", "combined", "passed", "fallback")  # zkfl_round_report
NARROW_REPORT_FIELDS = ("keys", "screened", "combined", "passed", "groups", "bad_groups", "fallback")  # zkfl_narrow_report
ROUND_GROUP, ROUND_NARROW_MIN = 64, 4096  # ZKFL_ROUND_GROUP, ZKFL_ROUND_NARROW_MIN


class VerifyingKey(_Handle):
    """A verification key made device-resident (zkfl_vkey_load): vk_bytes is the vk image of
    Context.verify (zkfl.groth16.vk_bytes).  Any number may be resident on a context."""
    _free = "zkfl_vkey_free"

    def __init__(self, ctx: Context, vk_bytes: bytes):
        h = _P()
        check(lib().zkfl_vkey_load(ctx.h, vk_bytes, len(vk_bytes), C.byref(h)))
        self.h = h
        self.ctx = ctx
        ctx._own(self)
        npub = C.c_uint32()
        check(lib().zkfl_vkey_info(h, C.byref(npub)))
        self.n_public = npub.value


class ProvingKey(_Handle):
    """A .zkey made device-resident (bases expanded per MSM window)."""
    _free = "zkfl_key_free"

    def __init__(self, ctx: Context, zkey, shard: int = 0, n_shards: int = 1):
        """zkey: the key bytes, or its path (mapped and parsed on host threads: zkfl_zkey_file_open
        + zkfl_zkey_load_file).  shard / n_shards: keep only this shard's share of every query
        (split proofs, zkfl_zkey_load_shard); the default is the whole key."""
        h = _P()
        if isinstance(zkey, (str, os.PathLike)):
            if (shard, n_shards) != (0, 1):
                with open(zkey, "rb") as f:
                    zkey = f.read()
            else:
                fh = _P()
                check(lib().zkfl_zkey_file_open(os.fsencode(zkey), C.byref(fh)))
                try:
                    check(lib().zkfl_zkey_load_file(ctx.h, fh, C.byref(h)))
                finally:
                    lib().zkfl_zkey_file_close(fh)
        if h:
            pass
        elif n_shards == 1 and shard == 0:
            check(lib().zkfl_zkey_load(ctx.h, zkey, len(zkey), C.byref(h)))
        else:
            check(lib().zkfl_zkey_load_shard(ctx.h, zkey, len(zkey), shard, n_shards, C.byref(h)))
        self.h = h
        self.shard, self.n_shards = shard, n_shards
        self.ctx = ctx
        ctx._own(self)
        nv, npub, dom = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().zkfl_key_info(h, C.byref(nv), C.byref(npub), C.byref(dom)))
        self.n_vars, self.n_public, self.domain_size = nv.value, npub.value, dom.value

    def ab_shared(self) -> dict:
        """How the key holds its A query (zkfl_key_ab_shared): form "D" (A = B1 + sum w_i (A_i - B1_i))
        or "A", this shard's wires with one base in both queries, and the A slot's base count."""
        d, sh, nb = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().zkfl_key_ab_shared(self.h, C.byref(d), C.byref(sh), C.byref(nb)))
        return {"form": "D" if d.value else "A", "shared_wires": sh.value, "a_bases": nb.value}

    def set_groups(self, rep):
        """The key's partition of its wires (zkfl_key_set_groups): rep[i] = the first wire of i's
        group, one entry per wire; None drops the grouped form.  Proof bytes do not depend on it."""
        if rep is None:
            check(lib().zkfl_key_set_groups(self.h, None, 0))
            return
        arr = (C.c_uint32 * max(1, len(rep)))(*rep)
        check(lib().zkfl_key_set_groups(self.h, arr, len(rep)))

    def learn_groups(self, w: "ResidentWitness"):
        """Partition the wires by w's equal values >= 2^128 (zkfl_key_learn_groups)."""
        check(lib().zkfl_key_learn_groups(self.ctx.h, self.h, w.h))

    def groups(self) -> dict:
        """The key's partition (zkfl_key_groups): groups, non-representative wires, per query the
        bases of the plain form and those that still carry a scalar, the build time, and the
        non-zero differences of the key's last grouped proof."""
        g = GroupsInfo()
        check(lib().zkfl_key_groups(self.h, C.byref(g)))
        r = GroupRowsInfo()
        check(lib().zkfl_key_group_rows(self.h, C.byref(r)))
        return {"grouped": bool(g.grouped), "learned": bool(g.learned), "groups": g.groups, "non_rep": g.non_rep,
                "bases": dict(zip(GROUP_QUERIES, g.bases)), "bases_rep": dict(zip(GROUP_QUERIES, g.bases_rep)),
                "builds": g.builds, "last_miss": g.last_miss, "build_ms": g.build_ms,
                # the grouped ABC: row classes, K -> Kd, the wire lists, the last proof's repair
                "rows_grouped": bool(r.rows_grouped), "row_classes": r.row_classes, "terms": r.terms,
                "terms_rep": r.terms_rep, "wire_list": r.wire_list, "wires_over_cap": r.wires_over_cap,
                "last_dirty": r.last_dirty, "last_plain": bool(r.last_plain), "rows_build_ms": r.rows_build_ms}

    def debug_abc(self, w: "ResidentWitness", grouped: bool = True):
        """The ABC stage alone on slot 0 (zkfl_debug_abc) -> (a | b | c as 3 x domain x 32 B in
        standard form, non-zero differences, dirty constraints, plain flag)."""
        out = _buf(96 * self.domain_size)
        cnt = (C.c_uint32 * 3)()
        check(lib().zkfl_debug_abc(self.ctx.h, self.h, w.h, 1 if grouped else 0, out, cnt))
        return bytes(out), cnt[0], cnt[1], bool(cnt[2])

    def set_slots(self, slots: int):
        """Proofs kept in flight by prove_batch (each slot = 3 HIP streams + scratch)."""
        check(lib().zkfl_key_set_slots(self.h, slots))
        self.slots = slots

    def prove(self, wtns: bytes, rs: bytes | None = None):
        """-> (proof 256 B, [public signal ints])"""
        proof = _buf(256)
        pub = _buf(32 * max(1, self.n_public))
        npub = C.c_size_t()
        check(lib().zkfl_groth16_prove(self.ctx.h, self.h, wtns, len(wtns), rs, proof, pub, C.byref(npub)))
        pb = bytes(pub)
        return bytes(proof), [int.from_bytes(pb[32 * i:32 * i + 32], "little") for i in range(npub.value)]

    def upload(self, wtns: bytes) -> "ResidentWitness":
        return ResidentWitness(self, wtns)

    def prove_resident(self, w: "ResidentWitness", rs: bytes | None = None) -> bytes:
        proof = _buf(256)
        check(lib().zkfl_groth16_prove_resident(self.ctx.h, self.h, w.h, rs, proof))
        return bytes(proof)

    def prove_batch(self, ws, rs: bytes | None = None) -> list:
        n = len(ws)
        arr = (_P * n)(*[w.h for w in ws])
        out = _buf(256 * n)
        check(lib().zkfl_groth16_prove_batch(self.ctx.h, self.h, n, arr, rs, out))
        return _proofs(out, n)

    def prove_part_batch(self, ws, rs: bytes) -> list:
        """This shard's parts of n proofs (rs REQUIRED, n x 64 B, the same on every shard)
        -> [768 B] (zkfl_groth16_prove_part_batch)."""
        n = len(ws)
        if rs is None or len(rs) != 64 * n:
            raise ZkflError(-1, "prove_part_batch: rs must be n x 64 bytes")
        arr = (_P * max(1, n))(*[w.h for w in ws])
        out = _buf(PART_BYTES * max(1, n))
        check(lib().zkfl_groth16_prove_part_batch(self.ctx.h, self.h, n, arr, rs, out))
        ob = bytes(out)
        return [ob[PART_BYTES * i:PART_BYTES * (i + 1)] for i in range(n)]

    def full_prove_batch(self, prog: "WitnessProgram", inputs, rs: bytes | None = None):
        """input vectors (wprog.input_bytes / parse_inputs) -> [(proof 256 B, [public ints])]:
        witness and proof pipelined per slot on the GPU (zkfl_groth16_full_prove_batch)."""
        n = len(inputs)
        buf = prog._inputs(inputs)
        out = _buf(256 * max(1, n))
        pubs = _buf(32 * max(1, self.n_public) * max(1, n))
        check(lib().zkfl_groth16_full_prove_batch(self.ctx.h, self.h, prog.h, n, buf, rs, out, pubs))
        return _proofs_publics(out, pubs, n, self.n_public)

    def full_prove_json_batch(self, prog: "WitnessProgram", texts, rs: bytes | None = None):
        """input.json texts -> [(proof 256 B, [public ints])]: parsed by host threads while earlier
        proofs run (zkfl_groth16_full_prove_json_batch)."""
        n = len(texts)
        arr = (C.c_char_p * max(1, n))(*[t.encode() if isinstance(t, str) else t for t in texts])
        out = _buf(256 * max(1, n))
        pubs = _buf(32 * max(1, self.n_public) * max(1, n))
        check(lib().zkfl_groth16_full_prove_json_batch(self.ctx.h, self.h, prog.h, n, arr, rs, out, pubs))
        return _proofs_publics(out, pubs, n, self.n_public)

    def full_prove_json(self, prog: "WitnessProgram", input_json: str, rs: bytes | None = None):
        """snarkjs groth16.fullProve for one input.json text -> (proof 256 B, [public ints])."""
        out = _buf(256)
        pub = _buf(32 * max(1, self.n_public))
        check(lib().zkfl_groth16_full_prove_json(self.ctx.h, self.h, prog.h, input_json.encode(), rs, out, pub))
        return bytes(out), _ints(bytes(pub))[:self.n_public]

    def debug_parts(self, wtns: bytes):
        """-> (h list of ints, dict of MSM results as std affine bytes)"""
        h = _buf(32 * self.domain_size)
        m = _buf(384)
        check(lib().zkfl_debug_prove_parts(self.ctx.h, self.h, wtns, len(wtns), h, m))
        hb, mb = bytes(h), bytes(m)
        hs = [int.from_bytes(hb[32 * i:32 * i + 32], "little") for i in range(self.domain_size)]
        parts = dict(A=mb[0:64], B1=mb[64:128], B2=mb[128:256], C=mb[256:320], H=mb[320:384])
        return hs, parts


class ResidentWitness(_Handle):
    _free = "zkfl_witness_free"

    def __init__(self, key: ProvingKey, wtns: bytes | None = None, handle=None):
        if handle is not None:
            self.h = handle
            key.ctx._own(self)
            return
        h = _P()
        check(lib().zkfl_witness_upload(key.ctx.h, key.h, wtns, len(wtns), C.byref(h)))
        self.h = h
        key.ctx._own(self)


def parse_inputs(image: bytes, input_json: str, cap: int | None = None) -> bytes:
    """circom input.json -> flattened input vector via the program's signal table (host only).
    cap: room for this many values (default: the image's input count, header word 4 + 5)."""
    if cap is None:
        cap = max(1, int.from_bytes(image[16:20], "little") + int.from_bytes(image[20:24], "little"))
    out = _buf(32 * cap)
    n = C.c_size_t()
    check(lib().zkfl_wprog_parse_inputs(image, len(image), input_json.encode(), out, cap, C.byref(n)))
    return bytes(out)[:32 * n.value]


class WitnessProgram(_Handle):
    """A compiled circuit witness program (zkfl.wprog image) loaded on the device: the
    replacement of circom's <circuit>.wasm + generate_witness.cjs."""
    _free = "zkfl_wprog_free"

    def __init__(self, ctx: Context, image: bytes):
        h = _P()
        check(lib().zkfl_wprog_load(ctx.h, image, len(image), C.byref(h)))
        self.h, self.ctx = h, ctx
        ctx._own(self)
        nw, ni, npub = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().zkfl_wprog_info(h, C.byref(nw), C.byref(ni), C.byref(npub)))
        self.n_wires, self.n_inputs, self.n_public = nw.value, ni.value, npub.value
        self.wtns_size = lib().zkfl_wtns_size(h)

    def _inputs(self, inputs) -> bytes:
        buf = b"".join(inputs)
        if len(buf) != 32 * self.n_inputs * len(inputs):
            raise ZkflError(-1, f"expected {self.n_inputs} input values (32 B each) per witness")
        return buf

    def compute(self, inputs) -> list:
        """inputs: list of per-witness input byte strings (zkfl.wprog.input_bytes) -> .wtns images."""
        n = len(inputs)
        out = _buf(self.wtns_size * max(1, n))
        check(lib().zkfl_witness_compute(self.ctx.h, self.h, n, self._inputs(inputs), out))
        ob = bytes(out)
        return [ob[i * self.wtns_size:(i + 1) * self.wtns_size] for i in range(n)]

    def compute_json(self, input_json: str) -> bytes:
        """One witness from circom's input.json text -> .wtns image."""
        out = _buf(self.wtns_size)
        check(lib().zkfl_witness_compute_json(self.ctx.h, self.h, input_json.encode(), out))
        return bytes(out)

    def compute_resident(self, key: ProvingKey, inputs) -> list:
        """-> ResidentWitness per input, computed in HBM for `key` (no host round trip)."""
        n = len(inputs)
        arr = (_P * max(1, n))()
        check(lib().zkfl_witness_compute_resident(self.ctx.h, self.h, key.h, n, self._inputs(inputs), arr))
        return [ResidentWitness(key, handle=_P(arr[i])) for i in range(n)]


NO_CONSTRAINT = 0xFFFFFFFF   # Report.first of a witness whose wire 0 is not 1


class Report:
    """One witness's check (zkfl_r1cs_report): ``ok``; otherwise ``n_failed`` constraints do not
    hold, ``first`` is the lowest such index and ``a``, ``b``, ``c`` the values of <A, w>, <B, w>,
    <C, w> there (``first == NO_CONSTRAINT``: wire 0 is not 1, no constraint was looked at)."""

    def __init__(self, r: R1csReport):
        self.n_failed, self.first = int(r.n_failed), int(r.first)
        self.a, self.b, self.c = (int.from_bytes(bytes(x), "little") for x in (r.a, r.b, r.c))

    @property
    def ok(self) -> bool:
        return self.n_failed == 0

    def __repr__(self):
        if self.ok:
            return "Report(ok)"
        return f"Report(n_failed={self.n_failed}, first={self.first}, a={self.a}, b={self.b}, c={self.c})"


def _buffer_address(buf):
    """(address, length, an object to keep alive) of a bytes-like object, without copying it: bytes
    go through a char pointer, anything else (a bytearray, a read-only or writable mmap) through
    the buffer protocol."""
    if isinstance(buf, bytes):
        return C.cast(C.c_char_p(buf), _P), len(buf), buf
    mv = memoryview(buf)
    if not mv.contiguous:
        raise ValueError("buffer is not contiguous")
    if mv.readonly:
        # ctypes.from_buffer needs a writable buffer; numpy takes the address of a read-only one
        import numpy as np
        arr = np.frombuffer(mv, dtype=np.uint8)
        return _P(arr.ctypes.data), arr.nbytes, (arr, mv)
    arr = (C.c_uint8 * mv.nbytes).from_buffer(mv)
    return C.cast(arr, _P), mv.nbytes, (arr, mv)


def ptau_header(buf) -> dict:
    """A .ptau's layout validated and its header (zkfl_ptau_parse; host only, no device)."""
    addr, length, keep = _buffer_address(buf)
    h = PtauHeader()
    rc = lib().zkfl_ptau_parse(addr, length, C.byref(h))
    del keep
    check(rc)
    return h.as_dict()


class PtauReport:
    """One ptau check: ``checks`` maps each of PTAU_CHECKS to "pass" / "fail" / "not run";
    ``prepared``, ``power``; ``point`` = (section, lowest bad index, count) when the points check
    fails; ``chunks`` = the chunk passes that ran; ``error`` = the library's message naming the
    first failing check."""

    def __init__(self, rc: int, rep: PtauReportC, error: str):
        self.rc = rc
        self.ok = rc == ZKFL_OK
        self.error = error
        self.status = [int(x) for x in rep.status]
        self.checks = {name: KEY_STATES[rep.status[i]] for i, name in enumerate(PTAU_CHECKS)}
        self.failed = [name for name in PTAU_CHECKS if self.checks[name] == "fail"]
        self.first_failed = self.failed[0] if self.failed else None
        self.prepared = bool(rep.prepared)
        self.power = int(rep.power)
        self.chunks = int(rep.chunks)
        self.point = ((rep.point_section, rep.point_index, rep.point_count)
                      if self.checks["POINTS"] == "fail" else None)

    def lines(self) -> list:
        """One line per check, as `powersoftau check` prints them."""
        out = []
        for name in PTAU_CHECKS:
            line = f"{name}: {self.checks[name]}"
            if name == "POINTS" and self.point:
                line += f" (section {self.point[0]}, point {self.point[1]}, {self.point[2]} bad)"
            if name in PTAU_LAGRANGE_CHECKS and not self.prepared:
                line += " (not prepared)"
            out.append(line)
        return out

    def __repr__(self):
        return f"PtauReport({'ok' if self.ok else self.error})"


def r1cs_header(r1cs: bytes) -> dict:
    """A .r1cs validated as a whole and its header counts (zkfl_r1cs_parse; host only, no device)."""
    h = R1csHeader()
    check(lib().zkfl_r1cs_parse(r1cs, len(r1cs), C.byref(h)))
    return h.as_dict()


class R1cs(_Handle):
    """A circuit's .r1cs on the device, to check witnesses against (`snarkjs wtns check`)."""
    _free = "zkfl_r1cs_free"

    def __init__(self, ctx: Context, r1cs: bytes):
        h = _P()
        check(lib().zkfl_r1cs_load(ctx.h, r1cs, len(r1cs), C.byref(h)))
        self.h, self.ctx = h, ctx
        ctx._own(self)

    def info(self) -> dict:
        h = R1csHeader()
        check(lib().zkfl_r1cs_info(self.h, C.byref(h)))
        return h.as_dict()

    def _finish(self, rc, reps, n, reports):
        """-> the n reports; with reports=False the call's verdict alone (True: all satisfied)."""
        if rc not in (ZKFL_OK, -7):
            check(rc)
        self.last_error = lib().zkfl_last_error().decode(errors="replace") if rc else ""
        return [Report(reps[i]) for i in range(n)] if reports else rc == ZKFL_OK

    def check(self, wtns_list, reports: bool = True):
        """.wtns images -> [Report] (one batch, one copy back); a malformed witness, one of another
        length or with a value >= r raises ZkflError.  ``last_error`` keeps the library's message,
        which names the lowest failing witness and its first constraint."""
        n = len(wtns_list)
        arr = (C.c_char_p * max(1, n))(*wtns_list)
        lens = (C.c_size_t * max(1, n))(*[len(w) for w in wtns_list])
        reps = (R1csReport * max(1, n))() if reports else None
        return self._finish(lib().zkfl_r1cs_check(self.ctx.h, self.h, n, arr, lens, reps), reps, n, reports)

    def check_resident(self, ws, reports: bool = True):
        """The same for device-resident witnesses (ProvingKey.upload, WitnessProgram.compute_resident)."""
        n = len(ws)
        arr = (_P * max(1, n))(*[w.h for w in ws])
        reps = (R1csReport * max(1, n))() if reports else None
        return self._finish(lib().zkfl_r1cs_check_resident(self.ctx.h, self.h, n, arr, reps), reps, n, reports)

    def check_key(self, zkey: bytes, blocks: dict, rho: bytes | None = None, sigma: bytes | None = None):
        """zkfl_zkey_check: is ``zkey`` this circuit's Groth16 key over the ptau whose blocks are
        given?  blocks: power, L, L2, La, Lb, H0, alpha1, beta1, beta2 (zkfl/zkey.py::ptau_blocks).
        rho / sigma: None draws them from the OS CSPRNG; bytes (n_wires / domainSize x 32 B std) are
        for tests and forfeit soundness.  -> KeyReport; unusable arguments raise ZkflError."""
        keep = {k: bytes(blocks[k]) for k in ("L", "L2", "La", "Lb", "H0", "alpha1", "beta1", "beta2")}
        view = PtauView(power=int(blocks["power"]), L_len=len(keep["L"]), L2_len=len(keep["L2"]),
                        La_len=len(keep["La"]), Lb_len=len(keep["Lb"]), H0_len=len(keep["H0"]), **keep)
        rep = ZkeyReport()
        rc = lib().zkfl_zkey_check(self.ctx.h, self.h, zkey, len(zkey), C.byref(view), rho, sigma, C.byref(rep))
        if rc not in (ZKFL_OK, -8):
            check(rc)
        return KeyReport(rc, rep, lib().zkfl_last_error().decode(errors="replace") if rc else "")


class KeyReport:
    """One key check: ``checks`` maps each of KEY_CHECKS to "pass" / "fail" / "not run"; ``point``
    = (section, lowest bad index, count) when the points check fails, ``coef`` = (matrix, first
    row, count) when the coefficients differ; ``error`` = the library's message naming the first
    failing check."""

    def __init__(self, rc: int, rep: ZkeyReport, error: str):
        self.rc = rc
        self.ok = rc == ZKFL_OK
        self.error = error
        self.checks = {name: KEY_STATES[rep.status[i]] for i, name in enumerate(KEY_CHECKS)}
        self.failed = [name for name in KEY_CHECKS if self.checks[name] == "fail"]
        self.first_failed = self.failed[0] if self.failed else None
        self.point = ((rep.point_section, rep.point_index, rep.point_count)
                      if self.checks["points"] == "fail" else None)
        self.coef = ((rep.coef_matrix, rep.coef_row, rep.coef_count)
                     if self.checks["coefficients"] == "fail" else None)

    def lines(self) -> list:
        """One line per check, as `zkey check` prints them."""
        out = []
        for name in KEY_CHECKS:
            line = f"{name}: {self.checks[name]}"
            if name == "points" and self.point:
                line += f" (section {self.point[0]}, point {self.point[1]}, {self.point[2]} bad)"
            if name == "coefficients" and self.coef:
                line += f" (matrix {self.coef[0]}, row {self.coef[1]}, {self.coef[2]} rows differ)"
            out.append(line)
        return out
