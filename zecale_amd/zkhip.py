"""ctypes binding of the C ABI in include/zkhip.h (libzkhip.so, built in-tree by
__graft_entry__.build()).  Plain pointers and sizes only; numpy arrays carry the limbs.
There is no CPU implementation behind these calls: without the HIP library or a gfx950
device they raise."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZKHIP_LIB: another build of the same library (A/B builds, the mutation run of tools/mutation_abc5.sh); default: the in-tree one
LIB_PATH = os.environ.get("ZKHIP_LIB") or os.path.join(_HERE, "libzkhip.so")

EXPORTS = [
    "zkhip_init", "zkhip_set_device", "zkhip_get_device", "zkhip_device_count", "zkhip_fr_random", "zkhip_shutdown", "zkhip_strerror", "zkhip_last_error", "zkhip_set_msm_window", "zkhip_set_affine_levels",
    "zkhip_bases_upload", "zkhip_bases_upload_dev", "zkhip_bases_len", "zkhip_bases_free",
    "zkhip_bases_precompute", "zkhip_bases_table_window", "zkhip_set_crs_precompute", "zkhip_crs_table_window", "zkhip_set_batch_msms",
    "zkhip_msm", "zkhip_msm_dev", "zkhip_msm_raw", "zkhip_msm_submit", "zkhip_msm_collect",
    "zkhip_device_alloc", "zkhip_device_free", "zkhip_device_copy_in", "zkhip_last_accumulate_ms", "zkhip_last_accumulate_entries", "zkhip_prover_last_accumulate_entries",
    "zkhip_prover_set_streaming", "zkhip_set_table_naf", "zkhip_set_table_model", "zkhip_bases_table_model", "zkhip_fixed_base_mul", "zkhip_fixed_base_mul_dev", "zkhip_ntt", "zkhip_ntt_dev",
    "zkhip_r1cs_upload", "zkhip_r1cs_upload_ex", "zkhip_r1cs_set_domain", "zkhip_r1cs_free", "zkhip_r1cs_log_domain", "zkhip_r1cs_domain_size",
    "zkhip_domain_size", "zkhip_step_domain_size", "zkhip_domain_is_valid", "zkhip_groth16_setup_ex", "zkhip_dispatcher_outstanding", "zkhip_r1cs_is_satisfied", "zkhip_qap_h",
    "zkhip_crs_upload", "zkhip_crs_free", "zkhip_groth16_prove", "zkhip_last_prove_timings", "zkhip_groth16_verify",
    "zkhip_crs_upload_slice", "zkhip_groth16_prove_partial", "zkhip_groth16_finish",
    "zkhip_bls12_377_groth16_verify", "zkhip_aggregator_new", "zkhip_aggregator_free", "zkhip_aggregator_num_constraints",
    "zkhip_aggregator_num_variables", "zkhip_aggregator_num_primary_inputs", "zkhip_aggregator_get_r1cs",
    "zkhip_aggregator_witness", "zkhip_aggregator_witness_gpu", "zkhip_gpu_witness_new", "zkhip_gpu_witness_new_batched", "zkhip_gpu_witness_run", "zkhip_gpu_witness_run_batched", "zkhip_gpu_witness_free",
    "zkhip_gpu_witness_stats", "zkhip_prover_prove_dev", "zkhip_aggregator_check_inputs", "zkhip_aggregator_vk_hash", "zkhip_aggregator_num_proofs", "zkhip_aggregator_inputs_per_proof",
    "zkhip_prover_new", "zkhip_prover_create_streams", "zkhip_prover_prove", "zkhip_prover_timings", "zkhip_prover_free", "zkhip_prover_last_accumulate_ms",
    "zkhip_aggregator_pipeline_new", "zkhip_aggregator_pipeline_new_ex", "zkhip_crs_device", "zkhip_aggregator_pipeline_submit", "zkhip_aggregator_pipeline_wait", "zkhip_aggregator_pipeline_free",
    "zkhip_groth16_setup", "zkhip_groth16_setup_slice", "zkhip_keypair_crs_desc", "zkhip_keypair_vk", "zkhip_keypair_free", "zkhip_keypair_write", "zkhip_keypair_read",
    "zkhip_jac_to_affine", "zkhip_jac_add", "zkhip_to_canonical",
    "zkhip_last_accumulate_interval", "zkhip_crs_upload_ex", "zkhip_crs_upload_slice_ex", "zkhip_bases_precompute_ex", "zkhip_crs_table_kind", "zkhip_crs_finite_terms",
    "zkhip_bases_set_window", "zkhip_reset_time_base", "zkhip_measure_fq_mul_rate", "zkhip_internal_field_selftest", "zkhip_internal_field_ops_selftest", "zkhip_internal_point_ops_selftest", "zkhip_internal_tail_selftest", "zkhip_internal_pipeline_witness_sizing", "zkhip_internal_witness_run_program", "zkhip_internal_witness_run_program_wide", "zkhip_internal_witness_tape", "zkhip_internal_gpu_witness_run", "zkhip_internal_gpu_witness_run_wide", "zkhip_gpu_witness_set_waves", "zkhip_gpu_witness_plan", "zkhip_gpu_witness_last_ms", "zkhip_device_memory", "zkhip_last_prove_split", "zkhip_set_prove_split", "zkhip_host_alloc", "zkhip_host_free",
    "zkhip_msm_stream_new", "zkhip_msm_stream_submit", "zkhip_msm_stream_submit_host", "zkhip_msm_stream_collect", "zkhip_msm_stream_last_accumulate_ms",
    "zkhip_msm_stream_last_accumulate_interval", "zkhip_msm_stream_free", "zkhip_prover_new_slice", "zkhip_prover_prove_partial",
    "zkhip_dispatcher_new", "zkhip_dispatcher_size", "zkhip_dispatcher_submit", "zkhip_dispatcher_wait", "zkhip_dispatcher_stats", "zkhip_dispatcher_free",
    "zkhip_multi_prover_new", "zkhip_multi_prover_size", "zkhip_multi_prover_prove", "zkhip_multi_prover_timings", "zkhip_multi_prover_free",
    "zkhip_aggregator_app_new", "zkhip_aggregator_app_free", "zkhip_aggregator_app_num_constants", "zkhip_aggregator_app_constants", "zkhip_aggregator_app_mask",
    "zkhip_aggregator_witness_app", "zkhip_groth16_prove_app", "zkhip_prover_prove_app", "zkhip_prover_prove_app_dev", "zkhip_gpu_witness_run_batched_app",
    "zkhip_aggregator_pipeline_register_app", "zkhip_aggregator_pipeline_app_hits", "zkhip_dispatcher_register_app", "zkhip_device_copy_out", "zkhip_measure_ntt", "zkhip_key_partition", "zkhip_prover_timings_chained",
    "zkhip_verifier_new", "zkhip_verifier_num_inputs", "zkhip_verifier_verify_batch", "zkhip_verifier_free", "zkhip_internal_fq6_selftest", "zkhip_internal_pairing_product", "zkhip_internal_set_lockstep", "zkhip_internal_last_acc_path", "zkhip_internal_msm_tail",
    "zkhip_internal_set_msm_stream_layout",
    "zkhip_crs_table_model", "zkhip_prover_last_table_model", "zkhip_last_prove_table_model", "zkhip_internal_msm_multi",
    "zkhip_verifier_new_checked", "zkhip_verifier_verify_batch_checked", "zkhip_bw6_761_point_check", "zkhip_groth16_verify_checked",
    "zkhip_nested_verifier_new", "zkhip_nested_verifier_num_inputs", "zkhip_nested_verifier_verify_batch", "zkhip_nested_verifier_last_fallbacks",
    "zkhip_nested_verifier_free", "zkhip_internal_fq12_selftest", "zkhip_internal_nested_pairing_product",
    "zkhip_nested_verifier_new_checked", "zkhip_nested_verifier_verify_batch_checked", "zkhip_bls12_377_point_check", "zkhip_bls12_377_groth16_verify_checked",
    "zkhip_internal_ntt_packed", "zkhip_internal_ntt_set_one_each_max",
    "zkhip_verifier_verify_all", "zkhip_groth16_verify_all", "zkhip_internal_verify_all_value", "zkhip_internal_verify_all_finish_ms",
    "zkhip_nested_verifier_verify_all", "zkhip_nested_verifier_last_degenerate", "zkhip_bls12_377_groth16_verify_all",
    "zkhip_internal_nested_verify_all_value", "zkhip_internal_nested_verify_all_finish_ms",
    "zkhip_verifier_verify_batch_located", "zkhip_groth16_verify_batch_located", "zkhip_internal_verify_batch_located", "zkhip_internal_locate_trace",
    "zkhip_prover_set_checked", "zkhip_prover_last_refusal", "zkhip_crs_check", "zkhip_crs_check_host", "zkhip_internal_key_check_set_chunk", "zkhip_internal_key_check_last_ms",
    "zkhip_keypair_contribute", "zkhip_keypair_contribute_host", "zkhip_phase2_verify", "zkhip_phase2_verify_host", "zkhip_internal_phase2_last_ms", "zkhip_internal_phase2_set_form",
]


class ZkhipError(RuntimeError):
    """A failed C ABI call.  `code` is the library's return code (include/zkhip.h: ZKHIP_ERR_ARG -1, _NO_DEVICE -2, _HIP -3, _STATE -4)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


c_u64p_t = ctypes.POINTER(ctypes.c_uint64)
ERR_REFUSED = -6                  # ZKHIP_ERR_REFUSED: a checked prover refused its input (Prover.set_checked)
REFUSAL_ENCODING, REFUSAL_ONE, REFUSAL_UNSAT, REFUSAL_APP_MASK = 1, 2, 3, 4


class R1csDesc(ctypes.Structure):
    _fields_ = [("n_constraints", ctypes.c_size_t), ("n_vars", ctypes.c_size_t), ("n_primary", ctypes.c_size_t)] + [
        (f"{m}_{k}", ctypes.c_void_p) for m in "abc" for k in ("row_ptr", "col", "val")]


class KeyOpts(ctypes.Structure):
    """zkhip_key_opts: the options of a proving key / base set, carried by the handle (include/zkhip.h)."""
    _fields_ = [("precompute", ctypes.c_int), ("table_naf", ctypes.c_int), ("window", ctypes.c_int), ("batch_msms", ctypes.c_int),
                ("table_model", ctypes.c_int)]


TABLE_MODELS = {"xyzz": 0, "edwards": 1}


def key_opts(precompute=None, table_naf=None, window=0, batch_msms=None, table_model=None):
    """None = the process-wide default (the deprecated zkhip_set_* switches), True / False = this key's own choice.
    table_model: None / 0 / "xyzz" = XYZZ (default); 1 / "edwards" = the key's G1 query vectors also get Edwards tables and the G1 MSMs
    of its proofs add in that model (needs tables, one level per window: include/zkhip.h)."""
    t = lambda v: -1 if v is None else int(bool(v))
    model = 0 if table_model is None else TABLE_MODELS[table_model] if isinstance(table_model, str) else int(table_model)
    return KeyOpts(t(precompute), t(table_naf), int(window or 0), t(batch_msms), model)


class CrsDesc(ctypes.Structure):
    _fields_ = [("n_vars", ctypes.c_size_t), ("n_primary", ctypes.c_size_t), ("domain_size", ctypes.c_size_t)] + [
        (k, ctypes.c_void_p) for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2",
                                       "a_query", "b_g2_query", "b_g1_query", "h_query", "l_query")]


KEY_ELEMENTS = ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2", "a_query", "b_g2_query", "b_g1_query", "h_query", "l_query", "vk_abc")
KEY_PAIRS = ("beta_g1/beta_g2", "delta_g1/delta_g2", "b_g1_query/b_g2_query")
VERIFY_CODES = {0: "fine", 2: "ENCODING", 3: "OFF_CURVE", 4: "NOT_ORDER_R"}
NONE_INDEX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1      # (size_t)-1: "none" in a key report


class KeyElementReport(ctypes.Structure):
    """zkhip_key_element_report: points, those at infinity, refusals by code (ENCODING, OFF_CURVE, NOT_ORDER_R), the first refused index."""
    _fields_ = [("points", ctypes.c_size_t), ("infinity", ctypes.c_size_t), ("refused", ctypes.c_size_t * 3), ("first_refused", ctypes.c_size_t),
                ("first_code", ctypes.c_int)]

    def fields(self):
        return (int(self.points), int(self.infinity), tuple(int(v) for v in self.refused),
                None if self.first_refused == NONE_INDEX else int(self.first_refused), int(self.first_code))


class KeyReport(ctypes.Structure):
    """zkhip_key_report (include/zkhip.h: zkhip_crs_check).  `ok` is the verdict; fields() is the whole report as plain Python values
    ((size_t)-1 as None), describe() names what was refused: element, index and code."""
    _fields_ = [("e", KeyElementReport * len(KEY_ELEMENTS)), ("pairs", ctypes.c_int), ("pairs_evaluated", ctypes.c_int),
                ("b_infinity_mismatch", ctypes.c_size_t), ("structure", ctypes.c_int), ("structure_first", ctypes.c_size_t), ("ok", ctypes.c_int)]

    def fields(self):
        none = lambda v: None if v == NONE_INDEX else int(v)
        return dict(elements={name: self.e[k].fields() for k, name in enumerate(KEY_ELEMENTS)}, pairs=int(self.pairs),
                    pairs_evaluated=int(self.pairs_evaluated), b_infinity_mismatch=none(self.b_infinity_mismatch), structure=int(self.structure),
                    structure_first=none(self.structure_first), ok=int(self.ok))

    def describe(self):
        if self.ok:
            return "key check: ok"
        out = []
        for k, name in enumerate(KEY_ELEMENTS):
            if self.e[k].first_refused != NONE_INDEX:
                out.append("%s[%d]: %s (%d of %d points refused)" % (name, self.e[k].first_refused, VERIFY_CODES[self.e[k].first_code],
                                                                     sum(self.e[k].refused), self.e[k].points))
        for b, name in enumerate(KEY_PAIRS):
            if self.pairs >> b & 1:
                out.append("%s: the two are not the same multiple of their generators" % name)
            elif not self.pairs_evaluated >> b & 1:
                out.append("%s: not evaluated (a point was refused)" % name)
        if self.b_infinity_mismatch != NONE_INDEX:
            out.append("b_g1_query[%d] / b_g2_query[%d]: exactly one is the point at infinity" % ((self.b_infinity_mismatch,) * 2))
        if self.structure:
            where = "its length" if self.structure_first == NONE_INDEX else "index %d" % self.structure_first
            out.append("%s: %s disagrees with the constraint system" % (KEY_ELEMENTS[self.structure], where))
        return "key check: " + "; ".join(out)


class Contribution(ctypes.Structure):
    """zkhip_phase2_contribution: the record of one phase-2 contribution - the new delta in both groups, the commitment T and the
    response z (canonical) of the proof of knowledge.  to_bytes() / from_bytes(): the 624 bytes the transcript link hashes."""
    _fields_ = [("delta_g1", ctypes.c_uint64 * 24), ("delta_g2", ctypes.c_uint64 * 24), ("pok_commit", ctypes.c_uint64 * 24),
                ("pok_response", ctypes.c_uint64 * 6)]

    def to_bytes(self):
        return bytes(self)

    @classmethod
    def from_bytes(cls, b):
        if len(b) != ctypes.sizeof(cls):
            raise ZkhipError("a contribution record is %d bytes" % ctypes.sizeof(cls), -1)
        return cls.from_buffer_copy(b)


PHASE2_ELEMENTS = ("delta_g1", "delta_g2", "h", "l", "pok_commit")
PHASE2_RELATIONS = ("delta_g1'/delta_g2'", "ratio of H | L to delta", "proof of knowledge of s")


class Phase2Report(ctypes.Structure):
    """zkhip_phase2_report (include/zkhip.h: zkhip_phase2_verify).  `ok` is the verdict; fields() is the whole report as plain Python
    values ((size_t)-1 as None), describe() names what was refused."""
    _fields_ = [("changed", ctypes.c_int)] + [(k, KeyElementReport) for k in PHASE2_ELEMENTS] + [
        ("infinity_mismatch", ctypes.c_int), ("infinity_mismatch_first", ctypes.c_size_t), ("relations", ctypes.c_int),
        ("relations_evaluated", ctypes.c_int), ("ok", ctypes.c_int)]

    def fields(self):
        none = lambda v: None if v == NONE_INDEX else int(v)
        return dict(changed=int(self.changed) & 0xFFFFFFFF, elements={k: getattr(self, k).fields() for k in PHASE2_ELEMENTS},
                    infinity_mismatch=int(self.infinity_mismatch), infinity_mismatch_first=none(self.infinity_mismatch_first),
                    relations=int(self.relations), relations_evaluated=int(self.relations_evaluated), ok=int(self.ok))

    def describe(self):
        if self.ok:
            return "phase 2: ok"
        out = []
        changed = int(self.changed) & 0xFFFFFFFF
        if changed >> 31:
            return "phase 2: the two keys have different sizes"
        for k, name in enumerate(KEY_ELEMENTS):
            if changed >> k & 1:
                out.append("%s: %s" % (name, "the record's is not the new key's" if name.startswith("delta") else "changed"))
        for name in PHASE2_ELEMENTS:
            e = getattr(self, name)
            if e.first_refused != NONE_INDEX:
                out.append("%s'[%d]: %s (%d of %d points refused)" % (name, e.first_refused, VERIFY_CODES[e.first_code], sum(e.refused), e.points))
            elif name in ("delta_g1", "delta_g2", "pok_commit") and e.infinity:
                out.append("%s': the point at infinity" % name)
        if self.infinity_mismatch:
            out.append("%s[%d]: at infinity in exactly one of the two keys" % (KEY_ELEMENTS[self.infinity_mismatch], self.infinity_mismatch_first))
        for b, name in enumerate(PHASE2_RELATIONS):
            if self.relations >> b & 1:
                out.append("%s: fails" % name)
            elif not self.relations_evaluated >> b & 1:
                out.append("%s: not evaluated (a point was refused)" % name)
        return "phase 2: " + "; ".join(out)


class LocateStats(ctypes.Structure):
    """zkhip_locate_stats: what a located batch did"""
    _fields_ = [("chunks_failed", ctypes.c_uint32), ("rounds", ctypes.c_uint32), ("node_tests", ctypes.c_uint32), ("finish_proofs", ctypes.c_uint32),
                ("invalid", ctypes.c_uint32), ("descent_ms", ctypes.c_double), ("finish_ms", ctypes.c_double)]

    def fields(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LocateNode(ctypes.Structure):
    """zkhip_locate_node: one tested node of a located batch"""
    _fields_ = [("chunk", ctypes.c_uint32), ("level", ctypes.c_uint32), ("passed", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("index", ctypes.c_uint64), ("value", ctypes.c_uint64 * 72)]


class WitnessProgram(ctypes.Structure):
    """zkhip_witness_program: a laid-out program of the GPU witness interpreter (include/zkhip.h)."""
    _fields_ = [("code", ctypes.c_void_p), ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("n_pos", ctypes.c_size_t), ("level_start", ctypes.c_void_p),
                ("n_levels", ctypes.c_size_t), ("chain_start", ctypes.c_uint32), ("out_ref", ctypes.c_void_p), ("n_vars", ctypes.c_size_t),
                ("consts", ctypes.c_void_p), ("n_consts", ctypes.c_size_t), ("n_inputs", ctypes.c_size_t)]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZkhipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(the HIP library is the only compute path; there is no CPU fallback)")
    # several prover instances run on their own streams: more hardware queues than the runtime's default 4
    # (only effective if the HIP runtime has not been initialised yet in this process)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    lib = ctypes.CDLL(LIB_PATH)
    c_u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.zkhip_init.argtypes = [ctypes.c_int]
    lib.zkhip_set_device.argtypes = [ctypes.c_int]
    lib.zkhip_strerror.restype = ctypes.c_char_p
    lib.zkhip_strerror.argtypes = [ctypes.c_int]
    lib.zkhip_last_error.restype = ctypes.c_char_p
    lib.zkhip_set_msm_window.argtypes = [ctypes.c_int]
    lib.zkhip_bases_upload.argtypes = [c_u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_bases_upload_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_bases_len.restype = ctypes.c_size_t
    lib.zkhip_bases_len.argtypes = [ctypes.c_void_p]
    lib.zkhip_bases_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_bases_precompute.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.zkhip_bases_table_window.argtypes = [ctypes.c_void_p]
    lib.zkhip_set_crs_precompute.argtypes = [ctypes.c_int]
    lib.zkhip_crs_table_window.argtypes = [ctypes.c_void_p]
    lib.zkhip_msm.argtypes = [ctypes.c_void_p, ctypes.c_size_t, c_u64p, ctypes.c_size_t, ctypes.c_int, c_u64p]
    lib.zkhip_msm_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, c_u64p]
    lib.zkhip_msm_submit.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    lib.zkhip_msm_collect.argtypes = [ctypes.c_int, c_u64p]
    lib.zkhip_device_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_device_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_device_copy_in.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.zkhip_msm_raw.argtypes = [c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_int, c_u64p]
    lib.zkhip_fixed_base_mul.argtypes = [c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_int, c_u64p]
    lib.zkhip_fixed_base_mul_dev.argtypes = [c_u64p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lib.zkhip_ntt.argtypes = [c_u64p, ctypes.c_uint, ctypes.c_int, ctypes.c_int]
    lib.zkhip_ntt_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int]
    lib.zkhip_r1cs_upload.argtypes = [ctypes.POINTER(R1csDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_r1cs_upload_ex.argtypes = [ctypes.POINTER(R1csDesc), ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_r1cs_set_domain.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.zkhip_step_domain_size.argtypes = [ctypes.c_size_t]
    lib.zkhip_step_domain_size.restype = ctypes.c_size_t
    lib.zkhip_domain_is_valid.argtypes = [ctypes.c_size_t]
    lib.zkhip_r1cs_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_r1cs_log_domain.argtypes = [ctypes.c_void_p]
    lib.zkhip_r1cs_log_domain.restype = ctypes.c_uint
    lib.zkhip_r1cs_domain_size.argtypes = [ctypes.c_void_p]
    lib.zkhip_r1cs_domain_size.restype = ctypes.c_size_t
    lib.zkhip_domain_size.argtypes = [ctypes.c_size_t]
    lib.zkhip_domain_size.restype = ctypes.c_size_t
    lib.zkhip_r1cs_is_satisfied.argtypes = [ctypes.c_void_p, c_u64p, ctypes.POINTER(ctypes.c_int)]
    lib.zkhip_qap_h.argtypes = [ctypes.c_void_p, c_u64p, c_u64p]
    lib.zkhip_crs_upload.argtypes = [ctypes.POINTER(CrsDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_crs_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_crs_upload_ex.argtypes = [ctypes.POINTER(CrsDesc), ctypes.POINTER(KeyOpts), ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_crs_upload_slice_ex.argtypes = [ctypes.POINTER(CrsDesc)] + [ctypes.c_size_t] * 6 + [ctypes.POINTER(KeyOpts), ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_crs_table_kind.argtypes = [ctypes.c_void_p]
    lib.zkhip_crs_finite_terms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    lib.zkhip_bases_precompute_ex.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.zkhip_groth16_prove.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64p, c_u64p, c_u64p, c_u64p]
    lib.zkhip_last_prove_timings.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zkhip_crs_upload_slice.argtypes = [ctypes.POINTER(CrsDesc)] + [ctypes.c_size_t] * 6 + [ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_groth16_prove_partial.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, c_u64p]
    lib.zkhip_groth16_finish.argtypes = [c_u64p] * 9
    lib.zkhip_groth16_verify.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, ctypes.POINTER(ctypes.c_int)]
    lib.zkhip_last_accumulate_ms.restype = ctypes.c_float
    lib.zkhip_last_accumulate_entries.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    lib.zkhip_prover_last_accumulate_entries.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    lib.zkhip_jac_to_affine.argtypes = [c_u64p, c_u64p]
    lib.zkhip_jac_add.argtypes = [c_u64p, c_u64p, c_u64p]
    lib.zkhip_keypair_write.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.zkhip_keypair_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_prover_new.argtypes = [ctypes.c_void_p, ctypes.POINTER(R1csDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_prover_create_streams.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.zkhip_prover_set_streaming.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.zkhip_prover_prove.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, c_u64p, c_u64p]
    lib.zkhip_prover_timings.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.zkhip_prover_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_prover_last_accumulate_ms.argtypes = [ctypes.c_void_p]
    lib.zkhip_prover_last_accumulate_ms.restype = ctypes.c_float
    vpp = ctypes.POINTER(ctypes.c_void_p)
    lib.zkhip_host_alloc.argtypes = [ctypes.c_size_t, vpp]
    lib.zkhip_host_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_msm_stream_new.argtypes = [ctypes.c_void_p, ctypes.c_int, vpp]
    lib.zkhip_msm_stream_submit.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, c_u64p]
    lib.zkhip_msm_stream_submit_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, c_u64p]
    lib.zkhip_msm_stream_collect.argtypes = [ctypes.c_void_p, ctypes.c_uint64, c_u64p]
    lib.zkhip_msm_stream_last_accumulate_ms.argtypes = [ctypes.c_void_p]
    lib.zkhip_msm_stream_last_accumulate_ms.restype = ctypes.c_float
    lib.zkhip_msm_stream_last_accumulate_interval.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.zkhip_msm_stream_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_prover_new_slice.argtypes = [ctypes.c_void_p, ctypes.POINTER(R1csDesc), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vpp]
    lib.zkhip_prover_prove_partial.argtypes = [ctypes.c_void_p, c_u64p, c_u64p]
    lib.zkhip_dispatcher_new.argtypes = [ctypes.c_void_p, ctypes.POINTER(CrsDesc), ctypes.POINTER(KeyOpts), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_uint, vpp]
    lib.zkhip_dispatcher_size.argtypes = [ctypes.c_void_p]
    lib.zkhip_dispatcher_submit.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, c_u64p, c_u64p, c_u64p, c_u64p]
    lib.zkhip_dispatcher_wait.argtypes = [ctypes.c_void_p, ctypes.c_uint64, c_u64p, c_u64p]
    lib.zkhip_dispatcher_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    lib.zkhip_dispatcher_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_multi_prover_new.argtypes = [ctypes.POINTER(CrsDesc), ctypes.POINTER(R1csDesc), ctypes.POINTER(KeyOpts), ctypes.POINTER(ctypes.c_int), ctypes.c_int, vpp]
    lib.zkhip_multi_prover_size.argtypes = [ctypes.c_void_p]
    lib.zkhip_multi_prover_prove.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, c_u64p, c_u64p]
    lib.zkhip_multi_prover_timings.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.zkhip_multi_prover_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_aggregator_pipeline_new.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.zkhip_aggregator_pipeline_submit.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, c_u64p, c_u64p, c_u64p, ctypes.POINTER(ctypes.c_uint64)]
    lib.zkhip_aggregator_pipeline_wait.argtypes = [ctypes.c_void_p, ctypes.c_uint64, c_u64p, c_u64p]
    lib.zkhip_aggregator_pipeline_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_verifier_new.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, vpp]
    lib.zkhip_verifier_num_inputs.argtypes = [ctypes.c_void_p]
    lib.zkhip_verifier_num_inputs.restype = ctypes.c_size_t
    lib.zkhip_verifier_verify_batch.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_void_p]
    lib.zkhip_verifier_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_verifier_new_checked.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, vpp]
    lib.zkhip_verifier_verify_batch_checked.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_void_p]
    lib.zkhip_bw6_761_point_check.argtypes = [c_u64p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.zkhip_groth16_verify_checked.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, ctypes.c_void_p]
    lib.zkhip_verifier_verify_all.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    lib.zkhip_groth16_verify_all.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, c_u64p, ctypes.c_size_t, c_u64p,
                                             ctypes.POINTER(ctypes.c_int)]
    lib.zkhip_internal_verify_all_value.argtypes = [ctypes.c_int, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, c_u64p]
    lib.zkhip_internal_verify_all_finish_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.zkhip_internal_fq6_selftest.argtypes = [ctypes.c_int, c_u64p, c_u64p, ctypes.c_size_t, c_u64p]
    lib.zkhip_internal_pairing_product.argtypes = [ctypes.c_int, c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_size_t, c_u64p]
    lib.zkhip_nested_verifier_new.argtypes = [c_u64p, ctypes.c_size_t, vpp]
    lib.zkhip_nested_verifier_num_inputs.argtypes = [ctypes.c_void_p]
    lib.zkhip_nested_verifier_num_inputs.restype = ctypes.c_size_t
    lib.zkhip_nested_verifier_verify_batch.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_void_p]
    lib.zkhip_nested_verifier_last_fallbacks.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    lib.zkhip_nested_verifier_free.argtypes = [ctypes.c_void_p]
    lib.zkhip_nested_verifier_new_checked.argtypes = [c_u64p, ctypes.c_size_t, vpp]
    lib.zkhip_nested_verifier_verify_batch_checked.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_void_p]
    lib.zkhip_bls12_377_point_check.argtypes = [c_u64p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.zkhip_bls12_377_groth16_verify_checked.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, c_u64p, c_u64p, ctypes.c_void_p]
    lib.zkhip_internal_fq12_selftest.argtypes = [ctypes.c_int, c_u64p, c_u64p, ctypes.c_size_t, c_u64p]
    lib.zkhip_internal_nested_pairing_product.argtypes = [ctypes.c_int, c_u64p, c_u64p, ctypes.c_size_t, ctypes.c_size_t, c_u64p]
    lib.zkhip_nested_verifier_verify_all.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    lib.zkhip_nested_verifier_last_degenerate.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    lib.zkhip_bls12_377_groth16_verify_all.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, c_u64p, ctypes.c_size_t, c_u64p,
                                                       ctypes.POINTER(ctypes.c_int)]
    lib.zkhip_internal_nested_verify_all_value.argtypes = [ctypes.c_int, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, c_u64p]
    lib.zkhip_internal_nested_verify_all_finish_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    if hasattr(lib, "zkhip_verifier_verify_batch_located"):      # (as below: an older build has no located batches)
        stp = ctypes.POINTER(LocateStats)
        lib.zkhip_verifier_verify_batch_located.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, ctypes.c_void_p, stp]
        lib.zkhip_groth16_verify_batch_located.argtypes = [c_u64p, c_u64p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, c_u64p, ctypes.c_size_t, c_u64p,
                                                           ctypes.c_void_p, stp]
        lib.zkhip_internal_verify_batch_located.argtypes = [ctypes.c_int, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_size_t, c_u64p, ctypes.c_void_p, stp, c_u64p]
        lib.zkhip_internal_locate_trace.argtypes = [ctypes.c_void_p, ctypes.POINTER(LocateNode), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(lib, "zkhip_crs_check"):      # (ZKHIP_LIB may name an older build of the library: tools/key_check_ab.py measures against one)
        for f in (lib.zkhip_crs_check, lib.zkhip_crs_check_host):
            f.argtypes = [ctypes.POINTER(CrsDesc), c_u64p, ctypes.POINTER(R1csDesc), c_u64p, ctypes.POINTER(KeyReport)]
        lib.zkhip_prover_set_checked.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.zkhip_prover_last_refusal.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
        lib.zkhip_internal_key_check_set_chunk.argtypes = [ctypes.c_size_t]
        lib.zkhip_internal_key_check_last_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    if hasattr(lib, "zkhip_keypair_contribute"):      # (as above: an older build has no phase-2 contributions)
        u8p = ctypes.c_char_p
        for f in (lib.zkhip_keypair_contribute, lib.zkhip_keypair_contribute_host):
            f.argtypes = [ctypes.c_void_p, c_u64p, c_u64p, u8p, vpp, ctypes.POINTER(Contribution), ctypes.c_void_p]
        for f in (lib.zkhip_phase2_verify, lib.zkhip_phase2_verify_host):
            f.argtypes = [ctypes.POINTER(CrsDesc), ctypes.POINTER(CrsDesc), ctypes.POINTER(Contribution), u8p, c_u64p, ctypes.POINTER(Phase2Report),
                          ctypes.c_void_p]
        lib.zkhip_internal_phase2_last_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
        lib.zkhip_internal_phase2_set_form.argtypes = [ctypes.c_int]
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        lib = load()
        raise ZkhipError(f"zkhip error {rc} ({lib.zkhip_strerror(rc).decode()}): {lib.zkhip_last_error().decode()}", rc)


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def init(device=0):
    _check(load().zkhip_init(device))


def set_device(device):
    """Library device of the calling thread for the entry points without a handle (handles carry their own device)."""
    _check(load().zkhip_set_device(device))


def get_device():
    return load().zkhip_get_device()


def device_count():
    return load().zkhip_device_count()


def fr_random():
    """One uniform element of Fr (6 Montgomery limbs) from the OS entropy source."""
    out = np.zeros(6, dtype=np.uint64)
    _check(load().zkhip_fr_random(_p(out)))
    return out


def set_msm_window(c):
    _check(load().zkhip_set_msm_window(c))


def set_affine_levels(levels):
    """Batched-affine levels in front of the XYZZ bucket accumulation: -1 automatic, 0 none, up to 4."""
    _check(load().zkhip_set_affine_levels(int(levels)))


def set_batch_msms(on):
    """Table-backed keys: run the five MSMs of a proof through one launch sequence (default) or one each."""
    _check(load().zkhip_set_batch_msms(int(bool(on))))


def set_table_naf(on):
    """window tables with every bit position + non-adjacent-form scalars (zkhip_set_table_naf): 1 on, 0 off, -1 environment"""
    _check(load().zkhip_set_table_naf(int(on)))


def set_table_model(model):
    """point model of the single MSMs over window tables built from now on (zkhip_set_table_model): 1 Edwards, 0 XYZZ, -1 environment"""
    _check(load().zkhip_set_table_model(int(model)))


def set_crs_precompute(on):
    """Whether Crs uploads build window tables for the five query vectors (default: on)."""
    _check(load().zkhip_set_crs_precompute(int(bool(on))))


class Bases:
    """A base-point set resident in HBM (the proving key's query vectors)."""

    def __init__(self, handle):
        self.handle = handle

    @classmethod
    def upload(cls, bases_affine):
        a = np.ascontiguousarray(bases_affine, dtype=np.uint64).reshape(-1, 24)
        h = ctypes.c_void_p()
        _check(load().zkhip_bases_upload(_p(a), a.shape[0], ctypes.byref(h)))
        return cls(h)

    @classmethod
    def upload_dev(cls, dev_ptr, n):
        h = ctypes.c_void_p()
        _check(load().zkhip_bases_upload_dev(ctypes.c_void_p(dev_ptr), n, ctypes.byref(h)))
        return cls(h)

    def __len__(self):
        return load().zkhip_bases_len(self.handle)

    def precompute(self, c=0, table_naf=None):
        """Build the window table (2^(c w) P_i for every window position): all later msm calls use it.
        table_naf: None = the process default, True = every bit position + NAF scalars, False = one level per window."""
        _check(load().zkhip_bases_precompute_ex(self.handle, c, -1 if table_naf is None else int(bool(table_naf))))
        return self

    @property
    def table_window(self):
        return load().zkhip_bases_table_window(self.handle)

    @property
    def table_model(self):
        """1: single MSMs over this set accumulate on G1's 2-isogenous Edwards curve, 0: in XYZZ"""
        load().zkhip_bases_table_model.argtypes = [ctypes.c_void_p]
        return load().zkhip_bases_table_model(self.handle)

    def set_window(self, c):
        """Plain base set: window of the MSMs over it (0 = by the number of terms); an option of this handle."""
        load().zkhip_bases_set_window.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _check(load().zkhip_bases_set_window(self.handle, int(c)))
        return self

    def free(self):
        if self.handle:
            load().zkhip_bases_free(self.handle)
            self.handle = None

    def msm(self, scalars, offset=0, montgomery=True):
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 6)
        out = np.zeros(36, dtype=np.uint64)
        _check(load().zkhip_msm(self.handle, offset, _p(s), s.shape[0], int(montgomery), _p(out)))
        return out

    def msm_submit(self, dev_ptr, n, slot, offset=0, montgomery=True):
        """Enqueue an MSM on `slot` (0..7) and return; msm_collect(slot) waits for the result."""
        _check(load().zkhip_msm_submit(self.handle, offset, ctypes.c_void_p(dev_ptr), n, int(montgomery), slot))

    def msm_dev(self, dev_ptr, n, offset=0, montgomery=True):
        out = np.zeros(36, dtype=np.uint64)
        _check(load().zkhip_msm_dev(self.handle, offset, ctypes.c_void_p(dev_ptr), n, int(montgomery), _p(out)))
        return out


class MsmStream:
    """A stream of MSMs over one resident base set behind a handle (zkhip_msm_stream_*): `depth` MSMs in flight on contexts the
    stream owns.  submit() returns a ticket, collect(ticket) the Jacobian sum (ticket 0 / None: the oldest in flight)."""

    def __init__(self, bases, depth=8):
        h = ctypes.c_void_p()
        _check(load().zkhip_msm_stream_new(bases.handle, depth, ctypes.byref(h)))
        self.handle, self.depth, self._bases = h, depth, bases

    def submit(self, dev_ptr, n, offset=0, montgomery=True):
        t = ctypes.c_uint64(0)
        _check(load().zkhip_msm_stream_submit(self.handle, offset, ctypes.c_void_p(dev_ptr), n, int(montgomery), ctypes.byref(t)))
        return t.value

    def submit_host(self, host_ptr, n, offset=0, montgomery=True):
        """host_ptr: address of n x 6 u64 in host memory (a numpy array's ctypes.data, or a PinnedBuffer's ptr); it must stay valid
        until the ticket is collected."""
        t = ctypes.c_uint64(0)
        _check(load().zkhip_msm_stream_submit_host(self.handle, offset, ctypes.c_void_p(host_ptr), n, int(montgomery), ctypes.byref(t)))
        return t.value

    def collect(self, ticket=None):
        out = np.zeros(36, dtype=np.uint64)
        _check(load().zkhip_msm_stream_collect(self.handle, int(ticket or 0), _p(out)))
        return out

    def last_accumulate_ms(self):
        return float(load().zkhip_msm_stream_last_accumulate_ms(self.handle))

    def last_accumulate_interval(self):
        t = (ctypes.c_float * 2)()
        _check(load().zkhip_msm_stream_last_accumulate_interval(self.handle, t))
        return float(t[0]), float(t[1])

    def free(self):
        if self.handle:
            load().zkhip_msm_stream_free(self.handle)
            self.handle = None


class PinnedBuffer:
    """Pinned host memory owned by the library (zkhip_host_alloc) holding a copy of `host_array`: the source of asynchronous uploads."""

    def __init__(self, host_array):
        a = np.ascontiguousarray(host_array)
        p = ctypes.c_void_p()
        _check(load().zkhip_host_alloc(a.nbytes, ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, a.nbytes
        ctypes.memmove(self.ptr, a.ctypes.data, a.nbytes)

    def free(self):
        if self.ptr:
            load().zkhip_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


class DeviceBuffer:
    """A host array copied into device memory owned by the library (for the *_dev / submit entry points)."""

    def __init__(self, host_array):
        a = np.ascontiguousarray(host_array)
        p = ctypes.c_void_p()
        _check(load().zkhip_device_alloc(a.nbytes, ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, a.nbytes
        _check(load().zkhip_device_copy_in(ctypes.c_void_p(self.ptr), a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    def free(self):
        if self.ptr:
            load().zkhip_device_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


def msm_collect(slot):
    out = np.zeros(36, dtype=np.uint64)
    _check(load().zkhip_msm_collect(slot, _p(out)))
    return out


def msm_raw(bases_affine, scalars, montgomery=True):
    a = np.ascontiguousarray(bases_affine, dtype=np.uint64).reshape(-1, 24)
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 6)
    assert a.shape[0] == s.shape[0]
    out = np.zeros(36, dtype=np.uint64)
    _check(load().zkhip_msm_raw(_p(a), _p(s), a.shape[0], int(montgomery), _p(out)))
    return out


def fixed_base_mul(base_affine, scalars, montgomery=True):
    """out[i] = scalars[i] * base (affine, n x 24 limbs) - the batch exponentiation of Groth16 setup."""
    b = np.ascontiguousarray(base_affine, dtype=np.uint64).reshape(24)
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 6)
    out = np.zeros((s.shape[0], 24), dtype=np.uint64)
    _check(load().zkhip_fixed_base_mul(_p(b), _p(s), s.shape[0], int(montgomery), _p(out)))
    return out


def fixed_base_mul_dev(base_affine, d_scalars_ptr, n, d_out_ptr, montgomery=True):
    b = np.ascontiguousarray(base_affine, dtype=np.uint64).reshape(24)
    _check(load().zkhip_fixed_base_mul_dev(_p(b), ctypes.c_void_p(d_scalars_ptr), n, int(montgomery), ctypes.c_void_p(d_out_ptr)))


def ntt(data, log_d, inverse=False, coset=False):
    """FFT / iFFT / cosetFFT / icosetFFT of 2^log_d Fr elements (n x 6 limbs); returns a new array."""
    a = np.array(data, dtype=np.uint64).reshape(-1, 6).copy()
    assert a.shape[0] == 1 << log_d
    _check(load().zkhip_ntt(_p(a), log_d, int(inverse), int(coset)))
    return a


def ntt_dev(dev_ptr, log_d, inverse=False, coset=False):
    _check(load().zkhip_ntt_dev(ctypes.c_void_p(dev_ptr), log_d, int(inverse), int(coset)))


def make_r1cs_desc(A, B, C, n_vars, n_primary):
    """zkhip_r1cs_desc over CSR triples (row_ptr u32[n+1], col u32[nnz], val u64[nnz, 6]).  Returns (desc, keep): `keep` holds
    the arrays the descriptor points into and must stay alive while the descriptor is used (e.g. for Prover(crs, desc))."""
    keep = []
    d = R1csDesc()
    d.n_constraints = len(A[0]) - 1
    d.n_vars, d.n_primary = n_vars, n_primary
    for name, (rp, col, val) in zip("abc", (A, B, C)):
        rp = np.ascontiguousarray(rp, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 6)
        assert len(rp) == d.n_constraints + 1 and len(col) == len(val) == int(rp[-1])
        keep += [rp, col, val]
        setattr(d, name + "_row_ptr", rp.ctypes.data)
        setattr(d, name + "_col", col.ctypes.data if len(col) else None)
        setattr(d, name + "_val", val.ctypes.data if len(val) else None)
    return d, keep


DOMAIN_DEFAULT = 0                # ZKHIP_DOMAIN_DEFAULT: the reference's forced power of two (libzeth passes force_pow_2_domain = true)
DOMAIN_STEP = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1     # ZKHIP_DOMAIN_STEP: libfqfft's unforced choice (2^k or 2^k + 2^r)


def _domain_arg(domain):
    return ctypes.c_size_t(DOMAIN_DEFAULT if not domain else (DOMAIN_STEP if domain in ("step", -1, DOMAIN_STEP) else int(domain)))


class R1cs:
    """A constraint system resident in HBM.  A, B, C: CSR triples (row_ptr u32[n+1], col u32[nnz], val u64[nnz, 6]).
    domain: None = the reference's forced power-of-two evaluation domain; "step" = libfqfft's unforced choice; an int = that many
    points (what a proving key says).  zkhip_groth16_prove moves the handle to its key's domain by itself."""

    def __init__(self, A, B, C, n_vars, n_primary, domain=None):
        self._keep = []
        d = R1csDesc()
        d.n_constraints = len(A[0]) - 1
        d.n_vars, d.n_primary = n_vars, n_primary
        for name, (rp, col, val) in zip("abc", (A, B, C)):
            rp = np.ascontiguousarray(rp, dtype=np.uint32)
            col = np.ascontiguousarray(col, dtype=np.uint32)
            val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 6)
            assert len(rp) == d.n_constraints + 1 and len(col) == len(val) == int(rp[-1])
            self._keep += [rp, col, val]
            setattr(d, name + "_row_ptr", rp.ctypes.data)
            setattr(d, name + "_col", col.ctypes.data if len(col) else None)
            setattr(d, name + "_val", val.ctypes.data if len(val) else None)
        self.n_vars, self.n_primary, self.n_constraints = n_vars, n_primary, d.n_constraints
        h = ctypes.c_void_p()
        _check(load().zkhip_r1cs_upload_ex(ctypes.byref(d), _domain_arg(domain), ctypes.byref(h)))
        self.handle = h
        self._keep = []

    @property
    def log_d(self):
        return int(load().zkhip_r1cs_log_domain(self.handle))

    @property
    def domain_size(self):
        """Points of the handle's CURRENT domain: a power of two (default), or 2^k + 2^r (libfqfft's step_radix2_domain)."""
        return int(load().zkhip_r1cs_domain_size(self.handle))

    def set_domain(self, domain):
        _check(load().zkhip_r1cs_set_domain(self.handle, _domain_arg(domain)))

    def is_satisfied(self, z):
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(self.n_vars, 6)
        ok = ctypes.c_int(0)
        _check(load().zkhip_r1cs_is_satisfied(self.handle, _p(zz), ctypes.byref(ok)))
        return bool(ok.value)

    def qap_h(self, z):
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(self.n_vars, 6)
        h = np.zeros((self.domain_size, 6), dtype=np.uint64)
        _check(load().zkhip_qap_h(self.handle, _p(zz), _p(h)))
        return h

    def free(self):
        if self.handle:
            load().zkhip_r1cs_free(self.handle)
            self.handle = None


class Crs:
    """The Groth16 proving key resident in HBM.  pk: dict with alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2
    (24 limbs) and the query arrays A, B2, B1, H, L (n x 24 limbs)."""

    def __init__(self, pk, n_vars, n_primary, domain_size, opts=None):
        d = CrsDesc()
        d.n_vars, d.n_primary, d.domain_size = n_vars, n_primary, domain_size
        keep = []
        for field, key, rows in (("alpha_g1", "alpha_g1", 1), ("beta_g1", "beta_g1", 1), ("beta_g2", "beta_g2", 1),
                                 ("delta_g1", "delta_g1", 1), ("delta_g2", "delta_g2", 1), ("a_query", "A", n_vars),
                                 ("b_g2_query", "B2", n_vars), ("b_g1_query", "B1", n_vars), ("h_query", "H", domain_size - 1),
                                 ("l_query", "L", n_vars - n_primary - 1)):
            a = np.ascontiguousarray(pk[key], dtype=np.uint64).reshape(-1, 24)  # (extra keys such as "vk" are ignored)
            assert a.shape[0] == rows, (key, a.shape, rows)
            keep.append(a)
            setattr(d, field, a.ctypes.data if a.size else None)
        h = ctypes.c_void_p()
        _check(load().zkhip_crs_upload_ex(ctypes.byref(d), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h)))
        self.handle = h

    @property
    def table_window(self):
        """Window size of the key's precomputed tables (0: plain key)."""
        return load().zkhip_crs_table_window(self.handle)

    @property
    def table_kind(self):
        """0: plain key, 1: one table level per window, 2: every bit position (scalars in non-adjacent form)."""
        return load().zkhip_crs_table_kind(self.handle)

    @property
    def table_model(self):
        """1: the key's G1 MSMs add on G1's 2-isogenous Edwards curve (key_opts(table_model=1) took effect), 0: XYZZ."""
        lib = load()
        lib.zkhip_crs_table_model.argtypes = [ctypes.c_void_p]
        return lib.zkhip_crs_table_model(self.handle)

    def finite_terms(self):
        """Bases of A, B-G2, B-G1, H, L that are not the point at infinity (the terms an MSM over the key can have)."""
        out = (ctypes.c_size_t * 5)()
        _check(load().zkhip_crs_finite_terms(self.handle, out))
        return [int(v) for v in out]

    def free(self):
        if self.handle:
            load().zkhip_crs_free(self.handle)
            self.handle = None

    @classmethod
    def upload_slice(cls, pk, n_vars, n_primary, domain_size, a_range, h_range, l_range, opts=None):
        """This rank's slice of the proving key: ranges are (lo, hi) into the A/B queries, the H query and the L query."""
        d = CrsDesc()
        d.n_vars, d.n_primary, d.domain_size = n_vars, n_primary, domain_size
        keep = []
        for field, key in (("alpha_g1", "alpha_g1"), ("beta_g1", "beta_g1"), ("beta_g2", "beta_g2"), ("delta_g1", "delta_g1"),
                           ("delta_g2", "delta_g2"), ("a_query", "A"), ("b_g2_query", "B2"), ("b_g1_query", "B1"), ("h_query", "H"),
                           ("l_query", "L")):
            a = np.ascontiguousarray(pk[key], dtype=np.uint64).reshape(-1, 24)
            keep.append(a)
            setattr(d, field, a.ctypes.data if a.size else None)
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        _check(load().zkhip_crs_upload_slice_ex(ctypes.byref(d), a_range[0], a_range[1] - a_range[0], h_range[0], h_range[1] - h_range[0],
                                                l_range[0], l_range[1] - l_range[0], ctypes.byref(opts) if opts is not None else None,
                                                ctypes.byref(h)))
        self.handle = h
        self.ranges = (a_range, h_range, l_range)
        return self


def key_partition(pk, n_vars, n_primary, domain_size, parts):
    """zkhip_key_partition on host arrays: (a_cuts, h_cuts, l_cuts), parts + 1 values each.  Host code, no device."""
    d = CrsDesc()
    d.n_vars, d.n_primary, d.domain_size = n_vars, n_primary, domain_size
    keep = []
    for field, key in (("a_query", "A"), ("b_g2_query", "B2"), ("b_g1_query", "B1"), ("h_query", "H"), ("l_query", "L")):
        a = np.ascontiguousarray(pk[key], dtype=np.uint64).reshape(-1, 24)
        keep.append(a)
        setattr(d, field, a.ctypes.data if len(a) else None)
    cuts = [(ctypes.c_size_t * (parts + 1))() for _ in range(3)]
    lib = load()
    lib.zkhip_key_partition.argtypes = [ctypes.POINTER(CrsDesc), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.zkhip_key_partition(ctypes.byref(d), parts, cuts[0], cuts[1], cuts[2]))
    return tuple([int(x) for x in c] for c in cuts)


def crs_from_slice_arrays(consts, slices, n_vars, n_primary, domain_size, a_range, h_range, l_range):
    """Like Crs.upload_slice, but from arrays that hold ONLY this rank's slices (A, B2, B1: a_hi - a_lo points; H; L):
    what a rank of a multi-GPU job keeps in host memory.  consts: alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2."""
    d = CrsDesc()
    d.n_vars, d.n_primary, d.domain_size = n_vars, n_primary, domain_size
    keep = []
    for field in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2"):
        a = np.ascontiguousarray(consts[field], dtype=np.uint64).reshape(24)
        keep.append(a)
        setattr(d, field, a.ctypes.data)
    for field, key, lo, n in (("a_query", "A", a_range[0], a_range[1] - a_range[0]), ("b_g2_query", "B2", a_range[0], a_range[1] - a_range[0]),
                              ("b_g1_query", "B1", a_range[0], a_range[1] - a_range[0]), ("h_query", "H", h_range[0], h_range[1] - h_range[0]),
                              ("l_query", "L", l_range[0], l_range[1] - l_range[0])):
        a = np.ascontiguousarray(slices[key], dtype=np.uint64).reshape(-1, 24)
        assert a.shape[0] == n, (key, a.shape, n)
        keep.append(a)
        # the descriptor addresses the FULL vector: element `lo` of it is the first element of this slice
        setattr(d, field, (a.ctypes.data - lo * 192) if n else None)
    c = Crs.__new__(Crs)
    h = ctypes.c_void_p()
    _check(load().zkhip_crs_upload_slice(ctypes.byref(d), a_range[0], a_range[1] - a_range[0], h_range[0], h_range[1] - h_range[0],
                                         l_range[0], l_range[1] - l_range[0], ctypes.byref(h)))
    c.handle = h
    c.ranges = (a_range, h_range, l_range)
    return c


def groth16_prove_partial(crs_slice, r1cs, z):
    """The five partial sums (5 x 36 limbs) of this rank's key slice."""
    zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(r1cs.n_vars, 6)
    out = np.zeros((5, 36), dtype=np.uint64)
    (a0, _), (h0, _), (l0, _) = crs_slice.ranges
    _check(load().zkhip_groth16_prove_partial(crs_slice.handle, r1cs.handle, _p(zz), a0, h0, l0, _p(out)))
    return out


def groth16_finish(pk, sums, r, s):
    c = lambda a: _p(np.ascontiguousarray(a, dtype=np.uint64))
    out = np.zeros(72, dtype=np.uint64)
    _check(load().zkhip_groth16_finish(c(pk["alpha_g1"]), c(pk["beta_g1"]), c(pk["beta_g2"]), c(pk["delta_g1"]), c(pk["delta_g2"]),
                                       c(np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1)), c(r), c(s), _p(out)))
    return out


def groth16_prove(crs, r1cs, z, r, s):
    """Proof (A in G1, B in G2, C in G1) as 72 limbs, affine.  r, s: Fr in Montgomery form (6 limbs)."""
    zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(r1cs.n_vars, 6)
    out = np.zeros(72, dtype=np.uint64)
    _check(load().zkhip_groth16_prove(crs.handle, r1cs.handle, _p(zz), _p(np.ascontiguousarray(r, dtype=np.uint64)),
                                      _p(np.ascontiguousarray(s, dtype=np.uint64)), _p(out)))
    return out


def groth16_verify(vk, inputs, proof):
    """vk: dict alpha (G1), beta, delta (G2), ABC ((n+1) x 24 limbs); inputs: n x 6 limbs; proof: 72 limbs.
    Host code: works without a GPU."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    abc = c(vk["ABC"]).reshape(-1, 24)
    inp = c(inputs).reshape(-1, 6)
    assert abc.shape[0] == inp.shape[0] + 1
    ok = ctypes.c_int(0)
    _check(load().zkhip_groth16_verify(_p(c(vk["alpha"])), _p(c(vk["beta"])), _p(c(vk["delta"])), _p(abc), _p(inp), inp.shape[0],
                                       _p(c(proof)), ctypes.byref(ok)))
    return bool(ok.value)


# status of a proof on the checked routes (include/zkhip.h ZKHIP_VERIFY_*): the low nibble of its byte; the high nibble is the mask of
# the elements that fail with that code
VERIFY_ACCEPT, VERIFY_REJECT, VERIFY_ENCODING, VERIFY_OFF_CURVE, VERIFY_NOT_ORDER_R = range(5)
VERIFY_MASK_A, VERIFY_MASK_B, VERIFY_MASK_C, VERIFY_MASK_INPUT = 0x10, 0x20, 0x40, 0x80


def bw6_761_point_check(point, g2):
    """Host code: 0, VERIFY_ENCODING, VERIFY_OFF_CURVE or VERIFY_NOT_ORDER_R for one point (24 limbs, x | y; all zero is the point at
    infinity and passes).  g2: the point belongs on y^2 = x^3 + 4, else on y^2 = x^3 - 1."""
    pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(24)
    code = ctypes.c_int(-1)
    _check(load().zkhip_bw6_761_point_check(_p(pt), 1 if g2 else 0, ctypes.byref(code)))
    return code.value


def groth16_verify_checked(vk, inputs, proof):
    """groth16_verify behind the checks of the checked batch verifier, on the host: returns the proof's status byte (code in the low
    nibble, mask of the failing elements in the high one), the byte Verifier.verify_batch_checked gives.  A key that fails the checks
    raises (ZKHIP_ERR_ARG)."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    abc = c(vk["ABC"]).reshape(-1, 24)
    inp = c(inputs).reshape(-1, 6)
    assert abc.shape[0] == inp.shape[0] + 1
    st = np.zeros(1, dtype=np.uint8)
    _check(load().zkhip_groth16_verify_checked(_p(c(vk["alpha"])), _p(c(vk["beta"])), _p(c(vk["delta"])), _p(abc), _p(inp), inp.shape[0],
                                               _p(c(proof)), st.ctypes.data))
    return int(st[0])


def _rho_limbs(rho, count):
    """None, or count combination scalars (ints below 2^128, or count x 2 words) -> count x 2 words, little endian"""
    if rho is None:
        return None
    if len(rho) and isinstance(rho[0], int):
        rho = [[r & (2 ** 64 - 1), r >> 64] for r in rho]
    return np.ascontiguousarray(rho, dtype=np.uint64).reshape(count, 2)


def groth16_verify_all(vk, inputs, proofs, rho=None):
    """ONE random-combination check of a whole batch on the host (zkhip_groth16_verify_all; works without a GPU): True iff
    prod_i t(rho_i A_i, B_i) t(S_acc, -g2) t(sigma alpha, -beta) t(S_C, -delta) is one.  vk as for groth16_verify; inputs:
    count x n x 6 limbs; proofs: count x 72 limbs; rho: None (drawn from the OS) or count non-zero scalars below 2^128 - supplied
    scalars are for tests and reproducible measurements only."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    abc = c(vk["ABC"]).reshape(-1, 24)
    pr = c(proofs).reshape(-1, 72)
    inp = c(inputs).reshape(pr.shape[0], abc.shape[0] - 1, 6)
    rl = _rho_limbs(rho, pr.shape[0])
    ok = ctypes.c_int(0)
    _check(load().zkhip_groth16_verify_all(_p(c(vk["alpha"])), _p(c(vk["beta"])), _p(c(vk["delta"])), _p(abc), abc.shape[0] - 1, _p(inp), _p(pr),
                                           pr.shape[0], None if rl is None else _p(rl), ctypes.byref(ok)))
    return bool(ok.value)


# the batch verifier's kernels (zecale_amd/csrc/pairing.cuh / pairing.hip): a verification owns eight lanes, so one wave holds
# VERIFIER_GROUP of them and one 128-thread workgroup VERIFIER_WORKGROUP (tests size their batches around both); the reduction trees
# of a combined batch take VERIFIER_STRIP values per strip, and a batch runs in chunks of VERIFIER_CHUNK proofs
VERIFIER_GROUP = 8
VERIFIER_WORKGROUP = 16
VERIFIER_STRIP = 8
VERIFIER_CHUNK = 16384


class Verifier:
    """Groth16 verification in batches on the GPU (zkhip_verifier): the pairing of groth16_verify as gfx950 kernels.  vk as for
    groth16_verify.  The handle owns its stream and work space on the calling thread's device; one batch in flight per handle,
    several handles - one host thread each - run side by side.
    verify_batch checks nothing: every coordinate and input must be fully reduced and every point on its curve and of order r (or
    infinity), or its result is undefined - it is for proofs the caller made.  For anybody else's proofs make the handle with
    checked=True: the key's points are validated on the device (a key that fails raises, the message names the element), and
    verify_batch_checked validates encoding, curve and order of every proof point before the pairing and says per proof why it
    was refused."""

    def __init__(self, vk, checked=False):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        abc = c(vk["ABC"]).reshape(-1, 24)
        self.handle = ctypes.c_void_p()
        self.checked = bool(checked)
        new = load().zkhip_verifier_new_checked if checked else load().zkhip_verifier_new
        _check(new(_p(c(vk["alpha"])), _p(c(vk["beta"])), _p(c(vk["delta"])), _p(abc), abc.shape[0] - 1, ctypes.byref(self.handle)))
        self.n_inputs = int(load().zkhip_verifier_num_inputs(self.handle))

    def verify_batch(self, inputs, proofs):
        """inputs: count x n_inputs x 6 limbs; proofs: count x 72 limbs.  Returns a bool array, one verdict per proof."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        ok = np.zeros(pr.shape[0], dtype=np.uint8)
        _check(load().zkhip_verifier_verify_batch(self.handle, _p(inp), _p(pr), pr.shape[0], ok.ctypes.data))
        return ok.astype(bool)

    def verify_batch_checked(self, inputs, proofs):
        """As verify_batch on a handle made with checked=True, every proof point validated first.  Returns (codes, masks), uint8 arrays:
        codes[i] is VERIFY_ACCEPT, VERIFY_REJECT, or the first of VERIFY_ENCODING, VERIFY_OFF_CURVE, VERIFY_NOT_ORDER_R that an element
        of proof i has; masks[i] the elements that have it (VERIFY_MASK_A | _B | _C | _INPUT, zero for ACCEPT and REJECT)."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        st = np.zeros(pr.shape[0], dtype=np.uint8)
        _check(load().zkhip_verifier_verify_batch_checked(self.handle, _p(inp), _p(pr), pr.shape[0], st.ctypes.data))
        return st & np.uint8(0x0F), st & np.uint8(0xF0)

    def verify_all(self, inputs, proofs, rho=None, status=False):
        """ONE random-combination check of the whole batch (zkhip_verifier_verify_all): True iff every proof is valid, up to a
        chance of about 2^-128 - PROVIDED every point has order r, which an unchecked handle does not check: it is for proofs the
        caller made.  rho: None (drawn from the OS) or count non-zero scalars below 2^128, for tests and reproducible measurements
        only.  status=True (a handle made with checked=True): every proof point is validated first, a refused proof is left out
        and fails the batch; returns (verdict, status bytes: the refusal byte of verify_batch_checked per proof, or 0)."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        rl = _rho_limbs(rho, pr.shape[0])
        st = np.zeros(max(pr.shape[0], 1), dtype=np.uint8) if status else None       # (never zero-length: its address says "status wanted")
        ok = ctypes.c_int(0)
        _check(load().zkhip_verifier_verify_all(self.handle, _p(inp), _p(pr), pr.shape[0], None if rl is None else _p(rl), ctypes.byref(ok),
                                                None if st is None else st.ctypes.data))
        return (bool(ok.value), st[:pr.shape[0]].tobytes()) if status else bool(ok.value)

    def verify_batch_located(self, inputs, proofs, rho=None):
        """Per-proof verdicts by way of the combined check with its trees retained (zkhip_verifier_verify_batch_located): an
        all-valid batch costs what verify_all costs; a batch that fails is searched from the chunk roots down, one host finish per
        round, and the proofs a cost rule finds cheaper to check one by one go through verify_batch's kernels.  Returns what
        verify_batch returns, or on a handle made with checked=True what verify_batch_checked returns (the point checks run in
        front).  rho and the precondition on an unchecked handle: as verify_all."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        rl = _rho_limbs(rho, pr.shape[0])
        out = np.zeros(pr.shape[0], dtype=np.uint8)
        self._locate_stats = LocateStats()
        _check(load().zkhip_verifier_verify_batch_located(self.handle, _p(inp), _p(pr), pr.shape[0], None if rl is None else _p(rl), out.ctypes.data,
                                                          ctypes.byref(self._locate_stats)))
        return (out & np.uint8(0x0F), out & np.uint8(0xF0)) if self.checked else out.astype(bool)

    def last_locate_stats(self):
        """Of the last verify_batch_located on this handle: dict of chunks_failed, rounds, node_tests (the chunk round included),
        finish_proofs (proofs handed to the per-proof route), invalid, descent_ms, finish_ms; None before the first call."""
        st = getattr(self, "_locate_stats", None)
        return None if st is None else st.fields()

    def verify_batch_combined(self, inputs, proofs, locate=False):
        """Per-proof verdicts by way of the combined check: all ones when verify_all passes, and only otherwise the per-proof
        route - verify_batch's bool array, or on a handle made with checked=True verify_batch_checked's (codes, masks), in front
        of which verify_all runs with the point checks.  Measured (profiles/verify_combined.txt) an all-valid batch is
        cheaper this way at EVERY size from one proof on (0.57 of the per-proof batch at 1 proof, 0.54 at 1,024, 0.39 at 16,384): there
        is no batch size below which it does not pay; a batch with an invalid proof costs both routes (1.4 to 1.5 x the per-proof
        one), so it pays where batches are mostly valid.  locate=True: verify_batch_located instead, which finds the invalid proofs
        of a failed batch from the combined check's own trees (profiles/verify_locate.txt)."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
        if locate:
            return self.verify_batch_located(inputs, pr)
        if self.checked:
            if self.verify_all(inputs, pr, status=True)[0]:
                return np.zeros(pr.shape[0], dtype=np.uint8), np.zeros(pr.shape[0], dtype=np.uint8)
            return self.verify_batch_checked(inputs, pr)
        if self.verify_all(inputs, pr):
            return np.ones(pr.shape[0], dtype=bool)
        return self.verify_batch(inputs, pr)

    def last_finish_ms(self):
        """Host time of the last verify_all behind the device's work: the three shared pairs and the final exponentiation."""
        ms = ctypes.c_double(0)
        _check(load().zkhip_internal_verify_all_finish_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def free(self):
        if self.handle:
            load().zkhip_verifier_free(self.handle)
            self.handle = None


def verify_all_value(route, verifier, inputs, proofs, rho):
    """Test hook: the reduced GT value of the combined product of Verifier.verify_all, 6 x 12 ABI limbs.  route "host" or "gpu"; on a
    checked handle both routes leave the proofs out that the point checks refuse."""
    pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
    inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], verifier.n_inputs, 6)
    rl = _rho_limbs(rho, pr.shape[0])
    out = np.zeros((6, 12), dtype=np.uint64)
    _check(load().zkhip_internal_verify_all_value({"host": 0, "gpu": 1}[route], verifier.handle, _p(inp), _p(pr), pr.shape[0], _p(rl), _p(out)))
    return out


def verify_batch_located_value(route, verifier, inputs, proofs, rho):
    """Test hook: Verifier.verify_batch_located by route - "gpu", or "host": the host route under the handle's key - with the batch's
    reduced GT value.  Returns (verdicts as verify_batch_located gives them, value 6 x 12 ABI limbs); Verifier.last_locate_stats and
    locate_trace tell about this call."""
    pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 72)
    inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], verifier.n_inputs, 6)
    rl = _rho_limbs(rho, pr.shape[0])
    out, value = np.zeros(pr.shape[0], dtype=np.uint8), np.zeros((6, 12), dtype=np.uint64)
    verifier._locate_stats = LocateStats()
    _check(load().zkhip_internal_verify_batch_located({"host": 0, "gpu": 1}[route], verifier.handle, _p(inp), _p(pr), pr.shape[0], _p(rl),
                                                      out.ctypes.data, ctypes.byref(verifier._locate_stats), _p(value)))
    return ((out & np.uint8(0x0F), out & np.uint8(0xF0)) if verifier.checked else out.astype(bool)), value


def locate_trace(verifier):
    """Test hook: every node the last verify_batch_located on the handle tested, in the order of the rounds: a list of dicts chunk,
    level (0: a single proof), index, passed, value (the reduced value of the node's combined check, 6 x 12 ABI limbs)."""
    n = ctypes.c_size_t(0)
    _check(load().zkhip_internal_locate_trace(verifier.handle, None, 0, ctypes.byref(n)))
    buf = (LocateNode * max(n.value, 1))()
    _check(load().zkhip_internal_locate_trace(verifier.handle, buf, n.value, ctypes.byref(n)))
    return [{"chunk": int(b.chunk), "level": int(b.level), "index": int(b.index), "passed": bool(b.passed),
             "value": np.array(b.value, dtype=np.uint64).reshape(6, 12)} for b in buf[:n.value]]


def groth16_verify_batch_located(vk, inputs, proofs, rho=None):
    """Per-proof verdicts by way of the combined check on the host alone (zkhip_groth16_verify_batch_located; works without a GPU):
    the route Verifier.verify_batch_located is pinned on.  Arguments as groth16_verify_all.  Returns (bool array, stats dict)."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    abc = c(vk["ABC"]).reshape(-1, 24)
    pr = c(proofs).reshape(-1, 72)
    inp = c(inputs).reshape(pr.shape[0], abc.shape[0] - 1, 6)
    rl = _rho_limbs(rho, pr.shape[0])
    ok, st = np.zeros(pr.shape[0], dtype=np.uint8), LocateStats()
    _check(load().zkhip_groth16_verify_batch_located(_p(c(vk["alpha"])), _p(c(vk["beta"])), _p(c(vk["delta"])), _p(abc), abc.shape[0] - 1, _p(inp), _p(pr),
                                                     pr.shape[0], None if rl is None else _p(rl), ok.ctypes.data, ctypes.byref(st)))
    return ok.astype(bool), st.fields()


def fq6_selftest(op, a, b):
    """Test hook: the pairing kernels' per-lane Fq6 bodies.  op "mul" / "sqr" / "mul_line" (b_0 + b_3 w^3 + b_4 w^4);
    a, b: n x 6 x 12 ABI limbs; returns n x 6 x 12 limbs."""
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 6, 12)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 6, 12)
    assert x.shape == y.shape
    out = np.zeros_like(x)
    _check(load().zkhip_internal_fq6_selftest({"mul": 0, "sqr": 1, "mul_line": 2}[op], _p(x), _p(y), x.shape[0], _p(out)))
    return out


def pairing_product(route, g1, g2):
    """Test hook: reduced GT values of products of pairings.  g1, g2: count x pairs x 24 limbs (pairs <= 4); route "host" or "gpu".
    Returns count x 6 x 12 ABI limbs."""
    x = np.ascontiguousarray(g1, dtype=np.uint64)
    y = np.ascontiguousarray(g2, dtype=np.uint64)
    assert x.ndim == 3 and x.shape == y.shape and x.shape[2] == 24
    out = np.zeros((x.shape[0], 6, 12), dtype=np.uint64)
    _check(load().zkhip_internal_pairing_product({"host": 0, "gpu": 1}[route], _p(x), _p(y), x.shape[1], x.shape[0], _p(out)))
    return out


def bls12_377_groth16_verify(nested_vk, inputs, proof):
    """Nested (BLS12-377) Groth16 verification on the host.  nested_vk: 60 + 12 (k+1) limbs (alpha | beta | delta | ABC);
    inputs: k x 6 limbs; proof: 48 limbs (a | b | c)."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    vk, pr, inp = c(nested_vk), c(proof), c(inputs).reshape(-1, 6)
    assert vk.size == 60 + 12 * (inp.shape[0] + 1) and pr.size == 48
    ok = ctypes.c_int(0)
    _check(load().zkhip_bls12_377_groth16_verify(_p(vk[:12]), _p(vk[12:36]), _p(vk[36:60]), _p(vk[60:]), _p(inp), inp.shape[0],
                                                 _p(pr[:12]), _p(pr[12:36]), _p(pr[36:]), ctypes.byref(ok)))
    return bool(ok.value)


def bls12_377_point_check(point, g2):
    """Host code: 0, VERIFY_ENCODING, VERIFY_OFF_CURVE or VERIFY_NOT_ORDER_R for one nested point: 12 limbs (x | y), or with g2 24
    (x.c0 | x.c1 | y.c0 | y.c1).  The nested format has no point at infinity: all zero is VERIFY_OFF_CURVE."""
    pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(24 if g2 else 12)
    code = ctypes.c_int(-1)
    _check(load().zkhip_bls12_377_point_check(_p(pt), 1 if g2 else 0, ctypes.byref(code)))
    return code.value


def bls12_377_groth16_verify_checked(nested_vk, inputs, proof):
    """bls12_377_groth16_verify behind the checks of the checked nested batch verifier, on the host: returns the proof's status byte
    (code in the low nibble, mask of the failing elements in the high one), the byte NestedVerifier.verify_batch_checked gives.  A key
    that fails the point checks raises (ZKHIP_ERR_ARG, the message names the element and the code)."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    vk, pr, inp = c(nested_vk), c(proof), c(inputs).reshape(-1, 6)
    assert vk.size == 60 + 12 * (inp.shape[0] + 1) and pr.size == 48
    st = np.zeros(1, dtype=np.uint8)
    _check(load().zkhip_bls12_377_groth16_verify_checked(_p(vk[:12]), _p(vk[12:36]), _p(vk[36:60]), _p(vk[60:]), _p(inp), inp.shape[0],
                                                         _p(pr[:12]), _p(pr[12:36]), _p(pr[36:]), st.ctypes.data))
    return int(st[0])


def bls12_377_groth16_verify_all(nested_vk, inputs, proofs, rho=None):
    """ONE random-combination check of a whole batch of nested proofs on the host (zkhip_bls12_377_groth16_verify_all; works without
    a GPU): True iff prod_i e(rho_i A_i, B_i) e(S_acc, -g2) e(sigma alpha, -beta) e(S_C, -delta) is one and no proof has a point off
    its curve.  nested_vk: 60 + 12 (k + 1) limbs; inputs: count x k x 6 limbs; proofs: count x 48 limbs; rho: None (drawn from the OS)
    or count non-zero scalars below 2^128 - supplied scalars are for tests and reproducible measurements only."""
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    vk = c(nested_vk).reshape(-1)
    k = (vk.size - 60) // 12 - 1
    assert k >= 0 and vk.size == 60 + 12 * (k + 1)
    pr = c(proofs).reshape(-1, 48)
    inp = c(inputs).reshape(pr.shape[0], k, 6)
    rl = _rho_limbs(rho, pr.shape[0])
    ok = ctypes.c_int(0)
    _check(load().zkhip_bls12_377_groth16_verify_all(_p(vk[:12]), _p(vk[12:36]), _p(vk[36:60]), _p(vk[60:]), k, _p(inp), _p(pr), pr.shape[0],
                                                     None if rl is None else _p(rl), ctypes.byref(ok)))
    return bool(ok.value)


# the nested batch verifier's kernels (zecale_amd/csrc/pairing_bls.cuh / pairing_bls.hip): a verification owns sixteen lanes, so one
# wave holds NESTED_VERIFIER_GROUP of them and one 128-thread workgroup NESTED_VERIFIER_WORKGROUP; a batch runs in chunks of
# NESTED_VERIFIER_CHUNK proofs; the reduction trees of a combined batch take NESTED_VERIFIER_STRIP values per strip
NESTED_VERIFIER_GROUP = 4
NESTED_VERIFIER_WORKGROUP = 8
NESTED_VERIFIER_CHUNK = 8192
NESTED_VERIFIER_STRIP = 8


class NestedVerifier:
    """Nested (BLS12-377) Groth16 verification in batches on the GPU (zkhip_nested_verifier): the verdicts of bls12_377_groth16_verify
    from gfx950 kernels.  nested_vk: 60 + 12 (k + 1) limbs (alpha | beta | delta | ABC), k = inputs_per_proof.  The key is checked on
    the host when the handle is made (a refused key raises, the message names the element).  One batch in flight per handle; handles
    run side by side, one host thread each.
    verify_batch tests curve membership only: every coordinate and input must be fully reduced, and no point is tested for order r -
    it is for proofs the caller made.  For anybody else's proofs make the handle with checked=True: the key's points are validated on
    the host first (encoding, curve, order; a key that fails raises, the message names the element and the code), and
    verify_batch_checked validates every proof point and input on the device before the pairing and says per proof why it was
    refused."""

    def __init__(self, nested_vk, inputs_per_proof, checked=False):
        vk = np.ascontiguousarray(nested_vk, dtype=np.uint64).reshape(-1)
        assert vk.size == 60 + 12 * (inputs_per_proof + 1)
        self.handle = ctypes.c_void_p()
        self.checked = bool(checked)
        new = load().zkhip_nested_verifier_new_checked if checked else load().zkhip_nested_verifier_new
        _check(new(_p(vk), inputs_per_proof, ctypes.byref(self.handle)))
        self.n_inputs = int(load().zkhip_nested_verifier_num_inputs(self.handle))

    def verify_batch(self, inputs, proofs):
        """inputs: count x n_inputs x 6 limbs; proofs: count x 48 limbs (a | b | c).  Returns a bool array, one verdict per proof."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 48)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        ok = np.zeros(pr.shape[0], dtype=np.uint8)
        _check(load().zkhip_nested_verifier_verify_batch(self.handle, _p(inp), _p(pr), pr.shape[0], ok.ctypes.data))
        return ok.astype(bool)

    def verify_batch_checked(self, inputs, proofs):
        """As verify_batch on a handle made with checked=True, every proof point and input validated first.  Returns (codes, masks),
        uint8 arrays: codes[i] is VERIFY_ACCEPT, VERIFY_REJECT, or the first of VERIFY_ENCODING, VERIFY_OFF_CURVE, VERIFY_NOT_ORDER_R
        that an element of proof i has; masks[i] the elements that have it (VERIFY_MASK_A | _B | _C | _INPUT, zero for ACCEPT and REJECT)."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 48)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        st = np.zeros(pr.shape[0], dtype=np.uint8)
        _check(load().zkhip_nested_verifier_verify_batch_checked(self.handle, _p(inp), _p(pr), pr.shape[0], st.ctypes.data))
        return st & np.uint8(0x0F), st & np.uint8(0xF0)

    def last_fallbacks(self):
        """How many proofs of the last batch the device handed to the host verifier (a degenerate chord-and-tangent step)."""
        n = ctypes.c_size_t(0)
        _check(load().zkhip_nested_verifier_last_fallbacks(self.handle, ctypes.byref(n)))
        return int(n.value)

    def verify_all(self, inputs, proofs, rho=None, status=False):
        """ONE random-combination check of the whole batch (zkhip_nested_verifier_verify_all): True iff every proof is valid, up to a
        chance of about 2^-128 - PROVIDED every point has order r, which an unchecked handle does not check: it is for proofs the
        caller made.  rho: None (drawn from the OS) or count non-zero scalars below 2^128, for tests and reproducible measurements
        only.  status=True (a handle made with checked=True): every proof point and input is validated first, a refused proof is left
        out and fails the batch; returns (verdict, status bytes: the refusal byte of verify_batch_checked per proof, or 0).
        This route answers the GROUP LAW's statement: it ACCEPTS the one kind of valid statement on which verify_batch, like the host
        verifier whose affine accumulator chain it reproduces, says 0 - the accumulator meeting -2^j ABC_i at a clear bit j of input i
        (tests/nested_verify_fixtures.degenerate_statement(8, negated=True)) - and hands no proof to the host (last_fallbacks() is not
        touched).  A proof whose B has a degenerate line schedule fails the batch; last_degenerate() counts them."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 48)
        inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], self.n_inputs, 6)
        rl = _rho_limbs(rho, pr.shape[0])
        st = np.zeros(max(pr.shape[0], 1), dtype=np.uint8) if status else None       # (never zero-length: its address says "status wanted")
        ok = ctypes.c_int(0)
        _check(load().zkhip_nested_verifier_verify_all(self.handle, _p(inp), _p(pr), pr.shape[0], None if rl is None else _p(rl), ctypes.byref(ok),
                                                       None if st is None else st.ctypes.data))
        return (bool(ok.value), st[:pr.shape[0]].tobytes()) if status else bool(ok.value)

    def verify_batch_combined(self, inputs, proofs):
        """Per-proof verdicts by way of the combined check: all ones when verify_all passes, and only otherwise the per-proof route -
        verify_batch's bool array, or on a handle made with checked=True verify_batch_checked's (codes, masks), in front of which
        verify_all runs with the point checks.  Where verify_all passes the answer is the group law's: a statement on which the
        accumulator meets -2^j ABC_i at a clear bit gets 1 here and 0 from verify_batch (see verify_all).  A batch with an invalid
        proof costs both routes; profiles/nested_verify_combined.txt and DESIGN 9e have the measurement."""
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 48)
        if self.checked:
            if self.verify_all(inputs, pr, status=True)[0]:
                return np.zeros(pr.shape[0], dtype=np.uint8), np.zeros(pr.shape[0], dtype=np.uint8)
            return self.verify_batch_checked(inputs, pr)
        if self.verify_all(inputs, pr):
            return np.ones(pr.shape[0], dtype=bool)
        return self.verify_batch(inputs, pr)

    def last_degenerate(self):
        """How many proofs of the last verify_all had a B with a degenerate line schedule (left out; they fail the batch)."""
        n = ctypes.c_size_t(0)
        _check(load().zkhip_nested_verifier_last_degenerate(self.handle, ctypes.byref(n)))
        return int(n.value)

    def last_finish_ms(self):
        """Host time of the last verify_all behind the device's work: the sums, S_acc, the three shared pairs, the final exponentiation."""
        ms = ctypes.c_double(0)
        _check(load().zkhip_internal_nested_verify_all_finish_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def free(self):
        if self.handle:
            load().zkhip_nested_verifier_free(self.handle)
            self.handle = None


def fq12_selftest(op, a, b):
    """Test hook: the nested pairing kernels' per-lane Fq12 bodies.  op "mul" / "sqr" / "mul_line" (b_0 + b_1 w + b_3 w^3 + b_7 w^7 +
    b_9 w^9); a, b: n x 12 x 6 ABI limbs; returns n x 12 x 6 limbs."""
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 12, 6)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 12, 6)
    assert x.shape == y.shape
    out = np.zeros_like(x)
    _check(load().zkhip_internal_fq12_selftest({"mul": 0, "sqr": 1, "mul_line": 2}[op], _p(x), _p(y), x.shape[0], _p(out)))
    return out


def nested_pairing_product(route, g1, g2):
    """Test hook: reduced GT values of products of BLS12-377 pairings.  g1: count x pairs x 12 limbs, g2: count x pairs x 24 (pairs <= 4);
    route "host" or "gpu".  Returns count x 12 x 6 ABI limbs."""
    x = np.ascontiguousarray(g1, dtype=np.uint64)
    y = np.ascontiguousarray(g2, dtype=np.uint64)
    assert x.ndim == 3 and y.ndim == 3 and x.shape[:2] == y.shape[:2] and x.shape[2] == 12 and y.shape[2] == 24
    out = np.zeros((x.shape[0], 12, 6), dtype=np.uint64)
    _check(load().zkhip_internal_nested_pairing_product({"host": 0, "gpu": 1}[route], _p(x), _p(y), x.shape[1], x.shape[0], _p(out)))
    return out


def nested_verify_all_value(route, verifier, inputs, proofs, rho):
    """Test hook: the reduced GT value of the combined product of NestedVerifier.verify_all over the proofs that are not left out,
    12 x 6 ABI limbs.  route "host" or "gpu"; on a checked handle both routes leave the proofs out that the point checks refuse."""
    pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 48)
    inp = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(pr.shape[0], verifier.n_inputs, 6)
    rl = _rho_limbs(rho, pr.shape[0])
    out = np.zeros((12, 6), dtype=np.uint64)
    _check(load().zkhip_internal_nested_verify_all_value({"host": 0, "gpu": 1}[route], verifier.handle, _p(inp), _p(pr), pr.shape[0], _p(rl), _p(out)))
    return out


class AggregatorCircuit:
    """Mirror of libzecale::aggregator_circuit<wpp, wsnark, nverifier, NumProofs> (aggregator_circuit.hpp:32-114):
    builds the wrapping circuit on construction; `witness` performs the generate_r1cs_witness half of prove()."""

    def __init__(self, num_proofs=2, inputs_per_nested_proof=1):
        h = ctypes.c_void_p()
        _check(load().zkhip_aggregator_new(num_proofs, inputs_per_nested_proof, ctypes.byref(h)))
        self.handle = h
        self.num_proofs, self.inputs_per_nested_proof = num_proofs, inputs_per_nested_proof
        lib = load()
        self.num_constraints = lib.zkhip_aggregator_num_constraints(h)
        self.num_variables = lib.zkhip_aggregator_num_variables(h)

    def num_primary_inputs(self):
        return load().zkhip_aggregator_num_primary_inputs(self.handle)

    def get_constraint_system(self):
        """CSR triples (row_ptr, col, val) of A, B, C as numpy arrays (copies)."""
        d = R1csDesc()
        _check(load().zkhip_aggregator_get_r1cs(self.handle, ctypes.byref(d)))
        out = []
        for m in "abc":
            n = d.n_constraints
            rp = np.ctypeslib.as_array(ctypes.cast(getattr(d, m + "_row_ptr"), ctypes.POINTER(ctypes.c_uint32)), (n + 1,)).copy()
            nnz = int(rp[-1])
            col = np.ctypeslib.as_array(ctypes.cast(getattr(d, m + "_col"), ctypes.POINTER(ctypes.c_uint32)), (nnz,)).copy()
            val = np.ctypeslib.as_array(ctypes.cast(getattr(d, m + "_val"), ctypes.POINTER(ctypes.c_uint64)), (nnz, 6)).copy()
            out.append((rp, col, val))
        return out

    def witness(self, nested_vk, nested_proofs, nested_inputs):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        vk, pr, inp = c(nested_vk), c(nested_proofs), c(nested_inputs)
        k = self.inputs_per_nested_proof
        assert vk.size == 60 + 12 * (k + 1) and pr.size == 48 * self.num_proofs and inp.size == 6 * k * self.num_proofs
        z = np.zeros((self.num_variables, 6), dtype=np.uint64)
        _check(load().zkhip_aggregator_witness(self.handle, _p(vk), _p(pr), _p(inp), _p(z)))
        return z

    def witness_gpu(self, nested_vk, nested_proofs, nested_inputs):
        """The same assignment computed on the GPU (zkhip_aggregator_witness_gpu): needs zkhip.init()."""
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        vk, pr, inp = c(nested_vk), c(nested_proofs), c(nested_inputs)
        k = self.inputs_per_nested_proof
        assert vk.size == 60 + 12 * (k + 1) and pr.size == 48 * self.num_proofs and inp.size == 6 * k * self.num_proofs
        z = np.zeros((self.num_variables, 6), dtype=np.uint64)
        _check(load().zkhip_aggregator_witness_gpu(self.handle, _p(vk), _p(pr), _p(inp), _p(z)))
        return z

    def witness_gpu_batched(self, batches, wpg=None, segment=None, app=None, waves=None):
        """batches: list of (nested_vk, nested_proofs, nested_inputs) -> (assignments u64 [n, n_vars, 6], degenerate bool [n], primary
        inputs) from ONE launch sequence of the circuit's generic program (what zkhip_gpu_witness_run_batched runs), or of `app`'s own
        program (zkhip_gpu_witness_run_batched_app: nested_vk is ignored and the assignments are masked), through the test hook
        zkhip_internal_gpu_witness_run.  wpg (witnesses per workgroup: 1, 2, 4) and segment (chunks per
        launch) reach witness_launch as given; None = the process-wide default.  waves: waves per witness (1: k_witness; 2, 4, 8, 16:
        k_witness_wide; 0: auto); None = 1, the narrow kernel, through the hook without the argument.  A degenerate batch's
        assignment is unusable."""
        lib = load()
        n, m, l = len(batches), self.num_variables, self.num_primary_inputs()
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        k = self.inputs_per_nested_proof
        vks, prs, ins = [c(b[0]) for b in batches], [c(b[1]) for b in batches], [c(b[2]) for b in batches]
        assert all(v.size == 60 + 12 * (k + 1) for v in vks) and all(x.size == 48 * self.num_proofs for x in prs) and all(x.size == 6 * k * self.num_proofs for x in ins)
        gw = ctypes.c_void_p()
        lib.zkhip_gpu_witness_new_batched.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        _check(lib.zkhip_gpu_witness_new_batched(self.handle, n, ctypes.byref(gw)))
        dz = ctypes.c_void_p()
        try:
            _check(lib.zkhip_device_alloc(n * m * 48, ctypes.byref(dz)))
            arr = lambda xs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in xs])
            prim = np.zeros((n, l, 6), dtype=np.uint64)
            deg = (ctypes.c_int * n)()
            args = [gw, app.handle if app is not None else None, n, None if app is not None else arr(vks), arr(prs), arr(ins), dz, _p(prim), deg, int(wpg or 0), int(segment or 0)]
            types = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                     c_u64p_t, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_uint]
            if waves is None:
                lib.zkhip_internal_gpu_witness_run.argtypes = types
                _check(lib.zkhip_internal_gpu_witness_run(*args))
            else:
                lib.zkhip_internal_gpu_witness_run_wide.argtypes = types + [ctypes.c_int]
                _check(lib.zkhip_internal_gpu_witness_run_wide(*args, int(waves)))
            z = np.zeros((n, m, 6), dtype=np.uint64)
            lib.zkhip_device_copy_out.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            _check(lib.zkhip_device_copy_out(z.ctypes.data, dz, n * m * 48))
            return z, np.array([bool(deg[i]) for i in range(n)]), prim
        finally:
            if dz:
                lib.zkhip_device_free(dz)
            lib.zkhip_gpu_witness_free(gw)

    def witness_tape(self):
        """Test hook, host only: the recorded program of the circuit as the GPU generator uploads it (a dict of numpy copies, the
        layout of witness_run_program)."""
        wp = WitnessProgram()
        _check(load().zkhip_internal_witness_tape(self.handle, ctypes.byref(wp)))
        cp = lambda ptr, n, dt: np.frombuffer(ctypes.string_at(ptr, n * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
        return dict(code=cp(wp.code, wp.n_pos, np.uint8), a=cp(wp.a, wp.n_pos, np.int32), b=cp(wp.b, wp.n_pos, np.int32),
                    level_start=cp(wp.level_start, wp.n_levels + 1, np.uint32), chain_start=int(wp.chain_start), out_ref=cp(wp.out_ref, wp.n_vars, np.int32),
                    consts=cp(wp.consts, wp.n_consts * 6, np.uint64).reshape(-1, 6), n_inputs=int(wp.n_inputs))

    def gpu_witness_plan(self, waves=0):
        """Host only (zkhip_gpu_witness_plan): what the circuit's recorded program asks of the device with `waves` waves per witness
        (0 = the width auto picks): dict of chunks, levels, waves, steps (sum over levels of ceil(chunks / waves)), value_bytes."""
        lib = load()
        lib.zkhip_gpu_witness_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
        out = (ctypes.c_size_t * 4)()
        _check(lib.zkhip_gpu_witness_plan(self.handle, int(waves), out))
        if int(waves) == 0:
            waves = int(out[2])
            _check(lib.zkhip_gpu_witness_plan(self.handle, waves, out))
        return dict(chunks=int(out[0]), levels=int(out[1]), waves=int(waves), steps=int(out[2]), value_bytes=int(out[3]))

    def gpu_witness_stats(self):
        out = (ctypes.c_size_t * 6)()
        _check(load().zkhip_gpu_witness_stats(self.handle, out))
        return dict(zip(["recorded", "positions", "levels", "multiplications", "inversions", "constants"], [int(x) for x in out]))

    def check_inputs(self, nested_vk, nested_proofs):
        """True iff every point of the nested key and proofs is on its curve (proof.is_well_formed() in the reference's stack)."""
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        ok = ctypes.c_int(0)
        _check(load().zkhip_aggregator_check_inputs(self.handle, _p(c(nested_vk)), _p(c(nested_proofs)), ctypes.byref(ok)))
        return bool(ok.value)

    def free(self):
        if self.handle:
            load().zkhip_aggregator_free(self.handle)
            self.handle = None


class GpuWitness:
    """zkhip_gpu_witness: work space for up to max_batches witnesses in flight and the device buffer their assignments are left in.
    waves: waves per witness of the levelled program (zkhip_gpu_witness_set_waves: 1, 2, 4, 8, 16; 0 or None = auto)."""

    def __init__(self, agg, max_batches=1, waves=None):
        lib = load()
        self._agg, self.max_batches, self.handle, self.d_z = agg, int(max_batches), None, None
        gw = ctypes.c_void_p()
        lib.zkhip_gpu_witness_new_batched.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        _check(lib.zkhip_gpu_witness_new_batched(agg.handle, self.max_batches, ctypes.byref(gw)))
        self.handle = gw
        try:
            self.set_waves(waves or 0)
            dz = ctypes.c_void_p()
            _check(lib.zkhip_device_alloc(self.max_batches * agg.num_variables * 48, ctypes.byref(dz)))
            self.d_z = dz
        except Exception:
            self.free()
            raise

    def set_waves(self, waves):
        lib = load()
        lib.zkhip_gpu_witness_set_waves.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _check(lib.zkhip_gpu_witness_set_waves(self.handle, int(waves)))

    def run(self, batches):
        """batches: list of (nested_vk, nested_proofs, nested_inputs) -> (device pointers of the assignments (integers, valid until the
        next run), degenerate bool [n], primary inputs u64 [n, n_primary, 6]): zkhip_gpu_witness_run_batched"""
        lib = load()
        n, m, l = len(batches), self._agg.num_variables, self._agg.num_primary_inputs()
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        vks, prs, ins = [c(b[0]) for b in batches], [c(b[1]) for b in batches], [c(b[2]) for b in batches]
        arr = lambda xs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in xs])
        prim = np.zeros((n, l, 6), dtype=np.uint64)
        deg = (ctypes.c_int * n)()
        lib.zkhip_gpu_witness_run_batched.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_u64p_t,
                                                      ctypes.POINTER(ctypes.c_int)]
        _check(lib.zkhip_gpu_witness_run_batched(self.handle, n, arr(vks), arr(prs), arr(ins), self.d_z, _p(prim), deg))
        return [int(self.d_z.value) + i * m * 48 for i in range(n)], np.array([bool(deg[i]) for i in range(n)]), prim

    def last_ms(self):
        """milliseconds the kernels of the last run took on the device (zkhip_gpu_witness_last_ms)"""
        lib = load()
        lib.zkhip_gpu_witness_last_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        ms = ctypes.c_double(0)
        _check(lib.zkhip_gpu_witness_last_ms(self.handle, ctypes.byref(ms)))
        return float(ms.value)

    def copy_out(self, i):
        m = self._agg.num_variables
        z = np.zeros((m, 6), dtype=np.uint64)
        lib = load()
        lib.zkhip_device_copy_out.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        _check(lib.zkhip_device_copy_out(z.ctypes.data, ctypes.c_void_p(int(self.d_z.value) + i * m * 48), m * 48))
        return z

    def free(self):
        lib = load()
        if self.d_z:
            lib.zkhip_device_free(self.d_z)
            self.d_z = None
        if self.handle:
            lib.zkhip_gpu_witness_free(self.handle)
            self.handle = None


class AggregatorApp:
    """A registered application (zkhip_aggregator_app; RegisterApplication in the reference, aggregator_server.cpp:170-235): the
    constants of its nested key for one proving key - positions, values, the four cached points - computed once.  `witness` gives
    the MASKED assignment of a batch (zeros at those positions), `prove` the same proof as groth16_prove on the full one."""

    def __init__(self, agg, crs, nested_vk):
        vk = np.ascontiguousarray(nested_vk, dtype=np.uint64).reshape(-1)
        assert vk.size == 60 + 12 * (agg.inputs_per_nested_proof + 1)
        h = ctypes.c_void_p()
        lib = load()
        lib.zkhip_aggregator_app_new.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, ctypes.POINTER(ctypes.c_void_p)]
        _check(lib.zkhip_aggregator_app_new(agg.handle, crs.handle, _p(vk), ctypes.byref(h)))
        self.handle, self._agg, self._crs = h, agg, crs
        lib.zkhip_aggregator_app_num_constants.restype = ctypes.c_size_t
        lib.zkhip_aggregator_app_num_constants.argtypes = [ctypes.c_void_p]
        self.num_constants = int(lib.zkhip_aggregator_app_num_constants(h))

    def constants(self):
        """(positions u32[n], values u64[n, 6], vk_hash u64[6], points u64[4, 36])"""
        pos = np.zeros(self.num_constants, dtype=np.uint32)
        val = np.zeros((self.num_constants, 6), dtype=np.uint64)
        h, pts = np.zeros(6, dtype=np.uint64), np.zeros((4, 36), dtype=np.uint64)
        lib = load()
        lib.zkhip_aggregator_app_constants.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, c_u64p_t, c_u64p_t]
        _check(lib.zkhip_aggregator_app_constants(self.handle, pos.ctypes.data, _p(val), _p(h), _p(pts)))
        return pos, val, h, pts

    def mask(self, z):
        """A full assignment generated under this application's key, masked (copy)."""
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 6).copy()
        lib = load()
        lib.zkhip_aggregator_app_mask.argtypes = [ctypes.c_void_p, c_u64p_t]
        _check(lib.zkhip_aggregator_app_mask(self.handle, _p(zz)))
        return zz

    def witness(self, nested_proofs, nested_inputs):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        pr, inp = c(nested_proofs), c(nested_inputs)
        k = self._agg.inputs_per_nested_proof
        assert pr.size == 48 * self._agg.num_proofs and inp.size == 6 * k * self._agg.num_proofs
        z = np.zeros((self._agg.num_variables, 6), dtype=np.uint64)
        lib = load()
        lib.zkhip_aggregator_witness_app.argtypes = [ctypes.c_void_p, c_u64p_t, c_u64p_t, c_u64p_t]
        _check(lib.zkhip_aggregator_witness_app(self.handle, _p(pr), _p(inp), _p(z)))
        return z

    def witness_gpu(self, batches):
        """batches: list of (nested_proofs, nested_inputs) -> list of MASKED assignments generated on the GPU by the application's own
        program in ONE launch sequence (zkhip_gpu_witness_run_batched_app); a degenerate batch yields None."""
        lib = load()
        n, m, l = len(batches), self._agg.num_variables, self._agg.num_primary_inputs()
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        prs, ins = [c(b[0]) for b in batches], [c(b[1]) for b in batches]
        gw = ctypes.c_void_p()
        lib.zkhip_gpu_witness_new_batched.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        _check(lib.zkhip_gpu_witness_new_batched(self._agg.handle, n, ctypes.byref(gw)))
        dz = ctypes.c_void_p()
        _check(lib.zkhip_device_alloc(n * m * 48, ctypes.byref(dz)))
        try:
            arr = lambda xs: (ctypes.c_void_p * n)(*[x.ctypes.data for x in xs])
            prim = np.zeros((n, l, 6), dtype=np.uint64)
            deg = (ctypes.c_int * n)()
            lib.zkhip_gpu_witness_run_batched_app.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, ctypes.POINTER(ctypes.c_int)]
            _check(lib.zkhip_gpu_witness_run_batched_app(gw, self.handle, n, arr(prs), arr(ins), dz, _p(prim), deg))
            z = np.zeros((n, m, 6), dtype=np.uint64)
            lib.zkhip_device_copy_out.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            _check(lib.zkhip_device_copy_out(z.ctypes.data, dz, n * m * 48))
            return [None if deg[i] else z[i] for i in range(n)], prim
        finally:
            lib.zkhip_device_free(dz)
            lib.zkhip_gpu_witness_free(gw)

    def prove(self, r1cs, z_masked, r, s):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        zz, r, s = c(z_masked).reshape(r1cs.n_vars, 6), c(r), c(s)
        out = np.zeros(72, dtype=np.uint64)
        lib = load()
        lib.zkhip_groth16_prove_app.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, c_u64p_t, c_u64p_t, c_u64p_t]
        _check(lib.zkhip_groth16_prove_app(self._crs.handle, r1cs.handle, self.handle, _p(zz), _p(r), _p(s), _p(out)))
        return out

    def free(self):
        if self.handle:
            load().zkhip_aggregator_app_free(self.handle)
            self.handle = None


class Prover:
    """A prover instance (zkhip_prover): own streams and work space, one proof in flight; several instances, one host
    thread each, keep several proofs in flight on one GPU.  `crs` must outlive the instance."""

    def __init__(self, crs, r1cs_desc):
        h = ctypes.c_void_p()
        _check(load().zkhip_prover_new(crs.handle, ctypes.byref(r1cs_desc), ctypes.byref(h)))
        self.handle, self._crs = h, crs

    def prove(self, z, r, s):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        z, r, s = c(z), c(r), c(s)
        out = np.zeros(72, dtype=np.uint64)
        _check(load().zkhip_prover_prove(self.handle, _p(z), _p(r), _p(s), _p(out)))
        return out

    def prove_dev(self, d_z, r, s):
        """zkhip_prover_prove_dev: the assignment already in DEVICE memory (an integer pointer: n_vars x 6 limbs, what GpuWitness.run
        leaves there)."""
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        r, s = c(r), c(s)
        out = np.zeros(72, dtype=np.uint64)
        lib = load()
        lib.zkhip_prover_prove_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, c_u64p_t, c_u64p_t]
        _check(lib.zkhip_prover_prove_dev(self.handle, ctypes.c_void_p(int(d_z)), _p(r), _p(s), _p(out)))
        return out

    def prove_app(self, app, z_masked, r, s):
        """The same proof from a MASKED assignment and the application's constants (zkhip_prover_prove_app)."""
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        z, r, s = c(z_masked), c(r), c(s)
        out = np.zeros(72, dtype=np.uint64)
        lib = load()
        lib.zkhip_prover_prove_app.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, c_u64p_t, c_u64p_t, c_u64p_t]
        _check(lib.zkhip_prover_prove_app(self.handle, app.handle, _p(z), _p(r), _p(s), _p(out)))
        return out

    def prove_app_dev(self, app, d_z_masked, r, s):
        """zkhip_prover_prove_app_dev: the masked assignment already in DEVICE memory (an integer pointer; what the application's GPU
        program writes).  Precondition: it is masked (see include/zkhip.h) - not checked."""
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        r, s = c(r), c(s)
        out = np.zeros(72, dtype=np.uint64)
        lib = load()
        lib.zkhip_prover_prove_app_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_u64p_t, c_u64p_t, c_u64p_t]
        _check(lib.zkhip_prover_prove_app_dev(self.handle, app.handle, ctypes.c_void_p(int(d_z_masked)), _p(r), _p(s), _p(out)))
        return out

    def create_streams(self, which):
        """zkhip_prover_create_streams: for a caller with several instances - which = 0 for all of them, then which = 1 for all"""
        _check(load().zkhip_prover_create_streams(self.handle, int(which)))

    def set_streaming(self, on=True):
        """this instance shares the GPU with others: total work over single-proof latency (zkhip_prover_set_streaming)"""
        _check(load().zkhip_prover_set_streaming(self.handle, int(bool(on))))

    def set_checked(self, on=True):
        """zkhip_prover_set_checked: prove / prove_dev / prove_app / prove_app_dev refuse an assignment that is not reduced, does not
        start with ONE, does not satisfy the system or is not masked: ZkhipError with code ERR_REFUSED (-6), no proof; last_refusal()
        says why.  Proofs of acceptable input are unchanged."""
        _check(load().zkhip_prover_set_checked(self.handle, int(bool(on))))

    def last_refusal(self):
        """(kind, index) of this instance's last proof: kind 0 = not refused, else REFUSAL_ENCODING / _ONE / _UNSAT / _APP_MASK
        (include/zkhip.h); index: the variable, or the first constraint that fails."""
        kind, index = ctypes.c_int(0), ctypes.c_size_t(0)
        _check(load().zkhip_prover_last_refusal(self.handle, ctypes.byref(kind), ctypes.byref(index)))
        return int(kind.value), int(index.value)

    def last_accumulate_ms(self):
        return float(load().zkhip_prover_last_accumulate_ms(self.handle))

    def last_accumulate_entries(self):
        out = ctypes.c_uint64(0)
        _check(load().zkhip_prover_last_accumulate_entries(self.handle, ctypes.byref(out)))
        return int(out.value)

    def last_table_model(self):
        """1: the G1 MSMs of this instance's last proof accumulated on the Edwards curve, 0: in XYZZ (zkhip_prover_last_table_model)."""
        out = ctypes.c_int(0)
        lib = load()
        lib.zkhip_prover_last_table_model.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        _check(lib.zkhip_prover_last_table_model(self.handle, ctypes.byref(out)))
        return int(out.value)

    def timings(self):
        t = (ctypes.c_double * 8)()
        _check(load().zkhip_prover_timings(self.handle, t))
        out = dict(zip(["upload_z", "qap", "msm_A", "msm_B2", "msm_B1", "msm_H", "msm_L", "host_tail"], list(t)))
        out["chained"] = bool(load().zkhip_prover_timings_chained(self.handle))       # True: upload_z / qap are enqueueing times
        return out

    def free(self):
        if self.handle:
            load().zkhip_prover_free(self.handle)
            self.handle = None


class AggregatorPipeline:
    """Streaming aggregator_circuit::prove (zkhip_aggregator_pipeline_*): submit() returns a ticket at once, wait(ticket)
    returns (primary_inputs, proof).  Witness generation, the GPU prover and the host tail of successive batches overlap."""

    def __init__(self, agg, crs, gpu_slots=2, witness_workers=2, gpu_witness=False, app_cache=True, hybrid=False):
        """app_cache: keep a zkhip_aggregator_app per nested key seen and prove its batches from masked assignments (default; the
        proofs are the same either way).  hybrid (with gpu_witness): two host generators beside the GPU batchers."""
        h = ctypes.c_void_p()
        lib = load()
        lib.zkhip_aggregator_pipeline_new_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p)]
        flags = (1 if gpu_witness else 0) | (0 if app_cache else 2) | (4 if (hybrid and gpu_witness) else 0)
        _check(lib.zkhip_aggregator_pipeline_new_ex(agg.handle, crs.handle, gpu_slots, witness_workers, flags, ctypes.byref(h)))
        self.handle, self._agg, self._crs = h, agg, crs
        self.n_primary = agg.num_primary_inputs()

    def register_app(self, nested_vk):
        """RegisterApplication's part in the prover: the application's constants are computed now (zkhip_aggregator_pipeline_register_app)."""
        vk = np.ascontiguousarray(nested_vk, dtype=np.uint64).reshape(-1)
        lib = load()
        lib.zkhip_aggregator_pipeline_register_app.argtypes = [ctypes.c_void_p, c_u64p_t]
        _check(lib.zkhip_aggregator_pipeline_register_app(self.handle, _p(vk)))

    def app_hits(self):
        lib = load()
        lib.zkhip_aggregator_pipeline_app_hits.restype = ctypes.c_size_t
        lib.zkhip_aggregator_pipeline_app_hits.argtypes = [ctypes.c_void_p]
        return int(lib.zkhip_aggregator_pipeline_app_hits(self.handle))

    def submit(self, nested_vk, nested_proofs, nested_inputs, r, s):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        vk, pr, inp, r, s = c(nested_vk), c(nested_proofs), c(nested_inputs), c(r), c(s)
        k, npf = self._agg.inputs_per_nested_proof, self._agg.num_proofs
        assert vk.size == 60 + 12 * (k + 1) and pr.size == 48 * npf and inp.size == 6 * k * npf and r.size == 6 and s.size == 6
        t = ctypes.c_uint64(0)
        _check(load().zkhip_aggregator_pipeline_submit(self.handle, _p(vk), _p(pr), _p(inp), _p(r), _p(s), ctypes.byref(t)))
        return t.value

    def wait(self, ticket):
        prim = np.zeros((self.n_primary, 6), dtype=np.uint64)
        proof = np.zeros(72, dtype=np.uint64)
        _check(load().zkhip_aggregator_pipeline_wait(self.handle, ticket, _p(prim), _p(proof)))
        return prim, proof

    def free(self):
        if self.handle:
            load().zkhip_aggregator_pipeline_free(self.handle)
            self.handle = None


def _int_list(devices):
    d = [int(x) for x in devices]
    return (ctypes.c_int * len(d))(*d), len(d)


class AggregatorDispatcher:
    """The GPUs of a node behind ONE streaming prover (zkhip_dispatcher_*): a resident copy of the key and a pipeline per entry of
    `devices` (an index may repeat: two contexts on one GPU), every batch goes to the entry with the fewest batches outstanding.
    Same submit / wait as AggregatorPipeline.  keypair: a Keypair (its proving half is uploaded to every entry)."""

    def __init__(self, agg, keypair, devices, opts=None, gpu_slots=32, witness_workers=10, gpu_witness=False, app_cache=True, hybrid=False):
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(keypair.handle, ctypes.byref(d)))
        arr, n = _int_list(devices)
        h = ctypes.c_void_p()
        _check(load().zkhip_dispatcher_new(agg.handle, ctypes.byref(d), ctypes.byref(opts) if opts is not None else None, arr, n,
                                           gpu_slots, witness_workers, (1 if gpu_witness else 0) | (0 if app_cache else 2) | (4 if (hybrid and gpu_witness) else 0),
                                           ctypes.byref(h)))
        self.handle, self._agg, self._kp = h, agg, keypair
        self.n_primary = agg.num_primary_inputs()
        self.size = n

    def submit(self, nested_vk, nested_proofs, nested_inputs, r, s):
        c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        vk, pr, inp, r, s = c(nested_vk), c(nested_proofs), c(nested_inputs), c(r), c(s)
        k, npf = self._agg.inputs_per_nested_proof, self._agg.num_proofs
        assert vk.size == 60 + 12 * (k + 1) and pr.size == 48 * npf and inp.size == 6 * k * npf and r.size == 6 and s.size == 6
        t = ctypes.c_uint64(0)
        _check(load().zkhip_dispatcher_submit(self.handle, _p(vk), _p(pr), _p(inp), _p(r), _p(s), ctypes.byref(t)))
        return t.value

    def wait(self, ticket):
        prim = np.zeros((self.n_primary, 6), dtype=np.uint64)
        proof = np.zeros(72, dtype=np.uint64)
        _check(load().zkhip_dispatcher_wait(self.handle, ticket, _p(prim), _p(proof)))
        return prim, proof

    def register_app(self, nested_vk):
        """RegisterApplication on every entry (zkhip_dispatcher_register_app)."""
        vk = np.ascontiguousarray(nested_vk, dtype=np.uint64).reshape(-1)
        lib = load()
        lib.zkhip_dispatcher_register_app.argtypes = [ctypes.c_void_p, c_u64p_t]
        _check(lib.zkhip_dispatcher_register_app(self.handle, _p(vk)))

    def stats(self):
        """Batches handed to each entry of the device list so far."""
        out = (ctypes.c_size_t * self.size)()
        _check(load().zkhip_dispatcher_stats(self.handle, out))
        return list(out)

    def outstanding(self):
        """Batches each entry still owes a collector (what submit's least-loaded routing looks at)."""
        out = (ctypes.c_size_t * self.size)()
        _check(load().zkhip_dispatcher_outstanding(self.handle, out))
        return list(out)

    def free(self):
        if self.handle:
            load().zkhip_dispatcher_free(self.handle)
            self.handle = None


class MultiProver:
    """One proof over a key partitioned across `devices` (zkhip_multi_prover_*): a slice and a prover instance per entry, host
    threads side by side, partial sums added on the host, one tail.  The proof equals the whole-key proof limb for limb."""

    def __init__(self, keypair, r1cs_desc, devices, opts=None):
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(keypair.handle, ctypes.byref(d)))
        arr, n = _int_list(devices)
        h = ctypes.c_void_p()
        _check(load().zkhip_multi_prover_new(ctypes.byref(d), ctypes.byref(r1cs_desc), ctypes.byref(opts) if opts is not None else None, arr, n, ctypes.byref(h)))
        self.handle, self._kp, self._desc, self.size = h, keypair, r1cs_desc, n

    def prove(self, z, r, s):
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 6)
        r, s = (np.ascontiguousarray(a, dtype=np.uint64).reshape(6) for a in (r, s))
        out = np.zeros(72, dtype=np.uint64)
        _check(load().zkhip_multi_prover_prove(self.handle, _p(z), _p(r), _p(s), _p(out)))
        return out

    def timings(self):
        t = (ctypes.c_double * 3)()
        _check(load().zkhip_multi_prover_timings(self.handle, t))
        return dict(zip(["slowest_slice", "host_additions", "host_tail"], list(t)))

    def free(self):
        if self.handle:
            load().zkhip_multi_prover_free(self.handle)
            self.handle = None


class Keypair:
    """Groth16 keypair from a trusted setup on the GPU (mirror of wsnark::generate_setup / keypair)."""

    def __init__(self, r1cs_desc, tau, alpha, beta, delta, domain=None):
        """domain: None = the forced power of two the reference's generate_setup uses; "step" = libfqfft's unforced choice (an
        option; not a reference deployment's key); an int = that many points."""
        h = ctypes.c_void_p()
        c = lambda a: _p(np.ascontiguousarray(a, dtype=np.uint64))
        lib = load()
        lib.zkhip_groth16_setup_ex.argtypes = [ctypes.POINTER(R1csDesc), c_u64p_t, c_u64p_t, c_u64p_t, c_u64p_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        _check(lib.zkhip_groth16_setup_ex(ctypes.byref(r1cs_desc), c(tau), c(alpha), c(beta), c(delta), _domain_arg(domain), ctypes.byref(h)))
        self.handle = h

    @classmethod
    def setup_slice(cls, r1cs_desc, tau, alpha, beta, delta, parts, part, opts=None, domain=None):
        """zkhip_groth16_setup_slice: this rank's share of a trusted setup -> (keypair WITHOUT queries: vk() and consts() work, Crs slice
        with .ranges).  Only the slice is multiplied out, on the device; nothing of the proving half visits the host."""
        lib = load()
        c = lambda a: _p(np.ascontiguousarray(a, dtype=np.uint64))
        lib.zkhip_groth16_setup_slice.argtypes = [ctypes.POINTER(R1csDesc), c_u64p_t, c_u64p_t, c_u64p_t, c_u64p_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p)]
        hc, hk = ctypes.c_void_p(), ctypes.c_void_p()
        rng = (ctypes.c_size_t * 6)()
        _check(lib.zkhip_groth16_setup_slice(ctypes.byref(r1cs_desc), c(tau), c(alpha), c(beta), c(delta), _domain_arg(domain), int(parts), int(part),
                                             ctypes.byref(opts) if opts is not None else None, ctypes.byref(hc), rng, ctypes.byref(hk)))
        kp = cls.__new__(cls)
        kp.handle = hk
        crs = Crs.__new__(Crs)
        crs.handle = hc
        crs.ranges = ((int(rng[0]), int(rng[1])), (int(rng[2]), int(rng[3])), (int(rng[4]), int(rng[5])))
        return kp, crs

    @property
    def domain_size(self):
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(self.handle, ctypes.byref(d)))
        return int(d.domain_size)

    def write(self, path):
        """Mirror of wsnark::keypair_write_bytes (aggregator_server.cpp:88-94); the library's own container format."""
        _check(load().zkhip_keypair_write(self.handle, str(path).encode()))

    @classmethod
    def read(cls, path):
        """Mirror of wsnark::keypair_read_bytes (aggregator_server.cpp:77-86)."""
        h = ctypes.c_void_p()
        _check(load().zkhip_keypair_read(str(path).encode(), ctypes.byref(h)))
        kp = cls.__new__(cls)
        kp.handle = h
        return kp

    def upload_crs(self, opts=None):
        """opts: key_opts(...) - this key's own table / launch options (None: the process defaults)."""
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(self.handle, ctypes.byref(d)))
        if d.n_vars and not d.a_query:
            raise ZkhipError("this keypair holds no query vectors (Keypair.setup_slice): there is nothing to upload")
        crs = Crs.__new__(Crs)
        h = ctypes.c_void_p()
        _check(load().zkhip_crs_upload_ex(ctypes.byref(d), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h)))
        crs.handle = h
        return crs

    def consts(self):
        """alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2 of the proving key (24 limbs each): what zkhip_groth16_finish takes."""
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(self.handle, ctypes.byref(d)))
        return {k: np.ctypeslib.as_array(ctypes.cast(getattr(d, k), c_u64p_t), (24,)).copy()
                for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2")}

    def pk_arrays(self):
        """Host copies of the proving half (dict in the layout Crs / the test oracle take) plus n_vars, n_primary, domain_size."""
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(self.handle, ctypes.byref(d)))
        m, l, dom = d.n_vars, d.n_primary, d.domain_size
        if m and not d.a_query:
            raise ZkhipError("this keypair holds no query vectors (Keypair.setup_slice: the slice lives on the device; vk() and consts() are what it keeps)")
        arr = lambda ptr, n: (np.ctypeslib.as_array(ctypes.cast(ptr, c_u64p_t), (n, 24)).copy() if n else np.zeros((0, 24), dtype=np.uint64))
        pk = {k: arr(getattr(d, k), 1).reshape(24) for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2")}
        pk.update(A=arr(d.a_query, m), B2=arr(d.b_g2_query, m), B1=arr(d.b_g1_query, m), H=arr(d.h_query, dom - 1), L=arr(d.l_query, m - l - 1))
        return pk, m, l, dom

    def vk(self):
        a, b, dl = (np.zeros(24, dtype=np.uint64) for _ in range(3))
        abc = c_u64p_t()
        n = load().zkhip_keypair_vk(self.handle, _p(a), _p(b), _p(dl), ctypes.byref(abc))
        return dict(alpha=a, beta=b, delta=dl, ABC=np.ctypeslib.as_array(abc, (n, 24)).copy())

    def contribute(self, s=None, k=None, prev_digest=b"\0" * 32, host=False):
        """zkhip_keypair_contribute / _host (host=True: no device): one phase-2 contribution on top of this key ->
        (the new Keypair, its Contribution record, the new transcript digest).  delta is multiplied by the secret s, every point of H
        and L by s^-1; tau, alpha and beta stay whoever's they were (include/zkhip.h states the scope).  s, k: six Montgomery limbs
        each, for tests; None draws them from the OS, and nobody ever sees them."""
        lib = load()
        if len(prev_digest) != 32:
            raise ZkhipError("prev_digest is 32 bytes", -1)
        c = lambda a: _p(np.ascontiguousarray(a, dtype=np.uint64)) if a is not None else None
        h, rec, digest = ctypes.c_void_p(), Contribution(), ctypes.create_string_buffer(32)
        _check((lib.zkhip_keypair_contribute_host if host else lib.zkhip_keypair_contribute)(self.handle, c(s), c(k), bytes(prev_digest), ctypes.byref(h),
                                                                                           ctypes.byref(rec), digest))
        kp = Keypair.__new__(Keypair)
        kp.handle = h
        return kp, rec, digest.raw

    def free(self):
        if self.handle:
            load().zkhip_keypair_free(self.handle)
            self.handle = None


def make_crs_desc(pk, n_vars, n_primary, domain_size):
    """zkhip_crs_desc over a key's arrays (the dict Crs takes).  Returns (desc, keep): `keep` holds the arrays the descriptor points
    into and must stay alive while the descriptor is used."""
    d = CrsDesc()
    d.n_vars, d.n_primary, d.domain_size = n_vars, n_primary, domain_size
    keep = []
    for field, key in (("alpha_g1", "alpha_g1"), ("beta_g1", "beta_g1"), ("beta_g2", "beta_g2"), ("delta_g1", "delta_g1"), ("delta_g2", "delta_g2"),
                       ("a_query", "A"), ("b_g2_query", "B2"), ("b_g1_query", "B1"), ("h_query", "H"), ("l_query", "L")):
        a = np.ascontiguousarray(pk[key], dtype=np.uint64).reshape(-1, 24)
        keep.append(a)
        setattr(d, field, a.ctypes.data if a.size else None)
    return d, keep


def check_key(key, vk_abc=None, r1cs=None, rho=None, host=False):
    """zkhip_crs_check / zkhip_crs_check_host (host=True: no device): validate a proving key BEFORE it is uploaded -> KeyReport.
    key: a Keypair (its own ABC is checked as vk_abc unless one is given), a CrsDesc, or (pk dict, n_vars, n_primary, domain_size) as
    Crs takes them.  vk_abc: (n_primary + 1) x 24 limbs or None.  r1cs: an R1csDesc, or the (desc, keep) of make_r1cs_desc, for the
    structure check; None: no structure check.  rho: n_vars 128-bit scalars (ints, or n_vars x 2 words) for tests and reproducible
    runs; None: drawn from the OS."""
    lib = load()
    keep = None
    if isinstance(key, Keypair):
        d = CrsDesc()
        _check(lib.zkhip_keypair_crs_desc(key.handle, ctypes.byref(d)))
        if d.n_vars and not d.a_query:
            raise ZkhipError("this keypair holds no query vectors (Keypair.setup_slice): there is nothing to check")
        if vk_abc is None:
            vk_abc = key.vk()["ABC"]
    elif isinstance(key, CrsDesc):
        d = key
    else:
        d, keep = make_crs_desc(*key)
    abc = None
    if vk_abc is not None:
        abc = np.ascontiguousarray(vk_abc, dtype=np.uint64).reshape(-1, 24)
        if abc.shape[0] != d.n_primary + 1:
            raise ZkhipError("vk_abc must hold n_primary + 1 points", -1)
    cs = r1cs[0] if isinstance(r1cs, tuple) else r1cs
    rl = _rho_limbs(rho, d.n_vars) if rho is not None else None
    rep = KeyReport()
    _check((lib.zkhip_crs_check_host if host else lib.zkhip_crs_check)(ctypes.byref(d), _p(abc) if abc is not None else None,
                                                                       ctypes.byref(cs) if cs is not None else None,
                                                                       _p(rl) if rl is not None else None, ctypes.byref(rep)))
    del keep
    return rep


def key_check_set_chunk(points):
    """Test hook: points per launch of the key check's point kernel (0: the library's rule)."""
    _check(load().zkhip_internal_key_check_set_chunk(int(points)))


def key_check_last_ms():
    """Of this thread's last check_key: longest single point-check launch (device time), all point checks, the B relation's two sums,
    the host's pairings (wall time), then the point checks of each of the eleven elements, milliseconds."""
    out = (ctypes.c_double * (4 + len(KEY_ELEMENTS)))()
    _check(load().zkhip_internal_key_check_last_ms(out))
    return [float(v) for v in out]


def _key_desc(key):
    """A Keypair, a CrsDesc or (pk dict, n_vars, n_primary, domain_size) -> (CrsDesc, what must stay alive beside it)."""
    if isinstance(key, Keypair):
        d = CrsDesc()
        _check(load().zkhip_keypair_crs_desc(key.handle, ctypes.byref(d)))
        if d.n_vars and not d.a_query:
            raise ZkhipError("this keypair holds no query vectors (Keypair.setup_slice): there is nothing to check")
        return d, key
    if isinstance(key, CrsDesc):
        return key, None
    return make_crs_desc(*key)


def phase2_verify(before, after, contribution, prev_digest, rho=None, host=False):
    """zkhip_phase2_verify / _host (host=True: no device): is `after` an honest phase-2 contribution on top of `before`? ->
    (Phase2Report, the new transcript digest or None when the report is not ok).  before, after: as check_key takes a key; `before`
    must have been validated already (check_key, or an earlier accepted contribution).  rho: (domain_size - 1) + (n_vars -
    n_primary - 1) 128-bit scalars for tests and reproducible runs; None: drawn from the OS."""
    lib = load()
    if len(prev_digest) != 32:
        raise ZkhipError("prev_digest is 32 bytes", -1)
    db, keep_b = _key_desc(before)
    da, keep_a = _key_desc(after)
    rl = _rho_limbs(rho, (db.domain_size - 1) + (db.n_vars - db.n_primary - 1)) if rho is not None else None
    rep, digest = Phase2Report(), ctypes.create_string_buffer(32)
    _check((lib.zkhip_phase2_verify_host if host else lib.zkhip_phase2_verify)(ctypes.byref(db), ctypes.byref(da), ctypes.byref(contribution),
                                                                             bytes(prev_digest), _p(rl) if rl is not None else None,
                                                                             ctypes.byref(rep), digest))
    del keep_b, keep_a
    return rep, (digest.raw if rep.ok else None)


def phase2_set_form(form):
    """Test / measurement hook: the kernel form of contribute's device route - 0 the default (endomorphism), 1 the baseline (only in a
    build with both forms: ZkhipError otherwise), 2 the endomorphism form."""
    _check(load().zkhip_internal_phase2_set_form(int(form)))


def phase2_last_ms():
    """Of this thread's last contribute / phase2_verify, milliseconds (zkhip_internal_phase2_last_ms): [0] the device time of its
    longest single launch (contribute: the multiplication kernel, verify: the point check; 0 on the host routes), [3] the whole call.
    contribute: [1] / [2] h_query / l_query (wall time, staging included), [4] the copy of the key, [5] delta' in both groups,
    [6] commitment, response and hashes, [7] the device time of ALL launches of the multiplication kernel.
    verify: [1] the byte comparison of the unchanged elements, [2] the infinity patterns, [4] point checks, [5] the four sums,
    [6] the host relations."""
    out = (ctypes.c_double * 8)()
    _check(load().zkhip_internal_phase2_last_ms(out))
    return [float(v) for v in out]


def r1cs_desc_from_aggregator(agg):
    d = R1csDesc()
    _check(load().zkhip_aggregator_get_r1cs(agg.handle, ctypes.byref(d)))
    return d


def r1cs_from_desc(desc, domain=None):
    """Upload a constraint system described by a zkhip_r1cs_desc (e.g. the aggregator circuit's).  domain: as R1cs."""
    r = R1cs.__new__(R1cs)
    h = ctypes.c_void_p()
    _check(load().zkhip_r1cs_upload_ex(ctypes.byref(desc), _domain_arg(domain), ctypes.byref(h)))
    r.handle, r._keep = h, []
    r.n_vars, r.n_primary, r.n_constraints = desc.n_vars, desc.n_primary, desc.n_constraints
    return r


def aggregator_vk_hash(nested_vk, inputs_per_nested_proof=1):
    vk = np.ascontiguousarray(nested_vk, dtype=np.uint64).reshape(-1)
    out = np.zeros(6, dtype=np.uint64)
    _check(load().zkhip_aggregator_vk_hash(_p(vk), inputs_per_nested_proof, _p(out)))
    return out


def domain_size(min_size):
    """Points of the reference's evaluation domain for min_size points: the forced power of two (host code)."""
    return int(load().zkhip_domain_size(min_size))


def step_domain_size(min_size):
    """Points of the domain libfqfft picks for min_size points when not forced: 2^k, or 2^k + 2^r (host code)."""
    return int(load().zkhip_step_domain_size(min_size))


def domain_is_valid(d):
    return bool(load().zkhip_domain_is_valid(d))


def last_prove_timings():
    t = (ctypes.c_double * 8)()
    _check(load().zkhip_last_prove_timings(t))
    return dict(zip(["upload_z", "qap", "msm_A", "msm_B2", "msm_B1", "msm_H", "msm_L", "host_tail"], list(t)))


def set_prove_split(mode):
    """0: a proof's five MSMs in one launch sequence (default); 1 / 2: the four MSMs over z beside the QAP map, H behind it (gated / not)"""
    _check(load().zkhip_set_prove_split(int(mode)))


def last_prove_split():
    """True: this thread's last plain proof ran as two launch sequences (the four MSMs over z beside the QAP map, H behind it)"""
    return bool(load().zkhip_last_prove_split())


def last_prove_table_model():
    """1: the G1 MSMs of the last proof of the plain entry points accumulated on the Edwards curve (zkhip_last_prove_table_model)."""
    return int(load().zkhip_last_prove_table_model())


def jac_to_affine(jac):
    j = np.ascontiguousarray(jac, dtype=np.uint64)
    out = np.zeros(24, dtype=np.uint64)
    _check(load().zkhip_jac_to_affine(_p(j), _p(out)))
    return out


def jac_add(a, b):
    out = np.zeros(36, dtype=np.uint64)
    _check(load().zkhip_jac_add(_p(np.ascontiguousarray(a, dtype=np.uint64)), _p(np.ascontiguousarray(b, dtype=np.uint64)), _p(out)))
    return out


def last_accumulate_ms():
    return float(load().zkhip_last_accumulate_ms())


def last_accumulate_entries():
    """Mixed additions of the k_accumulate launch zkhip_last_accumulate_ms timed (the non-zero digits it sorted)."""
    out = ctypes.c_uint64(0)
    _check(load().zkhip_last_accumulate_entries(ctypes.byref(out)))
    return int(out.value)


def set_lockstep(mode, min_buckets=-1):
    """Test / A-B knob of the Edwards accumulation's lockstep route (zkhip_internal_set_lockstep): mode 0 sliced, 1 the device decides,
    -1 the environment (ZKHIP_LOCKSTEP); min_buckets: non-empty buckets a launch needs for it (-1: the chip's own figure)."""
    _check(load().zkhip_internal_set_lockstep(int(mode), int(min_buckets)))


def set_msm_stream_layout(layout):
    """Test / A-B knob (zkhip_internal_set_msm_stream_layout): how the MsmStreams made from now on place their HIP streams: 0 a pair
    per context at its first submit, 1 all primaries then all secondaries up front, 2 primaries only; -1 the environment / default."""
    _check(load().zkhip_internal_set_msm_stream_layout(int(layout)))


def last_acc_path():
    """The route the last single MSM's accumulation took, read back from the device: 1 lockstep, 0 sliced, -1 not an Edwards launch."""
    out = ctypes.c_int(-1)
    _check(load().zkhip_internal_last_acc_path(ctypes.byref(out)))
    return int(out.value)


def msm_multi(sets, scalars, model, montgomery=False):
    """Test hook zkhip_internal_msm_multi: len(sets) <= 4 table-backed Bases of one window, job k over the first len(scalars[k]) bases of
    sets[k], through ONE launch sequence.  model 0 XYZZ, 1 Edwards.  Returns (K x 36 Jacobian limbs, acc_path)."""
    K = len(sets)
    sc = [np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 6) for s in scalars]
    assert len(sc) == K
    hs = (ctypes.c_void_p * K)(*[b.handle for b in sets])
    ps = (ctypes.c_void_p * K)(*[s.ctypes.data if s.size else None for s in sc])
    ns = (ctypes.c_size_t * K)(*[s.shape[0] for s in sc])
    out = np.zeros((K, 36), dtype=np.uint64)
    path = ctypes.c_int(-2)
    lib = load()
    lib.zkhip_internal_msm_multi.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), c_u64p_t]
    _check(lib.zkhip_internal_msm_multi(hs, ps, ns, K, int(montgomery), int(model), ctypes.byref(path), _p(out)))
    return out, int(path.value)


def msm_tail(items_affine, W, lo_bits, edw=False, total=False):
    """Test hook: the tail of the bucket reduction alone (zkhip_internal_msm_tail).  items_affine: uint64 [2W][N][24], the W hi groups
    first (all-zero = infinity); returns uint64 [W or 2W][36] Jacobian points: 2^lo_bits sum (i+1) hi[i] + sum (i+1) lo[i] per window,
    then, with total, the plain sums of the lo groups.  edw: the Edwards kernels - every output is TWICE that sum."""
    x = np.ascontiguousarray(items_affine, dtype=np.uint64).reshape(2 * W, -1, 24)
    out = np.zeros((W * (2 if total else 1), 36), dtype=np.uint64)
    lib = load()
    lib.zkhip_internal_msm_tail.argtypes = [ctypes.c_int, c_u64p_t, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, c_u64p_t]
    _check(lib.zkhip_internal_msm_tail(int(edw), _p(x), int(W), x.shape[1], int(lo_bits), int(total), _p(out)))
    return out


def field_selftest(field, limbs_in):
    """Test hook: the device's multiplier bodies on raw limbs.  field 0 = Fq (27 limbs), 1 = Fr (14); limbs_in: uint32 [n][4][NL] =
    cases of (a, b, c, d); returns uint32 [n][3][NL] = (a b / R, a^2 / R, (a b + c d) / R)."""
    nl = 27 if field == 0 else 14
    x = np.ascontiguousarray(limbs_in, dtype=np.uint32).reshape(-1, 4, nl)
    out = np.zeros((x.shape[0], 3, nl), dtype=np.uint32)
    lib = load()
    lib.zkhip_internal_field_selftest.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _check(lib.zkhip_internal_field_selftest(int(field), x.ctypes.data, x.shape[0], out.ctypes.data))
    return out


def field_ops_selftest(field, op, operands):
    """Test hook: one function of the device's field layer on raw limbs (zkhip_internal_field_ops_selftest; the op codes are listed in
    include/zkhip.h).  field 0 = Fq (27 limbs), 1 = Fr (14); operands: uint32 [n][3][NL] = cases of (a, b, c), one GPU lane per case in
    order; returns uint32 [n][NL + 1]: the result and a flag word."""
    nl = 27 if field == 0 else 14
    x = np.ascontiguousarray(operands, dtype=np.uint32).reshape(-1, 3, nl)
    out = np.zeros((x.shape[0], nl + 1), dtype=np.uint32)
    lib = load()
    lib.zkhip_internal_field_ops_selftest.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _check(lib.zkhip_internal_field_ops_selftest(int(field), int(op), x.ctypes.data, x.shape[0], out.ctypes.data))
    return out


def point_ops_selftest(op, mem, rows, table=None):
    """Test hook: one function of the device's point layer on raw limbs (zkhip_internal_point_ops_selftest; the op codes and the row
    layouts are listed in include/zkhip.h).  rows: uint32 [n][224], one case per GPU lane (four lanes for the quad forms) in order;
    mem 0 / 1: limb-major / slot references; table: uint32 [m][72] precomputed Edwards points for the lockstep run.  Returns uint32
    [n][217]: the accumulator, a flag word, and B afterwards."""
    x = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 224)
    out = np.zeros((x.shape[0], 217), dtype=np.uint32)
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint32).reshape(-1, 72)
    lib = load()
    lib.zkhip_internal_point_ops_selftest.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                      ctypes.c_void_p]
    _check(lib.zkhip_internal_point_ops_selftest(int(op), int(mem), x.ctypes.data, x.shape[0], None if tab is None else tab.ctypes.data,
                                                 0 if tab is None else tab.shape[0], out.ctypes.data))
    return out


def witness_run_program(prog, inputs, wpg=4, segment=2048, waves=1):
    """Test hook: a caller's program through the GPU witness generator's own upload, launch and kernels
    (zkhip_internal_witness_run_program).  prog: dict with code u8 [n], a / b i32 [n], level_start u32 [levels + 1], chain_start,
    out_ref i32 [n_vars], consts u64 [c, 6] (ABI form), n_inputs; inputs: u64 [batches, n_inputs, 6] (ABI form).  The library
    validates the program first and raises ZkhipError (code -1) for one that breaks a structural rule; zero batches validates only
    and needs no device.  waves: waves per witness (1: k_witness, through the hook without the argument; 2, 4, 8, 16: k_witness_wide,
    whole levels per launch; 0: auto).  Returns (assignments u64 [batches, n_vars, 6], flags u32 [batches])."""
    arrs = dict(code=np.ascontiguousarray(prog["code"], dtype=np.uint8), a=np.ascontiguousarray(prog["a"], dtype=np.int32), b=np.ascontiguousarray(prog["b"], dtype=np.int32),
                level_start=np.ascontiguousarray(prog["level_start"], dtype=np.uint32), out_ref=np.ascontiguousarray(prog["out_ref"], dtype=np.int32),
                consts=np.ascontiguousarray(prog["consts"], dtype=np.uint64).reshape(-1, 6))
    n = arrs["code"].size
    assert arrs["a"].size == n and arrs["b"].size == n and arrs["level_start"].size >= 1
    x = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, int(prog["n_inputs"]), 6) if int(prog["n_inputs"]) else np.zeros((len(inputs), 0, 6), dtype=np.uint64)
    ptr = lambda k: arrs[k].ctypes.data if arrs[k].size else None
    wp = WitnessProgram(ptr("code"), ptr("a"), ptr("b"), n, arrs["level_start"].ctypes.data, arrs["level_start"].size - 1, int(prog["chain_start"]),
                        ptr("out_ref"), arrs["out_ref"].size, ptr("consts"), arrs["consts"].shape[0], int(prog["n_inputs"]))
    batches = x.shape[0]
    z = np.zeros((batches, arrs["out_ref"].size, 6), dtype=np.uint64)
    flags = np.zeros(max(batches, 1), dtype=np.uint32)
    lib = load()
    if waves == 1:
        lib.zkhip_internal_witness_run_program.argtypes = [ctypes.POINTER(WitnessProgram), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
        _check(lib.zkhip_internal_witness_run_program(ctypes.byref(wp), x.ctypes.data if x.size else None, batches, int(wpg), int(segment), z.ctypes.data if z.size else None,
                                                      flags.ctypes.data))
    else:
        lib.zkhip_internal_witness_run_program_wide.argtypes = [ctypes.POINTER(WitnessProgram), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_int,
                                                                ctypes.c_void_p, ctypes.c_void_p]
        _check(lib.zkhip_internal_witness_run_program_wide(ctypes.byref(wp), x.ctypes.data if x.size else None, batches, int(wpg), int(segment), int(waves),
                                                           z.ctypes.data if z.size else None, flags.ctypes.data))
    return z, flags[:batches]


def measure_fq_mul_rate():
    """Fq multiplications per second of the device, measured now (dependent fp_mul chains, two waves per SIMD)."""
    v = ctypes.c_double(0)
    _check(load().zkhip_measure_fq_mul_rate(ctypes.byref(v)))
    return float(v.value)


def measure_ntt(log_d, inverse=False, coset=False, batch=1, reps=10):
    """ms per size-2^log_d transform, the pass kernels alone (zkhip_measure_ntt: HIP events on the passes' stream)."""
    out = ctypes.c_double(0)
    lib = load()
    lib.zkhip_measure_ntt.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    _check(lib.zkhip_measure_ntt(log_d, int(inverse), int(coset), batch, reps, ctypes.byref(out)))
    return out.value


def ntt_packed(data, log_d, inverse=False, coset=False, in_transposed=False):
    """Test hook: the engine's batched transform on 1 .. 3 vectors in device LOCATION order (zkhip_internal_ntt_packed; the hook
    permutes nothing: natural order on one side of a transform of 2^12 elements or more, transposed order on the other).
    data: uint64 [nbuf, 2^log_d, 6] = ABI limbs (form 0), or uint32 [nbuf, 2^log_d, 12] = the packed device words (form 1).
    Returns a new array of the same shape and type."""
    a = np.asarray(data)
    assert a.dtype in (np.uint64, np.uint32) and a.ndim == 3 and a.shape[1:] == (1 << log_d, 6 if a.dtype == np.uint64 else 12), (a.dtype, a.shape)
    out = np.ascontiguousarray(a).copy()
    lib = load()
    lib.zkhip_internal_ntt_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    _check(lib.zkhip_internal_ntt_packed(out.ctypes.data, 0 if a.dtype == np.uint64 else 1, a.shape[0], int(log_d), int(inverse), int(coset), int(in_transposed)))
    return out


def ntt_set_one_each_max(log_d_max):
    """Test / measurement knob (zkhip_internal_ntt_set_one_each_max): transforms above 2^log_d_max run the wide tiles; -1: the
    environment (ZKHIP_NTT_ONE_EACH_MAX) or the default 22.  Process-wide; results do not depend on it."""
    _check(load().zkhip_internal_ntt_set_one_each_max(int(log_d_max)))


def reset_time_base():
    """Record the origin of the accumulate intervals again (float milliseconds lose resolution far from their origin)."""
    _check(load().zkhip_reset_time_base())


def last_accumulate_interval():
    """(begin, end) of the last collected MSM's accumulation launch, ms on the device's time base."""
    t = (ctypes.c_float * 2)()
    _check(load().zkhip_last_accumulate_interval(t))
    return float(t[0]), float(t[1])
