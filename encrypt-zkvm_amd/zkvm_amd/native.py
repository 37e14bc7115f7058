"""ctypes binding of libzkvm_gpu.so (include/zkvm_gpu.h).

The product path: every prove goes through this library's HIP kernels.  There is no CPU
fallback -- if the library is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent.parent
# ZKVM_GPU_LIB selects an alternative in-tree build (A/B experiments); default lib/libzkvm_gpu.so
LIB_PATH = Path(os.environ.get("ZKVM_GPU_LIB", PKG_ROOT / "lib" / "libzkvm_gpu.so"))

ZK_OK = 0
ZK_ERR_INVALID_ARG = -1
ZK_ERR_BUFFER_TOO_SMALL = -2
ZK_ERR_DEVICE = -3
ZK_ERR_OUT_OF_MEMORY = -4
ZK_ERR_PEER = -5
ZK_ERR_PENDING = -6
ZK_ERR_CANCELLED = -7
ZK_ERR_PROGRAM = -10
ZK_ERR_STACK = -11
ZK_ERR_CHIPLETS = -12
ZK_ERR_DEGREE = -20
ZK_ERR_TRACE = -21
ZK_ERR_DEGREES = -22
ZK_ERR_VERIFY = -30

MAX_COLS, MAX_TCONS, MAX_ASSERTS, MAX_CCOLS, MAX_FRI, MAX_REM, MAX_Q = 32, 32, 32, 16, 16, 256, 255

# every symbol include/zkvm_gpu.h declares (checked by tests/test_native_abi.py)
EXPORTED = (
    "zk_last_error", "zk_device_count", "zk_runtime_versions", "zk_device_pci_bus_id", "zk_device_synchronize",
    "zk_prover_create", "zk_prover_create_shard", "zk_prover_destroy",
    "zk_prover_acquire", "zk_prover_release", "zk_prover_pool_trim", "zk_prover_trace_buffer",
    "zk_prove", "zk_prove_columns", "zk_prove_columns_ex", "zk_host_alloc", "zk_host_free", "zk_host_register",
    "zk_host_unregister", "zk_prove_device", "zk_lde_new", "zk_lde_read_frame", "zk_lde_query", "zk_lde_free",
    "zk_eval_constraints", "zk_commit_composition", "zk_comp_query", "zk_comp_free", "zk_prover_stage_times", "zk_prover_profile", "zk_prover_kernel_stats", "zk_prover_kernel_ops", "zk_prover_exchange_stats", "zk_prover_exchange_stats_ex", "zk_prover_shard_schedule", "zk_prover_upload_stats", "zk_prover_upload_derived", "zk_prover_upload_fixed", "zk_prover_coeff_sources", "zk_prover_set_upload_schedule", "zk_prover_proof_info", "zk_vm_trace",
    "zk_verify", "zk_comm_create_loopback", "zk_comm_unique_id", "zk_comm_create_rccl", "zk_comm_create_host", "zk_comm_destroy", "zk_comm_set_measure", "zk_comm_set_trace_split", "zk_prove_sharded",
    "zk_program_compile", "zk_program_trace", "zk_program_free", "zk_vm_last_error", "zk_vm_trace_device",
    "zk_vm_prove",
    "zk_vm_prove_sharded",
    "zk_validate_device", "zk_validate_columns", "zk_prover_set_validate", "zk_prover_validation",
    "zk_degrees_device", "zk_degrees_columns", "zk_prover_set_validate_degrees", "zk_prover_degrees",
    "zk_lde_new_columns", "zk_eval_constraints_ext", "zk_commit_composition_ext",
    "zk_lde_read_rows", "zk_comp_read_rows",
    "zk_comm_agreement",
    "zk_degrees_sharded",
    "zk_queue_create", "zk_queue_destroy", "zk_queue_set_validate", "zk_queue_set_validate_degrees", "zk_queue_pause",
    "zk_queue_resume", "zk_queue_submit_columns", "zk_queue_submit_device", "zk_queue_submit_vm", "zk_queue_wait",
    "zk_queue_poll", "zk_queue_wait_any", "zk_queue_cancel", "zk_queue_job_validation", "zk_queue_job_degrees",
    "zk_queue_stats",
)


# zk_exchange_fn (include/zkvm_gpu.h): int fn(void *ctx, int op, const void *send, void *recv, size_t bytes)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
XCHG_ALL_TO_ALL, XCHG_ALL_GATHER = 0, 1


class ZkError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code


class Options(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in
                ("num_queries", "blowup", "grinding", "field_extension", "fri_folding", "fri_rem_max_deg")]


class PubInputs(C.Structure):
    _fields_ = [("program_hash", C.c_uint8 * 32), ("stack_outputs", C.c_uint8 * 256),
                ("lwe_size", C.c_uint32), ("delta", C.c_uint32)]


class ProofInfo(C.Structure):
    """zk_proof_info (include/zkvm_gpu.h): what the last proof on a prover did."""
    _fields_ = [("schedule", C.c_int32), ("hint_redos", C.c_uint32), ("hint_sets", C.c_uint32),
                ("hinted_sparse", C.c_uint32), ("derived", C.c_uint32), ("fixed_sets", C.c_uint32)]


class JobResult(C.Structure):
    """zk_job_result (include/zkvm_gpu.h): what a proof queue delivers for one job."""
    _fields_ = [("status", C.c_int32), ("prover", C.c_int32), ("proof_len", C.c_uint64),
                ("queued_ms", C.c_float), ("run_ms", C.c_float), ("running_at_start", C.c_uint32), ("_pad", C.c_uint32),
                ("info", ProofInfo), ("message", C.c_char * 512)]

    def to_dict(self) -> dict:
        d = {f: getattr(self, f) for f in ("status", "prover", "proof_len", "queued_ms", "run_ms", "running_at_start")}
        d["info"] = {f: getattr(self.info, f) for f, _ in ProofInfo._fields_}
        d["message"] = self.message.decode(errors="replace")
        return d


class Validation(C.Structure):
    """zk_validation (include/zkvm_gpu.h): the report of one trace validation (Trace::validate of winterfell 0.9)."""
    _fields_ = [
        ("trace_len", C.c_uint64), ("steps_checked", C.c_uint64), ("failing_steps", C.c_uint64),
        ("t_count", C.c_uint64 * MAX_TCONS), ("t_first", C.c_uint64 * MAX_TCONS),
        ("t_value", C.c_uint8 * (16 * MAX_TCONS)),
        ("a_failed", C.c_uint32), ("a_mask", C.c_uint32),
        ("a_col", C.c_uint32 * MAX_ASSERTS), ("a_step", C.c_uint64 * MAX_ASSERTS),
        ("a_expected", C.c_uint8 * (16 * MAX_ASSERTS)), ("a_found", C.c_uint8 * (16 * MAX_ASSERTS)),
        ("first_kind", C.c_int32), ("first_index", C.c_int32), ("first_step", C.c_uint64),
    ]

    NUM_TCONS, NUM_ASSERTS = 20, 22  # ProcessorAir: evaluate_transition's results, get_assertions' entries

    def to_dict(self) -> dict:
        """The report as plain ints (field elements as Python ints), the arrays cut to the AIR's 20 constraints
        and 22 assertions."""
        t, a = self.NUM_TCONS, self.NUM_ASSERTS
        el = lambda b, k: int.from_bytes(bytes(b[16 * k:16 * k + 16]), "little")  # noqa: E731
        return {
            "trace_len": self.trace_len, "steps_checked": self.steps_checked, "failing_steps": self.failing_steps,
            "t_count": list(self.t_count[:t]), "t_first": list(self.t_first[:t]),
            "t_value": [el(self.t_value, k) for k in range(t)],
            "a_failed": self.a_failed, "a_mask": self.a_mask,
            "a_col": list(self.a_col[:a]), "a_step": list(self.a_step[:a]),
            "a_expected": [el(self.a_expected, k) for k in range(a)],
            "a_found": [el(self.a_found, k) for k in range(a)],
            "first_kind": self.first_kind, "first_index": self.first_index, "first_step": self.first_step,
        }


class Agreement(C.Structure):
    """zk_agreement (include/zkvm_gpu.h): what the ranks of the last sharded call agreed on."""
    _fields_ = [
        ("code", C.c_int32), ("rank_a", C.c_int32), ("rank_b", C.c_int32),
        ("detect", C.c_int32), ("clock", C.c_int32), ("hints", C.c_int32), ("hints_equal", C.c_int32),
        ("validate", C.c_int32), ("world", C.c_uint32), ("_pad", C.c_uint32),
        ("control_calls", C.c_uint64), ("control_bytes", C.c_uint64), ("field", C.c_char * 32),
        ("validate_degrees", C.c_int32), ("_pad2", C.c_int32),
    ]

    def to_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if not f.startswith("_pad")}
        d["field"] = self.field.decode()
        return d


# The control record and the partial reports of csrc/shard_agree.hpp (AgreeRecord: 256 bytes, ValPartial: 1160,
# DegPartial: 312), for the test entry points bound in zkvm_amd/shard_diag.py
AGREE_VERSION, AGREE_MSG = 1, 120
SRC_HOST, SRC_DEVICE, SRC_FIXED = 0, 1, 2
ASSERT_ROW0, ASSERT_LAST = 0x155557, 0x2AAAA8


class AgreeRecord(C.Structure):
    _fields_ = [
        ("version", C.c_uint32), ("world", C.c_uint32), ("rank", C.c_uint32), ("status", C.c_int32),
        ("n", C.c_uint64), ("opt", C.c_uint32 * 6), ("pub_hash", C.c_uint8 * 32),
        ("source", C.c_uint32), ("split_rep", C.c_int32), ("measure", C.c_uint32), ("validate", C.c_uint32),
        ("detect", C.c_uint32),
        ("hint_fresh", C.c_uint32), ("hint_S", C.c_uint32), ("hint_clk", C.c_uint32), ("hint_N8", C.c_uint32),
        ("hint_N32", C.c_uint32),
        ("msg", C.c_char * AGREE_MSG), ("validate_degrees", C.c_uint32), ("reserved", C.c_uint8 * 12),
    ]


class ValPartial(C.Structure):
    _fields_ = [
        ("version", C.c_uint32), ("rank", C.c_uint32), ("status", C.c_int32), ("amask", C.c_uint32),
        ("first", C.c_uint64), ("count", C.c_uint64), ("failing_steps", C.c_uint64),
        ("t_count", C.c_uint64 * 20), ("t_first", C.c_uint64 * 20), ("t_value", C.c_uint8 * (16 * 20)),
        ("a_mask", C.c_uint32), ("_pad", C.c_uint32), ("a_found", C.c_uint8 * (16 * 22)),
        ("msg", C.c_char * AGREE_MSG),
    ]


class DegPartial(C.Structure):
    """One rank's partial report of a sharded degree check: top[k] is the highest GLOBAL coefficient index k1 + n k2 of
    Q_k that is non-zero in the rank's k1 range [first, first + count), bit k of nonzero that there is one."""
    _fields_ = [
        ("version", C.c_uint32), ("rank", C.c_uint32), ("status", C.c_int32), ("nonzero", C.c_uint32),
        ("first", C.c_uint64), ("count", C.c_uint64), ("top", C.c_uint64 * 20),
        ("msg", C.c_char * AGREE_MSG),
    ]


assert C.sizeof(AgreeRecord) == 256 and C.sizeof(ValPartial) == 1160 and C.sizeof(DegPartial) == 312


class Degrees(C.Structure):
    """zk_degrees (include/zkvm_gpu.h): the report of one transition-constraint degree check
    (validate_transition_degrees of winterfell 0.9)."""
    _fields_ = [
        ("trace_len", C.c_uint64), ("ce_len", C.c_uint64),
        ("expected", C.c_uint64 * MAX_TCONS), ("actual", C.c_uint64 * MAX_TCONS),
        ("mismatch_mask", C.c_uint32), ("zero_mask", C.c_uint32), ("over_mask", C.c_uint32), ("_pad", C.c_uint32),
        ("max_actual", C.c_uint64), ("ce_len_needed", C.c_uint64),
    ]

    NUM_TCONS = 20  # ProcessorAir: evaluate_transition's results

    def to_dict(self) -> dict:
        """The report as plain ints, the arrays cut to the AIR's 20 constraints."""
        t = self.NUM_TCONS
        return {
            "trace_len": self.trace_len, "ce_len": self.ce_len,
            "expected": list(self.expected[:t]), "actual": list(self.actual[:t]),
            "mismatch_mask": self.mismatch_mask, "zero_mask": self.zero_mask, "over_mask": self.over_mask,
            "max_actual": self.max_actual, "ce_len_needed": self.ce_len_needed,
        }


class Record(C.Structure):
    _fields_ = [
        ("trace_len", C.c_uint32), ("lde_len", C.c_uint32), ("width", C.c_uint32), ("num_ccols", C.c_uint32),
        ("num_fri_layers", C.c_uint32), ("remainder_len", C.c_uint32), ("num_positions", C.c_uint32),
        ("_pad", C.c_uint32),
        ("trace_root", C.c_uint8 * 32),
        ("coeff_t", C.c_uint8 * (16 * MAX_TCONS)), ("coeff_b", C.c_uint8 * (16 * MAX_ASSERTS)),
        ("constraint_root", C.c_uint8 * 32), ("z", C.c_uint8 * 16),
        ("ood_trace_z", C.c_uint8 * (16 * MAX_COLS)), ("ood_trace_zg", C.c_uint8 * (16 * MAX_COLS)),
        ("ood_constraints", C.c_uint8 * (16 * MAX_CCOLS)),
        ("deep_t", C.c_uint8 * (16 * MAX_COLS)), ("deep_c", C.c_uint8 * (16 * MAX_CCOLS)),
        ("fri_roots", C.c_uint8 * (32 * MAX_FRI)), ("fri_alphas", C.c_uint8 * (16 * MAX_FRI)),
        ("remainder", C.c_uint8 * (16 * MAX_REM)), ("remainder_commitment", C.c_uint8 * 32),
        ("pow_nonce", C.c_uint64), ("positions", C.c_uint64 * (MAX_Q + 1)),
    ]


class Dump(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("trace_polys", "trace_lde", "trace_leaves", "composition",
                                          "comp_polys", "comp_lde", "deep", "fri_layer1")]


_lib = None
_runtime = None


def mapped_files(prefix: str) -> list:
    """Distinct files (resolved paths) mapped into this process whose name starts with `prefix`."""
    found = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith(prefix):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


class _RefuseSecondRuntime:
    """sys.meta_path guard installed once the library has mapped the HIP runtime it links (/opt/rocm): importing
    torch afterwards would map torch's bundled libamdhip64 as a SECOND runtime (torch asks for the soname
    libamdhip64.so, which the loaded libamdhip64.so.7 does not satisfy).  A process that needs both must import
    torch first; the library then shares torch's copy (one runtime, recorded by runtime_info())."""

    def find_spec(self, name, path=None, target=None):
        if name == "torch" or name.startswith("torch."):
            raise ImportError(
                f"zkvm_amd: {LIB_PATH.name} has already mapped {runtime_info()['hip_runtime']}; importing torch now "
                f"would load torch's own HIP runtime as a second one -- import torch before the first native.lib() "
                f"call, or keep GPU work torch-free")
        return None


def runtime_info() -> dict:
    """The HIP runtime and RCCL this process's library runs on: the mapped files and their versions."""
    global _runtime
    if _runtime is None:
        L = lib()
        hv, rv = C.c_int(0), C.c_int(0)
        rc = L.zk_runtime_versions(C.byref(hv), C.byref(rv))
        hips, rccls = mapped_files("libamdhip64.so"), mapped_files("librccl.so")
        _runtime = {"hip_runtime": hips[0] if len(hips) == 1 else hips, "rccl": rccls[0] if len(rccls) == 1 else rccls,
                    "hip_runtime_version": hv.value if rc == ZK_OK else None,
                    "rccl_version": rv.value if rc == ZK_OK else None,
                    "torch_loaded_first": "torch" in __import__("sys").modules}
    return dict(_runtime)


def lib():
    global _lib
    if _lib is None:
        import sys
        if not LIB_PATH.exists():
            raise ZkError(ZK_ERR_DEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C encrypt-zkvm_amd)")
        L = C.CDLL(str(LIB_PATH))
        hips = mapped_files("libamdhip64.so")
        if len(hips) != 1:
            raise ZkError(ZK_ERR_DEVICE, f"{len(hips)} HIP runtimes mapped into this process ({hips}): exactly one "
                                         f"must serve {LIB_PATH.name}")
        if "torch" not in sys.modules and not any(isinstance(f, _RefuseSecondRuntime) for f in sys.meta_path):
            sys.meta_path.insert(0, _RefuseSecondRuntime())
        vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
        L.zk_last_error.restype = C.c_char_p
        L.zk_device_count.argtypes = [C.POINTER(i32)]
        L.zk_runtime_versions.argtypes = [C.POINTER(i32), C.POINTER(i32)]
        L.zk_device_pci_bus_id.argtypes = [i32, C.c_char_p, i32]
        L.zk_device_synchronize.argtypes = [i32]
        L.zk_prover_create.argtypes = [i32, sz, u32, C.POINTER(vp)]
        L.zk_prover_create_shard.argtypes = [i32, sz, i32, C.POINTER(vp)]
        L.zk_prover_destroy.argtypes = [vp]
        L.zk_prover_destroy.restype = None
        L.zk_prover_acquire.argtypes = [i32, sz, u32, C.POINTER(vp)]
        L.zk_prover_release.argtypes = [vp]
        L.zk_prover_release.restype = None
        L.zk_prover_pool_trim.argtypes = [i32]
        L.zk_prover_trace_buffer.argtypes = [vp, C.POINTER(vp)]
        L.zk_prove.argtypes = [vp, vp, sz, C.POINTER(Options), C.POINTER(PubInputs), vp, C.POINTER(sz)]
        L.zk_prove_columns.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(Options), C.POINTER(PubInputs), vp,
                                       C.POINTER(sz)]
        L.zk_prove_columns_ex.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(Options), C.POINTER(PubInputs), vp,
                                          C.POINTER(sz), C.POINTER(Record), C.POINTER(Dump)]
        L.zk_host_alloc.argtypes = [sz, C.POINTER(vp)]
        L.zk_host_free.argtypes = [vp]
        L.zk_host_free.restype = None
        L.zk_host_register.argtypes = [vp, sz]
        L.zk_host_unregister.argtypes = [vp]
        L.zk_prove_device.argtypes = [vp, vp, sz, C.POINTER(Options), C.POINTER(PubInputs), vp, C.POINTER(sz),
                                      C.POINTER(Record), C.POINTER(Dump)]
        L.zk_validate_device.argtypes = [vp, vp, sz, C.POINTER(PubInputs), C.POINTER(Validation)]
        L.zk_validate_columns.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(PubInputs), C.POINTER(Validation)]
        L.zk_prover_set_validate.argtypes = [vp, i32]
        L.zk_prover_validation.argtypes = [vp, C.POINTER(Validation)]
        if hasattr(L, "zk_degrees_device"):  # (an A/B library of an earlier commit, ZKVM_GPU_LIB, has none of the four)
            L.zk_degrees_device.argtypes = [vp, vp, sz, C.POINTER(PubInputs), C.POINTER(Degrees), vp]
            L.zk_degrees_columns.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(PubInputs), C.POINTER(Degrees), vp]
            L.zk_prover_set_validate_degrees.argtypes = [vp, i32]
            L.zk_prover_degrees.argtypes = [vp, C.POINTER(Degrees)]
        L.zk_lde_new.argtypes = [vp, vp, sz, sz, u32, C.POINTER(vp), vp]
        L.zk_lde_read_frame.argtypes = [vp, sz, vp, vp]
        L.zk_lde_query.argtypes = [vp, vp, sz, vp, vp, C.POINTER(sz)]
        L.zk_lde_free.argtypes = [vp]
        L.zk_lde_free.restype = None
        L.zk_eval_constraints.argtypes = [vp, C.POINTER(PubInputs), vp, vp, vp]
        L.zk_commit_composition.argtypes = [vp, vp, u32, C.POINTER(vp), vp, vp]
        L.zk_comp_query.argtypes = [vp, vp, sz, vp, vp, C.POINTER(sz)]
        L.zk_comp_free.argtypes = [vp]
        L.zk_comp_free.restype = None
        if hasattr(L, "zk_lde_new_columns"):  # (an A/B library of an earlier commit, ZKVM_GPU_LIB, has none of the three)
            # (p, columns[28], n, blowup, out, root, polys_out)
            L.zk_lde_new_columns.argtypes = [vp, C.POINTER(vp), sz, u32, C.POINTER(vp), vp, vp]
            # (lde, pub, ext, coeff_t, coeff_b, out)
            L.zk_eval_constraints_ext.argtypes = [vp, C.POINTER(PubInputs), u32, vp, vp, vp]
            # (lde, composition, ext, num_cols, out, root, polys_out)
            L.zk_commit_composition_ext.argtypes = [vp, vp, u32, u32, C.POINTER(vp), vp, vp]
        if hasattr(L, "zk_lde_read_rows"):  # (likewise: the bulk reads came later)
            # (handle, first, count, rows_out)
            L.zk_lde_read_rows.argtypes = [vp, sz, sz, vp]
            L.zk_comp_read_rows.argtypes = [vp, sz, sz, vp]
        L.zk_prover_stage_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32, C.POINTER(i32)]
        L.zk_prover_profile.argtypes = [vp, i32]
        L.zk_prover_set_upload_schedule.argtypes = [vp, i32]
        L.zk_prover_proof_info.argtypes = [vp, C.POINTER(ProofInfo)]
        L.zk_prover_kernel_stats.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(i32),
                                             C.POINTER(C.c_double), i32, C.POINTER(i32)]
        L.zk_prover_kernel_ops.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), i32, C.POINTER(i32)]
        L.zk_prover_upload_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.zk_prover_upload_derived.argtypes = [vp, C.POINTER(u32)]
        L.zk_prover_upload_fixed.argtypes = [vp, C.POINTER(u32)]
        if hasattr(L, "zk_prover_coeff_sources"):  # (an A/B library of an earlier commit has none)
            L.zk_prover_coeff_sources.argtypes = [vp, C.POINTER(u32)]
            # (in[13] as zk_diag_upload_plan, bit 6 of in[12]: ZK_COEFF_SRC; n) -> UploadPlan::coeff_src
            L.zk_diag_upload_plan_coeff_src.argtypes = [vp, sz]
            # (device, planes[29 n], modes[28], w[28], cpolys, ccols, n, ext, z, zg, alpha_t, alpha_c, coeff_b, bnd1, c,
            #  ood_out, deep_out, col0_out, flag_out)
            L.zk_diag_coeff_sources.argtypes = [i32, vp, vp, vp, vp, i32, sz, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                vp, vp]
        L.zk_prover_exchange_stats.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                               C.POINTER(i32), i32, C.POINTER(i32)]
        L.zk_verify.argtypes = [vp, sz, C.POINTER(PubInputs), u32, C.c_char_p, sz]
        L.zk_comm_create_loopback.argtypes = [i32, C.POINTER(vp)]
        L.zk_comm_unique_id.argtypes = [vp]
        L.zk_comm_create_rccl.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
        L.zk_comm_create_host.argtypes = [i32, i32, EXCHANGE_FN, vp, C.POINTER(vp)]
        L.zk_comm_destroy.argtypes = [vp]
        L.zk_comm_destroy.restype = None
        L.zk_comm_set_measure.argtypes = [vp, i32]
        L.zk_comm_set_trace_split.argtypes = [vp, i32]
        L.zk_prover_exchange_stats_ex.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_double), C.POINTER(i32), i32, C.POINTER(i32)]
        L.zk_prover_shard_schedule.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
        L.zk_prove_sharded.argtypes = [vp, C.POINTER(vp), i32, vp, sz, C.POINTER(Options), C.POINTER(PubInputs), vp,
                                       C.POINTER(sz), C.POINTER(Record)]
        if hasattr(L, "zk_degrees_sharded"):  # (an A/B library of an earlier commit, ZKVM_GPU_LIB, has none)
            # (comm, provers[nlocal], nlocal, trace, n, pub, out, quotients_out[nlocal])
            L.zk_degrees_sharded.argtypes = [vp, C.POINTER(vp), i32, vp, sz, C.POINTER(PubInputs), C.POINTER(Degrees),
                                             C.POINTER(vp)]
        L.zk_vm_trace.argtypes = [C.c_char_p, vp, sz, vp, sz, u32, u32, vp, vp, sz, C.POINTER(sz), vp, vp]
        L.zk_vm_last_error.restype = C.c_char_p
        L.zk_program_compile.argtypes = [C.c_char_p, C.POINTER(vp), vp, C.POINTER(sz)]
        L.zk_program_trace.argtypes = [vp, vp, sz, vp, sz, u32, u32, vp, vp, sz, C.POINTER(sz), vp]
        L.zk_vm_trace_device.argtypes = [vp, vp, vp, sz, vp, sz, u32, u32, vp, C.POINTER(sz), vp]
        L.zk_vm_prove.argtypes = [vp, vp, vp, sz, vp, sz, u32, u32, vp, C.POINTER(Options), vp, C.POINTER(sz), vp, vp]
        L.zk_vm_prove_sharded.argtypes = [vp, vp, C.c_int, vp, vp, sz, vp, sz, u32, u32, vp, C.POINTER(Options), vp,
                                          C.POINTER(sz), vp, vp]
        L.zk_diag_vm_states.argtypes = [vp, vp, sz, vp, sz, u32, u32, sz, sz, vp, vp]
        L.zk_program_free.argtypes = [vp]
        L.zk_program_free.restype = None
        L.zk_diag_mul_limbs_host.argtypes = [vp, vp, vp, sz]
        L.zk_diag_mul_limbs_host.restype = None
        L.zk_diag_dot_host.argtypes = [vp, vp, sz, vp]
        L.zk_diag_dot_host.restype = None
        L.zk_diag_blake3_host.argtypes = [vp, sz, vp]
        L.zk_diag_blake3_host.restype = None
        # (in[13], n, masks[8], counts[7], cols[4 W], width[W], off[W + 1], pb[W + 1], gsz[W])
        if hasattr(L, "zk_diag_upload_plan"):  # (an A/B library of an earlier commit, ZKVM_GPU_LIB, has none)
            L.zk_diag_upload_plan.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "zk_diag_shard_rounds"):
            # (U[nU], nU, G, rep, out[rounds (3 + 2 G)], cap, rounds) / (M, G, is_node, idx[count], count, out[3 count])
            L.zk_diag_shard_rounds.argtypes = [vp, i32, i32, i32, vp, sz, vp]
            L.zk_diag_shard_locate.argtypes = [C.c_uint64, i32, i32, vp, sz, vp]
        L.zk_diag_field_op.argtypes = [i32, i32, vp, vp, vp, sz]
        L.zk_diag_blake3_rows.argtypes = [i32, vp, i32, sz, vp]
        L.zk_diag_ntt.argtypes = [i32, vp, sz, i32, i32, vp, vp]
        L.zk_diag_make_ws_host.argtypes = [vp, vp]
        L.zk_diag_make_ws_host.restype = None
        # (device, in, n, ncols, blowup, r0, rstride, ncos, from_evals, out)
        L.zk_diag_lde.argtypes = [i32, vp, sz, i32, u32, i32, i32, i32, i32, vp]
        if hasattr(L, "zk_diag_ood"):  # (an A/B library of an earlier commit has none of the three)
            # (device, tpolys, cpolys, ccols, n, ext, z, zg, rank, G, out)
            L.zk_diag_ood.argtypes = [i32, vp, vp, i32, sz, i32, vp, vp, i32, i32, vp]
            # (device, tpolys, cpolys, ccols, n, ext, z, zg, alpha_t, alpha_c, out)
            L.zk_diag_deep.argtypes = [i32, vp, vp, i32, sz, i32, vp, vp, vp, vp, vp]
            # (device, seed32, start, count, bits, best_out)
            L.zk_diag_grind.argtypes = [i32, vp, C.c_uint64, u32, i32, C.POINTER(C.c_uint64)]
        if hasattr(L, "zk_diag_fri_layer"):
            # (device, tpolys, cpolys, ccols, n, ext, z, zg, alpha_t, alpha_c, parts, out)
            L.zk_diag_deep_parts.argtypes = [i32, vp, vp, i32, sz, i32, vp, vp, vp, vp, i32, vp]
            # (device, layer, L, ext, fold, lb, wstride, alpha, root_out, next_out)
            L.zk_diag_fri_layer.argtypes = [i32, vp, sz, i32, i32, i32, sz, vp, vp, vp]
        if hasattr(L, "zk_diag_composition"):
            # (device, comp, n, blowup, ext, ncols, nce, tpolys, coeff_b, bnd1, polys_out, root_out, flag_out)
            L.zk_diag_composition.argtypes = [i32, vp, sz, u32, i32, i32, i32, vp, vp, vp, vp, vp, C.POINTER(u32)]
            # (device, comp, n, ext, ncols, parts, tpolys, coeff_b, bnd1, polys_out, flag_out)
            L.zk_diag_composition_parts.argtypes = [i32, vp, sz, i32, i32, i32, vp, vp, vp, vp, C.POINTER(u32)]
        if hasattr(L, "zk_diag_detect"):
            # (device, cols, n, ncols, c0, how, parts, flags_out[4 * 28], last_out[28], polys_out)
            L.zk_diag_detect.argtypes = [i32, vp, sz, i32, i32, i32, i32, vp, vp, vp]
            # (device, trace, n, blowup, flags_out, polys_out, lde_out, root_out)
            L.zk_diag_trace_commit.argtypes = [i32, vp, sz, u32, vp, vp, vp, vp]
            # (device, last[28], sparse_mask, clock, n, blowup, polys_out, lde_out)
            L.zk_diag_column_fills.argtypes = [i32, vp, u32, i32, sz, u32, vp, vp]
            # (device, packed, packed_len, count, col[], width[], off[], last, n, out)
            L.zk_diag_expand_narrow.argtypes = [i32, vp, sz, i32, vp, vp, vp, vp, sz, vp]
            # (op, col, aux, r0, r1, width, dst) -> the check's verdict / (r0, r1, R, ranges_out, cap, count_out)
            L.zk_diag_host_rows.argtypes = [i32, vp, vp, sz, sz, i32, vp]
            L.zk_diag_row_tasks.argtypes = [sz, sz, sz, vp, sz, C.POINTER(sz)]
        if hasattr(L, "zk_comm_agreement"):  # (an A/B library of an earlier commit has none)
            L.zk_comm_agreement.argtypes = [vp, C.POINTER(Agreement)]
        if hasattr(L, "zk_diag_merkle"):
            # (device, leaves, nl, l3_min_log, pf_blocks, block_p, nodes_out, guard_out[2 * 4096], leaves_out, positions,
            #  k, proof_out, proof_len)
            L.zk_diag_merkle.argtypes = [i32, vp, sz, i32, u32, u32, vp, vp, vp, vp, sz, vp, C.POINTER(sz)]
        if hasattr(L, "zk_queue_create"):  # (an A/B library of an earlier commit, ZKVM_GPU_LIB, has no proof queue)
            u64 = C.c_uint64
            L.zk_queue_create.argtypes = [i32, sz, u32, i32, C.POINTER(vp)]
            L.zk_queue_destroy.argtypes = [vp]
            L.zk_queue_destroy.restype = None
            L.zk_queue_set_validate.argtypes = [vp, i32]
            L.zk_queue_set_validate_degrees.argtypes = [vp, i32]
            L.zk_queue_pause.argtypes = [vp]
            L.zk_queue_resume.argtypes = [vp]
            # (q, columns[28] / d_trace, n, opt, pub, proof_out, proof_cap, job)
            L.zk_queue_submit_columns.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(Options), C.POINTER(PubInputs), vp, sz,
                                                  C.POINTER(u64)]
            L.zk_queue_submit_device.argtypes = [vp, vp, sz, C.POINTER(Options), C.POINTER(PubInputs), vp, sz,
                                                 C.POINTER(u64)]
            # (q, prog, public, num_public, secret, num_secret, lwe_size, delta, last_row, opt, proof_out, proof_cap,
            #  outputs, program_hash, job)
            L.zk_queue_submit_vm.argtypes = [vp, vp, vp, sz, vp, sz, u32, u32, vp, C.POINTER(Options), vp, sz, vp, vp,
                                             C.POINTER(u64)]
            L.zk_queue_wait.argtypes = [vp, u64, C.POINTER(JobResult)]
            L.zk_queue_poll.argtypes = [vp, u64, C.POINTER(JobResult)]
            L.zk_queue_wait_any.argtypes = [vp, C.POINTER(u64), C.POINTER(JobResult)]
            L.zk_queue_cancel.argtypes = [vp, u64]
            L.zk_queue_job_validation.argtypes = [vp, u64, C.POINTER(Validation)]
            L.zk_queue_job_degrees.argtypes = [vp, u64, C.POINTER(Degrees)]
            L.zk_queue_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), C.POINTER(u32),
                                         C.POINTER(u32)]
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != ZK_OK:
        msg = lib().zk_last_error()
        raise ZkError(rc, f"{what}: {msg.decode() if msg else ''}")


def device_count() -> int:
    c = C.c_int(0)
    lib().zk_device_count(C.byref(c))
    return c.value


def pci_bus_id(device: int) -> str:
    buf = C.create_string_buffer(32)
    check(lib().zk_device_pci_bus_id(device, buf, len(buf)), "zk_device_pci_bus_id")
    return buf.value.decode()


def synchronize(device: int):
    check(lib().zk_device_synchronize(device), "zk_device_synchronize")


def hip_runtime():
    """ctypes handle of the HIP runtime the library runs on (the same mapped file: dlopen returns its handle)."""
    path = runtime_info()["hip_runtime"]
    h = C.CDLL(path)
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h
