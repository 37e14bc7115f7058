/*
 * zkvm_gpu.h -- C ABI of the MI355X (gfx950) STARK prover for the Encrypt-zkVM execution trace.
 *
 * Drop-in boundary: every entry point below replaces one piece of the reference's
 * `impl winterfell::Prover for ExecutionProver` (prover/src/lib.rs:40-77) as driven by
 * `vm::prove` (vm/src/lib.rs:13-29).  The reference Rust host would bind these through a
 * thin FFI (see INTEGRATION.md for the cgo-style/Rust `extern "C"` stubs).
 *
 * Conventions
 *  - Field elements are winterfell f128 values (p = 2^128 - 45*2^40 + 1), canonical,
 *    16 bytes little-endian each (the `f128::BaseElement` byte format).
 *  - Trace matrices are column-major: column c occupies bytes [c*n*16, (c+1)*n*16).  The
 *    column order is the one `Processor::trace` emits (vm/src/processor/mod.rs:76-84):
 *    clk, 5 opcode bits, hash flag, 4 sponge words, stack depth, 16 stack registers (28 total).
 *  - All functions return ZK_OK (0) or a negative status, never abort, and leave a message
 *    for zk_last_error() (thread-local).  Buffers are owned by the caller.
 *  - A zk_prover owns one GPU's device memory and one HIP stream.  Calls on one prover are not
 *    reentrant; different provers may be used from different threads concurrently.
 */
#ifndef ZKVM_GPU_H
#define ZKVM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_OK 0
#define ZK_ERR_INVALID_ARG -1
#define ZK_ERR_BUFFER_TOO_SMALL -2
#define ZK_ERR_DEVICE -3
#define ZK_ERR_OUT_OF_MEMORY -4
#define ZK_ERR_PEER -5      /* sharded proof: another rank refused it (that rank and its reason in the message) */
#define ZK_ERR_PENDING -6   /* zk_queue_poll: the job has not finished */
#define ZK_ERR_CANCELLED -7 /* proof queue: the job was cancelled before it started */
#define ZK_ERR_PROGRAM -10  /* ProgramError (vm/src/program/errors.rs) */
#define ZK_ERR_STACK -11    /* StackError (vm/src/processor/errors.rs:4-42) */
#define ZK_ERR_CHIPLETS -12 /* ChipletsError (vm/src/processor/errors.rs:44-71) */
#define ZK_ERR_DEGREE -20   /* proof written, but the trace does not satisfy ProcessorAir */
#define ZK_ERR_VERIFY -30   /* zk_verify: the proof is rejected (reason in msg) */

#define ZK_TRACE_WIDTH 28
#define ZK_MAX_COLS 32
#define ZK_MAX_TCONS 32
#define ZK_MAX_ASSERTS 32
#define ZK_MAX_CCOLS 16
#define ZK_MAX_FRI_LAYERS 16
#define ZK_MAX_REMAINDER 256
#define ZK_MAX_QUERIES 255

/* ProofOptions::new(num_queries, blowup, grinding, field_extension, fri_folding, fri_rem_max_deg)
 * -- the reference hard-codes (32, 8, 0, None, 8, 127) at vm/src/lib.rs:20.
 * field_extension: 1 = FieldExtension::None, 2 = FieldExtension::Quadratic; 3 (Cubic) is refused
 * with ZK_ERR_INVALID_ARG (winter-math implements no cubic extension of f128). */
typedef struct {
    uint32_t num_queries;
    uint32_t blowup;
    uint32_t grinding;
    uint32_t field_extension;
    uint32_t fri_folding;
    uint32_t fri_rem_max_deg;
} zk_options;

/* air::PublicInputs (air/src/lib.rs:18-47) plus the two ServerKey values the constraints use
 * (lwe_size = k + 1, delta = q / p; fhe/src/server_key.rs:78-124, fhe/src/parameters.rs:17).
 * The reference also carries the ServerKey's secret bits here; the constraints never read them. */
typedef struct {
    uint8_t program_hash[2][16];
    uint8_t stack_outputs[16][16];
    uint32_t lwe_size;
    uint32_t delta;
} zk_pub_inputs;

/* Every deterministic intermediate of one proof (for stage-wise parity checks).  Same layout as
 * the oracle's or_record. */
typedef struct {
    uint32_t trace_len, lde_len, width, num_ccols, num_fri_layers, remainder_len;
    uint32_t num_positions;
    uint32_t _pad;
    uint8_t trace_root[32];
    uint8_t coeff_t[ZK_MAX_TCONS][16];
    uint8_t coeff_b[ZK_MAX_ASSERTS][16];
    uint8_t constraint_root[32];
    uint8_t z[16];
    uint8_t ood_trace_z[ZK_MAX_COLS][16];
    uint8_t ood_trace_zg[ZK_MAX_COLS][16];
    uint8_t ood_constraints[ZK_MAX_CCOLS][16];
    uint8_t deep_t[ZK_MAX_COLS][16];
    uint8_t deep_c[ZK_MAX_CCOLS][16];
    uint8_t fri_roots[ZK_MAX_FRI_LAYERS][32];
    uint8_t fri_alphas[ZK_MAX_FRI_LAYERS][16];
    uint8_t remainder[ZK_MAX_REMAINDER][16];
    uint8_t remainder_commitment[32];
    uint64_t pow_nonce;
    uint64_t positions[ZK_MAX_QUERIES + 1];
} zk_record;

/* Optional host copies of full-size intermediates (NULL = skip), natural LDE order.  A trace the AIR rejects at
 * the out-of-domain identity (ZK_ERR_DEGREE before the DEEP stage) still fills the six up to comp_lde. */
typedef struct {
    uint8_t *trace_polys;  /* 28 * n coefficients, column-major */
    uint8_t *trace_lde;    /* N * 28, row-major */
    uint8_t *trace_leaves; /* N * 32 */
    uint8_t *composition;  /* 8n evaluations over the constraint-evaluation domain */
    uint8_t *comp_polys;   /* c * n coefficients, column-major */
    uint8_t *comp_lde;     /* N * c, row-major */
    uint8_t *deep;         /* N evaluations */
    uint8_t *fri_layer1;   /* N / fold evaluations */
} zk_dump;

typedef struct zk_prover zk_prover;
typedef struct zk_trace_lde zk_trace_lde;

const char *zk_last_error(void);
int zk_device_count(int *count);

/* ---- the runtime this library is linked against (no reference counterpart: host plumbing) ----
 * The library needs libamdhip64.so.7 and librccl.so.1 (RUNPATH /opt/rocm/lib).  A host that also loads another
 * copy of either (PyTorch bundles its own) must load it first, or the process maps two HIP runtimes; these calls let a
 * host get what it needs from the copy the library uses instead.  zk_runtime_versions: hipRuntimeGetVersion and
 * ncclGetVersion of the mapped copies.  zk_device_pci_bus_id: "dddd:bb:dd.f" of a device (the host's NUMA binding
 * reads /sys/bus/pci/devices/<id>/numa_node).  zk_device_synchronize: hipDeviceSynchronize on one device (the bench's
 * barriers). */
int zk_runtime_versions(int *hip_runtime, int *rccl);
int zk_device_pci_bus_id(int device, char *bus_id, int len);
int zk_device_synchronize(int device);

/* ---- prover object: device memory sized for traces up to max_trace_len rows ----
 * Process-wide side effect: the first zk_prover_create on a device that the process has not used yet
 * sets hipDeviceScheduleSpin for that device, so every host thread waiting on a stream of that device
 * (this library's transcript round trips, and any other code's syncs) busy-spins instead of yielding
 * (-0.05 ms per 2^20 proof).  Set ZK_SPIN_WAIT=0 in the environment to keep the runtime's default. */
int zk_prover_create(int device, size_t max_trace_len, uint32_t max_blowup, zk_prover **out);
/* A prover sized for ONE rank of a `world`-way coset-sharded proof (zk_prove_sharded, blowup 8): the buffers of
 * the LDE domain (trace and composition LDE, DEEP, NTT scratch, Merkle subtrees) hold the rank's 8/world cosets
 * only -- about 12.6 GB per rank at 2^22, world 8, against 50 GB for a full prover.  It serves zk_prove_sharded
 * with that world size; every single-GPU entry point refuses it (ZK_ERR_INVALID_ARG). */
int zk_prover_create_shard(int device, size_t max_trace_len, int world, zk_prover **out);
void zk_prover_destroy(zk_prover *p);
/* Process-wide pool for callers that build a prover per proof, as the reference does (ExecutionProver::new inside
 * vm::prove, vm/src/lib.rs:24): zk_prover_acquire returns an idle pooled full prover of this device with at least
 * these sizes (the smallest such; its per-size tables are already built), else creates one; zk_prover_release hands
 * it back instead of freeing its ~12.5 GB (2^20).  Thread-safe.  zk_prover_pool_trim frees the idle provers of one
 * device (-1: every device) and returns how many. */
int zk_prover_acquire(int device, size_t max_trace_len, uint32_t max_blowup, zk_prover **out);
void zk_prover_release(zk_prover *p);
int zk_prover_pool_trim(int device);
/* device pointer to a scratch region large enough for a 28 x max_trace_len trace (so callers can
 * stage a device-resident trace without their own allocator) */
int zk_prover_trace_buffer(zk_prover *p, void **d_trace);

/* Prover::prove (vm/src/lib.rs:26 -> winterfell generate_proof), whole proof.
 * Host trace variant: trace is 28 x n, column-major, host memory.  The trace goes up in column groups on
 * a copy stream, each group's interpolation and coset LDE starting as soon as it is in HBM.  From
 * page-locked memory (zk_host_alloc / zk_host_register) the copies are DMAs at the link rate; pageable
 * memory works too, staged by the HIP runtime at a lower rate.  The trace is not read after return. */
int zk_prove(zk_prover *p, const uint8_t *trace, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
             uint8_t *proof_out, size_t *proof_len);
/* The same with one pointer per column (n * 16 bytes each): winterfell's ColMatrix / TraceTable keeps
 * every column in its own Vec<f128> (vm/src/lib.rs:18), which binds here without a flattening copy. */
int zk_prove_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_options *opt,
                     const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len);
/* ... with the optional record / dumps of zk_prove_device */
int zk_prove_columns_ex(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_options *opt,
                        const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len, zk_record *rec,
                        const zk_dump *dump);
/* Page-locked host memory for traces (hipHostMalloc, usable from every device), e.g. the buffer the
 * VM writes its trace into (zk_vm_trace), and page-locking of a caller's own buffer (hipHostRegister:
 * costs about as much as one copy of it, so register buffers that are reused). */
int zk_host_alloc(size_t bytes, void **ptr);
void zk_host_free(void *ptr);
int zk_host_register(void *ptr, size_t bytes);
int zk_host_unregister(void *ptr);
/* Device trace variant (trace already resident in HBM on this prover's device), with optional
 * record / dumps.  proof_len is in/out: capacity in, bytes written out; ZK_ERR_BUFFER_TOO_SMALL
 * reports the needed size. */
int zk_prove_device(zk_prover *p, const void *d_trace, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                    uint8_t *proof_out, size_t *proof_len, zk_record *rec, const zk_dump *dump);

/* ---- trace validation: winterfell 0.9 Prover::prove runs `trace.validate(&air)` under #[cfg(debug_assertions)]
 * before it proves (Trace::validate: every assertion of get_assertions against the trace, then evaluate_transition
 * at every step 0 .. n - 1 - num_transition_exemptions), and panics with the first failure:
 *   "trace does not satisfy assertion main_trace(col, step) == value"
 *   "main transition constraint i did not evaluate to ZERO at step s"
 * Here the whole trace is checked on the GPU and every failure is counted, not only the first.
 * Semantics.  Base field; trace 28 x n column-major, n and lwe_size bounded as for zk_prove.  Transition constraints:
 * evaluate_transition (air/src/lib.rs:104-168) at steps s = 0 .. n - 3 (set_num_transition_exemptions(2), lib.rs:94),
 * frame = rows (s, s + 1), periodic values = row s mod 16 of CYCLE_MASK || round constants (lib.rs:201-225).
 * Assertions: the 22 of get_assertions in that method's order (lib.rs:170-195): clk@0, depth@0, (7+i)@0 and
 * (7+i)@n-2 for i < 2, (12+i)@0 and (12+i)@n-2 for i < 8.  First failure, as winterfell would hit it: the lowest
 * failing assertion, else the lowest failing step and at it the lowest constraint.  Row n - 1 is never constrained.
 * Values are 16-byte little-endian field elements. */
#define ZK_ERR_TRACE -21 /* validation: the trace violates ProcessorAir; no proof was written */
typedef struct {
    uint64_t trace_len, steps_checked;  /* n, n - 2 */
    uint64_t failing_steps;             /* steps with at least one non-zero transition constraint */
    uint64_t t_count[ZK_MAX_TCONS];     /* per constraint (evaluate_transition's result index): steps where it is non-zero */
    uint64_t t_first[ZK_MAX_TCONS];     /* the lowest such step, UINT64_MAX if none */
    uint8_t t_value[ZK_MAX_TCONS][16];  /* its value at t_first (zero if none) */
    uint32_t a_failed, a_mask;          /* count; bit k = assertion k in get_assertions order */
    uint32_t a_col[ZK_MAX_ASSERTS];
    uint64_t a_step[ZK_MAX_ASSERTS];
    uint8_t a_expected[ZK_MAX_ASSERTS][16], a_found[ZK_MAX_ASSERTS][16]; /* all 22 filled */
    int32_t first_kind;                 /* 0 valid, 1 assertion, 2 transition */
    int32_t first_index;                /* the assertion / constraint of the first failure (-1 if valid) */
    uint64_t first_step;
} zk_validation;
/* Trace::validate of a trace resident in this prover's device's HBM (e.g. in zk_prover_trace_buffer).  ZK_OK for a
 * valid trace, ZK_ERR_TRACE otherwise; `out` is filled either way.  On failure zk_last_error() carries the first
 * failure in winterfell's wording above, then "; <failing steps> failing steps, <failed assertions> failed
 * assertions".  One pass over the trace (448 B per row) and one small read; for each failing constraint the two
 * rows at its first step are read back and evaluated on the host as well (t_value), and ZK_ERR_DEVICE is returned if
 * the host finds zero where the device did not.  Refused (ZK_ERR_INVALID_ARG) for a prover of
 * zk_prover_create_shard, like every single-GPU entry point. */
int zk_validate_device(zk_prover *p, const void *d_trace, size_t n, const zk_pub_inputs *pub, zk_validation *out);
/* The same for a host trace, one pointer per column (winterfell's ColMatrix, as zk_prove_columns).  A debugging aid:
 * it costs one full upload -- the 28 columns are copied whole into the prover's trace buffer (none of zk_prove's
 * sparse, narrow, fixed or derived column classes) and validated there. */
int zk_validate_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_pub_inputs *pub,
                        zk_validation *out);
/* on = 1: the debug-build behaviour of Prover::prove.  zk_prove, zk_prove_columns(_ex) and zk_prove_device validate
 * the trace first (host traces through zk_validate_columns, then proved from the host columns as always), and
 * zk_vm_prove validates the trace it has written.  A failing trace returns ZK_ERR_TRACE with *proof_len = 0: no
 * proof is written and no column hint or snapshot is touched.  A valid trace goes on to the same proof bytes.
 * Default 0: nothing is validated, and a bad trace ends in ZK_ERR_DEGREE after the whole proof, as before.
 * The setting applies to rank-sized provers (zk_prover_create_shard) too: zk_prove_sharded and zk_vm_prove_sharded
 * validate first, split by rows over the ranks, when ANY rank's prover has it on ("what the ranks agree on" below). */
int zk_prover_set_validate(zk_prover *p, int on);
/* The report of the last validation that ran on p (by either call above or by a proof with the switch on);
 * ZK_ERR_INVALID_ARG if none has run. */
int zk_prover_validation(const zk_prover *p, zk_validation *out);

/* ---- transition constraint degrees: the second check of a winterfell 0.9 debug build.  Inside
 * DefaultConstraintEvaluator::evaluate, under #[cfg(debug_assertions)], validate_transition_degrees() takes every
 * transition constraint's evaluations over the constraint-evaluation (CE) domain, divides them by the transition
 * divisor, interpolates, and compares each quotient's degree with the one the AIR declares
 * (TransitionConstraintDegree, air/src/lib.rs:69-90); a mismatch panics with
 *   "transition constraint degrees didn't match\nexpected: [...]\nactual:   [...]"
 * (winterfell is not part of this repository: these semantics are recollected, like every winterfell citation of
 * DESIGN.md section 2; the anchor is that the reference's own example trace meets its declared degrees exactly under
 * this reading).  The reference is built around the check: set_num_transition_exemptions(2) (lib.rs:92-94) and the
 * thread_rng() last row of Processor::trace give every column polynomial degree n - 1.  A trace whose last row is not
 * generic (zeros, a copy of row n - 2) proves and verifies here, yet stops a debug build of the reference.
 * Semantics.  Base field; the CE domain is 3 <w_8n> (the AIR's CE blowup is 8, whatever the proof options say).
 * C_k(x), k < 20: evaluate_transition on the LDE frame (x, x g) with the periodic column polynomials at x, no
 * composition coefficients.  Q_k = C_k / D, D = (x^n - 1) / ((x - g^(n-2))(x - g^(n-1))), interpolated from its 8n
 * values; actual[k] = the index of Q_k's highest non-zero coefficient, 0 for the zero polynomial (polynom::degree_of).
 * expected[k] = base_k (n - 1) + cyc_k 15 n / 16 - (n - 2) with base = [1,5,2,6,6,6,7,7,6,6,6,6,4,7,4,4,2,2,2,2] and
 * cyc = 1 for k >= 12 (the hash constraints' periodic column of cycle 16).  The trace passes iff actual == expected
 * for all 20.  winterfell's second assertion, next_pow2(max(max actual, n + 1)) == 8n, is implied by a match; its left
 * side is reported (ce_len_needed) and does not decide the status. */
#define ZK_ERR_DEGREES -22   /* the transition constraint degrees differ from ProcessorAir's declared ones */
typedef struct {
    uint64_t trace_len, ce_len;               /* n, 8n */
    uint64_t expected[ZK_MAX_TCONS], actual[ZK_MAX_TCONS];
    uint32_t mismatch_mask, zero_mask, over_mask; /* bit k: actual != expected; Q_k == 0; actual > expected */
    uint32_t _pad;
    uint64_t max_actual, ce_len_needed;       /* next_pow2(max(max_actual, n + 1)) */
} zk_degrees;
/* validate_transition_degrees of a trace resident in this prover's device's HBM (28 x n column-major, n bounded as for
 * zk_prove; of pub only lwe_size and delta are read).  ZK_OK or ZK_ERR_DEGREES; `out` is filled either way, and on
 * failure zk_last_error() is winterfell's three-line message above with both vectors formatted as Rust's {:>3?}
 * ("[  1, 509, 128, ...]").  quotients_out (optional): the 20 x 8n coefficients of the Q_k, coefficient j of Q_k at
 * element k * 8n + j, 16 bytes little-endian each.  The check costs about a proof: a dense interpolation and 8-coset
 * LDE of all 28 columns (none of zk_prove's column classes), 20 quotient planes, 160 size-n inverse transforms.  It
 * runs in the prover's own buffers (trace polynomials, trace LDE, NTT scratch), so like a proof it ends the validity of
 * any zk_trace_lde / zk_comp_commit handle of this prover.  Refused (ZK_ERR_INVALID_ARG) for a prover of
 * zk_prover_create_shard. */
int zk_degrees_device(zk_prover *p, const void *d_trace, size_t n, const zk_pub_inputs *pub, zk_degrees *out,
                      uint8_t *quotients_out);
/* The same for a host trace, one pointer per column (winterfell's ColMatrix): the 28 columns are copied whole into the
 * prover's trace buffer and checked there. */
int zk_degrees_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_pub_inputs *pub,
                       zk_degrees *out, uint8_t *quotients_out);
/* on = 1: zk_prove, zk_prove_columns(_ex), zk_prove_device and zk_vm_prove run validate_transition_degrees before they
 * prove, after Trace::validate when zk_prover_set_validate is on as well (the order of a debug build: Prover::prove
 * validates the trace, then the evaluator checks the degrees).  A mismatch returns ZK_ERR_DEGREES with *proof_len = 0:
 * no proof is written and no column hint or snapshot is touched.  A pass goes on to the same proof bytes.  Default 0:
 * nothing changes, and zk_prover_set_validate keeps its meaning.  The setting applies to rank-sized provers
 * (zk_prover_create_shard) too: zk_prove_sharded and zk_vm_prove_sharded check the degrees first, split over the ranks
 * by CE coset and then by coefficient range (zk_degrees_sharded below), when ANY rank's prover has it on, after the
 * sharded trace validation when that is on as well. */
int zk_prover_set_validate_degrees(zk_prover *p, int on);
/* The report of the last degree check that ran on p (by either call above or by a proof with the switch on);
 * ZK_ERR_INVALID_ARG if none has run. */
int zk_prover_degrees(const zk_prover *p, zk_degrees *out);

/* ---- plug point 1: Prover::new_trace_lde (prover/src/lib.rs:55-62) -> DefaultTraceLde ---- */
/* interpolate the trace, extend it over the blowup coset domain and commit to its rows.
 * The LDE lives in the prover's device memory until zk_lde_free. */
int zk_lde_new(zk_prover *p, const uint8_t *trace, size_t width, size_t n, uint32_t blowup, zk_trace_lde **out,
               uint8_t root[32]);
/* TraceLde::read_main_trace_frame_into: rows lde_step and (lde_step + blowup) mod N */
int zk_lde_read_frame(zk_trace_lde *lde, size_t lde_step, uint8_t *cur, uint8_t *next);
/* TraceLde::query: rows at positions (width elements each, in the caller's order) + batch Merkle proof bytes
 * (u8 number of paths, then per path u8 length and its 32-byte digests: BatchMerkleProof's serialization).  The
 * positions (1 .. 255 of them, any order) must be distinct: a repeated one is ZK_ERR_INVALID_ARG, as
 * MerkleTree::prove_batch refuses it (DuplicateLeafIndex).  proof_len: in, the capacity of proof_out; out, the
 * proof's length -- also with ZK_ERR_BUFFER_TOO_SMALL, after which a call with that capacity succeeds.
 * zk_comp_query takes the same. */
int zk_lde_query(zk_trace_lde *lde, const uint64_t *positions, size_t k, uint8_t *rows_out, uint8_t *proof_out,
                 size_t *proof_len);
/* A slice of DefaultTraceLde's main segment RowMatrix (Prover::new_trace_lde, prover/src/lib.rs:55-62): rows
 * (first + k) mod N, k < count, of the trace LDE in natural order, row-major, 28 elements of 16 bytes each.  The
 * frame TraceLde::read_main_trace_frame_into(s) reads is rows s and s + blowup of it.  first < N, 1 <= count <=
 * N + blowup (a window of frames may run past the end of the domain: it wraps).  The layout change runs on the GPU;
 * rows_out takes contiguous copies (page-locked memory, zk_host_alloc / zk_host_register: at the link rate).
 * ZK_ERR_INVALID_ARG, before any launch and with rows_out untouched: a NULL handle or buffer, first >= N, count == 0,
 * count > N + blowup.  The call reads the prover's device state and writes its NTT scratch only: both kinds of
 * handle stay valid, so do the composition values a zk_eval_constraints_ext(out = NULL) left for
 * zk_commit_composition_ext(NULL), and no hint, snapshot or proof state is touched -- a proof on the prover afterwards
 * has the bytes it would have had.  zk_comp_read_rows keeps all of this too. */
int zk_lde_read_rows(zk_trace_lde *lde, size_t first, size_t count, uint8_t *rows_out);
void zk_lde_free(zk_trace_lde *lde);

/* ---- plug point 2: Prover::new_evaluator (prover/src/lib.rs:65-72) + evaluate ----
 * DefaultConstraintEvaluator over ProcessorAir: coeff_t = 20 transition coefficients,
 * coeff_b = 22 boundary coefficients (assertions sorted by (stride, step, column));
 * out receives the 8n composition-trace values in natural CE-domain order. */
int zk_eval_constraints(zk_trace_lde *lde, const zk_pub_inputs *pub, const uint8_t *coeff_t, const uint8_t *coeff_b,
                        uint8_t *out);

/* ---- plug point 3: Prover::build_constraint_commitment (winterfell 0.9 provided method;
 * SURVEY.md 8(b); its input is the CompositionPolyTrace new_evaluator's evaluate returns,
 * prover/src/lib.rs:65-72) ----
 * composition: the 8n values zk_eval_constraints writes (natural CE-domain order).  Interpolates them
 * over the CE coset, splits the polynomial into num_cols column polynomials of n coefficients
 * (CompositionPoly; polys_out, optional: num_cols x n, column-major), extends each over the trace
 * LDE's blowup coset domain and commits to the rows (ConstraintCommitment; root).  Returns
 * ZK_ERR_DEGREE (no handle) when the polynomial has a coefficient at or beyond num_cols * n.  The
 * handle reads the prover's device memory: valid until the next proof or commitment on that prover. */
typedef struct zk_comp_commit zk_comp_commit;
int zk_commit_composition(zk_trace_lde *lde, const uint8_t *composition, uint32_t num_cols, zk_comp_commit **out,
                          uint8_t root[32], uint8_t *polys_out);
/* ConstraintCommitment::query: rows (num_cols elements each) at positions + batch Merkle proof bytes */
int zk_comp_query(zk_comp_commit *comp, const uint64_t *positions, size_t k, uint8_t *rows_out, uint8_t *proof_out,
                  size_t *proof_len);
/* The same as zk_lde_read_rows for ConstraintCommitment's evaluations (winterfell keeps them as a RowMatrix<E>):
 * rows (first + k) mod N, k < count, of num_cols E elements (ext = 2: 32 bytes each, a then b), as zk_comp_query
 * returns them.  The same refusals and the same guarantees: nothing but the prover's NTT scratch is written. */
int zk_comp_read_rows(zk_comp_commit *comp, size_t first, size_t count, uint8_t *rows_out);
void zk_comp_free(zk_comp_commit *comp);

/* ---- the three plug points over the challenge field, with the polynomial tables ----
 * winterfell's trait methods are generic over E: FieldElement<BaseField = f128>; with FieldExtension::Quadratic the
 * composition coefficients, the CompositionPolyTrace<E> and the committed rows are E values.  Conventions of the calls
 * below: ext = 1 (E = f128) or 2 (the quadratic extension); 3 is refused with ZK_ERR_INVALID_ARG, as in zk_options.
 * An E element is 32 bytes: component a, then component b, 16 bytes little-endian each -- the form of the proof's own
 * out-of-domain frame.  With ext = 1 every E buffer is the plain 16-byte layout of the calls above, and the results
 * are theirs byte for byte.  Like them, the calls refuse a prover of zk_prover_create_shard. */
/* Prover::new_trace_lde (prover/src/lib.rs:55-62) -> (DefaultTraceLde, TracePolyTable).  zk_lde_new with one pointer
 * per column (n * 16 bytes each, winterfell's ColMatrix, as zk_prove_columns: no flattening copy) and the polynomial
 * table: polys_out (optional) receives the 28 x n interpolation coefficients, column-major -- what winterfell builds
 * the out-of-domain frame and the DEEP polynomial from.  The commitment runs without column hints, so every
 * coefficient is written before it is copied out.  Same root and same LDE as zk_lde_new on the flattened trace. */
int zk_lde_new_columns(zk_prover *p, const uint8_t *const *columns, size_t n, uint32_t blowup, zk_trace_lde **out,
                       uint8_t root[32], uint8_t *polys_out);
/* ConstraintEvaluator<E>::evaluate of DefaultConstraintEvaluator (Prover::new_evaluator, prover/src/lib.rs:65-72):
 * coeff_t = 20 and coeff_b = 22 E elements (the ConstraintCompositionCoefficients<E> the channel draws), out = the 8n
 * E values of the CompositionPolyTrace<E> in natural CE-domain order.  The trace and the constraints are base-field,
 * so each component of out is zk_eval_constraints with that component of every coefficient.  out = NULL: the values
 * stay in the prover's device memory for a zk_commit_composition_ext(composition = NULL) on this handle; any proof,
 * commitment, evaluation or check on the prover in between ends their validity. */
int zk_eval_constraints_ext(zk_trace_lde *lde, const zk_pub_inputs *pub, uint32_t ext, const uint8_t *coeff_t,
                            const uint8_t *coeff_b, uint8_t *out);
/* Prover::build_constraint_commitment over E (winterfell 0.9 provided method): composition = 8n E
 * values in natural CE-domain order, or NULL for the values the last zk_eval_constraints_ext(out = NULL) on this handle
 * left on the device with the same ext (ZK_ERR_INVALID_ARG if there are none, if ext differs, or if a proof or another
 * commitment has run on the prover since: that ends the validity of the retained values).  num_cols in [1, 8];
 * polys_out (optional): num_cols x n E elements, column-major -- the columns of CompositionPoly.  ZK_ERR_DEGREE (no
 * handle) when either component has a non-zero coefficient at or beyond num_cols * n.  The handle records ext:
 * zk_comp_query on it returns rows of num_cols E elements, and its batch Merkle proof is over leaves BLAKE3(row
 * bytes), as the whole-proof path commits them. */
int zk_commit_composition_ext(zk_trace_lde *lde, const uint8_t *composition, uint32_t ext, uint32_t num_cols,
                              zk_comp_commit **out, uint8_t root[32], uint8_t *polys_out);

/* ---- one proof sharded over several GPUs ----
 * The LDE domain is split by coset: rank g of `world` (1, 2, 4 or 8; blowup 8) owns the block of cosets
 * g * 8/world .. (g + 1) * 8/world - 1.  Exchanges (Merkle block nodes, composition coefficient slices, FRI layer 1,
 * openings)
 * go through a zk_comm: RCCL over xGMI with one process per GPU (zk_comm_unique_id on rank 0,
 * shared out of band, then zk_comm_create_rccl on every rank), or an in-process loopback that drives
 * every rank from one process (tests; one prover per rank), or a caller transport (zk_comm_create_host).
 * Every rank passes the same host trace (column-major, 28 x n x 16 B; rank g reads and uploads only
 * columns g, g + world, g + 2 world, ... and receives the other columns' polynomials from their owners),
 * or NULL: the whole trace already sits in each prover's zk_prover_trace_buffer.  Every rank receives
 * the same proof bytes, identical to zk_prove's. */
typedef struct zk_comm zk_comm;
int zk_comm_create_loopback(int world, zk_comm **out);
int zk_comm_unique_id(uint8_t id[128]);
int zk_comm_create_rccl(const uint8_t id[128], int rank, int world, int device, zk_comm **out);
/* A communicator over a caller-supplied transport (MPI, gloo, TCP; also across nodes): one rank per process.
 * For every exchange the library copies this rank's device chunk(s) to host memory, calls fn, and copies recv
 * back to the device.  op ZK_XCHG_ALL_TO_ALL: send holds `world` chunks of `bytes` (chunk d is for rank d), recv
 * receives `world` chunks (chunk s came from rank s); op ZK_XCHG_ALL_GATHER: send is one chunk of `bytes`, recv
 * receives the `world` chunks in rank order.  fn returns 0 on success (anything else fails the proof with
 * ZK_ERR_DEVICE); every rank calls it the same number of times with the same op and bytes. */
typedef int (*zk_exchange_fn)(void *ctx, int op, const void *send, void *recv, size_t bytes);
enum { ZK_XCHG_ALL_TO_ALL = 0, ZK_XCHG_ALL_GATHER = 1 };
int zk_comm_create_host(int rank, int world, zk_exchange_fn fn, void *ctx, zk_comm **out);
void zk_comm_destroy(zk_comm *comm);
/* Measurement mode of a loopback communicator (tools/shard_model.py): every rank's kernels and the exchange copies
 * run on ONE stream in program order, so each compute segment of the schedule (zk_prover_shard_schedule) is the
 * ranks' compute alone, serialised (no overlap, no exchange time inside); the proof bytes are unchanged.  on = 0
 * returns to the normal mode (exchanges on their own stream, overlapped with compute).  Refused for RCCL and
 * host-exchange communicators. */
int zk_comm_set_measure(zk_comm *comm, int on);
/* The trace interpolation's split when the trace is already in every rank's HBM (trace = NULL, zk_vm_prove_sharded):
 * `replicated` of the columns to interpolate are interpolated and extended by every rank itself, at the start, under
 * the first two coefficient all-gathers; the others are split round robin and all-gathered.  -1 (the default): the
 * library's choice (four columns), from tools/shard_model.py's replay of measured schedules.
 * Same proof bytes for every value. */
int zk_comm_set_trace_split(zk_comm *comm, int replicated);
int zk_prove_sharded(zk_comm *comm, zk_prover **provers, int nlocal, const uint8_t *trace, size_t n,
                     const zk_options *opt, const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len,
                     zk_record *rec);
/* ---- what the ranks agree on before a sharded proof touches the GPU ----
 * Every sharded entry point (world > 1) first runs its own argument checks into a status instead of returning, then
 * exchanges one 256-byte control record per rank over the communicator's control channel -- a host-to-host all-gather
 * (loopback: a memcpy; host exchange: the caller's callback with ZK_XCHG_ALL_GATHER on host buffers, no device round
 * trip; RCCL: a small device staging buffer the communicator owns) that needs nothing from a prover -- and every rank
 * maps the same records to the same outcome.  The one exception: a null or wrong-shaped communicator or prover list is
 * refused at once (no exchange is possible).  The record holds a layout version, world, rank, n, every member of
 * zk_options, a BLAKE3 of zk_pub_inputs, the trace source (host / device / preprocessed), the communicator's
 * zk_comm_set_trace_split and zk_comm_set_measure settings, the prover's zk_prover_set_validate switch, what this
 * process can detect (ZK_SPARSE, ZK_CLOCK and its tables), the column-hint set it would use, and its status.
 *  1. A rank whose own checks failed returns its own code and message, as before; every other rank returns ZK_ERR_PEER
 *     with "rank r refused the proof: <code>: <message>" (the lowest such rank).
 *  2. A field that must match differs -- world, n, options, public inputs, trace source, the two communicator
 *     settings: every rank returns ZK_ERR_INVALID_ARG with "sharded proof: ranks disagree on <field> (rank a: x, rank
 *     b: y)", the first differing field in that order, options by member (options.num_queries), the two lowest ranks
 *     holding different values.
 *  3. Otherwise: column detection and the derived clock run iff every rank can (AND); the column hints of a host trace
 *     are used iff every rank holds the same set (else every rank proves without and drops its set: no redo pass); the
 *     trace is validated first iff any rank's switch is on (OR).
 * So the ZK_* switches and the provers' histories no longer have to match across ranks for the collectives to pair
 * up: every rank issues the same collectives in the same order.  After 1 or 2 nothing else has run: communicator and
 * provers stay usable, and the next call with matching inputs proves as always.  zk_vm_prove_sharded takes the
 * preprocessed trace source only when no local prover validates, so there the switches must match (else: case 2,
 * "trace source").  Deadlines on a peer that never arrives are the transport's (the caller's callback, RCCL).
 * Sharded validation: rank g checks steps [g n / world, min((g + 1) n / world, n - 2)) of the trace -- in place for a
 * device trace, for a host trace from an upload of only its rows -- the partial reports are all-gathered over the
 * control channel and merged, every local prover stores the merged report, read with zk_prover_validation, and a failing
 * trace returns ZK_ERR_TRACE on every rank with *proof_len = 0 and zk_validate_device's message, before any data
 * collective.  zk_prover_exchange_stats lists the control exchanges as "control" and "validate_report".
 * Sharded degree check (any rank's zk_prover_set_validate_degrees; after the validation, before the proof's own data
 * collectives): "transition constraint degrees" above, unchanged, with the work split twice.  Every rank interpolates
 * the whole trace (a host trace: all 28 columns copied whole into every rank's trace buffer, a debugging aid) and
 * extends it over its own 8 / world CE cosets only; it forms the 20 quotients there, inverse-transforms them per
 * coset and sends each rank its n / world coefficients of every coset (one all-to-all, "degrees_slices": 20 x 8 x
 * n / world elements received per rank); a rank then forms coefficients k1 + n k2, k2 < 8, of its k1 range with the
 * composition's cross-coset step and keeps only each quotient's highest non-zero index.  The partial reports travel
 * over the control channel ("degrees_report"), every rank merges them (maximum of the tops, OR of the non-zero bits)
 * and every local prover stores the merged report (zk_prover_degrees).  A mismatch returns ZK_ERR_DEGREES on every
 * rank with *proof_len = 0 and zk_degrees_device's message; no hint state moves.  It runs in a rank-sized prover's own
 * buffers (trace LDE and NTT scratch of 28 x 8 / world x n each) and allocates nothing per call.  Cost: about a
 * single-GPU check's front (the dense interpolation, repeated on every rank) plus 1 / world of the rest; loopback on
 * one GPU at 2^20: 21 / 22 / 27 ms at world 2 / 4 / 8 against 15 ms single-GPU (profiles/shard_degrees_time.txt).  The
 * preprocessed trace source of zk_vm_prove_sharded is taken only when no local prover has either switch on. */
typedef struct {
    int32_t code;           /* ZK_OK; ZK_ERR_PEER (case 1); ZK_ERR_INVALID_ARG (case 2); the same on every rank */
    int32_t rank_a, rank_b; /* case 1: the rank that refused, -1; case 2: the two ranks named; else -1, -1 */
    int32_t detect, clock;  /* case 3: every rank detects sparse columns / may derive the clock */
    int32_t hints;          /* case 3: the ranks' hint sets are equal and fresh: this proof uses them */
    int32_t hints_equal;    /* case 3: the ranks' hint sets are equal (an equal empty set is no disagreement) */
    int32_t validate;       /* case 3: the trace is validated first */
    uint32_t world, _pad;
    uint64_t control_calls, control_bytes; /* control exchanges of the call, and the bytes each rank received in them */
    char field[32];         /* case 2: the field named; case 1: "status" */
    int32_t validate_degrees, _pad2; /* case 3: the transition constraint degrees are checked first */
} zk_agreement;
/* The outcome of the last sharded call on this communicator (ZK_ERR_INVALID_ARG if none has exchanged records). */
int zk_comm_agreement(const zk_comm *comm, zk_agreement *out);
/* The sharded degree check on its own: the control exchange of a proof first (refusals and disagreements as there;
 * the record's options are all zero), then the check described above.  `trace`: the flat column-major host trace of
 * zk_prove_sharded, or NULL: the trace is already in every prover's trace buffer.  ZK_OK or ZK_ERR_DEGREES, the same
 * report (`out`, optional) and message on every rank.  quotients_out (optional): nlocal pointers, a NULL entry skips
 * that rank; local rank l receives its slice of the coefficients, 20 x 8 x kg elements of 16 bytes with kg = n / world:
 * element [k][k2][kl] is coefficient k1 + n k2 of Q_k, k1 = rank kg + kl.  Lengths as a sharded proof's cross step:
 * n / world >= 8 and n >= 16 world.  world == 1 forwards to zk_degrees_columns / zk_degrees_device. */
int zk_degrees_sharded(zk_comm *comm, zk_prover **provers, int nlocal, const uint8_t *trace, size_t n,
                       const zk_pub_inputs *pub, zk_degrees *out, uint8_t *const *quotients_out);
/* The collectives of the last sharded proof on this (local rank 0) prover, aggregated by name (control,
 * validate_report, degrees_slices, degrees_report, trace_coeffs,
 * trace_digests, trace_roots, comp_slices, comp_columns, degree_flags, comp_digests, comp_roots, ood_parts,
 * deep_totals, deep_slices, fri0_digests, fri0_roots, fri_layer1, openings): ms between HIP events recorded on the
 * stream the collective runs on around each call (waiting for slower ranks included), bytes this rank received from
 * the other ranks, and the number of calls.  Valid once the proof has returned, until the next proof.  The two control
 * exchanges run on the host: their ms is host wall time, and they are all a refused or invalid proof lists. */
int zk_prover_exchange_stats(zk_prover *p, const char **names, float *ms, double *bytes, int *calls, int cap,
                             int *count);
/* The same with each collective's exposed time beside its total: exposed_ms is how long the compute stream waited
 * for it (events around the stream wait; 0 when the collective finished under the compute issued meanwhile).  The
 * collectives run on a stream of their own (round 6), so only what a stage waits for shows up as exposed. */
int zk_prover_exchange_stats_ex(zk_prover *p, const char **names, float *ms, float *exposed_ms, double *bytes,
                                int *calls, int cap, int *count);
/* The last sharded proof's schedule on this (local rank 0) prover, as JSON: the order in which the library started
 * exchanges, waited for them and ran the compute segments between (each segment's measured ms, and whether only the
 * lead rank ran it), for tools/shard_model.py.  *len = bytes needed (with the NUL); ZK_ERR_BUFFER_TOO_SMALL when
 * cap is short.  In the measurement mode (zk_comm_set_measure) the segments are the serialised ranks' compute. */
int zk_prover_shard_schedule(zk_prover *p, char *buf, size_t cap, size_t *len);
/* The host-to-device trace traffic of the last proof from host columns (zk_prove / zk_prove_columns): bytes copied,
 * the columns taken as sparse (zero but the last row: their last value only), and the columns uploaded packed as 8-
 * or 32-bit integers (narrow; each value checked on the host first).  Bit c = trace column c.  Every proof starts a
 * new record, so after a proof of a device-resident trace (zk_prove_device, zk_vm_prove) all four read zero. */
int zk_prover_upload_stats(zk_prover *p, uint64_t *bytes, uint32_t *sparse_cols, uint32_t *narrow8_cols,
                           uint32_t *narrow32_cols);
/* the columns of the last host-column proof that were derived from the AIR instead of uploaded and transformed: bit 0,
 * the clock (rows 0 .. n-2 of any accepted trace hold 0 .. n-2: air/src/constrains.rs clock constraint and the
 * clk[0] = 0 assertion), checked against the caller's column by host threads */
int zk_prover_upload_derived(zk_prover *p, uint32_t *derived_cols);
/* the columns of the last host-column proof taken as fixed (bit c): columns 1 .. 11 (opcode bits, hash flag, sponge,
 * stack depth) depend on the program and lwe_size only, up to the random last row.  The first proof of a (trace length,
 * program hash) that runs with learned hints -- a prover's second proof of it -- snapshots their coefficients and LDE
 * (less the last row's share) on the device, 1.6 GB at 2^20, and rows 0 .. n-2 on the host; from the next proof on they
 * are neither uploaded nor transformed but formed by one streaming pass from the snapshot and the last-row values,
 * while host threads compare every row 0 .. n-2 of the caller's columns with the snapshot.  A mismatch voids the proof,
 * which is redone from every column (hint_redos), and the class is not tried again for that program.  At most two
 * snapshots per prover (zk_proof_info::fixed_sets), least recently used evicted.  Columns hinted sparse keep that
 * class.  A fixed column that is also narrow stays listed in narrow8_cols / narrow32_cols of zk_prover_upload_stats;
 * its bytes are not counted: `bytes` is what crossed the link.  ZK_FIXED=0 in the environment turns the class off. */
int zk_prover_upload_fixed(zk_prover *p, uint32_t *fixed_cols);
/* the columns of the last proof (bit c) whose interpolation coefficients were never written: once a host-column proof
 * forms columns from a snapshot, the derived clock, the fixed columns and the hinted sparse columns are each
 * base_c + w_c e_(n-1) (e_(n-1): the Lagrange interpolant of the last row), and the stages that are linear in the trace
 * polynomials -- the boundary quotient, the out-of-domain frame, the DEEP combination -- read base_c and e_(n-1) where
 * they already lie and fold the scalars w_c in.  Same proof bytes.  ZK_COEFF_SRC=0 in the environment writes them. */
int zk_prover_coeff_sources(zk_prover *p, uint32_t *cols);
/* How a host-resident trace goes up (zk_prove / zk_prove_columns).  ZK_SCHED_AUTO (the default): the latency schedule
 * for a proof that starts with no other proof in flight on its device, else the throughput schedule.
 * ZK_SCHED_THROUGHPUT: the narrow (packed) columns in two parts through the copy engine between 64-MB column groups.
 * ZK_SCHED_LATENCY: the first two column groups start crossing at once and the packed narrow columns are expanded by a
 * kernel reading the pinned bytes, in small parts, so the first kernels start ~0.2 ms into the call.  Same proof bytes.
 * (No reference counterpart: winterfell's prover has no upload; a tuning knob for servers.) */
enum { ZK_SCHED_AUTO = 0, ZK_SCHED_THROUGHPUT = 1, ZK_SCHED_LATENCY = 2 };
int zk_prover_set_upload_schedule(zk_prover *p, int schedule);
/* What the last proof on this prover did.  schedule: the upload schedule the last host-column proof ran
 * (ZK_SCHED_THROUGHPUT or ZK_SCHED_LATENCY; 0 after a device-trace proof).  The AUTO rule, as a contract: a proof takes
 * the latency schedule iff no other proof -- single-GPU or a rank of a sharded proof -- is in flight on its device
 * when it starts (a proof counts as in flight from entry until its uploads and kernels have drained).
 * hint_redos: proofs this prover voided and redid because a column hint was refuted (cumulative).  hint_sets: the
 * (trace length, program hash) column-hint sets it holds (at most 8, least recently used evicted).  hinted_sparse /
 * derived: the sparse columns (bit c) and derived columns (bit 0, the clock) the last proof took from its hints.
 * fixed_sets: the fixed-column snapshots it holds (zk_prover_upload_fixed; at most 2).  After a sharded host-trace
 * proof hinted_sparse / derived are what it took from the hint set the ranks agreed on (zero without one), and
 * hint_redos counts the sharded proofs redone as well. */
typedef struct {
    int32_t schedule;
    uint32_t hint_redos;
    uint32_t hint_sets;
    uint32_t hinted_sparse;
    uint32_t derived;
    uint32_t fixed_sets;
} zk_proof_info;
int zk_prover_proof_info(const zk_prover *p, zk_proof_info *out);

/* ---- verifier: winterfell::verify::<ProcessorAir, Blake3_256, DefaultRandomCoin> (vm/src/lib.rs:93-98)
 * for the proof layout above, on the host (no GPU needed).  min_security: conjectured bits required
 * (the reference's test asks 95 for its options).  Returns ZK_OK, or ZK_ERR_VERIFY with the reason in
 * msg. */
int zk_verify(const uint8_t *proof, size_t proof_len, const zk_pub_inputs *pub, uint32_t min_security, char *msg,
              size_t msg_cap);

/* ---- per-stage timing of the last proof (ms), for benchmarks ---- */
int zk_prover_stage_times(zk_prover *p, const char **names, float *ms, int cap, int *count);
/* per-kernel device time (HIP events on the prover's stream) and algorithmic HBM bytes accumulated
 * since the last reset; enabled by zk_prover_profile(p, 1).  Passing all-NULL arrays resets. */
int zk_prover_profile(zk_prover *p, int enable);
int zk_prover_kernel_stats(zk_prover *p, const char **names, float *total_ms, int *launches, double *total_bytes,
                           int cap, int *count);
/* the same kernels (same order) with their algorithmic f128 multiplies and additions/subtractions
 * (0 where a kernel's operation count is not modelled; the NTT passes are) */
int zk_prover_kernel_ops(zk_prover *p, double *total_muls, double *total_addsubs, int cap, int *count);

/* ---- VM trace generator (harness; vm::Processor::run + trace, vm/src/processor/mod.rs:61-95) ----
 * source: assembly text (Program::compile); public: u8 inputs; secret: ciphertexts of lwe_size
 * elements; last_row: the 28 values the reference draws from thread_rng().  trace_out receives
 * 28 x n column-major with n <= cap_rows; outputs = 16 stack values; hash = program hash.
 * trace_out = NULL is a size query: *n_out is set from the compiled program alone (the VM does not
 * run) and ZK_ERR_BUFFER_TOO_SMALL is returned. */
int zk_vm_trace(const char *source, const uint8_t *public_in, size_t num_public, const uint8_t *secret,
                size_t num_secret, uint32_t lwe_size, uint32_t delta, const uint8_t *last_row, uint8_t *trace_out,
                size_t cap_rows, size_t *n_out, uint8_t *outputs, uint8_t *program_hash);
/* The same in the reference's two steps.  zk_program_compile = Program::compile (vm/src/program/mod.rs:37-131):
 * parse, pad, hash; the handle keeps the chiplet's per-step sponge states the hash computation produced (they
 * depend on the code alone).  zk_program_trace = Processor::run + trace (vm/src/processor/mod.rs:61-95) of that
 * program on these inputs: the stack machine runs once sequentially (errors, chunk states), then threads
 * (ZK_VM_THREADS, else OMP_NUM_THREADS, else all cores) write the rows.  trace_out = NULL runs the program and
 * reports n (ZK_ERR_BUFFER_TOO_SMALL).  A compiled program may be traced from several threads at once. */
typedef struct zk_program zk_program;
int zk_program_compile(const char *source, zk_program **out, uint8_t *program_hash, size_t *trace_len);
int zk_program_trace(const zk_program *prog, const uint8_t *public_in, size_t num_public, const uint8_t *secret,
                     size_t num_secret, uint32_t lwe_size, uint32_t delta, const uint8_t *last_row,
                     uint8_t *trace_out, size_t cap_rows, size_t *n_out, uint8_t *outputs);
void zk_program_free(zk_program *prog);
const char *zk_vm_last_error(void);

/* ---- vm::prove (vm/src/lib.rs:13-29) with the trace written on the GPU ----
 * zk_vm_trace_device = Processor::run + output + trace (vm/src/processor/mod.rs:61-101) into the prover's own trace
 * buffer (zk_prover_trace_buffer, 28 x n column-major): the host runs the stack machine once (every error the
 * reference raises, with its status and text in zk_vm_last_error / zk_last_error; the 16 outputs) and uploads its
 * state every 64 rows plus the inputs (~6 MB at 2^20 instead of the 448 MiB trace); kernels replay the machine and
 * write the rows.  lwe_size must be in [1, 5] (the AIR's range).  last_row: the 28 values Processor::trace draws from
 * thread_rng() (mod.rs:86-92), or NULL to draw them here (uniform nonzero field elements).  Returns once the trace is
 * in HBM.  Works on every prover, a rank of a sharded proof included (then zk_prove_sharded with trace = NULL). */
int zk_vm_trace_device(zk_prover *p, zk_program *prog, const uint8_t *public_in, size_t num_public,
                       const uint8_t *secret, size_t num_secret, uint32_t lwe_size, uint32_t delta,
                       const uint8_t *last_row, size_t *n_out, uint8_t *outputs);
/* The whole of vm::prove on one GPU: the device trace above, then ExecutionProver::new(options, program hash,
 * outputs, server key) + prove (vm/src/lib.rs:20-26) on it -- the same proof bytes as zk_prove of the host VM's trace.
 * outputs (16 x 16 B) and program_hash (2 x 16 B) are optional outputs (the reference returns (hash, output, proof)). */
int zk_vm_prove(zk_prover *p, zk_program *prog, const uint8_t *public_in, size_t num_public, const uint8_t *secret,
                size_t num_secret, uint32_t lwe_size, uint32_t delta, const uint8_t *last_row, const zk_options *opt,
                uint8_t *proof_out, size_t *proof_len, uint8_t *outputs, uint8_t *program_hash);
/* vm::prove as ONE proof sharded over the ranks of `comm`: every local rank writes the trace into its
 * own HBM (zk_vm_trace_device: the host stack pass is repeated per process, no trace crosses PCIe or xGMI), then
 * zk_prove_sharded over the device traces.  last_row is REQUIRED (every rank must write the same trace; the caller
 * draws it once and broadcasts it).  The same proof bytes as zk_vm_prove / zk_prove of that trace, on every rank. */
int zk_vm_prove_sharded(zk_comm *comm, zk_prover **provers, int nlocal, zk_program *prog, const uint8_t *public_in,
                        size_t num_public, const uint8_t *secret, size_t num_secret, uint32_t lwe_size, uint32_t delta,
                        const uint8_t *last_row, const zk_options *opt, uint8_t *proof_out, size_t *proof_len,
                        uint8_t *outputs, uint8_t *program_hash);

/* ---- proof queue: one host thread keeps several proofs in flight (no reference counterpart: vm::prove,
 * vm/src/lib.rs:13-29, is one thread that proves one program and then takes the next) ----
 * Every zk_prove* / zk_vm_prove call blocks its caller, and a device gives its best throughput with three provers at
 * work.  A zk_queue owns `provers` (1 .. 8; 3 is the recommendation: P + 1 = 4 streams fit
 * HIP's default hardware queues) full provers of one device, taken with zk_prover_acquire and handed back with
 * zk_prover_release at destroy, and one worker thread bound to each for the queue's lifetime (which keeps the worker's
 * thread-local tables warm).  A job is one blocking call -- zk_prove_columns, zk_prove_device or zk_vm_prove -- run by a
 * worker on its prover: the same code path, the same proof bytes.  (The section stands at the end of the header, not
 * after the prover pool, because zk_job_result holds a zk_proof_info and zk_queue_submit_vm takes a zk_program.)
 * Jobs and provers.  Jobs start in submission order.  Among the idle provers a job takes the one whose last job had
 * the same (trace length, program hash) -- column hints and fixed-column snapshots are kept per prover and per such
 * key -- else the idle prover used least recently.  Queued jobs and idle provers are matched in one step, so resuming
 * a paused queue that holds k <= P jobs marks k jobs running before any of them completes.
 * Copied at submit: the 28 column pointers, *opt, *pub, the public and secret inputs and last_row.  What must stay
 * valid until the job is done: the column data, d_trace, the program handle and the output buffers (proof_out, outputs,
 * program_hash); after that the trace is not read, as with zk_prove.
 * Argument checks.  Submit runs the blocking call's argument checks against the queue's sizes (null pointers, and for
 * column and device jobs the trace length, options and lwe_size checks of zk_prove) and returns their code with their
 * zk_last_error() text at once; no job is created.  zk_vm_prove's remaining checks are part of the VM run (the
 * program's length against the prover, the input counts), so for a VM job only the null pointers are checked at submit.
 * Everything that can only fail later arrives in the job's status and message: ZK_ERR_BUFFER_TOO_SMALL (proof_len then
 * holds the needed size), ZK_ERR_TRACE, ZK_ERR_DEGREES, ZK_ERR_DEGREE, the VM's errors, device errors.
 * Delivery.  zk_queue_wait and zk_queue_wait_any return ZK_OK once they have delivered a result, whatever the job's
 * status, and set the caller's zk_last_error() to the job's message.  Each job is delivered exactly once; after that
 * its id is unknown (ZK_ERR_INVALID_ARG); ids are never reused.  zk_queue_wait_any delivers jobs in the order they
 * finished and returns ZK_ERR_INVALID_ARG when nothing is pending or undelivered.  zk_queue_poll is zk_queue_wait that
 * returns ZK_ERR_PENDING instead of blocking.  The wait calls block on a condition variable; only the workers spin on
 * the device.  zk_queue_cancel succeeds only on a job that has not started: it is then delivered with status
 * ZK_ERR_CANCELLED, prover -1 and its buffers untouched; a running, finished or delivered job gives
 * ZK_ERR_INVALID_ARG.  zk_queue_destroy cancels the queued jobs (their buffers stay untouched), waits for the running
 * ones and drops every undelivered result.  All calls are thread-safe; destroy must be the last one.
 * The provers of a queue come from and return to the process-wide pool: blocking calls on other provers, and other
 * queues, keep working beside it.  A job is a proof like any other for the AUTO upload schedule, so a job that starts
 * on an idle device takes the latency schedule.  One device per queue: a queue does not span devices, and sharded
 * proofs (zk_prove_sharded) are not queue jobs. */
typedef struct zk_queue zk_queue;
typedef struct {
    int32_t status;            /* what the blocking call would have returned; ZK_ERR_CANCELLED */
    int32_t prover;            /* index 0 .. P-1 of the prover that ran it, -1 if none */
    uint64_t proof_len;        /* bytes written; the needed size with ZK_ERR_BUFFER_TOO_SMALL */
    float queued_ms, run_ms;   /* host wall time waiting for a prover / inside the call */
    uint32_t running_at_start; /* jobs already running when this one started */
    uint32_t _pad;
    zk_proof_info info;        /* zk_prover_proof_info right after the call */
    char message[512];         /* zk_last_error() of the worker thread after a failed call, truncated; else empty */
} zk_job_result;

int zk_queue_create(int device, size_t max_trace_len, uint32_t max_blowup, int provers, zk_queue **out);
void zk_queue_destroy(zk_queue *q);
/* zk_prover_set_validate / zk_prover_set_validate_degrees on every prover of the queue; refused (ZK_ERR_INVALID_ARG)
 * while a job is queued or running. */
int zk_queue_set_validate(zk_queue *q, int on);
int zk_queue_set_validate_degrees(zk_queue *q, int on);
/* pause: no job starts, running jobs finish; submit, cancel and the wait calls keep working.  resume: see above. */
int zk_queue_pause(zk_queue *q);
int zk_queue_resume(zk_queue *q);
/* proof_cap: the capacity of proof_out (the blocking calls' *proof_len on entry); *job: the job's id. */
int zk_queue_submit_columns(zk_queue *q, const uint8_t *const *columns, size_t n, const zk_options *opt,
                            const zk_pub_inputs *pub, uint8_t *proof_out, size_t proof_cap, uint64_t *job);
/* d_trace: a trace in the queue's device's HBM (any prover's zk_prover_trace_buffer, or the caller's own allocation) */
int zk_queue_submit_device(zk_queue *q, const void *d_trace, size_t n, const zk_options *opt,
                           const zk_pub_inputs *pub, uint8_t *proof_out, size_t proof_cap, uint64_t *job);
/* zk_vm_prove; last_row may be NULL (drawn by the library), outputs and program_hash are optional */
int zk_queue_submit_vm(zk_queue *q, zk_program *prog, const uint8_t *public_in, size_t num_public,
                       const uint8_t *secret, size_t num_secret, uint32_t lwe_size, uint32_t delta,
                       const uint8_t *last_row, const zk_options *opt, uint8_t *proof_out, size_t proof_cap,
                       uint8_t *outputs, uint8_t *program_hash, uint64_t *job);
int zk_queue_wait(zk_queue *q, uint64_t job, zk_job_result *res);
int zk_queue_poll(zk_queue *q, uint64_t job, zk_job_result *res);
int zk_queue_wait_any(zk_queue *q, uint64_t *job, zk_job_result *res);
int zk_queue_cancel(zk_queue *q, uint64_t job);
/* The validation / degree report of a job that has not been delivered yet (zk_prover_validation / zk_prover_degrees
 * right after its call, kept with the job).  Both block until the job has finished, as zk_queue_wait does, and deliver
 * nothing: the job is still there for a wait call.  ZK_ERR_INVALID_ARG for an unknown (or delivered) id and for a job
 * during which that check did not run (the switch was off, the job was cancelled). */
int zk_queue_job_validation(zk_queue *q, uint64_t job, zk_validation *out);
int zk_queue_job_degrees(zk_queue *q, uint64_t job, zk_degrees *out);
/* submitted: jobs accepted; completed: jobs a prover has finished (cancelled jobs are in neither `completed` nor
 * `queued`); queued / running: now; peak_running: the most jobs running at once so far.  Any pointer may be NULL. */
int zk_queue_stats(const zk_queue *q, uint64_t *submitted, uint64_t *completed, uint32_t *queued, uint32_t *running,
                   uint32_t *peak_running);

#ifdef __cplusplus
}
#endif
#endif
