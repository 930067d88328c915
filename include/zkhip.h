/* zkhip - C ABI of the MI355X (gfx950) wrapping-prover kernels.
 *
 * This is the drop-in boundary for the hot path of clearmatics/zecale:
 *   libzecale::aggregator_circuit::prove -> wsnarkT::generate_proof(pk, pb)
 *   (reference libzecale/circuits/aggregator_circuit.tcc:168; policy class wsnarkT =
 *    libzeth::groth16_snark<libff::bw6_761_pp>, aggregator_server/aggregator_server.cpp:61).
 * The reference has no FFI of its own (its seams are C++ template parameters); the
 * entry points below are what a `groth16_snark_hip<wppT>` policy class binds.
 *
 * Conventions
 *   - Field elements are little-endian arrays of 64-bit limbs in Montgomery form, radix 2^768
 *     (Fq, 12 limbs) / 2^384 (Fr, 6 limbs), fully reduced - libff's in-memory Fp_model layout.
 *   - Affine points: x then y (24 limbs).  The point at infinity is the all-zero pattern.
 *   - Jacobian points: X, Y, Z (36 limbs), infinity <=> Z = 0.  Both G1 and G2 of BW6-761 are
 *     over Fq, so every point entry point serves both groups.
 *   - All functions return ZKHIP_OK (0) or a negative error code; no exceptions cross the ABI.
 *   - Devices: zkhip_init(device) once per GPU the process uses.  Every handle (base set, proving key, constraint
 *     system, prover) remembers the GPU it was created on and every entry point binds the CALLING THREAD to that
 *     GPU first (HIP's current device is per host thread), so handles may be used from any thread.  Entry points
 *     without a handle run on the calling thread's library device: zkhip_set_device, default = the first GPU
 *     initialised.  One process can drive all GPUs of a node this way (the reference server is one process:
 *     aggregator_server/aggregator_server.cpp:390-416).
 *   - The handle-less entry points and the ones that share the library's own work space are serialised per GPU
 *     by the library; zkhip_prover / zkhip_pipeline instances run side by side.
 *   - `_dev` variants take DEVICE pointers (e.g. torch tensor data_ptr()); the others take host
 *     pointers and stage through HBM themselves.
 */
#ifndef ZKHIP_H
#define ZKHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKHIP_OK 0
#define ZKHIP_ERR_ARG (-1)        /* bad argument */
#define ZKHIP_ERR_NO_DEVICE (-2)  /* no gfx950 device / HIP runtime unavailable */
#define ZKHIP_ERR_HIP (-3)        /* a HIP call failed; see zkhip_last_error() */
#define ZKHIP_ERR_STATE (-4)      /* library not initialised / handle invalid */
#define ZKHIP_ERR_NO_TICKET (-5)  /* pipeline / dispatcher wait: this ticket was never issued or has been collected already
                                     (ZKHIP_ERR_ARG from a wait means the BATCH failed: malformed or degenerate nested proofs) */
#define ZKHIP_ERR_REFUSED (-6)    /* a checked prover refused its input; zkhip_prover_last_refusal says why */

typedef struct zkhip_bases zkhip_bases; /* opaque: a base-point set resident in HBM */

/* replaces: libff::bw6_761_pp::init_public_params() + device selection
 * (aggregator_server/aggregator_server.cpp:476-477) */
int zkhip_init(int device);
/* library device of the calling thread for the entry points that take no handle (the device must be initialised) */
int zkhip_set_device(int device);
int zkhip_get_device(void);              /* -1 before the first zkhip_init */
int zkhip_device_count(void);            /* GPUs visible to the process (0 without a HIP runtime) */
int zkhip_device_memory(size_t* free_bytes, size_t* total_bytes);  /* of the calling thread's library device, now (either may be null) */
void zkhip_shutdown(void);
const char* zkhip_strerror(int code);
const char* zkhip_last_error(void);

/* Options of a base set / proving key.  They are resolved ONCE, when the key is uploaded, and travel with the handle: two threads
 * (or two GPUs) loading keys with different options do not see each other's choice.  A field left at its "default" value takes
 * the process-wide default, i.e. what the deprecated zkhip_set_* switches below last set. */
typedef struct {
  int precompute;   /* -1: default (on);  0: plain base sets;  1: window tables (2^(c w) P_i for every window position) */
  int table_naf;    /* -1: default (off, or ZKHIP_TABLE_NAF);  0: one table level per window;  1: EVERY bit position + scalars in
                       non-adjacent form (378 levels: within ZKHIP_NAF_TABLE_GB, default 48 GB per key, else one level per window) */
  int window;       /*  0: automatic from the length;  else the window c of the table, in [4, 22] */
  int batch_msms;   /* -1: default (on);  0: one launch sequence per MSM;  1: the five MSMs of a proof in one launch sequence */
  int table_model;  /*  0: default, XYZZ;  1: the key's four G1 query vectors (A, B-G1, H, L) also get their tables in precomputed form
                       on G1's 2-isogenous twisted Edwards curve (1.5 x the tables' memory on top), and the G1 MSMs of a proof add in
                       that model: with batch_msms all four in ONE launch sequence, B-G2 (no such curve: XYZZ) in a second one beside
                       it.  Proofs are identical.  The LAST field, 0 its default: ZKHIP_KEY_OPTS_DEFAULT and every initialiser of the
                       four fields above leave it 0.  Rules (any other value, or a rule broken: ZKHIP_ERR_ARG at upload):
                         - needs tables: with precompute = 0 (given, or the resolved process-wide default) it is an error;
                         - Edwards tables have one level per window: with table_naf = 1 it is an error; with table_naf = -1 the key
                           gets one level per window whatever the process-wide default (zkhip_set_table_naf, ZKHIP_TABLE_NAF) says;
                         - the key is on the Edwards model only if ALL four G1 vectors got their Edwards form: a point that is not
                           of order r, or the memory guard of zkhip_set_table_model, leaves an ordinary XYZZ key (the forms already
                           built are freed) and the upload succeeds: zkhip_crs_table_model tells.  The XYZZ tables always stay. */
} zkhip_key_opts;
#define ZKHIP_KEY_OPTS_DEFAULT {-1, -1, 0, -1}

/* DEPRECATED process-wide switches (kept for callers of rounds 1-2): they set the DEFAULTS that zkhip_key_opts falls back to.
 * Window size (bits) of the bucket method; 0 = automatic from len. */
int zkhip_set_msm_window(int c);
/* Bucket accumulation: number of batched-affine levels (pairwise sums inside the buckets, one shared inversion per lane) that
 * run before the XYZZ accumulation; -1 = automatic (currently NONE at every size: measured slower on gfx950).  A
 * measurement / test knob, process-wide, read when an MSM plan is made.  Results do not depend on it. */
int zkhip_set_affine_levels(int levels);

/* replaces: holding r1cs_gg_ppzksnark_proving_key query vectors in host memory
 * (aggregator_server/aggregator_server.cpp:483-514 loads the keypair once).
 * Copies `len` affine points (len x 24 limbs) into HBM in the kernels' packed layout. */
int zkhip_bases_upload(const uint64_t* bases_affine, size_t len, zkhip_bases** out);
int zkhip_bases_upload_dev(const void* d_bases_affine, size_t len, zkhip_bases** out);
size_t zkhip_bases_len(const zkhip_bases* b);
void zkhip_bases_free(zkhip_bases* b);
/* Window table for a resident base set (a proving key stays in HBM for the life of the server, the reference keeps it
 * in RAM: aggregator_server.cpp:483-514): stores 2^(c w) P_i for every window position w, so that all digit positions
 * of a scalar share one bucket window.  Costs ceil(378/c) x the memory of the base set, once; results of zkhip_msm are
 * unchanged (same group element).  c = 0 chooses the window from the length.  zkhip_crs_upload builds the tables of a
 * key by default; zkhip_set_crs_precompute(0) turns that off. */
int zkhip_bases_precompute(zkhip_bases* b, int c);
/* the same with the kind of table as an argument (zkhip_key_opts.table_naf: -1 default, 0 one level per window, 1 every bit position) */
int zkhip_bases_precompute_ex(zkhip_bases* b, int c, int table_naf);
int zkhip_bases_table_window(const zkhip_bases* b);      /* 0: no table */
/* plain base set (no table): the window c of the bucket method for the MSMs over THIS set, 0 = by the number of terms (default),
 * else 4 .. 18.  An option of the handle, like zkhip_key_opts of a key (the process-wide zkhip_set_msm_window is deprecated). */
int zkhip_bases_set_window(zkhip_bases* b, int c);
int zkhip_set_crs_precompute(int on);
/* on = 1: window tables built from now on hold EVERY bit position (378 levels, sixteen times the memory) and scalars are recoded in
   non-adjacent form: an eighth fewer point additions per scalar, but measured slower once the tables outgrow the TLB (DESIGN.md
   section 5) - off by default; 0: one level per window; -1: the environment's ZKHIP_TABLE_NAF decides.  Results are identical. */
int zkhip_set_table_naf(int on);
/* model = 1 (default): the window tables of G1 base sets built from now on by zkhip_bases_precompute[_ex] (one level per window) get a
   second, precomputed form on G1's 2-isogenous twisted Edwards curve, and single MSMs over such a set add in that model (fewer field
   products per addition); 0: XYZZ only; -1: the environment's ZKHIP_TABLE_MODEL (xyzz | edwards) decides.
   The Edwards form needs every base to be a point of ORDER r on G1's curve; building it checks that (2 [1/2 mod r] P = P), and a set
   that fails (a G2 set, points outside the subgroup) stays XYZZ, as does a set whose Edwards form (1.5 x the table's memory) would
   leave less than a quarter of the device's memory free.  Results are identical. */
int zkhip_set_table_model(int model);
/* 1: single MSMs over this set accumulate in the Edwards model, 0: XYZZ */
int zkhip_bases_table_model(const zkhip_bases* b);
/* Table-backed keys of up to 2^20 points per query vector: the five MSMs of a proof go through one launch sequence
 * (default on; off = one launch sequence per MSM, 2 or 5 of them in flight).  A tuning / comparison switch. */
int zkhip_set_batch_msms(int on);

/* replaces: libff::multi_exp<G, Fr, multi_exp_method_BDLO12>(bases, scalars, chunks)
 * as called five times by r1cs_gg_ppzksnark_prover (reached from aggregator_circuit.tcc:168).
 * result = sum_{i<len} scalars[i] * bases[offset + i].
 * scalars: len x 6 limbs, Montgomery form (scalars_montgomery = 1) or canonical integers (0). */
int zkhip_msm(const zkhip_bases* bases, size_t offset, const uint64_t* scalars, size_t len, int scalars_montgomery,
              uint64_t out_jac[36]);
int zkhip_msm_dev(const zkhip_bases* bases, size_t offset, const void* d_scalars, size_t len, int scalars_montgomery,
                  uint64_t out_jac[36]);
/* Device pointers handed to *_dev / submit entry points must hold complete data: the library runs on its own non-blocking
 * streams, which are not ordered against the caller's streams (synchronise the producing stream first). */
/* Device memory for host code that has no HIP runtime of its own (the *_dev entry points take device pointers). */
int zkhip_device_alloc(size_t bytes, void** out);
int zkhip_device_free(void* p);
int zkhip_device_copy_in(void* dst, const void* src, size_t bytes);
int zkhip_device_copy_out(void* dst_host, const void* src_device, size_t bytes);

/* Asynchronous form of zkhip_msm_dev for a stream of MSMs on resident bases: submit enqueues the MSM on one of EIGHT
 * slots (0 .. 7) and returns, collect waits for it.  d_scalars must stay valid until collect.  With several slots in flight the
 * sort, the stitching and the latency-bound bucket reduction of one MSM run under the accumulation of another (measured at
 * 2^20 terms: 75 / 77 / 80 Mscalar/s with 2 / 3 / 4 in flight); each slot holds its own work space (1.3 GB at 2^20 terms). */
int zkhip_msm_submit(const zkhip_bases* bases, size_t offset, const void* d_scalars, size_t len, int scalars_montgomery, int slot);
int zkhip_msm_collect(int slot, uint64_t out_jac[36]);
/* The same stream of MSMs behind a HANDLE (the slot numbers above are process-wide: two threads streaming on one GPU collide).
 * A zkhip_msm_stream owns `depth` (1 .. 16) MSM contexts - streams and work space, like a zkhip_prover - on the GPU of its base
 * set; any number of streams run side by side.  submit enqueues on a free context and returns a ticket (ZKHIP_ERR_STATE when all
 * `depth` are in flight); collect waits for that ticket (0 = the oldest in flight).  replaces: one libff::multi_exp call
 * (reached from aggregator_circuit.tcc:168) per ticket.  d_scalars must stay valid until its ticket is collected.
 * submit_host takes HOST scalars (as libff holds them): one asynchronous copy in front of the MSM's kernels on the context's own
 * stream - truly asynchronous from pinned memory (zkhip_host_alloc), staged by the runtime from pageable memory - so the 48 MB
 * uploads of the MSMs in flight travel under their kernels. */
typedef struct zkhip_msm_stream zkhip_msm_stream;
int zkhip_msm_stream_new(const zkhip_bases* bases, int depth, zkhip_msm_stream** out);     /* bases must outlive the stream */
int zkhip_msm_stream_submit(zkhip_msm_stream* st, size_t offset, const void* d_scalars, size_t len, int scalars_montgomery, uint64_t* ticket);
int zkhip_msm_stream_submit_host(zkhip_msm_stream* st, size_t offset, const uint64_t* scalars, size_t len, int scalars_montgomery, uint64_t* ticket);
int zkhip_msm_stream_collect(zkhip_msm_stream* st, uint64_t ticket, uint64_t out_jac[36]);
float zkhip_msm_stream_last_accumulate_ms(zkhip_msm_stream* st);               /* of the MSM collected last */
int zkhip_msm_stream_last_accumulate_interval(zkhip_msm_stream* st, float out_ms[2]);
void zkhip_msm_stream_free(zkhip_msm_stream* st);                              /* waits for what is still in flight */
/* pinned host memory for callers without a HIP runtime of their own (the source of submit_host's asynchronous copies) */
int zkhip_host_alloc(size_t bytes, void** out);
int zkhip_host_free(void* p);
/* one-shot form (BASELINE config 2): host bases + host scalars */
int zkhip_msm_raw(const uint64_t* bases_affine, const uint64_t* scalars, size_t len, int scalars_montgomery,
                  uint64_t out_jac[36]);

/* replaces: the fixed-base batch exponentiations of r1cs_gg_ppzksnark_generator, reached from
 * aggregator_circuit::generate_trusted_setup (libzecale/circuits/aggregator_circuit.tcc:100-109).
 * out[i] = scalars[i] * base, affine (len x 24 limbs).  base: one affine point (host memory).
 * The _dev form reads scalars from and writes points to DEVICE memory. */
int zkhip_fixed_base_mul(const uint64_t base_affine[24], const uint64_t* scalars, size_t len, int scalars_montgomery,
                         uint64_t* out_affine);
int zkhip_fixed_base_mul_dev(const uint64_t base_affine[24], const void* d_scalars, size_t len, int scalars_montgomery,
                             void* d_out_affine);

/* replaces: libfqfft::basic_radix2_domain<Fr>::FFT / iFFT / cosetFFT / icosetFFT as used by
 * r1cs_to_qap_witness_map (reached from aggregator_circuit.tcc:168).  In place, natural order in
 * and out, 2^log_d elements of 6 limbs (Montgomery form); domain <omega>, omega = 15^((r-1)/2^log_d),
 * coset generator g = 15.   dir: 0 = forward, 1 = inverse.   coset: 0 / 1.   log_d <= 22.
 *   forward, coset:   a_i <- a_i g^i, then FFT          inverse, coset:   iFFT, then a_i <- a_i g^-i */
int zkhip_ntt(uint64_t* data, unsigned log_d, int dir, int coset);
int zkhip_ntt_dev(void* d_data, unsigned log_d, int dir, int coset);

/* ---- R1CS, QAP witness map and the Groth16 prover ---------------------------------------- */
/* A constraint system <A_i,z> * <B_i,z> = <C_i,z>, i < n_constraints, in CSR form; z = (1, primary,
 * auxiliary) has n_vars entries.  Replaces libsnark::r1cs_constraint_system<Fr<wppT>> as returned by
 * aggregator_circuit::get_constraint_system() (libzecale/circuits/aggregator_circuit.hpp:99-101). */
typedef struct {
  size_t n_constraints, n_vars, n_primary;
  const uint32_t *a_row_ptr, *a_col; const uint64_t* a_val;   /* row_ptr: n+1, col: nnz, val: nnz x 6 limbs */
  const uint32_t *b_row_ptr, *b_col; const uint64_t* b_val;
  const uint32_t *c_row_ptr, *c_col; const uint64_t* c_val;
} zkhip_r1cs_desc;
typedef struct zkhip_r1cs zkhip_r1cs;
/* THE EVALUATION DOMAIN of the QAP (a7).  A system of n constraints and l primary inputs interpolates n + l + 1 points.
 *   - The reference reaches libsnark through libzeth's groth16_snark, whose generate_setup / generate_proof
 *     (libzecale/circuits/aggregator_circuit.tcc:108, :168) pass force_pow_2_domain = true: the domain is libfqfft's
 *     basic_radix2_domain of 2^ceil(log2(n + l + 1)) points.  That is the DEFAULT of every entry
 *     point here: the wrapping circuit (44,183 constraints + 5) lives on 65,536 points and its key's H query has 65,535 entries.
 *   - ZKHIP_DOMAIN_STEP asks for what libfqfft's get_evaluation_domain picks when NOT forced: a power of two if n + l + 1 is one,
 *     else step_radix2_domain of 2^k + 2^r points (49,152 for the wrapping circuit: a quarter fewer H terms).  An explicit option -
 *     NOT what a reference deployment uses, and unpinnable here (libfqfft and the reference's keys are absent from its tree).
 *   - Any other value must be a size one of those two rules can return (zkhip_domain_is_valid) and at least n + l + 1.
 * THE PROVING KEY IS AUTHORITATIVE: zkhip_crs_desc.domain_size says which domain a key was generated on, and every prover
 * (zkhip_groth16_prove, zkhip_prover_new[_slice], zkhip_multi_prover_new, the pipelines) works on the key's domain - a 65,536-point
 * key from a reference-style setup and a 49,152-point key from zkhip_groth16_setup_ex(.., ZKHIP_DOMAIN_STEP, ..) both prove.  A
 * zkhip_r1cs handle handed to zkhip_groth16_prove with a key of another domain is moved to it (zkhip_r1cs_set_domain; the matrices
 * stay in HBM, the domain's work buffers are rebuilt once).  A key whose domain cannot hold the system is refused (ZKHIP_ERR_ARG). */
#define ZKHIP_DOMAIN_DEFAULT ((size_t)0)       /* the reference's forced power of two */
#define ZKHIP_DOMAIN_STEP (~(size_t)0)         /* libfqfft's unforced get_evaluation_domain: a power of two or 2^k + 2^r */
int zkhip_r1cs_upload(const zkhip_r1cs_desc* d, zkhip_r1cs** out);                        /* = _ex(d, ZKHIP_DOMAIN_DEFAULT, out) */
int zkhip_r1cs_upload_ex(const zkhip_r1cs_desc* d, size_t domain_size, zkhip_r1cs** out);
int zkhip_r1cs_set_domain(zkhip_r1cs* r, size_t domain_size);   /* no proof may be in flight on the handle */
void zkhip_r1cs_free(zkhip_r1cs* r);
size_t zkhip_r1cs_domain_size(const zkhip_r1cs* r);     /* d: the points of the handle's current domain (a key's H query: d - 1) */
/* ceil(log2 d): log2 d exactly for a radix-2 domain (the default); for a step domain 2^k + 2^r it is k + 1 - use
 * zkhip_r1cs_domain_size where the number of points matters */
unsigned zkhip_r1cs_log_domain(const zkhip_r1cs* r);
/* host code, no device: the domain size for min_size = n + l + 1 points under each rule, and whether a size is a domain at all */
size_t zkhip_domain_size(size_t min_size);              /* forced power of two (the reference, the default) */
size_t zkhip_step_domain_size(size_t min_size);         /* libfqfft unforced: 2^k, or 2^k + 2^r */
int zkhip_domain_is_valid(size_t domain_size);          /* 1 / 0 */

/* replaces: protoboard::is_satisfied() under DEBUG (aggregator_circuit.tcc:159-164); *ok = 1/0 */
int zkhip_r1cs_is_satisfied(zkhip_r1cs* r, const uint64_t* z, int* ok);

/* replaces: libsnark::r1cs_to_qap_witness_map(cs, primary, auxiliary, 0, 0, 0, force_pow_2 = true) -
 * coefficients_for_H, over the handle's domain (above).  h_out: d x 6 limbs (h_{d-1} = 0). */
int zkhip_qap_h(zkhip_r1cs* r, const uint64_t* z, uint64_t* h_out);

/* The proving key (replaces r1cs_gg_ppzksnark_proving_key<bw6_761_pp> held by the server,
 * aggregator_server/aggregator_server.cpp:483-514).  All points affine, 24 limbs each.
 * Lengths: a_query, b_g2_query, b_g1_query: n_vars;  h_query: d - 1;  l_query: n_vars - n_primary - 1. */
typedef struct {
  size_t n_vars, n_primary, domain_size;
  const uint64_t *alpha_g1, *beta_g1, *beta_g2, *delta_g1, *delta_g2;
  const uint64_t *a_query, *b_g2_query, *b_g1_query, *h_query, *l_query;
} zkhip_crs_desc;
typedef struct zkhip_crs zkhip_crs;
int zkhip_crs_upload(const zkhip_crs_desc* d, zkhip_crs** out);
/* the same with the key's options as an argument (opts == NULL: all defaults) */
int zkhip_crs_upload_ex(const zkhip_crs_desc* d, const zkhip_key_opts* opts, zkhip_crs** out);
void zkhip_crs_free(zkhip_crs* c);
int zkhip_crs_table_kind(const zkhip_crs* c);            /* 0: no tables, 1: one level per window, 2: every bit position (NAF scalars) */
int zkhip_crs_table_model(const zkhip_crs* c);           /* 1: the key's G1 MSMs add on the Edwards curve (zkhip_key_opts.table_model took effect), 0: XYZZ */
/* bases of the five query vectors (A, B-G2, B-G1, H, L) that are not the point at infinity: the terms an MSM over the key can
 * actually have (a base at infinity produces no bucket entry) */
int zkhip_crs_finite_terms(const zkhip_crs* c, size_t out[5]);
int zkhip_crs_table_window(const zkhip_crs* c);          /* window of the key's tables, 0: none */
int zkhip_crs_device(const zkhip_crs* c);                /* the GPU that holds the key */

/* ---- key check: validate a proving key before it is uploaded ------------------------------------------------------------------
 * stands beside: r1cs_gg_ppzksnark_proving_key read from a file or an MPC (aggregator_server/aggregator_server.cpp:483-514); the
 * reference trusts what it loads.  zkhip_crs_upload[_ex] checks nothing either: a key with an unreduced limb, a point off its curve or
 * outside the group of order r, a G1 point in the B-G2 vector, or B-G1 / B-G2 queries that do not belong together uploads without
 * complaint and every proof made from it fails to verify later, somewhere else.  zkhip_crs_check says what is wrong and where:
 *   1. POINTS.  Every point of the key is fully reduced and either all zero (the point at infinity, which passes) or on its curve and
 *      of order r: the checks and codes of the checked verifier (ZKHIP_VERIFY_ENCODING / _OFF_CURVE / _NOT_ORDER_R, the first that
 *      applies).  beta_g2, delta_g2 and b_g2_query are checked on y^2 = x^3 + 4, everything else on y^2 = x^3 - 1.  On the device: one
 *      lane per point of a staged chunk of one element (csrc/key_check.hip k_key_point_check, the lane body of the checked verifier).
 *   2. PAIRS.  t(beta_g1, g2) t(-g1, beta_g2) == 1 and the same for delta, on the host.  For the B queries ONE random combination:
 *      S1 = sum rho_i B-G1[i], S2 = sum rho_i B-G2[i] with the SAME 128-bit scalars (two MSMs on the device), then
 *      t(S1, g2) t(-g1, S2) == 1 on the host.  A relation is only evaluated when none of its points was refused in step 1: GT has prime
 *      order r, and WHEN EVERY B POINT HAS ORDER r a pair of vectors with B-G1[i] != s_i g1 for B-G2[i] = s_i g2 passes with probability
 *      about 2^-128 over the rho_i - with a point of small order in a vector the error term can have small order and be cancelled by its
 *      scalar with noticeable probability, which is why the relation is left unevaluated then (the precondition zkhip_verifier_verify_all
 *      documents, for the same reason).  The infinity patterns of the two B vectors must agree index by index.
 *   3. STRUCTURE (only with cs).  n_vars and n_primary are the system's and domain_size is a domain that holds it (n + l + 1 points);
 *      a query base is at infinity exactly where the setup's polynomial for that variable is identically zero: A[i] iff i > n_primary
 *      and column i of A holds no non-zero coefficient (variables 0 .. n_primary carry the input-consistency rows of the QAP instance
 *      map), B-G1[i] and B-G2[i] iff column i of B holds none, L[i - n_primary - 1] iff columns i of A, B and C hold none; H and vk_abc
 *      have no base at infinity.  A host loop over column occupancy; this is the check that catches "the key of another circuit".
 * vk_abc: the (n_primary + 1) x 24 limbs of the verification key's ABC, checked as the eleventh element, or NULL.
 * rho: n_vars x 2 words (little endian, 128 bits each, none zero: ZKHIP_ERR_ARG) for tests and reproducible runs only - scalars that
 * somebody who made the key knows or can predict prove nothing -, or NULL to draw them from the OS (getrandom; ZKHIP_ERR_STATE if that
 * fails, as zkhip_verifier_verify_all).
 * Returns ZKHIP_OK whenever the check RAN: the verdict is out->ok and the report.  ZKHIP_ERR_ARG: null arguments, implausible sizes
 * (n_vars < n_primary + 1, no valid domain, a vector of 2^30 points or more).
 * zkhip_crs_check runs on the calling thread's library device (zkhip_set_device) on a stream and work space of its own.
 * zkhip_crs_check_host: the same report on the host alone (no device, no zkhip_init; the point checks on up to 16 threads, the sums by
 * host scalar multiplications): the reference the device route is pinned on. */
enum { ZKHIP_KEY_ALPHA_G1, ZKHIP_KEY_BETA_G1, ZKHIP_KEY_BETA_G2, ZKHIP_KEY_DELTA_G1, ZKHIP_KEY_DELTA_G2,
       ZKHIP_KEY_A, ZKHIP_KEY_B_G2, ZKHIP_KEY_B_G1, ZKHIP_KEY_H, ZKHIP_KEY_L, ZKHIP_KEY_VK_ABC, ZKHIP_KEY_ELEMENTS };   /* elements of a key, in report order */
typedef struct {
  size_t points, infinity;   /* points of the element; those at infinity (all zero) */
  size_t refused[3];         /* points refused as ENCODING, OFF_CURVE, NOT_ORDER_R */
  size_t first_refused;      /* the smallest refused index, (size_t)-1: none */
  int first_code;            /* its code (ZKHIP_VERIFY_*), 0: none */
} zkhip_key_element_report;
typedef struct {
  zkhip_key_element_report e[ZKHIP_KEY_ELEMENTS];
  int pairs;                  /* bit 0 beta_g1/beta_g2, bit 1 delta_g1/delta_g2, bit 2 B-G1/B-G2: set = the relation FAILS */
  int pairs_evaluated;        /* same bits: set = the relation was evaluated (it is not when one of its points was refused) */
  size_t b_infinity_mismatch; /* first i with exactly one of B-G1[i], B-G2[i] at infinity, (size_t)-1: none */
  int structure;              /* 0 fine / not asked; else the element (ZKHIP_KEY_A ..) whose length or infinity pattern disagrees with the
                                 system: a wrong n_vars is reported at ZKHIP_KEY_A, n_primary at ZKHIP_KEY_L, the domain at ZKHIP_KEY_H */
  size_t structure_first;     /* the first index that disagrees ((size_t)-1 for a length) */
  int ok;                     /* 1 iff nothing above is refused, failing, unevaluated or disagreeing */
} zkhip_key_report;
int zkhip_crs_check(const zkhip_crs_desc* key, const uint64_t* vk_abc, const zkhip_r1cs_desc* cs, const uint64_t* rho, zkhip_key_report* out);
int zkhip_crs_check_host(const zkhip_crs_desc* key, const uint64_t* vk_abc, const zkhip_r1cs_desc* cs, const uint64_t* rho, zkhip_key_report* out);

/* ---- phase-2 contributions: re-randomise delta of a key, and verify somebody else's re-randomisation ----------------------------
 * stands beside: the circuit-specific ("phase 2") round of a setup ceremony.  zkhip_groth16_setup* is a single-party setup whose caller
 * knows delta; a party who RECEIVES a key can add its own randomness with zkhip_keypair_contribute, and whoever coordinates checks that
 * turn with zkhip_phase2_verify.  As long as ONE contributor of the chain discards its s, nobody knows delta.
 * SCOPE.  Phase 2 re-randomises delta ONLY.  A key is sound only if tau, alpha and beta are unknown as well: that takes a
 * powers-of-tau ceremony and the linear-combination step that turns its output into this circuit's queries, neither of which this
 * library has.  A key from zkhip_groth16_setup* with contributions on top still has a tau, alpha and beta that the first party knew.
 * THE MATHS (Groth16 without gamma, as zkhip_groth16_setup builds it): H_j = tau^j Z(tau) / delta g1 and
 * L_i = (beta A_i + alpha B_i + C_i)(tau) / delta g1.  A contribution with the secret s in [1, r) gives
 *   delta_g1' = s delta_g1, delta_g2' = s delta_g2, H'_j = s^-1 H_j, L'_i = s^-1 L_i (a base at infinity stays there);
 * everything else, the verification key's ABC included, is unchanged: the new verification key differs in delta_g2 only, and
 * setup(tau, alpha, beta, delta s) equals contribute(setup(tau, alpha, beta, delta), s) limb for limb.
 * On the device the 2 x up to 2^22 multiplications by the ONE scalar s^-1 run one lane per point of a staged chunk, every lane on the
 * same recoded digits (csrc/phase2.hip k_common_scalar_mul: s^-1 = k1 + k2 lambda along G1's endomorphism, half the doublings); the
 * digits, and the call's own copies of s, k and s^-1, are cleared on the device and the host before the call returns.
 * A contribution before -> after with its record is ACCEPTED iff all five hold:
 *   1. UNCHANGED.  n_vars, n_primary, domain_size, alpha_g1, beta_g1, beta_g2, a_query, b_g2_query, b_g1_query are byte-identical (and
 *      the record's delta_g1 / delta_g2 are the new key's).
 *   2. POINTS.  delta_g1', delta_g2', every H'_j, every L'_i and the record's commitment T pass the checks of zkhip_crs_check (same
 *      codes); delta' or T at infinity is refused; the infinity pattern of H' and L' equals that of H and L index by index.
 *   3. DELTA PAIR.  t(delta_g1', g2) t(-g1, delta_g2') == 1.
 *   4. RATIO.  With 128-bit non-zero rho over the concatenation H | L, the same scalars on both keys, S = sum rho_i (H | L)_i and
 *      S' = sum rho_i (H' | L')_i: t(S', delta_g2') t(-S, delta_g2) == 1.  Evaluated ONLY when step 2 refused nothing - the rule of
 *      zkhip_crs_check and zkhip_verifier_verify_all, for the same reason: with a point of small order among the summands the error
 *      term can have small order and be cancelled by its scalar with noticeable probability.
 *   5. PROOF OF KNOWLEDGE of s (Schnorr on the base delta_g1, Fiat-Shamir).  T = k delta_g1; c = the first 16 bytes, little endian, of
 *      SHA-256("zkhip phase2 pok v1" | prev_digest | delta_g1 | delta_g1' | T); z = k + c s mod r, canonical (NOT Montgomery) and
 *      below r; the check is [z] delta_g1 == T + [c] delta_g1'.  Points are hashed as their 24 ABI limbs, little endian.
 * The transcript link: new_digest = SHA-256("zkhip phase2 link v1" | prev_digest | the record's 624 bytes).
 * PRECONDITION: `before` is a key that zkhip_crs_check, or an earlier accepted contribution, has validated; its points are not checked
 * again (and the multiplication kernel assumes points of order r).
 * s, k: six limbs in Montgomery form, non-zero and below r (ZKHIP_ERR_ARG otherwise), or NULL to draw them from the OS (getrandom;
 * ZKHIP_ERR_STATE if that fails: there is no weaker generator behind it).  Passing them is for tests: whoever knows s knows the
 * contribution's share of delta.  rho: ((domain_size - 1) + (n_vars - n_primary - 1)) x 2 words, none zero (ZKHIP_ERR_ARG), for
 * tests and reproducible runs only - scalars that the contributor knows or can predict prove nothing -, or NULL to draw them.
 * zkhip_keypair_contribute: *after is a new keypair (zkhip_keypair_free; _vk carries the new delta_g2, _write / _read work on it).
 * zkhip_phase2_verify returns ZKHIP_OK whenever it RAN: the verdict is out->ok; new_digest is written only when ok.  Keys whose sizes
 * differ are a report (changed bit 31, nothing else evaluated), not an error.  The device route checks the points with
 * k_key_point_check and sums with the MSM engine; pairings and the proof of knowledge run on the host.
 * The _host forms: the same results on the host alone (no device, no zkhip_init, up to 16 threads): what the device route is pinned on. */
typedef struct zkhip_keypair zkhip_keypair;      /* zkhip_groth16_setup, zkhip_keypair_read (below) */
typedef struct { uint64_t delta_g1[24], delta_g2[24], pok_commit[24], pok_response[6]; } zkhip_phase2_contribution;
typedef struct {
  int changed;                 /* bit per element of step 1 that differs (ZKHIP_KEY_* numbering; the DELTA bits: the record's delta is not the
                                  new key's), sizes: bit 31 */
  zkhip_key_element_report delta_g1, delta_g2, h, l, pok_commit;   /* the NEW points; first_refused / first_code as in the key check */
  int infinity_mismatch;       /* 0, or ZKHIP_KEY_H / ZKHIP_KEY_L */
  size_t infinity_mismatch_first;   /* its first index, (size_t)-1: none */
  int relations, relations_evaluated;   /* bit 0 delta pair, bit 1 ratio, bit 2 proof of knowledge: set = FAILS / was evaluated */
  int ok;
} zkhip_phase2_report;
int zkhip_keypair_contribute(const zkhip_keypair* before, const uint64_t s[6], const uint64_t k[6], const uint8_t prev_digest[32],
                             zkhip_keypair** after, zkhip_phase2_contribution* rec, uint8_t new_digest[32]);
int zkhip_keypair_contribute_host(const zkhip_keypair* before, const uint64_t s[6], const uint64_t k[6], const uint8_t prev_digest[32],
                                  zkhip_keypair** after, zkhip_phase2_contribution* rec, uint8_t new_digest[32]);
int zkhip_phase2_verify(const zkhip_crs_desc* before, const zkhip_crs_desc* after, const zkhip_phase2_contribution* rec,
                        const uint8_t prev_digest[32], const uint64_t* rho, zkhip_phase2_report* out, uint8_t new_digest[32]);
int zkhip_phase2_verify_host(const zkhip_crs_desc* before, const zkhip_crs_desc* after, const zkhip_phase2_contribution* rec,
                             const uint8_t prev_digest[32], const uint64_t* rho, zkhip_phase2_report* out, uint8_t new_digest[32]);

/* replaces: wsnarkT::generate_proof(pk, pb) = libsnark::r1cs_gg_ppzksnark_prover (called at
 * libzecale/circuits/aggregator_circuit.tcc:168), with the randomisers (r, s) injected so that
 * results can be compared bit for bit.  z: n_vars x 6 limbs.  proof_affine: A (G1), B (G2), C (G1). */
int zkhip_groth16_prove(const zkhip_crs* crs, zkhip_r1cs* r1cs, const uint64_t* z, const uint64_t r[6], const uint64_t s[6],
                        uint64_t proof_affine[72]);
/* Multi-GPU form (the proving key is partitioned across the GPUs of a node, one process per GPU):
 *   zkhip_crs_upload_slice   uploads this rank's slice of every query vector: [a_lo, a_lo+a_len) of the A / B queries,
 *                            [h_lo, ..) of H, [l_lo, ..) of L (full-key descriptor + ranges)
 *   zkhip_groth16_prove_partial  QAP map (replicated) + the five MSMs over the slice -> 5 Jacobian partial sums
 *                            (A, B-G2, B-G1, H, L: 5 x 36 limbs)
 *   ... the ranks exchange and add the partial sums (RCCL all-gather of 1440 bytes, zecale_amd/dist.py) ...
 *   zkhip_groth16_finish     host tail on the summed values.
 * zkhip_groth16_prove is exactly prove_partial over the whole key followed by finish. */
int zkhip_crs_upload_slice(const zkhip_crs_desc* full_key, size_t a_lo, size_t a_len, size_t h_lo, size_t h_len, size_t l_lo, size_t l_len,
                           zkhip_crs** out);
int zkhip_crs_upload_slice_ex(const zkhip_crs_desc* full_key, size_t a_lo, size_t a_len, size_t h_lo, size_t h_len, size_t l_lo, size_t l_len,
                              const zkhip_key_opts* opts, zkhip_crs** out);
int zkhip_groth16_prove_partial(const zkhip_crs* crs_slice, zkhip_r1cs* r1cs, const uint64_t* z, size_t a_lo, size_t h_lo, size_t l_lo,
                                uint64_t sums_jac[180]);
int zkhip_groth16_finish(const uint64_t alpha_g1[24], const uint64_t beta_g1[24], const uint64_t beta_g2[24], const uint64_t delta_g1[24],
                         const uint64_t delta_g2[24], const uint64_t sums_jac[180], const uint64_t r[6], const uint64_t s[6],
                         uint64_t proof_affine[72]);
/* phase timings of the last zkhip_groth16_prove, milliseconds: [0] upload z, [1] QAP (SpMV + 7 NTT),
 * [2..6] the five MSMs A, B2, B1, H, L, [7] host tail */
int zkhip_last_prove_timings(double out_ms[8]);

/* Prover instances.  The entry points above share one set of device work space and are serialised by the library;
 * a zkhip_prover owns its streams, MSM work space and QAP buffers, so several host threads (one instance each) keep
 * several proofs in flight on one GPU.  At the wrapping circuit's size (50k constraints) one proof cannot fill the
 * chip: the phases after the bucket accumulation are chains of short launches.  Same results as zkhip_groth16_prove.
 * replaces: one wsnarkT::generate_proof call (aggregator_circuit.tcc:168) per instance and call. */
typedef struct zkhip_prover zkhip_prover;
int zkhip_prover_new(const zkhip_crs* crs, const zkhip_r1cs_desc* cs, zkhip_prover** out);   /* crs must outlive the prover */
/* on != 0: this prover shares the GPU with others (a server's slots): the latency-bound launches of the bucket reduction then use
   one lane per point addition instead of four - less total work, a longer single proof -, slices of the bucket accumulation are twice
   as long, and from its second proof on the instance enqueues the upload of the assignment and the QAP map on the stream of its MSM
   launch sequence: the calling thread waits once, for the MSM results (zkhip_prover_timings then reports enqueueing times for the
   first two phases; ZKHIP_STREAM_CHAIN=0 in the environment keeps the waits).  The streaming pipeline sets it on its provers. */
int zkhip_prover_set_streaming(zkhip_prover* p, int on);
/* no counterpart: for a caller that owns SEVERAL instances which will prove at the same time (the streaming prover does this itself).
 * The runtime spreads streams over its hardware queues in creation order and kernels of streams that share a queue do not overlap; an
 * instance in streaming mode keeps one of its three streams busy.  Call with which = 0 for every instance (the busy streams: spread
 * evenly), then with which = 1 for every instance (the idle ones), before the first proof; without it the streams are created by the
 * first proofs, in whatever order the provers' threads arrive.  Either call creates only what the instance does not have yet, and
 * the instance keeps its streams until it is freed. */
int zkhip_prover_create_streams(zkhip_prover* p, int which);
int zkhip_prover_prove(zkhip_prover* p, const uint64_t* z, const uint64_t r[6], const uint64_t s[6], uint64_t proof_affine[72]);
/* the same with the assignment already in device memory (n_vars x 6 limbs, e.g. from zkhip_gpu_witness_run; must be complete) */
int zkhip_prover_prove_dev(zkhip_prover* p, const void* d_z, const uint64_t r[6], const uint64_t s[6], uint64_t proof_affine[72]);
/* Checked proving (stands beside: _pb.is_satisfied() under DEBUG, aggregator_circuit.tcc:159-164).  zkhip_prover_prove* turns an
 * unsatisfying or unreduced assignment into an unverifiable proof and returns ZKHIP_OK, and zkhip_prover_prove_app_dev ORs an unmasked
 * device assignment into the application's constants.  With zkhip_prover_set_checked(p, 1) the four entry points zkhip_prover_prove,
 * _prove_dev, _prove_app and _prove_app_dev write NO proof for such input and return ZKHIP_ERR_REFUSED; zkhip_prover_last_refusal gives
 * the kind and the index.  If several kinds apply the smallest kind is reported, and the smallest index of that kind.  For acceptable
 * input the proof is limb-identical to the unchecked prover's.
 * The flags are written by checking variants of the kernels that touch the data anyway - the conversion of the assignment compares the
 * raw limbs with r, entry 0 with ONE and, for prove_app[_dev], the two operands of the merge; a first-failing-row form of the
 * satisfiability check reads <A,z>, <B,z>, <C,z> where the QAP map leaves them before any transform - and they reach the host in the
 * synchronisation the proof has anyway: no additional host wait, in every strategy (one launch sequence, Edwards key, split, chained).
 * The MSMs of a refused proof run; their result is dropped.  A checked zkhip_prover_prove_app reports an unmasked HOST assignment as
 * ZKHIP_REFUSAL_APP_MASK too (unchecked: ZKHIP_ERR_ARG from the host's own look at the positions, as before).
 * Default 0: every kernel and launch sequence is the unchecked prover's.  Not for provers over a slice of the key (ZKHIP_ERR_STATE);
 * the streaming pipeline and the dispatcher generate their own assignments and have no checked form.
 * last_refusal: *kind = 0 when p's last proof was not refused. */
#define ZKHIP_REFUSAL_ENCODING 1 /* an assignment entry >= r            (index: the variable) */
#define ZKHIP_REFUSAL_ONE 2      /* z[0] is not the constant ONE */
#define ZKHIP_REFUSAL_UNSAT 3    /* <A_i,z><B_i,z> != <C_i,z>          (index: the FIRST such constraint) */
#define ZKHIP_REFUSAL_APP_MASK 4 /* prove_app[_dev]: masked assignment non-zero at a constant's position (index: the variable) */
int zkhip_prover_set_checked(zkhip_prover* p, int on);          /* default 0 */
int zkhip_prover_last_refusal(zkhip_prover* p, int* kind, size_t* index);
int zkhip_prover_timings(zkhip_prover* p, double out_ms[8]);   /* as zkhip_last_prove_timings, for p's last proof */
/* 1 if p's last proof was chained (streaming mode, see zkhip_prover_set_streaming): slots [0] and [1] above are then the time it took
 * to ENQUEUE the upload and the QAP map, and the five MSM slots hold the whole device time of the proof */
int zkhip_prover_timings_chained(zkhip_prover* p);
/* (2: p's last proof was SPLIT - with ZKHIP_PROVE_SPLIT=1, an option that is OFF by default because it measured slower, a prover
 * that is not streaming runs the four MSMs over the assignment beside the QAP map and the H MSM behind it, two launch sequences:
 * slot [1] is then the time to enqueue the map and both sequences, the MSM slots the device time of all of it.)  The same question
 * for the plain entry points
 * (zkhip_groth16_prove[_partial|_app]) on the calling thread's device: */
int zkhip_last_prove_split(void);
/* *out = 1: the G1 MSMs of p's last proof accumulated on the Edwards curve (a key with zkhip_key_opts.table_model = 1 that took
 * effect: four G1 MSMs in one launch sequence and B-G2 in a second, or with batch_msms = 0 one sequence per MSM), 0: XYZZ - an
 * XYZZ key, or a strategy that fell back.  Read from the launches themselves, not from the key.  With such a key the five MSM slots
 * of zkhip_prover_timings all hold the time from the first launch to the collection of BOTH sequences, zkhip_prover_last_accumulate_ms
 * the sum of the two accumulation launches and zkhip_prover_last_accumulate_entries the entries of both.
 * zkhip_last_prove_table_model: the same for the plain entry points on the calling thread's device. */
int zkhip_prover_last_table_model(zkhip_prover* p, int* out);
int zkhip_last_prove_table_model(void);
/* the option itself, process-wide (provers that are NOT streaming): 0 one launch sequence (default), 1 two sequences with the H
 * accumulation gated behind the first, 2 not gated.  Proofs are bit-identical in every mode. */
int zkhip_set_prove_split(int mode);
float zkhip_prover_last_accumulate_ms(zkhip_prover* p);          /* as zkhip_last_accumulate_ms, for p's last proof */
int zkhip_prover_last_accumulate_entries(zkhip_prover* p, uint64_t* out);   /* as zkhip_last_accumulate_entries, for p's last proof */
void zkhip_prover_free(zkhip_prover* p);
/* A prover instance over a SLICE of the key (zkhip_crs_upload_slice[_ex] with the same three offsets): own streams and work space
 * like any zkhip_prover, so several slices - on several GPUs, or several contexts of one - run side by side.  It only produces
 * partial sums: zkhip_prover_prove_partial = zkhip_groth16_prove_partial on this instance (QAP map + five MSMs over the slice). */
int zkhip_prover_new_slice(const zkhip_crs* crs_slice, const zkhip_r1cs_desc* cs, size_t a_lo, size_t h_lo, size_t l_lo, zkhip_prover** out);
int zkhip_prover_prove_partial(zkhip_prover* p, const uint64_t* z, uint64_t sums_jac[180]);

/* replaces: wsnarkT::verify(primary_inputs, proof, vk) (libzecale/tests/aggregator/aggregator_dummy_test.cpp:61-62)
 * = libsnark r1cs_gg_ppzksnark_verifier_strong_IC for the Clearmatics Groth16 (no gamma in the key:
 * testdata/dummy_app/aggregator_vk.json), i.e. the equation of contracts/Groth16BW6_761.sol:166-176.
 * Host code (verification is not on the prover's hot path); needs no device and no zkhip_init.
 * vk_abc: (n_inputs + 1) x 24 limbs; inputs: n_inputs x 6 limbs; proof: A (G1), B (G2), C (G1) affine. */
int zkhip_groth16_verify(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                         const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs, const uint64_t proof_affine[72],
                         int* ok);

/* ---- Groth16 verification in batches on the device ------------------------------------------------------------------------------
 * replaces: wsnarkT::verify(primary_inputs, proof, vk) (libzecale/tests/aggregator/aggregator_dummy_test.cpp:61-62), the same seam
 * and the same equation as zkhip_groth16_verify above, for MANY proofs under one key at once: the reduced Tate pairing of
 * zkhip_groth16_verify as gfx950 kernels (pairing.cuh / pairing.hip), eight lanes per verification, and
 * acc = ABC_0 + sum x_i ABC_i per proof on the device.  Verdicts equal zkhip_groth16_verify's on every input that meets the
 * PRECONDITIONS: every coordinate and input is fully reduced, and every point of the key and of the proofs is on its curve and of
 * order r, or the point at infinity (all zero).  zkhip_verifier_new and zkhip_verifier_verify_batch do NOT check them (their result
 * on other inputs is undefined) and are for proofs the caller made or has checked; for proofs from anybody else use the CHECKED
 * route below (zkhip_verifier_new_checked / zkhip_verifier_verify_batch_checked), which validates every point on the device before
 * the pairing.  The fixed G2 generator paired with acc, and "a pair with a member at infinity contributes 1" are the host route's.
 * A handle owns its stream and work space and lives on the calling thread's library device (zkhip_set_device); ONE batch is in
 * flight per handle, several handles - one host thread each - run beside each other and beside provers.  There is no CPU fallback:
 * ZKHIP_ERR_NO_DEVICE / ZKHIP_ERR_STATE without an initialised device.  count == 0 returns ZKHIP_OK; n_inputs == 0 is valid.
 * vk_abc: (n_inputs + 1) x 24 limbs; inputs: count x n_inputs x 6 limbs; proofs_affine: count x [A (G1) | B (G2) | C (G1)];
 * ok: count bytes, 1 = accepted. */
typedef struct zkhip_verifier zkhip_verifier;
int zkhip_verifier_new(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                       const uint64_t* vk_abc, size_t n_inputs, zkhip_verifier** out);
size_t zkhip_verifier_num_inputs(const zkhip_verifier* v);
int zkhip_verifier_verify_batch(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, uint8_t* ok);
void zkhip_verifier_free(zkhip_verifier* v);

/* ---- checked batches: the verifier for proofs somebody else made --------------------------------------------------------------
 * One status byte per proof.  Low nibble: the code below.  High nibble: the elements of the proof that fail with that code
 * (ZKHIP_VERIFY_MASK_*; zero for ACCEPT and REJECT).  The code is the FIRST of ENCODING, OFF_CURVE, NOT_ORDER_R that applies to any
 * element of the proof, and the mask names exactly the elements failing with that code, so the byte is a function of the proof alone
 * and the device and the host routes give the same one.  The all-zero point is the point at infinity and passes the point checks
 * (the pairing then decides as in the unchecked route); a point with x = 0 and y != 0 is not infinity. */
#define ZKHIP_VERIFY_ACCEPT 0       /* all checks pass and the pairing product is one */
#define ZKHIP_VERIFY_REJECT 1       /* all checks pass, the pairing product is not one */
#define ZKHIP_VERIFY_ENCODING 2     /* a coordinate's 12 limbs are >= q, or an input's 6 limbs are >= r (not fully reduced Montgomery form) */
#define ZKHIP_VERIFY_OFF_CURVE 3    /* encodings fine; a point is neither all-zero nor on its curve (A, C: y^2 = x^3 - 1; B: y^2 = x^3 + 4) */
#define ZKHIP_VERIFY_NOT_ORDER_R 4  /* encodings fine, every point on its curve; [r] P != O for some point */
#define ZKHIP_VERIFY_MASK_A 0x10
#define ZKHIP_VERIFY_MASK_B 0x20
#define ZKHIP_VERIFY_MASK_C 0x40
#define ZKHIP_VERIFY_MASK_INPUT 0x80
/* zkhip_verifier_new_checked: as zkhip_verifier_new, but first validates the key's n_inputs + 4 points on the device (the kernel the
 * batches use, once): each is fully reduced and either at infinity or on its curve and of order r.  A key that fails is refused with
 * ZKHIP_ERR_ARG, zkhip_last_error() naming the first offending element (alpha, beta, delta, ABC[i]) and its code.  Only handles
 * made here serve zkhip_verifier_verify_batch_checked (ZKHIP_ERR_STATE otherwise); they serve zkhip_verifier_verify_batch as well.
 * zkhip_verifier_verify_batch_checked: before the pairing, one lane per proof point compares the raw limbs with q, checks the curve
 * equation and computes [r] P (double-and-add, 377 doublings and 135 additions); the inputs are compared with r.  A refused proof
 * enters the pairing kernels as points at infinity and zeros, its status comes from the checks alone.  Same chunking, stream and
 * synchronisation as the unchecked route; on every proof with status 0 or 1, status == 0 equals zkhip_verifier_verify_batch's ok.
 * count == 0 returns ZKHIP_OK.  status: count bytes. */
int zkhip_verifier_new_checked(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                               const uint64_t* vk_abc, size_t n_inputs, zkhip_verifier** out);
int zkhip_verifier_verify_batch_checked(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                                        uint8_t* status);
/* The same checks on the host (no device, no zkhip_init): the reference the device route is pinned on.
 * zkhip_bw6_761_point_check: *code = 0, ZKHIP_VERIFY_ENCODING, _OFF_CURVE or _NOT_ORDER_R for one point (x | y); g2 != 0 selects
 * y^2 = x^3 + 4.  zkhip_groth16_verify_checked: the status byte zkhip_verifier_verify_batch_checked gives for this proof (its
 * verdict, where nothing is refused, is zkhip_groth16_verify's); ZKHIP_ERR_ARG for a key that fails the checks. */
int zkhip_bw6_761_point_check(const uint64_t p[24], int g2, int* code);
int zkhip_groth16_verify_checked(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                 const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs, const uint64_t proof_affine[72],
                                 uint8_t* status);

/* ---- combined batches: ONE random-combination check for a whole batch ------------------------------------------------------------
 * zkhip_verifier_verify_batch answers "which of these proofs are valid?" and pays a full pairing product per proof.  The callers
 * that verify in bulk mostly ask "are these ALL valid?".  For proofs (A_i, B_i, C_i) with inputs x_i under one key and independent
 * non-zero 128-bit scalars rho_i the batch is accepted iff
 *     prod_i t(rho_i A_i, B_i) * t(S_acc, -g2) * t(sigma alpha, -beta) * t(S_C, -delta) == 1,
 *     sigma = sum_i rho_i (mod r),  S_acc = sigma ABC_0 + sum_j (sum_i rho_i x_ij mod r) ABC_j,  S_C = sum_i rho_i C_i:
 * ONE Miller pair, two 128-bit scalar multiplications and a share of two reduction trees per proof on the device, the three shared
 * pairs and the single final exponentiation once per batch on the host.  GT has prime order r, so WHEN EVERY POINT HAS ORDER r a batch
 * with an invalid proof passes with probability about 2^-128 over the choice of the rho_i.
 * PRECONDITIONS on an unchecked handle: those of zkhip_verifier_verify_batch - and they matter MORE here.  There a point outside the
 * group of order r spoils the verdict of its own proof; here the argument for the whole batch rests on GT elements of order r: with a
 * point of small order somebody can make an invalid proof whose error term has small order and is cancelled by the random scalar with
 * noticeable probability, or by a second proof.  Proofs somebody else made go through a handle of zkhip_verifier_new_checked with
 * `status` set.
 * all_ok = 1 iff the check passes.  rho: count x 2 words (little endian, 128 bits each, none zero: ZKHIP_ERR_ARG), or NULL to draw
 * them from the OS (getrandom; ZKHIP_ERR_STATE if that fails, there is no weaker generator behind it) - a caller-supplied rho is for
 * tests and reproducible measurements only: scalars an adversary knows or can predict prove nothing.
 * status: NULL, or count bytes on a handle of zkhip_verifier_new_checked: the point checks of zkhip_verifier_verify_batch_checked run
 * in front, status[i] is that route's refusal byte (ENCODING / OFF_CURVE / NOT_ORDER_R with its mask) or 0; a refused proof is left
 * out of the product and the sums and makes all_ok 0.  status != NULL on an unchecked handle: ZKHIP_ERR_STATE.
 * count == 0: all_ok = 1.  A failed batch does not say which proof is at fault: zkhip_verifier_verify_batch does, and
 * zkhip_verifier_verify_batch_located (below) finds it from this check's own intermediate values.
 * zkhip_groth16_verify_all: the same check on the host alone (no device, no zkhip_init; the per-proof work on up to 16 threads), the
 * route the device one is pinned on; like zkhip_groth16_verify it first fails a batch with a point off its curve. */
int zkhip_verifier_verify_all(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                              const uint64_t* rho, int* all_ok, uint8_t* status);
int zkhip_groth16_verify_all(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                             const uint64_t* vk_abc, size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs_affine,
                             size_t count, const uint64_t* rho, int* all_ok);

/* ---- located batches: per-proof verdicts by way of the combined check ------------------------------------------------------------
 * The combined check reduces the proofs' Miller values and the rho_i C_i in trees of arity 8, chunk by chunk of 16,384 proofs.  A
 * tree node is the product and the sum over a contiguous range of proofs; with the sums of rho_i and rho_i x_ij over the same range it
 * is a complete combined check of that sub-batch under the same scalars, with the same 2^-128 bound.  This route keeps every level
 * of the trees on the device until the call returns (1.2 KB per proof) and, when the batch fails, searches them from the chunk roots down: a round fetches
 * the children of the nodes that failed (one small kernel, one copy) and the host finishes each as it finishes a batch, up to 16 in
 * parallel.  A node that passes clears its range, a leaf that fails is an invalid proof.  Before every round a cost rule
 * (csrc/locate.hpp) compares the rounds that are left with the per-proof route on the proofs still in doubt, and hands those to
 * zkhip_verifier_verify_batch's kernels when that is cheaper (many invalid proofs spread wide).  An all-valid batch costs what
 * zkhip_verifier_verify_all costs.  A batch above 2^20 proofs is cut into consecutive located batches.
 * verdict: count bytes.  On a handle of zkhip_verifier_new: 1 / 0 as zkhip_verifier_verify_batch.  On a handle of
 * zkhip_verifier_new_checked: the status byte of zkhip_verifier_verify_batch_checked - the point checks run in front, a refused proof
 * is left out of every node and every sum and gets its refusal byte.
 * rho: as zkhip_verifier_verify_all (count x 2 words, none zero, or NULL to draw them from the OS).
 * PRECONDITIONS on an unchecked handle: those of zkhip_verifier_verify_all, for the same reason and for every node: the argument
 * rests on GT elements of order r, so every point must be fully reduced, on its curve and of order r (or infinity).  Proofs
 * somebody else made go through a checked handle.
 * stats (may be NULL): what the call did - chunks whose root failed, rounds and node tests of the descent (the chunk round included),
 * proofs handed to the per-proof route, proofs found invalid (REJECT / 0), and the host clock time of the descent and of that route.
 * zkhip_groth16_verify_batch_located: the same route on the host alone (no device, no zkhip_init), the one the device route is
 * pinned on: the nodes' values come from the host's Miller loops, the descent is the same code.  Like zkhip_groth16_verify_all it
 * looks at the curve first: a proof with a point off its curve gets 0 and is left out, a key with one fails every proof.  ok: 1 / 0. */
typedef struct {
  uint32_t chunks_failed, rounds, node_tests, finish_proofs, invalid;
  double descent_ms, finish_ms;
} zkhip_locate_stats;
int zkhip_verifier_verify_batch_located(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                                        const uint64_t* rho, uint8_t* verdict, zkhip_locate_stats* stats);
int zkhip_groth16_verify_batch_located(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                       const uint64_t* vk_abc, size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs_affine,
                                       size_t count, const uint64_t* rho, uint8_t* ok, zkhip_locate_stats* stats);

/* ---- the wrapping (aggregator) circuit: host code, no device needed ------------------------------- */
/* Nested objects are over BLS12-377, whose base field is Fr of BW6-761: coordinates are 6-limb Montgomery
 * elements.  G1 affine = x | y (12 limbs); G2 affine = x.c0 | x.c1 | y.c0 | y.c1 (24 limbs), Fq2 = Fq[u]/(u^2+5).
 * nested_vk   = alpha (12) | beta (24) | delta (24) | ABC_0 .. ABC_k (12 each), k = inputs_per_proof
 * nested_proofs = num_proofs x [ a (12) | b (24) | c (12) ];  nested_inputs = num_proofs x k x 6 limbs. */

/* replaces: nsnark::verify for the nested curve (libzecale/tests/circuits/dummy_application_test.cpp:32-44):
 * Groth16 over BLS12-377, Clearmatics variant without gamma. */
int zkhip_bls12_377_groth16_verify(const uint64_t vk_alpha_g1[12], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                   const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs,
                                   const uint64_t proof_a[12], const uint64_t proof_b[24], const uint64_t proof_c[12], int* ok);

/* ---- nested (BLS12-377) Groth16 verification in batches on the device ----------------------------- */
/* stands beside: nsnark::verify (libzecale/tests/circuits/dummy_application_test.cpp:32-44), one proof per call on the host in the
 * reference and in zkhip_bls12_377_groth16_verify above; the reference has no batched counterpart.  The optimal-ate pairing of that
 * function as gfx950 kernels (csrc/pairing_bls.cuh / pairing_bls.hip): sixteen lanes per verification, the lines of the key's -beta,
 * -delta and of the negated generator and the doubling chains 2^j ABC_i prepared once per handle on the host.
 * nested_vk, nested_proofs and nested_inputs are laid out as above; inputs_per_proof 0 .. 16.
 * PRECONDITION: every coordinate and input is FULLY REDUCED (below the modulus of Fr of BW6-761); the device does not look, and no
 * point is tested for order r.  For proofs from anybody else use the CHECKED route below (zkhip_nested_verifier_new_checked).
 * zkhip_nested_verifier_new checks the key on the HOST before it touches a device: a point off its curve, or a key whose own
 * chains meet a degenerate chord-and-tangent step (an ABC_i, i >= 1, with a multiple 2^j ABC_i of y = 0 - (-1, 0) for one; a zero
 * slope denominator in the line schedule of beta, delta) is refused with ZKHIP_ERR_ARG, zkhip_last_error() naming the element.
 * ok[i] equals the *ok of zkhip_bls12_377_groth16_verify on the same key, inputs and proof: A, B, C are checked against their curves on
 * the device (off the curve, all-zero included: 0), and a proof for which a step of the host's affine arithmetic is degenerate (the input
 * accumulator meets +-2^j ABC_i at step j of input i, whether bit j is set or clear - the host forms that sum at every bit and
 * selects afterwards; a zero among the 69 slope denominators of B) is not decided on the device but handed to that host function
 * inside the call; zkhip_nested_verifier_last_fallbacks says how many of the last batch went that way.
 * Threads: as zkhip_verifier - the handle owns its stream and work space on the calling thread's library device, one batch in
 * flight per handle, handles run beside each other and beside provers.  There is no CPU fallback for a batch as a whole:
 * ZKHIP_ERR_NO_DEVICE / ZKHIP_ERR_STATE without an initialised device.  count == 0 returns ZKHIP_OK. */
typedef struct zkhip_nested_verifier zkhip_nested_verifier;
int zkhip_nested_verifier_new(const uint64_t* nested_vk, size_t inputs_per_proof, zkhip_nested_verifier** out);
size_t zkhip_nested_verifier_num_inputs(const zkhip_nested_verifier* v);
int zkhip_nested_verifier_verify_batch(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs, size_t count,
                                       uint8_t* ok);
int zkhip_nested_verifier_last_fallbacks(const zkhip_nested_verifier* v, size_t* out);
void zkhip_nested_verifier_free(zkhip_nested_verifier* v);

/* ---- checked nested batches: the nested verifier for proofs somebody else made ------------------------------------------------
 * The unchecked route above tests curve membership only, and the optimal-ate pairing is bilinear only on G1 x G2: BLS12-377's G1 has a
 * 125-bit cofactor ((-1, 0), (0, 1) and (2, 3) are on y^2 = x^3 + 1 with orders 2, 3 and 6), its twist a 502-bit one, and an input
 * travels as a 377-bit field element of which the accumulator reads 253 bits (x and x + r share a verdict).  The checked route gives
 * one status byte per proof with the codes and masks of ZKHIP_VERIFY_* / ZKHIP_VERIFY_MASK_* above and the same rule: the FIRST of
 * ENCODING, OFF_CURVE, NOT_ORDER_R that any element has, the high nibble naming exactly the elements with that code.
 *   ENCODING     a coordinate's 6 limbs are >= the modulus of Fr of BW6-761 (A, C: 2 coordinates, B: 4); an input's 6 limbs are >= that
 *                modulus, or its canonical value is >= r of BLS12-377 (r - 1 passes; r and 2^253 - 1 do not)
 *   OFF_CURVE    the point is not on y^2 = x^3 + 1 (A, C) or y^2 = x^3 + 1/u (B).  The nested format has NO point at infinity: the
 *                all-zero point fails its curve equation by itself and is OFF_CURVE - unlike the BW6-761 route above, where it passes
 *   NOT_ORDER_R  [r] P != O, r = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001 (253 bits), by double-and-add over
 *                r's bits (253 doublings, 88 additions; complete formulas, csrc/pairing_bls.cuh nested_point_has_order_r)
 * zkhip_nested_verifier_new_checked: runs these point checks on alpha, beta, delta, ABC_0 .. ABC_k ON THE HOST before anything else
 * reads the key (and so without a device too): a key that fails is refused with ZKHIP_ERR_ARG, zkhip_last_error() naming the first
 * offending element (alpha:, beta:, delta:, ABC[i]:) and its code in brackets.  After that it does what zkhip_nested_verifier_new does.
 * Only handles made here serve zkhip_nested_verifier_verify_batch_checked (ZKHIP_ERR_STATE otherwise); they serve
 * zkhip_nested_verifier_verify_batch as well.
 * zkhip_nested_verifier_verify_batch_checked: in front of the kernels of the unchecked route one lane per proof point (the B points
 * first, so that a wave holds one kind of point) and one per proof's inputs run the checks; a lane stops at its first failure.  A
 * refused proof gets its byte from the checks alone: it runs through the pairing kernels on stand-in values, is never handed to the
 * host and never counted in zkhip_nested_verifier_last_fallbacks.  A proof nothing refuses gets ACCEPT or REJECT as the unchecked
 * route decides it (status == 0 equals its ok); degenerate steps of the input accumulator still go to the host function and are
 * counted.  A B of order r cannot have a degenerate line schedule - kQ = +-Q or 2kQ = O would need r | k -+ 1 or r | 2k for a k below
 * 2^64 - so on the checked route fallbacks come from the input accumulator only.  count == 0 returns ZKHIP_OK.  status: count bytes. */
int zkhip_nested_verifier_new_checked(const uint64_t* nested_vk, size_t inputs_per_proof, zkhip_nested_verifier** out);
int zkhip_nested_verifier_verify_batch_checked(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs,
                                               size_t count, uint8_t* status);
/* The same checks on the host (no device, no zkhip_init; csrc/nested_point_check_host.hpp): the route the device's is pinned on.
 * zkhip_bls12_377_point_check: *code = 0, ZKHIP_VERIFY_ENCODING, _OFF_CURVE or _NOT_ORDER_R for one point: 12 limbs (x | y) or, with
 * g2 != 0, 24 (x.c0 | x.c1 | y.c0 | y.c1).  zkhip_bls12_377_groth16_verify_checked: the status byte
 * zkhip_nested_verifier_verify_batch_checked gives for this proof (where nothing is refused, zkhip_bls12_377_groth16_verify's
 * verdict); ZKHIP_ERR_ARG, with the element and code in zkhip_last_error(), for a key that fails the point checks. */
int zkhip_bls12_377_point_check(const uint64_t* p, int g2, int* code);
int zkhip_bls12_377_groth16_verify_checked(const uint64_t vk_alpha_g1[12], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                           const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs, const uint64_t proof_a[12],
                                           const uint64_t proof_b[24], const uint64_t proof_c[12], uint8_t* status);

/* ---- combined nested batches: ONE random-combination check for a whole batch ---------------------------------------------------
 * zkhip_nested_verifier_verify_batch answers "which of these proofs are valid?" and pays four Miller pairs and a full final
 * exponentiation per proof.  Screening asks "are these ALL valid?".  For proofs (A_i, B_i, C_i) with inputs x_i under one nested key
 * and independent non-zero 128-bit scalars rho_i the batch is accepted iff
 *     prod_i e(rho_i A_i, B_i) * e(S_acc, -g2) * e(sigma alpha, -beta) * e(S_C, -delta) == 1,
 *     sigma = sum_i rho_i (mod r),  S_acc = sigma ABC_0 + sum_j (sum_i rho_i x_ij mod r) ABC_j,  S_C = sum_i rho_i C_i
 * (r the order of BLS12-377's groups, x_ij the low 253 bits of the input's canonical value mod r, e and "== 1" those of the per-proof
 * route): ONE Miller pair, two 128-bit scalar multiplications and a share of two reduction trees per proof on the device, no input
 * accumulator chain; the sums, k + 1 scalar multiplications for S_acc, the three shared pairs and the single final exponentiation
 * once per batch on the host.  GT has prime order r, so WHEN EVERY POINT HAS ORDER r a batch with an invalid proof passes with
 * probability about 2^-128 over the choice of the rho_i.
 * PRECONDITIONS on an unchecked handle: those of zkhip_nested_verifier_verify_batch - and they matter MORE here.  There a point outside
 * the group of order r spoils the verdict of its own proof; here the argument for the whole batch rests on GT elements of order r:
 * with a point of small order somebody can make an invalid proof whose error term has small order and is cancelled by the random
 * scalar with noticeable probability, or by a second proof.  Proofs somebody else made go through a handle of
 * zkhip_nested_verifier_new_checked with `status` set.
 * THE STATEMENT: this route answers the group law's.  The per-proof route reproduces the host's affine accumulator chain, and for one
 * kind of statement the host says 0 where the group law says valid - the accumulator meets -2^j ABC_i at a CLEAR bit j of input i;
 * this route ACCEPTS such a statement (and never hands a proof to the host for its accumulator: there is no chain).
 * What a proof does to the batch: a point off its curve (all zero included: the nested format has no infinity) fails the batch and is
 * left out of the value; so does a B whose line schedule has a zero slope denominator - it cannot have order r, so under the
 * precondition failing is right; zkhip_nested_verifier_last_degenerate counts them in the last combined batch (the per-proof route
 * hands such a proof to the host).  rho_i A_i = O (an A of small order, e.g. (-1, 0) under an even scalar): that pair contributes one.
 * all_ok = 1 iff the check passes.  rho: count x 2 words (little endian, 128 bits each, none zero: ZKHIP_ERR_ARG), or NULL to draw
 * them from the OS (getrandom; ZKHIP_ERR_STATE if that fails, there is no weaker generator behind it) - a caller-supplied rho is for
 * tests and reproducible measurements only: scalars an adversary knows or can predict prove nothing.
 * status: NULL, or count bytes on a handle of zkhip_nested_verifier_new_checked: the checks of
 * zkhip_nested_verifier_verify_batch_checked run in front, status[i] is that route's refusal byte (ENCODING / OFF_CURVE / NOT_ORDER_R
 * with its mask) or 0; a refused proof is left out of the product and the sums and makes all_ok 0.  status != NULL on an unchecked
 * handle: ZKHIP_ERR_STATE.  count == 0: all_ok = 1.  A failed batch does not say which proof is at fault: the per-proof routes do.
 * zkhip_bls12_377_groth16_verify_all: the same check on the host alone (no device, no zkhip_init; the per-proof work on up to 16
 * threads), the route the device one is pinned on. */
int zkhip_nested_verifier_verify_all(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs, size_t count,
                                     const uint64_t* rho, int* all_ok, uint8_t* status);
int zkhip_nested_verifier_last_degenerate(const zkhip_nested_verifier* v, size_t* out);
int zkhip_bls12_377_groth16_verify_all(const uint64_t vk_alpha_g1[12], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                       const uint64_t* vk_abc, size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs, size_t count,
                                       const uint64_t* rho, int* all_ok);

/* replaces: libzecale::aggregator_circuit<wppT, wsnarkT, nverifierT, NumProofs>(inputs_per_nested_proof)
 * (libzecale/circuits/aggregator_circuit.hpp:32-114; constructor .tcc:17-98): builds the constraint system.
 * num_proofs 1 .. 32 (one result bit per nested proof, packed into one primary input), inputs_per_proof 1 .. 16; anything else:
 * ZKHIP_ERR_ARG.  32 proofs with one input each are 575,723 constraints (a 2^20 domain), with nine inputs 1,230,075 (2^21). */
typedef struct zkhip_aggregator zkhip_aggregator;
int zkhip_aggregator_new(size_t num_proofs, size_t inputs_per_proof, zkhip_aggregator** out);
void zkhip_aggregator_free(zkhip_aggregator* a);
size_t zkhip_aggregator_num_proofs(const zkhip_aggregator* a);
size_t zkhip_aggregator_inputs_per_proof(const zkhip_aggregator* a);
size_t zkhip_aggregator_num_constraints(const zkhip_aggregator* a);
size_t zkhip_aggregator_num_variables(const zkhip_aggregator* a);      /* including the constant ONE */
size_t zkhip_aggregator_num_primary_inputs(const zkhip_aggregator* a); /* aggregator_circuit::num_primary_inputs, .tcc:172-180 */
/* replaces: get_constraint_system() (aggregator_circuit.hpp:99-101); pointers stay valid while `a` lives */
int zkhip_aggregator_get_r1cs(const zkhip_aggregator* a, zkhip_r1cs_desc* out);
/* replaces: the generate_r1cs_witness calls of aggregator_circuit::prove (.tcc:136-157): full assignment
 * z = (1, primary, auxiliary), n_vars x 6 limbs; primary = [vk hash, packed results, nested inputs ...] */
int zkhip_aggregator_witness(zkhip_aggregator* a, const uint64_t* nested_vk, const uint64_t* nested_proofs,
                             const uint64_t* nested_inputs, uint64_t* z_out);
/* replaces: the well-formedness checks libsnark applies to a proof before it is used (proof.is_well_formed(); in the circuit:
 * the G1 / G2 checker gadgets of r1cs_gg_ppzksnark_proof_variable, groth16_verifier_parameters.hpp:16-27): *ok = 1 iff every
 * point of the nested key and of the nested proofs lies on its curve (BLS12-377 G1: y^2 = x^3 + 1, G2: y^2 = x^3 + 1/u).
 * zkhip_aggregator_witness itself computes an assignment for ANY input; for an off-curve proof point that assignment violates
 * the circuit's curve constraints (no wrapping proof exists).  The streaming prover and the C++ mirror call this first. */
int zkhip_aggregator_check_inputs(const zkhip_aggregator* a, const uint64_t* nested_vk, const uint64_t* nested_proofs, int* ok);
/* replaces: verification_key_hash_gadget::compute_hash(vk, num_inputs) (verification_key_hash_gadget.tcc:42-59) */
int zkhip_aggregator_vk_hash(const uint64_t* nested_vk, size_t inputs_per_proof, uint64_t out[6]);

/* Witness generation ON THE GPU: the same assignment as zkhip_aggregator_witness, limb for limb, computed by a device kernel that
 * interprets the straight-line program recorded from the circuit (witness_tape.cpp, witness.hip).  One batch occupies one wave of
 * the levelled program and one of the key-hash chain (a workgroup of up to sixteen waves where the program is wide: batches of
 * many nested proofs, zkhip_gpu_witness_set_waves) for ~tens of milliseconds: the gain is not latency (the host generator takes 8 ms on three cores) but host cores - a server keeps
 * many batches in flight and the GPU generates their witnesses under the provers' kernels.
 *   zkhip_aggregator_witness_gpu   one batch, host in / host out (allocates its work space: a test / convenience entry point)
 *   zkhip_gpu_witness_*            work space for one batch in flight on the calling thread's device; run() leaves the assignment
 *                                  in DEVICE memory (d_z_out: n_vars x 6 limbs, ready for zkhip_prover_prove_dev) and returns the
 *                                  primary inputs.  ZKHIP_ERR_ARG when an inversion met zero (degenerate nested points, where the
 *                                  host generator branches): fall back to zkhip_aggregator_witness for that batch.
 * replaces: the generate_r1cs_witness calls of aggregator_circuit::prove (aggregator_circuit.tcc:136-157, aggregator_gadget.tcc:87-112) */
int zkhip_aggregator_witness_gpu(zkhip_aggregator* a, const uint64_t* nested_vk, const uint64_t* nested_proofs, const uint64_t* nested_inputs,
                                 uint64_t* z_out);
typedef struct zkhip_gpu_witness zkhip_gpu_witness;
int zkhip_gpu_witness_new(zkhip_aggregator* a, zkhip_gpu_witness** out);
int zkhip_gpu_witness_run(zkhip_gpu_witness* w, const uint64_t* nested_vk, const uint64_t* nested_proofs, const uint64_t* nested_inputs,
                          void* d_z_out, uint64_t* primary_inputs);
 /* several batches in ONE launch sequence (a workgroup each: n witnesses take as long as one).  d_z_out: n x n_vars x 6 limbs,
 * contiguous; primary_inputs: n x n_primary x 6 limbs; degenerate[i] != 0: batch i met an inversion of zero, its assignment is void */
int zkhip_gpu_witness_new_batched(zkhip_aggregator* a, size_t max_batches, zkhip_gpu_witness** out);
int zkhip_gpu_witness_run_batched(zkhip_gpu_witness* w, size_t n, const uint64_t* const* nested_vk, const uint64_t* const* nested_proofs,
                                  const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate);
void zkhip_gpu_witness_free(zkhip_gpu_witness* w);
/* Waves per witness of the levelled program, for every later run of this handle: 1 = one wave per witness (k_witness); 2, 4, 8, 16 = a
 * workgroup of that many waves per witness that share each level of the program and meet at a barrier after it (k_witness_wide:
 * worth it where a level holds several 64-instruction chunks - 5.4 on average at 32 nested proofs, 1.07 at two); 0 = auto, the
 * default: one wave below 1.5 chunks per level on average, eight from there on (profiles/batch32_witness.txt).  Anything else: ZKHIP_ERR_ARG.  The assignment is the same at every width. */
int zkhip_gpu_witness_set_waves(zkhip_gpu_witness* w, int waves);
/* milliseconds the kernels of w's last run took on the device, all its batches together (HIP events on the run's stream, from before
 * the first launch to after the kernel that writes the assignments; the copies are outside) */
int zkhip_gpu_witness_last_ms(zkhip_gpu_witness* w, double* ms);
/* HOST ONLY: what the recorded program of the circuit asks of the device.  out[0] chunks of 64 instructions in the levelled program,
 * out[1] its levels, out[2] sum over levels of ceil(chunks of the level / waves) - the chunk-times on the critical path when `waves`
 * waves share each level -, out[3] bytes of values per witness in flight (zkhip_gpu_witness_new_batched allocates max_batches times
 * that and fails with ZKHIP_ERR_HIP, naming the bytes, when the device does not have them).  waves = 0: out[2] is THE WIDTH auto
 * picks for this program instead (ask again with that width for its steps). */
int zkhip_gpu_witness_plan(zkhip_aggregator* a, int waves, size_t out[4]);
/* the recorded program: [0] operations recorded, [1] positions after levelling (with padding), [2] dependent levels,
 * [3] multiplications, [4] inversions, [5] distinct constants */
int zkhip_gpu_witness_stats(zkhip_aggregator* a, size_t out[6]);

/* ---- PER-APPLICATION CONSTANTS -----------------------------------------------------------------------------------------------
 * The reference registers an application - a nested verification key - once (RegisterApplication, aggregator_server.cpp:170-235)
 * and then aggregates batch after batch of ITS proofs (GenerateAggregatedTransaction, :279-348).  Everything the wrapping circuit
 * derives from the nested key alone is the same in every one of those batches: the key's variables, the MiMC chain of its hash
 * (verification_key_hash_gadget.tcc:36-40), the lines of -beta and -delta (aggregator_gadget.tcc:93) and the doubling chains
 * 2^j ABC_i of the input accumulators - 9,038 of the 44,206 variables at batch 2 with one input per nested proof.  Their share of
 * the A, B-G2, B-G1 and L sums of a proof, sum z_i Base_i over those positions, is FOUR CONSTANT POINTS per (application, proving
 * key).  A zkhip_aggregator_app computes both once:
 *   - the constant positions (auxiliary variables only: the constant ONE and the primary inputs - the key's hash among them - stay
 *     ordinary entries) and their values, by recording the circuit with the key as constants (witness_tape.cpp): what the
 *     recorder folds does not depend on the proofs;
 *   - the four points, by one masked MSM per query over the resident key.
 * Per batch, the generators then produce a MASKED assignment - zero at the constant positions: a zero scalar produces no bucket
 * entry, so the five MSMs lose a sixth of their entries - the QAP map runs on (masked | constants), H is untouched, and the tail adds
 * the four points.  The proof is the same group elements as without the handle: bit-identical (tests/test_app_cache_gpu.py).
 * The handle belongs to ONE proving key (its GPU) and ONE circuit; crs and a must outlive it. */
typedef struct zkhip_aggregator_app zkhip_aggregator_app;
int zkhip_aggregator_app_new(zkhip_aggregator* a, const zkhip_crs* crs, const uint64_t* nested_vk, zkhip_aggregator_app** out);
void zkhip_aggregator_app_free(zkhip_aggregator_app* app);
size_t zkhip_aggregator_app_num_constants(const zkhip_aggregator_app* app);
/* positions (num_constants, ascending), their values (x 6 limbs), the key's hash (primary input 0) and the four cached points
 * (A, B-G2, B-G1, L: 4 x 36 limbs, Jacobian); any pointer may be null */
int zkhip_aggregator_app_constants(const zkhip_aggregator_app* app, uint32_t* positions, uint64_t* values, uint64_t vk_hash[6], uint64_t points_jac[144]);
/* a FULL assignment generated under the application's key -> masked in place (ZKHIP_ERR_ARG if a constant position holds another value) */
int zkhip_aggregator_app_mask(const zkhip_aggregator_app* app, uint64_t* z);
/* replaces: the generate_r1cs_witness calls of aggregator_circuit::prove (aggregator_circuit.tcc:136-157) for a batch of the
 * registered application: the proof sections only (the key's hash and lines are not recomputed), masked assignment out */
int zkhip_aggregator_witness_app(const zkhip_aggregator_app* app, const uint64_t* nested_proofs, const uint64_t* nested_inputs, uint64_t* z_out);
/* replaces: wsnarkT::generate_proof (aggregator_circuit.tcc:168) for a masked assignment: same proof as zkhip_groth16_prove /
 * zkhip_prover_prove[_dev] on the full one.  A host assignment that is not masked is refused (ZKHIP_ERR_ARG). */
int zkhip_groth16_prove_app(const zkhip_crs* crs, zkhip_r1cs* r1cs, const zkhip_aggregator_app* app, const uint64_t* z_masked, const uint64_t r[6],
                            const uint64_t s[6], uint64_t proof_affine[72]);
int zkhip_prover_prove_app(zkhip_prover* p, const zkhip_aggregator_app* app, const uint64_t* z_masked, const uint64_t r[6], const uint64_t s[6],
                           uint64_t proof_affine[72]);
/* PRECONDITION of the device form (not checked - a check would cost a pass over the assignment per proof): d_z_masked is an assignment
 * of THIS application with zero at every constant position (zkhip_aggregator_app_constants' `positions`) - what
 * zkhip_gpu_witness_run_batched_app writes.  The QAP map ORs the constants into it limb-wise, so a full or foreign assignment gives a
 * wrong H and a proof that does not verify, with ZKHIP_OK.  The host forms above refuse such an assignment. */
int zkhip_prover_prove_app_dev(zkhip_prover* p, const zkhip_aggregator_app* app, const void* d_z_masked, const uint64_t r[6], const uint64_t s[6],
                               uint64_t proof_affine[72]);
/* zkhip_gpu_witness_run_batched for n batches of ONE application, by the application's own device program (the key folded in: no
 * key-hash launch, an eighth fewer multiplications): masked assignments in device memory, ready for zkhip_prover_prove_app_dev */
int zkhip_gpu_witness_run_batched_app(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_proofs,
                                      const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate);

/* Streaming form of aggregator_circuit::prove for a server that wraps batch after batch (the reference's
 * GenerateAggregatedTransaction loop, aggregator_server.cpp:300-420, handles one batch at a time on the CPU):
 * `witness_workers` host threads generate witnesses (zkhip_aggregator_witness) while `gpu_slots` prover instances
 * keep that many proofs in flight on the GPU; the host tail of one proof overlaps the device work of the next.
 * submit copies its inputs and returns a ticket (it blocks only while 4 x (gpu_slots + witness_workers) batches are
 * still unproved; finished batches wait for their collector and never block a submitter); wait blocks until that batch is done and returns the extended proof: primary inputs
 * (num_primary_inputs x 6 limbs: vk hash, packed results, nested inputs) and the proof (a | b | c, 72 limbs).
 * Every result is bit-identical to zkhip_aggregator_witness + zkhip_groth16_prove on the same inputs, r and s.
 * gpu_slots and witness_workers: 1 .. 64 each.  ZKHIP_PIPELINE_STATS=1 in the environment prints, when a pipeline is freed, the time
 * a proof spent in a prover, the time a prover waited for an assignment and the host witness time (stderr). */
typedef struct zkhip_pipeline zkhip_pipeline;
int zkhip_aggregator_pipeline_new(zkhip_aggregator* a, const zkhip_crs* crs, int gpu_slots, int witness_workers, zkhip_pipeline** out);
/* flags: ZKHIP_PIPELINE_GPU_WITNESS - the witness workers generate the assignment on the GPU (zkhip_gpu_witness_run: each worker is
 * a host thread that waits on its batch's kernel; the assignment never leaves the device) and fall back to the host generator for a
 * degenerate batch.  Results are the same proofs. */
#define ZKHIP_PIPELINE_GPU_WITNESS 1u
/* ZKHIP_PIPELINE_NO_APP_CACHE - a pipeline keeps a zkhip_aggregator_app per nested key it has seen (at most 32; built by the first
 * batch of a key or by zkhip_aggregator_pipeline_register_app) and proves that key's batches from masked assignments; this flag (or
 * ZKHIP_NO_APP_CACHE in the environment) turns that off.  The proofs are the same either way. */
#define ZKHIP_PIPELINE_NO_APP_CACHE 2u
/* ZKHIP_PIPELINE_HYBRID_WITNESS (with ZKHIP_PIPELINE_GPU_WITNESS) - two host generator threads (ZKHIP_HYBRID_HOST_WORKERS: 1 .. 16) work
 * the same queue as the GPU batchers, taking a batch only while MORE than one full witness launch (16 batches) is queued - what the
 * batchers could not start on anyway (a launch of three batches takes as long as one of sixteen).  Round 5, one MI355X, batch 2: between
 * the pure modes in host cores (2.9-3.4; host 4.1-4.7, GPU 2.1-2.4) and, run by run, between 6 % below and 3 % above the host
 * generator in proofs/s.  Results are the same proofs. */
#define ZKHIP_PIPELINE_HYBRID_WITNESS 4u
int zkhip_aggregator_pipeline_new_ex(zkhip_aggregator* a, const zkhip_crs* crs, int gpu_slots, int witness_workers, unsigned flags, zkhip_pipeline** out);
/* replaces: RegisterApplication's part in the prover (aggregator_server.cpp:170-235 stores the key; here its constants are computed,
 * ~0.2 s, so that the application's first batch does not pay for them).  ZKHIP_ERR_ARG: a key with a point off its curve. */
int zkhip_aggregator_pipeline_register_app(zkhip_pipeline* p, const uint64_t* nested_vk);
size_t zkhip_aggregator_pipeline_app_hits(const zkhip_pipeline* p);     /* batches proved from an application's constants so far */
int zkhip_aggregator_pipeline_submit(zkhip_pipeline* p, const uint64_t* nested_vk, const uint64_t* nested_proofs,
                                     const uint64_t* nested_inputs, const uint64_t r[6], const uint64_t s[6], uint64_t* ticket);
int zkhip_aggregator_pipeline_wait(zkhip_pipeline* p, uint64_t ticket, uint64_t* primary_inputs, uint64_t proof_affine[72]);
void zkhip_aggregator_pipeline_free(zkhip_pipeline* p);

/* replaces: wsnarkT::generate_setup(pb) = libsnark::r1cs_gg_ppzksnark_generator, reached from
 * aggregator_circuit::generate_trusted_setup (libzecale/circuits/aggregator_circuit.tcc:100-109).
 * QAP evaluation at tau on the host, the batch exponentiations on the GPU (zkhip_fixed_base_mul).
 * The toxic waste is an argument so that tests can reproduce keys; a deployment passes fresh randomness and
 * forgets it.  All four scalars: 6 limbs, Montgomery form, non-zero.  (zkhip_keypair: declared with the phase-2 section above.) */
int zkhip_groth16_setup(const zkhip_r1cs_desc* cs, const uint64_t tau[6], const uint64_t alpha[6], const uint64_t beta[6],
                        const uint64_t delta[6], zkhip_keypair** out);
/* the same with the evaluation domain as an argument (see zkhip_r1cs_upload_ex): ZKHIP_DOMAIN_DEFAULT = the forced power of two that
 * libzeth's generate_setup uses (what zkhip_groth16_setup does), ZKHIP_DOMAIN_STEP = libfqfft's unforced choice, else a valid size */
int zkhip_groth16_setup_ex(const zkhip_r1cs_desc* cs, const uint64_t tau[6], const uint64_t alpha[6], const uint64_t beta[6],
                           const uint64_t delta[6], size_t domain_size, zkhip_keypair** out);
/* ONE RANK'S SHARE of the same setup, for a key partitioned over the GPUs of a node (BASELINE configs[3]): the exponents are
 * evaluated on the host as above, the three index ranges are cut into `parts` contiguous slices of equal FINITE terms - the cuts
 * zkhip_key_partition makes on a finished key: an exponent of zero is a base at infinity - and only slice `part` is multiplied out,
 * on the device, straight into the base sets and window tables of *slice_out (a handle like zkhip_crs_upload_slice_ex's; the points
 * never visit the host).  ranges: a_lo, a_hi, h_lo, h_hi, l_lo, l_hi of the slice.  *vk_out (optional): a keypair WITHOUT query
 * vectors - its verification half (zkhip_keypair_vk) and the five constants zkhip_groth16_finish needs (zkhip_keypair_crs_desc).
 * replaces: the same generate_setup call, run by N processes that each keep an N-th of pk. */
int zkhip_groth16_setup_slice(const zkhip_r1cs_desc* cs, const uint64_t tau[6], const uint64_t alpha[6], const uint64_t beta[6],
                              const uint64_t delta[6], size_t domain_size, int parts, int part, const zkhip_key_opts* opts,
                              zkhip_crs** slice_out, size_t ranges[6], zkhip_keypair** vk_out);
/* proving half: pointers into the keypair (valid while it lives) */
int zkhip_keypair_crs_desc(const zkhip_keypair* kp, zkhip_crs_desc* out);
/* verification half: alpha (G1), beta, delta (G2), abc = (n_primary + 1) x 24 limbs; returns n_primary + 1 */
size_t zkhip_keypair_vk(const zkhip_keypair* kp, uint64_t alpha_g1[24], uint64_t beta_g2[24], uint64_t delta_g2[24],
                        const uint64_t** abc);
/* replaces: wsnarkT::keypair_write_bytes / keypair_read_bytes (aggregator_server.cpp:77-94: the server writes the key after
 * the first setup and reads it on later starts).  The reference's byte layout lives in the absent libzeth; this is the library's
 * own container (header, the limb arrays as they cross this ABI, checksum): not interchangeable with a reference key file. */
int zkhip_keypair_write(const zkhip_keypair* kp, const char* path);
int zkhip_keypair_read(const char* path, zkhip_keypair** out);
void zkhip_keypair_free(zkhip_keypair* kp);

/* duration (ms, HIP events on the library's stream) of the dominant kernel of the last MSM */
float zkhip_last_accumulate_ms(void);
/* The entries that launch accumulated: the non-zero digits of its scalars = the mixed additions of k_accumulate (a zero scalar, a zero
 * digit and a base at infinity produce none - a witness of mostly small values has far fewer than terms x digits).  Read back from the
 * sort's histogram: a measurement aid that synchronises the device (bench.py's roofline numerator); 0 before the first launch. */
int zkhip_last_accumulate_entries(uint64_t* out);
/* begin and end of that launch (ms, HIP events) on a per-device time base: a caller that keeps several MSMs in flight
 * (zkhip_msm_submit / collect) can see how their accumulations overlap and take the union of the intervals */
int zkhip_last_accumulate_interval(float out_ms[2]);
/* The time base above is recorded when the library first plans an MSM on a GPU; the values are FLOAT milliseconds since then (1 us
 * of resolution for ~8 s, 0.06 ms after an hour).  A caller that compares intervals records the origin again at the start of its
 * timed region (calling thread's library device). */
int zkhip_reset_time_base(void);
/* The Fq multiplier's own peak on the calling thread's library device, measured NOW: dependent chains of 761-bit Montgomery products
 * at the accumulation kernel's occupancy, chip-wide products per second (~25 ms of device time).  The bound that binds this path is
 * the integer multiplier, and its rate differs between boxes and power states of the same model: a measurement states
 * its fraction against the peak of the run it was taken in. */
int zkhip_measure_fq_mul_rate(double* fq_mul_per_s);
/* The transform kernels of zkhip_ntt ALONE (no conversion from / to the ABI's limbs, no allocation): `batch` (1 .. 3: the QAP map
 * transforms its A, B, C vectors in the same launches) resident vectors of 2^log_d elements, `reps` timed transforms after one
 * untimed, HIP events on the stream the passes run on.  *ms_per_transform = elapsed / (reps x batch).  dir / coset as zkhip_ntt.
 * replaces: nothing - the measurement behind bench.py's ntt roofline (2 d 48 B per transform). */
int zkhip_measure_ntt(unsigned log_d, int dir, int coset, int batch, int reps, double* ms_per_transform);
/* Test hooks of the transform passes in device layout (no counterpart).
 * ntt_packed: the engine's batched transform once on `nbuf` (1 .. 3) host vectors of 2^log_d elements, back to back in `data`, in
 * place.  Elements are in device LOCATION order: element i of a host vector goes to location i of its device buffer and comes back
 * from location i - the hook permutes nothing.  A vector of 2^12 elements or more is in natural order on one side of a transform and
 * in TRANSPOSED order on the other (K = 2^ceil(log_d / 2), N2 = 2^log_d / K: element k1 + K k2 at location k1 N2 + k2);
 * in_transposed says on which side the input is and is ignored below 2^12.  form 0: ABI limbs, 6 x u64 per element, canonical;
 * form 1: the packed device words, 12 x u32 per element, holding value 2^406 mod r plus any multiple of r with the total below
 * 2^384, copied in and out untouched (the transforms' input contract: below 8 r, below 64 r for the forward coset transform).  dir / coset as zkhip_ntt.  A bad argument -
 * a forward coset transform with in_transposed at 2^12 or more among them - gives ZKHIP_ERR_ARG; nothing is launched and `data` is
 * left as it was.
 * ntt_set_one_each_max: process-wide override of ZKHIP_NTT_ONE_EACH_MAX - sizes up to 2^log_d_max take one sub-transform per
 * workgroup, larger ones the wide tiles (2048 elements per workgroup); -1: the environment / default (22).  A test and measurement
 * knob: results do not depend on it. */
int zkhip_internal_ntt_packed(void* data, int form, int nbuf, unsigned log_d, int dir, int coset, int in_transposed);
int zkhip_internal_ntt_set_one_each_max(int log_d_max);   /* -1: the environment / default (22) */
/* Test hook (no counterpart): the device build's three multiplier bodies - the code every kernel runs (fp29.cuh / fp29_chain.cuh) - on
 * operands given limb by limb: field 0 = Fq (27 limbs of 29 bits), 1 = Fr (14); limbs_in holds n cases of (a, b, c, d), limbs_out
 * receives n x { a b / R, a^2 / R, (a b + c d) / R } in the device's own form (R = 2^783 / 2^406).  Operands must respect the
 * bodies' contract (limbs below 2^29 except the top one, products below 2^10 R p). */
int zkhip_internal_field_selftest(int field, const uint32_t* limbs_in, size_t n, uint32_t* limbs_out);
/* Test hook (no counterpart): the rest of the device build's field layer (fp29.cuh, fp_inv.cuh) on raw limbs, one function per call
 * and one GPU lane per case, 64 lanes a workgroup (case i is lane i % 64 of wave i / 64).  limbs_in holds n cases of three operands
 * (a, b, c) of NL 32-bit words each (NL = 27 / 14); limbs_out receives n x (NL words, one flag word).  op:
 *   0 fp_add(a, b)   1 fp_dbl(a)   2 .. 5 fp_sub<K>(a, b), K = 2, 4, 8, 16   6 fp_sub_sub2<8>(a, b, c)   7 fp_cond_sub_p(a)
 *   8 .. 11 fp_cond_sub_kp<K>(a), K = 1, 2, 4, 8   12 fp_canon_4p(a)   13 fp_canon(a)   14 fp_is_zero_2p(a): a and, in the flag, 0 / 1
 *   15 fp_unpack32 then fp_pack32: N32 words in a, N32 words out (N32 = 24 / 12)   16 fp_pack32 then fp_unpack32 of the limbs a
 *   17 fp_to_abi then fp_from_abi   18 fp_abi_to_canonical_words: N32 words in a, N32 words out   19 fp_inv(a)
 *   32 + log2 K: fp_sub_k<K>(a, b) for the K the library itself uses (Fq: 1, 32; Fr: 2, 4, 8, 16, 64, 128)
 * An op the field does not have gives ZKHIP_ERR_ARG.  Operands must respect each function's documented contract. */
int zkhip_internal_field_ops_selftest(int field, int op, const uint32_t* limbs_in, size_t n, uint32_t* limbs_out);
/* Test hook (no counterpart): the device build's point layer (csrc/ec.cuh, ec_mem.cuh, ec_edw.cuh) on raw limbs, one function per call.
 * One GPU lane per case, 64 lanes a workgroup (case i is lane i % 64 of wave i / 64); the quad forms take four lanes a case (lanes
 * 4 (i % 16) .. 4 (i % 16) + 3 of wave i / 16).  Operands are staged in the form the function takes in the library - registers, a packed
 * point in global memory, a memory reference (mem 0: limb-major array, stride n; mem 1: the slot structure), the LDS images and a
 * register Y - and nothing is converted, reduced or normalised on the way.
 * limbs_in, per case 224 words: A = X | Y | ZZ | ZZZ (Edwards: X | Y | Z | T), 27 limbs of 29 bits each; B = the same, or x | y of a
 * register affine operand, or the words of a packed operand (48 / 72); neg; three entries (index | neg << 31 into `table`, n_table
 * precomputed Edwards points of 72 words) and their count, for op 18.
 * limbs_out, per case 217 words: the accumulator's four coordinates (an X kept packed in LDS: its 24 words and three zeros; op 17: the
 * 72 packed words), a flag word - the function's return value, for a void function whether the result's ZZ / Z tests as zero - and B
 * as it stands afterwards.  op:
 *   0 xyzz_dbl_affine(B)   1 xyzz_dbl(A)   2 xyzz_madd(A, B)   3 xyzz_add(A, B)   4 xyzz_neg(A)
 *   5 madd_mem   6 madd_lds_regy   7 add_lds_regy   8 add_mem_s   9 dbl_mem   10 add_mem_quad   11 dbl_mem_quad
 *   12 edw_madd_lds_regy   13 edw_add_lds_regy   14 edw_add_mem   15 edw_add_mem_quad   16 edw_dbl_mem_quad   17 edw_from_affine(B)
 *   18 edw_pre_issue, edw_open_lds_pre, then count - 1 edw_madd_lds_pre, driven as k_accumulate_edw_lock drives them (count 1 .. 3,
 *      descending inside a wave)
 * mem 1 is for the ops that take a memory reference (5 .. 11, 13 .. 16).  An unknown op, a mem the op does not take or an entry
 * past the table gives ZKHIP_ERR_ARG and nothing is launched.  Operands must respect each function's documented contract. */
int zkhip_internal_point_ops_selftest(int op, int mem, const uint32_t* limbs_in, size_t n, const uint32_t* table, size_t n_table,
                                      uint32_t* limbs_out);
/* Test hooks of the Edwards accumulation's lockstep route (no counterpart).  A single MSM over a table in the Edwards model always
 * enqueues two accumulations, one bucket per lane (k_accumulate_edw_lock) and sliced (k_accumulate_edw); a word the device writes
 * per launch decides which of them runs.
 * set_lockstep: mode 0 = every launch sliced, 1 = the device decides, -1 = the environment (ZKHIP_LOCKSTEP); min_buckets = the
 * non-empty buckets a launch needs for the lockstep route (-1: two waves for every SIMD of the chip; tests on small sets lower it).
 * last_acc_path: the word of the launch zkhip_last_accumulate_ms was read from, copied back when this is called and never
 * otherwise: 1 lockstep, 0 sliced, -1 not an Edwards launch. */
int zkhip_internal_set_lockstep(int mode, int min_buckets);
int zkhip_internal_last_acc_path(int* out);
/* Test hook of the merged launch (no counterpart; otherwise reachable through whole proofs only): K <= 4 MSMs, job k over the first
 * n[k] bases of sets[k] with the host scalars scalars[k] (n[k] x 6 limbs), through ONE launch sequence.  The sets are table-backed,
 * one level per window, all of one window (zkhip_bases_precompute).  model 0: XYZZ; 1: the Edwards accumulation
 * (k_accumulate_edw_multi for K > 1) - a set with terms but without an Edwards form (a G2 set) gives ZKHIP_ERR_STATE before anything is
 * enqueued.  *acc_path as zkhip_internal_last_acc_path for this launch; out_jac: K x 36 limbs. */
int zkhip_internal_msm_multi(const zkhip_bases* const* sets, const uint64_t* const* scalars, const size_t* n, int K, int montgomery, int model,
                             int* acc_path, uint64_t* out_jac);
/* Test / A-B hook (no counterpart; results never depend on it).
 * set_msm_stream_layout: how the zkhip_msm_streams made from now on place their contexts' HIP streams:
 * 0 = every context creates its pair at its first submit, 1 = all primaries, then all secondaries, when the stream is made,
 * 2 = primaries only, a context's whole launch sequence on it; -1 = the environment (ZKHIP_MSM_STREAM_LAYOUT) / default. */
int zkhip_internal_set_msm_stream_layout(int layout);
/* Test hook of the bucket reduction's tail (no counterpart): the two small weighted sums per bucket window by bit planes and
 * R * hi + lo, alone.  items_affine: 2W groups of N affine points (24 limbs each, all-zero = infinity), the W hi
 * groups first; item i of a group has weight i + 1.  out_jac[w] = 2^lo_bits sum_i (i+1) hi_w[i] + sum_i (i+1) lo_w[i], and, if total,
 * out_jac[W + w] = sum_i lo_w[i] (36 limbs each).  edw 0: XYZZ points; 1: the Edwards model - the items go through chi, the results
 * back through psi, and psi(chi(P)) = 2 P: every output is TWICE the sum above.  W in 1 .. 5, N a power of two in 2 .. 2048. */
int zkhip_internal_msm_tail(int edw, const uint64_t* items_affine, int W, unsigned N, int lo_bits, int total, uint64_t* out_jac);
/* Test hooks of the pairing kernels (no counterpart).
 * fq6_selftest: n independent operand sets through the per-lane bodies of pairing.cuh inside a real kernel, eight lanes per set:
 * op 0 = a b, 1 = a^2, 2 = a (b_0 + b_3 w^3 + b_4 w^4) (the sparse line product; b's other coefficients are ignored) in
 * Fq6 = Fq[w]/(w^6 + 4).  a, b, out: n x 6 coefficients x 12 ABI limbs.
 * pairing_product: out[i] = prod_{p < pairs_per_product} t(g1[i][p], g2[i][p]), the REDUCED value (6 x 12 ABI limbs, canonical), of
 * `count` products; g1, g2: count x pairs_per_product x 24 limbs; pairs_per_product in 1 .. 4.  route 0: the host code of
 * zkhip_groth16_verify (needs no device); route 1: the kernels of zkhip_verifier_verify_batch. */
int zkhip_internal_fq6_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
int zkhip_internal_pairing_product(int route, const uint64_t* g1, const uint64_t* g2, size_t pairs_per_product, size_t count, uint64_t* out);
/* verify_all_value: the REDUCED GT value of zkhip_verifier_verify_all's combined product (6 x 12 ABI limbs; one iff the check passes)
 * for the handle's key; rho is required.  route 0: the host code of zkhip_groth16_verify_all without its curve check; route 1: the
 * device route.  On a handle of zkhip_verifier_new_checked both routes run the point checks first and leave a refused proof out.
 * verify_all_finish_ms: the host's time in the last device-route call on this handle behind the last chunk's synchronisation (the
 * shared pairs and the final exponentiation). */
int zkhip_internal_verify_all_value(int route, zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                                    const uint64_t* rho, uint64_t out[72]);
/* key_check_set_chunk: points per launch of zkhip_crs_check's point kernel, process-wide; 0: the rule (csrc/pairing.cuh
 * key_check_chunk, 2^17).  Lets tests cross chunk boundaries at a few hundred points.
 * key_check_last_ms: of the calling thread's last zkhip_crs_check[_host]: [0] the device time of its longest single point-check launch
 * (0 on the host route), [1] the wall time of all its point checks (staging included), [2] of the two sums of the B relation, [3] of
 * the host's pairings, [4 + e] of the point checks of element e, milliseconds. */
int zkhip_internal_key_check_set_chunk(size_t points);
int zkhip_internal_key_check_last_ms(double out_ms[4 + ZKHIP_KEY_ELEMENTS]);
/* phase2_last_ms: of the calling thread's last phase-2 call: [0] the device time of its longest single launch (contribute: the
 * multiplication kernel, verify: the point check; 0 on the host routes), [3] the whole call, wall time.  contribute: [1] / [2] h_query /
 * l_query (staging included), [4] the copy of the key, [5] delta' in both groups, [6] commitment, response and hashes, [7] the device
 * time of ALL launches of the multiplication kernel (what [1] + [2] exceeds it by is all that overlapping copies could hide).
 * verify: [1] the byte comparison of step 1, [2] the infinity patterns, [4] point checks, [5] four sums, [6] host relations.  Milliseconds.
 * The chunk of the multiplication kernel is the key check's (zkhip_internal_key_check_set_chunk). */
int zkhip_internal_phase2_last_ms(double out_ms[8]);
/* phase2_set_form: which form of the multiplication kernel zkhip_keypair_contribute runs, process-wide: 0 the build's default (the
 * endomorphism form), 2 the same by name, 1 the signed-binary baseline over all of s^-1 - only in a build with
 * -DZKHIP_PHASE2_BOTH_FORMS (tools/phase2_ab.py measures the two against each other), ZKHIP_ERR_STATE otherwise.  Outputs are identical. */
int zkhip_internal_phase2_set_form(int form);
int zkhip_internal_verify_all_finish_ms(const zkhip_verifier* v, double* ms);
/* verify_batch_located: zkhip_verifier_verify_batch_located by route - 1: the device route; 0: the host route of
 * zkhip_groth16_verify_batch_located under the handle's key, without its curve check, and on a checked handle behind the host's point
 * checks, with the handle's kind of verdict bytes.  rho is required.  value (may be NULL): the REDUCED GT value of the batch's combined
 * check, 72 ABI limbs - what zkhip_internal_verify_all_value gives under the same rho (of the last located batch of a call that was cut).
 * locate_trace: every node the last located call on this handle tested (either route; the last located batch of a call that was cut),
 * in the order of the rounds: chunk, level (0: a single proof), index within the level, passed, and the REDUCED value of the node's
 * combined check (6 x 12 ABI limbs; one iff passed).  *count gets the number of nodes; at most cap are written to out (may be NULL). */
typedef struct {
  uint32_t chunk, level, passed, reserved;
  uint64_t index;
  uint64_t value[72];
} zkhip_locate_node;
int zkhip_internal_verify_batch_located(int route, zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                                        const uint64_t* rho, uint8_t* verdict, zkhip_locate_stats* stats, uint64_t* value);
int zkhip_internal_locate_trace(const zkhip_verifier* v, zkhip_locate_node* out, size_t cap, size_t* count);
/* Test hooks of the nested pairing kernels (no counterpart).
 * fq12_selftest: n independent operand sets through the per-lane bodies of pairing_bls.cuh inside a real kernel, sixteen lanes per
 * set: op 0 = a b, 1 = a^2, 2 = a (b_0 + b_1 w + b_3 w^3 + b_7 w^7 + b_9 w^9) (the sparse line product; b's other coefficients are
 * ignored) in Fq12 = Fq[w]/(w^12 + 5) over the nested base field.  a, b, out: n x 12 coefficients x 6 ABI limbs.
 * nested_pairing_product: out[i] = prod_{p < pairs_per_product} e(g1[i][p], g2[i][p]), the REDUCED value f^(3 (q^12 - 1) / r)
 * (12 x 6 ABI limbs, canonical); g1: 12 limbs per point, g2: 24; pairs_per_product in 1 .. 4.  route 0: the host code
 * (multi_miller_loop and final_exponentiation of csrc/circuit/bls12_377.hpp, needs no device); route 1: the kernels of
 * zkhip_nested_verifier_verify_batch.  A point off its curve: ZKHIP_ERR_ARG on both routes. */
int zkhip_internal_fq12_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
int zkhip_internal_nested_pairing_product(int route, const uint64_t* g1, const uint64_t* g2, size_t pairs_per_product, size_t count, uint64_t* out);
/* nested_verify_all_value: the REDUCED GT value of zkhip_nested_verifier_verify_all's combined product over the proofs that are not
 * left out (12 x 6 ABI limbs; one iff the product check passes) for the handle's key; rho is required.  route 0: the host code of
 * zkhip_bls12_377_groth16_verify_all; route 1: the device route.  On a handle of zkhip_nested_verifier_new_checked both routes run the
 * point checks first and leave a refused proof out.  nested_verify_all_finish_ms: the host's time in the last device-route call on this
 * handle behind the last chunk's synchronisation (the sums, the scalar multiplications, the shared pairs, the final exponentiation). */
int zkhip_internal_nested_verify_all_value(int route, zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs,
                                           size_t count, const uint64_t* rho, uint64_t out[72]);
int zkhip_internal_nested_verify_all_finish_ms(const zkhip_nested_verifier* v, double* ms);
/* Test hook (no counterpart), HOST ONLY - works without a device: the prover's tail (row a9) on the paths a healthy proof never
 * takes: `rounds` proofs abandoned between the start of the tail's key-only scalar multiplications and their collection, the key's
 * tables freed at once (run under the CPU AddressSanitizer build); a delta of small order (`small_order_g1`, e.g. (1, 0)) whose
 * fixed-base table must be refused in favour of variable-base products.  g1 / g2: the curve generators, 24 limbs each. */
int zkhip_internal_tail_selftest(const uint64_t g1[24], const uint64_t g2[24], const uint64_t small_order_g1[24], int rounds);
/* Test hooks of the GPU witness generator (no counterpart).  A laid-out straight-line program over Fr as witness.hip interprets it
 * (witness_tape.h has the instruction codes): positions [0, chain_start) in levels of whole 64-position chunks, run by k_witness,
 * positions [chain_start, n_pos) in execution order, run by k_witness_chain; operands >= 0 name an earlier position, < 0 the
 * constant -1 - index; assignment entry i is the value at out_ref[i]. */
typedef struct zkhip_witness_program {
  const uint8_t* code;
  const int32_t* a;
  const int32_t* b;
  size_t n_pos;
  const uint32_t* level_start; /* n_levels + 1 positions, the last one = chain_start */
  size_t n_levels;
  uint32_t chain_start;
  const int32_t* out_ref;
  size_t n_vars;
  const uint64_t* consts; /* n_consts x 6 limbs, ABI form */
  size_t n_consts;
  size_t n_inputs;
} zkhip_witness_program;
/* Runs a caller's program through the product's own upload, launch and kernels: `batches` (0 .. 256) input vectors of n_inputs x 6
 * limbs (ABI form), `witnesses_per_workgroup` 1, 2 or 4, `segment_chunks` chunks of the levelled part per launch (1 .. 2^20).
 * z_out: batches x n_vars x 6 limbs (ABI form, canonical); flags_out: one word per batch, non-zero where a WT_INV met zero.
 * The program is VALIDATED on the host first - every level whole chunks; a levelled operand in an earlier level, a chain operand
 * earlier in the chain and not before chain_start; constant, input and out_ref indices in range; bit index below 384; k of
 * WT_SUBK + k in 1 .. 11; no WT_SUB, no unknown code - and refused with ZKHIP_ERR_ARG before anything is uploaded, so an accepted
 * program cannot address outside its buffers.  batches = 0 validates only and needs no device.  The VALUE contract (bounds of the
 * lazy reduction: sums up to 2^12 r, subtrahends up to 2^k r, inversion operands up to 4 r) is the caller's: breaking it gives
 * wrong values, never a wrong address. */
int zkhip_internal_witness_run_program(const zkhip_witness_program* p, const uint64_t* inputs, size_t batches, int witnesses_per_workgroup,
                                       unsigned segment_chunks, uint64_t* z_out, uint32_t* flags_out);
/* The same with the waves per witness given (zkhip_gpu_witness_set_waves: 0, 1, 2, 4, 8, 16; the hook above passes 1).  The wide
 * kernels run whole levels per launch: the first level boundary at which a launch holds segment_chunks chunks or more. */
int zkhip_internal_witness_run_program_wide(const zkhip_witness_program* p, const uint64_t* inputs, size_t batches, int witnesses_per_workgroup,
                                            unsigned segment_chunks, int waves, uint64_t* z_out, uint32_t* flags_out);
/* HOST ONLY: how a GPU-witness pipeline sizes itself - out[0] witnesses per launch (at most wit_batch, which is 16 or ZKHIP_WIT_BATCH)
 * and out[1] batcher threads (at most workers) such that out[0] x out[1] x value_bytes stays under a quarter of mem_total: the batch
 * is halved first (rounding up, down to one), then batchers are dropped (down to one). */
int zkhip_internal_pipeline_witness_sizing(size_t value_bytes, size_t mem_total, size_t wit_batch, int workers, size_t out[2]);
/* HOST ONLY: the recorded program of the circuit, as zkhip_gpu_witness_run uploads it (pointers into the handle, valid until
 * zkhip_aggregator_free). */
int zkhip_internal_witness_tape(zkhip_aggregator* a, zkhip_witness_program* out);
/* zkhip_gpu_witness_run_batched (app = null) or zkhip_gpu_witness_run_batched_app (nested_vk = null) with the launch's two tuning
 * knobs given by the caller instead of ZKHIP_WITNESS_WPG / ZKHIP_WITNESS_SEGMENT: 0 = the process-wide default. */
int zkhip_internal_gpu_witness_run(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_vk,
                                   const uint64_t* const* nested_proofs, const uint64_t* const* nested_inputs, void* d_z_out,
                                   uint64_t* primary_inputs, int* degenerate, int witnesses_per_workgroup, unsigned segment_chunks);
/* The same with the waves per witness given (0 = auto; the hook above passes 1) */
int zkhip_internal_gpu_witness_run_wide(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_vk,
                                        const uint64_t* const* nested_proofs, const uint64_t* const* nested_inputs, void* d_z_out,
                                        uint64_t* primary_inputs, int* degenerate, int witnesses_per_workgroup, unsigned segment_chunks, int waves);

/* replaces: libff::Fr<wppT>::random_element() as r1cs_gg_ppzksnark_prover draws the proof's randomisers r, s (reached from
 * aggregator_circuit.tcc:168) and the generator its toxic waste: one field element uniform in Fr, 6 Montgomery limbs, from the
 * operating system's entropy source.  Host code. */
int zkhip_fr_random(uint64_t out[6]);

/* Montgomery limbs -> canonical integer limbs (little-endian), for the JSON / EVM encodings of the reference
 * (SURVEY App. A.2, A.3): which = 0 for Fq (12 limbs), 1 for Fr (6 limbs).  Host code. */
int zkhip_to_canonical(int which, const uint64_t* in, uint64_t* out);

/* ---- the GPUs of one node behind one process (multi_device.cpp: host code on the entry points above, no collective) ----------
 * The reference server is ONE process that owns the prover (aggregator_server.cpp:106-118, 279-348, 390-416; OpenMP is its only
 * parallelism, CMakeLists.txt:80-84); a drop-in on an 8-GPU node must drive all eight from that process.  `devices` lists GPU
 * indices; an index may repeat ("0,0": two contexts on GPU 0 - how a one-GPU box rehearses N > 1).  Both constructors call
 * zkhip_init for the GPUs they use and leave the calling thread's library device as they found it.
 *
 * Replicas (BASELINE configs[4], SURVEY 8e "whole proofs"): one resident copy of the key and one streaming pipeline
 * (zkhip_aggregator_pipeline_*) per list entry; submit hands a batch to the entry with the fewest batches outstanding.
 * replaces: aggregator_circuit::prove as GenerateAggregatedTransaction calls it (aggregator_server.cpp:318-319), on every GPU. */
typedef struct zkhip_dispatcher zkhip_dispatcher;
int zkhip_dispatcher_new(zkhip_aggregator* a, const zkhip_crs_desc* key, const zkhip_key_opts* opts, const int* devices, int n_devices,
                         int gpu_slots, int witness_workers, unsigned flags /* ZKHIP_PIPELINE_* */, zkhip_dispatcher** out);
int zkhip_dispatcher_size(const zkhip_dispatcher* d);                          /* entries of the device list */
int zkhip_dispatcher_submit(zkhip_dispatcher* d, const uint64_t* nested_vk, const uint64_t* nested_proofs, const uint64_t* nested_inputs,
                            const uint64_t r[6], const uint64_t s[6], uint64_t* ticket);
int zkhip_dispatcher_wait(zkhip_dispatcher* d, uint64_t ticket, uint64_t* primary_inputs, uint64_t proof_affine[72]);
int zkhip_dispatcher_register_app(zkhip_dispatcher* d, const uint64_t* nested_vk);    /* zkhip_aggregator_pipeline_register_app on every entry */
int zkhip_dispatcher_stats(const zkhip_dispatcher* d, size_t* submitted_per_entry);   /* batches given to each entry so far */
int zkhip_dispatcher_outstanding(const zkhip_dispatcher* d, size_t* per_entry);        /* submitted and not yet collected, per entry */
void zkhip_dispatcher_free(zkhip_dispatcher* d);
/* One proof over a key PARTITIONED across the list (BASELINE configs[3]): entry k holds the k-th contiguous slice of
 * the A / B, H and L queries (equal finite terms per slice: zkhip_key_partition) and a prover instance on it; prove
 * runs the slices on a host thread each, adds the 5 x 288-byte partial sums in list order on the host (zkhip_jac_add) and finishes
 * once (zkhip_groth16_finish).  Same proof as zkhip_groth16_prove over the whole key.
 * replaces: wsnarkT::generate_proof (aggregator_circuit.tcc:168) for a key that one GPU should not hold or prove alone. */
/* How a key is cut for N devices / ranks: cuts[0 .. parts] (parts + 1 values each) of the A / B queries (one range for the three: the
 * weight of an index is the number of its finite bases among A, B-G2, B-G1), of H and of L - contiguous slices of equal FINITE terms
 * (a base at infinity - a third of a real key's B query - produces no bucket entry).  Host code; zkhip_multi_prover_new and
 * zecale_amd/dist.py (one process per GPU) cut by this rule. */
int zkhip_key_partition(const zkhip_crs_desc* key, int parts, size_t* a_cuts, size_t* h_cuts, size_t* l_cuts);
typedef struct zkhip_multi_prover zkhip_multi_prover;
int zkhip_multi_prover_new(const zkhip_crs_desc* key, const zkhip_r1cs_desc* cs, const zkhip_key_opts* opts, const int* devices, int n_devices,
                           zkhip_multi_prover** out);
int zkhip_multi_prover_size(const zkhip_multi_prover* mp);
int zkhip_multi_prover_prove(zkhip_multi_prover* mp, const uint64_t* z, const uint64_t r[6], const uint64_t s[6], uint64_t proof_affine[72]);
/* ms of the last proof: [0] the slowest slice (upload z + QAP map + five MSMs), [1] the host additions, [2] the host tail */
int zkhip_multi_prover_timings(zkhip_multi_prover* mp, double out_ms[3]);
void zkhip_multi_prover_free(zkhip_multi_prover* mp);

/* host helpers on results (tiny, serial): Jacobian -> affine (infinity -> all zero), a + b */
int zkhip_jac_to_affine(const uint64_t jac[36], uint64_t aff[24]);
int zkhip_jac_add(const uint64_t a[36], const uint64_t b[36], uint64_t out[36]);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_H */
