/*
 * b3wit.h — C-ABI of the MI355X-native batched witness generator for the reference's BLAKE3
 * circom circuits (libb3wit.so).  Plain C: pointers and sizes only, no HIP / torch types.
 *
 * Every entry point names the piece of the reference interface it stands in for
 * (paths relative to the reference repo banyancomputer/hot-proofs-blake3-circom):
 *   WC  = blake3_nova_js/witness_calculator.js  (the circom-emitted loader, the drop-in boundary)
 *   WASM exports = the functions WC calls on the compiled circuit instance (same file, cited lines)
 *
 * Status codes: 0 ok; 1..6 are the circom runtime exception codes WC maps to text at
 * WC:21-37 (1 Signal not found, 2 Too many signals set, 3 Signal already set, 4 Assert Failed,
 * 5 Not enough memory, 6 Input signal array access exceeds the size); >= 100 are runtime errors
 * of this library.  No function throws; a ctx / batch is not thread-safe, distinct ones are.
 */
#ifndef B3WIT_H
#define B3WIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Circuits = the committed circom builds of the reference. */
#define B3W_CIRCUIT_COMPRESSION_BN254 0 /* build/blake3_compression/blake3_compression_js/blake3_compression.wasm  N=24093 */
#define B3W_CIRCUIT_NOVA_BN254        1 /* build/blake3_nova_js/blake3_nova.wasm (--prime bn128, O2)               N=23291 */
#define B3W_CIRCUIT_NOVA_VESTA        2 /* build/blake3_nova_pasta_js/blake3_nova_pasta.wasm (--prime vesta, O2)   N=23291 */
#define B3W_CIRCUIT_NOVA_BN254_O1     3 /* build/blake3_nova/blake3_nova_js/blake3_nova.wasm (circomkit build)      N=24614 */
#define B3W_CIRCUIT_UNKNOWN         (-1)

#define B3W_OK                     0
#define B3W_E_SIGNAL_NOT_FOUND     1
#define B3W_E_TOO_MANY_SIGNALS     2
#define B3W_E_SIGNAL_ALREADY_SET   3
#define B3W_E_ASSERT_FAILED        4
#define B3W_E_NOT_ENOUGH_MEMORY    5
#define B3W_E_ARRAY_ACCESS         6
#define B3W_E_BAD_ARGUMENT       100
#define B3W_E_NO_DEVICE          101 /* no HIP device / HIP runtime error: the product has no CPU path */
#define B3W_E_HIP                102
#define B3W_E_DOMAIN             103 /* batch status only: record outside the batch kernels' domain (DESIGN.md "Input domain");
                                        b3w_calc_witness evaluates such inputs with the exact kernel instead */
#define B3W_E_NOT_ALL_INPUTS     104 /* WC:166-168 "Not all inputs have been set" */
#define B3W_E_RCCL               105 /* librccl missing or a collective failed — RCCL's, the host transport's or the caller's
                                        (b3w_last_error has the text) */

typedef struct b3w_ctx b3w_ctx;
typedef struct b3w_batch b3w_batch;

/* Library / ABI version (major<<16 | minor). */
uint32_t b3w_abi_version(void);

/* Which committed circuit is this WASM?  Replaces WebAssembly.compile(code) at WC:7: the
 * builder receives the .wasm bytes; the native path keys on their sha256. */
int32_t b3w_identify_wasm(const uint8_t *code, size_t len);

/* Replaces WebAssembly.instantiate + `new WitnessCalculator(instance, sanityCheck)` (WC:19,78,
 * ctor WC:109-125).  device = HIP device ordinal (>= 0).  Fails with B3W_E_NO_DEVICE when the
 * HIP runtime has no such device — there is no CPU fallback. */
int32_t b3w_create(int32_t circuit, int32_t device, b3w_ctx **out);
void b3w_destroy(b3w_ctx *ctx);

/* WASM exports getFieldNumLen32 / getRawPrime / getWitnessSize / getInputSize /
 * getVersion+getMinorVersion+getPatchVersion (read by the ctor WC:112-122 and WC:166). */
int32_t b3w_info(const b3w_ctx *ctx, uint32_t *n32, uint8_t prime_le[32], uint32_t *witness_size,
                 uint32_t *input_size, uint32_t version[3]);

/* WASM export getInputSignalSize(hMSB,hLSB) (WC:141): number of values the input signal whose
 * FNV-1a-64 name hash (WC:325-337) is `fnv1a64_of_name` takes; 0 when the circuit has no such input. */
int32_t b3w_input_signal_size(const b3w_ctx *ctx, uint64_t fnv1a64_of_name);

/* One witness = WASM exports init + setInputSignal x inputs + getWitness x N as driven by
 * _doCalculateWitness (WC:131-169) and calculateBinWitness (WC:190-205).
 *   name_hashes[k], counts[k] : FNV-1a-64 of the k-th input name and how many values it carries
 *   values_le32               : sum(counts) field elements, 32-byte little-endian, already
 *                               reduced into [0,p) (WC:319-323 normalize), in key order
 *   out_body                  : witness_size*32 bytes, canonical little-endian elements
 * Any field elements are accepted: canonical records run through the batch kernel, everything else
 * through the exact (256-bit field arithmetic) device kernel — both on the GPU.
 * Size errors mirror WC:142-150 (B3W_E_TOO_MANY_SIGNALS / B3W_E_ARRAY_ACCESS /
 * B3W_E_NOT_ALL_INPUTS); a failed circuit assert returns B3W_E_ASSERT_FAILED and b3w_last_error gives
 * the reference WASM's own trace text ("Assert Failed.\nError in template Bits34_1 line: 201\n...").
 * ORDER (WC:136-160): keys are taken as given; per key the size check, then its values; the circuit runs when the
 * last missing input has been set, before the keys BEHIND the completing one are looked at.  So a failed assert
 * wins over the fault of a later key, the fault of an earlier key over the assert; when a later key is refused
 * (an unknown name with values: B3W_E_TOO_MANY_SIGNALS) the circuit HAS run and out_body holds the witness — the
 * JS shim and the Python mirror call with the keys up to the completing one, log what the circuit logs, and look
 * at the rest themselves (tests/golden/order.json, tests/test_order_parity.py). */
int32_t b3w_calc_witness(b3w_ctx *ctx, const uint64_t *name_hashes, const uint32_t *counts,
                         const uint8_t *values_le32, uint32_t nkeys, uint8_t *out_body);

/* The 76-byte .wtns v2 preamble calculateWTNSBin builds at WC:215-262 ("wtns", version 2,
 * 2 sections, section 1 {n8, prime, nWitness}, section 2 id + length). */
int32_t b3w_write_wtns_header(const b3w_ctx *ctx, uint8_t out[76]);

/* Text of the last error on this ctx (the trace WC appends after "Assert Failed.\n", WC:41,38). */
int32_t b3w_last_error(const b3w_ctx *ctx, char *buf, size_t len);

/* ---- batch fast path (no counterpart in the reference: it computes one witness per call) ----
 * Inputs are packed u32 records, all words canonical (< 2^32):
 *   compression (28 words): h[8] m[16] t[2] b d
 *   nova        (32 words): n_blocks block_count h[8] chunk_idx_low chunk_idx_high leaf_depth
 *                           total_depth depth m[16] b
 * Witness bodies stay in HBM: n bodies of witness_size*32 bytes, body i at out + i*pitch.   */

/* Kernel launch only; every pointer is a DEVICE pointer, `stream` is a hipStream_t (NULL = default
 * stream).  No allocation, no synchronisation: safe inside stream capture.
 *   d_records : n * input_size u32                     d_bodies : n * pitch bytes (pitch % 32 == 0,
 *   d_public  : n * public_words u32 or NULL             pitch >= witness_size*32)
 *   d_status  : n int32 or NULL (0 ok, 4 assert failed, 103 outside the fast-path domain) */
int32_t b3w_batch_run_device(b3w_ctx *ctx, const uint32_t *d_records, uint32_t n, uint8_t *d_bodies,
                             uint64_t pitch, uint32_t *d_public, int32_t *d_status, void *stream);

/* Number of u32 public-output words per witness written to d_public: compression 16 (out[16]),
 * nova 15 (w[1..15]: n_blocks_out block_count_out h_out[8] total_depth_out depth_out
 * chunk_idx_low_out chunk_idx_high_out leaf_depth_out). */
uint32_t b3w_public_words(const b3w_ctx *ctx);

/* Convenience wrappers that own device buffers (hipMalloc) for up to `capacity` witnesses. */
int32_t b3w_batch_alloc(b3w_ctx *ctx, uint32_t capacity, uint64_t pitch /* 0 = witness_size*32 */, b3w_batch **out);
void b3w_batch_free(b3w_batch *batch);
/* H2D of n records + kernel on `stream`, then stream sync. */
int32_t b3w_batch_run(b3w_batch *batch, const uint32_t *host_records, uint32_t n, void *stream);
/* D2H of the public outputs (n * public_words u32) and per-witness status (n int32, may be NULL). */
int32_t b3w_batch_outputs(b3w_batch *batch, uint32_t *host_public, int32_t *host_status);
/* D2H of one full body (witness_size*32 bytes). */
int32_t b3w_batch_fetch(b3w_batch *batch, uint32_t index, uint8_t *out_body);
/* Zero-copy handle for on-GPU consumers: device pointer of body 0, and the pitch. */
void *b3w_batch_device_ptr(b3w_batch *batch, uint64_t *pitch);

/* ---- body-buffer placement (no counterpart in the reference) ------------------------------------
 * MI355X HBM consists of three classes of physical memory (DESIGN.md "Placement"): the witness kernels' store
 * pattern — one stream per body — runs about 25 % faster when the bodies being written at any moment are spread
 * over two classes than when they all sit in one, which is where a plain hipMalloc puts them.  b3w_bodies_alloc
 * returns a linear device buffer of at least `bytes` bytes whose 256 MiB pieces alternate between two classes
 * (found by timing short store probes against two reference pieces while the buffer is assembled through the HIP
 * virtual-memory API);
 * *placement reports what was achieved — and "mixed" is only reported when ONE REAL witness launch of this context's
 * circuit into the buffer is at least 10 % faster than into a plain hipMalloc buffer (measured once per context; a buffer
 * that fails the check stays usable and is reported as INTERLEAVED: its pieces do alternate, but on this box, today,
 * plain buffers were as fast — no speed claim; B3W_PLACE_CHECK=0 skips the check).  Use the pointer like
 * any device pointer (kernels, hipMemcpy); release it
 * with b3w_bodies_free.  B3W_PLACEMENT=plain in the environment turns the search off.
 * b3w_batch_alloc places its body buffer this way. */
#define B3W_PLACEMENT_PLAIN 0 /* one class (no search, search failed, or a buffer below 512 MiB) */
#define B3W_PLACEMENT_MIXED 1 /* alternating classes, and measured >= 10 % faster than plain buffers */
#define B3W_PLACEMENT_INTERLEAVED 2 /* alternating classes, measured gain below 10 % (this box's plain buffers were fast themselves) */
int32_t b3w_bodies_alloc(b3w_ctx *ctx, uint64_t bytes, void **d_ptr, int32_t *placement);
int32_t b3w_bodies_free(b3w_ctx *ctx, void *d_ptr);
/* The allocator keeps up to 3 x 12 GiB of classified-but-unused physical memory per device for the next buffer (and two
 * 256 MiB reference pieces for good); b3w_bodies_trim returns that reserve to the driver. */
void b3w_bodies_trim(void);
/* Memory a CONTEXT keeps: when a b3w_chain is destroyed its ring buffers (batch_steps bodies each — 12 GB for 16 384 nova steps)
 * stay with the context for the next chain of the same ring geometry, because placed buffers use up address space for good.
 * Bounds: spares of one ring size at a time (a chain of another geometry releases them first) and at most 26 GiB in all.
 * Neither torch nor RCCL can see that memory; b3w_ctx_trim(ctx) releases it (to the placement pool — follow with
 * b3w_bodies_trim to hand it to the driver), b3w_destroy does the same. */
int32_t b3w_ctx_trim(b3w_ctx *ctx);
/* Bounds of the placement allocator, in GiB (negative = leave as is): `search_gib` = new physical memory one search may
 * touch transiently beyond the buffer itself (default and most: 160, and never more than half of what is free — released again at
 * the end of the search; what ends a search first is its time limit, b3w_bodies_search_limit); `pool_gib` = labelled memory kept pooled for later buffers, all three labels together (default 12).
 * Also B3W_PLACE_SEARCH_GIB / B3W_PLACE_POOL_GIB in the environment.  Other allocators in the process (torch, RCCL) cannot
 * see pooled memory: b3w_bodies_trim hands it back. */
void b3w_bodies_configure(int64_t search_gib, int64_t pool_gib);
/* What placement costs.  A search ends — and the buffer is plain — when it has not found a second class of memory after
 * `seconds` (default 5; B3W_PLACE_SEARCH_S; <= 0 = no limit) as well as when it runs out of its GiB budget.
 * b3w_bodies_search_stats: out[0] = seconds spent inside searching b3w_bodies_alloc calls on the ctx's device so far (probes,
 * seam checks), out[1] = GiB of new physical memory those searches created (most of it released again), out[2] = searches that
 * ended on the time limit, out[3] = the time limit, out[4] = seconds spent in the real-kernel check of "mixed" buffers (the three
 * plain yardstick buffers are measured once per context). */
void b3w_bodies_search_limit(double seconds);
int32_t b3w_bodies_search_stats(const b3w_ctx *ctx, double out[5]);
/* Where a search's time goes: seconds this process has spent inside hipMemCreate (out[0]), hipMemMap + hipMemSetAccess (out[1]), the
 * timed store probes (out[2]) and hipMemUnmap + hipMemRelease (out[3]) on the ctx's device.  The first is the driver's: a call
 * returns in microseconds until the process's footprint crosses some tens of GiB and then one call takes seconds
 * (profiles/r05/place_cost.log). */
int32_t b3w_bodies_search_breakdown(const b3w_ctx *ctx, double out[4]);
/* Harness helper: the pure-store ceiling of a body buffer — GB/s of `iters` passes (after 2 untimed ones) of kernels that do
 * nothing but the witness kernels' stores into n bodies at d_bodies + i * pitch (16-byte aligned; pitch 0 = witness_size * 32):
 * shape 0 = body streams, one wave per 4 bodies and 1 KiB per body and step (the fused kernels' EXPAND phase without trace, slot
 * table or LDS), 1 = the same per 8 bodies, 2 = the runtime's fill shape (256 workgroups over 4 KiB tiles; the sweep kernels'),
 * 3 / 4 = PACED persistent body streams (512 single-wave workgroups taking groups of 4 / 8 bodies in turn, four vector-ALU instructions
 * in front of every store: a store-only kernel without any issues faster than HBM drains and fills it SLOWER — the best store-only
 * shapes of tools/ubench/store_sweep.hip on a placed buffer), 5 = 8 bodies per wave, paced, one wave per group, 6 / 7 = the fill-ordered
 * witness kernel's store order (variant 200: one contiguous 4 MiB window chip-wide) paced by s_sleep / by vector-ALU instructions (the best of five / six
 * paces each: the rate is a cliff in the pace) — the only store-only shapes that fill a caller's plain buffer as fast as a placed one (7.0 TB/s).
 * What a witness kernel's achieved bandwidth on the SAME buffer is to be read against (bench.py: roofline.of_measured_ceiling).
 * HIP events on `stream`; waits for them.  The buffer's contents are overwritten. */
int32_t b3w_bodies_store_rate(b3w_ctx *ctx, void *d_bodies, uint32_t n, uint64_t pitch, int32_t shape, uint32_t iters, void *stream,
                              double *gb_per_s);
/* out[0] address-space arena of the ctx's device in bytes, out[1] of it used up (never reused), out[2] pooled bytes,
 * out[3] bytes of live placed buffers, out[4] their number, out[5] physical 256 MiB handles created so far. */
int32_t b3w_bodies_stats(const b3w_ctx *ctx, uint64_t out[6]);
/* Placement of a batch's own body buffer. */
int32_t b3w_batch_placement(const b3w_batch *batch);

/* Timing helper for harnesses: records HIP events around `iters` back-to-back launches of the
 * batch kernel on `stream` and returns the average kernel time in milliseconds (device pointers
 * as in b3w_batch_run_device). */
int32_t b3w_batch_time_device(b3w_ctx *ctx, const uint32_t *d_records, uint32_t n, uint8_t *d_bodies,
                              uint64_t pitch, uint32_t *d_public, int32_t *d_status, void *stream,
                              uint32_t iters, float *avg_ms);

/* On-device consumer #1: the rank-1 constraint check  <A_k, z> * <B_k, z> - <C_k, z> = 0  for every constraint k of an
 * R1CS and every witness body z in HBM — what the reference's consumers do with a witness first: circom_tester's
 * expectPass / checkConstraints (test/blake3_hash.test.ts:36) and synthesize_with_vec, which enforces every R1CS row over
 * the witness variables (rust_fold/src/utils.rs:17-88, rows read from the circuit's .r1cs by circom-scotia).
 * The constraint system is the caller's: `r1cs_image` is a complete iden3 .r1cs file image (format version 1: header,
 * constraints, wire map) over the ctx's field with nWires = witness_size — the circuit's own .r1cs where the maintainer
 * has it (the reference checkout does not: .MISSING_LARGE_BLOBS), or one this repository derives (tools/gen_r1cs.py ->
 * hot-proofs-blake3-circom_amd/constraints/: blake3_compression.r1cs.gz and blake3_nova_bn254_o1.r1cs.gz from the circuit
 * text with circom's signal numbering rule; blake3_nova_bn254.r1cs.gz and blake3_nova_vesta.r1cs.gz — the O2 builds — by
 * aligning the reference's O2 witnesses with its O1 witnesses and eliminating the missing wires; gunzip first).
 * The check is independent of the witness kernels: full field arithmetic on the 32-byte elements as they lie in the
 * body, no knowledge of the circuit beyond the file.
 *   d_violations[i] = number of constraints body i violates (0 = a valid witness); an element >= p counts as a violation
 *                     of every constraint that reads it;   d_first[i] (may be NULL) = lowest violated constraint index
 *                     (file order), 0xFFFFFFFF if none. */
typedef struct b3w_r1cs b3w_r1cs;
int32_t b3w_r1cs_create(b3w_ctx *ctx, const uint8_t *r1cs_image, size_t len, b3w_r1cs **out);
int32_t b3w_r1cs_info(const b3w_r1cs *r1cs, uint32_t *n_constraints, uint32_t *n_wires, uint64_t *n_terms,
                      uint32_t *n_pub_out, uint32_t *n_pub_in, uint32_t *n_prv_in);
/* Which formulation the checks of this system take: 1 = the tile kernels (rows local enough: at most 1 024 wires outside
 * any tile of 1 024 consecutive wires — every circom circuit seen so far), 0 = the gather kernel (any system). */
int32_t b3w_r1cs_is_tiled(const b3w_r1cs *r1cs);
void b3w_r1cs_destroy(b3w_r1cs *r1cs);
/* d_bodies 16-byte aligned, pitch a multiple of 16 (0 = witness_size * 32).
 * Stream capture: b3w_batch_run_device, b3w_batch_verify_device and b3w_r1cs_check_device only enqueue kernels on `stream`
 * (no allocation, no synchronisation, no memset nodes), so a caller may capture a loop of small batches into a hipGraph and
 * replay it (tests/test_gpu_graph_capture.py); b3w_batch_commit_device too once its scratch has grown to the batch size, and
 * b3w_r1cs_check_device after its first call on that stream (which allocates the stream's deferred-row scratch, a fixed
 * 27 MB for these systems): check once before capturing — a first check on a stream that is being captured is refused
 * (B3W_E_BAD_ARGUMENT, b3w_last_error says why) instead of allocating inside the capture.  A system keeps the scratch of at most
 * eight streams: when a ninth comes, the least recently used one is released once its last check has finished (streams seen
 * under capture keep theirs until b3w_r1cs_destroy).  One check at a time per stream. */
int32_t b3w_r1cs_check_device(b3w_ctx *ctx, const b3w_r1cs *r1cs, const uint8_t *d_bodies, uint32_t n, uint64_t pitch,
                              uint32_t *d_violations, uint32_t *d_first, void *stream);
/* The same on the witnesses of the last b3w_batch_run; host arrays of n entries (host_first may be NULL). */
int32_t b3w_batch_r1cs_check(b3w_batch *batch, const b3w_r1cs *r1cs, uint32_t *host_violations, uint32_t *host_first);
/* A ready-made consumer for the chained pass (b3w_chain_run_leaves / run_parents): checks every batch of step witnesses
 * against the step circuit's constraints while it sits in the ring — synthesize_with_vec's job (rust_fold/src/utils.rs:17-88)
 * for every step of the fold.  `user` = a b3w_r1cs_sink; d_violations has room for every step of the pass (step order).
 * `next` / `next_user` (may be NULL) name a second consumer that runs on the same batch afterwards, e.g. b3w_commit_consumer
 * with its b3w_commit_sink: witness -> constraint check -> commitment, nothing but counts and points kept. */
typedef struct {
  b3w_ctx *ctx;
  const b3w_r1cs *r1cs;
  uint32_t *d_violations;
  void (*next)(void *user, const uint8_t *d_bodies, uint64_t pitch, uint64_t first_step, uint32_t count, void *stream);
  void *next_user;
  int32_t error; /* first non-zero status of a check launch, 0 = none */
} b3w_r1cs_sink;
void b3w_r1cs_consumer(void *user, const uint8_t *d_bodies, uint64_t pitch, uint64_t first_step, uint32_t count, void *stream);

/* A cheaper tamper check of n witness bodies in HBM (NOT independent evidence: it shares the witness kernels' trace code
 * and slot table).  The circuits are deterministic (the inputs fix every
 * signal), so a body satisfies all constraints iff it equals the witness recomputed from its own input
 * slots; the kernel reads each body once (HBM-read bound) and compares every 16-byte unit.
 * d_mismatch[i] = number of differing units of body i: 0 = valid witness; 0xFFFFFFFF = the body's inputs are
 * rejected by the circuit, are not plain 32-bit values, or make a record that b3w_batch_run_device answers with 103
 * (outside this path's domain: DESIGN.md "Input domain" has the closed-form rule).
 * The record is read from the FIRST slot the layout gives each input atom — compression: slots 17..44; nova: word 0 from slot 1,
 * words 1..9 from 17..25, 10..13 from 13, 14, 15, 11, words 14..31 from 28..45, i.e. for words 0 and 10..13 from the public OUTPUTS
 * that share the input's atom (n_blocks_out, chunk_idx_low_out, chunk_idx_high_out, leaf_depth_out, total_depth_out).  Every other
 * copy of an input atom (nova slots 16, 26, 27) is compared like any slot: tampered alone it counts as one differing unit.  Stands where the
 * reference's consumers check a witness against the R1CS (circom_tester expectPass, test/blake3_hash.test.ts:36;
 * synthesize_with_vec's constraints, rust_fold/src/utils.rs:17-88). */
int32_t b3w_batch_verify_device(b3w_ctx *ctx, const uint8_t *d_bodies, uint32_t n, uint64_t pitch, uint32_t *d_mismatch,
                                void *stream);

/* On-device consumer #2: Pedersen commitments C_i = sum_s w_i[s] * G[s - first_slot] over slots s >= first_slot of n
 * witness bodies in HBM — what the folding prover does with a step witness right after `synthesize`
 * (rust_fold/src/main.rs:166-179 -> arecibo's prove_step commits to W).  The group is the one
 * whose scalar field is the circuit's field: BN254 G1 for the bn128 circuits, the Pallas curve for the --prime vesta
 * build (short Weierstrass, a = 0).  The generators are the caller's (arecibo's commitment key): affine points,
 * x then y, 32-byte little-endian each, standard (non-Montgomery) form, one per committed slot.
 * b3w_commit_key_create precomputes 2^k * G for the slots that hold more than one bit, so committing a witness is
 * "add the points of its set bits" (no doublings).  Output: n affine points (x, y as above; all zero = the point
 * at infinity); d_status (may be NULL): 0 ok, 103 = the body is outside the key's DOMAIN (not a body of the batch kernels).
 * The domain is a rule about the committed slots' values, each slot's 32 bytes taken as a little-endian 256-bit integer, by the
 * slot's class under the key (b3w_slot_widths and, for a folded key, folded[]):
 *   a bit slot (width 1)                          holds 0 or 1;
 *   a 32-bit slot, also one cut down to one bit
 *   of its word by folded[] = 0x80 | i            holds a value below 2^32 (the key then commits bit i of it);
 *   a 64-bit slot                                 holds a value below 2^64;
 *   a 256-bit slot (the IsZero inverses too)      holds anything, values >= p included: the integer is committed as it stands,
 *                                                 which is the commitment of its residue on the curve whose order is the prime;
 *   a slot folded away (folded[] = 1)             holds anything: it is not read and commits nothing;
 *   a slot below first_slot                       never matters.
 * A body inside the domain gets exactly sum_s committed[s] * G[s - first_slot]; it need not be a witness of the circuit.  A body
 * outside it gets status 103 and an UNSPECIFIED point (with d_status NULL there is no telling which points those are); the other
 * bodies of the launch are not affected.  b3w_commit_key_counts counts a flagged body as well: the non-zero windows of the low bits
 * its slots' classes keep.  tests/commit_domain_ref.py states this rule in plain integers. */
#define B3W_CURVE_BN254_G1 0 /* y^2 = x^3 + 3 over q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47 */
#define B3W_CURVE_PALLAS   1 /* y^2 = x^3 + 5 over 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001: the Pallas curve
                               * (pasta_curves; generator (-1, 2)), whose SCALAR field is the prime circom calls "vesta" — the group
                               * arecibo's PallasEngine commits in for the --prime vesta build (rust_fold/src/main.rs:366) */
#define B3W_CURVE_VESTA    B3W_CURVE_PALLAS /* older name of the same id, after the circuit's prime; kept for source compatibility */
typedef struct b3w_commit_key b3w_commit_key;
int32_t b3w_commit_key_create(b3w_ctx *ctx, int32_t curve, uint32_t first_slot, const uint8_t *host_generators, b3w_commit_key **out);
/* The same with the table's window width chosen by the caller: every `window_bits` consecutive bits of the witness share one
 * table of 2^window_bits - 1 precomputed subset sums.  12: 1.2-1.3 GB of HBM, 0.03 s set-up;  16: 14-15 GB, 0.3 s, a
 * quarter fewer point additions per witness (+15-18 % throughput);  18 (r05): 51 GB for an unfolded nova key, 25 for a folded
 * one, 1 s, another ninth fewer additions (+7.6 %) — HBM spent for VALU work on a 288 GB card.  0 = automatic
 * (b3w_commit_key_create): the environment's B3W_COMMIT_WINDOW, else the widest of 18, 16, 12 whose table takes at most a
 * quarter of the free device memory. */
int32_t b3w_commit_key_create_ex(b3w_ctx *ctx, int32_t curve, uint32_t first_slot, const uint8_t *host_generators, uint32_t window_bits,
                                 b3w_commit_key **out);
/* FOLDED keys.  A witness satisfies its circuit's LINEAR constraints, so a slot that is a linear combination of others — every
 * 32-bit word of these circuits is the sum of its bit slots — need not be committed by itself: with w_k = sum_j a_kj w_j,
 * w_k G_k = sum_j w_j (a_kj G_k), i.e. the caller adds a_kj G_k to the generator of slot j once and marks slot k as folded
 * (folded[k - first_slot] != 0: no table windows, the slot's bytes are not even read for their value).  The commitment of every
 * body that satisfies those relations is the same point; half of the point additions are gone (46 289 -> 23 377 virtual slots
 * for blake3_compression).  folded[k] = 0x80 | i keeps ONE virtual slot of a 32-bit word: bit i of its value, with the generator
 * given for it (the O2 builds: a word is 31 bit slots + 2^i * the bit circom's O2 pass took out of the witness).
 * A body that violates the relations (not a witness) gets the commitment of the witness its remaining slots
 * determine: run the constraint check where that matters.  The Python binding derives the relations from an .r1cs image and folds
 * the generators (fold.py: CommitKey(..., fold=image)).  b3w_slot_widths: bits a slot can hold (1, 32, 64, 256) as the
 * commitment kernel cuts it into virtual slots. */
int32_t b3w_commit_key_create_folded(b3w_ctx *ctx, int32_t curve, uint32_t first_slot, const uint8_t *host_generators,
                                     const uint8_t *folded /* witness_size - first_slot flags, or NULL */, uint32_t window_bits,
                                     b3w_commit_key **out);
int32_t b3w_slot_widths(b3w_ctx *ctx, uint16_t *out_bits /* witness_size */);
uint32_t b3w_commit_key_window(const b3w_commit_key *key);     /* 12, 16 or 18 */
/* Statistics for harnesses: while counting is on (on != 0 resets and starts, 0 stops; both wait for the device), every commit
 * launch with this key adds its number of mixed point additions (one per non-zero window and per tabulated inverse: 8 field
 * multiplications + 2 squarings each — the work the kernel's VALU roofline is priced in) to a device counter.
 * b3w_commit_key_counts: out[0] = additions, out[1] = witnesses committed, since counting was switched on (waits for the device). */
int32_t b3w_commit_key_count(b3w_commit_key *key, int32_t on);
int32_t b3w_commit_key_counts(const b3w_commit_key *key, uint64_t out[2]);
void b3w_commit_key_destroy(b3w_commit_key *key);
/* d_bodies and d_points 16-byte aligned, pitch a multiple of 16 (0 = witness_size * 32). */
int32_t b3w_batch_commit_device(b3w_ctx *ctx, const b3w_commit_key *key, const uint8_t *d_bodies, uint32_t n, uint64_t pitch,
                                uint8_t *d_points /* n * 64 bytes */, int32_t *d_status, void *stream);
/* The same for the witnesses of the last b3w_batch_run; host_points receives n * 64 bytes, host_status n int32 (may be NULL). */
int32_t b3w_batch_commit(b3w_batch *batch, const b3w_commit_key *key, uint8_t *host_points, int32_t *host_status);

/* Commitments straight from the input records, without the witness bodies: a witness is an expansion of a 3.7-11 KB
 * trace image through the slot table, so its bits — all the commitment needs — are pieces of image words.  Equal to
 * b3w_batch_run_device followed by b3w_batch_commit_device, at the speed of the point additions alone (the 771 KB body
 * is neither written nor read).  d_public (may be NULL) and d_status (required) receive what b3w_batch_run_device
 * writes; a record whose status is not 0 gets the point at infinity (all zero).
 * O2 nova circuits: the 67 IsZero inverses of a step (256 virtual bit slots each, 39 % of a folded key) are 1/k of small signed
 * k the record determines, so the key also holds, per gadget, the points (+-1/k) G for |k| <= 2 047 (18 MB, 10 ms of set-up)
 * and this path adds ONE point per gadget instead of sixteen windows; a larger |k| goes through the windows as before.
 * b3w_batch_commit_device does the same with bodies: k from the body's input slots, the point taken only when the body's inverse
 * slot holds exactly +-1/k — a body that says anything else is committed to as it stands.
 * Same points either way (tests/test_gpu_commit.py); B3W_COMMIT_INVTAB=0 builds keys without the tables. */
int32_t b3w_commit_records_device(b3w_ctx *ctx, const b3w_commit_key *key, const uint32_t *d_records, uint32_t n, uint8_t *d_points,
                                  uint32_t *d_public, int32_t *d_status, void *stream);

/* The same from and to host buffers (n records of 28 / 32 words; n * 64 bytes of points; public outputs and status may be NULL). */
int32_t b3w_commit_records(b3w_ctx *ctx, const b3w_commit_key *key, const uint32_t *host_records, uint32_t n, uint8_t *host_points,
                           uint32_t *host_public, int32_t *host_status);

/* A ready-made consumer for the chained pass (b3w_chain_run_leaves / run_parents below): commits every batch of step
 * witnesses while it sits in the ring, so that of a 28 TB pass only one 64-byte point per step is kept.
 * `user` = a b3w_commit_sink whose d_points has room for every step of the pass (n_leaf + n_parent points, step order);
 * d_status may be NULL. */
typedef struct {
  b3w_ctx *ctx;
  const b3w_commit_key *key;
  uint8_t *d_points;
  int32_t *d_status;
  int32_t error; /* first non-zero status of a commit launch, 0 = none */
} b3w_commit_sink;
void b3w_commit_consumer(void *user, const uint8_t *d_bodies, uint64_t pitch, uint64_t first_step, uint32_t count, void *stream);

/* Same check on the witnesses of the last b3w_batch_run; host_mismatch receives n counts. */
int32_t b3w_batch_verify(b3w_batch *batch, uint32_t *host_mismatch);

/* Streaming .wtns writer (the hand-off the reference does one file at a time: generate_witness.js:15-18,
 * circomkit `witness` in test/witness_gen.test.ts:41, then `snarkjs groth16 prove` reads the file, :47-49): witnesses
 * [first, first+count) of the last b3w_batch_run are copied to the host through two pinned staging buffers (D2H of chunk
 * k+1 overlaps the file writes of chunk k) and written as <dir>/<prefix><index>.wtns, each byte-identical to
 * calculateWTNSBin's image (76-byte header + body, one writev per file).  The files are written by `threads` writer threads
 * (0 = B3W_WTNS_THREADS, else min(16, cores)).  Witnesses whose status is not 0 are skipped.  Returns the number of files
 * written in *written.  Rates: profiles/r04/wtns_writer.log (PCIe D2H alone: about 56 GB/s = 72 k witnesses/s). */
int32_t b3w_batch_write_wtns(b3w_batch *batch, uint32_t first, uint32_t count, const char *dir, const char *prefix,
                             uint32_t *written);
int32_t b3w_batch_write_wtns_ex(b3w_batch *batch, uint32_t first, uint32_t count, const char *dir, const char *prefix,
                                uint32_t threads, uint32_t *written);

/* Choose the fastest bit-identical kernel variant for THIS output buffer: the body-stream kernels (variants 0 / 3 / 8: fastest
 * on a buffer from b3w_bodies_alloc), the fill-ordered fused kernel (200; compression circuit and nova O2 builds: fastest on a
 * caller's own plain hipMalloc / torch buffer — 7.0-7.2 against 5.5 TB/s on one-class memory — and the default there even without
 * this call), the same paced lighter (201: fastest of all where its pace holds, which only a measurement on
 * the buffer says) and the two-kernel sweep path (100), DESIGN.md "Witness kernels".  An integrator that brings its own buffers calls this once per (context, buffer).  Runs and times each candidate on the caller's device
 * buffers, which end up holding the correct witnesses, and keeps the winner in the ctx for later
 * b3w_batch_run_device calls of more than 2 560 witnesses.  Batches up to 2 560 witnesses follow the default policy — SLICED
 * (several waves per body, DESIGN.md "Batch size") or, from 128 witnesses / 512 nova steps on, the fill order — unless B3W_VARIANT says otherwise; for such an n the call only times that
 * shape and reports it (*chosen_variant = 20 + waves per body).  Allocates the sweep scratch on first use; not for stream
 * capture. */
int32_t b3w_batch_autotune_device(b3w_ctx *ctx, const uint32_t *d_records, uint32_t n, uint8_t *d_bodies,
                                  uint64_t pitch, uint32_t *d_public, int32_t *d_status, void *stream,
                                  int32_t *chosen_variant, float *chosen_ms);

/* ---- chained ("nova fold") mode: step-input planner -----------------------------------------
 * Device counterpart of the reference's per-step input construction: Blake3BlockCompressCircuit::
 * {new, update_for_step, format_input} (rust_fold/src/blake3_circuit.rs:160-289), Blake3CompressPubIO::new
 * (:83-110) and the sibling-CV extraction of hash_with_path (rust_fold/src/blake3_hash.rs:17-93).
 * Because the chaining value is plain BLAKE3, the records of ALL steps of ALL chunks are produced
 * by a native pre-pass and every step witness becomes independent (b3w_batch_run_device on the
 * records).  Records use the nova batch input format.  All pointers are device pointers. */
uint64_t b3w_chain_num_chunks(uint64_t preimage_len);       /* ceil(len / 1024), at least 1 */
uint64_t b3w_chain_num_leaf_steps(uint64_t preimage_len);   /* total number of 64-byte blocks */
uint32_t b3w_chain_path_len(uint64_t chunk, uint64_t n_chunks); /* parents above `chunk` in BLAKE3's tree */

/* Leaf steps of chunks [first_chunk, first_chunk + n_chunks_local): 16 records per chunk (fewer for the
 * last, partial chunk), record j of chunk c at d_records + ((c - first_chunk)*16 + j)*32 words; the chunk
 * chaining values (8 words each) go to d_chunk_cvs.  d_preimage points at byte first_chunk*1024. */
int32_t b3w_chain_plan_leaves_device(b3w_ctx *ctx, const uint8_t *d_preimage, uint64_t preimage_len, uint64_t first_chunk,
                                     uint32_t n_chunks_local, uint32_t *d_records, uint32_t *d_chunk_cvs, void *stream);

/* BLAKE3 tree over n_chunks chunk CVs.  d_levels: (2*n_chunks + 64) * 8 words; the caller fills level 0
 * (words [0, 8*n_chunks)) with the chunk CVs, level j+1 follows level j.  d_root receives the root
 * chaining value = the BLAKE3 hash words (for n_chunks == 1 the chunk CV already is the root). */
int32_t b3w_chain_tree_device(b3w_ctx *ctx, uint32_t *d_levels, uint64_t n_chunks, uint32_t *d_root, void *stream);

/* Parent steps of the paths of chunks [first_chunk, +n_chunks_local), for ANY chunk count, planned the way the
 * reference's driver plans them (hash_with_path, rust_fold/src/blake3_hash.rs:58-84: the PathNode at height g carries the
 * node's right child CV when bit g of the chunk index is clear, else its left child CV; format_input, blake3_circuit.rs:
 * 230-245: that CV as m[0..7], zeros above, b = 64; h and depth come from the previous step).  Chunk c gets
 * b3w_chain_path_len(c, n) records, bottom up (record g: height g, depth = path_len - 1 - g), starting at row
 * b3w_chain_parent_row(c, n) - b3w_chain_parent_row(first_chunk, n) of d_records; in a complete tree that is row
 * (c - first_chunk) * log2(n).  The step circuit takes left/right from the same index bits (Blake3GetDownLeftPath,
 * circuits/blake3_nova.circom:47-84), which is the leaf's real position only when b3w_chain_path_provable(c, n) = 1
 * (every leaf of a complete tree; in an incomplete tree the leaves of the leading power-of-two subtree and those later ones
 * whose position happens to agree): exactly those paths end in h_out = BLAKE3(preimage).  For the other leaves the records are
 * still the reference's, and so is the (wrong) final value — tests/golden/incomplete_trees.nova_vesta.json holds the
 * reference WASM's transcript.  d_levels must have been through b3w_chain_tree_device. */
uint64_t b3w_chain_num_parent_steps(uint64_t preimage_len, uint64_t first_chunk, uint64_t n_chunks_local);
uint64_t b3w_chain_parent_row(uint64_t chunk, uint64_t n_chunks);       /* chunk == n_chunks: the total */
int32_t b3w_chain_path_provable(uint64_t chunk, uint64_t n_chunks);
int32_t b3w_chain_plan_parents_device(b3w_ctx *ctx, const uint32_t *d_levels, uint64_t n_chunks, uint64_t preimage_len,
                                      uint64_t first_chunk, uint32_t n_chunks_local, uint32_t *d_records, void *stream);

/* ---- multi-GPU exchange: RCCL over xGMI, for hosts that do not bring their own collectives ------------
 * One process per GPU.  Witness bodies never leave the GPU that produced them; what the fold needs
 * from every rank are the per-step public outputs (h_out ...: 15 or 16 words per step) and, in chained mode, the
 * chunk chaining values (8 words per chunk).  b3w_comm_allgather is ncclAllGather on the caller's stream.
 * librccl is loaded at run time on first use (an RCCL already loaded into the process is reused).
 *   rank 0:  b3w_comm_unique_id(id)  -> hand the 128 bytes to the other ranks (file, socket, environment)
 *   all:     b3w_comm_create(ctx, id, rank, nranks, &comm)
 *            b3w_comm_allgather(comm, d_local, d_all, bytes_per_rank, stream)     d_all = nranks * bytes_per_rank
 * The Python harness uses torch.distributed ("nccl" = RCCL) for the same exchange instead. */
typedef struct b3w_comm b3w_comm;
#define B3W_COMM_ID_BYTES 128
int32_t b3w_comm_unique_id(uint8_t id[B3W_COMM_ID_BYTES]);
int32_t b3w_comm_create(b3w_ctx *ctx, const uint8_t id[B3W_COMM_ID_BYTES], int32_t rank, int32_t nranks, b3w_comm **out);
/* Two more transports behind the same b3w_comm, so that everything below that takes one — b3w_batch_allgather_public,
 * b3w_chain_run_parents_sharded, b3w_chain_allgather_hout[_host] — also runs where RCCL cannot: several ranks on ONE GPU
 * (rehearsals of an N-GPU job, tests of the rank > 0 paths), hosts without librccl, or a caller that already has collectives.
 *   b3w_comm_create_host      the processes of one host, through a POSIX shared-memory segment: every rank passes the same
 *                             `name` ("/something-unique-to-the-job"; rank 0 creates the segment, the others wait for it, the
 *                             name is removed again once all are attached).  An all-gather is D2H into pinned memory, the
 *                             segment, H2D — it WAITS for `stream` (not for stream capture).  Every wait gives up after
 *                             B3W_HOSTCOMM_TIMEOUT_S seconds (default 120) with B3W_E_RCCL on all ranks.
 *   b3w_comm_create_external  the caller's collective: `allgather(user, d_send, d_recv, bytes_per_rank, stream)` must leave
 *                             d_recv[r * bytes_per_rank ..) = rank r's d_send[0 .. bytes_per_rank) for every r, ordered on `stream`
 *                             like a kernel launched there (it may also simply wait for the stream), and return 0; any other
 *                             value fails the calling entry point with B3W_E_RCCL.  Device pointers; called on the thread
 *                             that called into the library, with ctx's device current. */
typedef int32_t (*b3w_allgather_fn)(void *user, const void *d_send, void *d_recv, uint64_t bytes_per_rank, void *stream);
int32_t b3w_comm_create_host(b3w_ctx *ctx, const char *name, int32_t rank, int32_t nranks, b3w_comm **out);
int32_t b3w_comm_create_external(b3w_ctx *ctx, int32_t rank, int32_t nranks, b3w_allgather_fn allgather, void *user, b3w_comm **out);
int32_t b3w_comm_rank(const b3w_comm *comm);
int32_t b3w_comm_size(const b3w_comm *comm);
void b3w_comm_destroy(b3w_comm *comm);
int32_t b3w_comm_allgather(b3w_comm *comm, const void *d_send, void *d_recv, uint64_t bytes_per_rank, void *stream);
/* The public outputs of the last b3w_batch_run of every rank (all ranks ran the same number n of witnesses):
 * host_all receives nranks * n * public_words u32 in rank order.  Device-side gather + one D2H. */
int32_t b3w_batch_allgather_public(b3w_batch *batch, b3w_comm *comm, uint32_t *host_all);

/* ---- chained mode: the whole pass, natively ---------------------------------------------------
 * What rust_fold/src/main.rs:41-203 does one step at a time for one chunk path, for ALL steps of the chunk range
 * [first_chunk, first_chunk + n_chunks_local) of a preimage (one rank's share; a single GPU takes all chunks):
 *   b3w_chain_run_leaves   pageable or pinned host slices of the preimage -> HBM on a copy stream, overlapped with
 *                          the leaf planner and the nova witness kernels of earlier slices on `stream`
 *   (multi-GPU: all-gather the chunk chaining values of b3w_chain_local_cvs across ranks — 32 B per chunk)
 *   b3w_chain_run_parents  BLAKE3 tree over all chunk CVs, parent-step records of the local chunks' paths (any chunk
 *                          count: b3w_chain_plan_parents_device), their witnesses
 * Witness bodies go through a ring of `ring` placed buffers (b3w_bodies_alloc) of `batch_steps` bodies each: a
 * 1 GiB preimage is 28 TB of witness.  After each batch `consumer` (may be NULL) is called with the device pointer
 * of the batch; it must enqueue its work on `stream` — the buffer is overwritten `ring` batches later.
 * Step records, public outputs (15 words per step) and status live in device arrays owned by the object: leaf
 * steps first (chunk order, block order), then the parent steps (chunk order, height order).  Nothing is
 * synchronised: results are valid once `stream` has drained. */
typedef struct b3w_chain b3w_chain;
typedef void (*b3w_batch_consumer)(void *user, const uint8_t *d_bodies, uint64_t pitch, uint64_t first_step, uint32_t count,
                                   void *stream);
int32_t b3w_chain_create(b3w_ctx *ctx, uint64_t preimage_len, uint64_t first_chunk, uint32_t n_chunks_local,
                         uint32_t batch_steps, uint32_t ring, int32_t with_parents, b3w_chain **out);
void b3w_chain_destroy(b3w_chain *chain);
/* Commitments only: from now on the pass computes one commitment per step straight from the step records
 * (b3w_commit_records_device) into d_points (n_leaf + n_parent points of 64 bytes, step order) and writes no witness
 * bodies; the consumer arguments of the run calls are ignored.  key = NULL switches back to bodies. */
int32_t b3w_chain_commit_only(b3w_chain *chain, const b3w_commit_key *key, uint8_t *d_points);
/* The same commitments (from the step records, at the speed of the point additions) WHILE the bodies are written as usual —
 * constraint check and consumers see every batch: the fold-shaped pass "witness -> check -> commit" where the commitment does not
 * read the 745 KB body back (b3w_batch_commit_device / b3w_commit_consumer do: they are for bodies the library did not make).
 * A step's commitment from its record equals the commitment of the body the witness kernel writes for it (tests/test_gpu_commit.py).
 * The commit kernels are bound by the vector ALUs, the witness kernels by HBM writes, so the commitments get a stream of the
 * chain's own beside the witness kernels; b3w_chain_commit_overlap says how far that goes. */
int32_t b3w_chain_commit_from_records(b3w_chain *chain, const b3w_commit_key *key, uint8_t *d_points);
/* Where the commitments of b3w_chain_commit_from_records run, per batch of steps (call before or after it; it holds for the chain):
 *   SERIAL  on the caller's stream, in front of the batch's witness kernel: nothing runs side by side
 *   FREE    on the chain's commit stream, ordered only behind the batch's planner: they run beside the witness kernels of this and
 *           later batches and `stream` waits for them at the end of each run call (4.5 M steps/s against 3.9 serial, 64 MiB)
 *   GATED   on the commit stream beside THIS batch's witness kernel only: whatever reads the batch on `stream` afterwards — the
 *           constraint check of b3w_chain_check_constraints, the consumer — starts when both have finished and has the device to
 *           itself, and the next batch's commitments start behind it (the check wants every vector register and most of the LDS of
 *           a CU: beside it the commit kernel only gets in its way)
 *   AUTO    (default) GATED when the chain checks constraints or the run call has a consumer, else FREE */
#define B3W_COMMIT_OVERLAP_AUTO   (-1)
#define B3W_COMMIT_OVERLAP_SERIAL 0
#define B3W_COMMIT_OVERLAP_FREE   1
#define B3W_COMMIT_OVERLAP_GATED  2
int32_t b3w_chain_commit_overlap(b3w_chain *chain, int32_t mode);
/* d_points = NULL above: the chain keeps the points itself; this copies them (n_leaf + n_parent times 64 bytes) to the host. */
int32_t b3w_chain_commitments(b3w_chain *chain, uint8_t *host_points, void *stream);
/* Constraint check inside the chained pass: after this call (r1cs = a system of the chain's context; NULL turns it off) every
 * batch of step witnesses is checked against the step circuit while it sits in the ring, before the consumer sees it;
 * b3w_chain_violations copies the per-step counts (n_leaf + n_parent entries, step order; 0 = the step satisfies every
 * constraint) to the host once `stream` has drained. */
int32_t b3w_chain_check_constraints(b3w_chain *chain, const b3w_r1cs *r1cs);
int32_t b3w_chain_violations(b3w_chain *chain, uint32_t *host_violations, void *stream);
uint32_t *b3w_chain_violations_device(b3w_chain *chain);   /* device: n_leaf + n_parent counts, NULL before b3w_chain_check_constraints */
int32_t b3w_chain_run_leaves(b3w_chain *chain, const uint8_t *host_preimage /* byte 0 of the WHOLE preimage */,
                             b3w_batch_consumer consumer, void *user, void *stream);
int32_t b3w_chain_run_parents(b3w_chain *chain, const uint32_t *d_all_chunk_cvs /* n_chunks*8 words; NULL = the local ones,
                              single rank */, b3w_batch_consumer consumer, void *user, void *stream);
/* Contiguous, balanced chunk ranges (the first n_chunks % nranks ranks take one extra chunk): what rank `rank` passes
 * to b3w_chain_create as first_chunk / n_chunks_local. */
void b3w_chain_shard(uint64_t n_chunks, int32_t rank, int32_t nranks, uint64_t *first_chunk, uint32_t *n_chunks_local);
/* b3w_chain_run_parents for a sharded pass: all-gathers the chunk chaining values over `comm` (32 B per chunk; shards
 * padded to the largest — equal shards are gathered where they lie, without a copy) and continues with the tree and this
 * rank's parent steps.  The chain must have been created with this rank's b3w_chain_shard range, and b3w_chain_run_leaves
 * of the same pass must have been called.  The exchange, the tree and the parent plan run on a stream of the CHAIN's —
 * beside the leaf witness kernels still queued on `stream`, which only joins for the parent witnesses — so an external
 * transport's callback (b3w_comm_create_external) is handed that stream, not the caller's. */
int32_t b3w_chain_run_parents_sharded(b3w_chain *chain, b3w_comm *comm, b3w_batch_consumer consumer, void *user, void *stream);
/* The fold's exchange in chained mode (BASELINE config 4: "RCCL gather of h_out"): the folding driver consumes z_{i+1} = the
 * public outputs of step i (Blake3CompressPubIO::to_vec, rust_fold/src/blake3_circuit.rs:111-123, fed back at
 * rust_fold/src/main.rs:166-179), of which h_out — public words 2..9 — is the running chaining value.  One ncclAllGather over
 * `comm` of this rank's h_out rows (packed to 8 words a row, shards padded to the largest) and a scatter into
 *   d_leaf_hout   : b3w_chain_num_leaf_steps(len) * 8 u32, GLOBAL step order (chunk, block): row 16 c + blocks(c) - 1 is chunk
 *                   c's chaining value
 *   d_parent_hout : b3w_chain_parent_row(n_chunks, n_chunks) * 8 u32, (chunk, height) order: the last row of a provable chunk
 *                   path is BLAKE3(preimage)
 * on every rank (either pointer may be NULL).  Enqueued on `stream` behind the pass; exchange buffers are allocated on the
 * first sharded call of a chain and kept, so a pass that has run once neither allocates nor synchronises. */
int32_t b3w_chain_allgather_hout(b3w_chain *chain, b3w_comm *comm, uint32_t *d_leaf_hout, uint32_t *d_parent_hout, void *stream);
/* The same into host arrays (for bindings that hold no device memory: Node).  Waits for `stream`. */
int32_t b3w_chain_allgather_hout_host(b3w_chain *chain, b3w_comm *comm, uint32_t *host_leaf_hout, uint32_t *host_parent_hout, void *stream);
/* How long the two exchanges of the last sharded pass took on this rank's device, in milliseconds (HIP events on the stream each ran on):
 * out_ms[0] = chunk chaining values (staging + all-gather + compaction, b3w_chain_run_parents_sharded), out_ms[1] = h_out (pack +
 * all-gather + scatter, b3w_chain_allgather_hout); 0 for an exchange that has not run.  Waits for those events. */
int32_t b3w_chain_exchange_ms(b3w_chain *chain, float out_ms[2]);
int32_t b3w_chain_info(const b3w_chain *chain, uint64_t *n_leaf_steps, uint64_t *n_parent_steps, uint64_t *n_chunks,
                       uint32_t *path_len, int32_t *placement);
/* Waits for `stream`, then copies the results to the host: (n_leaf + n_parent) * 15 public-output words, as many
 * status words, the 8 root words (after run_parents).  Any pointer may be NULL. */
int32_t b3w_chain_outputs(b3w_chain *chain, uint32_t *host_public, int32_t *host_status, uint32_t *host_root, void *stream);
uint32_t *b3w_chain_records(b3w_chain *chain);     /* device: (n_leaf + n_parent) * 32 u32 */
uint32_t *b3w_chain_public(b3w_chain *chain);      /* device: (n_leaf + n_parent) * 15 u32 */
int32_t *b3w_chain_status(b3w_chain *chain);       /* device: (n_leaf + n_parent) int32 */
uint32_t *b3w_chain_local_cvs(b3w_chain *chain);   /* device: n_chunks_local * 8 u32 */
uint32_t *b3w_chain_root(b3w_chain *chain);        /* device: 8 u32 = BLAKE3(preimage) words, after run_parents */

/* ---- bao outboards and challenged chunk paths (ABI 1.1) -------------------------------------------------
 * A data-availability challenge names a few chunk indices; the provider answers from the file and its bao OUTBOARD
 * (bao 0.12, 1 KiB chunks, as rust_fold/src/blake3_hash.rs:17-93 consumes it):
 *   outboard = 8-byte little-endian content length, then the n_chunks - 1 parent nodes of BLAKE3's tree in pre-order,
 *              64 bytes each (left child CV, right child CV: 8 little-endian words each); at most one chunk: the header alone.
 *   pre-order: the root is node 0; a node at position p over m chunks (k = the largest power of two below m) has its left
 *              subtree from p + 1 and its right subtree from p + k.
 *   slice of chunk c = the header, the nodes of c's path root first, the chunk's bytes [c*1024, min(len, c*1024 + 1024)).
 * b3w_bao_outboard_device: the outboard and the 8 root words (= BLAKE3(preimage)) of a preimage in device memory.  d_outboard:
 * b3w_bao_outboard_size(len) bytes, 8-byte aligned; d_levels: caller's scratch of (2 n_chunks + 64) * 8 u32 (b3w_chain_tree_device's
 * format; it holds the tree's level arrays afterwards); d_root: 8 u32.  No allocation. */
uint64_t b3w_bao_outboard_size(uint64_t preimage_len);                /* 8 + 64 * (n_chunks - 1) */
int32_t b3w_bao_outboard_device(b3w_ctx *ctx, const uint8_t *d_preimage, uint64_t preimage_len, uint8_t *d_outboard,
                                uint32_t *d_levels, uint32_t *d_root, void *stream);
/* Host only.  The pre-order indices of chunk's path nodes, root first (b3w_chain_path_len of them, at most 64): the nodes a
 * provider reads from an outboard on disk (node i lies at byte 8 + 64 i). */
int32_t b3w_bao_path_nodes(uint64_t chunk, uint64_t n_chunks, uint64_t *out_index, uint32_t *out_count);
/* Host only.  The bao slice of one chunk: *out_len = 8 + 64 * path_len + the chunk's byte count, and with out != NULL the bytes.
 * outboard: the whole outboard of a preimage of preimage_len bytes (its header must say so); chunk_bytes: the chunk's bytes. */
int32_t b3w_bao_slice(const uint8_t *outboard, uint64_t preimage_len, uint64_t chunk, const uint8_t *chunk_bytes, uint8_t *out,
                      uint64_t *out_len);
/* Rows of the step records of sampled chunk paths, sample-major: sample s owns rows [row_first[s], row_first[s + 1]) — its
 * leaf blocks, then its parent steps bottom up (the order a fold of that one path consumes them).  row_first: n_samples + 1
 * entries.  Returns the total row count, or -B3W_E_BAD_ARGUMENT (an index >= n_chunks; duplicates are fine). */
int64_t b3w_sample_rows(uint64_t preimage_len, const uint64_t *host_chunks, uint32_t n_samples, uint64_t *row_first);
/* The step records of the sampled chunk paths (rows as b3w_sample_rows says; 32 u32 each), from the outboard and the sampled
 * chunks' bytes alone (d_chunk_bytes: 1024 bytes per sample, bytes past the preimage's end ignored): word for word the records
 * b3w_chain_plan_leaves_device / b3w_chain_plan_parents_device write for those chunks, sibling-by-index-bit rule included.
 * Every path is verified top down as bao's decoder does (root node against `root` with the ROOT flag, each lower node against its
 * half of the node above, the chunk's CV against its half of the lowest node; one chunk: its ROOT-flagged output against `root`).
 * d_sample_status[s]: 0 verified, 1 the chunk's bytes do not match, 2 a path node or the root does not match, 3 the outboard's
 * header is not preimage_len.  Records are written for failing samples too; a sample never affects another.  Nova contexts
 * only.  The witnesses, commitments and constraint checks of the records are the batch calls' (b3w_batch_run_device,
 * b3w_commit_records_device, b3w_r1cs_check_device).  Asynchronous on `stream`; waits for this context's previous call. */
int32_t b3w_sample_plan_device(b3w_ctx *ctx, uint64_t preimage_len, const uint8_t *d_outboard, const uint32_t *root /* host, 8 u32 */,
                               const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_chunk_bytes, uint32_t *d_records,
                               int32_t *d_sample_status, void *stream);

/* ---- the same over a batch of files (ABI 1.2) -------------------------------------------------------------
 * A provider holds very many files, most of them small.  The batch calls take all of them at once: the outboards and roots in a
 * number of launches that does not depend on the file count (at most four: files of at most 64 chunks packed several to a wave; the others a
 * workgroup per TILE of 1 024 chunks, chunk CVs and the tile's tree in LDS, every node written straight to its pre-order place; one
 * workgroup per 1 024 tile CVs of the files of more than one tile; and, only with a file past 1 GiB, one more over those groups'
 * CVs, so files up to 1 TiB take the same route as all the others: no fall-back to the single-file stages), and one planning
 * call for challenges that name (file, chunk) pairs.  Nothing of a tile goes through level arrays: the scratch holds one CV per
 * tile of the files of more than 64 chunks plus one per group of 1 024 tiles: 32 bytes per tile (1 MiB of file) + 32 per group. */
/* Host only.  Outboards of a batch are packed in file order: file f's outboard (b3w_bao_outboard_size(lens[f]) bytes, byte for byte
 * what b3w_bao_outboard_device writes for that file alone) lies at [ob_first[f], ob_first[f + 1]) of d_outboards; every entry is a
 * multiple of 8.  ob_first: n_files + 1 entries.  Returns the total byte count. */
uint64_t b3w_bao_batch_layout(const uint64_t *host_lens, uint32_t n_files, uint64_t *ob_first);
/* Host only.  Bytes of caller's scratch the batch call needs for these lengths (may be 0: no file of more than 64 chunks). */
uint64_t b3w_bao_batch_scratch_bytes(const uint64_t *host_lens, uint32_t n_files);
/* File f is bytes [host_offsets[f], + host_lens[f]) of d_arena (any offsets: gaps, overlaps, repeats, unaligned starts, zero lengths;
 * a file that starts 16-byte aligned is read in whole 16-byte quarters).  d_outboards: 8-byte aligned; d_roots: 8 u32 per file
 * (= BLAKE3 of the file); d_scratch: 16-byte aligned.  The per-file table goes through staging the context owns (pinned host +
 * device, grow-only, freed with the context); nothing else is allocated.  n_files == 0: a no-op.  B3W_E_BAD_ARGUMENT before anything
 * is launched for a null pointer, a small scratch or a file of more than 2^30 chunks.  Asynchronous on `stream`; waits for this
 * context's previous batch call. */
int32_t b3w_bao_outboard_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets, const uint64_t *host_lens,
                                      uint32_t n_files, uint8_t *d_outboards, uint32_t *d_roots, void *d_scratch,
                                      uint64_t scratch_bytes, void *stream);
/* Rows of the step records of samples (host_files[s], host_chunks[s]), sample-major as b3w_sample_rows.  -B3W_E_BAD_ARGUMENT for a
 * file index >= n_files or a chunk index not below its file's chunk count. */
int64_t b3w_sample_rows_batch(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_chunks,
                              uint32_t n_samples, uint64_t *row_first);
/* b3w_sample_plan_device over a batch: d_outboards packed as b3w_bao_batch_layout says, d_roots ON THE DEVICE as the batch outboard
 * call left them, d_chunk_bytes 1 024 bytes per sample.  Records and statuses sample by sample those of b3w_sample_plan_device
 * on that sample's file alone; a bad sample touches no other, of its own file or another.  n_samples == 0: a no-op.  Nova contexts
 * only. */
int32_t b3w_sample_plan_batch_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint8_t *d_outboards,
                                     const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_chunks,
                                     uint32_t n_samples, const uint8_t *d_chunk_bytes, uint32_t *d_records,
                                     int32_t *d_sample_status, void *stream);

/* ---- outboards over chunk groups (ABI 1.3) ------------------------------------------------------------------
 * The full outboard costs 64 bytes per KiB of file.  A GROUP outboard is built over chunk groups of G = 2^group_log chunks: every
 * node of BLAKE3's tree over more than G chunks splits at a multiple of G, so those nodes are the parent nodes of BLAKE3's tree
 * shape over the file's n_groups = ceil(n_chunks / G) groups.  The group outboard = the 8-byte LE length, then those n_groups - 1
 * nodes in pre-order, 64 bytes each: the full outboard with every node over at most G chunks left out, in the same order (1 / G of
 * its size; a file of at most G chunks: the header alone).  A chunk's path = its group's path in the tree over groups (stored),
 * then the path of chunk c - first inside a BLAKE3 tree over the group's own min(G, n_chunks - first) chunks, first = c / G * G
 * (recomputed from the group's bytes at challenge time).  group_log = 0 is the full outboard.  A group_log above
 * B3W_BAO_MAX_GROUP_LOG is refused with B3W_E_BAD_ARGUMENT (the host-only size / layout calls return 0). */
#define B3W_BAO_MAX_GROUP_LOG 6 /* a group fits the lanes of one wave */
/* Host only.  8 + 64 * (n_groups - 1). */
uint64_t b3w_bao_group_outboard_size(uint64_t preimage_len, uint32_t group_log);
/* Host only.  b3w_bao_batch_layout for group outboards: packed in file order, every entry's start a multiple of 8. */
uint64_t b3w_bao_group_batch_layout(const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint64_t *ob_first);
/* Host only.  The indices in the group outboard of the stored part of the chunk's path, root first (out_index: room for 64). */
int32_t b3w_bao_group_path_nodes(uint64_t chunk, uint64_t n_chunks, uint32_t group_log, uint64_t *out_index, uint32_t *out_count);
/* b3w_bao_outboard_batch_device writing group outboards (packed as b3w_bao_group_batch_layout says): the same contract in every
 * other respect — the same arena rules, scratch (b3w_bao_batch_scratch_bytes), launch count (at most four), roots left on the
 * device, nothing written outside a file's own entry. */
int32_t b3w_bao_group_outboard_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets,
                                            const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint8_t *d_outboards,
                                            uint32_t *d_roots, void *d_scratch, uint64_t scratch_bytes, void *stream);
/* b3w_sample_plan_batch_device from group outboards.  d_group_bytes: 1024 << group_log bytes per sample, the bytes of the group
 * that holds the sampled chunk (file bytes from (chunk >> group_log << group_log) * 1024 on; bytes past the file's end ignored).
 * Rows are b3w_sample_rows_batch's (they do not depend on group_log), and the records are word for word those
 * b3w_sample_plan_batch_device writes from the full outboard.  d_sample_status[s]: 0 verified; 1 the GROUP's bytes do not match —
 * any byte of the sampled chunk's group, not only the sampled chunk's own, since the group's recomputed CV is what is held against
 * the stored path; 2 a stored node or the root does not match; 3 the header is not the file's length.  Records are written either
 * way; a bad sample touches no other.  n_samples == 0: a no-op.  Nova contexts only. */
int32_t b3w_sample_plan_group_batch_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                                           const uint8_t *d_group_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                           const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_group_bytes,
                                           uint32_t *d_records, int32_t *d_sample_status, void *stream);

/* ---- bao slices (ABI 1.4) ---------------------------------------------------------------------------------------
 * The SLICE of one chunk is what travels between the party that stores a file and the party that proves or checks a challenge
 * (the reference's hash_with_path extracts it and decodes it against the hash, rust_fold/src/blake3_hash.rs:17-93):
 *   slice of chunk c = the 8-byte LE length || the P = b3w_chain_path_len(c, n_chunks) nodes of c's path, root first, 64 bytes each
 *                      || the chunk's bytes [c*1024, min(len, c*1024 + 1024)); an empty file's slice is the header alone.
 * The provider makes slices from its outboards — full or GROUP outboards, the slices are the same standard ones any bao decoder
 * takes — and the prover plans the step records from the slices and the files' roots alone: it needs no outboard.  Every call here
 * is a batch call over samples (host_files[s], host_chunks[s]) as b3w_sample_plan_batch_device takes them. */
/* Host only.  8 + 64 P + the chunk's byte count; 0 for a chunk not below the chunk count. */
uint64_t b3w_bao_slice_size(uint64_t preimage_len, uint64_t chunk);
/* Host only.  Slices of a batch are packed in sample order: sample s's slice is the b3w_bao_slice_size bytes from slice_first[s]
 * of d_slices.  Every start is 8 modulo 16 (so also a multiple of 8): with d_slices 16-byte aligned the nodes and the chunk's
 * bytes, which follow the 8-byte header, lie on 16-byte boundaries, and the kernels move and read them 16 bytes at a time.  The
 * bytes in front of the first slice and between slices are padding that no call reads or writes.  slice_first: n_samples + 1
 * entries, the last one the total.  Returns the total byte count of d_slices, or -B3W_E_BAD_ARGUMENT for a file index >= n_files
 * or a chunk index not below its file's chunk count. */
int64_t b3w_bao_slice_batch_layout(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_chunks,
                                   uint32_t n_samples, uint64_t *slice_first);
/* Host only.  Bao's top-down decoder for one slice (slice_len must be b3w_bao_slice_size(preimage_len, chunk), else
 * B3W_E_BAD_ARGUMENT; so is a chunk out of range): for callers without a GPU.  *out_status: 0 verified, 1 the chunk's bytes do not
 * match, 2 a path node or the root does not match (one chunk: its ROOT-flagged output is what meets the root, so a wrong root is
 * 1 there), 3 the header is not preimage_len; 3 wins over 2 over 1, as in the planners.  out_chunk (room for 1024 bytes) and
 * out_bytes may be NULL; the bytes are handed out only with status 0 (*out_bytes = 0 otherwise). */
int32_t b3w_bao_slice_decode(const uint8_t *slice, uint64_t slice_len, uint64_t preimage_len, uint64_t chunk, const uint32_t *root /* 8 u32 */,
                             uint8_t *out_chunk, uint32_t *out_bytes, int32_t *out_status);
/* The provider's side: the slices of the samples into d_slices (16-byte aligned, packed as b3w_bao_slice_batch_layout says).
 * group_log = 0: d_outboards are full outboards (b3w_bao_batch_layout), d_bytes 1 024 bytes per sample (the sampled chunk's).
 * group_log = 1 .. B3W_BAO_MAX_GROUP_LOG: d_outboards are group outboards (b3w_bao_group_batch_layout), d_bytes 1024 << group_log
 * bytes per sample (the sampled chunk's group's, as b3w_sample_plan_group_batch_device takes them); the nodes inside the group are
 * recomputed.  Either way the same standard slices.  Nothing is verified (an extractor does not): the header is the outboard's.
 * One launch; the sample table goes through the context's staging, nothing else is allocated.  B3W_E_BAD_ARGUMENT before anything
 * is written for a group_log above the maximum, a null or misaligned pointer, a bad file or chunk index.  n_samples == 0: a no-op.
 * Any context.  Asynchronous on `stream`; waits for this context's previous batch call. */
int32_t b3w_bao_slice_batch_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards,
                                   const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_bytes,
                                   uint8_t *d_slices, void *stream);
/* The prover's side: b3w_sample_plan_batch_device from the slices alone — no outboard.  d_slices: 16-byte aligned, packed as
 * b3w_bao_slice_batch_layout says for these samples; d_roots: 8 u32 per file ON THE DEVICE.  Every slice is verified top down
 * against its file's root.  Rows are b3w_sample_rows_batch's; records and statuses (the same four codes) are word for word those
 * of b3w_sample_plan_batch_device for the same samples; records are written either way and a bad slice touches no other sample.
 * One launch.  n_samples == 0: a no-op.  Nova contexts only. */
int32_t b3w_sample_plan_slices_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *d_roots,
                                      const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices,
                                      uint32_t *d_records, int32_t *d_sample_status, void *stream);

/* ---- verification: whole files against their outboards (still ABI 1.4: new names only) ---------------------------
 * Bao's decoder applied to every UNIT of a file at once, for the party that takes files and outboards in, scrubs what it stores or
 * repairs after a fault.  A unit is a chunk (group_log = 0, full outboards) or a group of 2^group_log chunks (group outboards); a
 * file has max(1, ceil(n_chunks / 2^group_log)) of them.  A unit's status is the status b3w_sample_plan_batch_device /
 * b3w_sample_plan_group_batch_device give a sample in that unit, the first rule that applies:
 *   3  the outboard's 8-byte header is not the file's length (every unit of the file)
 *   2  a stored node on the unit's path fails: the root node hashed with PARENT | ROOT is not the file's root, or a lower stored
 *      node hashed with PARENT is not its half of the stored node above it
 *   1  the unit's CV, computed from the file's bytes (the levels inside a group recomputed), is not its half of the lowest stored
 *      node on its path; a file of one unit has no stored node: its ROOT-flagged CV is held against the root (a wrong root: 1)
 *   0  otherwise
 * Every node check is stored data against stored data, so one bad byte of a chunk marks that unit alone (1), one bad byte of a
 * node exactly the units below that node (2), a wrong root every unit of that file and no other file. */
/* Host only.  Statuses of a batch are packed in file order, one byte a unit: file f's are entries [unit_first[f], unit_first[f + 1])
 * of d_unit_status.  unit_first: n_files + 1 entries, the last one the total, which is also returned (0 for a group_log above
 * B3W_BAO_MAX_GROUP_LOG or a null pointer). */
uint64_t b3w_bao_verify_layout(const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint64_t *unit_first);
/* Host only.  Bytes of caller's scratch b3w_bao_verify_batch_device needs for these lengths: the CV expected of a tile and a flag
 * (36 bytes) per tile of 1 024 chunks of the files of more than one tile, the same per 1 024 tiles of the files of more than
 * 1 024 tiles, rounded up to 16; 0 where no file has more than one tile. */
uint64_t b3w_bao_verify_scratch_bytes(const uint64_t *host_lens, uint32_t n_files);
/* Files as b3w_bao_outboard_batch_device takes them ([host_offsets[f], + host_lens[f]) of d_arena, any offsets); d_outboards packed
 * as b3w_bao_batch_layout (group_log = 0) or b3w_bao_group_batch_layout says, 8-byte aligned; d_roots: 8 u32 per file ON THE
 * DEVICE.  Outputs, all on the device, none needs clearing: d_unit_status, one byte a unit, packed as b3w_bao_verify_layout says;
 * d_file_status[f], the largest status among file f's units; d_first_bad[f] (8-byte aligned), the lowest unit index of file f
 * with a non-zero status, or UINT64_MAX.  Nothing is read back to the host.  At most four launches whatever the file count — no
 * more than the outboard call's: the nodes above the tiles are checked first, from the stored nodes alone (one launch, one more
 * for files past 1 GiB), then the files of at most 64 chunks and the tiles of the others write final statuses.  d_scratch: 16-byte
 * aligned, b3w_bao_verify_scratch_bytes; the per-file tables go through the context's staging, nothing else is allocated.
 * n_files == 0: a no-op.  B3W_E_BAD_ARGUMENT before anything is written for a group_log above the maximum, a null or misaligned
 * pointer, a small scratch, a null arena with a file that is not empty, or a file of more than 2^30 chunks.  Any context.
 * Asynchronous on `stream`; waits for this context's previous batch call. */
int32_t b3w_bao_verify_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets, const uint64_t *host_lens,
                                    uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *d_roots,
                                    uint8_t *d_unit_status, int32_t *d_file_status, uint64_t *d_first_bad, void *d_scratch,
                                    uint64_t scratch_bytes, void *stream);
/* Host only, one file, for callers without a GPU: the same statuses from `data` (len bytes), its outboard (full, or the group
 * outboard of group_log) and the root (8 u32).  unit_status: room for max(1, ceil(n_chunks / 2^group_log)) bytes; file_status and
 * first_bad may be NULL.  B3W_E_BAD_ARGUMENT for a null pointer or a group_log above the maximum. */
int32_t b3w_bao_verify(const uint8_t *data, uint64_t len, const uint8_t *outboard, uint32_t group_log, const uint32_t *root /* 8 u32 */,
                       uint8_t *unit_status, int32_t *file_status, uint64_t *first_bad);

/* ---- outboards and verification of a file streamed in windows (still ABI 1.4: new names only) ----------------------
 * The calls above take the whole file resident in device memory.  A stream session takes ONE file of known length window by window,
 * for the party that ingests from disk or the network and for files larger than device memory: the file's bytes need only be on the
 * device a window at a time, and a window is 1 MiB (a tile of 1 024 chunks) or any multiple.  The session is a host object: it holds
 * the caller's device pointers and a bit per tile pushed, and no device memory of its own.  Several sessions may be open on one
 * context; one session is used by one host thread at a time.
 * RESULTS are those of the batch calls for the same file as a batch of one, byte for byte: d_outboard and d_root after finish are
 * what b3w_bao_outboard_batch_device (group_log = 0) or b3w_bao_group_outboard_batch_device write; d_unit_status, d_file_status and
 * d_first_bad are what b3w_bao_verify_batch_device writes.
 * REFUSALS are B3W_E_BAD_ARGUMENT with a b3w_last_error text; a refused call launches nothing and leaves the session as it was. */
typedef struct b3w_bao_stream b3w_bao_stream;
#define B3W_BAO_STREAM_OUTBOARD 0
#define B3W_BAO_STREAM_VERIFY   1
/* Host only.  Bytes of caller's scratch a session over a file of `len` bytes needs: b3w_bao_batch_scratch_bytes of the one length
 * (kind B3W_BAO_STREAM_OUTBOARD: 32 bytes a tile and per 1 024 tiles) or b3w_bao_verify_scratch_bytes of it (B3W_BAO_STREAM_VERIFY);
 * 0 for any other kind. */
uint64_t b3w_bao_stream_scratch_bytes(uint64_t len, uint32_t kind);
/* Opens an outboard session: group_log = 0 the full outboard (b3w_bao_outboard_size bytes at d_outboard), 1 .. B3W_BAO_MAX_GROUP_LOG
 * the group outboard (b3w_bao_group_outboard_size).  d_outboard 8-byte aligned, d_root 8 u32 on the device, d_scratch 16-byte
 * aligned; all three stay the caller's and must live until the work of finish is done.  Launches nothing.  Refused: a group_log
 * above the maximum, a file of more than 2^30 chunks, a null or misaligned pointer, a small scratch. */
int32_t b3w_bao_stream_outboard_begin(b3w_ctx *ctx, uint64_t len, uint32_t group_log, uint8_t *d_outboard, uint32_t *d_root, void *d_scratch,
                                      uint64_t scratch_bytes, b3w_bao_stream **out_session);
/* Opens a verification session against an outboard and a root that are resident (as they arrived from elsewhere); the outputs as
 * b3w_bao_verify_batch_device's for one file (d_unit_status: max(1, ceil(n_chunks / 2^group_log)) bytes).  For a file of more than
 * one tile it launches, on `stream`, the check of the stored nodes above the tiles (one launch, two past 1 GiB), which also
 * initialises d_file_status and d_first_bad; every push waits for that work ON THE DEVICE (an event of the session), whatever
 * stream it is given.  Refused as above, and for a null or misaligned output. */
int32_t b3w_bao_stream_verify_begin(b3w_ctx *ctx, uint64_t len, uint32_t group_log, const uint8_t *d_outboard, const uint32_t *d_root,
                                    uint8_t *d_unit_status, int32_t *d_file_status, uint64_t *d_first_bad, void *d_scratch,
                                    uint64_t scratch_bytes, void *stream, b3w_bao_stream **out_session);
/* The bytes [offset, offset + bytes) of the file lie at d_window (any byte alignment; 16-byte aligned windows take the fast loads).
 * offset is a multiple of 1 MiB; bytes is a positive multiple of 1 MiB unless the window ends at the file's end.  Windows may come
 * in any order and on any stream, each tile once.  One launch, a workgroup per tile of the window; nothing is allocated, no table is
 * uploaded and the host waits for no earlier call.  d_window may be reused once this push's work on `stream` is done.
 * Verification: the statuses of the window's units are FINAL once this push's work on `stream` is done, so a bad window can be
 * dropped before the rest arrives.  Refused: an offset off a 1 MiB boundary, an empty window or a null pointer, a window that
 * reaches past the file's end or that is not whole tiles and does not end at the file's end, a tile pushed before, a push after
 * finish.  A file of no bytes takes no push. */
int32_t b3w_bao_stream_push(b3w_bao_stream *session, uint64_t offset, const uint8_t *d_window, uint64_t bytes, void *stream);
/* THE CALLER ORDERS `stream` BEHIND EVERY PUSH (the same stream, or events of the pushes' streams it has made `stream` wait for).
 * Outboard sessions: the nodes above the tiles and the root from the tile CVs in the scratch (one launch for a file of more than
 * one tile, two past 1 GiB; none for one tile, whose push wrote the root).  Verification: nothing is launched, the pushes have left
 * d_file_status and d_first_bad final.  A file of no bytes gets its one launch here.  Refused: a tile that has not been pushed, a
 * second finish. */
int32_t b3w_bao_stream_finish(b3w_bao_stream *session, void *stream);
/* Frees the host object (NULL: a no-op); work already enqueued is not waited for and needs nothing of the session. */
void b3w_bao_stream_free(b3w_bao_stream *session);

/* ---- many stream sessions in one launch (still ABI 1.4: new names only) ---------------------------------------------
 * A push costs the latency of one tile's workgroup whatever the window holds, and pushes on one stream run one behind the other: a
 * party with several hundred uploads open, each receiving small windows, is bound by launches.  These two take the windows (the
 * finishes) of MANY sessions and make one grid of them.  Entry i of push_many means exactly what b3w_bao_stream_push(sessions[i],
 * offsets[i], d_windows[i], bytes[i], stream) means, under the same per-window rules, and the bytes left behind (outboards, roots,
 * tile CVs in the scratches; unit statuses, file statuses, first bad units) are byte for byte those of the per-session calls.
 * All sessions of one call belong to `ctx` and are of ONE kind, all outboard or all verification; group_log may differ from session
 * to session; a session may appear more than once in a push_many whose entries name disjoint tiles of it.  n == 0: B3W_OK, nothing
 * launched.
 * LAUNCHES: push_many is ONE launch whatever n and the tile count are (a call that mixes group_log = 0 with group_log > 0 runs the
 * group kernel for all: at group_log = 0 it stores the same nodes).  Verification: `stream` is made to wait ON THE DEVICE for the
 * begin work of every distinct session in the call; the host waits for nothing.  finish_many: one launch over the first merge storey
 * of all outboard sessions of more than one tile, one more if any session is past 1 GiB, one more for the sessions of no bytes: at
 * most three whatever n is; verification sessions take the last one alone.  The caller orders `stream` behind every push.
 * THE TABLE: which session, tile and window a workgroup takes is a row of 88 bytes per entry, copied to the device on `stream` in
 * front of the launch through a ring of 8 staging slots in the context (pinned host + device, grow-only, an event each).  Once the
 * slots have grown to the calls' size nothing is allocated, and the host waits for earlier device work only where all 8 slots are
 * still in flight.  One context is used by one host thread at a time.
 * REFUSALS ARE ATOMIC: if any entry would be refused the call returns B3W_E_BAD_ARGUMENT, nothing is launched and NO session's
 * state changes; b3w_last_error names the entry's index and the reason.  Refused: what b3w_bao_stream_push / _finish refuse, a null
 * array, a null session, a session of another context, sessions of mixed kinds, a tile named twice within the call, a session that
 * appears twice in finish_many, more than 2^31 - 1 tiles (workgroups) in one call. */
int32_t b3w_bao_stream_push_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, const uint64_t *offsets, const uint8_t *const *d_windows,
                                 const uint64_t *bytes, uint32_t n, void *stream);
int32_t b3w_bao_stream_finish_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, uint32_t n, void *stream);

/* ---- outboards of streamed files whose length is not known up front (still ABI 1.4: new names only) ------------------
 * The sessions above take the file's length at begin: the pre-order place of every node depends on the total chunk count.  An upload
 * over chunked transfer encoding, a pipe or an archive member being produced has no length until its last byte.  An OPEN session takes
 * an upper bound (capacity_bytes) instead, FULL tiles of 1 MiB in any order and on any stream, and the length only at finish.
 * WHY IT WORKS: a full tile of 1 024 chunks is a complete subtree whatever the length turns out to be; its (1024 >> group_log) - 1
 * stored nodes are contiguous in the file's pre-order (group) outboard, in an order of their own that does not depend on the file, and
 * only the START of that run depends on the total; its chaining value is not ROOT-flagged unless the file is exactly that tile.  A push
 * hashes its tiles into tile-local BLOCKS of a staging area of the caller's; finish moves every block to its place (one launch, a copy
 * of the outboard: 64 MiB per GiB of file at group_log = 0, 960 bytes a MiB at 6) and runs the merge storeys of the sessions above.
 * RESULTS after b3w_bao_stream_open_finish are byte for byte those of the batch calls for the same bytes as a batch of one — header,
 * every node, root — and nothing beyond b3w_bao_group_outboard_size(len, group_log) bytes of d_outboard is written.
 * REFUSALS as above: B3W_E_BAD_ARGUMENT, a b3w_last_error text, nothing launched, the session as it was and still usable. */
#define B3W_BAO_STREAM_OPEN 2
/* The staging bytes that are no block's: block t lies at byte 8 + t * ((1024 >> group_log) - 1) * 64 of a 16-byte-aligned staging,
 * 8 bytes off a 16-byte boundary as the nodes of a 16-byte-aligned outboard are, and 8 bytes follow the last block. */
#define B3W_BAO_STREAM_OPEN_STAGING_PAD 16
/* Host only.  floor(capacity_bytes / 1 MiB) * ((1024 >> group_log) - 1) * 64 + B3W_BAO_STREAM_OPEN_STAGING_PAD; 0 for a group_log
 * above B3W_BAO_MAX_GROUP_LOG. */
uint64_t b3w_bao_stream_open_staging_bytes(uint64_t capacity_bytes, uint32_t group_log);
/* Host only.  32 bytes per MiB of capacity (rounded up, at least one) and per 1 024 of those: the tile and group CVs of any length up
 * to the capacity.  Never 0. */
uint64_t b3w_bao_stream_open_scratch_bytes(uint64_t capacity_bytes);
/* Host only.  The node index, in the outboard (group_log = 0) or group outboard of a file of `len` bytes, of the first node of the
 * block of full tile `tile`: what the relocation computes on the device.  The block's nodes follow it without a gap.  UINT64_MAX
 * where (tile + 1) MiB > len (not a full tile of that file) or group_log is above the maximum. */
uint64_t b3w_bao_stream_open_block_pos(uint64_t len, uint32_t group_log, uint64_t tile);
/* Opens a session of kind B3W_BAO_STREAM_OPEN for a file of at most capacity_bytes.  d_staging and d_scratch: 16-byte aligned, at
 * least what the two size calls say; both stay the caller's and must live until the work of open_finish is done.  Launches nothing
 * and has no device memory of its own.  Refused: a null context or session pointer, a group_log above the maximum, a capacity of
 * more than 2^30 chunks, a null or misaligned pointer, a small staging or scratch.
 * b3w_bao_stream_push takes an open session under these rules: offset a multiple of 1 MiB; bytes a POSITIVE MULTIPLE of 1 MiB (there
 * is no ragged window: what does not fill a tile goes to open_finish); offset + bytes <= capacity_bytes; each tile once; not after
 * open_finish.  One launch, a workgroup per tile; no header and no root are written.
 * b3w_bao_stream_push_many takes a call whose sessions are ALL open (open is a kind: mixed with sessions of known length the call is
 * refused atomically), group_log free per session, through the same table and staging ring: one launch.
 * b3w_bao_stream_finish and _finish_many refuse an open session (finish_many atomically): open sessions end through
 * b3w_bao_stream_open_finish, or many of them at once through b3w_bao_stream_open_finish_many; b3w_bao_stream_free frees it. */
int32_t b3w_bao_stream_open_begin(b3w_ctx *ctx, uint64_t capacity_bytes, uint32_t group_log, void *d_staging, uint64_t staging_bytes,
                                  void *d_scratch, uint64_t scratch_bytes, b3w_bao_stream **out_session);
/* The end of the file: with T tiles pushed the file is len = T MiB + tail_bytes, and d_tail holds its last tail_bytes < 1 MiB bytes
 * (any alignment; NULL where tail_bytes is 0; it must live until `stream` has passed this call's work).  THE CALLER ORDERS `stream`
 * BEHIND EVERY PUSH.  d_outboard: 8-byte aligned (16-byte aligned outboards are moved 16 bytes at a time, the others 8), at least
 * b3w_bao_group_outboard_size(len, group_log) of outboard_bytes; d_root: 8 u32 on the device.  *out_len (may be NULL) = len.
 * AT MOST FOUR LAUNCHES whatever the length: the tail's tile through the kernel of the sessions above with the now known length (for
 * T = 0 that is the whole file, rooted; a file of no bytes gets its one launch); the relocation of the blocks, which also writes the
 * header; the merge storey over the tile CVs (files of more than one tile) and the one above it (past 1 GiB).  A file of exactly
 * 1 MiB is one block and no storey: its root is computed in the relocation launch from the block's first node.
 * Refused: pushed tiles that are not exactly 0 .. T - 1 (the text names the lowest missing one), tail_bytes >= 1 MiB, a null tail
 * with bytes, len above the capacity, a small outboard, a null or misaligned d_outboard / d_root, a session that is finished or not
 * open. */
int32_t b3w_bao_stream_open_finish(b3w_bao_stream *session, const uint8_t *d_tail, uint64_t tail_bytes, uint8_t *d_outboard,
                                   uint64_t outboard_bytes, uint32_t *d_root, void *stream, uint64_t *out_len);
/* b3w_bao_stream_open_finish for MANY open sessions of `ctx` at once: entry i means exactly what b3w_bao_stream_open_finish(
 * sessions[i], d_tails[i], tail_bytes[i], d_outboards[i], outboard_bytes[i], d_roots[i], stream, &out_lens[i]) means, and the bytes it
 * leaves are that call's: header, every node, root, and nothing behind b3w_bao_group_outboard_size(len, group_log).  group_log is free
 * per session.  out_lens may be NULL.  THE CALLER ORDERS `stream` BEHIND EVERY PUSH of every session.  n == 0: B3W_OK, nothing launched.
 * AT MOST FOUR LAUNCHES whatever n and the lengths are: the tails' tiles of all sessions that have one (files of no bytes among them),
 * the relocation of all blocks with the headers, the first merge storey of all files of more than one tile, the second of all files
 * past 1 GiB.  One table of 88-byte rows, a row per session and launch it takes part in, goes through the staging ring of the many-calls
 * above; a call that mixes group_log = 0 with larger ones runs the group kernels for all.  The host waits for nothing.
 * REFUSALS ARE ATOMIC as in the many-calls above (B3W_E_BAD_ARGUMENT, nothing launched, no session changed, b3w_last_error names the
 * entry and the reason): what open_finish refuses per entry, a null array (out_lens excepted), a null session, a session of another
 * context, a session that is not open, a session twice in the call, more than 2^31 - 1 workgroups in one of the four grids.
 * Two entries whose outboards or roots overlap are NOT looked for: that is the caller's business, as with two calls of open_finish. */
int32_t b3w_bao_stream_open_finish_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, const uint8_t *const *d_tails,
                                        const uint64_t *tail_bytes, uint8_t *const *d_outboards, const uint64_t *outboard_bytes,
                                        uint32_t *const *d_roots, uint32_t n, void *stream, uint64_t *out_lens);

/* ---- challenged paths and slices read in place from the file arena (still ABI 1.4: new names only) -----------------
 * b3w_sample_plan_batch_device, b3w_sample_plan_group_batch_device and b3w_bao_slice_batch_device take a dense copy of the sampled
 * chunks' (or groups') bytes, which the caller has to gather first.  These two take the arena the outboard and verification calls
 * read — file f is bytes [host_offsets[f], + host_lens[f]) of d_arena, any offsets: gaps, overlaps, repeats, zero lengths, a start at
 * ANY byte — and read each sample's bytes where they lie: a provider that holds the arena, the offsets and the outboards answers a
 * challenge with no kernel of its own and no copy.
 * group_log = 0: d_outboards are full outboards packed as b3w_bao_batch_layout says; 1 .. B3W_BAO_MAX_GROUP_LOG: group outboards
 * packed as b3w_bao_group_batch_layout says (8-byte aligned either way).  Samples are (host_files[s], host_chunks[s]).
 * Both: ONE launch; the per-sample table (48 bytes a sample: the existing calls' five words and the file's arena offset) goes through
 * the context's staging and nothing else is allocated; no byte outside [offset, offset + len) of a sample's OWN file is read — not the
 * bytes behind a ragged last chunk, not the chunks a short last group lacks — so what lies between and behind the files never
 * matters.  A chunk lies at offset mod 16: the hashing takes 16-byte loads from a 16-byte-aligned chunk and smaller ones otherwise
 * (a file that starts 16-byte aligned is the fast case, as in b3w_bao_outboard_batch_device); the results do not depend on it.
 * B3W_E_BAD_ARGUMENT before anything is written for a null pointer (d_arena may be NULL where every sampled file is empty), a
 * misaligned d_outboards / d_slices, a group_log above the maximum, a file index >= n_files, a chunk index not below its file's
 * chunk count, or a sampled file that reaches past arena_bytes (the arena's size: the bound that keeps every read inside it).
 * n_samples == 0: a no-op.  Asynchronous on `stream`; waits for this context's previous batch call. */
/* Rows are b3w_sample_rows_batch's; the records (word for word), the four status codes and their precedence are those of
 * b3w_sample_plan_batch_device (group_log = 0) / b3w_sample_plan_group_batch_device on the gathered bytes of the same arena; d_roots
 * 8 u32 per file ON THE DEVICE.  Records are written for failing samples too; a bad sample touches no other.  Nova contexts only. */
int32_t b3w_sample_plan_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                     const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards,
                                     const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_chunks,
                                     uint32_t n_samples, uint32_t *d_records, int32_t *d_sample_status, void *stream);
/* The slices b3w_bao_slice_batch_device makes, into d_slices (16-byte aligned, packed as b3w_bao_slice_batch_layout says).  Only each
 * sample's b3w_bao_slice_size bytes are written: the padding between slices is neither read nor written.  The chunk's bytes are
 * moved in 16-byte stores; the loads are 16 bytes wide from a source at 0 modulo 16, 8 at 8, 4 at 4 and 12, single bytes otherwise,
 * as far as the source text goes (a compiler for a device that takes unaligned loads may merge them).  Nothing is verified.  Any
 * context. */
int32_t b3w_bao_slice_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                   const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards,
                                   const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, uint8_t *d_slices,
                                   void *stream);

/* ---- slices taken in: the receiver's side (still ABI 1.4: new names only) --------------------------------------------
 * A party that holds only a file's ROOT and is sent chunks with their paths — fetching a sparse file, repairing the units a ranged
 * verification marked bad, following a remote read.  b3w_bao_slice_ingest_device is the mirror image of b3w_bao_slice_arena_device and
 * takes its arguments the same way: the files are [host_offsets[f], + host_lens[f]) of d_arena at any byte offset, d_outboards (8-byte
 * aligned) is packed as b3w_bao_batch_layout (group_log 0) / b3w_bao_group_batch_layout (1 .. 6) says, d_slices (16-byte aligned) holds
 * the samples' slices packed as b3w_bao_slice_batch_layout says, d_roots 8 u32 per file ON THE DEVICE.  d_arena, d_outboards and
 * d_slices must not overlap (not checked).
 *   d_sample_status[s]: the four codes and the precedence of b3w_bao_slice_decode / b3w_sample_plan_slices_device — 3 the header is not
 *   the length, 2 a path node or the root fails, 1 the chunk's bytes fail (a one-chunk file's wrong root is 1), else 0.
 *   NOTHING UNVERIFIED IS WRITTEN: a sample writes only after its whole slice has verified against the root; one with a non-zero status
 *   writes its status and nothing else.  A verified sample writes exactly (a) the chunk's min(1024, len - 1024 c) bytes at d_arena +
 *   offset[f] + 1024 c, no byte in front of or behind them (stores as wide as the destination is aligned: 16 / 8 / 4 / 1 bytes, the ragged
 *   tail byte-wise), (b) the STORED nodes of its path at their pre-order places in file f's outboard — group_log 0: all of them;
 *   group_log > 0: the first b3w_bao_group_path_nodes of them, the nodes inside the group are verified and dropped — and (c) the 8-byte
 *   header.  An empty file's slice is its header: checked against the root of the empty input and written.
 *   Samples may repeat, come in any order and share path nodes: every writer of a byte that writes at all writes the same verified
 *   value, so a good and a bad slice of one chunk in one call leave the good one's bytes.  Once every chunk of a file has come in
 *   its outboard is the provider's byte for byte (b3w_bao_outboard_batch_device / b3w_bao_group_outboard_batch_device), from the traffic
 *   itself, and every other call here applies to it.  b3w_bao_slice_ingest_have_device ("the arrival bitmap" below) also records on the
 *   device which chunks have arrived.
 * One launch; the per-sample table (48 bytes a sample) goes through the context's staging and nothing else is allocated; the host waits
 * for nothing but this context's previous batch call.  B3W_E_BAD_ARGUMENT before anything is written for what
 * b3w_bao_slice_arena_device refuses and for a null d_roots / d_sample_status.  n_samples == 0: a no-op.  Any context.  Asynchronous on
 * `stream`.
 * When not to (MI355X): the call costs about 23 ns a slice, host loop included — 4 096 slices of a 1 GiB file 0.18 ms,
 * 65 536 1.52 ms, every chunk (1 048 576) 23.7 ms for 2.27 times the file's bytes in slices — where hashing the whole resident GiB
 * takes 0.43 ms (b3w_bao_outboard_batch_device, then compare the root) or 0.45 (b3w_bao_verify_batch_device against an outboard sent
 * once).  So: slices for the sparse fetch, the repair and the remote read, up to a few per cent of a file's chunks; a file that
 * arrives whole goes through the b3w_bao_stream_verify_* session or the batch calls on its bytes alone. */
int32_t b3w_bao_slice_ingest_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                    const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint8_t *d_outboards,
                                    const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_chunks,
                                    uint32_t n_samples, const uint8_t *d_slices, int32_t *d_sample_status, void *stream);
/* Host only: the same verdict and the same writes for ONE slice — `data` is the file (len bytes), `outboard` its (group) outboard.
 * B3W_E_BAD_ARGUMENT for what b3w_bao_slice_decode refuses, a group_log above the maximum and a null pointer; data may be NULL only for
 * an empty file. */
int32_t b3w_bao_slice_ingest(const uint8_t *slice, uint64_t slice_len, uint64_t preimage_len, uint64_t chunk, const uint32_t *root /* 8 u32 */,
                             uint32_t group_log, uint8_t *data, uint8_t *outboard, int32_t *out_status);

/* ---- the arrival bitmap: which chunks have come in, and what is still missing (still ABI 1.4: new names only) -------
 * A receiver that takes slices in needs to know which chunks it holds, what to ask for next and when a file is complete.  These calls
 * keep that record on the device and turn it into the run lists b3w_bao_verify_ranges_batch_device and
 * b3w_bao_outboard_update_batch_device take, so that fetch -> ingest -> "what is missing?" -> fetch closes without the caller copying
 * and scattering statuses.
 * THE BITMAP.  File f owns ceil(b3w_chain_num_chunks(len_f) / 64) words of 64 bits, from word word_first[f] of d_have; chunk c is bit
 * c & 63 of word word_first[f] + (c >> 6).  One bit per CHUNK at every group_log (slices are of one chunk at every group_log); an empty
 * file has one chunk and one bit.  The bits at and above the chunk count in a file's last word are pad bits: the library never sets
 * them and every reader masks them, so a stray pad bit never makes a run past the end of a file.  d_have is 8-byte aligned; the
 * caller clears it once; only b3w_bao_have_from_status_device ever clears a bit. */
#define B3W_BAO_HAVE_MISSING 0
#define B3W_BAO_HAVE_PRESENT 1
/* Host only: word_first [n_files + 1] -> the total number of words (0 for a null pointer). */
uint64_t b3w_bao_have_layout(const uint64_t *host_lens, uint32_t n_files, uint64_t *word_first /* n_files + 1 */);
/* b3w_bao_slice_ingest_device with the record: the same arguments in the same order, d_have in front of the stream.  It writes byte
 * for byte what that call writes — arena, outboards, statuses — and for every sample whose status is 0 it also ORs that chunk's bit
 * into d_have (one 8-byte atomic OR by the sample's first lane, behind that lane's stores).  A sample with another status sets
 * nothing; duplicates and samples that share a word are fine; no other bit changes.  One launch, the same choice of lanes a sample;
 * the per-file word offsets ride the staging behind the rows and nothing is allocated.  Refuses what that call refuses, and a null or
 * misaligned d_have, before anything is written.
 * When not to (MI355X): the record costs about 0.6 % — 65 536 slices of a 1 GiB file 1.534 ms with it against 1.525
 * without (the spread of the yardstick 0.001), 4 096 slices 0.181 against 0.180 — so the only reason for the plain call is a caller
 * that keeps no bitmap. */
int32_t b3w_bao_slice_ingest_have_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                         const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint8_t *d_outboards,
                                         const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_chunks,
                                         uint32_t n_samples, const uint8_t *d_slices, int32_t *d_sample_status, uint64_t *d_have,
                                         void *stream);
/* RUNS.  A UNIT is a chunk (group_log 0) or a group of 2^group_log chunks, the last one possibly ragged; group_log is only the
 * granularity of the report (a caller who wants chunk-exact runs of a file kept with group outboards passes 0).  kind
 * B3W_BAO_HAVE_PRESENT selects the units ALL of whose chunks are set, B3W_BAO_HAVE_MISSING those with at least one chunk clear: for
 * one group_log the two partition every file's units.  A run is a maximal stretch of selected units of ONE file; its row is
 * (d_run_file, d_run_first, d_run_count) = (file, first chunk, number of chunks): whole units, clipped to the file's chunk count, the
 * shape the ranged calls take.  Rows come in ascending (file, first chunk) order; runs merge across words and never cross files.
 *   *d_n_runs receives the number of runs FOUND, even above `capacity`; rows [0, min(found, capacity)) are written and no byte behind
 *   them is touched.  capacity == 0 with null row pointers is a count-only call.  A file of u units has at most ceil(u / 2) runs of
 *   one kind: the sum of that over the files is a capacity that always suffices.
 *   d_file_have[f] (may be NULL): the number of set bits of file f that are not pad bits, whatever kind and group_log; the file is
 *   complete when it equals the chunk count.
 * At most four launches whatever the file and run counts (count; the scan over the workgroups' totals; rows; counts from ends) and no
 * workgroup waits for another.  Asynchronous on `stream`; nothing is allocated beyond d_scratch (8-byte aligned, at least
 * b3w_bao_have_runs_scratch_bytes, host only) and the context's staging for the per-file tables; the host waits for nothing but this
 * context's previous batch call.  B3W_E_BAD_ARGUMENT before anything is written for a null or misaligned pointer (d_run_file 4-byte,
 * the others 8-byte; the row pointers may be NULL only with capacity 0), a group_log above B3W_BAO_MAX_GROUP_LOG, an unknown kind, a
 * scratch that is too small, or more than 2^26 bitmap words in total (2^32 chunks).  n_files == 0 writes *d_n_runs = 0.
 * When not to (MI355X): no call takes less than about 0.05 ms (count only; 0.10 with a few thousand rows brought to
 * the host).  One file of 2^20 chunks: the missing rows on the host in 0.11 ms (1 % missing, 10 426 rows), 0.22 (50 %, 262 147 rows)
 * and 0.10 (one run), where copying an ingest's 65 536 statuses to the host, scattering them into a map and making the rows with
 * numpy takes 0.67, 3.64 and 0.42; 262 144 files of 4 chunks: 0.66 ms against 8.18, 0.48 of it the host's per-file tables and their
 * upload (about 1.8 ns a file: the one cost that follows the file count).  Nothing smaller was measured: for a few files of a few
 * thousand chunks a caller that has the statuses on the host anyway may do as well there. */
uint64_t b3w_bao_have_runs_scratch_bytes(const uint64_t *host_lens, uint32_t n_files);
int32_t b3w_bao_have_runs_device(b3w_ctx *ctx, const uint64_t *d_have, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                                 uint32_t kind, uint64_t capacity, uint32_t *d_run_file, uint64_t *d_run_first, uint64_t *d_run_count,
                                 uint64_t *d_n_runs, uint64_t *d_file_have, void *d_scratch, uint64_t scratch_bytes, void *stream);
/* AFTER A RESTART: a bitmap from the unit statuses b3w_bao_verify_batch_device / b3w_bao_verify_ranges_batch_device write (packed as
 * b3w_bao_verify_layout says for this group_log) over the half-filled arena and outboards.  Bit c of file f becomes
 * status[unit_first[f] + (c >> group_log)] == 0; 0xFF (a unit the ranged call was not asked about) reads as absent.  Every word of
 * every file is written whole with its pad bits zero: the one call that clears bits.  One launch; the same staging, limits and
 * refusals (a null pointer, a misaligned d_have, a group_log above the maximum, more than 2^26 words).  n_files == 0: a no-op. */
int32_t b3w_bao_have_from_status_device(b3w_ctx *ctx, const uint8_t *d_unit_status, const uint64_t *host_lens, uint32_t n_files,
                                        uint32_t group_log, uint64_t *d_have, void *stream);
/* Host only, ONE file of preimage_len bytes whose bitmap starts at have[0]: the rows (without the file column), *n_runs and *n_have
 * (may be NULL) as the device call gives them for that file; and the bitmap from that file's unit statuses.  B3W_E_BAD_ARGUMENT for a
 * null pointer (the row pointers may be NULL with capacity 0), a group_log above the maximum or an unknown kind. */
int32_t b3w_bao_have_runs(const uint64_t *have, uint64_t preimage_len, uint32_t group_log, uint32_t kind, uint64_t capacity,
                          uint64_t *run_first, uint64_t *run_count, uint64_t *n_runs, uint64_t *n_have);
int32_t b3w_bao_have_from_status(const uint8_t *unit_status, uint64_t preimage_len, uint32_t group_log, uint64_t *have);

/* ---- outboard diff: the chunks two versions of a file share, from their outboards alone (still ABI 1.4: new names only) ----
 * A replica that holds a stale version `a` of a file and its outboard wants version `b`, of which it has only the outboard and the
 * root.  Every unit's chaining value is stored in its parent's node, and two equal CVs mean equal bytes: comparing them names the
 * chunks a already has.  The result is a bitmap in the arrival-bitmap layout of the b lengths, so b3w_bao_have_runs_device, the set
 * slice calls and b3w_bao_set_slice_ingest_device (with this bitmap as d_have) follow unchanged.  Nothing is hashed and no file byte read.
 * A PAIR i is (file host_pair_a[i] of side a, file host_pair_b[i] of side b).  A side is its lengths, its outboards as
 * b3w_bao_outboard_batch_device (group_log 0) / b3w_bao_group_outboard_batch_device make them, each at byte host_ob_first[f] of
 * d_outboards (any 8-byte-aligned places, read at paired files only), its group_log and its roots (8 words a file).  The two sides
 * may be the same buffers, and a file may appear in many pairs.
 * With G = max(group_log_a, group_log_b) a UNIT is 2^G chunks, the last one of a file possibly ragged.  Its STORED CV is the file's
 * root where the unit is the whole file, else the left or right half of the node over the unit's parent subtree, which every
 * outboard of group_log <= G holds (the finer outboard is read at the coarser level).  Unit u of b is SAME iff it exists in a, covers
 * the same chunks in both, is the whole file in both or in neither, and the two stored CVs are equal.  Pair i owns
 * ceil(num_chunks(len_b) / 64) words from word host_word_first[i] of d_same (host_word_first = b3w_bao_have_layout of the pairs' b
 * lengths, n_pairs + 1 entries); bit c is set iff chunk c's unit is same.  Every word of every pair is written whole with its pad bits
 * zero and nothing else is written.  A set bit means equal bytes.  A clear bit means "differs or not known": a chunk with equal bytes
 * still gets a clear bit where another chunk of its unit differs, and where its unit is the whole file on one side only.
 * One launch, a wave per word; the table of pairs (40 bytes a pair) rides the context's staging; asynchronous on `stream`; the host
 * waits for nothing but this context's previous batch call.  n_pairs == 0 is a no-op.  B3W_E_BAD_ARGUMENT before anything is written
 * for a null or misaligned pointer (outboards and d_same 8-byte, roots 4-byte, every paired outboard's place 8-byte), a group_log
 * above B3W_BAO_MAX_GROUP_LOG, a pair index not below its side's file count, a file of more than 2^30 chunks, an outboard that
 * reaches past its buffer's bytes, a host_word_first that is not that layout, or more than 2^26 words.
 * When not to (MI355X): no call takes less than about 0.02 ms (the table's upload and one launch).  One 1 GiB file, 1 % of its
 * chunks rewritten: 0.033 ms with full outboards, where copying the two outboards' 134 MB device to device takes 0.046 (spread
 * 0.00004) and the route without this call - b3w_bao_verify_batch_device of b's RESIDENT bytes against a's outboard, then
 * b3w_bao_have_from_status_device - 0.457; with group outboards of 16 chunks 0.021 against 0.0096 for the copy of 8 MB (the fixed
 * cost shows) and 0.440 for that route.  262 144 files of 4 chunks: 1.17 ms against 0.034 for the copy and 1.99 for that route - the
 * host's table costs about 4 ns a pair and is 40 bytes a pair to upload, the one cost that follows the pair count.  So: not for a
 * caller who already holds b's bytes and has to verify them anyway (that route's statuses are the same bitmap and a verification
 * besides; this call verifies NOTHING and believes both outboards - a replica that does not trust b's outboard learns of a lie only
 * when b3w_bao_verify_batch_device runs over the finished file), and with very many tiny files the gain over that route shrinks to
 * 1.7 times. */
int32_t b3w_bao_outboard_diff_device(b3w_ctx *ctx, const uint64_t *host_lens_a, const uint64_t *host_ob_first_a, const uint8_t *d_outboards_a,
                                     uint64_t outboards_a_bytes, const uint32_t *d_roots_a, uint32_t n_files_a, uint32_t group_log_a,
                                     const uint64_t *host_lens_b, const uint64_t *host_ob_first_b, const uint8_t *d_outboards_b,
                                     uint64_t outboards_b_bytes, const uint32_t *d_roots_b, uint32_t n_files_b, uint32_t group_log_b,
                                     const uint32_t *host_pair_a, const uint32_t *host_pair_b, uint32_t n_pairs,
                                     const uint64_t *host_word_first /* n_pairs + 1 */, uint64_t *d_same, void *stream);
/* Host only, ONE pair: same_words [ceil(num_chunks(len_b) / 64)] receives the words the device call leaves for it.
 * B3W_E_BAD_ARGUMENT for a null pointer, a group_log above the maximum or a file of more than 2^30 chunks. */
int32_t b3w_bao_outboard_diff(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a /* 8 u32 */, uint32_t group_log_a,
                              const uint8_t *outboard_b, uint64_t len_b, const uint32_t *root_b /* 8 u32 */, uint32_t group_log_b,
                              uint64_t *same_words);

/* ---- outboard delta: the nodes of a new version that a replica does not hold, served and verified on arrival (still ABI 1.4: new
 * names only) ----
 * The diff above needs ALL of b's outboard on the replica (67 MB for 1 GiB) and believes it.  A DELTA carries only the parent nodes
 * of b that a does not already hold, and the replica checks every one of them against b's root before it writes a byte - by hashing
 * the nodes alone, no file byte is read on either side.  The outboard the replica ends with is consistent with b's root down to every
 * unit's chaining value, so the diff -> b3w_bao_have_runs_device -> set slices -> b3w_bao_set_slice_ingest_device chain then runs
 * against an outboard the replica can trust, and the chunks may come from anybody.
 * SIDES AND PAIRS as in the diff call, but both sides have ONE group_log g: U = units of 2^g chunks, b's tree has U_b - 1 parent nodes
 * in pre-order, node p spans units [lo, lo + cnt), cnt >= 2.  host_pair_a[i] == B3W_BAO_DELTA_NO_A: the replica holds nothing, and
 * nothing is SAME for that pair (side a may then be all null with n_files_a = 0).
 * SAME.  The root (p = 0) is SAME iff the two files have the same chunk count and equal roots.  Node p > 0 is SAME iff a's tree has a
 * parent node over the same units, that node covers the same chunks in both files (min((lo + cnt) << g, num_chunks) agrees), it is not
 * a's root, and the two STORED CVs - the half of the node above that holds the node's CV, in each outboard - are equal.
 * The DELTA of a pair is b's parent nodes that are not SAME, pointwise, in pre-order.  On two outboards that are each consistent with
 * their root this is "descend from the two roots and stop at equal nodes" (equal CVs mean equal nodes below); the provider is defined
 * pointwise so that it is exact on any input.
 * BLOB of a pair, little-endian, 8-byte aligned: 8 bytes len_b; 8 bytes k, the nodes present; W = ceil((U_b - 1) / 64) bitmap words
 * (bit p set iff node p is present, pad bits zero); the k present nodes in pre-order, each byte for byte b's outboard node.  A file
 * of one unit: W = 0, k = 0, 16 bytes.  b3w_bao_outboard_delta_bound = 16 + 8 W + 64 (U_b - 1) always suffices.
 * WHAT THE APPLY PROVES: the outboard it writes is consistent with b's root GIVEN that the subtrees copied from a were consistent
 * with the CVs a stores for them (a's outboard is the replica's own).  It proves nothing about file bytes: the chunks still arrive
 * through the verifying receivers.
 * When not to (MI355X, tools/bao_delta_measure.py; medians of whole calls, the copy's two series 0.00004 ms apart).
 * One 1 GiB file, 1 % of its chunks rewritten, full outboards: the blob is 4.7 MB against b's outboard of 67.1 MB (0.07 of it); the
 * provider takes 0.065 ms where copying the two outboards takes 0.046 and the diff 0.032; the apply takes 0.108 ms where copying
 * b's outboard - what a trusting replica did - takes 0.022 and b3w_bao_verify_batch_device over b's RESIDENT file, the only check
 * there was, 0.432.  With group outboards of 16 chunks the same edits touch 47 % of the nodes: 1.96 MB against 4.19, provider 0.039
 * (copy 0.0096, diff 0.021), apply 0.049 (copy 0.0068, verify 0.421) - at that grain a rewritten 1 % of chunks is half the tree, and
 * the delta saves half the bytes, no more.  HALF of the chunks rewritten (full outboards): 57.8 MB against 67.1 (0.86), provider 0.083,
 * apply 0.120 - the delta still costs less than verifying the file, but it saves almost nothing on the wire; send the outboard and
 * check it (outboard_check's route: 0.150 ms for 1 GiB, 0.35 of the verification, and no file byte needed).  262 144 files of 4
 * chunks, one chunk rewritten in every tenth: 9.6 MB against 52.4, but the provider takes 1.94 ms (diff 1.13, copy 0.034) and the
 * apply 2.02 where the verification of the resident files takes 1.52 and the copy 0.018: the host's table (72 bytes a pair to upload,
 * a few ns a pair to fill) and a workgroup's worth of scan per 1 024 pairs are the cost, and the kernels' share cannot be told apart
 * from the table's in these figures.  So: not for very many tiny files that are resident anyway, not where most of the tree
 * changed, and never as a check of file bytes. */
#define B3W_BAO_DELTA_NO_A 0xFFFFFFFFu
#define B3W_BAO_DELTA_MALFORMED 1
#define B3W_BAO_DELTA_BAD_HASH 2
#define B3W_BAO_DELTA_NOT_HELD 3
/* Host only.  The bytes that always suffice for one pair's blob (0: a group_log above the maximum); the extents of the pairs' blobs
 * at their bounds -> the total bytes, delta_first [n_pairs + 1] (host_pair_b NULL: pair i is file i; 0: a null pointer, a group_log
 * above the maximum or a pair index not below n_files_b); the scratch both device calls want for these pairs (0 likewise). */
uint64_t b3w_bao_outboard_delta_bound(uint64_t len_b, uint32_t group_log);
uint64_t b3w_bao_outboard_delta_layout(const uint64_t *host_lens_b, uint32_t n_files_b, const uint32_t *host_pair_b, uint32_t n_pairs, uint32_t group_log,
                                       uint64_t *delta_first);
uint64_t b3w_bao_outboard_delta_scratch_bytes(const uint64_t *host_lens_b, uint32_t n_files_b, const uint32_t *host_pair_b, uint32_t n_pairs,
                                              uint32_t group_log);
/* THE PROVIDER.  Pair i's blob goes to bytes [host_delta_first[i], host_delta_first[i + 1]) of d_delta: the caller chooses the
 * capacities, each extent 8-byte aligned and at least 16 + 8 W.  Every pair's header and bitmap are written whole, the nodes
 * [0, min(k, what the extent holds)); d_n_nodes[i] is k AS FOUND, even above the capacity (the header's k too), and nothing beyond the
 * extent is written - b3w_bao_have_runs_device's capacity rule.  No file byte is read and nothing is hashed.
 * At most FOUR launches whatever the pair and node counts: mark (a wave per bitmap word, a lane per node, the ballot the word), count
 * and scan (have_runs' scan over the words' counts), compact (a lane copies its node to its rank).  Nothing is allocated beyond
 * d_scratch (b3w_bao_outboard_delta_scratch_bytes) and the context's staging (72 bytes a pair); asynchronous on `stream`; the host
 * waits for nothing but this context's previous batch call.  n_pairs == 0 is a no-op.  B3W_E_BAD_ARGUMENT before anything is written
 * for what b3w_bao_outboard_diff_device refuses, two different group_logs, an extent too small for its header and bitmap, a
 * host_delta_first that is misaligned, does not rise (overlapping extents) or reaches past delta_bytes, a blob buffer that overlaps
 * either outboard buffer, or a scratch that is null, misaligned or too small. */
int32_t b3w_bao_outboard_delta_device(b3w_ctx *ctx, const uint64_t *host_lens_a, const uint64_t *host_ob_first_a, const uint8_t *d_outboards_a,
                                      uint64_t outboards_a_bytes, const uint32_t *d_roots_a, uint32_t n_files_a, const uint64_t *host_lens_b,
                                      const uint64_t *host_ob_first_b, const uint8_t *d_outboards_b, uint64_t outboards_b_bytes, const uint32_t *d_roots_b,
                                      uint32_t n_files_b, uint32_t group_log_a, uint32_t group_log_b, const uint32_t *host_pair_a, const uint32_t *host_pair_b,
                                      uint32_t n_pairs, const uint64_t *host_delta_first /* n_pairs + 1 */, uint8_t *d_delta, uint64_t delta_bytes,
                                      uint64_t *d_n_nodes, void *d_scratch, uint64_t scratch_bytes, void *stream);
/* THE REPLICA.  Side a is read only; of side b the call takes the lengths and the roots.  The blobs are UNTRUSTED: every index
 * derived from a blob is bounded by the extent before it is used, and a hostile blob yields a status, never a read or write outside
 * the buffers named in the call.  Per pair the status is the first that applies at the lowest node, d_first_bad that node (~0: none):
 *   B3W_BAO_DELTA_MALFORMED  the header's length is not len_b, k is not the bitmap's popcount or k nodes reach past the extent (all
 *                            three at node 0); a pad bit is set (at the bit's index); a present node whose parent is absent; the
 *                            root absent although it is not SAME; the root present although U_b = 1 (k is not 0 then)
 *   B3W_BAO_DELTA_BAD_HASH   a present node's parent compression (ROOT flag iff p = 0) is not b's root at p = 0, else not the half
 *                            of its parent's node in the blob
 *   B3W_BAO_DELTA_NOT_HELD   an absent child of a present node that is itself a parent subtree is not SAME against a's outboard (the
 *                            CV taken from the present node against a's stored CV); with B3W_BAO_DELTA_NO_A every such child
 * Status 0, and only then, writes the pair's output outboard whole at byte host_ob_first_out[i] of d_outboards_out: the length,
 * present nodes at their pre-order places, every absent node from a's outboard at the place of the same span in a's tree.  Any other
 * status leaves the output extent untouched.  The output extents lie in rising order of i and do not overlap.  Where the output
 * buffer overlaps a's outboard buffer the call is IN PLACE: every pair's output is then a's own outboard (same place, U_a = U_b); the
 * copies are no-ops and only present nodes are written - the equal-length recipe.  Any other overlap with a's outboards, and any
 * overlap with the blob buffer, is refused.
 * FOUR launches whatever the counts (count, scan, check, write; the write reads the pair's status on the device); no workgroup waits
 * for another; scratch, staging and stream as the provider.  B3W_E_BAD_ARGUMENT before anything is written for what the provider
 * refuses on side a, the lengths, the pairs and host_delta_first, and for the outputs as said above. */
int32_t b3w_bao_outboard_delta_apply_device(b3w_ctx *ctx, const uint64_t *host_lens_a, const uint64_t *host_ob_first_a, const uint8_t *d_outboards_a,
                                            uint64_t outboards_a_bytes, const uint32_t *d_roots_a, uint32_t n_files_a, const uint64_t *host_lens_b,
                                            const uint32_t *d_roots_b, uint32_t n_files_b, uint32_t group_log, const uint32_t *host_pair_a,
                                            const uint32_t *host_pair_b, uint32_t n_pairs, const uint64_t *host_delta_first /* n_pairs + 1 */,
                                            const uint8_t *d_delta, uint64_t delta_bytes, const uint64_t *host_ob_first_out /* n_pairs */,
                                            uint8_t *d_outboards_out, uint64_t outboards_out_bytes, int32_t *d_pair_status, uint64_t *d_first_bad,
                                            void *d_scratch, uint64_t scratch_bytes, void *stream);
/* Host only, ONE pair, the device calls' bytes and statuses (outboard_a NULL: B3W_BAO_DELTA_NO_A).  The provider writes into
 * blob [blob_bytes >= 16 + 8 W] by the capacity rule and *n_nodes = k as found.  The replica reads blob [blob_bytes] and, with
 * *status 0 only, writes outboard_out [8 + 64 (U_b - 1)], which may be outboard_a itself where U_a = U_b.  B3W_E_BAD_ARGUMENT for a
 * null pointer, a group_log above the maximum, a file of more than 2^30 chunks or a blob_bytes below 16 + 8 W. */
int32_t b3w_bao_outboard_delta(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a /* 8 u32 */, const uint8_t *outboard_b, uint64_t len_b,
                               const uint32_t *root_b /* 8 u32 */, uint32_t group_log, uint8_t *blob, uint64_t blob_bytes, uint64_t *n_nodes);
int32_t b3w_bao_outboard_delta_apply(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a /* 8 u32 */, uint64_t len_b,
                                     const uint32_t *root_b /* 8 u32 */, uint32_t group_log, const uint8_t *blob, uint64_t blob_bytes,
                                     uint8_t *outboard_out, int32_t *status, uint64_t *first_bad);

/* ---- range slices: the slice of a run of chunks, extracted and taken in (still ABI 1.4: new names only) -------------
 * The run lists above name what is missing as rows (file, first chunk, chunks); the slice calls above carry ONE chunk a slice, so a
 * run of k chunks costs k slices and k whole paths (2 312 bytes for 1 024 of payload in a file of 2^20 chunks).  A RANGE SLICE carries
 * every shared node once.  A range is (file f, first chunk a, chunks k), k >= 1, a + k <= b3w_chain_num_chunks(len_f).  Its slice is the
 * 8-byte little-endian length, then the tree in pre-order restricted to the range: a parent node whose span meets [a, a + k) gives its
 * 64 bytes, then its left subtree if that meets the range, then its right one likewise; a chunk c of the range gives its
 * min(1024, len - 1024 c) bytes.  This is the slice `bao slice` makes for those bytes; an empty file's slice is its header.  With
 * k = 1 it is b3w_bao_slice's slice byte for byte.
 * PLACES.  U(a, c) = the parent nodes whose span meets [a, c] (the union of the paths of chunks a .. c).  Chunk c lies at
 * 8 + 64 U(a, c) + 1024 (c - a); a node X over [lo, hi) that meets the range, c0 = max(lo, a), lies at place(c0) - 64 (the nodes of
 * c0's path at or below X).  The size is 8 + 64 U(a, a + k - 1) + the range's bytes: 1 114 696 for 1 024 aligned chunks of 2^20
 * (1.063 times the payload; 1 024 one-chunk slices are 2.258 times).
 * PACKING.  Slice r starts at slice_first[r], 8 modulo 16 as b3w_bao_slice_batch_layout does it: with d_slices 16-byte aligned every
 * node sits 8 off a 16-byte boundary and every chunk on one.  Padding is neither read nor written.
 * THE RECEIVER IS DEFINED BY PROJECTION.  The projection of a range slice onto chunk c — the header, the nodes of c's path found in
 * the slice root first, c's bytes — is the one-chunk slice of c.  Chunk status = b3w_bao_slice_decode's status of the projection (3 the
 * header is not the length, 2 a path node or the root fails, 1 the chunk's bytes fail, the first that applies; a one-chunk file's
 * wrong root is 1).  Writes = the union over the chunks of status 0 of what b3w_bao_slice_ingest writes for the projection: the
 * chunk's bytes and no byte beside them, the STORED nodes of its path (group_log 0: all; above 0: those above the group, the others are
 * verified and dropped), the header; and the chunk's bit in the bitmap where one is given.  Nothing unverified is written: a bad node
 * keeps out the chunks below it and no other.  Range status = the largest chunk status of the range, range first bad = the first
 * chunk (its index within the file) whose status is not 0, UINT64_MAX when there is none — what b3w_bao_verify_ranges_batch_device
 * reports for a range.  Ranges may overlap, repeat and come in any order, in one call and across calls: every writer of a byte that
 * writes at all writes the same verified value. */
/* Host only.  The slice's byte count; 0 for n_chunks == 0 or a range that reaches past the file's chunk count. */
uint64_t b3w_bao_range_slice_size(uint64_t preimage_len, uint64_t first_chunk, uint64_t n_chunks);
/* Host only.  slice_first [n_ranges + 1] -> the total bytes, or -B3W_E_BAD_ARGUMENT (a null pointer, a file index >= n_files, a range
 * b3w_bao_range_slice_size refuses), like b3w_bao_slice_batch_layout. */
int64_t b3w_bao_range_slice_batch_layout(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                                         const uint64_t *host_count, uint32_t n_ranges, uint64_t *slice_first /* n_ranges + 1 */);
/* Host only.  The slice of one range from the file's outboard (group_log 0: the full one; 1 .. 6: the group outboard) and range_bytes:
 * the bytes of the range's chunks (group_log 0), or of the whole groups the range touches, from the first chunk of the first such
 * group, clipped to the file (group_log > 0: the nodes inside those groups are recomputed from them).  out == NULL: -> the size.
 * Otherwise -> the bytes written (the size), or -B3W_E_BAD_ARGUMENT for a refused range, a group_log above the maximum, a null pointer
 * (range_bytes may be NULL for an empty file) or out_len below the size. */
int64_t b3w_bao_range_slice(const uint8_t *outboard, uint64_t preimage_len, uint32_t group_log, uint64_t first_chunk, uint64_t n_chunks,
                            const uint8_t *range_bytes, uint8_t *out, uint64_t out_len);
/* Host only.  The sequential top-down decoder: the slice is read front to back, every node against its half of the node above it.
 * *out_status / *out_first_bad (may be NULL) are the range status and first bad chunk defined above; out_bytes (may be NULL; room for
 * 1024 n_chunks) receives the bytes of the chunks of status 0 at 1024 (c - first_chunk), the others' places are left alone.
 * B3W_E_BAD_ARGUMENT for a null slice, root or out_status, a refused range, or a slice_len that is not b3w_bao_range_slice_size. */
int32_t b3w_bao_range_slice_decode(const uint8_t *slice, uint64_t slice_len, uint64_t preimage_len, uint64_t first_chunk, uint64_t n_chunks,
                                   const uint32_t *root /* 8 u32 */, uint8_t *out_bytes, int32_t *out_status, uint64_t *out_first_bad);
/* Host only.  The receiver for ONE range: the same verdict and the writes defined above into `data` (the file), `outboard` (its
 * outboard of this group_log) and `have` (may be NULL; the file's bitmap from its word 0).  Refuses what the decoder refuses, a
 * group_log above the maximum and a null outboard (data may be NULL only for an empty file). */
int32_t b3w_bao_range_slice_ingest(const uint8_t *slice, uint64_t slice_len, uint64_t preimage_len, uint64_t first_chunk, uint64_t n_chunks,
                                   const uint32_t *root /* 8 u32 */, uint32_t group_log, uint8_t *data, uint8_t *outboard, uint64_t *have,
                                   int32_t *out_status, uint64_t *out_first_bad);
/* THE PROVIDER.  The range slices of ranges (host_files[r], host_first[r], host_count[r]) into d_slices (16-byte aligned, packed as
 * b3w_bao_range_slice_batch_layout says); the other arguments are b3w_bao_slice_arena_device's.  Nothing is verified.  Only each
 * slice's own bytes are written, each by one lane; no byte outside a range's own file is read.  group_log > 0: the chunks of every
 * group the range touches are hashed and the nodes inside those groups come from that, as in b3w_bao_slice_arena_device.
 * Both device calls: a ROW is (range, block of B aligned chunks).  A range of at most 64 chunks takes rows of B = 64, a wave each (one
 * or two a range); a longer one takes a workgroup of 1 024 lanes per tile of 1 024 chunks it touches.  At most TWO launches here and
 * THREE in the receiver (the rows of each kind, and a wave per range that reduces its rows' results), whatever the ranges; no
 * workgroup waits for another.  One table (64 bytes a range, 8 a row) goes through the context's staging and nothing else is
 * allocated; asynchronous on `stream`; any context; the host waits for nothing but this context's previous batch call.  REFUSALS ARE
 * ATOMIC (B3W_E_BAD_ARGUMENT before anything is launched or written; b3w_last_error names the range): what the one-chunk twins refuse,
 * a range with count 0 or that reaches past its file's chunk count, more than 2^31 - 1 rows of one kind.  n_ranges == 0: a no-op. */
int32_t b3w_bao_range_slice_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                         const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards,
                                         const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count,
                                         uint32_t n_ranges, uint8_t *d_slices, void *stream);
/* Host only.  Bytes of scratch the receiver needs: 16 per row (0 for a null pointer or a range the layout call refuses). */
uint64_t b3w_bao_range_slice_ingest_scratch_bytes(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files,
                                                  const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges);
/* THE RECEIVER, with the semantics above; the arguments of b3w_bao_slice_ingest_have_device with (first, count) for the chunk, the two
 * range outputs (int32, and uint64 8-byte aligned, in the order the ranges were given; neither needs clearing) for the sample status,
 * d_have (may be NULL: no record; else 8-byte aligned, bits set with one atomic OR of a whole word per wave) and the scratch (16-byte
 * aligned, b3w_bao_range_slice_ingest_scratch_bytes).  Every node of the slice inside a block is hashed once by its row, in LDS, and
 * the verdicts go down through flags as in the ranged verification; the nodes above a block (at most 22 for files up to 4 GiB) are
 * checked once per row, side by side.  Also refused: a scratch that is too small, null or misaligned, a misaligned d_have, a null or
 * misaligned output.
 * WHEN NOT TO (MI355X, one 1 GiB file; the yardstick is a build of the commit before these calls doing the same job with
 * one slice a chunk: bao.runs_chunks + b3w_bao_slice_arena_device, b3w_bao_slice_ingest_have_device).  64 runs of 1 024 chunks at starts
 * that are not tile-aligned (68 MiB of slices against 145): the provider 0.081 ms against 4.37, the receiver 0.214 against 1.525 (the
 * yardstick's spread 0.047 and 0.0003); at group_log 4 0.158 and 0.202, the file at 1 modulo 16 0.084 and 0.222.  4 096 runs of 16: 0.32
 * against 4.25 and 0.47 against 1.52.  The whole file as one range: 1.11 ms to take in (bao.verify_batch plus a device copy of the
 * bytes: 0.85) and 0.80 to extract.  SHORT RUNS LOSE IN THE RECEIVER: a range takes at least a wave, and a wave with one or two busy
 * lanes hashes no faster than the one-chunk kernel's sixteen samples a wave.  65 536 runs of ONE chunk (the same bytes either way): the
 * receiver 7.31 ms against 1.53, the provider 5.35 against 5.16 (spread 0.65); the 262 507 runs of a bitmap with half its chunks
 * missing (2 chunks a run on average, 851 MiB of slices against 1 158): the provider 13.3 ms against 38.7, the receiver 21.1 against
 * 11.7.  So: range slices for runs from about sixteen chunks on, where they save both bytes and time; runs of one or two chunks
 * through bao.runs_chunks and the one-chunk calls, unless the bytes on the wire matter more than the receiver's milliseconds.  Where
 * between 2 and 16 chunks a run the two cross was not measured, nor were files past 1 GiB or the kernels one by one. */
int32_t b3w_bao_range_slice_ingest_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                          const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint8_t *d_outboards,
                                          const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first,
                                          const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices, int32_t *d_range_status,
                                          uint64_t *d_range_first_bad, uint64_t *d_have /* may be NULL */, void *d_scratch,
                                          uint64_t scratch_bytes, void *stream);
/* THE PROVER: step records of challenged chunk RUNS planned from range slices alone, b3w_sample_plan_slices_device's twin.  DEFINED BY
 * PROJECTION like the receiver: for every chunk c of every range, the status is the one b3w_sample_plan_slices_device gives the
 * projection of the range slice onto c (3 header, 2 a path node or the root, 1 the chunk's bytes, 0 verified; 3 over 2 over 1; a
 * one-chunk file's wrong root is 1), and the records are word for word the rows that call writes for the projection: the leaf
 * blocks, then the parent steps bottom up - the chained words where the chunk failed or its path is not provable
 * (b3w_chain_path_provable), the words straight from the nodes otherwise.  Records are written for failing chunks too; a bad node
 * spoils the chunks below it and no other.  Ranges may overlap, repeat and come in any order; each writes its own rows.
 * ROWS.  Range r owns rows [range_row_first[r], range_row_first[r + 1]), its chunks in ascending order, each chunk's rows as
 * b3w_sample_rows_batch lays out one sample: the rows are exactly b3w_sample_rows_batch's over the ranges broken into chunks.  The
 * per-chunk outputs are packed the same way: range r's chunks at [chunk_first[r], chunk_first[r] + host_count[r]), chunk_first the
 * running sum of the counts. */
/* Host only.  range_row_first [n_ranges + 1]; chunk_row_first (NULL, or the total chunk count + 1: every chunk's first row, the total
 * behind them) and chunk_provable (NULL, or the total chunk count: b3w_chain_path_provable of every chunk) are filled only when asked
 * for.  -> the total rows, or -B3W_E_BAD_ARGUMENT for what b3w_bao_range_slice_batch_layout refuses.  The per-range totals are a
 * closed form (the sum of the path lengths over a prefix of the tree, O(depth) a range); only the two optional arrays cost a step
 * a chunk. */
int64_t b3w_sample_rows_ranges(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                               const uint64_t *host_count, uint32_t n_ranges, uint64_t *range_row_first /* n_ranges + 1 */,
                               uint64_t *chunk_row_first /* NULL, or total chunks + 1 */, uint8_t *chunk_provable /* NULL, or total chunks */);
/* d_slices: the packed range slices (16-byte aligned, b3w_bao_range_slice_batch_layout); d_records: 32 words a row,
 * b3w_sample_rows_ranges' total; d_chunk_status: an int32 a chunk; d_range_status / d_range_first_bad: what
 * b3w_bao_range_slice_ingest_device gives (the largest chunk status; the first chunk of the file whose status is not 0, UINT64_MAX
 * for none; 8-byte aligned).  THE SCRATCH is 16 bytes a row of the table (16-byte aligned): the rows are the receiver's, so its size
 * is what b3w_bao_range_slice_ingest_scratch_bytes says for the same ranges.  A row is (range, block of 64 or 1 024 aligned chunks) as
 * in the receiver: lane = chunk; the chunk's leaf records written in place while its CV goes to LDS; the block's nodes hashed once in
 * LDS and the nodes above it side by side; then every lane writes its parent records from the slice's own nodes.  At most THREE
 * launches (short rows, tile rows, the per-range reduce); one table (64 bytes a range, 16 a row) through the context's staging and
 * nothing else allocated; asynchronous on `stream`; nova contexts only.  Every byte and row count is 64 bits wide: a whole 1 GiB file
 * as one range is 37 748 736 rows, 4.8 GB of records.  n_ranges == 0: a no-op.  REFUSALS ARE ATOMIC (B3W_E_BAD_ARGUMENT before
 * anything is launched or written - records, statuses, range outputs and scratch untouched; b3w_last_error names the range): a null
 * or misaligned pointer, a scratch that is too small, a file index >= n_files, a range with count 0 or that reaches past its file's
 * chunk count, a file of more than 2^30 chunks, more than 2^31 - 1 rows of one kind, a context that is not a nova circuit's.
 * WHEN NOT TO (MI355X, one 1 GiB file; the yardstick is a build of the commit before this call planning the same chunks
 * from one-chunk slices with b3w_sample_plan_slices_device).  64 runs of 1 024 chunks at starts that are not tile-aligned: 0.432 ms
 * against 1.714 (the yardstick's spread 0.0008), 302 MB of records at 700 GB/s; 4 096 runs of 16: 0.525 against 1.715.  SHORT RUNS LOSE
 * as in the receiver: a range takes at least a wave, and its one busy lane writes the parent rows the one-chunk kernel spreads over
 * sixteen lanes - 65 536 runs of ONE chunk 7.93 ms against 1.72, the 262 507 runs of a half-missing bitmap 23.4 against 13.4.  So:
 * runs of one or two chunks through bao.runs_chunks and b3w_sample_plan_slices_device, longer ones through this call; where between
 * 2 and 16 chunks a run the two cross was not measured, nor were files past 1 GiB. */
int32_t b3w_sample_plan_range_slices_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *d_roots,
                                            const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count,
                                            uint32_t n_ranges, const uint8_t *d_slices, uint32_t *d_records, int32_t *d_chunk_status,
                                            int32_t *d_range_status, uint64_t *d_range_first_bad, void *d_scratch, uint64_t scratch_bytes,
                                            void *stream);

/* ---- set slices: ONE slice for all the wanted runs of a file, extracted and taken in (still ABI 1.4: new names only) -
 * A range slice carries one run, and every run repeats its whole path down from the root: the 262 507 runs of a half-arrived 1 GiB file
 * are 892 MB of range slices for 537 MB of payload, and a run of one or two chunks keeps one or two lanes of its wave busy.  A SET SLICE
 * carries the union of a file's runs, every shared node once - the response to a multi-range bao request.
 * THE RANGE LIST.  The calls take the range calls' (host_files, host_first, host_count, n_ranges) with one more condition: the ranges
 * come ascending by (file, first chunk) and disjoint - within a file first[i] >= first[i-1] + count[i-1]; touching runs are allowed.
 * This is what b3w_bao_have_runs_device emits.  A SET is the maximal stretch of consecutive ranges of one file, so a file appears in at
 * most one set; sets are numbered in order of appearance; S is the union of a set's ranges.
 * THE SET SLICE is the 8-byte little-endian length, then the tree in pre-order restricted to S: a parent node whose span meets S gives
 * its 64 bytes, then its left subtree if that meets S, then its right one likewise; a chunk c of S gives its min(1024, len - 1024 c)
 * bytes.  With one run it is the range slice byte for byte; with every chunk the whole-file range slice.
 * PLACES.  U_S(c) = the parent nodes whose span meets S n [0, c]; rank_S(c) = the chunks of S below c.  Chunk c of S lies at
 * 8 + 64 U_S(c) + 1024 rank_S(c) (only the file's last chunk is short, and nothing follows it).  A node X over [lo, lo + size) that
 * meets S, c0 = min(S n span), lies at place(c0) - 64 (the nodes of c0's path at or below X): between X and c0 the slice holds c0's
 * path alone.  The size is 8 + 64 U_S(max S) + the bytes of S: never more than the sum of the runs' range slices, and less whenever a
 * file of more than one chunk has more than one run.
 * PACKING.  Set s starts at slice_first[s], 8 modulo 16, as b3w_bao_range_slice_batch_layout does it.
 * THE RECEIVER IS DEFINED BY PROJECTION, as the range receiver with "range" read as "set": the projection of a set slice onto one of its
 * chunks is that chunk's one-chunk slice; chunk status = b3w_bao_slice_decode's status of the projection (3 over 2 over 1; a one-chunk
 * file's wrong root is 1); writes = the union over the chunks of status 0 of what b3w_bao_slice_ingest writes for the projection (the
 * chunk's bytes, the stored nodes of its path at this group_log, the header, the chunk's bit where a bitmap is given).  Nothing
 * unverified is written; a bad node keeps out the chunks below it and no other.  Set status = the largest chunk status; set first bad =
 * the first chunk of the file whose status is not 0, UINT64_MAX for none.  Per-chunk statuses are packed set by set: set s's wanted
 * chunks, ascending, at [set_chunk_first[s], set_chunk_first[s + 1]). */
/* The host calls below take files of any length; the DEVICE calls refuse a file of more than 2^30 chunks (1 TiB), whose blocks lie
 * deeper than the 24 places a row of their table carries. */
/* Host only.  The bytes of one file's set slice, O(ranges x depth), no step a chunk; 0 for an empty list or a refused one (an empty
 * run, one past the file's chunk count, a list that is not ascending or not disjoint). */
uint64_t b3w_bao_set_slice_size(uint64_t preimage_len, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges);
/* Host only.  The sets of a range list and where their slices lie -> the total bytes, or -B3W_E_BAD_ARGUMENT (a null list, a file
 * index >= n_files, a list b3w_bao_set_slice_size refuses, files that do not ascend).  Every output may be NULL: set_file (room for
 * n_ranges), set_range_first (n_ranges + 1: set s is ranges [set_range_first[s], set_range_first[s + 1])), set_chunk_first
 * (n_ranges + 1: the running sum of the sets' wanted chunks, the index base of the per-chunk status), slice_first (n_ranges + 1),
 * *n_sets.  Only the first *n_sets (+ 1) entries are written. */
int64_t b3w_bao_set_slice_batch_layout(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                                       const uint64_t *host_count, uint32_t n_ranges, uint32_t *set_file, uint32_t *set_range_first,
                                       uint64_t *set_chunk_first, uint64_t *slice_first, uint32_t *n_sets);
/* Host only.  The set slice of one file from its outboard of this group_log and the FILE's bytes (`data`: the whole file's place; at
 * group_log 0 only the chunks of S are read, above 0 the chunks of every group S touches, and the nodes inside those groups are
 * recomputed).  out == NULL: -> the size.  Otherwise -> the bytes written, or -B3W_E_BAD_ARGUMENT for a refused list, a group_log
 * above the maximum, a null pointer (data may be NULL for an empty file) or out_len below the size. */
int64_t b3w_bao_set_slice(const uint8_t *outboard, uint64_t preimage_len, uint32_t group_log, const uint64_t *host_first,
                          const uint64_t *host_count, uint32_t n_ranges, const uint8_t *data, uint8_t *out, uint64_t out_len);
/* Host only.  The sequential top-down decoder.  out_bytes (may be NULL; room for 1024 |S|) gets the bytes of the chunks of status 0 at
 * 1024 rank_S(c), the others' places are left alone; chunk_status (may be NULL) one int32 a wanted chunk, ascending; *out_first_bad may
 * be NULL.  B3W_E_BAD_ARGUMENT for a null slice, root or out_status, a refused list, or a slice_len that is not
 * b3w_bao_set_slice_size. */
int32_t b3w_bao_set_slice_decode(const uint8_t *slice, uint64_t slice_len, uint64_t preimage_len, const uint64_t *host_first,
                                 const uint64_t *host_count, uint32_t n_ranges, const uint32_t *root /* 8 u32 */, uint8_t *out_bytes,
                                 int32_t *chunk_status, int32_t *out_status, uint64_t *out_first_bad);
/* Host only.  The receiver for ONE file: the decoder's verdicts and the writes defined above into `data` (the file), `outboard` (its
 * outboard of this group_log) and `have` (may be NULL; the file's bitmap from its word 0).  Refuses what the decoder refuses, a
 * group_log above the maximum and a null outboard (data may be NULL only for an empty file). */
int32_t b3w_bao_set_slice_ingest(const uint8_t *slice, uint64_t slice_len, uint64_t preimage_len, const uint64_t *host_first,
                                 const uint64_t *host_count, uint32_t n_ranges, const uint32_t *root /* 8 u32 */, uint32_t group_log,
                                 uint8_t *data, uint8_t *outboard, uint64_t *have, int32_t *chunk_status, int32_t *out_status,
                                 uint64_t *out_first_bad);
/* THE PROVIDER.  The set slices of the list's sets into d_slices (16-byte aligned, packed as b3w_bao_set_slice_batch_layout says); the
 * other arguments are b3w_bao_range_slice_arena_device's.  Nothing is verified; every byte of a slice has one writer; no byte outside
 * a set's own file is read; padding is not written.  group_log > 0: the chunks of every touched group are hashed and the nodes inside
 * the groups come from that, as the range provider does.
 * Both device calls: a ROW is (set, block of B aligned chunks with at least one wanted chunk).  A set whose first and last wanted
 * chunks lie in the same or in adjacent aligned 64-chunk blocks takes one or two rows of B = 64, a wave each (every file of at most 64
 * chunks); any other set a workgroup of 1 024 lanes per touched tile - the 262 507 runs of a half-arrived 1 GiB file are 1 024
 * workgroups with every wanted lane busy.  The device never sees the run list: a row carries the mask of its wanted chunks.  At most
 * TWO launches here and THREE in the receiver (the rows of each kind, and a wave per set that reduces its rows' results); no workgroup
 * waits for another.  THE TABLE grows with sets and rows, never with ranges or chunks: 64 bytes a set, and a row of 64 chunks 224
 * bytes, one of 1 024 chunks 344: set and block (8), the place of the row's first wanted chunk and its rank (16), the places of the
 * D <= 24 nodes above the block in the slice (192: files of up to 2^30 chunks; a longer file is refused), the mask (8 or 128); a
 * node above a block is moved by the row that holds the first wanted chunk below it, which the row reads off the places (the
 * receiver stores it from every row with a verified chunk: the same verified bytes).  It goes through the context's staging
 * and nothing else is allocated; asynchronous on `stream`; the host waits for nothing but this context's previous batch call; every
 * byte count and place is 64 bits wide.  REFUSALS ARE ATOMIC (B3W_E_BAD_ARGUMENT before anything is launched or written;
 * b3w_last_error names the range): what the range twins refuse, a list that is not ascending or not disjoint (named as such), a file
 * of more than 2^30 chunks, more than 2^31 - 1 rows of one kind.  n_ranges == 0: a no-op. */
int32_t b3w_bao_set_slice_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                       const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards,
                                       const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count,
                                       uint32_t n_ranges, uint8_t *d_slices, void *stream);
/* Host only.  Bytes of scratch the receiver needs: 16 per row (0 for a null pointer or a list the layout call refuses). */
uint64_t b3w_bao_set_slice_ingest_scratch_bytes(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files,
                                                const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges);
/* THE RECEIVER, with the semantics above; b3w_bao_range_slice_ingest_device's arguments with the two outputs a SET (int32, and uint64
 * 8-byte aligned, in set order) and d_chunk_status (may be NULL; an int32 a wanted chunk at set_chunk_first[s] + rank).  Also refused:
 * a scratch that is too small, null or misaligned, a misaligned d_have or d_chunk_status, a null or misaligned output.
 * WHEN NOT TO (MI355X, one 1 GiB file; the yardsticks are a build of the commit before these calls doing the same job by
 * both existing routes, its range calls and bao.runs_chunks + its one-chunk calls; device events round whole calls; no profiler run).
 * The 262 507 runs of a bitmap with half its chunks missing (593 MB of set slice, 892 of range slices, 1 213 of one-chunk slices): the
 * provider 3.20 ms against 13.22 (range) and 16.18 (one-chunk), the receiver 3.70 against 20.86 and 16.85, the yardsticks' spreads
 * below 0.23; 65 536 runs of ONE chunk: 0.78 against 3.51 and 1.73, 1.30 against 5.45 and 2.17.  FEW WANTED CHUNKS IN MANY TILES LOSE
 * TO THE RANGE CALLS: a set takes a workgroup of 1 024 lanes per touched tile, and 4 096 runs of 16 scattered over the file keep 64
 * lanes of each of 1 009 tiles busy - the provider 0.35 ms against the range call's 0.25, the receiver 0.78 against 0.39 (the one-chunk
 * route 1.50 and 2.16).  LONG RUNS GAIN NOTHING: 64 runs of 1 024 chunks 0.110 against the range provider's 0.081 and 0.237 against
 * the range receiver's 0.214 (at group_log 4: 0.190 / 0.158 and 0.226 / 0.202), for 0.03 % fewer bytes.  One cause that is known and
 * was not measured apart: the tile kernels take 92 and 76 VGPRs, so ONE workgroup of 1 024 lanes is resident a CU where the range
 * tile kernels (52 / 53) fit two.  So: set slices for the many
 * short runs of a half-arrived file, the range calls for a few long runs or a sparse scatter of medium ones; the one-chunk calls win
 * none of these shapes against the better of the two.  The list must be ascending and disjoint and a file is in one set a call, which
 * the range calls do not ask.  Not measured: where between 64 and 512 wanted chunks a tile the two cross, files past 1 GiB, many files
 * a call, the kernels one by one. */
int32_t b3w_bao_set_slice_ingest_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                        const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint8_t *d_outboards,
                                        const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first,
                                        const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices, int32_t *d_set_status,
                                        uint64_t *d_set_first_bad, int32_t *d_chunk_status /* may be NULL */,
                                        uint64_t *d_have /* may be NULL */, void *d_scratch, uint64_t scratch_bytes, void *stream);
/* THE PLANNER: the prover's side of set slices, the twin of b3w_sample_plan_range_slices_device.  The list is the set calls' list
 * (ascending by (file, first chunk), disjoint, touching runs allowed); d_slices is packed as b3w_bao_set_slice_batch_layout says.
 * SEMANTICS, BY PROJECTION: every wanted chunk c of every set gets the status b3w_sample_plan_slices_device gives the projection of
 * the set slice onto c (3 over 2 over 1; a one-chunk file's wrong root is 1) and, word for word, the rows that call writes for the
 * projection - leaf blocks first, then parent steps bottom up; the chained words where the chunk failed or b3w_chain_path_provable
 * says no, the words straight from the nodes otherwise.  Records are written for failing chunks too.  A bad node spoils the wanted
 * chunks below it, in every row under it, and no other.  d_set_status / d_set_first_bad are what b3w_bao_set_slice_ingest_device
 * reports.
 * THE OUTPUT LAYOUT NEEDS NO NEW HOST CALL.  For an ascending disjoint list a set's wanted chunks in ascending order are the list's
 * chunks in order, so the rows are exactly b3w_sample_rows_ranges' over the same list: set s owns rows
 * [range_row_first[set_range_first[s]], range_row_first[set_range_first[s + 1]]), and its chunk statuses lie at set_chunk_first[s] +
 * rank, which is the running sum of the counts.  UNTAMPERED, d_records AND d_chunk_status ARE BYTE FOR BYTE WHAT
 * b3w_sample_plan_range_slices_device WRITES FOR THE SAME LIST FROM RANGE SLICES.
 * The kernel runs on the set receiver's rows and table (lane = chunk, `mine` the row's mask bit, so every wanted lane of a tile is
 * busy); beside the table a row carries the 64-bit number of its first record row, 8 bytes, from a closed form on the host (O(depth)
 * a run and a row, no step a chunk).  At most THREE launches (tile rows, rows of 64, b3w_bao_set_slice_ingest_device's reduce); one
 * table through the context's staging and nothing else allocated; asynchronous on `stream`; nova contexts only.  THE SCRATCH is 16
 * bytes a row: b3w_bao_set_slice_ingest_scratch_bytes for the same list.  Rows, places and byte counts are 64 bits wide.
 * n_ranges == 0: a no-op.  REFUSALS ARE ATOMIC (B3W_E_BAD_ARGUMENT before anything is launched or written - records, statuses, set
 * outputs and scratch untouched; b3w_last_error names the range): what the set calls refuse about the list (an unsorted or overlapping
 * one is named as such), a null or misaligned pointer, a scratch that is too small, a file of more than 2^30 chunks, more than
 * 2^31 - 1 rows of one kind, a context that is not a nova circuit's.
 * WHEN NOT TO (MI355X, one 1 GiB file; the yardsticks are a build of the commit before this call planning the same chunks,
 * b3w_sample_plan_range_slices_device over range slices and bao.runs_chunks + b3w_sample_plan_slices_device over one-chunk slices;
 * device events round whole calls, the three routes' records compared word for word before timing; no profiler run).  The 262 507 runs
 * of a bitmap with half its chunks missing, 2.4 GB of records: 5.08 ms against 18.38 (one-chunk, the faster; spread 0.03) and 23.10
 * (range; 0.08), from 593 MB of slices where the yardsticks read 1 213 and 892; 65 536 runs of ONE chunk: 1.53 against 2.01 (0.0005) and
 * 5.95 (0.06).  FEW WANTED CHUNKS IN MANY TILES LOSE TO THE RANGE PLANNER, as in the receiver: 4 096 runs of 16 scattered over the file
 * keep 64 lanes of each of 1 009 workgroups of 1 024 busy - 0.733 ms against the range planner's 0.447 (spread 0.001; one-chunk 1.80).
 * LONG RUNS GAIN NOTHING: 64 runs of 1 024 chunks 0.454 against 0.431 (0.0001), for 0.03 % fewer bytes.  So: this call for the many
 * short runs of a half-arrived file, the range planner for a few long runs or a sparse scatter of medium ones; the one-chunk planner
 * wins none of these shapes against the better of the two.  The list must be ascending and disjoint and a file is in one set a call,
 * which the range planner does not ask.  Not measured: where between 64 and 512 wanted chunks a tile the two cross, files past 1 GiB,
 * many files a call, the kernels one by one.  Not tested on the device: records past 2^32 bytes (4.8 GB of output; the host side of
 * it is held by tools/bao_set_plan_host_check.cpp). */
int32_t b3w_sample_plan_set_slices_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *d_roots,
                                          const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count,
                                          uint32_t n_ranges, const uint8_t *d_slices, uint32_t *d_records, int32_t *d_chunk_status,
                                          int32_t *d_set_status, uint64_t *d_set_first_bad, void *d_scratch, uint64_t scratch_bytes,
                                          void *stream);
/* THE PROVIDER FROM PACKED CHUNK BYTES ("sparse calls from packed chunk bytes" below): b3w_bao_set_slice_arena_device for files that
 * are not resident, (d_packed, packed_bytes) in place of (d_arena, arena_bytes, host_offsets).  EVERY OUTPUT BYTE IS WHAT THE ARENA
 * CALL WRITES for an arena with the same file bytes, outboards, list and group_log, and every byte it leaves alone stays.  The layout
 * is b3w_bao_packed_layout's over the same list: a file of at most 64 chunks lists all its chunks, any other file every chunk of
 * every group of 2^group_log chunks the set touches.  Beside the table a row carries the slot of its block's first listed chunk (8
 * bytes, looked up in the layout's runs on the host); a lane reads at its rank among the block's LISTED lanes - the mask bits at
 * group_log 0, the lanes of the touched groups above 0, every lane in a file of at most 64 chunks - and keeps its chunk index for the
 * counter and the length.  At most TWO launches, the same table, nothing allocated, any byte alignment of d_packed; no byte behind
 * total_bytes is read.  Refused, atomically: what the arena call refuses without the arena items, a null d_packed with
 * total_bytes > 0, packed_bytes < total_bytes (the message says how many are needed).
 * WHEN NOT TO (the same run; the yardstick is the parent's b3w_bao_set_slice_arena_device over the resident file, the two calls' slices
 * compared byte for byte before timing): a file that IS resident.  The packed call is never faster, and with many runs it is FAR
 * behind: the half-missing shape 7.04 ms against 3.18 (spread 0.001), 65 536 runs of one chunk 1.80 against 0.79, 4 096 runs of 16
 * 0.516 against 0.349; 64 runs of 1 024 chunks 0.134 against 0.113 (0.190 / 0.187 at group_log 4).  The kernels read the same bytes;
 * what the call adds is the packed layout over the run list on the host (the merged ranges, the layout's runs, a lookup a row), about
 * 15 ns a run - supposed from the shapes, not measured apart.  What it saves is the memory and the upload: 536 MB of listed chunks on
 * the device where the arena call needs the 1 GiB file.  Not timed: the gather into the packed buffer, files past 1 GiB. */
int32_t b3w_bao_set_slice_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens,
                                        uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files,
                                        const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, uint8_t *d_slices,
                                        void *stream);

/* ---- slices taken into packed chunk slots: the receiver's side for files that are not resident (still ABI 1.4: new names only) ---
 * The three receivers above write a chunk at d_arena + host_offsets[f] + 1024 c, so a node that fetches the missing half of a 1 GiB file
 * holds the whole GiB on the device to take in 537 MB, and a client that only wants verified bytes (bao's decode) has no device route.
 * These calls take their arena twin's arguments with a SLOT BUFFER (d_chunks, chunks_bytes) in place of (d_arena, arena_bytes,
 * host_offsets): one slot of 1 024 bytes per listed chunk, in the order of the per-chunk statuses.
 * SEMANTICS, BY PROJECTION.  Every status - per chunk / sample, per range / set, first bad - is what the arena twin reports for the
 * same slices, roots, list and group_log.  A chunk of status 0 gets its min(1024, len - 1024 c) bytes at d_chunks + 1024 slot; the
 * rest of a short last chunk's slot is not written; a chunk of any other status has its whole slot left alone: nothing unverified is
 * written.  The slot of a chunk:
 *   one-chunk slices   slot = i, the sample's index (repeated samples each have their own slot);
 *   range slices       slot = chunk_first[r] + (c - first[r]), chunk_first the running sum of the counts (the index of
 *                      b3w_sample_plan_range_slices_device's d_chunk_status; overlapping ranges each list their own slots);
 *   set slices         slot = set_chunk_first[s] + rank_S(c): d_chunk_status's index, the device form of b3w_bao_set_slice_decode's
 *                      out_bytes.
 * d_outboards != NULL: the header and the stored nodes of every verified chunk's path at this group_log go to their pre-order places,
 * byte for byte what the arena twin writes, and every other byte stays.  d_outboards == NULL: nothing but slots, statuses and the
 * optional bitmap is written - DECODE on the device.  d_have (may be NULL in all three) gets the arena calls' bits.
 * The same launches as the twins (1, <= 3, <= 3), the same table through the context's staging, the same scratch size calls; nothing
 * is allocated; asynchronous on `stream`.  d_chunks, d_outboards and d_slices must not overlap (not checked).  REFUSALS ARE ATOMIC
 * (B3W_E_BAD_ARGUMENT before anything is launched or written; b3w_last_error says what was wrong): what the twin refuses without the
 * arena items and without the null d_outboards, a null d_chunks with a list that is not empty, a d_chunks that is not 16-byte
 * aligned, chunks_bytes < 1024 x the listed chunks (the message says how many bytes are needed).  An empty list is a no-op.
 * WHEN NOT TO (MI355X, one 1 GiB file; the yardstick is the parent commit's arena receiver over the same slices into a
 * resident arena, the slots compared with the arena's chunks one by one before timing; device events round whole calls, alternating
 * medians; no profiler run): the packed calls read and write the same bytes as
 * their twins and their stores are denser, and they land at or just below them - the 262 507 runs of a half-missing bitmap as set slices
 * 3.34 ms against 3.41 (the yardstick's spread 0.001), 65 536 runs of ONE chunk 1.457 against 1.515 as one-chunk slices (0.0004) and 1.242
 * against 1.261 as set slices (0.0008), 4 096 runs of 16 as range slices 0.395 against 0.400 (0.0009).  LONG RUNS GAIN NOTHING AND LOSE A
 * HAIR: 64 runs of 1 024 chunks as range slices 0.2120 against 0.2113, 0.3 % and more than the spread of 0.00002 (cause not found: the
 * kernels take the same registers as their twins - 66 to 73 VGPRs the one-chunk kernel, 53 / 54 the range kernels, 76 / 60 the set kernels -
 * and the host does the same work); at group_log 4 0.1984 against 0.1985, inside the spread of 0.00004.  With d_outboards null the same
 * calls take 3.21, 1.415, 1.123, 0.357 and 0.176 ms.  What the calls save is the memory: 536 MB of slots where the arena receiver needs
 * the 1 GiB file resident for the half-missing shape (538 MB less), 67 MB against 1 GiB for 65 536 chunks.  So: a file that IS resident
 * keeps the arena calls (the chunks are then where every other call reads them); the choice between the three slice kinds is the arena
 * calls' (set slices for many short runs, range slices for a few long ones).  Not measured: the copy of the slots to the host and
 * bao.scatter_chunks, files past 1 GiB, many files a call, the kernels one by one.  Not tested on the device: slots past 2^32 bytes
 * (the slot arithmetic is 64 bits wide; tools/bao_receive_packed_host_check.cpp holds the host side of it). */
int32_t b3w_bao_slice_ingest_packed_device(b3w_ctx *ctx, uint8_t *d_chunks, uint64_t chunks_bytes, const uint64_t *host_lens, uint32_t n_files,
                                           uint32_t group_log, uint8_t *d_outboards /* may be NULL */, const uint32_t *d_roots,
                                           const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices,
                                           int32_t *d_sample_status, uint64_t *d_have /* may be NULL */, void *stream);
int32_t b3w_bao_range_slice_ingest_packed_device(b3w_ctx *ctx, uint8_t *d_chunks, uint64_t chunks_bytes, const uint64_t *host_lens, uint32_t n_files,
                                                 uint32_t group_log, uint8_t *d_outboards /* may be NULL */, const uint32_t *d_roots,
                                                 const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count,
                                                 uint32_t n_ranges, const uint8_t *d_slices, int32_t *d_range_status,
                                                 uint64_t *d_range_first_bad, uint64_t *d_have /* may be NULL */, void *d_scratch,
                                                 uint64_t scratch_bytes, void *stream);
int32_t b3w_bao_set_slice_ingest_packed_device(b3w_ctx *ctx, uint8_t *d_chunks, uint64_t chunks_bytes, const uint64_t *host_lens, uint32_t n_files,
                                               uint32_t group_log, uint8_t *d_outboards /* may be NULL */, const uint32_t *d_roots,
                                               const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count,
                                               uint32_t n_ranges, const uint8_t *d_slices, int32_t *d_set_status, uint64_t *d_set_first_bad,
                                               int32_t *d_chunk_status /* may be NULL */, uint64_t *d_have /* may be NULL */, void *d_scratch,
                                               uint64_t scratch_bytes, void *stream);

/* ---- set slices in windows: ONE set's slice taken in as it arrives (still ABI 1.4: new names only) ------------------------------------
 * The two set receivers above need the whole slice on the device before they verify a byte: the missing half of a 1 GiB file is one
 * slice of 593 MB.  A SESSION takes the slice of one set (one file) in WINDOWS cut at row boundaries, in slice order, and its outputs
 * are byte for byte those of the one-shot receiver over the whole slice.
 * DEFINITIONS.  The set is the set calls' list for one file: ascending, disjoint, touching runs allowed.  Its ROWS and their kind (64 or
 * 1 024 chunks) are b3w_bao_set_slice_ingest_device's.  Every element of the slice - a parent node or a chunk - has c0, the least wanted
 * chunk under it; the slice is pre-order, so c0 never falls along it and the rows cut it into consecutive SEGMENTS: cut[r] is the offset
 * of the first element whose c0 lies in row r's block, cut[0] = 0 (the header rides with row 0), cut[n_rows] the slice's size.  For
 * r > 0, cut[r] is the end of the last wanted chunk in front of the block.  A WINDOW is slice bytes [cut[i], cut[j]), i < j, and a
 * session's next window starts where the last one ended.  A segment is never longer than B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW = 8 + 64 x
 * (24 + 1 023) + 1 048 576 bytes.  Slices start at 8 modulo 16 in the one-shot layout, so every cut but 0 is 16-byte aligned there:
 * a window's first byte must lie at 8 modulo 16 for cut 0 and at 0 modulo 16 for any other cut.
 * WHAT IS CARRIED from window to window is the header and, a depth t < 24, the last node of that depth above a block seen so far: 16 +
 * 64 x 24 bytes at the front of the scratch.  The ancestor at depth t of any later row is that node (DESIGN.md 8g has the proof).
 * NOTHING CARRIED IS TRUSTED: a row hashes its carried nodes against the root exactly as it hashes slice nodes, so the statuses are the
 * one-shot call's by construction.  The carry is written by the push's last launch, after the window's rows have read it: PUSHES ARE A
 * SERIAL DEPENDENCY, and the caller orders each push behind the previous one (the same stream, or events). */
#define B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW 1115592ull
#define B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES 1552ull
#define B3W_BAO_SET_STREAM_ARENA  0 /* d_dest is the file's place in an arena: chunk c at d_dest + 1024 c, any byte alignment */
#define B3W_BAO_SET_STREAM_PACKED 1 /* d_dest is a slot buffer: the wanted chunk of rank k at d_dest + 1024 k, 16-byte aligned */
typedef struct b3w_bao_set_stream b3w_bao_set_stream;
/* Host only.  The windows of at most max_window_bytes, filled greedily with as many whole rows as fit: their ascending cut offsets,
 * windows + 1 values from 0 to the slice's size, into cuts_out when cap >= windows + 1 (nothing is written otherwise).  Returns the
 * number of windows either way; -B3W_E_BAD_ARGUMENT for a list the set calls refuse, no run, a file of more than 2^30 chunks or
 * max_window_bytes < B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW.  O(rows + runs), O(depth) a run on the file's ragged right edge; no step a
 * chunk. */
int64_t b3w_bao_set_slice_stream_cuts(uint64_t preimage_len, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges,
                                      uint64_t max_window_bytes, uint64_t *cuts_out, uint64_t cap);
/* Host only.  The session's scratch: B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES, then 16 bytes a row of the window with the most rows among
 * all windows of at most max_window_bytes, wherever they start.  0 where the cuts call refuses. */
uint64_t b3w_bao_set_slice_stream_scratch_bytes(uint64_t preimage_len, const uint64_t *host_first, const uint64_t *host_count,
                                                uint32_t n_ranges, uint64_t max_window_bytes);
/* Begins a session.  dest_kind B3W_BAO_SET_STREAM_ARENA: (d_dest, dest_bytes) is the file's place in an arena and d_outboard its
 * outboard at this group_log, with the meanings, alignments and nullabilities of b3w_bao_set_slice_ingest_device for one file at
 * offset 0.  B3W_BAO_SET_STREAM_PACKED: (d_dest, dest_bytes) is b3w_bao_set_slice_ingest_packed_device's slot buffer and d_outboard may
 * be NULL (decode only).  d_root: the file's 8 root words.  d_have, d_chunk_status may be NULL; d_have is the file's bitmap.  The row
 * table is built here, once, on the host (344 or 224 bytes a row) and the context's staging ring is grown to the largest window the
 * scratch allows; d_set_status and d_set_first_bad are set to 0 and UINT64_MAX ("none") on `stream`.  Refused, atomically (nothing
 * launched or written, *out_session NULL): what the one-shot call of that kind refuses, no run, an unknown kind, a scratch smaller than
 * B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES + 16, null or not 16-byte aligned. */
int32_t b3w_bao_set_slice_stream_begin(b3w_ctx *ctx, uint64_t preimage_len, uint32_t group_log, const uint64_t *host_first,
                                       const uint64_t *host_count, uint32_t n_ranges, const uint32_t *d_root, uint32_t dest_kind,
                                       uint8_t *d_dest, uint64_t dest_bytes, uint8_t *d_outboard, uint64_t *d_have /* may be NULL */,
                                       int32_t *d_chunk_status /* may be NULL */, int32_t *d_set_status, uint64_t *d_set_first_bad,
                                       void *d_scratch, uint64_t scratch_bytes, void *stream, b3w_bao_set_stream **out_session);
/* Takes in the window of `bytes` bytes at d_window, slice bytes [offset, offset + bytes): verifies its rows, writes their chunks, nodes,
 * bitmap bits and per-chunk statuses as the one-shot call does, folds the rows' results into d_set_status (the largest) and
 * d_set_first_bad (the least) - a bad window is known when its push is done - and carries the header and the nodes later rows need.  At
 * most THREE launches (in fact two: a set's rows are of one kind; then the fold, which also writes the carry); only this window's rows
 * go up, through a slot of the context's staging ring of eight.  TWO LIMITS: begin grows the slots that are free at that moment, so a
 * push that lands on a slot which was in flight then and is still too small frees and allocates it (hipHostMalloc / hipMalloc, which
 * wait for the device) - otherwise a push allocates nothing; and the host waits for nothing only while fewer than eight uploads of
 * this context are in flight: with every slot busy a push waits for the oldest (a session of many small windows does).  No byte
 * outside the window is read but the carry.  REFUSALS ARE ATOMIC and each names its reason: a finished
 * session or one whose slice is all pushed, a null window or no bytes, an offset that is not where the last window ended (out of
 * order), an end that is not on a cut, a first byte that is not at 8 (offset 0) or 0 modulo 16, more rows than the scratch holds.
 * Nothing is launched or written and the session stays usable.
 * WHEN NOT TO (MI355X, one 1 GiB file with half its chunks missing, 262 507 runs, 593 MB of slice in 1 024 rows; the
 * yardstick is a build of the parent commit's b3w_bao_set_slice_ingest_device loaded beside this library, over the same RESIDENT slice;
 * device events round whole calls - a whole session: begin, every push, finish, free -, the routes alternating, medians, every output
 * compared byte for byte before timing; no profiler run): A SLICE THAT IS ALREADY RESIDENT.  The one-shot call takes 3.39 ms (spread
 * 0.01).  A session costs begin - the one-shot call's host work, 2.8 ms with these runs - and then 0.17 ms a push (0.21 at 64 MiB) whatever the
 * window holds, because a push waits for the one before it and a window of a few rows leaves most of the device idle: 9 windows of
 * 64 MiB 4.66 ms (1.37 times the one-shot call), 74 of 8 MiB 15.8 ms (4.7 times), 986 of the least window 171.6 ms (50 times).  What
 * a session buys is the memory and the first verdict: two windows of 64 MiB are 134 MB on the device where the one-shot call holds
 * 593 MB, two of the least one 2.2 MB; and a tampered header is reported 2.95 ms after begin (begin and the first push) where the
 * one-shot call reports it 3.1 ms after the LAST byte has arrived.  So: windows as large as memory allows, never the least one for
 * throughput.  Not measured: the arrival itself (the copies that a session overlaps and the one-shot call must wait for), the packed
 * destination, files past 1 GiB, the kernels one by one. */
int32_t b3w_bao_set_slice_stream_push(b3w_bao_set_stream *session, uint64_t offset, const uint8_t *d_window, uint64_t bytes, void *stream);
/* Host only; no launch.  Refuses a session whose slice was not pushed to its end (or that is finished); afterwards every push is
 * refused.  The outputs are final when the last push is done. */
int32_t b3w_bao_set_slice_stream_finish(b3w_bao_set_stream *session);
/* Frees the host object (a session owns no device memory and no event); safe during an open graph capture.  NULL is a no-op. */
void b3w_bao_set_slice_stream_free(b3w_bao_set_stream *session);

/* ---- updates in place after writes to resident files (still ABI 1.4: new names only) --------------------------------
 * Every call above treats a file as immutable: after one rewritten block the only way to a correct outboard and root is the batch
 * call over the whole file again.  These calls make the cost follow the bytes written.  GIVEN an arena with its offsets and
 * lengths, the packed outboards and roots of those files as they were BEFORE some bytes changed, and a list of dirty ranges
 * (host_files[i], host_first_chunk[i], host_n_chunks[i]) that covers every changed byte, d_outboards and d_roots are afterwards byte
 * for byte what b3w_bao_outboard_batch_device (group_log = 0) / b3w_bao_group_outboard_batch_device (1 .. B3W_BAO_MAX_GROUP_LOG) write
 * for the arena as it is now.  LENGTHS DO NOT CHANGE: an append or a truncation moves every node of a pre-order outboard and is
 * b3w_bao_outboard_resize_batch_device's business ("resident files after appends and truncations" below).
 * A stored node is left CV || right CV, so the CV of every clean sibling on a dirty chunk's path is in the outboard already: only
 * dirty chunks are hashed from bytes.  A UNIT is a chunk (group_log = 0) or a group of 2^group_log chunks; a unit with a dirty chunk
 * is hashed whole.
 *   NOTHING EXTRA IS WRITTEN.  The only nodes written are those with a dirty unit below them, and of those only the halves over a
 *     dirty unit.  Of a file of more than 64 chunks no header is written and no byte outside its dirty units is read.  A dirty file of
 *     at most 64 chunks is rehashed whole (at most 64 KiB; header, nodes and root rewritten with the same values where nothing
 *     changed).  No byte of a file without a dirty range is read or written.
 *   AN INCOMPLETE LIST IS NOT DETECTED.  If the list misses a changed chunk the call cannot know: the result is an outboard that
 *     b3w_bao_verify_batch_device reports with status 1 at exactly that unit (where the unit's file has more than 64 chunks and no
 *     listed chunk shares the unit).
 *   Ranges may be unsorted, overlapping or duplicated: the host sorts and merges them.  A range of 0 chunks is dropped.
 *   n_ranges == 0: B3W_OK, nothing launched.
 * WHEN TO CALL THE BATCH CALL INSTEAD (measured on an MI355X): the cost follows the DIRTY TILES of 1 024 chunks and the
 * number of ranges, not the dirty chunks; a tile with one dirty chunk costs about what the batch call spends on a whole tile.  One
 * 4 KiB write into a 1 GiB file: 0.09 ms against the batch call's 0.42; 1 024 scattered writes (0.4 % of the chunks): 0.22 ms; 4 096
 * (1.6 %, a write in every tile): 0.42 ms, the batch call's time; more: slower than the batch call, up to 1.4 times with every chunk
 * dirty in few ranges and several times with hundreds of thousands of ranges (about 17 ns of host work a range).  So: this call while
 * fewer than about one tile in two holds a write, or while the dirty files are a small part of a batch of small files (4 096 of
 * 262 144 files of 4 KiB: 0.11 ms against 1.10); the batch call otherwise. */
/* Host only.  Bytes of caller's scratch b3w_bao_outboard_update_batch_device needs for these ranges: 32 per dirty tile of 1 024
 * chunks of the files of more than one tile, plus 32 per dirty span of 1 024 tiles of the files past 1 GiB; files of one tile need
 * none.  host_lens is indexed by host_files[i] (which is not checked here).  0 for a null pointer or no range. */
uint64_t b3w_bao_update_scratch_bytes(const uint64_t *host_lens, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                      const uint64_t *host_n_chunks, uint32_t n_ranges);
/* host_ob_first: the files' outboard byte offsets as b3w_bao_batch_layout / b3w_bao_group_batch_layout return them — taken, not
 * recomputed, so that the call's host work and its table grow with the ranges and the dirty tiles and never with n_files.
 * d_roots: 8 u32 per file ON THE DEVICE.  d_scratch: 16-byte aligned, b3w_bao_update_scratch_bytes.
 * AT MOST FOUR LAUNCHES whatever the number of ranges, files or dirty tiles: the dirty files of at most 64 chunks through the batch
 * call's kernel for them; a workgroup per dirty tile of the larger files; one per span of 1 024 tiles that holds a dirty tile; one
 * more launch over the spans for files past 1 GiB.  One table (184 bytes per workgroup of the last three, 32 per small file) goes
 * through the staging ring of the many-calls above; nothing else is allocated, the host waits for nothing.
 * REFUSALS ARE ATOMIC: every range is checked first, and a refused call launches nothing and writes nothing (B3W_E_BAD_ARGUMENT,
 * b3w_last_error names the range): a null pointer (d_arena may be NULL where every dirty file is empty), group_log above the
 * maximum, a file index >= n_files, a range that reaches past its file's chunk count (an empty file has one chunk), a dirty file
 * that reaches past arena_bytes or has more than 2^30 chunks, d_outboards off 8 bytes, a small, null or misaligned scratch.
 * Any context.  Asynchronous on `stream`. */
int32_t b3w_bao_outboard_update_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                             const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                                             const uint64_t *host_ob_first, uint8_t *d_outboards, uint32_t *d_roots,
                                             const uint32_t *host_files, const uint64_t *host_first_chunk,
                                             const uint64_t *host_n_chunks, uint32_t n_ranges, void *d_scratch, uint64_t scratch_bytes,
                                             void *stream);
/* Host only, one file in host memory, for callers without a GPU: the same sparse walk.  `outboard` (full, or the group outboard of
 * group_log) and `root` (8 u32) are updated in place for the dirty ranges of `data` (len bytes): only the nodes with a dirty unit
 * below them are written, no byte outside the dirty units is read.  B3W_E_BAD_ARGUMENT, nothing written, for a null pointer, a
 * group_log above the maximum or a range that reaches past the chunk count. */
int32_t b3w_bao_outboard_update(const uint8_t *data, uint64_t len, uint8_t *outboard, uint32_t group_log,
                                const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges,
                                uint32_t *root /* 8 u32 */);

/* ---- verification of listed chunk ranges of resident files (still ABI 1.4: new names only) ----------------------------
 * b3w_bao_verify_batch_device reads every byte of every file.  These calls make the cost of CHECKING follow the bytes of interest, as
 * the update call does for writing: a provider that has served a 4 KiB read, a scrubber that takes a slice per pass, a repairer that
 * re-checks what it has rewritten.  GIVEN the arena, outboards and roots as the update call takes them and a list of ranges
 * (host_files[i], host_first_chunk[i], host_n_chunks[i]):
 *   d_unit_status (packed as b3w_bao_verify_layout says, one byte a unit): the byte of every unit that holds a listed chunk is
 *     afterwards the byte b3w_bao_verify_batch_device writes there for the same arena, outboards and roots — the same rules (3 header,
 *     2 a stored node on the path or the root, 1 the unit's bytes, 0), the first that applies.  NO OTHER BYTE OF THE BUFFER IS WRITTEN,
 *     so a scrubber can pass the same buffer to successive calls.  One exception: a listed file of at most 64 chunks is verified whole
 *     and ALL its unit bytes are written, with the whole-file call's values.
 *   d_range_status[i] (int32) and d_range_first_bad[i] (uint64, 8-byte aligned), in the order the ranges were given: the largest
 *     status among the units range i touches, and the lowest unit index WITHIN THE FILE with a non-zero status among them, or
 *     UINT64_MAX.  A range of 0 chunks gets 0 and UINT64_MAX.  None of the three outputs needs clearing.
 *   WHAT IS READ.  A unit with a listed chunk is hashed whole.  Of a file of more than 64 chunks no arena byte outside its listed units
 *     is read, the only stored nodes read are those with a listed unit below them (such a node is read whole), and the header is read
 *     by one workgroup.  No byte of a file without a range is read.  Nothing of the arena, the outboards or the roots is written.
 *   Ranges may be unsorted, overlapping or repeated: the host sorts and merges them for the walk.  n_ranges == 0: B3W_OK, nothing
 *     launched.
 * WHEN TO CALL b3w_bao_verify_batch_device INSTEAD (measured on an MI355X): a call that touches one tile is latency
 * from end to end.  One 4 KiB range of a 1 GiB file: 0.10 ms against the whole-file call's 0.43; 64 scattered 4 KiB ranges: 0.13;
 * 1 024: 0.23; 4 096 (a range in nearly every tile, 1.6 % of the chunks): 0.41, level with the whole-file call; EVERY chunk in one
 * range: 0.59, 1.36 times the whole-file call.  4 096 listed files of 262 144 of 4 KiB: 0.13 ms against 1.57.  So: this call while
 * the ranges leave tiles out or leave most chunks of the tiles they touch unlisted; the whole-file call when most of the file is
 * listed (where exactly the two cross between 1.6 % and 100 % was not measured). */
/* Host only.  Bytes of caller's scratch b3w_bao_verify_ranges_batch_device needs for these ranges: 36 (an expected CV and a word)
 * per listed tile of 1 024 chunks of the files of more than one tile, plus 36 per listed span of 1 024 tiles of the files past 1 GiB,
 * rounded up to 16; files of one tile (the files of at most 64 chunks among them) need none.  host_lens is indexed by host_files[i]
 * (which is not checked here).  0 for a null pointer or no range. */
uint64_t b3w_bao_verify_ranges_scratch_bytes(const uint64_t *host_lens, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                             const uint64_t *host_n_chunks, uint32_t n_ranges);
/* host_ob_first (b3w_bao_batch_layout / b3w_bao_group_batch_layout) and host_unit_first (b3w_bao_verify_layout) are taken, not
 * recomputed, and read at listed files only: the call's host work and its table grow with the ranges and the listed tiles and never
 * with n_files.  d_roots: 8 u32 per file ON THE DEVICE.  d_scratch: 16-byte aligned, b3w_bao_verify_ranges_scratch_bytes.
 * AT MOST FIVE LAUNCHES whatever the number of ranges, files or tiles: the listed files of at most 64 chunks; for files past 1 GiB a
 * workgroup per file over its listed spans; a workgroup per span of 1 024 tiles that holds a listed tile (these two read stored nodes
 * alone and leave, per listed tile, the CV it must have and whether the path above or the header is bad); a workgroup per listed
 * tile; a workgroup per range that reduces the status bytes just written.  One table (208 bytes per workgroup of the middle three, 24
 * per range, 48 per small file) goes through the staging ring of the many-calls above; nothing else is allocated, the host waits for
 * nothing.
 * REFUSALS ARE ATOMIC: every range is checked first, and a refused call launches nothing and writes nothing (B3W_E_BAD_ARGUMENT,
 * b3w_last_error names the range): the update call's list (a null pointer — d_arena may be NULL where every listed file is empty —
 * group_log above the maximum, a file index >= n_files, a range that reaches past its file's chunk count, a listed file that reaches
 * past arena_bytes or has more than 2^30 chunks, d_outboards or an outboard offset off 8 bytes, a small, null or misaligned scratch),
 * and a null output pointer, d_range_first_bad off 8 bytes or d_range_status off 4.  Any context.  Asynchronous on `stream`. */
int32_t b3w_bao_verify_ranges_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                           const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                                           const uint64_t *host_ob_first, const uint8_t *d_outboards, const uint32_t *d_roots,
                                           const uint32_t *host_files, const uint64_t *host_first_chunk,
                                           const uint64_t *host_n_chunks, uint32_t n_ranges, const uint64_t *host_unit_first,
                                           uint8_t *d_unit_status, int32_t *d_range_status, uint64_t *d_range_first_bad, void *d_scratch,
                                           uint64_t scratch_bytes, void *stream);
/* Host only, one file in host memory, for callers without a GPU: the same sparse walk.  unit_status (room for the file's
 * max(1, ceil(n_chunks / 2^group_log)) units) is written at the listed units only, whatever the file's size; range_status and
 * range_first_bad (n_ranges entries each) may be NULL.  Only the listed units' bytes and the nodes with a listed unit below them are
 * read; with no chunk listed nothing is read at all.  B3W_E_BAD_ARGUMENT, nothing written, for a null pointer, a group_log above
 * the maximum or a range that reaches past the chunk count. */
int32_t b3w_bao_verify_ranges(const uint8_t *data, uint64_t len, const uint8_t *outboard, uint32_t group_log, const uint32_t *root /* 8 u32 */,
                              const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges, uint8_t *unit_status,
                              int32_t *range_status, uint64_t *range_first_bad);

/* ---- sparse calls from packed chunk bytes: files that are NOT resident (still ABI 1.4: new names only) ------------------
 * The update call, the ranged verification and the range-slice provider read only the chunks their ranges list, yet they take the
 * arena: the whole file has to be in device memory for them to find those chunks at offset + 1024 c.  A provider whose file is on
 * disk (the streamed sessions above are for it) gathers the listed chunks alone into a PACKED buffer and calls the twins below.
 * THE LISTED CHUNKS of a call with (host_lens, group_log, ranges (file, first_chunk, n_chunks)):
 *   a file of at most 64 chunks with a range that is not empty lists ALL its chunks (the small kernels rehash and verify it whole);
 *   any other file lists every chunk of every unit of 2^group_log chunks that a range touches, clamped to the file
 * — the chunks the arena calls hash.  Every listed chunk takes one SLOT of 1 024 bytes: listed files in ascending index, within a
 * file its distinct listed chunks in ascending order, slots numbered from 0 across the call; a file's short last chunk fills the
 * front of its slot and the rest of that slot is never read.  Chunk c lies at d_packed + 1024 slot(c), and the chunks an input range
 * lists are consecutive slots whatever the order, overlap or repetition of the ranges. */
/* Host only.  The layout: the listed chunks of range i are the file's chunks [range_first[i], range_first[i] + range_chunks[i]), to
 * be copied to slot range_slot[i] onwards (ranges that share a chunk name the same slot for it); an empty range gets range_chunks[i]
 * = 0 (and slot and first 0).  The three arrays (n_ranges entries each) may be NULL.  *total_slots: the slots of the call;
 * *total_bytes: the end of the last byte any call reads, 1024 (total_slots - 1) + the bytes of the chunk in the last slot, 0 with
 * nothing listed.  B3W_E_BAD_ARGUMENT, nothing written, for what the sparse calls refuse: a null pointer (the totals; the inputs
 * where n_ranges > 0), group_log above the maximum, a file index >= n_files, a range that reaches past its file's chunk count, a
 * listed file of more than 2^30 chunks.  O(n_ranges log n_ranges); host_lens is read at listed files only. */
int32_t b3w_bao_packed_layout(const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint32_t *host_files,
                              const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges, uint64_t *range_slot,
                              uint64_t *range_first, uint64_t *range_chunks, uint64_t *total_slots, uint64_t *total_bytes);
/* The three twins: the arguments of b3w_bao_outboard_update_batch_device, b3w_bao_verify_ranges_batch_device and
 * b3w_bao_range_slice_arena_device with (d_packed, packed_bytes) for (d_arena, arena_bytes, host_offsets).  d_packed holds the listed
 * chunks of THIS call's ranges and group_log as b3w_bao_packed_layout places them, at any byte alignment (16-byte aligned it is read
 * in 16-byte pieces, as an arena file at such an offset).  EVERY OUTPUT BYTE IS WHAT THE ARENA COUNTERPART WRITES for an arena that
 * holds the same file bytes, with the same outboards, roots, ranges and group_log, and every byte it leaves alone stays untouched:
 * outboard nodes, header, roots; unit statuses, range statuses, first bad units; slices.  The same launch bounds (four, five, two),
 * the same scratch (b3w_bao_update_scratch_bytes, b3w_bao_verify_ranges_scratch_bytes), the same table through the same staging;
 * nothing is allocated, the host waits for nothing.  The tile kernels are instantiations that address by rank: a row carries the
 * slot of its tile's first listed chunk, and lane t reads behind the listed chunks of the tile below t while its counter and its
 * length stay those of chunk 1 024 tile + t; the small-file launches, the storeys above the tiles and the reduction are the arena
 * calls' own kernels.  In a range slice the source of chunk c of range r is d_packed + 1024 (range_slot[r] + c - range_first[r]).
 * REFUSALS ARE ATOMIC and name the range: the arena calls' lists without the arena items (null arena, a file past arena_bytes), and
 * a null d_packed where total_bytes > 0, and packed_bytes < total_bytes (b3w_last_error gives the number needed).  No byte at or
 * behind total_bytes, and no byte of a slot behind a short last chunk, is read.
 * WHEN NOT TO (MI355X; device events round whole calls against the arena call of the same build): a file that IS
 * resident.  The arena calls read it in place, need no gather and no layout, and are the faster calls on every shape measured: one,
 * 64 ranges of 4 KiB or 64 runs of 1 024 chunks of a 1 GiB file 1 to 2 us behind; 4 096 ranges of 4 KiB 0.412 ms against 0.388 (update),
 * 0.422 against 0.400 (ranged verification), 0.431 against 0.262 (range slices: this call sorts the ranges, the arena call does not);
 * 4 096 listed files of 4 KiB 0.181 against 0.106, 0.199 against 0.127, 0.446 against 0.329.  The difference is the layout on the
 * host.  What the packed calls save is device memory and upload: total_bytes instead of the files. */
int32_t b3w_bao_outboard_update_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens,
                                              uint32_t n_files, uint32_t group_log, const uint64_t *host_ob_first, uint8_t *d_outboards,
                                              uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                              const uint64_t *host_n_chunks, uint32_t n_ranges, void *d_scratch, uint64_t scratch_bytes,
                                              void *stream);
int32_t b3w_bao_verify_ranges_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens,
                                            uint32_t n_files, uint32_t group_log, const uint64_t *host_ob_first, const uint8_t *d_outboards,
                                            const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                            const uint64_t *host_n_chunks, uint32_t n_ranges, const uint64_t *host_unit_first,
                                            uint8_t *d_unit_status, int32_t *d_range_status, uint64_t *d_range_first_bad, void *d_scratch,
                                            uint64_t scratch_bytes, void *stream);
int32_t b3w_bao_range_slice_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens,
                                          uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files,
                                          const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, uint8_t *d_slices,
                                          void *stream);

/* ---- resident files after appends and truncations (still ABI 1.4: new names only) -------------------------------------
 * The update call above follows writes that keep a file's length.  These calls follow a CHANGE of length.  In a pre-order outboard
 * the PLACE of every node can move when the length changes; the VALUES below a tile of 1 024 chunks that is full before and after
 * do not ("open-length sessions" above): such a tile's (1 024 >> group_log) - 1 stored nodes are one contiguous block whose start
 * alone depends on the length, and its chaining value is the parent compression of the block's first node.  GIVEN the arena with a
 * file's bytes at its NEW length (the first min(old, new) bytes what they were) and its outboard for the OLD length as the batch
 * calls made it, the file's outboard at its new place and its root are afterwards byte for byte what
 * b3w_bao_outboard_batch_device (group_log = 0) / b3w_bao_group_outboard_batch_device write for the arena as it is now with the new
 * lengths: header, every node.  With T = b3w_bao_resize_kept_tiles(old, new):
 *   the blocks of tiles 0 .. T - 1 are MOVED from the old outboard to the new one and their CVs taken from their first nodes;
 *   the tiles from T on are hashed from the arena; the one or two merge storeys above the tile CVs are run again.
 *   NOTHING EXTRA IS READ OR WRITTEN.  No arena byte of a listed file below T MiB is read (a truncation to a whole number of MiB reads
 *     no arena byte at all; a file that ends up exactly one full tile gets its root from the block's first node).  d_old_outboards is
 *     never written.  Of d_new_outboards only the listed files' b3w_bao_group_outboard_size(new_len, group_log) bytes are written, of
 *     d_roots only the listed files' rows.  Nothing of an unlisted file is read or written.
 *   host_files[0 .. n_resized): the files whose length changed, each at most once.  An equal length is allowed and gives the same
 *     bytes at the new place.  n_resized == 0: B3W_OK, nothing launched.
 *   The old and the new outboard of a file are different extents (no resizing within one buffer).
 * WHEN TO CALL THE BATCH CALL INSTEAD (measured on an MI355X): only the kept tiles are a gain.  4 KiB appended to (or
 * cut from) a 1 GiB file: 0.17 ms against the batch call's 0.42 (0.16 at group_log = 4), the same for 1 MiB and for 64 MiB appended:
 * a call that hashes a tile costs that one workgroup's latency, the move of 64 MiB of outboard about 0.02 ms.  512 MiB grown to
 * 1 GiB: 0.27 against 0.42; 1 GiB cut to 512 MiB (nothing hashed): 0.05 against 0.25.  Files below 1 MiB at either length keep no
 * tile and are hashed whole through a kernel that is slower than the batch call's: 16 384 files growing from 64 to 68 KiB take 1.63
 * ms against 1.43.  So: this call where the listed files keep whole MiB tiles, the batch call for files below 1 MiB. */
/* Host only.  floor(min(old_len, new_len) / 1 MiB): the tiles whose nodes are moved, not recomputed. */
uint64_t b3w_bao_resize_kept_tiles(uint64_t old_len, uint64_t new_len);
/* Host only.  Bytes of caller's scratch for the listed files at their NEW lengths: 32 per tile (a last partial tile counts) of every
 * listed file of more than one tile, plus 32 per 1 024 tiles (rounded up) of those past 1 GiB; a file listed twice counts twice.
 * host_new_lens is indexed by host_files[i] (which is not checked here).  0 for a null pointer or n_resized == 0. */
uint64_t b3w_bao_resize_scratch_bytes(const uint64_t *host_new_lens, const uint32_t *host_files, uint32_t n_resized);
/* File f is bytes [host_offsets[f], + host_new_lens[f]) of d_arena (any byte alignment); d_old_outboards + host_old_ob_first[f] holds
 * its outboard for host_old_lens[f]; d_new_outboards + host_new_ob_first[f] receives the one for host_new_lens[f]; d_roots: 8 u32 per
 * file ON THE DEVICE.  The ob_first arrays are taken, not recomputed, and only [f] of listed files is read: they need not be the packed
 * layouts of b3w_bao_batch_layout, any 8-byte-aligned places will do, and the call's host work and its table grow with n_resized and
 * never with n_files.  Blocks move in 16-byte pieces where the old and the new place are both 16-byte aligned and in 8-byte pieces
 * otherwise; the bytes are the same.  d_scratch: 16-byte aligned, b3w_bao_resize_scratch_bytes.
 * AT MOST FIVE LAUNCHES whatever n_resized and the lengths: the listed files of at most 64 chunks (new length) through the batch
 * call's kernel for them; the relocation of all kept blocks with the headers, the kept tiles' CVs and the one-tile roots; the tiles
 * from T on of the larger files; the first merge storey; the second, for files past 1 GiB.  One table (at most 328 bytes a listed
 * file) goes through the staging ring of the many-calls above; nothing else is allocated, the host waits for nothing.
 * REFUSALS ARE ATOMIC: every entry is checked first, and a refused call launches nothing and writes nothing (B3W_E_BAD_ARGUMENT,
 * b3w_last_error names the entry): a null pointer (d_arena may be NULL where no listed file needs a byte read), group_log above the
 * maximum, a file index >= n_files, a file listed twice, a listed file that reaches past arena_bytes at its new length or has more
 * than 2^30 chunks at either length, an outboard place off 8 bytes, a listed file whose own old and new outboard extents overlap
 * (addresses are compared; overlaps between different files' extents are the caller's business), a small, null or misaligned
 * scratch, more than 2^31 - 1 workgroups in a grid.  Any context.  Asynchronous on `stream`. */
int32_t b3w_bao_outboard_resize_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                             const uint64_t *host_old_lens, const uint64_t *host_new_lens, uint32_t n_files,
                                             uint32_t group_log, const uint64_t *host_old_ob_first, const uint8_t *d_old_outboards,
                                             const uint64_t *host_new_ob_first, uint8_t *d_new_outboards, uint32_t *d_roots,
                                             const uint32_t *host_files, uint32_t n_resized, void *d_scratch, uint64_t scratch_bytes,
                                             void *stream);
/* Host only, one file in host memory: the same walk (old blocks copied, the rest hashed with blake3_cv).  `data` is the file at its
 * new length (no byte below T MiB is read; NULL where none is needed), old_outboard its outboard for old_len; new_outboard receives
 * b3w_bao_group_outboard_size(new_len, group_log) bytes.  B3W_E_BAD_ARGUMENT, nothing written, for a null pointer, a group_log above
 * the maximum, more than 2^30 chunks at either length or outboards that overlap. */
int32_t b3w_bao_outboard_resize(const uint8_t *data, uint64_t new_len, const uint8_t *old_outboard, uint64_t old_len,
                                uint32_t group_log, uint8_t *new_outboard, uint32_t *root /* 8 u32 */);

#ifdef __cplusplus
}
#endif
#endif /* B3WIT_H */
