/*
 * pirgpu.h -- C ABI of the MI355X-native PIR server query path (libpirgpu.so).
 *
 * The reference (OpenMined/PIR) has no FFI seam: its boundary is the C++ class
 * API of PIRServer / PIRDatabase over Microsoft SEAL objects.  Every entry
 * point below replaces one reference interface, cited as file:line relative to
 * /root/reference.  The host-side C++ mirror of the reference classes
 * (pir_amd/csrc/pir_facade.h) and the ctypes binding (pir_amd/capi.py) are thin
 * wrappers over exactly these symbols; INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every host buffer, the
 *     library owns all device memory;
 *   - residue arrays use SEAL's in-memory layout (reference server.cpp:98,
 *     ct_reencoder.cpp:61):
 *        ciphertext   uint64_t[2][k][N]       (poly, residue, coefficient)
 *        Galois key   uint64_t[k][2][k+1][N]  (digit, component, key-level residue), NTT form
 *   - every function returns 0 on success or the numeric absl::StatusCode the
 *     reference would have returned (3 InvalidArgument, 9 FailedPrecondition,
 *     12 Unimplemented, 13 Internal); pirgpu_last_error() gives the message;
 *   - one context drives one GPU; every entry point takes the context's lock
 *     for its own duration, and pirgpu_process_request(s) holds it while a window of
 *     requests is served (key lookup / installation + every query); requests that
 *     arrive meanwhile are queued and served together afterwards.  Sequences the
 *     CALLER composes out of several calls (set keys + query, stage / run / fetch)
 *     are only atomic if the caller serialises them itself;
 *   - every result is a canonical residue in [0, q_j) and is bit-identical to
 *     the reference's SEAL CPU path on the same inputs.
 */
#ifndef PIRGPU_H_
#define PIRGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIRGPU_MAX_PRIMES 8
#define PIRGPU_MAX_DIMS 8

#define PIRGPU_OK 0
#define PIRGPU_INVALID_ARGUMENT 3
#define PIRGPU_FAILED_PRECONDITION 9
#define PIRGPU_UNIMPLEMENTED 12
#define PIRGPU_INTERNAL 13

typedef struct pirgpu_ctx pirgpu_ctx;

/* What PIRContext + PIRParameters carry (reference context.h:36-84,
 * pir/proto/payload.proto:45-69), flattened. */
typedef struct pirgpu_params {
  uint32_t poly_modulus_degree;            /* N: 2048, 4096, 8192, 16384 or 32768 (32768: integer NTTs; an explicit
                                              coefficient modulus of at most PIRGPU_MAX_PRIMES data primes) */
  uint32_t num_data_primes;                /* k: ciphertext level (first_context_data) */
  uint64_t coeff_modulus[PIRGPU_MAX_PRIMES]; /* q_0..q_{k-1} */
  uint64_t special_prime;                  /* key-switching prime p (last of SEAL's coeff_modulus) */
  uint64_t plain_modulus;                  /* t */
  uint32_t num_dimensions;                 /* d */
  uint32_t dimensions[PIRGPU_MAX_DIMS];    /* PIRParameters.dimensions */
  uint64_t num_pt;                         /* PIRParameters.num_pt */
  uint64_t num_items;                      /* PIRParameters.num_items (0 if coefficient-loaded) */
  uint32_t bytes_per_item;                 /* PIRParameters.bytes_per_item */
  uint32_t items_per_plaintext;            /* PIRParameters.items_per_plaintext */
  uint32_t bits_per_coeff;                 /* PIRParameters.bits_per_coeff (0 = floor(log2 t)) */
  uint32_t use_ciphertext_multiplication;  /* 0, or 1 together with PIRGPU_CREATE_CT_MULTIPLY (pirgpu_create_ex); 1 at
                                              plain pirgpu_create is Unimplemented */
  int32_t device;                          /* HIP device ordinal */
  /* Row sharding for multi-GPU (not in the reference): this context holds the
   * top-level indices [shard_begin, shard_end) of dimension 0 and produces the
   * partial reply for them; 0,0 = the whole database (an empty shard is any begin == end != 0,
   * e.g. dimensions[0],dimensions[0]; its partial reply is all zero). */
  uint32_t shard_begin;
  uint32_t shard_end;
  /* Slot sharding for multi-GPU (not in the reference; d = 2): this context holds the NTT slots
   * [slot_begin, slot_end) -- multiples of 16 out of the ring's k * N, device order -- of EVERY plaintext and serves the
   * pirgpu_slots_* step only; 0,0 = all slots.  (The base case of PIRDatabase::multiply, reference database.cpp:185-194,
   * is a dyadic product in NTT form: independent per slot.)
   * Memory: AFTER pirgpu_db_finalize(ctx, 1) such a context holds (slot_end - slot_begin) / (k N) of the packed database.
   * WHILE it is being loaded, a context made by pirgpu_create holds the full u64 staging copy of every plaintext as well
   * (every rank encodes and transforms the whole database, then packs its own slots out of it): the whole database at
   * 8 bytes per residue + its share of the operand layout.  A STREAMED context (pirgpu_create_ex with
   * PIRGPU_CREATE_STREAMED_DB) encodes and packs in row bands and never has the staging copy: the per-rank load-time peak
   * is the rank's share of the operand layout plus one load chunk (option DB_STREAM_MB of encoded plaintexts + their raw
   * bytes), so slot shards hold a database larger than one GPU's memory. */
  uint32_t slot_begin;
  uint32_t slot_end;
  /* Wide items (not in the reference, whose CreatePIRParameters refuses an item larger than one plaintext,
   * parameters.cpp:81-85): an item of up to plaintexts_per_item x B bytes, B = N * bits_per_coeff / 8 rounded down, is
   * stored as `planes` = plaintexts_per_item plaintexts, plane j holding bytes [j B, min((j + 1) B, bytes_per_item)) of
   * it.  Every plane is a database of num_pt plaintexts with these dimensions; one query is expanded once and answered
   * on all planes: the reply is planes x (the usual count) ciphertexts, plane-major, plane j's part being bit-identical
   * to the reference's answer on plane j alone.  0 and 1 both mean 1 (the reference's behaviour).  planes > 1 needs
   * items_per_plaintext == 1 and (planes - 1) B < bytes_per_item <= planes B, and serves one GPU only (no row or slot
   * shard).  Plaintext indices at this ABI are plane-major then: plane * num_pt + pt (pirgpu_db_load_coeffs,
   * pirgpu_db_read_plaintext, pirgpu_db_update_plaintexts; pirgpu_db_size and pirgpu_zero_plaintexts count all planes).
   * With PIRGPU_CREATE_CT_MULTIPLY (below) the usual count is 1: the reply is `planes` ciphertexts, plane j's being
   * bit-identical to that mode's reply on plane j alone. */
  uint32_t plaintexts_per_item;
  /* Modulus-switched results (not in the reference, which answers at the full data modulus): with 1 <= result_primes =
   * r < k every level result of PIRDatabase::multiply -- the row sums after the scan, every upper level's output, the
   * reply -- is switched from q_0..q_{k-1} down to q_0..q_{r-1} right after its inverse transform (database.cpp:250-254)
   * and before CiphertextReencoder::Encode reads it: k - r drop steps, last prime first, each the exact
   * floor((x + floor(q_m / 2)) / q_m) on the CRT representative (the project's reading of SEAL 3.5.6
   * Evaluator::mod_switch_to_next_inplace for BFV; not verified against a SEAL build).  Encode then enumerates
   * (poly, j < r, digit): pirgpu_expansion_ratio is the sum of the first r local ratios, the reply holds
   * planes x (2 x that)^(d-1) ciphertexts of [2][r][N] words each (pirgpu_reply_ct_words), and on the wire a reply
   * ciphertext is a SEAL ciphertext at that level of the chain (r residues, parms_id(N, q_0..q_{r-1}, t)).  Queries,
   * keys, database, expansion and scan stay at k primes.  0 = off (the reference's behaviour, every byte as before);
   * r >= k is InvalidArgument.  Switching does not commute with the sum over shards: r >= 1 with a row or slot shard is
   * InvalidArgument, and the multi-GPU entry points (packed exchange, pirgpu_slots_*, pirgpu_reduce_fixup*, the device
   * reply copies) return FailedPrecondition on such a context.  Capacities given in ciphertexts stay in ciphertexts. */
  uint32_t result_primes;
  /* Tables (not in the reference, whose PIRDatabase is one database): the context holds `tables` = T databases of exactly
   * these parameters -- num_items, num_pt, dimensions and item size describe ONE of them -- and every query names, in the
   * clear, the table it is answered from (pirgpu_query_use_table, pirgpu_batch_set_tables, pirgpu_process_request_table /
   * _requests_tables).  Expansion, key sets, the batch pipeline and the workspace are shared; the scan reads the named
   * table only; the reply is bit-identical to the reference's processQuery on the database made of that table's items
   * alone (same ciphertext count, same words), and a query fails with Internal ("transparent") exactly when ITS table
   * holds an all-zero plaintext.  0 and 1 both mean one table (every byte, status and reply as without the field).
   * T > 1 is served by one GPU and from a staging copy: with a row shard, a slot shard, plaintexts_per_item > 1 or
   * PIRGPU_CREATE_STREAMED_DB it is InvalidArgument, and T x num_pt must stay below 2^32.  All ring degrees, arithmetic
   * flavours, d = 1, 2, 3, both scan families, key sets and result_primes work with it.  Indices at this ABI are
   * table-major then: plaintext table * num_pt + pt (pirgpu_db_load_coeffs, pirgpu_db_read_plaintext,
   * pirgpu_db_update_plaintexts), item table * num_items + i (pirgpu_db_update_items; pirgpu_db_load_items takes all
   * T x num_items items); pirgpu_db_size and pirgpu_zero_plaintexts count all tables, pirgpu_scan_bytes one table,
   * pirgpu_db_memory the whole allocation (table t's operand layout is the bytes [t, t + 1) x out[0] / T of it).
   * DESIGN.md section 6.5. */
  uint32_t tables;
} pirgpu_params;

/* PIRContext::Create + PIRDatabase::Create(params) (reference context.cpp:37-50,
 * database.cpp:40-44): validates the parameters, builds NTT tables on the device. */
int pirgpu_create(const pirgpu_params* params, pirgpu_ctx** out);
/* pirgpu_create with flags (0: exactly pirgpu_create; unknown bits: InvalidArgument).
 * PIRGPU_CREATE_STREAMED_DB: the u64 staging copy of the database is never allocated (not in the reference; DESIGN.md
 * section 6.3).  Loads encode chunks of whole row bands -- 16 rows of the scanned matrix, option "db_stream_mb"
 * (default 256) megabytes of encoded plaintexts per chunk, at least one band -- into a scratch and store them straight
 * into the operand layout of the int8-MFMA scan, which is allocated (zero-filled) when the context is first used; the
 * load-time peak is that layout plus one chunk instead of plus 8 bytes per residue of the whole database.  Afterwards the
 * context behaves like one that was populated and then given pirgpu_db_finalize(ctx, 1) -- queries, updates,
 * pirgpu_db_read_plaintext, the refusals of a slot shard -- except that it CAN be reloaded (a load overwrites), and
 * pirgpu_db_finalize succeeds and frees nothing.  d = 1 is InvalidArgument here (its scans read the staging copy); a
 * context whose int8-MFMA scan is off (fewer than 8 rows, a modulus of 2^55 or more, option scan_mfma = 0) is created,
 * but its first load returns FailedPrecondition before anything is allocated for the database. */
#define PIRGPU_CREATE_STREAMED_DB 1u
/* PIRGPU_CREATE_CT_MULTIPLY: the reference's ciphertext-multiplication mode (PIRParameters.use_ciphertext_multiplication,
 * database.cpp:196-212,238-254).  The upper levels multiply the lower level's results by the
 * selectors, ciphertext by ciphertext, and relinearise: every level result and the reply are ONE ciphertext
 * (pirgpu_reply_ct_count = 1 for every d, reply [2][k][N]) instead of (2 ExpansionRatio)^(d-1).  The product is the EXACT
 * BFV product -- x0 = a0 b0, x1 = a0 b1 + a1 b0, x2 = a1 b1 over Z[x]/(x^N + 1) on the centred lifts, d_i = floor((t x_i +
 * (Q - 1) / 2) / Q) -- the quantity SEAL's Evaluator::multiply (BEHZ) approximates: a valid BFV ciphertext the reference
 * client decrypts, NOT claimed bit-equal to a SEAL build; that is why the mode needs this flag beside the field.  The
 * flag needs use_ciphertext_multiplication = 1 (InvalidArgument otherwise); the field without the flag stays
 * Unimplemented.  Row sums (scan + inverse transform) and d = 1 are the existing path, bit for bit.  d >= 2 needs the
 * client's relinearisation key, installed as the key of Galois element 1 of the query's key set (pirgpu_set_galois_key /
 * pirgpu_keyset_set_key with galois_elt = 1; expansion never uses that element): a query without it is InvalidArgument
 * ("RelinKeys missing") -- the reference would go on with size-3 ciphertexts, this server does not.  Wide items
 * (plaintexts_per_item > 1) are served, both forms of the mode: one reply ciphertext per plane (pirgpu_reply_ct_count =
 * planes, plane-major), plane j's bit-identical to the mode's reply on the database made of chunk j of every item.  One
 * GPU: with a row or slot shard, result_primes, tables > 1, PIRGPU_CREATE_STREAMED_DB, N = 32768, more than 6 data
 * primes or a chain whose auxiliary base does not hold the product (pirgpu_ctmult_plan) the create is InvalidArgument,
 * and the multi-GPU entry points return FailedPrecondition on such a context.  Option "ct_scratch_mb" (default 256, before
 * first use) bounds the scratch the products of one worker / lane run in; "ct_blocks" is a counter: get returns the
 * product blocks the upper levels have queued so far, set overwrites the count (0 to start over).  Option "ct_shared_sel"
 * (before first use; default 1 on a context with wide items, 0 on every other): the selector pair of a product, the same
 * for every row and plane of a level, is lifted to the auxiliary base and transformed once per level and group of queries
 * instead of once per pair -- exact modular arithmetic either way, the reply bits do not depend on it.  Counter
 * "ct_lifts" (get / set like "ct_blocks"): the polynomials the upper levels have lifted to the auxiliary base so far --
 * 4 per pair, or with ct_shared_sel 2 per pair and 2 dimensions[l] per query, level and group.  The test hooks
 * pirgpu_ct_multiply and pirgpu_ct_multiply_sum count into it as well (see there). */
#define PIRGPU_CREATE_CT_MULTIPLY 4u   /* (bit 1 stays unassigned: flags 2 and 3 remain InvalidArgument) */
/* PIRGPU_CREATE_CT_DEFERRED: deferred rounding ("lazy relinearisation"), a second definition of the
 * upper levels of PIRGPU_CREATE_CT_MULTIPLY and valid only together with it (alone: InvalidArgument).  The tensor
 * products of a row's children are summed over the integers before the one rounding: X_m = sum_i x_m,i, D_m = floor((t X_m
 * + (Q - 1) / 2) / Q), row = relinearise(D) -- one scale and one key switch per row and query instead of one per child.
 * The reply is a valid ciphertext of the same item with the same noise budget to within a rounding, NOT the bits of the
 * per-child form.  A sum of n = max(dimensions[l], l < d - 1) products must fit the auxiliary base
 * (pirgpu_ctmult_plan_terms): InvalidArgument at create otherwise.  Everything PIRGPU_CREATE_CT_MULTIPLY refuses stays
 * refused; d = 1 and the row sums are unchanged.  Counter option "ct_relins" (get / set like "ct_blocks", both forms of
 * the mode): the ciphertexts the upper levels have key-switched so far -- pairs, or rows x queries here. */
#define PIRGPU_CREATE_CT_DEFERRED 8u
/* PIRGPU_CREATE_PACKED_REPLIES: replies leave the device at the bit width of their moduli instead of 64 bits a residue
 * (not in the reference).  For modulus q_j the width is w_j = bit length of q_j - 1; polynomial
 * (c, j) of a reply ciphertext [2][r][N] (r = result_primes or k) becomes a little-endian bit stream of N w_j bits -- bit b
 * of coefficient i is stream bit i w_j + b -- stored as N w_j / 64 little-endian words, and a packed ciphertext is its 2 r
 * polynomials in the order (c, j).  The reply BEFORE packing is bit for bit what the context produces without the flag;
 * count, order and plane-major layout of the ciphertexts stay.  On such a context pirgpu_reply_ct_words is the packed
 * word count, and every fetch, download, host-reply and reply-buffer path moves packed words (capacities stay in
 * ciphertexts); pirgpu_reply_unpack, or pirclient_unpack_reply, gives the residues back.  On the wire a packed reply
 * ciphertext carries compression byte 0x80 in its inner array header: the client must come from this
 * tree.  Allowed with wide items, tables, result_primes, PIRGPU_CREATE_STREAMED_DB, every ring degree and d = 1, 2, 3.
 * One GPU: InvalidArgument at create with a row or slot shard or PIRGPU_CREATE_CT_MULTIPLY; the packed and slot-sharded
 * entry points, pirgpu_reduce_fixup* and the device reply copies are FailedPrecondition.  Without the flag no kernel is
 * launched and no buffer allocated for it. */
#define PIRGPU_CREATE_PACKED_REPLIES 16u
/* PIRGPU_CREATE_CT_COMPACT_REPLY: the reply of a ciphertext-multiplication context, modulus-switched and bit-packed (not
 * in the reference).  Valid only together with PIRGPU_CREATE_CT_MULTIPLY, with or without
 * PIRGPU_CREATE_CT_DEFERRED; without the CT flag the create is InvalidArgument.  Every level is computed bit for bit as
 * on a CT context without the flag, at all k primes -- the product is defined over the full modulus Q, nothing below
 * level 0 is switched.  The finished level-0 ciphertext of every plane (with d = 1: the row sum) is then switched to the
 * first r = result_primes primes by the drop steps of section 6.4 (0 <= r < k is accepted on such a context; r = 0 keeps
 * all k primes; r >= k stays InvalidArgument) and packed as PIRGPU_CREATE_PACKED_REPLIES packs, over those r (or k)
 * moduli.  pirgpu_reply_ct_count stays the number of planes, pirgpu_reply_ct_words is the packed word count,
 * pirgpu_reply_packing is 1, pirgpu_reply_unpacked_words is 2 r N (2 k N at r = 0); the wire form is that of a packed
 * reply at level r, and the client (pirclient with use_ciphertext_multiplication and the same result_primes) decrypts at
 * that level.  PIRGPU_CREATE_PACKED_REPLIES beside PIRGPU_CREATE_CT_MULTIPLY stays InvalidArgument with or without this
 * flag, and so does result_primes on a CT context without it.  Everything PIRGPU_CREATE_CT_MULTIPLY refuses otherwise
 * stays refused (row and slot shards, PIRGPU_CREATE_STREAMED_DB, tables > 1, N = 32768, k > 6); the multi-GPU entry
 * points, pirgpu_reduce_fixup* and the device reply copies are FailedPrecondition.  The transparent-ciphertext rule and
 * the hooks pirgpu_ct_multiply, pirgpu_ct_multiply_sum, pirgpu_relinearize, pirgpu_mod_switch and pirgpu_reply_pack are
 * unchanged.  (Bit 32 stays unknown: flags 32 | 16 remain InvalidArgument.) */
#define PIRGPU_CREATE_CT_COMPACT_REPLY 64u
int pirgpu_create_ex(const pirgpu_params* params, uint32_t flags, pirgpu_ctx** out);
void pirgpu_destroy(pirgpu_ctx* ctx);
/* Message of the calling thread's last failed call on this context (falls back to the context's last
 * failure when this thread has none). */
const char* pirgpu_last_error(const pirgpu_ctx* ctx);
/* Records an error message on the context (used by the wire-level layer). */
void pirgpu_set_error(pirgpu_ctx* ctx, const char* message);
/* The parameters the context was created with (shard range resolved). */
int pirgpu_get_params(const pirgpu_ctx* ctx, pirgpu_params* out);
/* Plaintexts per item of the context (pirgpu_params.plaintexts_per_item resolved: at least 1). */
uint32_t pirgpu_planes(const pirgpu_ctx* ctx);
/* last error of a failed pirgpu_create (no context to ask) */
const char* pirgpu_create_error(void);

/* PIRDatabase::populate(vector<string>) (reference database.cpp:84-110,
 * string_encoder.cpp:58-122).  items: num_items x bytes_per_item raw bytes,
 * item-major; must equal params.num_items.  Bit packing, plain lift and forward
 * NTT all run on the device; the encoded database stays resident in HBM. */
int pirgpu_db_load_items(pirgpu_ctx* ctx, const uint8_t* items, uint64_t num_items, uint32_t bytes_per_item);
/* Tables: loads or reloads table `table` alone (num_items == params.num_items items of it) and leaves the others as they
 * are; a query on a loaded table is answered while other tables are still empty (FailedPrecondition on those).  On a
 * context without tables, table 0 is the database.  Waits for the work queued on the context before it overwrites. */
int pirgpu_db_load_table_items(pirgpu_ctx* ctx, uint32_t table, const uint8_t* items, uint64_t num_items,
                               uint32_t bytes_per_item);
/* PIRDatabase::populate from already-encoded plaintexts (the IntegerEncoder path,
 * reference database.cpp:60-82): coeffs = n_pt x N coefficients, each < t,
 * zero padded; plaintext indices [first_pt, first_pt + n_pt). */
int pirgpu_db_load_coeffs(pirgpu_ctx* ctx, uint64_t first_pt, uint64_t n_pt, const uint64_t* coeffs);
/* PIRDatabase::size() (reference database.h:97) -- plaintexts loaded so far (wide items: over all planes). */
uint64_t pirgpu_db_size(const pirgpu_ctx* ctx);
/* Optional: bring the scan's operand-layout copy of the database up to date now (otherwise done lazily
 * by the first query after a load).  With release_staging != 0 (d >= 2 only) the u64 staging copy that
 * loads write into is freed afterwards: the database then occupies L/8 of its u64 size (plus tile
 * padding) and cannot be reloaded (FailedPrecondition); pirgpu_db_read_plaintext keeps working.
 * No reference counterpart (the reference keeps one vector<Plaintext>, database.h:126-133). */
int pirgpu_db_finalize(pirgpu_ctx* ctx, int release_staging);
/* In-place updates of a fully loaded database (FailedPrecondition before that: the first load is populate); no
 * reference counterpart (database.cpp:84-110 only repopulates).  Afterwards the context is indistinguishable from one
 * populated from scratch with the updated raw database: plaintexts, zero-plaintext count and every query path.  Work
 * and device scratch follow the number of touched plaintexts: only they are re-encoded, and only their columns of the
 * operand-layout copy are rewritten (no repack).  Works with the staging copy kept and after
 * pirgpu_db_finalize(ctx, 1).  The call first waits for all device work queued on the context, then applies the
 * update under the context's lock: no reply mixes old and new plaintexts, and a request made after the call returns
 * sees only the new database.  Argument errors (InvalidArgument) are found before anything changes.  n = 0: no-op.
 *
 * Replace items: item_indices[i] < params.num_items; items = n x bytes_per_item (== params.bytes_per_item), row i is
 * the new value of item item_indices[i].  A later entry wins over an earlier one with the same index.  Indices outside
 * this context's row shard are skipped (every rank of a row-sharded server can be given the same full list).  Every
 * other bit of a touched plaintext -- other items, padding, coefficient bits a coefficient load set -- is kept.
 * A slot shard (slot_begin / slot_end) with released staging returns FailedPrecondition: it holds 1 / G of each
 * plaintext and cannot recover the items it must keep.
 * Wide items (plaintexts_per_item > 1): every plane of a listed item is replaced (an item owns its plaintexts whole, so
 * nothing has to be kept and nothing of the old plaintexts is read). */
int pirgpu_db_update_items(pirgpu_ctx* ctx, uint64_t n, const uint64_t* item_indices, const uint8_t* items,
                           uint32_t bytes_per_item);
/* Replace whole plaintexts given as coefficient rows (each < t; the pirgpu_db_load_coeffs analogue of the above, for
 * any index set): pt_indices[i] < num_pt, coeffs = n x N.  A later entry wins; indices outside the row shard are
 * skipped.  Works on slot shards in every state (it needs no old content). */
int pirgpu_db_update_plaintexts(pirgpu_ctx* ctx, uint64_t n, const uint64_t* pt_indices, const uint64_t* coeffs);
/* SEAL's default build throws logic_error("result ciphertext is transparent") from multiply_plain when a
 * database plaintext is identically zero, which the reference surfaces as InternalError for every query
 * (database.cpp:308-315).  Default (allow == 0): same status.  allow != 0: return the mathematically defined
 * reply instead (what a SEAL built without SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT computes). */
int pirgpu_set_transparent_policy(pirgpu_ctx* ctx, int allow);
/* Row-sharded servers (not in the reference): the reference's transparent-ciphertext failure depends on the WHOLE
 * database, so the ranks exchange their shard's count once after loading (pir_amd.distributed.sync_zero_plaintexts:
 * one all-reduce) and tell their context how many identically-zero plaintexts the other shards hold; every rank then
 * takes the same decision.  pirgpu_check_ready returns what the next query would fail with before any kernel or
 * collective has run: FailedPrecondition (database not fully loaded), Internal (transparent), else 0. */
uint64_t pirgpu_zero_plaintexts(const pirgpu_ctx* ctx);
int pirgpu_set_remote_zero_plaintexts(pirgpu_ctx* ctx, uint64_t count);
/* Tables: identically-zero plaintexts of ONE table -- what decides the transparent-ciphertext failure of the queries that
 * name it (pirgpu_zero_plaintexts keeps counting the whole context); 0 for a table out of range. */
uint64_t pirgpu_table_zero_plaintexts(const pirgpu_ctx* ctx, uint32_t table);
int pirgpu_check_ready(pirgpu_ctx* ctx);
/* Test hook: read back one encoded plaintext [k][N] (NTT form) from HBM (wide items: pt_index = plane * num_pt + pt). */
int pirgpu_db_read_plaintext(pirgpu_ctx* ctx, uint64_t pt_index, uint64_t* out);
/* Device memory of the database, counted by the library at its own allocation sites (not a query of the device: other
 * processes may share it).  out[0] bytes of the operand-layout copy, out[1] bytes of the u64 staging copy (0 on a streamed
 * context, always), out[2] the largest number of bytes operand copy + staging copy + load/update scratch (raw upload
 * buffers, encode scratch, unit lists) ever held at once on this context, out[3] band_bytes of a streamed context --
 * 16 rows of the scanned matrix as u64 residues, the unit of its load chunks -- (0 otherwise).  Fixes the workspace
 * geometry like a first query (set workspace-shaping options before). */
int pirgpu_db_memory(const pirgpu_ctx* ctx, uint64_t out[4]);
/* Test hook: bytes [offset, offset + n) of the operand-layout copy (FailedPrecondition before it exists). */
int pirgpu_db_read_operand(pirgpu_ctx* ctx, uint64_t offset, uint64_t n, uint8_t* out);

/* What SEALDeserialize<GaloisKeys> yields per request (reference server.cpp:46-48):
 * install the key for one Galois element.  Keys stay on the device until cleared.
 * (These two operate on key set slot 0, the default set of every query entry point.) */
int pirgpu_set_galois_key(pirgpu_ctx* ctx, uint32_t galois_elt, const uint64_t* key);
int pirgpu_clear_galois_keys(pirgpu_ctx* ctx);

/* Per-client key sets.  In the reference the Galois keys are locals of one ProcessRequest call (server.cpp:46-48),
 * so requests of different clients are independent; here up to `capacity` clients' keys stay resident in HBM
 * (slots 1..capacity, least recently used evicted; slot 0 is the set above), every query names the slot it is
 * switched with, and the queries of ONE batch group may use different slots (the key-switch kernels index the key
 * of each query's client).
 *   keyset_lookup   finds the resident set that was claimed with exactly these `id` bytes (the wire layer uses the
 *                   serialized GaloisKeys object, any client identifier works); *slot = 0 when not resident.
 *                   verify = 0 accepts a match of length + a sampled fingerprint only; the caller must then confirm
 *                   with keyset_verify (byte-for-byte) before it releases a result computed with that slot.
 *   keyset_claim    empties a free slot -- or the least recently used one, after waiting for the work in flight --
 *                   and tags it with `id`; install the keys with keyset_set_key.  FailedPrecondition when every slot
 *                   belongs to the requests currently being processed together.
 *   keyset_release  empties a slot.
 *   query_use_keyset  slot for pirgpu_process_query / query_run / expand / substitute (default 0).
 *   batch_set_keysets one slot per staged query of the batch (after pirgpu_batch_stage, which resets them to 0).
 *   keyset_stats    [0] resident sets, [1] keys uploaded so far, [2] evictions, [3] capacity.
 * A `slot` is a HANDLE: slot index + the generation of the set living there (0 = the default set).  Once a set has been
 * evicted or released, every entry point that is given its old handle fails with FailedPrecondition ("stale key set
 * handle") instead of switching a query with whichever client's keys moved in -- claim it again.  The same holds for
 * handles the context REMEMBERS: a staged batch (batch_set_keysets) or the query_use_keyset selection whose set has been
 * evicted since fails its next run / expansion with FailedPrecondition.  keyset_claim never evicts a set that requests
 * in flight are pinned to (the wire layer's windows). */
int pirgpu_set_keyset_capacity(pirgpu_ctx* ctx, uint32_t capacity);
int pirgpu_keyset_lookup(pirgpu_ctx* ctx, const uint8_t* id, size_t id_len, int verify, uint32_t* slot);
int pirgpu_keyset_verify(pirgpu_ctx* ctx, uint32_t slot, const uint8_t* id, size_t id_len);
int pirgpu_keyset_claim(pirgpu_ctx* ctx, const uint8_t* id, size_t id_len, uint32_t* slot);
int pirgpu_keyset_release(pirgpu_ctx* ctx, uint32_t slot);
int pirgpu_keyset_set_key(pirgpu_ctx* ctx, uint32_t slot, uint32_t galois_elt, const uint64_t* key);
/* n keys of one set in one call (one wait for all uploads instead of one per key). */
int pirgpu_keyset_set_keys(pirgpu_ctx* ctx, uint32_t slot, uint32_t n, const uint32_t* galois_elts, const uint64_t* const* keys);
/* pirgpu_keyset_set_keys for seed-compressed keys: key i is given as its c0 halves c0[i] = [k][k+1][N] words
 * (any alignment -- they may point straight into request bytes) and seeds[i] = k x 64 bytes; the installed key is
 * exactly the one pirgpu_keyset_set_keys installs for key[j][0] = c0[i][j], key[j][1] = sample_poly_uniform(seed j)
 * (SEAL's BlakePRNG, re-sampled by a kernel on the device: DESIGN.md section 6.7). */
int pirgpu_keyset_set_keys_seeded(pirgpu_ctx* ctx, uint32_t slot, uint32_t n, const uint32_t* galois_elts,
                                  const void* const* c0, const uint8_t* const* seeds);
/* Test hook: n seeds -> out[n][k+1][N] over the context's key-level moduli (the kernel of the call above). */
int pirgpu_expand_seeds(pirgpu_ctx* ctx, const uint8_t* seeds, uint32_t n, uint64_t* out);
/* [0] objects expanded on the device so far, [1] draws those expansions rejected. */
int pirgpu_keyset_seed_stats(pirgpu_ctx* ctx, uint64_t stats[2]);
int pirgpu_query_use_keyset(pirgpu_ctx* ctx, uint32_t slot);
int pirgpu_batch_set_keysets(pirgpu_ctx* ctx, const uint32_t* slots, uint32_t count);
int pirgpu_keyset_stats(pirgpu_ctx* ctx, uint64_t stats[4]);

/* Tables (pirgpu_params.tables resolved: at least 1) and the table a query is answered from.
 *   query_use_table   table for pirgpu_process_query / query_run / multiply and pirgpu_check_ready; sticky like
 *                     pirgpu_query_use_keyset, default 0.
 *   batch_set_tables  one table per staged query of the batch (after pirgpu_batch_stage, which resets them to the
 *                     selected table for all); pirgpu_batch_run_selectors uses them when they were set for as many
 *                     queries as it is given.  The batch is served ordered by table -- equal tables share their pass
 *                     over that table -- and every reply lands at its query's own index: the caller never sees the order.
 * A table >= pirgpu_tables is InvalidArgument before anything is queued or changed.  A batch fails as a whole
 * (FailedPrecondition / Internal) when one of its tables is not fully loaded / holds an all-zero plaintext. */
uint32_t pirgpu_tables(const pirgpu_ctx* ctx);
int pirgpu_query_use_table(pirgpu_ctx* ctx, uint32_t table);
int pirgpu_batch_set_tables(pirgpu_ctx* ctx, const uint32_t* tables, uint32_t count);
/* Test hook (no context, no device): the order and the runs the batch pipeline forms for `count` queries naming these
 * tables, with groups of `group` queries: order[i] = the query served at position i (a stable sort by table);
 * run r = the positions [run_begin[r], run_begin[r + 1]) -- one table, inside one group.  order holds count entries,
 * run_begin count + 1, of which *n_runs + 1 are written. */
int pirgpu_plan_table_runs(const uint32_t* tables, uint32_t count, uint32_t group, uint32_t* order, uint32_t* run_begin,
                           uint32_t* n_runs);

/* PIRServer::processQuery minus (de)serialisation (reference server.cpp:173-195):
 * query = nq ciphertexts (coefficient form), reply = reply_count ciphertexts
 * (coefficient form).  reply_capacity is in ciphertexts. */
int pirgpu_process_query(pirgpu_ctx* ctx, const uint64_t* query, uint32_t nq, uint64_t* reply,
                         uint64_t reply_capacity, uint64_t* reply_count);
/* (2 * ExpansionRatio)^(d-1) (reference client.cpp:224-226, ct_reencoder.cpp:29-38), times plaintexts_per_item */
uint64_t pirgpu_reply_ct_count(const pirgpu_ctx* ctx);
/* CiphertextReencoder::ExpansionRatio (reference ct_reencoder.cpp:29-38); over the first result_primes primes when set */
uint32_t pirgpu_expansion_ratio(const pirgpu_ctx* ctx);
/* Words of one REPLY ciphertext: 2 * result_primes * N, or 2 * k * N when result_primes is 0.  Every reply buffer at
 * this ABI is [ciphertext][2][r][N], compact.  (PIRGPU_CREATE_PACKED_REPLIES: the packed word count, [ciphertext][words].) */
uint64_t pirgpu_reply_ct_words(const pirgpu_ctx* ctx);
/* Test hook for the modulus switch: cts = n coefficient-form ciphertexts [2][k][N] of canonical residues, out =
 * [n][2][r][N]; any 1 <= r < k on any context, whatever its result_primes (the launcher of the query path). */
int pirgpu_mod_switch(pirgpu_ctx* ctx, const uint64_t* cts, uint64_t n, uint32_t r, uint64_t* out);
/* Packed replies (PIRGPU_CREATE_PACKED_REPLIES): 1 on a context created with the flag, else 0; and the words of one reply
 * ciphertext before packing, 2 * r * N (== pirgpu_reply_ct_words without the flag). */
int pirgpu_reply_packing(const pirgpu_ctx* ctx);
uint64_t pirgpu_reply_unpacked_words(const pirgpu_ctx* ctx);
/* Test hooks for packed replies, on any context, for any 1 <= r <= k (the first r data primes): cts = n ciphertexts
 * [2][r][N] of canonical residues (InvalidArgument otherwise) through the device's pack kernel to out = [n][packed words];
 * and packed -> out [n][2][r][N] through the host's unpack (what a client runs; InvalidArgument if a coefficient decodes
 * to a value that is not below its modulus). */
int pirgpu_reply_pack(pirgpu_ctx* ctx, const uint64_t* cts, uint64_t n, uint32_t r, uint64_t* out);
int pirgpu_reply_unpack(pirgpu_ctx* ctx, const uint64_t* packed, uint64_t n, uint32_t r, uint64_t* out);

/* Ciphertext-multiplication mode, host only (no context, no device; like pirgpu_plan_table_runs): the auxiliary base a
 * context of this chain multiplies in -- the k + 2 largest primes == 1 (mod 2N) below 2^bits, bits = the size of the
 * largest data prime, descending, that are neither data primes nor the special prime -- into aux_primes[0 .. k + 2)
 * (*n_aux = k + 2), after checking in integers that Q B > 2 (t N (Q - 1)^2 / 2 + Q) and B > 2 (t N Q + 2).  InvalidArgument
 * (message: pirgpu_create_error) for k > 6, when there are not enough such primes, or when a bound fails. */
int pirgpu_ctmult_plan(uint32_t poly_modulus_degree, uint32_t num_data_primes, const uint64_t* coeff_modulus,
                       uint64_t special_prime, uint64_t plain_modulus, uint64_t* aux_primes, uint32_t* n_aux);
/* Test hooks of the mode (FailedPrecondition on a context without PIRGPU_CREATE_CT_MULTIPLY).  ct_multiply: n pairs of
 * coefficient-form ciphertexts a, b [n][2][k][N] -> out [n][3][k][N] = (d0, d1, d2), the exact product.  relinearize:
 * in [n][3][k][N] -> out [n][2][k][N] = (d0 + KS0(d2), d1 + KS1(d2)) with the relinearisation key of the selected key set
 * (pirgpu_query_use_keyset; the key of Galois element 1).
 * ct_multiply and ct_multiply_sum honour the option "ct_shared_sel": with 0 (the default of a context without wide
 * items) every pair lifts and transforms its four polynomials; with 1 the selectors b of the call (of each block of
 * pairs; of the whole row) are lifted to the auxiliary base and transformed once, in buffers of the call's own, read at
 * Q from the forward transform of a copy, and the products run in the shared-selector kernels of the query path -- the
 * same blocks, the same bits.  Both count into "ct_lifts": 4 per pair, or with ct_shared_sel 2 per pair and 2 per
 * selector lifted (a hook call has one selector per pair: 4 n on n pairs either way). */
/* pirgpu_ctmult_plan with the bound of a sum of up to `terms` products (deferred rounding): Q B > t terms N (Q - 1)^2 + 2 Q
 * and B > 2 (t terms N Q + 2).  terms = 1 is pirgpu_ctmult_plan. */
int pirgpu_ctmult_plan_terms(uint32_t poly_modulus_degree, uint32_t num_data_primes, const uint64_t* coeff_modulus,
                             uint64_t special_prime, uint64_t plain_modulus, uint64_t terms, uint64_t* aux_primes,
                             uint32_t* n_aux);
int pirgpu_ct_multiply(pirgpu_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out);
/* Test hook of the deferred rounding, on any ciphertext-multiplication context: n pairs a, b [n][2][k][N] in coefficient
 * form -> out [3][k][N] = (D0, D1, D2) of the SUM of their tensor products, run as one row of n children through the
 * blocks of the query path (ct_scratch_mb, carried accumulators, the row-sum kernel, one scale).  InvalidArgument when the
 * auxiliary base does not hold a sum of n products. */
int pirgpu_ct_multiply_sum(pirgpu_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out);
int pirgpu_relinearize(pirgpu_ctx* ctx, const uint64_t* in, uint64_t n, uint64_t* out);

/* Device-resident split of pirgpu_process_query for pipelining and measurement:
 * stage = H2D of the query, run = every kernel of the path (asynchronous on the
 * context's stream), fetch = D2H of the reply, sync = wait for the stream. */
int pirgpu_query_stage(pirgpu_ctx* ctx, const uint64_t* query, uint32_t nq);
/* query_stage without the wait: the upload is queued on the context's stream in front of query_run's kernels;
 * `pinned_query` (pirgpu_host_query_buffer or other pinned memory) must stay untouched until query_fetch returns. */
int pirgpu_query_stage_async(pirgpu_ctx* ctx, const uint64_t* pinned_query, uint32_t nq);
int pirgpu_query_run(pirgpu_ctx* ctx);
int pirgpu_query_fetch(pirgpu_ctx* ctx, uint64_t* reply, uint64_t reply_capacity, uint64_t* reply_count);
int pirgpu_sync(pirgpu_ctx* ctx);
/* hipDeviceSynchronize() on the context's device, through the HIP runtime the library itself is linked against: every
 * stream of the device, the library's own included.  (A measurement harness brackets its timed region with this when it
 * has no other handle on the runtime -- bench.py at one GPU, which does not import torch; not in the reference.) */
int pirgpu_device_synchronize(pirgpu_ctx* ctx);

/* Batch mode -- the `for (const auto& query : request.query())` loop of
 * PIRServer::ProcessRequest (reference server.cpp:60-63) with several queries in flight:
 * set_concurrency gives the context n_workers independent working sets (stream +
 * intermediates, ~0.4 GB each at N=4096 / dim_sum=324); batch_stage uploads `count`
 * queries of nq ciphertexts each; batch_run enqueues all of them (asynchronous) in rounds of
 * n_workers queries: groups of up to 8 queries are expanded together (the expansion kernels run
 * over nodes x queries) and, with the int8-MFMA scan (d >= 2), share one pass over the database;
 * consecutive groups alternate between two streams so that scan and expansion overlap
 * (n_workers = 16 keeps both busy); batch_fetch waits and downloads count x reply_ct_count
 * ciphertexts, reply i answering query i. */
int pirgpu_set_concurrency(pirgpu_ctx* ctx, uint32_t n_workers);
int pirgpu_batch_stage(pirgpu_ctx* ctx, const uint64_t* queries, uint32_t nq, uint32_t count);
int pirgpu_batch_run(pirgpu_ctx* ctx);
/* batch_stage without the wait: `pinned_queries` (pirgpu_host_query_buffer, or any pinned memory that stays untouched
 * until the batch has run) goes up in pieces of 8 queries, and each group of a later pirgpu_batch_run waits -- on the
 * device -- only for the pieces that hold its queries.  batch_unstage forgets the staged queries (and with them the
 * references to key sets that pirgpu_batch_set_keysets left).
 * A context has TWO independent sets of batch state (staged queries, replies, their key sets, the host-reply target and
 * its group events, pinned staging): pirgpu_batch_select picks the set the CALLING THREAD's later pirgpu_batch_* /
 * pirgpu_host_*_buffer calls work on (default 0).  Lanes and streams are shared, so batches run from the two sets
 * execute back to back in the order they were queued: one can be parsed, staged and queued while the other is still on
 * the GPU or on its way back to the host (what pirgpu_process_request(s) do with two request windows in flight). */
int pirgpu_batch_stage_async(pirgpu_ctx* ctx, const uint64_t* pinned_queries, uint32_t nq, uint32_t count);
int pirgpu_batch_unstage(pirgpu_ctx* ctx);
/* Compact queries.  Replaces: LoadCiphertexts (serialization.h:44) of a query the client
 * encrypted under the secret key and saved as Serializable<Ciphertext> -- the reference's client.cpp:137 encrypts under
 * the public key, so only this tree's client (pirclient_set_compact_queries) writes such a query.  A compact query
 * ciphertext is c0, [k][N] residues in coefficient form at the data level, plus the 64-byte public seed that defines
 * c1 = sample_poly_uniform(BlakePRNG(seed), q_0 .. q_{k-1}).  c0 comes in one of two forms:
 *   packed = 0   k N little-endian u64 words;
 *   packed = 1   polynomial j as the bit stream of its N coefficients at w_j = bit length of q_j - 1 bits each, N w_j / 64
 *                words (the stream of a packed reply, section 6.8).
 * In both the 8 words of the seed follow c0; query_compact_words is the size of one compact ciphertext in words
 * (k N + 8, or sum_j N w_j / 64 + 8).  `compact` holds [nq] (query_stage_compact) or [count][nq] (batch_stage_compact)
 * of them back to back.  The words are uploaded as they are, c0 is unpacked and c1 re-sampled by kernels on the device
 * (query_expand.hip, seed_expand.hip), and the context is then in exactly the state pirgpu_query_stage /
 * pirgpu_batch_stage(_async) leaves with the expanded [2][k][N] ciphertexts: run, fetch, key sets, tables and every
 * context kind work as they do there.  The _async forms take pinned host memory and return before the upload is done;
 * batch_stage_compact_async uploads and expands in the same pieces of 8 queries pirgpu_batch_stage_async uploads in.
 * Every c0 coefficient is checked on the host before anything is queued: one that is not below its modulus (a packed
 * value may be anywhere in [q, 2^w)) fails the call with InvalidArgument "ciphertext data is invalid (coefficient out of
 * range)" and nothing is staged.  A row- or slot-sharded context fails with FailedPrecondition: compact queries do not
 * feed the multi-GPU entry points.
 *   query_expand        test hook in the manner of pirgpu_expand_seeds: n compact ciphertexts -> out[n][2][k][N].
 *   query_expand_stats  [0] compact ciphertexts expanded on the device so far, [1] draws those expansions rejected. */
uint64_t pirgpu_query_compact_words(const pirgpu_ctx* ctx, int packed);
int pirgpu_query_stage_compact(pirgpu_ctx* ctx, const uint64_t* compact, uint32_t nq, int packed);
int pirgpu_query_stage_compact_async(pirgpu_ctx* ctx, const uint64_t* pinned_compact, uint32_t nq, int packed);
int pirgpu_batch_stage_compact(pirgpu_ctx* ctx, const uint64_t* compact, uint32_t nq, uint32_t count, int packed);
int pirgpu_batch_stage_compact_async(pirgpu_ctx* ctx, const uint64_t* pinned_compact, uint32_t nq, uint32_t count, int packed);
int pirgpu_query_expand(pirgpu_ctx* ctx, const uint64_t* compact, uint32_t n, int packed, uint64_t* out);
int pirgpu_query_expand_stats(pirgpu_ctx* ctx, uint64_t stats[2]);
int pirgpu_batch_select(pirgpu_ctx* ctx, uint32_t which);
int pirgpu_batch_fetch(pirgpu_ctx* ctx, uint64_t* replies, uint64_t reply_capacity, uint64_t* reply_count);
/* Replies on their way to the host while the batch is still running: with a PINNED host buffer set here (capacity in
 * ciphertexts; NULL switches it off), every group of a batch that fits it downloads its replies on its own stream as soon
 * as they exist; pirgpu_batch_fetch into that same buffer then only waits.  (What the wire layer does with
 * pirgpu_host_reply_buffer: 64 MB of replies per 64 queries no longer cross PCIe after the last kernel.) */
int pirgpu_batch_set_host_replies(pirgpu_ctx* ctx, uint64_t* pinned_host, uint64_t capacity);
/* Blocks until the NEXT group of the batch just run has its replies in that host buffer and reports how many leading
 * queries are complete (*ready; the batch's size once every group has been reported): the caller can serialise replies
 * [previous ready, *ready) while the later groups are still being computed.  (A batch served ordered by table,
 * pirgpu_batch_set_tables, finishes its queries out of submission order: *ready is then the number of LEADING queries
 * complete so far and may stay where it was from one group to the next.) */
int pirgpu_batch_next_host_replies(pirgpu_ctx* ctx, uint32_t* ready);
/* Multi-GPU, query-parallel expansion (not in the reference).  batch_expand runs
 * only oblivious_expansion + the selector NTT for the staged queries [first, first+count) and writes
 * their selection vectors (count x dim_sum ciphertexts, NTT form, device order) to caller-owned DEVICE
 * memory, e.g. this rank's slice of an RCCL all-gather buffer.  batch_run_selectors then runs
 * PIRDatabase::multiply for `count` queries whose selection vectors are already in DEVICE memory
 * (query i at device_sv + i * dim_sum ciphertexts) on this context's database shard; replies go to
 * the batch reply buffer like pirgpu_batch_run's. */
int pirgpu_batch_expand(pirgpu_ctx* ctx, uint32_t first, uint32_t count, uint64_t* device_dst);
int pirgpu_batch_run_selectors(pirgpu_ctx* ctx, const uint64_t* device_sv, uint32_t count);
/* Row-sharded multi-GPU runs with the PACKED selector exchange (d = 2 and the int8-MFMA scan on every rank;
 * DESIGN.md section 7).  What every rank needs from a query is (a) all its column selectors, in the scan's
 * B-operand layout (digit-packed signed bytes, one buffer per group of <= 8 queries), and (b) only its own rows'
 * dimension-0 selectors (NTT form, u64).  packed_selector_bytes: size of one group buffer (identical on every rank;
 * 0 if the packed exchange does not apply to this context).  batch_expand_packed: oblivious expansion + selector NTT
 * of the staged queries [first, first+count) in groups of 8 (group g = queries first+8g ..); writes group g's packed
 * column selectors to device_packed + g * packed_selector_bytes and, for every destination rank s holding rows
 * [row_cuts[s], row_cuts[s+1]), the block [count][rows of s][2][k][N] of row selectors, blocks back to back in
 * device_rows (= the send buffer of an all-to-all with split sizes count * rows_s * 2kN words).
 * batch_run_packed: PIRDatabase::multiply on this shard for n_ranks * per_rank queries whose packed groups arrive as
 * [source rank][group] (the all-gather of every rank's device_packed) and whose row selectors for THIS shard's rows
 * arrive as [query][my rows][2][k][N] (the all-to-all's receive buffer); replies go to the batch reply buffer,
 * query i = source rank i / per_rank, its query i % per_rank.  Needs pirgpu_set_concurrency(>= 8). */
uint64_t pirgpu_packed_selector_bytes(pirgpu_ctx* ctx);
int pirgpu_batch_expand_packed(pirgpu_ctx* ctx, uint32_t first, uint32_t count, uint8_t* device_packed,
                               uint64_t* device_rows, const uint32_t* row_cuts, uint32_t n_ranks);
int pirgpu_batch_run_packed(pirgpu_ctx* ctx, const uint8_t* device_packed, uint32_t n_ranks, uint32_t per_rank,
                            const uint64_t* device_rows);
/* Waits for the batch and copies its replies into caller-owned DEVICE memory (multi-GPU reduce). */
int pirgpu_batch_reply_copy_to_device(pirgpu_ctx* ctx, uint64_t* device_dst, uint64_t capacity);

/* Pipelined multi-GPU step: the same entry points without any host synchronisation, plus the
 * device-side ordering a caller needs to hang its collectives between them.  The library queues work on its own HIP
 * streams (a main stream, the batch lanes, the workers):
 *   stream_handle   the main stream (a hipStream_t), e.g. for torch.cuda.ExternalStream -- record / wait events on it;
 *   join            the main stream waits, on the device, for everything queued on lanes and workers so far;
 *   join_stream     the same, but it is `stream` (a hipStream_t of the caller) that waits -- the main stream does not,
 *                   so a later fork does not make every lane wait for every other lane's earlier work;
 *   fork            lanes and workers wait for everything the main stream has been made to wait for;
 *   batch_set_reply_buffer  later batches write their replies into the caller's device buffer (capacity in
 *                   ciphertexts; NULL restores the context's own buffer): a collective can read them where they are;
 *   batch_expand_packed_async      = batch_expand_packed, returns once the work is queued (join to get a completion point);
 *   batch_reply_copy_to_device_async  join + copy on the main stream, no wait;
 *   reduce_fixup_device_async      x mod q_j queued on `stream` (a hipStream_t of the caller; NULL = the main stream).
 * pirgpu_batch_run_packed / _run_selectors / _batch_run never wait for the device in either form. */
void* pirgpu_stream_handle(pirgpu_ctx* ctx);
int pirgpu_join(pirgpu_ctx* ctx);
int pirgpu_join_stream(pirgpu_ctx* ctx, void* stream);
int pirgpu_batch_set_reply_buffer(pirgpu_ctx* ctx, uint64_t* device_buf, uint64_t capacity);
int pirgpu_fork(pirgpu_ctx* ctx);
int pirgpu_batch_expand_packed_async(pirgpu_ctx* ctx, uint32_t first, uint32_t count, uint8_t* device_packed,
                                     uint64_t* device_rows, const uint32_t* row_cuts, uint32_t n_ranks);
int pirgpu_batch_reply_copy_to_device_async(pirgpu_ctx* ctx, uint64_t* device_dst, uint64_t capacity);
int pirgpu_reduce_fixup_device_async(pirgpu_ctx* ctx, uint64_t* device_ptr, uint64_t count, void* stream);
/* Row selectors of the packed exchange in 5 bytes per residue instead of 8 (moduli below 2^40: pack40_supported = 1):
 * `words` u64 residues (a multiple of 4) <-> words * 5 / 4 dwords in DEVICE memory, queued on `stream` (NULL: the main
 * stream).  Every 4 words become 5 dwords, so the packed form of a buffer can be cut wherever the word form is cut at a
 * multiple of 4 words -- e.g. into the per-rank pieces of an all-to-all. */
int pirgpu_pack40_supported(pirgpu_ctx* ctx);
int pirgpu_pack40_device_async(pirgpu_ctx* ctx, const uint64_t* words_in, uint32_t* packed, uint64_t words, void* stream);
int pirgpu_unpack40_device_async(pirgpu_ctx* ctx, const uint32_t* packed, uint64_t* words_out, uint64_t words, void* stream);

/* Slot-sharded multi-GPU step (not in the reference; d = 2, int8-MFMA scan).  G ranks hold the
 * slots [slot_cuts[g], slot_cuts[g+1]) of every plaintext (contexts created with slot_begin / slot_end; a context that
 * holds all slots serves the step too, as the G = 1 case).  One step of B queries, B / G per rank:
 *   slots_expand   oblivious expansion + selector NTT (reference server.cpp:105-171, database.cpp:190,222) of the staged
 *                  queries [first, first + count) in groups of 8; the whole NTT-form selection vectors stay in device_sv
 *                  (count x dim_sum ciphertexts, the context's own element type -- only slots_finish reads them) and the
 *                  column selectors are packed into the scan's B-operand layout, cut by destination rank: piece
 *                  [rank r][group g] of device_packed = the slots of rank r of group g, pirgpu_slots_packed_bytes(ctx,
 *                  slots of r) bytes each -- the send buffer of an all-to-all whose split sizes are groups x that;
 *   slots_scan     the base case of PIRDatabase::multiply (database.cpp:185-194,238-247) on this context's slots for
 *                  n_ranks x per_rank queries in ONE launch: device_packed = the all-to-all's receive buffer,
 *                  [source rank][group][my slots of that group]; row sums go to device_rowsums as
 *                  [source rank][query][row][component][my slots] u64 -- the send buffer of the all-to-all back;
 *   slots_finish   for the `count` queries this rank expanded: device_rowsums = that all-to-all's receive buffer,
 *                  [rank h][query][row][component][slots of h]; puts the pieces together and runs the rest of
 *                  PIRDatabase::multiply (inverse NTT, CiphertextReencoder::Encode, upper level, database.cpp:196-254)
 *                  with the row selectors in device_sv; reply i (reply_ct_count ciphertexts) at device_replies + i.
 * All three only queue work on the context's lanes.  after / then (hipStream_t of the caller, NULL = none): the lanes a
 * call uses first wait -- on the device -- for everything queued on `after` so far, and `then` waits for everything the
 * call queued: the caller's collectives are ordered against the step without a host wait and without a barrier over
 * all lanes.  Needs pirgpu_set_concurrency(>= 8).  No rank exchanges row selectors and there is no reduce: every reply
 * is computed whole by the rank that owns its query. */
uint64_t pirgpu_slots_packed_bytes(pirgpu_ctx* ctx, uint32_t slots);
int pirgpu_slots_expand_async(pirgpu_ctx* ctx, uint32_t first, uint32_t count, uint8_t* device_packed, uint64_t* device_sv,
                              const uint32_t* slot_cuts, uint32_t n_ranks, void* after, void* then);
int pirgpu_slots_scan_async(pirgpu_ctx* ctx, const uint8_t* device_packed, uint32_t n_ranks, uint32_t per_rank,
                            uint64_t* device_rowsums, void* after, void* then);
int pirgpu_slots_finish_async(pirgpu_ctx* ctx, const uint64_t* device_rowsums, uint32_t count, const uint64_t* device_sv,
                              const uint32_t* slot_cuts, uint32_t n_ranks, uint64_t* device_replies, void* after,
                              void* then);

/* PIRServer::oblivious_expansion (reference server.cpp:105-146): one ciphertext
 * -> num_items ciphertexts, coefficient form. */
int pirgpu_expand(pirgpu_ctx* ctx, const uint64_t* ct, uint32_t num_items, uint64_t* out);
/* PIRServer::oblivious_expansion, multi-ciphertext overload (reference server.cpp:148-171). */
int pirgpu_expand_multi(pirgpu_ctx* ctx, const uint64_t* cts, uint32_t num_cts, uint64_t total_items,
                        uint64_t* out);
/* PIRServer::substitute_power_x_inplace (reference server.cpp:67-76). */
int pirgpu_substitute_power_x(pirgpu_ctx* ctx, uint64_t* ct, uint32_t power);
/* PIRServer::multiply_inverse_power_of_x (reference server.cpp:78-103). */
int pirgpu_multiply_inverse_power_of_x(pirgpu_ctx* ctx, const uint64_t* ct, uint32_t k, uint64_t* out);
/* PIRDatabase::multiply (reference database.cpp:290-316): selection vector of
 * sv_count ciphertexts in coefficient form -> reply ciphertexts. */
int pirgpu_multiply(pirgpu_ctx* ctx, const uint64_t* selection_vector, uint64_t sv_count, uint64_t* reply,
                    uint64_t reply_capacity, uint64_t* reply_count);

/* Evaluator::transform_to_ntt_inplace / transform_from_ntt_inplace on count
 * ciphertexts (reference database.cpp:190,252) -- test hooks for the NTT kernels.
 * key_level = 0: ciphertext layout [2][k][N] over q_0..q_{k-1};
 * key_level = 1: polys is count x [k+1][N] over q_0..q_{k-1},p. */
int pirgpu_ntt_forward(pirgpu_ctx* ctx, uint64_t* polys, uint64_t count, int key_level);
int pirgpu_ntt_inverse(pirgpu_ctx* ctx, uint64_t* polys, uint64_t count, int key_level);

/* Multi-GPU reduce step (not in the reference): in place, x[i] <- x[i] mod q_j
 * over count ciphertexts whose words hold integer sums of per-shard partial
 * replies (each partial < q_j, so an 8-way sum fits 64 bits). device_ptr is a
 * device pointer (e.g. a torch tensor's data_ptr after the RCCL all-reduce). */
int pirgpu_reduce_fixup_device(pirgpu_ctx* ctx, uint64_t* device_ptr, uint64_t count);
/* Device pointer of the staged reply (valid until the next run) for collectives. */
uint64_t* pirgpu_reply_device_ptr(pirgpu_ctx* ctx);
/* Copies the reply of the last run into caller-owned DEVICE memory (e.g. a torch
 * tensor handed to RCCL); waits for the copy. capacity is in ciphertexts. */
int pirgpu_reply_copy_to_device(pirgpu_ctx* ctx, uint64_t* device_dst, uint64_t capacity);

/* Wire-level entry: PIRServer::ProcessRequest (reference server.cpp:44-65).
 * request = serialized pir.Request (pir/proto/payload.proto:27-36); on success
 * *response points to a malloc'd serialized pir.Response (payload.proto:39-42)
 * that the caller releases with pirgpu_free.  The SEAL 3.5.6 objects inside the bytes fields may be fully
 * expanded or seed-compressed (Serializable<>, what the reference client sends for its keys); relin_keys, when
 * present, are parsed and validated like server.cpp:53-58.  Atomic on the context (see Conventions). */
int pirgpu_process_request(pirgpu_ctx* ctx, const uint8_t* request, size_t request_len, uint8_t** response,
                           size_t* response_len);
/* The same for n independent requests (different clients) served TOGETHER: every client's Galois keys are looked up
 * among / installed into the resident key sets, all queries go through the batch pipeline as one batch (groups of 8
 * expanded together, each query with its own client's keys, one database pass per group), responses[i] answers
 * requests[i].  status[i] = what pirgpu_process_request would have returned for request i (a failing request does not
 * affect the others); the return value is the first non-zero status.  The requests are served in WINDOWS of at most 64
 * queries and capacity / 2 clients (pirgpu_set_keyset_capacity), two windows in flight: the next one is parsed, staged
 * and queued while the previous one's groups are still on the GPU and its replies are being downloaded and serialised.
 * Threads that call pirgpu_process_request(s) concurrently on one context share those two slots: requests that arrive
 * while both are taken are queued and served together by the next thread that gets one.  Host staging buffers the wire
 * layer uses (pinned, one pair per batch set). */
int pirgpu_process_requests(pirgpu_ctx* ctx, uint32_t n, const uint8_t* const* requests, const size_t* request_lens,
                            uint8_t** responses, size_t* response_lens, int* status);
/* The same two entries on a context with tables: request(s) answered from `table` / request i from tables[i] (every
 * query of a request goes to its request's table; a table out of range fails that request with InvalidArgument).  The
 * request and response bytes are the reference's, unchanged: the table travels beside them, not in them.
 * pirgpu_process_request(s) mean table 0. */
int pirgpu_process_request_table(pirgpu_ctx* ctx, uint32_t table, const uint8_t* request, size_t request_len,
                                 uint8_t** response, size_t* response_len);
int pirgpu_process_requests_tables(pirgpu_ctx* ctx, uint32_t n, const uint8_t* const* requests, const size_t* request_lens,
                                   const uint32_t* tables, uint8_t** responses, size_t* response_lens, int* status);
/* Message of request i of the calling thread's last pirgpu_process_requests / _end call ("" if it succeeded). */
const char* pirgpu_request_error(uint32_t i);
/* The same call in two halves, for ONE calling thread that wants two calls in flight (the reference's harness calls
 * ProcessRequest synchronously, benchmark.cpp:71-79; a server loop need not): begin hands the call to a serving thread of
 * the library and returns at once, end waits for it and returns what pirgpu_process_requests would have.  Every array
 * passed to begin (requests, lengths, responses, status) must stay alive and untouched until end returns; responses and
 * status are valid after end.  begin(i + 1) before end(i) lets call i + 1's parsing, staging and queueing run under
 * call i's tail -- what two calling threads get (two request windows in flight), without the caller owning a second
 * thread.  Every begin must be matched by exactly one end, and the context must outlive every call still pending. */
int pirgpu_process_requests_begin(pirgpu_ctx* ctx, uint32_t n, const uint8_t* const* requests, const size_t* request_lens,
                                  uint8_t** responses, size_t* response_lens, int* status, void** call);
int pirgpu_process_requests_end(void* call);
uint64_t* pirgpu_host_query_buffer(pirgpu_ctx* ctx, uint32_t queries);
uint64_t* pirgpu_host_reply_buffer(pirgpu_ctx* ctx, uint32_t queries);
/* Releases a response buffer.  The library keeps up to 256 MB of released buffers for later responses (a fresh megabyte
 * per reply would cost an mmap, its page faults and a munmap every time); pass only pointers the library returned. */
void pirgpu_free(void* p);

/* Measurement: mean duration of the phases of the pirgpu_query_run calls made since
 * profiling was enabled (or since the previous call of this function), taken with
 * HIP events on the context's own stream.  phase_ms[0..5] = expansion +
 * selection-vector NTT, (reserved, 0), database scan (the streaming kernel alone),
 * upper levels (inverse NTT of the scan rows, re-encode, multiply-accumulate),
 * final inverse NTT, total.  *runs receives the number of runs averaged. */
int pirgpu_last_timings(pirgpu_ctx* ctx, float phase_ms[6], uint32_t* runs);
/* Enable/disable the phase events above (default off: zero overhead). */
int pirgpu_set_profiling(pirgpu_ctx* ctx, int enabled);
/* Measurement, batch pipeline: with profiling enabled, the database-pass launches of the batches run since (up to 64)
 * are bracketed with HIP events on their lane's stream.  Mean / minimum duration of those launches -- the scan as it
 * actually runs inside the headline step: `workgroups` persistent workgroups (0 = one per CU) beside the other lane's
 * kernels, `queries` queries per pass -- and their number; waits for the batch and resets the collection. */
int pirgpu_batch_scan_timings(pirgpu_ctx* ctx, float* mean_ms, float* min_ms, uint32_t* launches, uint32_t* workgroups,
                              uint32_t* queries);
/* Bytes a single-query pass over the database reads: the digit-packed operand-layout copy when that pass
 * is the int8-MFMA scan (info[7] of pirgpu_scan_info), else num_pt(shard) * k * N * 8. */
uint64_t pirgpu_scan_bytes(const pirgpu_ctx* ctx);
/* How this context scans its database.  info[0] = 1 if the digit-sliced int8-MFMA scan is active
 * (0: 64-bit multiply-accumulate kernels), info[1] = digits per residue, info[2] = column chunks per
 * pass, info[3] = k-steps (64 columns) per chunk, info[4] = queries per database pass in batch mode,
 * info[5] = rows, info[6] = columns of the scanned matrix, info[7] = flags: bit 0 = single queries use the MFMA
 * scan as well (matrices wider than one column chunk may scan single queries with the 64-bit kernels), bit 1 = the top
 * digit of database and selectors is stored as a nibble (L - 1/2 bytes per residue instead of L). */
int pirgpu_scan_info(pirgpu_ctx* ctx, uint32_t info[8]);
/* Options by name (case-insensitive), e.g. "scan_mfma" (0 keeps the 64-bit multiply-accumulate scan for d >= 2),
 * "scan_mfma_wgs_batch" (workgroups of a database pass that shares the chip with another group), "scan_launches" (a
 * counter: the database-pass launches the batch pipeline queued so far; setting it overwrites the count).  The table
 * under "Options" in DESIGN.md section 6 lists all of them with kind and default; pir_amd/csrc/options.h declares them.
 * A name that was not set falls back to the environment variable
 * PIRGPU_<NAME> (the A/B scripts under tools/ use that), then to the built-in default; get_option returns -1 for
 * "built-in default".  Options that shape the workspace must be set before the context is first used
 * (FailedPrecondition afterwards).  The arithmetic flavour (PIRGPU_NTT_MODE) is fixed at pirgpu_create.
 * Environment variables are honoured only when PIRGPU_ALLOW_ENV=1 is set too (tests, A/B scripts): by default a
 * context's behaviour depends on its parameters and pirgpu_set_option alone.
 * One switch of the batch pipeline is environment only and NOT an option: PIRGPU_SCAN_MFMA_PAIR (0 | 1 | 2, default 1;
 * read when the context builds its workspace): two groups of 8 queries share one database read (5-digit moduli, d >= 2,
 * one column chunk, plain contexts).  With the default, the first call that queues at least four groups (32 queries
 * with 16 workers) allocates the second group's working buffers on both lanes -- per lane 8 x dim_sum ciphertexts of
 * selection vectors, one packed-selector buffer and one set of row sums: 340 + 104 + 170 MB per lane, about 1.2 GB in
 * all, at N = 4096, 2^20 x 288 B, d = 2 -- and keeps them for the context's life; they are not part of pirgpu_db_memory's
 * count.  Because the environment is honoured only behind PIRGPU_ALLOW_ENV=1, a caller cannot turn pairing off through
 * pirgpu_set_option; a deployment that must not spend that memory sets PIRGPU_ALLOW_ENV=1 PIRGPU_SCAN_MFMA_PAIR=0. */
int pirgpu_set_option(pirgpu_ctx* ctx, const char* name, int64_t value);
int pirgpu_get_option(pirgpu_ctx* ctx, const char* name, int64_t* value);
/* Arithmetic flavour of the transform kernels of this context: 0 = 64-bit integer Shoup/Harvey butterflies (any
 * modulus < 2^61), 1 = exact fp64 (all moduli < 2^46), 2 = exact fp64 with per-stage renormalisation (< 2^49).
 * Chosen from the largest modulus; PIRGPU_NTT_MODE=0|2 in the environment at pirgpu_create forces a more general
 * flavour (all three produce identical residues -- tests/test_gpu_ntt_modes.py). */
int pirgpu_ntt_mode(const pirgpu_ctx* ctx);
/* Which arithmetic paths the moduli (and the options) selected for this context; read-only.  info[0] = the flavour of
 * pirgpu_ntt_mode, info[1] = 1 if the fp64 inverse transform runs without per-pass renormalisation (bits of the
 * largest modulus + log2 N <= 52), info[2] = bytes per residue of the packed key-switch intermediates (5 / 6 / 7;
 * 8 = unpacked 64-bit words or doubles), info[3] = 1 if the expansion tree between fused levels is stored packed as
 * well, info[4] = 128-bit products summed before a reduction (2^(128 - 2 bits), at most 2^30), info[5] = flags: bit 0 =
 * fp64 fold of the scan's digit diagonals for single queries, bit 1 = for groups of queries, bit 2 = 28-bit limb accumulators in the 64-bit scan; info[6..7] = 0. */
int pirgpu_arith_info(pirgpu_ctx* ctx, uint32_t info[8]);
/* The walk this context's oblivious expansion takes for a group of B queries (1 .. 8) that each expand n slots
 * (1 .. N) out of one query ciphertext, with the selectors produced by the last level (every path but pirgpu_expand);
 * read-only, launches nothing.  One word per level j = 0 .. ceil_log2(n) - 1, in the order the levels are queued; *count
 * receives their number (n = 1: none), at most `cap` of them are written to out.  head_split = 1: the walk as a batch
 * takes it when HEAD_MODE (or asynchronous staging) moves the first HEAD_LEVELS levels to the head stream -- the head's
 * levels, then the lane's, picked up from the state the head left -- where the context's dimensions allow the split (one
 * query ciphertext per query, B > 1, at least two levels left for the lane); the unsplit walk otherwise.
 * Bits of a word:  0-1 form (0 unfused: digits, products of all moduli, combine; 1 fused: special-prime product, then
 * products + combine in one kernel; 2 last level in the NTT domain; 3 last level in coefficient form),  2 the tree is read
 * as 5-byte polynomials,  3 ... written as 5-byte polynomials,  4 the digit kernel also transforms c0 (wide NTT-domain last
 * level),  5 looped transforms in the digit kernel,  6 the level's kernels read c0 in NTT form,  7 the tree it leaves has c0
 * in NTT form,  8 c0 is converted in place before the level,  9 ... after it,  10 the combine step is cut at n * B
 * outputs,  11 only the special-prime product is inverse-transformed,  12 the level runs on the head stream,  13-14 0, or
 * the internal error the level would raise (1: 5-byte tree at a level that cannot read it, 2: 5-byte tree at an unfused
 * level, 3: NTT-form c0 at an unfused level; the walk ends there),  15 the context's batch path writes selectors as
 * doubles,  16-19 the level j.  After a walk whose last word has form 0 or 1 (or an empty one) the leaves still get their
 * forward transform. */
int pirgpu_expansion_forms(pirgpu_ctx* ctx, uint32_t B, uint32_t n, int head_split, uint32_t* out, uint32_t cap,
                           uint32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* PIRGPU_H_ */
