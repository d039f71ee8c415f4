/* blsbn254.h -- C ABI of the MI355X-native batched BLS-BN254 verification engine.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / HIP types.  Each entry point
 * names the operator of the reference crate (mikelodder7/bls-bn254, /root/reference) whose body a
 * Rust shim would replace with the extern "C" call (INTEGRATION.md shows the binding).  The
 * reference has no FFI and no BLS scheme layer; the verify / aggregate /
 * threshold entry points are the IETF CoreVerify / CoreAggregateVerify composition of its
 * primitives, min-sig variant (signatures in G1, public keys in G2).
 *
 * Byte formats (authoritative, big-endian field elements):
 *   G1  64 B  x || y                          G1Affine::to_uncompressed      g1.rs:297-302
 *   G2 128 B  x.c1 || x.c0 || y.c1 || y.c0    G2Affine::to_uncompressed      g2.rs:292-300
 *   Gt 384 B  c0.c0.c0, c0.c0.c1, c0.c1.c0 .. c1.c2.c1   Gt::to_repr         pairings.rs:499-514
 *   Fr  32 B  big-endian (both directions; the reference's LE to_repr, E11, is not reproduced)
 *   identity: G1 = (0, 1), G2 = (0, 1); on input x == 0 means identity (g1.rs:352-353, g2.rs:377)
 *   Decoding is strict: a coordinate >= p is an error (the reference masks bit 255 of G1
 *   coordinates, g1.rs:346-347; not reproduced).
 *   Compressed encodings (G1 32 B, G2 64 B, "compressed wire codecs" below) are accepted by exactly
 *   the entry points whose names say so: blsbn254_g1/g2_decompress_batch, blsbn254_g1/g2_inflate_batch
 *   and the *_compressed calls ("compressed input" below).  Every other entry point takes the
 *   uncompressed formats above and nothing else.
 *   msgs = concatenated message bytes, off = n+1 offsets (off[i]..off[i+1] is message i).
 *   bitmaps: ceil(n/8) bytes, bit i of the batch = bit (i & 7) of byte i >> 3.
 *
 * Return codes: 0 ok; 1..4 = Bn254Error::{InvalidScalarBytes, InvalidG1Bytes, InvalidG2Bytes,
 * InvalidGtBytes} in declaration order (error.rs:4-10), returned by the primitive entry points
 * when an operand does not decode (as the reference's TryFrom<&[u8]> does, macros.rs:130-136);
 * negative = BLSBN254_E_*.  In verify_batch a tuple that fails to decode or validate is NOT an
 * error: its bit in the output bitmap is cleared.
 *
 * Threading: a ctx owns one HIP stream and its device workspace on one GPU; calls on one ctx must
 * be externally serialized (the reference is pure and single-threaded, inner_types.rs:33-34).
 * The library never retains caller pointers past return.  There is NO CPU fallback: every entry
 * point fails with BLSBN254_E_NO_DEVICE when no gfx950 device is available.
 */
#ifndef BLSBN254_H
#define BLSBN254_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct blsbn254_ctx blsbn254_ctx;

#define BLSBN254_OK 0
#define BLSBN254_ERR_SCALAR 1 /* Bn254Error::InvalidScalarBytes */
#define BLSBN254_ERR_G1 2     /* Bn254Error::InvalidG1Bytes */
#define BLSBN254_ERR_G2 3     /* Bn254Error::InvalidG2Bytes */
#define BLSBN254_ERR_GT 4     /* Bn254Error::InvalidGtBytes */
#define BLSBN254_E_ARG (-1)
#define BLSBN254_E_HIP (-2)
#define BLSBN254_E_NOMEM (-3)
#define BLSBN254_E_NO_DEVICE (-4)
#define BLSBN254_E_RCCL (-5)

/* One context per GPU (device = HIP ordinal).  Replaces nothing in the reference (it has no
 * state); owns the stream, the workspace and the resident -G2gen line table.  The N-GPU form of SURVEY.md 8b
 * (a ctx over a device list) is blsbn254_multi below, built from these. */
int blsbn254_ctx_create(int device, blsbn254_ctx** out);
void blsbn254_ctx_destroy(blsbn254_ctx* ctx);
const char* blsbn254_strerror(int code);
const char* blsbn254_last_error(blsbn254_ctx* ctx); /* text of the last HIP error on this ctx */

/* ---- primitives, 1:1 with the reference operator API ------------------------------------- */
/* Size limits: entry points whose elements are independent (pairing_batch, miller_loop_batch, final_exponentiation,
 * verify_batch*, pop_verify_batch) accept any n and process it in chunks of 4 Mi elements; the product-type ones
 * (multi_miller_loop, aggregate_*, verify_batch_rlc) take at most 2^23 elements per call (BLSBN254_E_ARG beyond). */
/* pairing(&G1Affine, &G2Affine) -> Gt, pairings.rs:760-802 (pairing::Engine::pairing :685-696).
 * Identity in either slot gives Gt::IDENTITY.  The operands are decoded, not checked: any canonical coordinates (each below p)
 * are accepted -- every point of E(Fp), points of the twist outside the r-torsion, coordinates on no curve at all -- and every
 * size runs the same function of those coordinates whichever device form it takes (one wave, a quad of lanes or one lane per
 * pair): same values, same bytes.  A point that is the identity by its encoding (x = 0, whatever y is) gives the identity.  A
 * coordinate >= p anywhere in the batch is BLSBN254_ERR_G1 / _G2.  Pinned by tests/test_gpu_miller_forms.py. */
int blsbn254_pairing_batch(blsbn254_ctx* ctx, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* gt);
/* multi_miller_loop(&[(&G1Affine, &G2Prepared)]) -> MillerLoopResult, pairings.rs:808-857
 * (pairing::MultiMillerLoop :706-713).  Pairs with an identity member are skipped.  Output = the
 * 384-byte Fp12 Miller-loop value (before final exponentiation).  The operands are decoded, not checked, as for
 * blsbn254_pairing_batch: any canonical coordinates are accepted, every size runs the same function whichever device form it
 * takes, and a member that is the identity by its encoding (x = 0) has its pair skipped.  Pinned by
 * tests/test_gpu_miller_forms.py. */
int blsbn254_multi_miller_loop(blsbn254_ctx* ctx, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t ml_out[384]);
/* n_eq independent multi_miller_loop products (pairings.rs:808-857): equation g owns the pairs
 * g1[64*off[g] .. 64*off[g+1]) / g2[128*off[g] .. 128*off[g+1]) (off: n_eq + 1 non-decreasing element offsets, host array).
 * ml_out[384*g ..] = the product of its Miller values, byte-identical to blsbn254_multi_miller_loop on those pairs.
 * Identity pairs are skipped; an empty group gives Fp12::ONE.  Errors as blsbn254_multi_miller_loop: a pair that does not
 * decode returns BLSBN254_ERR_G1 / _G2 (first bad pair index in last_error).  off[n_eq] - off[0] <= 2^23 pairs and
 * n_eq <= 2^23, else BLSBN254_E_ARG.  n_eq == 0 returns 0. */
int blsbn254_multi_miller_loop_batch(blsbn254_ctx* ctx, const uint8_t* g1, const uint8_t* g2, const uint64_t* off,
                                     size_t n_eq, uint8_t* ml_out /* n_eq*384 */);
/* Bit g (LSB-first) = prod_{j in g} e(P_j, Q_j) == 1, i.e. the product above .final_exponentiation() == Gt::IDENTITY
 * (pairing::MillerLoopResult pairings.rs:698-704, MultiMillerLoop :706-713), AND every P_j decodes and is on the curve
 * (identity allowed), AND every Q_j decodes, is on the curve and lies in the r-torsion (identity allowed).  A bad point
 * clears its equation's bit; it is never an error.  An empty group holds.  Same size limits. */
int blsbn254_pairing_check_batch(blsbn254_ctx* ctx, const uint8_t* g1, const uint8_t* g2, const uint64_t* off,
                                 size_t n_eq, uint8_t* valid_bitmap /* ceil(n_eq/8) */);
/* blsbn254_pairing_check_batch by RANDOM LINEAR COMBINATION ACROSS EQUATIONS: the same arguments plus a seed, the same bitmap
 * (the check prod_j e(P_j, Q_j) == 1 of multi_miller_loop(..).final_exponentiation() == Gt::identity, pairings.rs:706-713 with
 * :698-704 and :808-857, per equation).  Arguments, layout, argument errors, size limits and the n_eq == 0 case are exactly those
 * of blsbn254_pairing_check_batch.  For a range R of equations with secret weights r_g
 *   prod_{g in R} [ prod_j e(P_gj, Q_gj) ]^(r_g)  =  prod_{distinct Q} e( sum_{(g,j): Q_gj = Q} r_g P_gj , Q )
 * so a call over u distinct G2 members (distinct by their 128 bytes) is decided by u table-only Miller loops and ONE final
 * exponentiation, after N weighted G1 points and N G1 additions, where the exact call runs a variable-Q Miller slot and a torsion
 * test per pair and a final exponentiation per equation.  Weighing P is the r_g-th power of e(P, Q) only for a Q in the r-torsion;
 * that is why only equations whose every Q is the identity or in the r-torsion take part, and each DISTINCT Q is tested once.
 * A pair is OK when P decodes and is on the curve (identity allowed) and Q decodes and is the identity or is on the curve and in
 * the r-torsion: the exact call's predicate.  A pair with a member that is the identity by its encoding (x = 0) is SKIPPED: it
 * contributes nothing.  An equation is ELIGIBLE when all its pairs are OK; an empty equation, or one whose pairs are all skipped,
 * is eligible and holds.  An ineligible equation has bit 0 -- the exact call's bit -- and costs no equation and no exact sub-call;
 * a bad point is never an error.
 * Round 1: when the G2 members repeat (N > 0, 2 u <= N and u <= 65536) all eligible equations of the call form one combined
 * equation; if it holds, every eligible equation has its bit set.  Otherwise the call IS the exact call (counted in out[6]).
 * Round 2, only when round 1 fails: the equations are cut into S segments of consecutive equations, each checked as its own
 * combined equation in one batched pass over the weighted points of round 1 (nothing is decoded or weighed twice);
 * S = min(256, N / (2 u)) unless blsbn254_set_pairing_check_rlc_segments fixes it (0 restores that rule, 1 = no second round,
 * 2 .. 4096 = S, never more segments than equations; anything else is BLSBN254_E_ARG), and the round is skipped when S < 2.  The
 * eligible equations of a segment that passes have their bits set.  The eligible equations of the segments that FAILED (all of
 * them when round 2 is skipped) are decided by blsbn254_pairing_check_batch itself on their contiguous equation ranges, adjacent
 * failed segments merged, and ranges with fewer than 2^15 pairs and equations between them made one; only the bits of eligible
 * equations are taken from it.  So bit g is bit g of the exact call on the same arguments, and can differ only where an invalid
 * range passed its equation: probability at most 2^-64 per equation checked, given a fresh secret seed.
 * Weights: r_g = a_g + b_g lambda (lambda the eigenvalue of phi(x, y) = (beta x, y) on G1) with the 32-bit a_g = the first 4 bytes
 * and b_g = the next 4 bytes, each big-endian, of SHA-256(seed || "PCRLC" || g as 8 bytes little-endian), g the equation's index
 * within the call; (0, 0) becomes (1, 0).  The 2^64 pairs give 2^64 distinct weights mod r, as for blsbn254_verify_batch_rlc.
 * seed = NULL (the production setting): the library draws 32 bytes from the OS (getrandom) inside the call, i.e. after
 * the batch is fixed.  A caller-supplied seed exists for reproducible tests; soundness then rests on that seed being
 * fresh and secret -- never reuse one, never derive it from public data.
 * Pending asynchronous verify calls are settled on entry and none is left pending.
 * blsbn254_pairing_check_rlc_stats, since the context was created: out[0] calls, out[1] equations decided by round 1, out[2]
 * equations decided by round 2, out[3] equations sent to the exact pipeline (the eligible equations inside the ranges of the
 * sub-calls; every equation of a call that did not take round 1), out[4] ineligible equations, out[5] combined equations checked,
 * out[6] calls that did not take round 1, out[7] segments that failed.  NULL out: BLSBN254_E_ARG. */
int blsbn254_pairing_check_batch_rlc(blsbn254_ctx* ctx, const uint8_t* g1, const uint8_t* g2, const uint64_t* off,
                                     size_t n_eq, const uint8_t seed[32] /* NULL: getrandom inside the call */,
                                     uint8_t* valid_bitmap /* ceil(n_eq/8) */);
int blsbn254_set_pairing_check_rlc_segments(blsbn254_ctx* ctx, size_t segments);
int blsbn254_pairing_check_rlc_stats(blsbn254_ctx* ctx, uint64_t out[8]);
/* per-pair Miller loops (no product): n outputs of 384 B.  The operands are decoded, not checked, as for
 * blsbn254_pairing_batch: any canonical coordinates are accepted, every size runs the same function whichever device form it
 * takes, and a pair with a member that is the identity by its encoding (x = 0) gives Fp12::ONE.  Pinned by
 * tests/test_gpu_miller_forms.py. */
int blsbn254_miller_loop_batch(blsbn254_ctx* ctx, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* ml_out);
/* MillerLoopResult::final_exponentiation, pairings.rs:50-178 (pairing::MillerLoopResult :698-704).  The input need not be a Miller
 * value: any twelve canonical coefficients (each below p, Gt::to_repr order) are accepted, and every size runs the same function
 * whichever device form it takes.  0 maps to 0 (384 zero bytes: the inversion's inv0 convention); an element of a proper
 * subfield (Fp, Fp2, Fp6) or of w Fp6 maps to the identity.  A coefficient >= p anywhere in the batch is BLSBN254_ERR_GT.
 * Pinned by tests/test_gpu_final_exp_forms.py. */
int blsbn254_final_exponentiation(blsbn254_ctx* ctx, const uint8_t* ml, size_t n, uint8_t* gt);
/* G1Projective::hash::<ExpandMsgXmd<Sha256>>(msg, dst), g1.rs:910-919; ::encode g1.rs:922-928 */
int blsbn254_hash_to_g1_batch(blsbn254_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t n,
                              const uint8_t* dst, size_t dst_len, uint8_t* out);
int blsbn254_encode_to_g1_batch(blsbn254_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t n,
                                const uint8_t* dst, size_t dst_len, uint8_t* out);
/* G2Projective::hash / ::encode, g2.rs:919-936 */
int blsbn254_hash_to_g2_batch(blsbn254_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t n,
                              const uint8_t* dst, size_t dst_len, uint8_t* out);
int blsbn254_encode_to_g2_batch(blsbn254_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t n,
                                const uint8_t* dst, size_t dst_len, uint8_t* out);
/* The message expander: the type parameter X: ExpandMsg of Fp::hash<X> / Fp::encode<X> (fp.rs:433-458), Fp2::hash<X>
 * (fp2.rs:463-487), G1Projective::hash<X> / encode<X> (g1.rs:910-928), G2Projective::hash<X> / encode<X> (g2.rs:919-936) and
 * Scalar::hash<X> (scalar.rs:554-563), as a setting of the context.  XMD: RFC 9380 5.3.1 (Keccak-256 and SHA3-256 with
 * s_in_bytes = 136); XOF: 5.3.2.  Keccak-256 is the hash of the EVM (domain byte 0x01), SHA3-256 the FIPS 202 one (0x06).
 * EVERY call that hashes a message follows the setting, without an argument of its own: the hash / encode calls above, verify
 * in all its forms (exact, RLC, compressed, prepared, _dev), aggregate verify with its batch and RLC forms, fast aggregate
 * verify, the key-set and committee calls, the threshold share checks and the checked combine, sign_batch, pop_prove_batch /
 * pop_verify_batch, keyset_create_checked and hash_to_scalar_batch.  blsbn254_keygen_batch does not: its HKDF-SHA-256 is fixed
 * by the BLS draft and is no ExpandMsg.  No result changes under the default.  The rules:
 *   - an id outside the table returns BLSBN254_E_ARG and changes nothing;
 *   - the setter settles the context first: pending asynchronous verify calls are resolved (a failed guess re-run) under the
 *     expander they were made with before the new one is stored;
 *   - a DST longer than 255 bytes is replaced as RFC 9380 5.3.3 says, with the CONTEXT's hash: H("H2C-OVERSIZE-DST-" || dst),
 *     32 bytes, for the XMD forms; H(..., 32) for the XOF forms (ceil(2 k / 8) with k = 128).
 * The multi-GPU handle has no call of its own: blsbn254_set_expander(blsbn254_multi_ctx(m, i), id) for each device i. */
#define BLSBN254_EXPAND_XMD_SHA256 0    /* ExpandMsgXmd<sha2::Sha256>, the default */
#define BLSBN254_EXPAND_XMD_KECCAK256 1 /* ExpandMsgXmd<sha3::Keccak256> */
#define BLSBN254_EXPAND_XMD_SHA3_256 2  /* ExpandMsgXmd<sha3::Sha3_256> */
#define BLSBN254_EXPAND_XOF_SHAKE128 3  /* ExpandMsgXof<sha3::Shake128> */
#define BLSBN254_EXPAND_XOF_SHAKE256 4  /* ExpandMsgXof<sha3::Shake256> */
int blsbn254_set_expander(blsbn254_ctx* ctx, int id);
int blsbn254_get_expander(const blsbn254_ctx* ctx); /* the id in force; BLSBN254_E_ARG for NULL */
/* The map behind every MESSAGE hashed to G1, as a setting of the context.  SVDW is RFC 9380's hash_to_curve as above; the two
 * others are the try-and-increment map of the BN254 BLS contracts deployed on the EVM (hashToG1(bytes32) and its kin), whose
 * layout is this library's: signatures in G1, keys in G2, e(sig, -G2gen) * e(H(m), pk) == 1.  The map, exactly as they compute it:
 *   x0     TAI_DIGEST: the message bytes read as ONE big-endian integer, reduced mod p; for 32 bytes uint256(h) % p.  Any other
 *          length is reduced the same way: a total function, with NO security claim for anything but a 32-byte digest.
 *          TAI_HASH: the 32-byte digest of the message, reduced mod p, under the plain hash of the context's expander: SHA-256
 *          (id 0), Keccak-256 (1), SHA3-256 (2), the first 32 bytes of SHAKE-128 (3) / SHAKE-256 (4).  No tag, no padding block.
 *   point  for k = 0, 1, 2, ...: x = x0 + k mod p, beta = x^3 + 3; the first x whose beta is a square gives (x, beta^((p+1)/4)):
 *          exactly that root, no sign rule.  (beta == 0 cannot happen on a curve of prime order.)  The search is bounded: after
 *          65 536 non-residues in a row (probability 2^-65536) the result is the off-curve point (0, 0), which no equation accepts.
 * The dst argument is accepted and IGNORED under both TAI ids: the map has no tag.
 * FOLLOW the setting: blsbn254_hash_to_g1_batch, verify in all its forms (exact, RLC, compressed, prepared, _dev, multi), aggregate
 * verify with its batch and RLC forms, fast aggregate verify, the key-set and committee families, the threshold share checks and
 * the checked combine, and blsbn254_sign_batch.
 * DO NOT follow it and keep SVDW with their tag: blsbn254_encode_to_g1_batch, the G2 and scalar hashes, blsbn254_pop_prove_batch,
 * blsbn254_pop_verify_batch and the proof check of blsbn254_keyset_create_checked.  Try-and-increment has no tag, so a proof of
 * possession under it would share its domain with messages; an EVM-side registration proof is an ordinary blsbn254_verify_batch
 * over the digest the application defines.
 * The rules are the expander's: an id outside the table returns BLSBN254_E_ARG and changes nothing; the setter settles the
 * context first (pending asynchronous verify calls are resolved under the old map before the new id is stored); the multi-GPU
 * handle has no call of its own: blsbn254_set_g1_map(blsbn254_multi_ctx(m, i), id) for each device i. */
#define BLSBN254_G1MAP_SVDW 0       /* RFC 9380 hash_to_curve, the default: nothing changes */
#define BLSBN254_G1MAP_TAI_DIGEST 1 /* try-and-increment, the message IS the digest */
#define BLSBN254_G1MAP_TAI_HASH 2   /* try-and-increment, digest = H(msg), H the plain hash of the context's expander */
int blsbn254_set_g1_map(blsbn254_ctx* ctx, int id);
int blsbn254_get_g1_map(const blsbn254_ctx* ctx); /* the id in force; BLSBN254_E_ARG for NULL */
/* G1Affine::from_uncompressed + is_on_curve (g1.rs:339-360, :383-391); G1 has cofactor 1 */
int blsbn254_g1_check_batch(blsbn254_ctx* ctx, const uint8_t* g1, size_t n, uint8_t* ok_bitmap);
/* G2Affine::from_uncompressed + is_on_curve + is_torsion_free (g2.rs:350-414, :733-736) */
int blsbn254_g2_check_batch(blsbn254_ctx* ctx, const uint8_t* g2, size_t n, uint8_t* ok_bitmap);

/* ---- BLS layer (build-defined composition; min-sig) ---------------------------------------- */
/* valid_i = sig_i in G1 \ {O}  and  pk_i in G2 \ {O} (on curve, torsion free)  and
 *           e(sig_i, -G2gen) * e(H(msg_i), pk_i) == 1 */
int blsbn254_verify_batch(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                          const uint8_t* sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap);
/* valid = prod_i e(H(msg_i), pk_i) * e(agg_sig, -G2gen) == 1, every pk_i valid, n >= 1.
 * PRECONDITION (rogue-key protection, IETF BLS section 3): this is CoreAggregateVerify -- the algebraic check only.  With a
 * basic-scheme tag (the suggested default DST ends in _NUL_) batches with repeated messages must be rejected;
 * alternatively use a proof-of-possession tag (_POP_) and only keys whose proof passed blsbn254_pop_verify_batch.
 * THIS call does not detect repeated messages (the reference has no BLS layer to pin either behaviour).  The library checks
 * the rule on the device, on the hash POINTS: blsbn254_hash_distinct_batch with one group (n_groups = 1, grp_off = {0, n})
 * gives the rule's bit for the messages of this call, of blsbn254_aggregate_verify_prepared, of
 * blsbn254_aggregate_partial and of blsbn254_aggregate_verify_multi; the batched calls have forms that apply it
 * themselves (blsbn254_aggregate_verify_batch_distinct, blsbn254_aggregate_verify_batch_rlc_distinct). */
int blsbn254_aggregate_verify(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                              const uint8_t agg_sig[64], const uint8_t* dst, size_t dst_len, int* valid);
/* blsbn254_aggregate_verify for many independent aggregates in one call: bit g (LSB-first) of valid_bitmap = *valid of
 * blsbn254_aggregate_verify on group g alone.  Group g owns the pairs grp_off[g] .. grp_off[g + 1] (element offsets, non-decreasing,
 * need not start at 0); pair indices are absolute: pair i has key pks[128 i ..] and message msgs[off[i] .. off[i + 1]), so off
 * holds grp_off[n_groups] + 1 entries; group g's aggregate signature is agg_sigs[64 g ..]; one dst serves all groups.
 * A group is valid when it has at least one pair (an empty group is INVALID, as the single call's n == 0), its signature decodes,
 * is not the identity and is on the curve, every key decodes, is not the identity, is on the curve and in the r-torsion, and
 * e(agg_sig, -G2gen) * prod_i e(H(msg_i), pk_i) == 1.  A bad point clears its group's bit and nothing else; it is never an
 * error of the call.  The PRECONDITION of blsbn254_aggregate_verify (rogue keys / repeated messages) holds per group: this call
 * does not apply the rule, blsbn254_aggregate_verify_batch_distinct does.
 * Two pairs per lane share one f^2 (the signature's pair, whose -G2gen is a constant and is never validated, included); the hash
 * points never leave the device.  BLSBN254_E_ARG: NULL arguments, decreasing offsets, pairs + n_groups > 2^23 (the signatures'
 * pairs count).  n_groups == 0 returns 0.  Launches span at most BLSBN254_CHUNK_LANES lanes.
 * blsbn254_aggregate_batch_stats, since the context was created: out[0] groups served, out[1] lanes run by the two-pair kernel,
 * out[2] calls served by the small forms (none in this build: every size takes the two-pair kernel), out[3] launches. */
int blsbn254_aggregate_verify_batch(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                                    const uint64_t* grp_off /* n_groups+1 */, const uint8_t* agg_sigs /* n_groups*64 */,
                                    size_t n_groups, const uint8_t* dst, size_t dst_len,
                                    uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_aggregate_batch_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* blsbn254_aggregate_verify_batch by RANDOM LINEAR COMBINATION ACROSS GROUPS: the same arguments plus a seed, the same bitmap.
 * Arguments, layout, argument errors and the n_groups == 0 and all-empty cases are exactly those of
 * blsbn254_aggregate_verify_batch.  For a range R of groups with secret weights r_g
 *   prod_{g in R} [ e(sig_g, -G2gen) prod_i e(H_gi, pk_gi) ]^(r_g)
 *     = e(sum_g r_g sig_g, -G2gen) * prod_{distinct pk} e(sum_{(g,i): pk_gi = pk} r_g H_gi, pk)
 * so a call over a pool of u keys is decided by u + 1 table-only Miller loops and ONE final exponentiation, after N weighted
 * hash points and N G1 additions, where the exact call runs a variable-Q Miller slot per pair and per signature and a final
 * exponentiation per group.
 * A group takes part only when it is ELIGIBLE: it has at least one pair, its signature decodes, is on the curve and is not the
 * identity, and every key of it is valid by the checks of the key preparation (decodes, not the identity, on the curve, in the
 * r-torsion).  An ineligible group has bit 0 -- the exact call's bit -- and costs no equation and no exact sub-call.
 * Round 1: when the keys repeat (u distinct keys among the N pairs of the call, 2 u <= N and u < 65536) all eligible groups of the
 * call form one virtual aggregate; if its equation holds, every eligible group has its bit set.  When the keys do not repeat the
 * call IS the exact call (counted in out[6]).  Round 2, only when round 1 fails: the groups are cut into S segments of consecutive
 * groups, each checked as its own virtual aggregate in one batched pass over the weighted points of round 1 (nothing is hashed or
 * weighed twice); S = min(16, N / (2 u)) unless blsbn254_set_aggregate_rlc_segments fixes it (0 restores that rule, 1 = no second
 * round, 2 .. 4096 = S, never more segments than groups; anything else is BLSBN254_E_ARG), and the round is skipped when S < 2.
 * The eligible groups of a segment that passes have their bits set.  The eligible groups of the segments that FAILED (all of them
 * when round 2 is skipped) are decided by blsbn254_aggregate_verify_batch's own pipeline on their contiguous group ranges, adjacent
 * failed segments merged, and ranges with fewer than 2^16 pairs and signatures between them made one; only the bits of eligible groups are taken from it.  So bit g is bit g of the exact call on the same arguments, and can
 * differ only where an invalid range passed its equation: probability at most 2^-64 per equation checked, given a fresh secret seed.
 * Weights: r_g = a_g + b_g lambda (lambda the eigenvalue of phi(x, y) = (beta x, y) on G1) with the 32-bit a_g = the first 4 bytes
 * and b_g = the next 4 bytes, each big-endian, of SHA-256(seed || "AGRLC" || g as 8 bytes little-endian || sig_g); (0, 0) becomes
 * (1, 0).  The 2^64 pairs give 2^64 distinct weights mod r, as for blsbn254_verify_batch_rlc.
 * seed = NULL (the production setting): the library draws 32 bytes from the OS (getrandom) inside the call, i.e. after
 * the batch is fixed.  A caller-supplied seed exists for reproducible tests; soundness then rests on that seed being
 * fresh and secret -- never reuse one, never derive it from public data.
 * The PRECONDITION of blsbn254_aggregate_verify (rogue keys / repeated messages) holds per group: this call does not apply the
 * rule, blsbn254_aggregate_verify_batch_rlc_distinct does.
 * Pending asynchronous verify calls are settled on entry and none is left pending.
 * blsbn254_aggregate_rlc_stats, since the context was created: out[0] calls, out[1] groups decided by round 1, out[2] groups decided
 * by round 2, out[3] groups sent to the exact pipeline (the eligible groups inside the ranges of the sub-calls: those of failed
 * segments, and those between two ranges made one; every group of a call that did not take round 1), out[4] ineligible groups, out[5] equations checked, out[6] calls that did not take round 1 (keys do not repeat),
 * out[7] segments that failed.  blsbn254_aggregate_batch_stats keeps counting whatever the exact sub-calls serve (the groups of
 * their ranges, ineligible ones between eligible ones included).  NULL out: BLSBN254_E_ARG. */
int blsbn254_aggregate_verify_batch_rlc(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                                        const uint64_t* grp_off /* n_groups+1 */, const uint8_t* agg_sigs /* n_groups*64 */,
                                        size_t n_groups, const uint8_t* dst, size_t dst_len,
                                        const uint8_t seed[32] /* NULL: getrandom inside the call */,
                                        uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_set_aggregate_rlc_segments(blsbn254_ctx* ctx, size_t segments);
int blsbn254_aggregate_rlc_stats(blsbn254_ctx* ctx, uint64_t out[8]);
/* THE DISTINCT-MESSAGE RULE, checked on the device.  Group g is REPEATED when two of its pairs have the same hash point: equal
 * affine (x, y) as field elements, under the context's expander and map.  A repeated group under a basic-scheme tag is open to a
 * rogue key (pk2 = [a] G2gen - pk1, sig = [a] H(m) passes for {(pk1, m), (pk2, m)} with nobody having signed), so the calls below
 * treat it as INVALID: never an error of the call, and it never touches its neighbours.
 * POINTS, NOT BYTES: under the try-and-increment maps different messages can share a point (BLSBN254_G1MAP_TAI_DIGEST: the digests
 * h and h + p; any map of the two: a start value x0 that is no x of the curve and x0 + 1), so comparing message bytes -- all a
 * caller can do, because the hash points never leave the device -- misses repeats that this rule finds.  Under the RFC 9380 map
 * the two notions agree up to collisions of the hash.
 * Scope: the same point in two DIFFERENT groups is no repeat; pairs in front of grp_off[0] belong to no group; an empty group is
 * not repeated (and stays invalid); key validity plays no part, a pair whose key does not decode still counts.
 * How: one lane per pair puts (group, canonical x, canonical y) into an open-addressing table of 2^k >= 2 N slots, seeded per
 * context, with a full comparison of group and point on every taken slot; the result does not depend on the order of arrival.
 * Memory the stage reserves in the context: 72 bytes per pair for the canonical points, 8 .. 16 bytes per pair for the table,
 * one byte and one bit per group.
 *
 * blsbn254_hash_distinct_batch: bit g (LSB-first) of dup_bitmap = group g is repeated.  Hashes as blsbn254_hash_to_g1_batch does;
 * msgs / off / grp_off as blsbn254_aggregate_verify_batch takes them; nothing else is computed.  Argument errors, n_groups == 0
 * (returns 0, nothing written), the all-empty case (all bits 0) and the size limits are those of blsbn254_aggregate_verify_batch.
 * blsbn254_aggregate_verify_batch_distinct / blsbn254_aggregate_verify_batch_rlc_distinct: bit g of valid_bitmap = bit g of
 * blsbn254_aggregate_verify_batch (of its _rlc form) on the same arguments AND NOT bit g of dup_bitmap; dup_bitmap may be NULL.
 * The stage runs on the hash points the call's pipeline has produced anyway (affine in the exact call, homogeneous -- normalised
 * by one inversion per pair -- in the RLC call): nothing is hashed twice and no point is downloaded.  Everything else, the
 * counters of blsbn254_aggregate_batch_stats / blsbn254_aggregate_rlc_stats included, is the parent call's.
 * blsbn254_msg_distinct_stats, since the context was created: out[0] calls that applied the rule, out[1] pairs inserted, out[2]
 * groups found repeated, out[3] slots of the last call's table.  NULL out: BLSBN254_E_ARG. */
int blsbn254_hash_distinct_batch(blsbn254_ctx* ctx, const uint8_t* msgs, const uint64_t* off,
                                 const uint64_t* grp_off /* n_groups+1 */, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                 uint8_t* dup_bitmap /* ceil(n_groups/8) */);
int blsbn254_aggregate_verify_batch_distinct(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                                             const uint64_t* grp_off /* n_groups+1 */, const uint8_t* agg_sigs /* n_groups*64 */,
                                             size_t n_groups, const uint8_t* dst, size_t dst_len,
                                             uint8_t* valid_bitmap /* ceil(n_groups/8) */,
                                             uint8_t* dup_bitmap /* ceil(n_groups/8), or NULL */);
int blsbn254_aggregate_verify_batch_rlc_distinct(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                                                 const uint64_t* grp_off /* n_groups+1 */, const uint8_t* agg_sigs /* n_groups*64 */,
                                                 size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                 const uint8_t seed[32] /* NULL: getrandom inside the call */,
                                                 uint8_t* valid_bitmap /* ceil(n_groups/8) */,
                                                 uint8_t* dup_bitmap /* ceil(n_groups/8), or NULL */);
int blsbn254_msg_distinct_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* Repeated signers.  blsbn254_verify_batch (and _dev) de-duplicates the public keys of a batch on the GPU (hash table over
 * the 128-byte encodings, full comparison on every hit) and, when at most half of them are distinct (and at most 65536),
 * validates each DISTINCT key once and turns it into its table of 88 line-coefficient triples -- G2Prepared::from,
 * pairings.rs:609-660 (E6: 88 entries, not 68) -- beside hash-to-G1; the tuples then run a table-only Miller loop
 * (multi_miller_loop over prepared terms, pairings.rs:808-857) in key-sorted order.  Same bitmap as the exact
 * per-tuple path, which batches of mostly distinct keys keep taking.  BLSBN254_AUTO_PREPARE=0 in the environment or
 * blsbn254_set_auto_prepare(ctx, 0) forces the exact path; blsbn254_path_stats counts the chunks each path served.
 * Small and mid-size calls.  A launch that does not fill the chip is bound by the latency of one lane's chain, so such calls
 * (verify, pairing, Miller loop, final exponentiation, aggregate verify) run the Miller loop and the hard part of the final
 * exponentiation with one WAVE per tuple up to 2048 tuples and with THREE LANES per tuple (a DPP quad: the three Fp6 products
 * of an Fp12 product side by side) up to 16384 -- same values, same bytes -- and verify chunks of those sizes take the
 * prepared-key path whatever their keys (the tables are what those Miller loops read; the per-key preparation itself runs four
 * lanes per key).  BLSBN254_WIDE_FE=0 / BLSBN254_TRI_MAX=0 switch the two forms off, BLSBN254_WIDE_FE_MAX=<n> /
 * BLSBN254_TRI_MAX=<n> move the limits, BLSBN254_QUAD_PREP=0 keeps the per-key preparation on one lane per key. */
int blsbn254_set_auto_prepare(blsbn254_ctx* ctx, int on);
/* Prepared keys stay resident.  A validator set's keys are the same from batch to batch, so the context keeps the tables of the
 * keys it has prepared: blsbn254_verify_batch (and _dev, on the counting and on the asynchronous path) and
 * blsbn254_verify_batch_rlc(_dev) look every distinct key of a batch up by its 128 bytes (hash table, full comparison) and
 * prepare only the keys that are new to the context; an invalid key is kept as invalid.  The store holds max_keys keys (default
 * 4096, BLSBN254_KEY_CACHE=<n>; 57 KB of device memory per key, 234 MB at the default, taken by the first call that uses it); it
 * has room for at least the key capacity of the call at hand -- a larger call reallocates it, which empties it.  A batch whose
 * distinct keys do not fit behind the resident ones (resident + distinct > max_keys; the keys are counted before they are looked
 * up, so a key set stays resident when it is at most half of max_keys) empties the store first -- decided on the device, no
 * read-back -- and costs what every batch costs without a store.  Results never depend on what is resident.  blsbn254_set_key_cache(ctx, 0) turns the store off: every call
 * prepares its keys.  Any other value empties the store and sets its size; the call waits for the device.
 * blsbn254_key_cache_stats (waits for the device too): out[0] keys found resident, out[1] keys prepared, out[2] times the store
 * was emptied because a batch did not fit, all counted on the device over every enqueued run (a run that the asynchronous path
 * discards and repeats counts twice); out[3] keys resident now. */
int blsbn254_set_key_cache(blsbn254_ctx* ctx, size_t max_keys /* <= 65536 */);
int blsbn254_key_cache_stats(blsbn254_ctx* ctx, uint64_t out[4] /* hits, misses, resets, resident */);
int blsbn254_path_stats(blsbn254_ctx* ctx, uint64_t out[2] /* prepared, exact */);
/* blsbn254_aggregate_verify over repeated keys (auto-prepare on; at most half of the n >= 1024 keys distinct, or at most 16383 pairs):
 * by bilinearity in the first argument  prod_{i: pk_i = pk} e(H(msg_i), pk) = e(sum_i H(msg_i), pk)  -- exact, no randomness --
 * the H(msg_i) of every distinct key are summed in G1 (n additions) and ONE Miller loop per distinct key runs
 * (multi_miller_loop over u + 1 prepared terms, pairings.rs:808-857).  Same boolean; the Miller value differs from the product
 * of the n per-pair values, which blsbn254_aggregate_partial keeps computing bit-exactly for the sharded API.
 * out[0] = calls served by key sums, out[1] = calls served pair by pair. */
int blsbn254_aggregate_path_stats(blsbn254_ctx* ctx, uint64_t out[2]);
/* The explicit form: prepare u keys once (device-resident, owned by the handle, tied to ctx), then verify any number of
 * batches against them, naming the key of every tuple by its index (key_idx[i] < u, else BLSBN254_E_ARG).  A key that
 * does not decode, is the identity, is off the curve or outside the r-torsion makes its tuples invalid (bit cleared). */
typedef struct blsbn254_g2prepared blsbn254_g2prepared;
int blsbn254_g2_prepare_batch(blsbn254_ctx* ctx, const uint8_t* pks /* u*128 */, size_t u, blsbn254_g2prepared** out);
void blsbn254_g2prepared_destroy(blsbn254_g2prepared* keys);
size_t blsbn254_g2prepared_count(const blsbn254_g2prepared* keys);
int blsbn254_g2prepared_valid(blsbn254_ctx* ctx, const blsbn254_g2prepared* keys, uint8_t* ok_bitmap /* ceil(u/8) */);
int blsbn254_verify_batch_prepared(blsbn254_ctx* ctx, const blsbn254_g2prepared* keys, const uint32_t* key_idx,
                                   const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, size_t n,
                                   const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap);
/* multi_miller_loop(&[(&G1Affine, &G2Prepared)]) -> MillerLoopResult (pairings.rs:808-857) with the second members given as
 * prepared keys by index: the 384-byte product of the n Miller values (same bytes as blsbn254_multi_miller_loop on the
 * plain points).  A pair whose G1 member is the identity is skipped, as in the reference; a G1 that does not decode
 * returns BLSBN254_ERR_G1, a referenced key that is not a valid G2 point returns BLSBN254_ERR_G2. */
int blsbn254_multi_miller_loop_prepared(blsbn254_ctx* ctx, const blsbn254_g2prepared* keys, const uint32_t* key_idx,
                                        const uint8_t* g1 /* n*64 */, size_t n, uint8_t ml_out[384]);
/* blsbn254_aggregate_verify with the public keys named by index into a prepared table: only 4 bytes per pair cross the
 * boundary instead of 128, and no key is validated or turned into lines again.  Same preconditions as aggregate_verify. */
int blsbn254_aggregate_verify_prepared(blsbn254_ctx* ctx, const blsbn254_g2prepared* keys, const uint32_t* key_idx,
                                       const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t agg_sig[64],
                                       const uint8_t* dst, size_t dst_len, int* valid);
/* The same check split for sharding over GPUs: every rank reduces ITS (pk_i, msg_i) to one
 * Fp12 partial product prod_i ML(H(msg_i), pk_i) (384 B; n = 0 gives Fp12::ONE) and reports whether all its
 * public keys validated; the partials are exchanged (all-gather of 384-byte records, Fp12 multiplication is
 * not an RCCL reduce op) and any rank finishes: valid = FE(prod partials * ML(agg_sig, -G2gen)) == 1. */
int blsbn254_aggregate_partial(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                               const uint8_t* dst, size_t dst_len, uint8_t ml_out[384], int* all_pks_ok);
int blsbn254_aggregate_finish(blsbn254_ctx* ctx, const uint8_t* partials /* k*384 */, size_t k, const uint8_t agg_sig[64], int* valid);
/* One shard may carry the aggregate signature's pair as well: its partial is then prod_i ML(H(msg_i), pk_i) * ML(agg_sig, -G2gen)
 * (the signature joins the batch as one more pair instead of a one-lane launch of its own), *sig_ok = the signature decodes,
 * is not the identity and is on the curve, and blsbn254_aggregate_finish is called with agg_sig = NULL. */
int blsbn254_aggregate_partial_with_sig(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                                        const uint8_t* dst, size_t dst_len, const uint8_t agg_sig[64], uint8_t ml_out[384],
                                        int* all_pks_ok, int* sig_ok);
/* Same result as blsbn254_verify_batch (same bitmap), computed with random linear combinations (SURVEY.md 8f rank 4;
 * bilinearity as in Gt::mul_by_scalar pairings.rs:585-600, multi_miller_loop over prepared keys pairings.rs:808-857).
 *
 * Batches that repeat keys (at most half as many distinct keys as tuples -- the same rule as verify_batch's prepared-key
 * path): every run of one key, in key-sorted order, is cut into chunks of at most G tuples (default 16,
 * blsbn254_set_rlc_group / BLSBN254_RLC_GROUP), and a chunk C with key pk is checked as ONE virtual tuple
 *   e(sum_{i in C} r_i sig_i, -G2gen) * e(sum_{i in C} r_i H(msg_i), pk) == 1
 * on the prepared-key verify path: 1/G as many Miller loops and final exponentiations.  The eligible tuples of a chunk that
 * fails are re-verified one by one on the exact prepared-key path, so a bit can only differ from verify_batch's when an
 * invalid chunk passes: probability about 2^-64 per chunk for a seed the adversary cannot predict.  Tuples whose
 * signature does not decode / is the identity / is off the curve, or whose key fails its checks, are reported invalid
 * directly and contribute to no sum.
 * Weights: r_i = a_i + b_i lambda (lambda = eigenvalue of the G1 endomorphism (x, y) -> (beta x, y)), with the 32-bit
 * a_i, b_i taken from SHA-256(seed || i || pk_i || sig_i || H(msg_i)); the 2^64 pairs give 2^64 distinct weights mod r.
 * Batches of distinct keys: groups of 16 tuples in the caller's order share the signature-side Miller loop and the final
 * exponentiation (host-pointer entry point; 64-bit weights), or take the exact path (device entry point).
 * seed = NULL (the production setting): the library draws 32 bytes from the OS (getrandom) inside the call, i.e. after
 * the batch is fixed.  A caller-supplied seed exists for reproducible tests; soundness then rests on that seed being
 * fresh and secret -- never reuse one, never derive it from public data. */
int blsbn254_verify_batch_rlc(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                              const uint8_t* sigs, size_t n, const uint8_t* dst, size_t dst_len,
                              const uint8_t seed[32], uint8_t* valid_bitmap);
/* The same with every buffer device-resident (the layout of blsbn254_verify_batch_dev); seed and dst are host pointers. */
int blsbn254_verify_batch_rlc_dev(blsbn254_ctx* ctx, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                                  const uint8_t* d_sigs, size_t n, const uint8_t* dst, size_t dst_len,
                                  const uint8_t seed[32], uint8_t* d_valid_bitmap);
/* tuples per chunk of the repeated-key variant: 2 <= group <= 4096 fixes it; 0 = automatic (the default): 16, raised to at
 * most 32 when the larger chunk saves a whole round of waves on the device (chunk count just above a multiple of CUs x 256) */
int blsbn254_set_rlc_group(blsbn254_ctx* ctx, size_t group);
/* The key round (on by default; BLSBN254_RLC_KEY_ROUND=0 or blsbn254_set_rlc_key_round(ctx, 0) skips it): before any chunk is
 * checked, ALL tuples of every key are checked as one virtual tuple per key -- u checks, run with one workgroup (two waves) per check.  A batch
 * without invalid signatures, the usual case, is decided there (262144 tuples over 1024 keys: 9.5 instead of 16.3 ms); if any key
 * fails, only the chunks of the failed keys are checked as described above (the key round then cost about 5 ms extra; a caller
 * whose batches keep failing it does not keep paying: after a failure the next 2, then 4, 8, 16 batches skip it, a pass resets
 * the back-off, and so does this call).  Same weights, same error bound. */
int blsbn254_set_rlc_key_round(blsbn254_ctx* ctx, int on);
/* counters since context creation: out[0] tuples on the repeated-key path, out[1] chunks checked, out[2] tuples re-verified
 * exactly after their chunk failed, out[3] tuples of distinct-key batches (no chunks), out[4] key rounds run, out[5] key rounds
 * that decided their batch (no chunk was checked) */
int blsbn254_rlc_stats(blsbn254_ctx* ctx, uint64_t out[6]);
/* impl Sum for G1Projective, g1.rs:561-565 */
int blsbn254_aggregate_sigs(blsbn254_ctx* ctx, const uint8_t* sigs, size_t n, uint8_t out[64]);
/* impl Sum for G2Projective, g2.rs:579-583: out = pk_0 + ... + pk_(n-1) (uncompressed; the identity encoding for n == 0).
 * Every point must decode and lie on the curve (else BLSBN254_ERR_G2); subgroup membership is not required of the terms
 * (the reference's Sum adds whatever G2Projective values it is given). */
int blsbn254_aggregate_pks(blsbn254_ctx* ctx, const uint8_t* pks /* n*128 */, size_t n, uint8_t out[128]);
/* IETF FastAggregateVerify, min-sig variant (build-defined composition, SURVEY.md 1: the reference has no BLS layer): ONE message
 * signed by n keys, e(sig, -G2gen) * e(H(msg), pk_0 + ... + pk_(n-1)) == 1 -- the sum by Sum for G2Projective (g2.rs:579-583),
 * then the CoreVerify of blsbn254_verify_batch on it (G1Projective::hash g1.rs:910-919, pairing pairings.rs:760-802), including
 * its KeyValidate on the SUM (not the identity, in the r-torsion).  As in the IETF procedure the individual keys are only
 * required to be curve points -- proof of possession (blsbn254_pop_verify_batch) is the caller's precondition; a key that
 * does not decode or is off the curve makes the result invalid, n == 0 likewise.  *valid = 0 / 1. */
int blsbn254_fast_aggregate_verify(blsbn254_ctx* ctx, const uint8_t* pks /* n*128 */, size_t n, const uint8_t* msg, size_t msg_len,
                                   const uint8_t sig[64], const uint8_t* dst, size_t dst_len, int* valid);
/* The same for n_groups independent (key set, message, signature) groups in one call -- the validator workload (thousands of
 * aggregates, each signed by hundreds of keys): group g owns the keys pks[128 * key_off[g] .. 128 * key_off[g + 1]) (key_off:
 * n_groups + 1 non-decreasing element offsets, host array), the message msgs[off[g] .. off[g + 1]) and sigs[64 g ..].  The
 * key sums run as segmented sums on the device (one lane per 16-point chunk, level by level), the n_groups sums then go
 * through the verify_batch pipeline.  Bit g of valid_bitmap (LSB-first) = group g verifies; a group with an undecodable /
 * off-curve key or with no key at all is invalid, never an error. */
int blsbn254_fast_aggregate_verify_batch(blsbn254_ctx* ctx, const uint8_t* pks, const uint64_t* key_off /* n_groups+1 */,
                                         const uint8_t* msgs, const uint64_t* off /* n_groups+1 */, const uint8_t* sigs /* n_groups*64 */,
                                         size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap /* ceil(n_groups/8) */);
/* FastAggregateVerify over a REGISTERED key set, the signers named by bitmaps -- the consumer that holds one committee and
 * receives a participation bitmap with each aggregate.  blsbn254_keyset_create uploads n_keys keys (1 <= n_keys <= 65536), decodes
 * and curve-checks each ONCE (G2Affine::from_uncompressed + is_on_curve, g2.rs:350-414) and keeps them on ctx's GPU with their
 * total; the handle owns its device memory, is tied to ctx, and several may be alive on one context.  A key that does not decode
 * or is off the curve is kept as a BAD key, never an error of the registration.  blsbn254_keyset_valid: KeyValidate per
 * registered key (decodes, not the identity, on the curve, in the r-torsion: is_torsion_free g2.rs:733-736) for the registrar;
 * the sums do not use it.
 * sel = n_groups rows of ceil(n_keys/8) bytes; bit i of a row (LSB-first, as every bitmap here) = key i signed.  A set bit at an
 * index >= n_keys (padding of a row's last byte) is BLSBN254_E_ARG, as are NULL arguments, a key set of another context and
 * n_groups above BLSBN254_CHUNK_LANES (4 Mi); n_groups == 0 returns 0.
 * blsbn254_keyset_sum_batch (impl Sum for G2Projective, g2.rs:579-583): out[128 g ..] = the bytes blsbn254_aggregate_pks gives on
 * the selected keys of row g in index order (the identity encoding for an empty row), status[g] = 1; a row that selects a bad
 * key gets status[g] = 0 and the identity encoding -- never an error of the call.
 * blsbn254_keyset_fast_aggregate_verify_batch: bit g of valid_bitmap = bit g of blsbn254_fast_aggregate_verify_batch on those
 * lists with the same msgs / off / sigs / dst: KeyValidate on the SUM only, a selected bad key makes the group invalid, an
 * identity member changes nothing, an empty row and an identity signature are invalid.
 * One bit per (group, key) crosses the boundary instead of 128 bytes; a lane adds the selected keys of ONE 32-key word with
 * mixed additions (Renes-Costello-Batina Alg 8); a row that selects more than half of the set is summed through its complement,
 * total - sum of the unselected keys, so no row costs more than n_keys/2 additions.  The path never changes a result.
 * blsbn254_keyset_stats, since the context was created: out[0] groups served, out[1] groups summed through the complement,
 * out[2] launches of the word kernel, out[3] key sets created. */
typedef struct blsbn254_keyset blsbn254_keyset;
int blsbn254_keyset_create(blsbn254_ctx* ctx, const uint8_t* pks /* n_keys*128 */, size_t n_keys, blsbn254_keyset** out);
void blsbn254_keyset_destroy(blsbn254_keyset* keys);
size_t blsbn254_keyset_count(const blsbn254_keyset* keys);
int blsbn254_keyset_valid(blsbn254_ctx* ctx, const blsbn254_keyset* keys, uint8_t* ok_bitmap /* ceil(n_keys/8) */);
int blsbn254_keyset_sum_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint8_t* sel, size_t n_groups,
                              uint8_t* out /* n_groups*128 */, uint8_t* status /* n_groups */);
int blsbn254_keyset_fast_aggregate_verify_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint8_t* sel,
                                                const uint8_t* msgs, const uint64_t* off /* n_groups+1 */, const uint8_t* sigs /* n_groups*64 */,
                                                size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_keyset_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* Checked signature aggregation over a registered key set -- what the node calls that collects the committee members' individual
 * signatures on one message and hands on what blsbn254_keyset_fast_aggregate_verify_batch consumes: per message the aggregate
 * signature and the participation bitmap, with the bad signatures left out.  Group g is one message msgs[msg_off[g] ..
 * msg_off[g + 1]) with the signatures received for it, the entries sig_off[g] .. sig_off[g + 1]: entry s says that key idx[s] of
 * the key set signed with sigs[64 s ..].  sig_off / msg_off: n_groups + 1 non-decreasing element / byte offsets, host arrays,
 * which need not start at 0 (idx, sigs and msgs are indexed by them as given); the outputs are indexed from the first group.
 * Inside a group the indices must be STRICTLY INCREASING: no key twice, and one canonical order of a group's entries.
 * BLSBN254_E_ARG (with a last_error text): NULL arguments, a key set of another context, decreasing offsets, n_groups above
 * BLSBN254_CHUNK_LANES (4 Mi), more than 2^23 entries, an idx >= n_keys, indices of a group that do not strictly increase; the
 * outputs are then untouched.  n_groups == 0 returns 0.  A bad entry or group is never an error of the call.
 * An entry is a CANDIDATE when its key has the KeyValidate bit blsbn254_keyset_valid reports (computed once, at registration)
 * and its signature decodes, is on the curve and is not the identity.  Other entries are left out silently: they never fail
 * their group and never cause the fallback.
 * Optimistic attempt, once for all groups of the call (one pass of enqueued work): A_g = the sum of the group's candidate
 * signatures, row_g = the candidates' bits, and the equation of blsbn254_keyset_fast_aggregate_verify_batch on (row_g, msg_g,
 * A_g).  Where it holds: status[g] = 0, out_sigs[64 g ..] = A_g, row g of out_sel (ceil(n_keys/8) bytes) = row_g.  The check is
 * of the SUM: signatures whose errors cancel in it (sigma_a + D, sigma_b - D) are both used, and the aggregate is correct.
 * Fallback, only for the groups that had a candidate and failed the equation (repacked into one sub-call): every candidate is
 * verified as blsbn254_verify_batch verifies (key, msg_g, signature), the entries whose bit is set are kept and summed again,
 * and the same single equation is run once more on the result.  It holds: status 0 with the kept set as the row.  It does not:
 * BLSBN254_ST_SHORT.  That second check exists for the one case per-signature verification does not exclude, kept keys whose
 * sum is the identity (P and -P both registered and both signing): such a group ends in BLSBN254_ST_SHORT, and choosing a
 * subset of it is left to the caller.  A group without entries, without a candidate or without a kept entry is
 * BLSBN254_ST_SHORT too.  A short group's outputs are the identity encoding (0, 1) and an all-zero row.
 * With status 0: blsbn254_keyset_fast_aggregate_verify_batch sets the group's bit for (row of out_sel, msg, out_sigs) under the
 * same dst, and out_sigs is byte-identical to blsbn254_aggregate_sigs on the selected entries' signatures.  A group's outcome
 * depends on its own inputs only: not on the attempt that served it, on launch boundaries or on its neighbours.  Pending
 * asynchronous verify calls are settled on entry and none is left pending.  The groups of this call are not counted by
 * blsbn254_keyset_stats (its launches of the word kernel neither); blsbn254_keyset_aggregate_stats, since the context was
 * created: out[0] groups settled by the optimistic attempt, out[1] groups sent to the fallback, out[2] signatures verified
 * individually, out[3] groups ending in BLSBN254_ST_SHORT. */
int blsbn254_keyset_aggregate_checked_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint32_t* idx /* N */, const uint8_t* sigs /* N*64 */, const uint64_t* sig_off /* n_groups+1 */,
        const uint8_t* msgs, const uint64_t* msg_off /* n_groups+1, bytes */, size_t n_groups,
        const uint8_t* dst, size_t dst_len,
        uint8_t* out_sigs /* n_groups*64 */, uint8_t* out_sel /* n_groups*ceil(n_keys/8) */, uint8_t* status /* n_groups */);
int blsbn254_keyset_aggregate_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* Checked merge of partial aggregates over a registered key set -- what an intermediate node of an aggregation tree calls: it
 * receives PARTIAL AGGREGATES for one message, each an aggregate signature with the bitmap of the keys that are in it, and hands
 * on one merged (aggregate, bitmap) pair without the bad contributions.  Group g is one message msgs[msg_off[g] .. msg_off[g + 1])
 * with the contributions con_off[g] .. con_off[g + 1]: contribution s is the row rows[s * ceil(n_keys/8) ..] (bit i = key i is in
 * it, LSB-first, as a row of sel) and the signature sigs[64 s ..].  con_off / msg_off: n_groups + 1 non-decreasing element / byte
 * offsets, host arrays, which need not start at 0 (rows, sigs and msgs are indexed by them as given); the outputs and the bits
 * of `used` are indexed from the first group and the first contribution of the call.
 * BLSBN254_E_ARG (with a last_error text): NULL arguments, a key set of another context, decreasing offsets, n_groups above
 * BLSBN254_CHUNK_LANES (4 Mi), more than 2^23 contributions, more than 2^30 bytes of rows, a row that sets a bit at an index
 * >= n_keys; the outputs are then untouched and nothing was enqueued.  n_groups == 0 returns 0.  A bad contribution or group is
 * never an error of the call.
 * A contribution is a CANDIDATE when its signature decodes, is on the curve and is not the identity, its row is not empty, and
 * every key its row selects has the KeyValidate bit blsbn254_keyset_valid reports (so a merged key sum is always in the
 * r-torsion).  SELECTION is greedy, in the order given: a contribution is selected when it is a candidate and its row is disjoint
 * from the union of the rows selected before it in its group.  The caller sets the priority by the order.  Everything else --
 * overlapping contributions, duplicates, non-candidates -- is left out silently: it never fails its group and never causes the
 * fallback.
 * Optimistic attempt, once for all groups of the call (one pass of enqueued work): A_g = the sum of the selected signatures,
 * row_g = the OR of the selected rows, and the equation of blsbn254_keyset_fast_aggregate_verify_batch on (row_g, msg_g, A_g).
 * Where it holds: status[g] = 0, out_sigs[64 g ..] = A_g, row g of out_sel = row_g, and the bits of the selected contributions
 * in `used`.  The check is of the SUM: contributions whose errors cancel in it (sigma_a + D, sigma_b - D) are both used, and the
 * aggregate is correct.
 * Fallback, only for the groups that selected something and failed the equation (repacked into one sub-call): EVERY candidate
 * of the group, not only the selected ones, is verified on its own by the same equation on (its row, msg_g, its signature); then
 * the same selection runs again with those bits as its mask -- once a bad contribution is gone, a later one that overlapped it
 * becomes admissible -- and the one equation decides again: status 0 with the new selection, or BLSBN254_ST_SHORT.  The second
 * check exists for kept rows whose keys sum to the identity (P and -P both registered).  A group without contributions, without a
 * candidate or with nothing kept is BLSBN254_ST_SHORT too.  A short group's outputs are the identity encoding (0, 1), an all-zero
 * row and no bit of `used`.
 * With status 0: blsbn254_keyset_fast_aggregate_verify_batch sets the group's bit for (row of out_sel, msg, out_sigs) under the
 * same dst, out_sigs is byte-identical to blsbn254_aggregate_sigs on the used signatures in order, and the row of out_sel is the
 * OR of the used rows.  A group's outcome depends on its own inputs only: not on the attempt that served it, on launch
 * boundaries or on its neighbours.  Pending asynchronous verify calls are settled on entry and none is left pending.  The groups
 * of this call count in neither blsbn254_keyset_stats nor blsbn254_keyset_aggregate_stats; blsbn254_keyset_merge_stats, since the
 * context was created: out[0] groups settled by the optimistic attempt, out[1] groups sent to the fallback, out[2] contributions
 * verified individually, out[3] groups ending in BLSBN254_ST_SHORT. */
int blsbn254_keyset_merge_checked_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint8_t* rows /* N*ceil(n_keys/8) */, const uint8_t* sigs /* N*64 */, const uint64_t* con_off /* n_groups+1 */,
        const uint8_t* msgs, const uint64_t* msg_off /* n_groups+1, bytes */, size_t n_groups,
        const uint8_t* dst, size_t dst_len,
        uint8_t* out_sigs /* n_groups*64 */, uint8_t* out_sel /* n_groups*ceil(n_keys/8) */,
        uint8_t* used /* ceil(N/8), bit s = contribution s of the call, LSB-first */, uint8_t* status /* n_groups */);
int blsbn254_keyset_merge_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* A key set registered WITH proofs of possession, stake weights on the handle, and FastAggregateVerify with a quorum -- what a
 * proof-of-stake verifier decides is not "does this aggregate verify" but "does a verifying aggregate carry the quorum's stake".
 * blsbn254_keyset_create_checked: blsbn254_keyset_create with one proof per key, proof i checked exactly as
 * blsbn254_pop_verify_batch checks (pk_i, proof_i) under pop_dst.  A key whose proof fails becomes a BAD key of the handle, in
 * every respect like a key that does not decode: its blsbn254_keyset_valid bit is 0, it is left out of the total, a row that
 * selects it gets status 0 from blsbn254_keyset_sum_batch and is invalid in blsbn254_keyset_fast_aggregate_verify_batch, and it
 * is never a candidate of the checked aggregation or merge.  A failing proof is never an error of the registration.  Argument
 * errors: those of blsbn254_keyset_create, and NULL proofs (or a NULL pop_dst with pop_dst_len > 0).  blsbn254_keyset_checked:
 * 1 for a handle created with proofs, else 0.  With proofs that all hold, every call on the handle gives the bytes it gives on
 * the handle blsbn254_keyset_create makes of the same keys.
 * blsbn254_keyset_set_weights: n_cols (1 .. BLSBN254_KS_MAX_COLS) stake columns, weights[q * n_keys + i] = column q of key i,
 * one column per quorum.  Calling again replaces the table (a stake change per epoch needs no new registration).  A column whose
 * sum over ALL n_keys entries does not fit 64 bits is BLSBN254_E_ARG with a last_error text, and nothing is changed: no later
 * sum can overflow.  The EFFECTIVE weight of a key without the blsbn254_keyset_valid bit is 0 (applied on the device, from the bits):
 * an identity key changes no key sum, so under plain arithmetic it could be selected in a verifying aggregate and lend it its
 * stake.  blsbn254_keyset_total_weight: the columns' sums of the effective weights.  A handle without a table has no columns:
 * blsbn254_keyset_total_weight and the two calls below return BLSBN254_E_ARG for it.
 * blsbn254_keyset_weight_batch: rows and argument checks as blsbn254_keyset_sum_batch; out[g * n_cols + q] = the sum of the
 * effective weights of column q over the set bits of row g, exact; an empty row gives 0.  One wave per row on the device.  The
 * rows blsbn254_keyset_aggregate_checked_batch / blsbn254_keyset_merge_checked_batch hand out in out_sel are rows of this call.
 * blsbn254_keyset_quorum_verify_batch: the arguments of blsbn254_keyset_fast_aggregate_verify_batch and ONE rule per call,
 * min_weight[q] per column.  Group g REACHES QUORUM when weights_out[g * n_cols + q] >= min_weight[q] for every column (a
 * minimum of 0 switches a column off).  Bit g of valid_bitmap is set when the group reaches quorum AND bit g of
 * blsbn254_keyset_fast_aggregate_verify_batch on the same inputs is set.  weights_out = what blsbn254_keyset_weight_batch
 * gives, always filled for every group: the caller reads the reason for a 0 bit from it.  The weights are computed and read
 * back FIRST (one small synchronisation); only the groups that reach quorum are then summed and paired, repacked by the host
 * into one sub-call where some do not; where none does, nothing more is launched.  A group's outcome depends on its own inputs
 * only.  Argument errors as blsbn254_keyset_fast_aggregate_verify_batch, plus NULL min_weight / weights_out, decreasing message
 * offsets and a handle without a table.  Pending asynchronous verify calls are settled on entry.  blsbn254_keyset_stats counts
 * only the groups that were summed.  blsbn254_keyset_weight_stats, since the context was created: out[0] groups weighed (by the
 * two calls), out[1] groups below quorum (not summed, not paired), out[2] launches of the weight kernel for them, out[3] tables
 * set. */
#define BLSBN254_KS_MAX_COLS 8
int blsbn254_keyset_create_checked(blsbn254_ctx* ctx, const uint8_t* pks /* n_keys*128 */, const uint8_t* proofs /* n_keys*64 */,
                                   size_t n_keys, const uint8_t* pop_dst, size_t pop_dst_len, blsbn254_keyset** out);
int blsbn254_keyset_checked(const blsbn254_keyset* keys);
int blsbn254_keyset_set_weights(blsbn254_ctx* ctx, blsbn254_keyset* keys, const uint64_t* weights /* n_cols*n_keys */, size_t n_cols);
int blsbn254_keyset_total_weight(blsbn254_ctx* ctx, const blsbn254_keyset* keys, uint64_t* out /* n_cols */);
int blsbn254_keyset_weight_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint8_t* sel, size_t n_groups,
                                 uint64_t* out /* n_groups*n_cols */);
int blsbn254_keyset_quorum_verify_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint8_t* sel,
        const uint8_t* msgs, const uint64_t* off /* n_groups+1 */, const uint8_t* sigs /* n_groups*64 */, size_t n_groups,
        const uint8_t* dst, size_t dst_len, const uint64_t* min_weight /* n_cols */,
        uint64_t* weights_out /* n_groups*n_cols */, uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_keyset_weight_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* COMMITTEES over a registered key set: a node holds ONE registry of keys, and each aggregate it receives is signed by a subset
 * of one committee -- a list of registry indices -- with participation bits that count positions in that list.
 * blsbn254_keyset_set_committees registers n_com (1 .. 65536) committees on the handle: committee c is
 * members[com_off[c] .. com_off[c+1]), indices into the key set.  Every committee has at least one member, com_off starts at 0
 * and does not decrease, com_off[n_com] = M <= 4 Mi (the default BLSBN254_CHUNK_LANES), every index is < n_keys, and no index
 * appears twice within one committee; committees may overlap one another freely.  A violation is BLSBN254_E_ARG with a last_error
 * that names the committee, and the handle keeps the table it had.  Calling again replaces the table.  A committee may contain
 * bad keys, identity keys and keys whose proof failed: they behave as in the full-width calls.  blsbn254_keyset_committee_count:
 * the committees of the handle, 0 before the first successful blsbn254_keyset_set_committees.
 * The three calls below take n_groups RAGGED groups: group g names committee com[g] and brings row
 * sel[sel_off[g] .. sel_off[g+1]) of exactly ceil(size(com[g]) / 8) bytes, bit j (LSB-first) = member j of the committee signed.
 * BLSBN254_E_ARG: a wrong row length, a set bit past the committee's last member, com[g] >= n_com, a handle without a table,
 * n_groups above BLSBN254_CHUNK_LANES; n_groups == 0 returns 0.  Each gives EXACTLY what its full-width counterpart gives for the
 * row with bit members[j] set for every set bit j:
 * blsbn254_keyset_committee_sum_batch: out / status of blsbn254_keyset_sum_batch (the identity encoding and status 0 for a row that
 * selects a bad key).  blsbn254_keyset_committee_fast_aggregate_verify_batch: the bits of
 * blsbn254_keyset_fast_aggregate_verify_batch.  blsbn254_keyset_committee_weight_batch: out of blsbn254_keyset_weight_batch
 * (effective weights: a key without the validity bit weighs 0); BLSBN254_E_ARG without a stake table.
 * A group in which more than half of its COMMITTEE signed is summed through the complement against the committee's total (kept
 * on the handle).  Pending asynchronous verify calls are settled on entry.  blsbn254_keyset_stats does not count these calls;
 * blsbn254_keyset_committee_stats, since the context was created: out[0] groups served, out[1] groups summed through the
 * complement, out[2] launches of the word kernel, out[3] committee tables set. */
int blsbn254_keyset_set_committees(blsbn254_ctx* ctx, blsbn254_keyset* keys, const uint32_t* members /* M */,
                                   const uint64_t* com_off /* n_com+1 */, size_t n_com);
size_t blsbn254_keyset_committee_count(const blsbn254_keyset* keys);
int blsbn254_keyset_committee_sum_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint32_t* com /* n_groups */,
        const uint8_t* sel, const uint64_t* sel_off /* n_groups+1, bytes */, size_t n_groups, uint8_t* out /* n_groups*128 */,
        uint8_t* status /* n_groups */);
int blsbn254_keyset_committee_fast_aggregate_verify_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint32_t* com /* n_groups */, const uint8_t* sel, const uint64_t* sel_off /* n_groups+1, bytes */,
        const uint8_t* msgs, const uint64_t* off /* n_groups+1 */, const uint8_t* sigs /* n_groups*64 */, size_t n_groups,
        const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_keyset_committee_weight_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint32_t* com /* n_groups */,
        const uint8_t* sel, const uint64_t* sel_off /* n_groups+1, bytes */, size_t n_groups, uint64_t* out /* n_groups*n_cols */);
int blsbn254_keyset_committee_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* Checked signature aggregation PER COMMITTEE of a registered key set -- blsbn254_keyset_aggregate_checked_batch for the collector
 * whose signatures arrive per committee: nothing in the call is as wide as the registry.  Group g is committee com[g] of the
 * handle's table (blsbn254_keyset_set_committees), one message msgs[msg_off[g] .. msg_off[g + 1]) and the entries sig_off[g] ..
 * sig_off[g + 1]: entry s says that member pos[s] of the committee signed with sigs[64 s ..].  pos[s] is a POSITION in the
 * committee's member list, not a registry index; inside a group the positions must be STRICTLY INCREASING.  sig_off / msg_off /
 * sel_off: n_groups + 1 non-decreasing element / byte / byte offsets, host arrays, which need not start at 0 (pos, sigs and msgs
 * are indexed by them as given; out_sigs and status are indexed from the first group).  sel_off is an INPUT: row g of out_sel is
 * written at out_sel + (sel_off[g] - sel_off[0]) and must be exactly ceil(size(com[g]) / 8) bytes long, the row rule of the three
 * read-side committee calls -- so (com, out_sel, sel_off) go unchanged to blsbn254_keyset_committee_fast_aggregate_verify_batch or
 * its _rlc form.  Bit j of a row = member j of the committee is in the aggregate.
 * For every group out_sigs[64 g ..] and status[g] are byte for byte what blsbn254_keyset_aggregate_checked_batch returns for the
 * same group with every entry translated to idx = members[com_off[com[g]] + pos] (and the entries re-sorted by idx: members may be
 * listed in any order, and the aggregate's affine encoding does not depend on the order of addition), and bit j of the row is set
 * exactly when bit members[com_off[com[g]] + j] of that call's row is.  Everything said there carries over: the candidate rule
 * (the key has the KeyValidate bit, the signature decodes, is on the curve and is not the identity), entries left out silently,
 * the one optimistic equation per group, the fallback that verifies every candidate of a failing group and runs the one equation
 * again, BLSBN254_ST_SHORT with the identity encoding and a zero row (P and -P both signing included), cancelling errors that
 * are both used, a group's outcome depending on its own inputs only, pending asynchronous verifies settled on entry.
 * BLSBN254_E_ARG (with a last_error text; the outputs are untouched and nothing was enqueued): NULL arguments, a key set of
 * another context, a handle without a committee table, com[g] >= n_com, pos[s] >= size(com[g]) (the text names the entry),
 * positions of a group that do not strictly increase (the text names the group), decreasing offsets, a row length other than
 * ceil(size / 8), more than 2^23 entries, n_groups above BLSBN254_CHUNK_LANES.  n_groups == 0 returns 0.
 * The groups of this call count in none of blsbn254_keyset_stats, blsbn254_keyset_aggregate_stats and
 * blsbn254_keyset_committee_stats; blsbn254_keyset_committee_aggregate_stats, since the context was created: out[0] groups settled
 * by the optimistic attempt, out[1] groups sent to the fallback, out[2] signatures verified individually, out[3] groups ending in
 * BLSBN254_ST_SHORT. */
int blsbn254_keyset_committee_aggregate_checked_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint32_t* com /* n_groups */,
        const uint32_t* pos /* N */, const uint8_t* sigs /* N*64 */, const uint64_t* sig_off /* n_groups+1 */,
        const uint8_t* msgs, const uint64_t* msg_off /* n_groups+1, bytes */,
        const uint64_t* sel_off /* n_groups+1, bytes */, size_t n_groups,
        const uint8_t* dst, size_t dst_len,
        uint8_t* out_sigs /* n_groups*64 */, uint8_t* out_sel /* sel_off[n_groups]-sel_off[0] */, uint8_t* status /* n_groups */);
int blsbn254_keyset_committee_aggregate_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* Checked merge of partial aggregates PER COMMITTEE of a registered key set -- blsbn254_keyset_merge_checked_batch for the
 * intermediate node whose partial aggregates arrive per committee: nothing in the call is as wide as the registry.  Group g is
 * committee com[g] of the handle's table (blsbn254_keyset_set_committees), one message msgs[msg_off[g] .. msg_off[g + 1]) and the
 * contributions con_off[g] .. con_off[g + 1]: contribution s brings the signature sigs[64 s ..] and a row of exactly
 * rb_g = ceil(size(com[g]) / 8) bytes, bit j (LSB-first) = member j of the committee is in the contribution.  The rows of a
 * group lie back to back from rows + row_off[g], in contribution order: row_off[g + 1] - row_off[g] must equal
 * (con_off[g + 1] - con_off[g]) * rb_g.  con_off / row_off / msg_off / sel_off: n_groups + 1 non-decreasing element / byte /
 * byte / byte offsets, host arrays, none of which needs to start at 0 (rows, sigs and msgs are indexed by them as given);
 * out_sigs and status are indexed from the first group of the call, the bits of `used` from its first contribution.  sel_off
 * is an INPUT, exactly as in blsbn254_keyset_committee_aggregate_checked_batch: row g of out_sel is written at
 * out_sel + (sel_off[g] - sel_off[0]) and is rb_g bytes long -- so the outputs of that call from several collectors,
 * concatenated, are the input of this one, and (com, out_sel, sel_off) go unchanged to
 * blsbn254_keyset_committee_fast_aggregate_verify_batch, its _rlc form and blsbn254_keyset_committee_weight_batch.
 * The call behaves as blsbn254_keyset_merge_checked_batch on the same handle with every contribution row replaced by its
 * SCATTERED row, the row with bit members[com_off[com[g]] + j] set for every set bit j (members of one committee are distinct:
 * disjoint in positions is disjoint in registry indices, and the greedy selection is the same): out_sigs[64 g ..] and status[g]
 * are byte for byte what that call returns, the bits of `used` are the same bits, and bit j of the row of out_sel is set exactly
 * when bit members[com_off[com[g]] + j] of that call's row is.  Everything said there carries over: the candidate rule (the
 * signature decodes, is on the curve and is not the identity, the row is not empty, every selected key has the KeyValidate
 * bit), greedy selection in the order given, what is left out silently, the one optimistic equation per group, the fallback
 * that verifies EVERY candidate of a failing group on its own and then selects again with those bits as the mask,
 * BLSBN254_ST_SHORT with the identity encoding, a zero row and no bit of `used` (kept keys that sum to the identity included),
 * cancelling errors that are both used, a group's outcome depending on its own inputs only, pending asynchronous verifies
 * settled on entry.
 * BLSBN254_E_ARG (with a last_error text; the outputs are untouched and nothing was enqueued): NULL arguments, a key set of
 * another context, a handle without a committee table, com[g] >= n_com (the text names the group), a row_off span that is not
 * count * rb_g or a sel_off span that is not rb_g (the text names the group), a row that sets a bit past the committee's last
 * member (the text names the contribution, counted from the first of the call), decreasing offsets in any of the four arrays,
 * more than 2^23 contributions, more than 2^30 bytes of rows, n_groups above BLSBN254_CHUNK_LANES.  n_groups == 0 returns 0.
 * The groups of this call count in none of the other stats calls; blsbn254_keyset_committee_merge_stats, since the context was
 * created: out[0] groups settled by the optimistic attempt, out[1] groups sent to the fallback, out[2] contributions verified
 * individually, out[3] groups ending in BLSBN254_ST_SHORT. */
int blsbn254_keyset_committee_merge_checked_batch(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint32_t* com /* n_groups */,
        const uint8_t* rows, const uint64_t* row_off /* n_groups+1, bytes */,
        const uint8_t* sigs /* N*64 */, const uint64_t* con_off /* n_groups+1 */,
        const uint8_t* msgs, const uint64_t* msg_off /* n_groups+1, bytes */,
        const uint64_t* sel_off /* n_groups+1, bytes */, size_t n_groups,
        const uint8_t* dst, size_t dst_len,
        uint8_t* out_sigs /* n_groups*64 */, uint8_t* out_sel /* sel_off[n_groups]-sel_off[0] */,
        uint8_t* used /* ceil(N/8) */, uint8_t* status /* n_groups */);
int blsbn254_keyset_committee_merge_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* blsbn254_keyset_fast_aggregate_verify_batch and blsbn254_keyset_committee_fast_aggregate_verify_batch by RANDOM LINEAR
 * COMBINATION PER MESSAGE: the same arguments plus a seed, the same bitmap.  The groups of a call whose messages are
 * byte-identical form a class; a class, in the caller's order, is cut into chunks of at most C groups (default 64,
 * blsbn254_set_keyset_rlc_group: 2 <= group <= 4096 fixes it, 0 restores the default, anything else is BLSBN254_E_ARG), and a
 * chunk with message m, key sums S_g and signatures sig_g is checked as ONE virtual tuple
 *   e(sum_g r_g sig_g, -G2gen) * e(H(m), sum_g r_g S_g) == 1
 * on the verify pipeline: 1/C as many Miller loops and final exponentiations where aggregates share their message.
 * A group takes part in its chunk's sums only when it is ELIGIBLE: its row selects no bad key, every key it adds has the
 * KeyValidate bit (so its sum lies in the r-torsion without a test of its own), its signature decodes, is on the curve and is
 * not the identity, and its sum is not the identity.  An eligible group of a chunk that passes has its bit set.  Every other
 * group -- not eligible, alone in its chunk or the only eligible member of it, in a chunk whose weighted sum is the identity, or
 * an eligible member of a chunk that FAILED -- is decided by the exact call's own pipeline on its sum, in one sub-call.  So bit g
 * is bit g of the exact call on the same arguments, and can differ only where an invalid group passed its chunk's check:
 * probability at most 2^-64 per chunk checked, given a fresh secret seed.
 * Weights: r_g = the first 8 bytes, big-endian, of SHA-256(seed || "KSRLC" || g as 8 bytes little-endian || sig_g); 0 becomes 1.
 * seed = NULL (the production setting): the library draws 32 bytes from the OS (getrandom) inside the call, i.e. after
 * the batch is fixed.  A caller-supplied seed exists for reproducible tests; soundness then rests on that seed being
 * fresh and secret -- never reuse one, never derive it from public data.
 * Argument errors and n_groups == 0 behave as in the exact calls (the offsets of the messages are checked before anything is
 * launched; msgs == NULL with a message of non-zero length is BLSBN254_E_ARG).  Pending asynchronous verify calls are settled
 * on entry and none is left pending.  blsbn254_keyset_stats / blsbn254_keyset_committee_stats count the sums as they do for
 * the exact calls.  blsbn254_keyset_rlc_stats, since the context was created: out[0] groups decided by a chunk that passed,
 * out[1] chunks checked, out[2] groups sent to the exact path because their chunk failed, out[3] groups sent there directly
 * (not eligible, or in a chunk that was not checked), out[4] message classes seen, out[5] calls. */
int blsbn254_keyset_fast_aggregate_verify_batch_rlc(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint8_t* sel /* n_groups*ceil(n_keys/8) */, const uint8_t* msgs, const uint64_t* off /* n_groups+1 */,
        const uint8_t* sigs /* n_groups*64 */, size_t n_groups, const uint8_t* dst, size_t dst_len,
        const uint8_t seed[32] /* NULL: getrandom inside the call */, uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_keyset_committee_fast_aggregate_verify_batch_rlc(blsbn254_ctx* ctx, const blsbn254_keyset* keys,
        const uint32_t* com /* n_groups */, const uint8_t* sel, const uint64_t* sel_off /* n_groups+1, bytes */,
        const uint8_t* msgs, const uint64_t* off /* n_groups+1 */, const uint8_t* sigs /* n_groups*64 */, size_t n_groups,
        const uint8_t* dst, size_t dst_len, const uint8_t seed[32] /* NULL: getrandom inside the call */,
        uint8_t* valid_bitmap /* ceil(n_groups/8) */);
int blsbn254_set_keyset_rlc_group(blsbn254_ctx* ctx, size_t group);
int blsbn254_keyset_rlc_stats(blsbn254_ctx* ctx, uint64_t out[6]);
/* Mul<Scalar> for G1Projective (g1.rs:518-534, multiply :821-841) and G2Projective (g2.rs:866-886), element-wise:
 * out_i = [k_i] P_i.  Points uncompressed, scalars 32 bytes big-endian (scalar.rs:229-233) and < r.  A point that does not
 * decode or is off the curve returns BLSBN254_ERR_G1 / BLSBN254_ERR_G2, a scalar >= r BLSBN254_ERR_SCALAR (the reference's
 * types make both unrepresentable); the identity and k = 0 give the identity.  Same point as the reference's 255-step
 * double-and-add, computed with 4-bit windows over the complete RCB formulas.  Not constant time. */
int blsbn254_g1_mul_batch(blsbn254_ctx* ctx, const uint8_t* g1 /* n*64 */, const uint8_t* scalars /* n*32 */, size_t n, uint8_t* out /* n*64 */);
int blsbn254_g2_mul_batch(blsbn254_ctx* ctx, const uint8_t* g2 /* n*128 */, const uint8_t* scalars /* n*32 */, size_t n, uint8_t* out /* n*128 */);
/* out = sum_i [k_i] P_i  (LinearCombination for G1Projective g1.rs:559 / G2Projective g2.rs:577, n-term form;
 * = Mul<Scalar> g1.rs:518-534 + Sum g1.rs:561-565).  Points uncompressed, scalars 32 B big-endian < r.  Errors as
 * blsbn254_g1_mul_batch: a point that does not decode or is off the curve -> BLSBN254_ERR_G1 / _G2 (the first such
 * index in last_error), a scalar >= r -> BLSBN254_ERR_SCALAR.  n == 0 -> the identity encoding.  n <= 2^23 per call
 * (BLSBN254_E_ARG beyond).  G2 points need not lie in the r-torsion: the result is the integer combination.
 * Bucket (Pippenger) method: G1 over the GLV halves, G2 over the full scalar; signed c-bit windows. */
int blsbn254_g1_msm(blsbn254_ctx* ctx, const uint8_t* g1 /* n*64 */, const uint8_t* scalars /* n*32 */, size_t n, uint8_t out[64]);
int blsbn254_g2_msm(blsbn254_ctx* ctx, const uint8_t* g2 /* n*128 */, const uint8_t* scalars /* n*32 */, size_t n, uint8_t out[128]);
/* window width of the bucket method: 0 = chosen from n (default), 2..16 = forced (tests, tuning); else BLSBN254_E_ARG */
int blsbn254_set_msm_window(blsbn254_ctx* ctx, int c);
/* since context creation: out[0] calls on the bucket path, out[1] calls on the small-n path, out[2] bucket entries
 * accumulated, out[3] chunks of bucket entries summed */
int blsbn254_msm_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* sum_i lambda_i * sig_i with Lagrange coefficients at 0 for the t distinct non-zero ids
 * (Mul<Scalar> g1.rs:518-534 + Sum; Fr arithmetic scalar.rs:523-548) */
int blsbn254_threshold_combine(blsbn254_ctx* ctx, const uint8_t* ids, const uint8_t* partial_sigs, size_t t, uint8_t out_sig[64]);
/* The Lagrange coefficients alone: out[i] = prod_{j != i} x_j / (x_j - x_i) as 32 bytes big-endian (Scalar mul / invert,
 * scalar.rs:523-548, :216-219).  ids that do not decode (>= r), are zero or repeat return BLSBN254_ERR_SCALAR. */
int blsbn254_lagrange_at_zero(blsbn254_ctx* ctx, const uint8_t* ids, size_t t, uint8_t* out /* t*32 */);
/* n_groups independent blsbn254_threshold_combine in one call.  Group g owns the shares off[g] .. off[g+1] of ids (32 B
 * each) and partial_sigs (64 B each); off = n_groups + 1 non-decreasing element offsets, host array (need not start at 0).
 * out_sigs[64 g ..] = sum_i lambda_i sigma_i of group g, byte-identical to blsbn254_threshold_combine on that group.
 * status[g] = 0, or the code the single call returns for that group alone: BLSBN254_ERR_SCALAR (an id >= r, == 0, or
 * repeated INSIDE the group; the same id in two groups is fine), else BLSBN254_ERR_G1 (a partial signature that does not
 * decode, or is off the curve).  The curve equation is tested here and NOT by the single call, which only requires a
 * partial signature to decode and returns whatever the addition formulas give for an off-curve one: "equal to the single
 * call" (bytes and code) therefore holds for inputs whose points are on the curve (the identity included) or do not
 * decode.  A bad group is never an error of the call: its output is the identity encoding (0, 1) and its neighbours are
 * unaffected.  An empty group gives the identity, status 0.  Groups of any size are accepted; the path is chosen by group
 * size (blsbn254_threshold_batch_stats), never the result.
 * Return: 0; BLSBN254_E_ARG for NULL arguments, decreasing offsets, more than 2^23 shares or groups.  n_groups == 0 -> 0. */
int blsbn254_threshold_combine_batch(blsbn254_ctx* ctx, const uint8_t* ids, const uint8_t* partial_sigs, const uint64_t* off,
                                     size_t n_groups, uint8_t* out_sigs /* n_groups*64 */, uint8_t* status /* n_groups */);
/* The coefficients alone: out[32 i ..] for every share i = 0 .. off[n_groups] - off[0], per group as
 * blsbn254_lagrange_at_zero; status as above (BLSBN254_ERR_SCALAR only); the coefficients of a bad group are zero bytes. */
int blsbn254_lagrange_at_zero_batch(blsbn254_ctx* ctx, const uint8_t* ids, const uint64_t* off, size_t n_groups,
                                    uint8_t* out /* N*32 */, uint8_t* status /* n_groups */);
/* since context creation: out[0] groups served by the lane-per-share kernels, out[1] groups handed to the single-group
 * pipeline (more shares than out[3]), out[2] launches of the lane-per-share pipeline; out[3] the hand-over size of this
 * build (a constant) */
int blsbn254_threshold_batch_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* The dealing side, over ragged groups.  A group g stands for one threshold key: t_g coefficients of its polynomial f_g, low
 * order first -- secret scalars a_0 .. a_{t-1} (32 B each) or their Feldman commitments C_j = [a_j] G2gen (128 B each) -- at
 * coef_off[g] .. coef_off[g+1], and n_g participant ids (32 B each) at id_off[g] .. id_off[g+1].  coef_off / id_off:
 * n_groups + 1 non-decreasing element offsets, host arrays, need not start at 0; outputs are indexed from the first id.
 * N = ids, T = coefficients of the call.  One lane per share; Horner from the highest coefficient down.
 * Return of all three: 0; BLSBN254_E_ARG for NULL arguments, decreasing offsets, more than 2^23 ids, coefficients or groups.
 * n_groups == 0 -> 0.  A bad group or share is never an error of the call.
 *
 * Key shares: out[32 i ..] = f_g(id_i) = sum_j a_j id_i^j mod r, canonical big-endian (Scalar multiply / add,
 * scalar.rs:523-548).  status[g] = BLSBN254_ERR_SCALAR when a coefficient or an id of the group is >= r or an id is 0 (which
 * would hand out the secret); the outputs of such a group are zero bytes.  Repeated ids are fine.  A group without coefficients
 * is the zero polynomial: zero bytes, status 0.  Signing side: not constant time (see blsbn254_sign_batch); the staged
 * coefficients and the device copy of the shares are zeroed in device memory before return. */
int blsbn254_fr_poly_eval_batch(blsbn254_ctx* ctx, const uint8_t* coeffs /* T*32 */, const uint64_t* coef_off, const uint8_t* ids /* N*32 */,
                                const uint64_t* id_off, size_t n_groups, uint8_t* out /* N*32 */, uint8_t* status /* n_groups */);
/* Public key shares: out_pks[128 i ..] = sum_j [id_i^j] C_j, uncompressed (Mul<Scalar> g2.rs:866-886 and Add g2.rs:789-831 for
 * G2Projective: acc = [id] acc + C_j with plain double-and-add over the complete formulas).  Every commitment is tested as
 * blsbn254_g2_check_batch tests a key (decodes, on the curve, in the r-torsion; the identity passes), so [id^j mod r] and the
 * integer Horner agree.  status[g] = BLSBN254_ERR_SCALAR for an id >= r or == 0, else BLSBN254_ERR_G2 for a commitment that
 * fails the test; the outputs of such a group are the identity encoding (what blsbn254_g2_mul_batch returns for k = 0).  A
 * group without commitments gives the identity, status 0.  The double-and-add loops over ONE bit count per launch, the largest
 * bit length of the launch's ids (computed on the host from the id bytes, ids that will be rejected included; at least 1, at
 * most 254): participant ids are small integers in practice, and ids below 2^16 cost 16/254 of full-width ones. */
int blsbn254_g2_poly_eval_batch(blsbn254_ctx* ctx, const uint8_t* commitments /* T*128 */, const uint64_t* coef_off, const uint8_t* ids /* N*32 */,
                                const uint64_t* id_off, size_t n_groups, uint8_t* out_pks /* N*128 */, uint8_t* status /* n_groups */);
/* Which partial signatures to leave out before blsbn254_threshold_combine_batch: bit i (LSB-first) of valid_bitmap = the bit
 * blsbn254_verify_batch gives for (out_pks_i, msg_g, partial_sigs_i) with out_pks of blsbn254_g2_poly_eval_batch, whose
 * arguments and status these are; group g's message is msgs[msg_off[g] .. msg_off[g+1]) (byte offsets, one message per group).
 * Every bit of a bad group is 0; a bad partial signature (does not decode, off the curve, the identity) clears its own bit only.
 * The public key shares never leave the device.  The group's message is hashed once per share.  Pending asynchronous verify
 * calls are settled on entry and none is left pending: the result is final on return. */
int blsbn254_threshold_verify_shares_batch(blsbn254_ctx* ctx, const uint8_t* commitments /* T*128 */, const uint64_t* coef_off,
                                           const uint8_t* ids /* N*32 */, const uint8_t* partial_sigs /* N*64 */, const uint64_t* id_off,
                                           const uint8_t* msgs, const uint64_t* msg_off /* n_groups+1 */, size_t n_groups,
                                           const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap /* ceil(N/8) */,
                                           uint8_t* status /* n_groups */);
/* since context creation: out[0] launches of the G2 evaluation kernel, out[1] shares evaluated in G2, out[2] shares evaluated
 * in Fr, out[3] the bit count the last G2 launch looped over */
int blsbn254_threshold_deal_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* What a receiver, an auditor or a complaint round does first: dealt key shares checked against their group's Feldman
 * commitments, [share_i] G2gen == sum_j [id_i^j] C_j, one equation in G2 per share and no pairing.  Groups, offsets and argument
 * errors are those of blsbn254_g2_poly_eval_batch (host arrays that need not start at 0; BLSBN254_E_ARG for NULL arguments,
 * decreasing offsets, more than 2^23 ids, coefficients or groups; n_groups == 0 -> 0); shares (32 B big-endian each, in the order
 * of the ids) == NULL with N > 0 is BLSBN254_E_ARG too.  status[g] is exactly what blsbn254_g2_poly_eval_batch writes for the
 * same commitments and ids (BLSBN254_ERR_SCALAR first, then BLSBN254_ERR_G2, else 0).  Bit i of valid_bitmap (LSB-first, in the
 * order of the ids; the pad bits of the last byte are 0) is 1 exactly when its group's status is 0, shares[i] is canonical
 * (< r), and [share_i] G2gen and sum_j [id_i^j] C_j are the same group element.  Equality includes the identity: a zero share is
 * valid exactly when f_g(id_i) = 0, and a group without commitments accepts zero shares only.  A share >= r clears its own bit
 * and never fails its group.  A bad group or share is never an error of the call.
 * The right-hand side is the evaluation of blsbn254_g2_poly_eval_batch (same kernels, left homogeneous; its launches go on
 * counting in blsbn254_threshold_deal_stats out[0], out[1], out[3]); the left one is a fixed-base multiplication out of a table
 * of the generator's multiples [d 2^(B w)] G2gen, B = blsbn254_threshold_key_check_stats out[3], which the context computes
 * on the device at the first call with N > 0 and keeps: 256 / B - 1 additions per share, no doubling; the comparison is
 * cross-multiplied, no inversion.  Nothing but the bitmap and the statuses leaves the device.
 * A share may be a secret (a receiver checks what it was sent).  The call is NOT constant time: the table is indexed by the
 * share's digits.  The staged shares are zeroed in device memory before the call returns, as blsbn254_fr_poly_eval_batch does
 * with its own; their decoded form (the digits) lives in registers only and is never written to memory.
 * Pending asynchronous verify calls are settled on entry; the result is final on return. */
int blsbn254_threshold_verify_key_shares_batch(blsbn254_ctx* ctx, const uint8_t* commitments /* T*128 */, const uint64_t* coef_off,
                                               const uint8_t* ids /* N*32 */, const uint8_t* shares /* N*32 */, const uint64_t* id_off,
                                               size_t n_groups, uint8_t* valid_bitmap /* ceil(N/8) */, uint8_t* status /* n_groups */);
/* since context creation: out[0] launches of the check kernel, out[1] shares checked, out[2] times this context built the
 * generator table (1 after the first call with N > 0, and it stays 1), out[3] the window width in bits (a constant of the build) */
int blsbn254_threshold_key_check_stats(blsbn254_ctx* ctx, uint64_t out[4]);
/* The combiner's call, over ragged groups: from a group's commitments, its message and the n_g >= t_g partial signatures it
 * received, the group signature sum_i lambda_i sigma_i over t_g good ones.  Arguments, offsets and argument errors are those of
 * blsbn254_threshold_verify_shares_batch (host arrays that need not start at 0; BLSBN254_E_ARG for NULL arguments, decreasing
 * offsets, more than 2^23 ids, coefficients or groups; n_groups == 0 -> 0), and out_sigs must not be NULL.  The threshold of
 * group g is its number of commitments, t_g = coef_off[g+1] - coef_off[g].  A group of more than 4096 shares (the size up to
 * which blsbn254_threshold_combine_batch runs one lane per share, blsbn254_threshold_batch_stats out[3]) makes the call return
 * BLSBN254_E_ARG.  The result never depends on the path taken, on launch boundaries or on how many groups share the call.
 *
 * A share is a CANDIDATE when its partial signature decodes, is on the curve and is not the identity; the others are left out
 * and never fail their group.  status[g], in this precedence: BLSBN254_ERR_SCALAR (an id of the group -- any of the n_g, not
 * only the ones used -- is >= r, is 0, or is repeated in the group), BLSBN254_ERR_G2 (a commitment fails the test of
 * blsbn254_g2_poly_eval_batch), BLSBN254_ST_SHORT (t_g == 0, or no t_g shares could be found whose combination verifies: fewer
 * than t_g candidates, or fewer than t_g candidates that verify individually), else 0.  A bad group is never an error of the
 * call: its out_sigs is the identity encoding (0, 1), all its used bits are 0, and its neighbours are unaffected.
 * With status 0, out_sigs[64 g ..] verifies under C_0 = commitments[coef_off[g]] for the group's message and dst, and
 * used_bitmap (LSB-first, in the order of the ids) marks exactly the t_g shares that were interpolated: the group's first t_g
 * candidates if their combination verifies under C_0 (ONE pairing equation per group, no key share evaluated), otherwise the
 * first t_g candidates whose bit blsbn254_threshold_verify_shares_batch sets (the per-share check runs for such groups only,
 * and its result is not verified again: partial signatures that verify individually interpolate to [f_g(0)] H(msg)).
 * A consequence of the optimistic rule: partial signatures whose errors cancel in the interpolation (lambda_1 delta_1 +
 * lambda_2 delta_2 = 0) are used and the group's signature is correct, although blsbn254_threshold_verify_shares_batch would
 * clear their bits.  Pending asynchronous verify calls are settled on entry and none is left pending. */
#define BLSBN254_ST_SHORT 5   /* a per-group status only, never a return value: no signature could be produced */
int blsbn254_threshold_combine_checked_batch(blsbn254_ctx* ctx, const uint8_t* commitments /* T*128 */, const uint64_t* coef_off,
                                             const uint8_t* ids /* N*32 */, const uint8_t* partial_sigs /* N*64 */, const uint64_t* id_off,
                                             const uint8_t* msgs, const uint64_t* msg_off /* n_groups+1 */, size_t n_groups,
                                             const uint8_t* dst, size_t dst_len, uint8_t* out_sigs /* n_groups*64 */,
                                             uint8_t* used_bitmap /* ceil(N/8) */, uint8_t* status /* n_groups */);
/* since context creation: out[0] groups settled by the optimistic attempt, out[1] groups sent to the per-share fallback, out[2]
 * shares verified individually, out[3] groups ending in BLSBN254_ST_SHORT */
int blsbn254_threshold_checked_stats(blsbn254_ctx* ctx, uint64_t out[4]);

/* ---- signing side (also used to generate large synthetic batches) ----------- */
/* sig_i = [sk_i] H(msg_i): G1Projective::hash (g1.rs:910-919) + Mul<Scalar> (g1.rs:518-534, :821-841).
 * sks = n x 32 B big-endian, each < r (else BLSBN254_ERR_SCALAR).  Not constant time (the reference's
 * ladder is; a verification engine handles public data -- do not use with production secrets).  The staged
 * secret keys are zeroed in device memory before the signing-side entry points return. */
int blsbn254_sign_batch(blsbn254_ctx* ctx, const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n,
                        const uint8_t* dst, size_t dst_len, uint8_t* sigs_out);
/* pk_i = [sk_i] G2gen: Mul<Scalar> for G2Projective (g2.rs:866-886) */
int blsbn254_sk_to_pk_batch(blsbn254_ctx* ctx, const uint8_t* sks, size_t n, uint8_t* pks_out);
/* sk_i = KeyGen(IKM_i, key_info): IETF BLS KeyGen (draft-irtf-cfrg-bls-signature-05 section 2.3) over
 * HKDF-SHA-256 with the salt the reference names (KEYGEN_SALT, helpers.rs:3) and L = 48; the reference
 * has the constant but no procedure.  ikm = n x ikm_len bytes, ikm_len >= 32 (else BLSBN254_E_ARG);
 * sks_out = n x 32 B big-endian, each in [1, r). */
int blsbn254_keygen_batch(blsbn254_ctx* ctx, const uint8_t* ikm, size_t ikm_len, size_t n,
                          const uint8_t* key_info, size_t key_info_len, uint8_t* sks_out);
/* Scalar::hash<ExpandMsgXmd<Sha256>> (scalar.rs:554-563): OS2IP(expand_message_xmd(msg, dst, 48)) mod r,
 * out = n x 32 B big-endian.  (The reference's Reduce<U384>, scalar.rs:393-402, subtracts r once and
 * truncates; the RFC 9380 hash_to_field value it is meant to produce is what is returned here.) */
int blsbn254_hash_to_scalar_batch(blsbn254_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t n,
                                  const uint8_t* dst, size_t dst_len, uint8_t* out);
/* Proof of possession (draft section 3.3.2 / 3.3.3): proof_i = [sk_i] H(pk_i bytes) with the 128-byte
 * uncompressed public key as the message and a caller-supplied POP tag as DST; pop_verify is CoreVerify of
 * (pk_i, pk_i bytes, proof_i), bitmap as in verify_batch. */
int blsbn254_pop_prove_batch(blsbn254_ctx* ctx, const uint8_t* sks, size_t n, const uint8_t* dst, size_t dst_len,
                             uint8_t* proofs_out);
int blsbn254_pop_verify_batch(blsbn254_ctx* ctx, const uint8_t* pks, const uint8_t* proofs, size_t n,
                              const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap);

/* ---- compressed wire codecs ------------------------------------------------- */
/* G1 32 B: x with bit 255 = parity of y (G1Affine::to_compressed g1.rs:283-288); decompression picks the root
 * whose parity equals the flag -- the corrected rule: the reference's from_compressed (g1.rs:311-328) selects
 * on y.is_high() ^ flag and mis-decodes about half of G1.  G2 64 B: x.c1 || x.c0 with
 * bit 255 = sgn0(y) (g2.rs:274-283, :309-340).  An operand that does not decode (coordinate >= p, or no
 * point with that x) returns BLSBN254_ERR_G1 / _G2.  Decompressed points are on the curve by construction;
 * G2 subgroup membership still has to be checked (blsbn254_g2_check_batch). */
int blsbn254_g1_compress_batch(blsbn254_ctx* ctx, const uint8_t* g1 /* n*64 */, size_t n, uint8_t* out /* n*32 */);
int blsbn254_g1_decompress_batch(blsbn254_ctx* ctx, const uint8_t* in /* n*32 */, size_t n, uint8_t* g1 /* n*64 */);
int blsbn254_g2_compress_batch(blsbn254_ctx* ctx, const uint8_t* g2 /* n*128 */, size_t n, uint8_t* out /* n*64 */);
int blsbn254_g2_decompress_batch(blsbn254_ctx* ctx, const uint8_t* in /* n*64 */, size_t n, uint8_t* g2 /* n*128 */);

/* ---- compressed input: per-element inflation, and the verify / key-set calls on wire-format operands ---- */
/* The per-element form of the decompress calls: a malformed element is never an error of the call.  Element i that decodes
 * gives status[i] = 1 and the bytes blsbn254_g1/g2_decompress_batch give for it; one that does not (a coordinate >= p, or no
 * point with that x) gives status[i] = 0 and THE MARKER, 0xFF in all of its 64 / 128 output bytes.  No entry point of this
 * library decodes the marker (its coordinates are >= p), so the output may be fed to any of them and a malformed element is
 * then treated as that entry point treats any undecodable one: a cleared bit in the verify calls, a bad key in a key set, its
 * error code in the primitives.  Same rule as decompression otherwise: flag = parity of y / sgn0(y), x == 0 is the identity
 * whatever the flag; G2 subgroup membership is not tested here.  Bad arguments (a null pointer with n > 0): BLSBN254_E_ARG, outputs untouched;
 * n == 0: 0. */
int blsbn254_g1_inflate_batch(blsbn254_ctx* ctx, const uint8_t* in /* n*32 */, size_t n, uint8_t* g1 /* n*64 */, uint8_t* status /* n */);
int blsbn254_g2_inflate_batch(blsbn254_ctx* ctx, const uint8_t* in /* n*64 */, size_t n, uint8_t* g2 /* n*128 */, uint8_t* status /* n */);
/* blsbn254_verify_batch / blsbn254_verify_batch_rlc on compressed public keys and signatures: the bitmap those calls give on
 * the outputs of blsbn254_g2_inflate_batch(pks) and blsbn254_g1_inflate_batch(sigs) -- a key or signature that does not
 * inflate clears its tuple's bit -- with the inflation done on the device between the upload and the pipeline: nothing but
 * the bitmap comes back.  Chunking, size limits, argument errors and the meaning of seed are those of the uncompressed calls. */
int blsbn254_verify_batch_compressed(blsbn254_ctx* ctx, const uint8_t* pks /* n*64 */, const uint8_t* msgs, const uint64_t* off,
                                     const uint8_t* sigs /* n*32 */, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap);
int blsbn254_verify_batch_rlc_compressed(blsbn254_ctx* ctx, const uint8_t* pks /* n*64 */, const uint8_t* msgs, const uint64_t* off,
                                         const uint8_t* sigs /* n*32 */, size_t n, const uint8_t* dst, size_t dst_len, const uint8_t seed[32],
                                         uint8_t* valid_bitmap);
/* Key-set registration from compressed keys: the handle blsbn254_keyset_create makes from the inflated keys, or, with proofs
 * (non-null: compressed too, 32 bytes each), the handle blsbn254_keyset_create_checked makes from the inflated keys and proofs;
 * every later call on the handle gives the bytes it gives on that one.  A key that does not inflate is a bad key of the handle,
 * a proof that does not inflate is a failing proof.  A proof's MESSAGE stays the 128-byte UNCOMPRESSED encoding of its key, as
 * blsbn254_pop_prove_batch signs it: compression changes how a proof travels, not what it signs.  proofs == NULL: pop_dst and
 * pop_dst_len are ignored.  Limits and argument errors as the uncompressed registrations. */
int blsbn254_keyset_create_compressed(blsbn254_ctx* ctx, const uint8_t* pks /* n_keys*64 */, const uint8_t* proofs /* n_keys*32 or NULL */,
                                      size_t n_keys, const uint8_t* pop_dst, size_t pop_dst_len, blsbn254_keyset** out);
/* blsbn254_keyset_fast_aggregate_verify_batch on compressed signatures: its bitmap on blsbn254_g1_inflate_batch(sigs).  keys:
 * a handle of any of the three registrations. */
int blsbn254_keyset_fast_aggregate_verify_batch_compressed(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint8_t* sel,
                                                           const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs /* n_groups*32 */,
                                                           size_t n_groups, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap);
/* The write side on wire bytes: a collector, a merger and a verifier that hold 32-byte signatures run on them end to end.
 * blsbn254_keyset_aggregate_checked_batch and blsbn254_keyset_committee_aggregate_checked_batch on compressed signatures in
 * and out: status and out_sel are byte for byte what the uncompressed call gives on blsbn254_g1_inflate_batch(sigs), and
 * out_sigs is blsbn254_g1_compress_batch of that call's out_sigs (a group that ends BLSBN254_ST_SHORT: the compressed
 * identity).  A signature that does not inflate is left out as any undecodable one is -- never an error of the call, never a
 * reason for the fallback.  Every other rule (arguments, limits, offsets, sel_off, the stats arrays, which are shared with the
 * uncompressed forms) is the uncompressed call's. */
int blsbn254_keyset_aggregate_checked_batch_compressed(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint32_t* idx,
                                                       const uint8_t* sigs /* N*32 */, const uint64_t* sig_off, const uint8_t* msgs,
                                                       const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                       uint8_t* out_sigs /* n_groups*32 */, uint8_t* out_sel, uint8_t* status);
int blsbn254_keyset_committee_aggregate_checked_batch_compressed(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint32_t* com,
                                                                 const uint32_t* pos, const uint8_t* sigs /* N*32 */, const uint64_t* sig_off,
                                                                 const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* sel_off,
                                                                 size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                                 uint8_t* out_sigs /* n_groups*32 */, uint8_t* out_sel, uint8_t* status);
/* blsbn254_keyset_merge_checked_batch and blsbn254_keyset_committee_merge_checked_batch likewise: the partial aggregates
 * arrive compressed, the merged aggregates leave compressed; status, out_sel and used are those of the uncompressed call on
 * blsbn254_g1_inflate_batch(sigs), out_sigs is blsbn254_g1_compress_batch of its out_sigs. */
int blsbn254_keyset_merge_checked_batch_compressed(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint8_t* rows,
                                                   const uint8_t* sigs /* N*32 */, const uint64_t* con_off, const uint8_t* msgs,
                                                   const uint64_t* msg_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                   uint8_t* out_sigs /* n_groups*32 */, uint8_t* out_sel, uint8_t* used, uint8_t* status);
int blsbn254_keyset_committee_merge_checked_batch_compressed(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint32_t* com,
                                                             const uint8_t* rows, const uint64_t* row_off, const uint8_t* sigs /* N*32 */,
                                                             const uint64_t* con_off, const uint8_t* msgs, const uint64_t* msg_off,
                                                             const uint64_t* sel_off, size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                             uint8_t* out_sigs /* n_groups*32 */, uint8_t* out_sel, uint8_t* used,
                                                             uint8_t* status);
/* blsbn254_keyset_committee_fast_aggregate_verify_batch on compressed signatures: its bitmap on
 * blsbn254_g1_inflate_batch(sigs), as blsbn254_keyset_fast_aggregate_verify_batch_compressed is for the full-width call. */
int blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed(blsbn254_ctx* ctx, const blsbn254_keyset* keys, const uint32_t* com,
                                                                     const uint8_t* sel, const uint64_t* sel_off, const uint8_t* msgs,
                                                                     const uint64_t* off, const uint8_t* sigs /* n_groups*32 */,
                                                                     size_t n_groups, const uint8_t* dst, size_t dst_len,
                                                                     uint8_t* valid_bitmap);

/* ---- device-resident variants (plumbing for callers that already hold the batch in HBM) ----- */
/* All d_* pointers are device pointers on ctx's GPU.  Work is enqueued on ctx's stream and is
 * complete after blsbn254_ctx_synchronize().  d_valid_bitmap needs ceil(n/8) bytes.
 * blsbn254_verify_batch_dev does not wait for the device in steady state.  The number of distinct public keys sizes the per-key
 * tables and chooses between the prepared-key and the exact per-tuple pipeline; the FIRST call on a context (and every call
 * after one that took the exact path, and calls of more than one 4 Mi-tuple chunk) reads that 4-byte count back before it enqueues the
 * pipeline.  After a call that took the prepared-key path, the next call is enqueued on the ASSUMPTION that its keys repeat
 * likewise (tables reserved for twice the last count; the device-side count bounds the per-key work) and returns at once; count
 * and a check of the assumption come back behind an event and are read by the next entry point on the context or by
 * blsbn254_ctx_synchronize.  If the assumption failed (a new key set, more keys than reserved), that call is re-run on the
 * counting path there -- before blsbn254_ctx_synchronize returns -- so the bitmap is final after blsbn254_ctx_synchronize as
 * always (a caller that only synchronises the raw stream of blsbn254_ctx_stream must not rely on it).  Up to four calls stay in
 * flight; the caller's device buffers must stay untouched until blsbn254_ctx_synchronize.  BLSBN254_ASYNC_VERIFY=0 or
 * blsbn254_set_async_verify(ctx, 0) makes every call count first; blsbn254_async_stats: out[0] chunks enqueued on the
 * assumption, out[1] of them re-run.  Launch size picks the kernels: up to 2048 tuples one workgroup of two waves per tuple,
 * up to 16384 three lanes per tuple, beyond one lane per tuple -- same values, same bitmap. */
int blsbn254_set_async_verify(blsbn254_ctx* ctx, int on);
int blsbn254_async_stats(blsbn254_ctx* ctx, uint64_t out[2] /* enqueued on the assumption, re-run */);
int blsbn254_verify_batch_dev(blsbn254_ctx* ctx, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
                              const uint8_t* d_sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* d_valid_bitmap);
int blsbn254_pairing_batch_dev(blsbn254_ctx* ctx, const uint8_t* d_g1, const uint8_t* d_g2, size_t n, uint8_t* d_gt,
                               uint8_t* d_status /* n bytes or NULL */);
int blsbn254_ctx_synchronize(blsbn254_ctx* ctx);
void* blsbn254_ctx_stream(blsbn254_ctx* ctx); /* the hipStream_t */

/* ---- Gt group operations and the field-primitive debug ABI ------------------------------------------------ */
/* Gt is written multiplicatively: the reference's `Gt + Gt` is the Fp12 product (pairings.rs:245-381 trait glue over
 * fp12.rs:203-210) and Gt::mul_by_scalar (pairings.rs:585-600) is gt^k, k = 32 bytes big-endian (any 256-bit value).
 * Operands that do not decode (a coefficient >= p) return BLSBN254_ERR_GT. */
int blsbn254_gt_mul_batch(blsbn254_ctx* ctx, const uint8_t* a /* n*384 */, const uint8_t* b /* n*384 */, size_t n, uint8_t* out);
int blsbn254_gt_pow_batch(blsbn254_ctx* ctx, const uint8_t* gt /* n*384 */, const uint8_t* scalars /* n*32 */, size_t n, uint8_t* out);
/* One field / tower primitive applied element-wise to n operands: the isolated parity pin of the device arithmetic
 * (the reference's fp6.rs / fp12.rs have no test vectors; tests fuzz this against the CPU oracle).
 * Element bytes are canonical big-endian coefficients: Fp 32 B; Fp2 64 B = c0 || c1 (NOT the c1 || c0 wire order of G2);
 * Fp6 192 B = c0.c0 c0.c1 c1.c0 c1.c1 c2.c0 c2.c1; Fp12 384 B in Gt::to_repr order.  b is read by the binary ops only
 * (pass NULL otherwise); a coefficient >= p returns BLSBN254_ERR_GT.  Fr 32 B (operations 64 .. 69). */
#define BLSBN254_OP_FP_MUL 0          /* Fp::multiply        fp.rs:404-407 */
#define BLSBN254_OP_FP_SQR 1          /* Fp::square          fp.rs:409-412 */
#define BLSBN254_OP_FP_INV 2          /* Fp::invert          fp.rs:207-210 (0 -> 0) */
#define BLSBN254_OP_FP_ADD 3          /* fp.rs:388 */
#define BLSBN254_OP_FP_SUB 4          /* fp.rs:396 */
#define BLSBN254_OP_FP_NEG 5          /* fp.rs:400 */
#define BLSBN254_OP_FP_SQRT 6         /* a root of a (sqrt_ratio, fp.rs:212-243: a^((p+1)/4)), or 0 when a is not a square */
#define BLSBN254_OP_FP_IS_SQUARE 7    /* is_square fp.rs:428-431 as the field element 1 / 0 */
#define BLSBN254_OP_FP_MUL_3B 8       /* mul_by_3b = 9 a      fp.rs:414 */
#define BLSBN254_OP_FP2_MUL 16        /* fp2.rs:377-390 */
#define BLSBN254_OP_FP2_SQR 17        /* fp2.rs:392-402 */
#define BLSBN254_OP_FP2_INV 18        /* fp2.rs:161-166 */
#define BLSBN254_OP_FP2_MUL_XI 19     /* times the Fp6 non-residue 9 + u (E1: not fp2.rs:415-420's 1 + u) */
#define BLSBN254_OP_FP2_CONJ 20       /* fp2.rs:428-437 */
#define BLSBN254_OP_FP2_SQRT 21       /* fp2.rs:172-218, a root or 0 */
#define BLSBN254_OP_FP6_MUL 32        /* fp6.rs:225-242 */
#define BLSBN254_OP_FP6_SQR 33        /* a * a (fp6.rs:244-259 is defective, E2) */
#define BLSBN254_OP_FP6_INV 34        /* fp6.rs:261-287, denominator corrected */
#define BLSBN254_OP_FP6_MUL_V 35      /* mul_by_non_residue fp6.rs:146-152 */
#define BLSBN254_OP_FP12_MUL 48       /* fp12.rs:203-210 */
#define BLSBN254_OP_FP12_SQR 49       /* fp12.rs:170-180 */
#define BLSBN254_OP_FP12_INV 50       /* fp12.rs:212-219 */
#define BLSBN254_OP_FP12_CONJ 51      /* fp12.rs:131-137 */
#define BLSBN254_OP_FP12_FROB1 52     /* frobenius_map^1..3 with the xi^((p^k-1)/6) constants (E3) */
#define BLSBN254_OP_FP12_FROB2 53
#define BLSBN254_OP_FP12_FROB3 54
#define BLSBN254_OP_FP12_CYC_SQR 55   /* cyclotomic_square pairings.rs:68-115 (the Granger-Scott formula on any input) */
#define BLSBN254_OP_FP12_MUL_034 56   /* sparse line product, a * (b.c0.c0 + b.c1.c0 w + b.c1.c1 v w)  (E7) */
/* the reference's Scalar, 32 B big-endian; an operand >= r returns BLSBN254_ERR_SCALAR */
#define BLSBN254_OP_FR_MUL 64         /* scalar.rs:523-548 */
#define BLSBN254_OP_FR_SQR 65
#define BLSBN254_OP_FR_INV 66         /* Scalar::invert scalar.rs:216-219 (0 -> 0) */
#define BLSBN254_OP_FR_ADD 67
#define BLSBN254_OP_FR_SUB 68
#define BLSBN254_OP_FR_NEG 69
int blsbn254_field_op_batch(blsbn254_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);

/* ---- multi-device (SURVEY.md 8b "ctx over a device list", 8e) -------------------------------------------- */
/* A blsbn254_multi owns one ctx (stream + workspace) per entry of `devices` (HIP ordinals; an ordinal may be listed more
 * than once -- two contexts on one GPU -- which is how a single-GPU box exercises this path).  A call runs one host
 * thread per entry.  Verify tuples are independent (the per-term independence of multi_miller_loop,
 * pairings.rs:819-824): device g takes a contiguous range of the batch (boundaries at multiples of 8 tuples) and
 * there is no data-path collective.  Calls on one blsbn254_multi must be externally serialized. */
typedef struct blsbn254_multi blsbn254_multi;
int blsbn254_multi_create(const int* devices, int ndev, blsbn254_multi** out);
void blsbn254_multi_destroy(blsbn254_multi* m);
int blsbn254_multi_device_count(blsbn254_multi* m);
blsbn254_ctx* blsbn254_multi_ctx(blsbn254_multi* m, int i); /* the i-th per-device ctx (owned by m) */
const char* blsbn254_multi_last_error(blsbn254_multi* m);
/* blsbn254_verify_batch over all devices of m: same arguments, same bitmap.  Host pointers in and out; every device
 * copies its slice of the bitmap into valid_bitmap (a host gather of disjoint slices). */
int blsbn254_verify_batch_multi(blsbn254_multi* m, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                                const uint8_t* sigs, size_t n, const uint8_t* dst, size_t dst_len, uint8_t* valid_bitmap);
/* blsbn254_verify_batch_rlc over all devices of m (each device verifies its contiguous shard with its own chunks and weights):
 * same bitmap as blsbn254_verify_batch_multi. */
int blsbn254_verify_batch_rlc_multi(blsbn254_multi* m, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                                    const uint8_t* sigs, size_t n, const uint8_t* dst, size_t dst_len,
                                    const uint8_t seed[32], uint8_t* valid_bitmap);
/* blsbn254_aggregate_verify over all devices of m: per-device blsbn254_aggregate_partial, the 384-byte partials are
 * gathered on the host, one blsbn254_aggregate_finish on the first device. */
int blsbn254_aggregate_verify_multi(blsbn254_multi* m, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, size_t n,
                                    const uint8_t agg_sig[64], const uint8_t* dst, size_t dst_len, int* valid);
/* Device-resident N-GPU verify with the bitmap exchange of SURVEY.md 8e.  Device g already holds ITS shard in HBM:
 * d_pks[g] (counts[g] x 128), d_msgs[g] with d_off[g] (counts[g] + 1 offsets relative to d_msgs[g]), d_sigs[g]
 * (counts[g] x 64); counts[g] is a multiple of 32 for every g but the last.  Every device writes its bits into a
 * zeroed full-length word array and the arrays are summed by ONE ncclAllReduce(ncclSum, ncclUint32) over xGMI
 * (disjoint bit sets: SUM == OR; RCCL has no bitwise op), so that on return d_full_bitmap[g] (4 * ceil(N / 32) bytes
 * on device g, N = sum of counts) holds the bitmap of the whole batch in global order on EVERY device.  librccl is
 * loaded with dlopen at first use (BLSBN254_E_RCCL if absent or on an RCCL error, e.g. one ordinal listed twice).
 * Status: exercised on hardware with a ONE-rank communicator only (the builder's and the pool's test boxes have one GPU;
 * RCCL rejects a communicator that lists an ordinal twice).  The ndev > 1 branch (ncclCommInitAll over ndev ordinals, grouped
 * all-reduce, shard placement) has a test that runs as soon as two devices are visible
 * (tests/test_gpu_sharded.py::test_c_abi_multi_device_resident_rccl_two_gpus); until it has run, treat ndev > 1 here as
 * unverified and prefer blsbn254_verify_batch_multi (host gather) or one process per GPU with torch.distributed. */
int blsbn254_verify_batch_multi_dev(blsbn254_multi* m, const uint8_t* const* d_pks, const uint8_t* const* d_msgs,
                                    const uint64_t* const* d_off, const uint8_t* const* d_sigs, const size_t* counts,
                                    const uint8_t* dst, size_t dst_len, uint8_t* const* d_full_bitmap);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------ */
/* When enabled, every kernel launch on the ctx is bracketed by HIP events on the ctx stream;
 * profile_read returns, per kernel name, the number of launches and the summed duration in ms
 * since the last reset (it synchronizes the stream). */
int blsbn254_profile_enable(blsbn254_ctx* ctx, int on);
int blsbn254_profile_reset(blsbn254_ctx* ctx);
int blsbn254_profile_read(blsbn254_ctx* ctx, char* names /* max_entries*32 */, uint64_t* launches, double* total_ms, int max_entries);

/* Measured whole-chip v_mad_u64_u32 issue rate (lane-MADs per second): the VALU roofline denominator. */
int blsbn254_valu_peak(blsbn254_ctx* ctx, double* mads_per_s);
/* The whole probe: out[0] v_mad_u64_u32 lane-MADs/s, out[1] plain 32-bit VOP2 lane-ops/s, out[2] / out[3] the shader
 * clock (Hz) the chip held under each of the two probe kernels (in-kernel s_memtime / s_memrealtime), out[4] compute
 * units, out[5] the 4-cycle single-wave issue ceiling at that clock = CUs x 4 SIMDs x 16 lanes x out[2]. */
int blsbn254_valu_probe(blsbn254_ctx* ctx, double out[6]);

#ifdef __cplusplus
}
#endif
#endif
