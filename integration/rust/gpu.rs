//! `src/inner_types/gpu.rs` — MI355X engine behind the crate's pairing front-end (feature `mi355x`).
//!
//! This file is NOT built in the engine's repository (its image has no Rust toolchain); it is the
//! reference-side half of the drop-in boundary described in INTEGRATION.md.  It depends on nothing but
//! the crate's own public byte codecs (`to_uncompressed` / `from_uncompressed`, `Gt::from_repr`) and on
//! `ffi.rs`, which is generated from `include/blsbn254.h`.
//!
//! Wiring (three edits in the crate):
//!   * `Cargo.toml`:  `[features] mi355x = ["std"]`
//!   * `build.rs`:    see `build.rs` beside this file (adds the library search path)
//!   * `src/inner_types.rs`:  `#[cfg(feature = "mi355x")] mod ffi; #[cfg(feature = "mi355x")] pub mod gpu;`
//!     and `pub use pairings::*;` (the module is private today, so `pairing`, `Gt`, `Bn254` are unreachable)
//! after which `pairings.rs` forwards its four entry points:
//!   `pairing(p, q)`                       -> `gpu::pairing(p, q)`
//!   `multi_miller_loop(terms)`            -> `gpu::multi_miller_loop(terms)`   (with `G2Prepared` = `gpu::G2Prepared`)
//!   `MillerLoopResult::final_exponentiation(&self)` -> `gpu::final_exponentiation(self)`
//!   `G1Projective::hash::<ExpandMsgXmd<Sha256>>`    -> `gpu::hash_to_g1(msg, dst)`
use super::ffi::{self, Ctx};
use super::{G1Affine, G2Affine, Gt, MillerLoopResult};
use crate::Bn254Error;
use core::ffi::c_int;
use std::sync::{Mutex, OnceLock};
use std::vec::Vec;

/// One engine context per process (GPU 0, or `BLSBN254_DEVICE`).  Calls on a context are serialized,
/// which matches the reference: it has no threads of its own and its types are `Send + Sync` markers.
struct Engine(*mut Ctx);
unsafe impl Send for Engine {}

fn engine() -> &'static Mutex<Engine> {
    static ENGINE: OnceLock<Mutex<Engine>> = OnceLock::new();
    ENGINE.get_or_init(|| {
        let device = std::env::var("BLSBN254_DEVICE").ok().and_then(|s| s.parse::<c_int>().ok()).unwrap_or(0);
        let mut ctx: *mut Ctx = core::ptr::null_mut();
        let rc = unsafe { ffi::blsbn254_ctx_create(device, &mut ctx) };
        // no CPU fallback by design: without a gfx950 device the engine refuses to start
        assert!(rc == 0 && !ctx.is_null(), "blsbn254_ctx_create failed with code {rc}");
        Mutex::new(Engine(ctx))
    })
}

/// Return codes 1..4 are the crate's own error enum in declaration order (`error.rs:4-10`).
fn check(rc: c_int) -> Result<(), Bn254Error> {
    match rc {
        0 => Ok(()),
        1 => Err(Bn254Error::InvalidScalarBytes),
        2 => Err(Bn254Error::InvalidG1Bytes),
        3 => Err(Bn254Error::InvalidG2Bytes),
        4 => Err(Bn254Error::InvalidGtBytes),
        other => panic!("blsbn254 device error {other}"),
    }
}

fn with_ctx<T>(f: impl FnOnce(*mut Ctx) -> T) -> T {
    let guard = engine().lock().expect("engine mutex poisoned");
    f(guard.0)
}

/// Concatenate messages and build the `n + 1` offsets the batch ABI takes.
fn pack(msgs: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let mut data = Vec::with_capacity(msgs.iter().map(|m| m.len()).sum());
    let mut off = Vec::with_capacity(msgs.len() + 1);
    off.push(0u64);
    for m in msgs {
        data.extend_from_slice(m);
        off.push(data.len() as u64);
    }
    (data, off)
}

fn bits(bitmap: &[u8], n: usize) -> Vec<bool> {
    (0..n).map(|i| (bitmap[i >> 3] >> (i & 7)) & 1 == 1).collect()
}

// ---------------------------------------------------------------- reference operator API

/// Body of `pairing` (`pairings.rs:760`), `Engine::pairing` (`:685-696`) and `pairing_with` (`:662-678`).
pub fn pairing(p: &G1Affine, q: &G2Affine) -> Gt {
    pairing_batch(core::slice::from_ref(p), core::slice::from_ref(q)).pop().expect("one pairing")
}

/// `n` independent pairings in one launch sequence.
pub fn pairing_batch(ps: &[G1Affine], qs: &[G2Affine]) -> Vec<Gt> {
    assert_eq!(ps.len(), qs.len());
    let n = ps.len();
    let g1: Vec<u8> = ps.iter().flat_map(|p| p.to_uncompressed()).collect();
    let g2: Vec<u8> = qs.iter().flat_map(|q| q.to_uncompressed()).collect();
    let mut out = vec![0u8; Gt::BYTES * n];
    with_ctx(|c| check(unsafe { ffi::blsbn254_pairing_batch(c, g1.as_ptr(), g2.as_ptr(), n, out.as_mut_ptr()) }))
        .expect("points produced by the crate's own encoders decode");
    out.chunks_exact(Gt::BYTES)
        .map(|b| Option::<Gt>::from(Gt::from_repr(b.try_into().expect("384 bytes"))).expect("engine output is canonical"))
        .collect()
}

/// Replacement for `G2Prepared` (`pairings.rs:609-660`, whose `From<G2Affine>` panics): the engine walks
/// the line steps itself, so the prepared form is the affine point.
#[derive(Copy, Clone, Debug)]
pub struct G2Prepared(pub G2Affine);

impl From<G2Affine> for G2Prepared {
    fn from(q: G2Affine) -> Self {
        Self(q)
    }
}

/// Body of `multi_miller_loop` (`pairings.rs:808-857`) and `MultiMillerLoop::multi_miller_loop` (`:706-713`):
/// the product of the Miller values of all terms (identity terms contribute 1, as `:820-823`).
pub fn multi_miller_loop(terms: &[(&G1Affine, &G2Prepared)]) -> MillerLoopResult {
    let g1: Vec<u8> = terms.iter().flat_map(|t| t.0.to_uncompressed()).collect();
    let g2: Vec<u8> = terms.iter().flat_map(|t| (t.1).0.to_uncompressed()).collect();
    let mut out = [0u8; Gt::BYTES];
    with_ctx(|c| check(unsafe { ffi::blsbn254_multi_miller_loop(c, g1.as_ptr(), g2.as_ptr(), terms.len(), out.as_mut_ptr()) }))
        .expect("points produced by the crate's own encoders decode");
    // same 12 x 32-byte layout as Gt::to_repr (pairings.rs:499-514); Gt::from_repr (:516-579) only decodes
    // the twelve coordinates, it makes no subgroup claim, so it also carries a raw Miller value
    MillerLoopResult(Option::<Gt>::from(Gt::from_repr(&out)).expect("engine output is canonical").0)
}

/// Body of `MillerLoopResult::final_exponentiation` (`pairings.rs:50-178`, trait impl `:698-704`).
pub fn final_exponentiation(f: &MillerLoopResult) -> Gt {
    let input = Gt(f.0).to_repr();
    let mut out = [0u8; Gt::BYTES];
    with_ctx(|c| check(unsafe { ffi::blsbn254_final_exponentiation(c, input.as_ptr(), 1, out.as_mut_ptr()) }))
        .expect("a field element encodes canonically");
    Option::<Gt>::from(Gt::from_repr(&out)).expect("engine output is canonical")
}

/// Body of `G1Projective::hash::<ExpandMsgXmd<Sha256>>` (`g1.rs:910-919`); `encode` (`:922-928`) is the
/// same call on `blsbn254_encode_to_g1_batch`.
pub fn hash_to_g1(msg: &[u8], dst: &[u8]) -> G1Affine {
    let off = [0u64, msg.len() as u64];
    let mut out = [0u8; G1Affine::UNCOMPRESSED_BYTES];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_hash_to_g1_batch(c, msg.as_ptr(), off.as_ptr(), 1, dst.as_ptr(), dst.len(), out.as_mut_ptr())
    }))
    .expect("hashing cannot fail");
    Option::<G1Affine>::from(G1Affine::from_uncompressed(&out)).expect("engine output is on the curve")
}

/// Body of `G2Projective::hash::<ExpandMsgXmd<Sha256>>` (`g2.rs:919-927`).
pub fn hash_to_g2(msg: &[u8], dst: &[u8]) -> G2Affine {
    let off = [0u64, msg.len() as u64];
    let mut out = [0u8; G2Affine::UNCOMPRESSED_BYTES];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_hash_to_g2_batch(c, msg.as_ptr(), off.as_ptr(), 1, dst.as_ptr(), dst.len(), out.as_mut_ptr())
    }))
    .expect("hashing cannot fail");
    Option::<G2Affine>::from(G2Affine::from_uncompressed(&out)).expect("engine output is in the subgroup")
}

/// `G2Affine::is_on_curve & is_torsion_free` (`g2.rs:404-414`, `:733-746`) for a batch of encoded keys.
pub fn g2_check_batch(pks: &[[u8; 128]]) -> Vec<bool> {
    let n = pks.len();
    let flat: Vec<u8> = pks.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe { ffi::blsbn254_g2_check_batch(c, flat.as_ptr(), n, bm.as_mut_ptr()) })).expect("no decode errors here");
    bits(&bm, n)
}

// ---------------------------------------------------------------- the BLS layer the crate lacks

/// CoreVerify of `n` independent (public key, message, signature) tuples; signatures in G1, keys in G2.
/// Malformed or invalid tuples clear their bit; they are not errors.
pub fn verify_batch(pks: &[[u8; 128]], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(pks.len() == msgs.len() && msgs.len() == sigs.len());
    let n = pks.len();
    let (data, off) = pack(msgs);
    let pk: Vec<u8> = pks.iter().flatten().copied().collect();
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_verify_batch(c, pk.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), bm.as_mut_ptr())
    }))
    .expect("per-tuple failures are reported in the bitmap");
    bits(&bm, n)
}

/// Batch verification by random linear combination: the same answers as `verify_batch` (an invalid chunk of 16 tuples passes
/// with probability about 2^-64), several times faster on batches that repeat public keys.  The weights are drawn inside the
/// library (OS randomness, after the batch is fixed).
pub fn verify_batch_rlc(pks: &[[u8; 128]], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(pks.len() == msgs.len() && msgs.len() == sigs.len());
    let n = pks.len();
    let (data, off) = pack(msgs);
    let pk: Vec<u8> = pks.iter().flatten().copied().collect();
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_verify_batch_rlc(c, pk.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(),
                                       std::ptr::null(), bm.as_mut_ptr())
    }))
    .expect("per-tuple failures are reported in the bitmap");
    bits(&bm, n)
}

/// CoreAggregateVerify: one aggregate signature over `n` (public key, message) pairs.
pub fn aggregate_verify(pks: &[[u8; 128]], msgs: &[&[u8]], agg_sig: &[u8; 64], dst: &[u8]) -> bool {
    assert_eq!(pks.len(), msgs.len());
    let (data, off) = pack(msgs);
    let pk: Vec<u8> = pks.iter().flatten().copied().collect();
    let mut valid: c_int = 0;
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_aggregate_verify(c, pk.as_ptr(), data.as_ptr(), off.as_ptr(), pks.len(), agg_sig.as_ptr(), dst.as_ptr(), dst.len(), &mut valid)
    }))
    .expect("invalid inputs yield valid = 0");
    valid == 1
}

/// `impl Sum for G1Projective` (`g1.rs:561-565`) over encoded signatures.
pub fn aggregate_sigs(sigs: &[[u8; 64]]) -> Result<[u8; 64], Bn254Error> {
    let flat: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut out = [0u8; 64];
    with_ctx(|c| check(unsafe { ffi::blsbn254_aggregate_sigs(c, flat.as_ptr(), sigs.len(), out.as_mut_ptr()) }))?;
    Ok(out)
}

/// Lagrange interpolation at zero of `t` partial signatures (`Mul<Scalar>` `g1.rs:518-534` + `Sum`);
/// `ids` are the 32-byte big-endian participant identifiers.
pub fn threshold_combine(ids: &[[u8; 32]], partials: &[[u8; 64]]) -> Result<[u8; 64], Bn254Error> {
    assert_eq!(ids.len(), partials.len());
    let id: Vec<u8> = ids.iter().flatten().copied().collect();
    let ps: Vec<u8> = partials.iter().flatten().copied().collect();
    let mut out = [0u8; 64];
    with_ctx(|c| check(unsafe { ffi::blsbn254_threshold_combine(c, id.as_ptr(), ps.as_ptr(), ids.len(), out.as_mut_ptr()) }))?;
    Ok(out)
}

/// What a combiner needs, for many committees at once (`blsbn254_threshold_combine_checked_batch`): `groups[g]` = the Feldman
/// commitments of group g (their number is its threshold), the (id, partial signature) pairs it received and its message.
/// Element g = `Ok((signature, used))` with `used[i]` telling whether share i was interpolated, or `Err(status)` with the
/// group's status byte (1 = a bad or repeated id, 3 = a bad commitment, 5 = too few usable partial signatures).  The first
/// t_g decodable partials are tried first and checked with ONE pairing equation under C_0; only a group that fails it has
/// every partial verified against its key share.
pub fn threshold_combine_checked_batch(groups: &[(&[[u8; 128]], &[([u8; 32], [u8; 64])], &[u8])], dst: &[u8]) -> Vec<Result<([u8; 64], Vec<bool>), u8>> {
    let n = groups.len();
    let (mut coff, mut goff) = (Vec::with_capacity(n + 1), Vec::with_capacity(n + 1));
    coff.push(0u64);
    goff.push(0u64);
    let (mut cm, mut id, mut ps): (Vec<u8>, Vec<u8>, Vec<u8>) = (Vec::new(), Vec::new(), Vec::new());
    let mut msgs: Vec<&[u8]> = Vec::with_capacity(n);
    for (commitments, shares, msg) in groups {
        for c in commitments.iter() { cm.extend_from_slice(c); }
        for (i, s) in shares.iter() { id.extend_from_slice(i); ps.extend_from_slice(s); }
        coff.push((cm.len() / 128) as u64);
        goff.push((id.len() / 32) as u64);
        msgs.push(msg);
    }
    let (data, moff) = pack(&msgs);
    let total = id.len() / 32;
    let mut out = vec![0u8; 64 * n];
    let mut used = vec![0u8; (total + 7) / 8];
    let mut status = vec![0u8; n];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_threshold_combine_checked_batch(c, cm.as_ptr(), coff.as_ptr(), id.as_ptr(), ps.as_ptr(), goff.as_ptr(), data.as_ptr(), moff.as_ptr(), n,
                                                      dst.as_ptr(), dst.len(), out.as_mut_ptr(), used.as_mut_ptr(), status.as_mut_ptr())
    }))
    .expect("per-group failures are reported in the status bytes");
    let all = bits(&used, total);
    (0..n).map(|g| match status[g] {
        0 => Ok((out[64 * g..64 * g + 64].try_into().expect("64 bytes"), all[goff[g] as usize..goff[g + 1] as usize].to_vec())),
        st => Err(st),
    }).collect()
}

// ---------------------------------------------------------------- group operators on the crate's own types

/// Body of `impl Mul<Scalar> for G1Projective` (`g1.rs:518-534`, `multiply :821-841`), element-wise over a slice:
/// `out[i] = scalars[i] * points[i]`.  Scalars are the 32-byte big-endian encoding (`scalar.rs:229-233`).
pub fn g1_mul_batch(points: &[G1Affine], scalars: &[[u8; 32]]) -> Result<Vec<G1Affine>, Bn254Error> {
    assert_eq!(points.len(), scalars.len());
    let n = points.len();
    let p: Vec<u8> = points.iter().flat_map(|x| x.to_uncompressed()).collect();
    let k: Vec<u8> = scalars.iter().flatten().copied().collect();
    let mut out = vec![0u8; 64 * n];
    with_ctx(|c| check(unsafe { ffi::blsbn254_g1_mul_batch(c, p.as_ptr(), k.as_ptr(), n, out.as_mut_ptr()) }))?;
    Ok(out.chunks_exact(64).map(|b| Option::<G1Affine>::from(G1Affine::from_uncompressed(b.try_into().unwrap())).expect("engine output is canonical")).collect())
}

/// Body of `impl Mul<Scalar> for G2Projective` (`g2.rs:866-886`), element-wise.
pub fn g2_mul_batch(points: &[G2Affine], scalars: &[[u8; 32]]) -> Result<Vec<G2Affine>, Bn254Error> {
    assert_eq!(points.len(), scalars.len());
    let n = points.len();
    let p: Vec<u8> = points.iter().flat_map(|x| x.to_uncompressed()).collect();
    let k: Vec<u8> = scalars.iter().flatten().copied().collect();
    let mut out = vec![0u8; 128 * n];
    with_ctx(|c| check(unsafe { ffi::blsbn254_g2_mul_batch(c, p.as_ptr(), k.as_ptr(), n, out.as_mut_ptr()) }))?;
    Ok(out.chunks_exact(128).map(|b| Option::<G2Affine>::from(G2Affine::from_uncompressed(b.try_into().unwrap())).expect("engine output is canonical")).collect())
}

/// Body of `impl Sum for G2Projective` (`g2.rs:579-583`) over affine public keys: the aggregate public key.
pub fn aggregate_pks(pks: &[[u8; 128]]) -> Result<[u8; 128], Bn254Error> {
    let flat: Vec<u8> = pks.iter().flatten().copied().collect();
    let mut out = [0u8; 128];
    with_ctx(|c| check(unsafe { ffi::blsbn254_aggregate_pks(c, flat.as_ptr(), pks.len(), out.as_mut_ptr()) }))?;
    Ok(out)
}

/// IETF FastAggregateVerify (min-sig): one message signed by all of `pks` (proof of possession is the caller's precondition).
pub fn fast_aggregate_verify(pks: &[[u8; 128]], msg: &[u8], sig: &[u8; 64], dst: &[u8]) -> bool {
    let flat: Vec<u8> = pks.iter().flatten().copied().collect();
    let mut valid: c_int = 0;
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_fast_aggregate_verify(c, flat.as_ptr(), pks.len(), msg.as_ptr(), msg.len(), sig.as_ptr(), dst.as_ptr(), dst.len(), &mut valid)
    }))
    .expect("invalid inputs yield valid = 0");
    valid == 1
}

/// The same for many (key set, message, signature) groups in one call: `groups[g]` = the keys of group g.
pub fn fast_aggregate_verify_batch(groups: &[&[[u8; 128]]], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(groups.len() == msgs.len() && msgs.len() == sigs.len());
    let n = groups.len();
    let mut koff = Vec::with_capacity(n + 1);
    koff.push(0u64);
    let mut flat: Vec<u8> = Vec::new();
    for g in groups {
        for k in g.iter() { flat.extend_from_slice(k); }
        koff.push((flat.len() / 128) as u64);
    }
    let (data, off) = pack(msgs);
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_fast_aggregate_verify_batch(c, flat.as_ptr(), koff.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), bm.as_mut_ptr())
    }))
    .expect("per-group failures are reported in the bitmap");
    bits(&bm, n)
}

/// Many independent aggregate signatures in one call (`blsbn254_aggregate_verify_batch`): `groups[g]` = the (key, message) pairs
/// of group g, `sigs[g]` its aggregate signature.  Element g = `aggregate_verify` on group g alone; an empty group is invalid.
pub fn aggregate_verify_batch(groups: &[&[([u8; 128], &[u8])]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(groups.len() == sigs.len());
    let n = groups.len();
    let mut goff = Vec::with_capacity(n + 1);
    goff.push(0u64);
    let mut flat: Vec<u8> = Vec::new();
    let mut msgs: Vec<&[u8]> = Vec::new();
    for g in groups {
        for (k, m) in g.iter() { flat.extend_from_slice(k); msgs.push(m); }
        goff.push(msgs.len() as u64);
    }
    let (data, off) = pack(&msgs);
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_aggregate_verify_batch(c, flat.as_ptr(), data.as_ptr(), off.as_ptr(), goff.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), bm.as_mut_ptr())
    }))
    .expect("per-group failures are reported in the bitmap");
    bits(&bm, n)
}

/// `aggregate_verify_batch` by random linear combination across groups (`blsbn254_aggregate_verify_batch_rlc`): the same answers
/// (an invalid range of groups passes its equation with probability at most 2^-64), one Miller loop per DISTINCT key of the call
/// and one final exponentiation where the keys repeat.  The weights are drawn inside the library (OS randomness, after the batch
/// is fixed).
pub fn aggregate_verify_batch_rlc(groups: &[&[([u8; 128], &[u8])]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(groups.len() == sigs.len());
    let n = groups.len();
    let mut goff = Vec::with_capacity(n + 1);
    goff.push(0u64);
    let mut flat: Vec<u8> = Vec::new();
    let mut msgs: Vec<&[u8]> = Vec::new();
    for g in groups {
        for (k, m) in g.iter() { flat.extend_from_slice(k); msgs.push(m); }
        goff.push(msgs.len() as u64);
    }
    let (data, off) = pack(&msgs);
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_aggregate_verify_batch_rlc(c, flat.as_ptr(), data.as_ptr(), off.as_ptr(), goff.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(),
                                                 std::ptr::null(), bm.as_mut_ptr())
    }))
    .expect("per-group failures are reported in the bitmap");
    bits(&bm, n)
}

// ---------------------------------------------------------------- repeated signers: keys prepared once (G2Prepared, batched)

/// The line tables of a set of public keys, resident on the GPU (`blsbn254_g2prepared`): what `G2Prepared::from`
/// (`pairings.rs:614-660`) computes per key, for a whole validator set at once.  Tied to the process-wide engine context.
pub struct PreparedKeys(*mut ffi::PreparedKeys);
unsafe impl Send for PreparedKeys {}

impl PreparedKeys {
    pub fn new(pks: &[[u8; 128]]) -> Self {
        let flat: Vec<u8> = pks.iter().flatten().copied().collect();
        let mut h: *mut ffi::PreparedKeys = core::ptr::null_mut();
        with_ctx(|c| check(unsafe { ffi::blsbn254_g2_prepare_batch(c, flat.as_ptr(), pks.len(), &mut h) })).expect("device error");
        PreparedKeys(h)
    }
    pub fn len(&self) -> usize { unsafe { ffi::blsbn254_g2prepared_count(self.0) } }
}
impl Drop for PreparedKeys {
    fn drop(&mut self) { let _g = engine().lock(); unsafe { ffi::blsbn254_g2prepared_destroy(self.0) } }
}

/// `verify_batch` against prepared keys: tuple i was signed under key `key_idx[i]`.
pub fn verify_batch_prepared(keys: &PreparedKeys, key_idx: &[u32], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(key_idx.len() == msgs.len() && msgs.len() == sigs.len());
    let n = msgs.len();
    let (data, off) = pack(msgs);
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_verify_batch_prepared(c, keys.0, key_idx.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), bm.as_mut_ptr())
    }))
    .expect("key index out of range");
    bits(&bm, n)
}

/// `multi_miller_loop` (`pairings.rs:808-857`) over (G1 point, prepared key) terms.
pub fn multi_miller_loop_prepared(keys: &PreparedKeys, terms: &[(&G1Affine, u32)]) -> Result<MillerLoopResult, Bn254Error> {
    let g1: Vec<u8> = terms.iter().flat_map(|t| t.0.to_uncompressed()).collect();
    let idx: Vec<u32> = terms.iter().map(|t| t.1).collect();
    let mut out = [0u8; 384];
    with_ctx(|c| check(unsafe { ffi::blsbn254_multi_miller_loop_prepared(c, keys.0, idx.as_ptr(), g1.as_ptr(), terms.len(), out.as_mut_ptr()) }))?;
    Ok(MillerLoopResult(Option::<Gt>::from(Gt::from_repr(&out)).expect("engine output is canonical").0))
}

// ---------------------------------------------------------------- a registered committee, signers named by bitmaps

/// A committee's public keys, resident on the GPU (`blsbn254_keyset`): decoded and curve-checked once, then summed per
/// aggregate by a participation bitmap (`ceil(n/8)` bytes per row, bit i LSB-first = key i signed).  Tied to the process-wide
/// engine context.  The second field is the number of stake columns set by `set_weights` (0: none).
pub struct KeySet(*mut ffi::KeySet, usize);
unsafe impl Send for KeySet {}

impl KeySet {
    pub fn new(pks: &[[u8; 128]]) -> Self {
        let flat: Vec<u8> = pks.iter().flatten().copied().collect();
        let mut h: *mut ffi::KeySet = core::ptr::null_mut();
        with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_create(c, flat.as_ptr(), pks.len(), &mut h) })).expect("an empty key set, or a device error");
        KeySet(h, 0)
    }
    /// The same with one proof of possession per key (`blsbn254_keyset_create_checked`), verified under `pop_dst` as
    /// `pop_verify_batch` verifies it: a key whose proof fails is a bad key of the set, as one that does not decode.
    pub fn new_checked(pks: &[[u8; 128]], proofs: &[[u8; 64]], pop_dst: &[u8]) -> Self {
        assert_eq!(pks.len(), proofs.len());
        let flat: Vec<u8> = pks.iter().flatten().copied().collect();
        let pf: Vec<u8> = proofs.iter().flatten().copied().collect();
        let mut h: *mut ffi::KeySet = core::ptr::null_mut();
        with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_create_checked(c, flat.as_ptr(), pf.as_ptr(), pks.len(), pop_dst.as_ptr(), pop_dst.len(), &mut h) }))
            .expect("an empty key set, or a device error");
        KeySet(h, 0)
    }
    pub fn checked(&self) -> bool { unsafe { ffi::blsbn254_keyset_checked(self.0) == 1 } }
    /// 1 to 8 stake columns of `len()` entries each (`blsbn254_keyset_set_weights`); replaces an earlier table.  `Err`: a
    /// column whose sum does not fit 64 bits, and nothing is changed.  A key without the `valid()` bit weighs 0.
    pub fn set_weights(&mut self, columns: &[&[u64]]) -> Result<(), Bn254Error> {
        assert!(columns.iter().all(|col| col.len() == self.len()));
        let flat: Vec<u64> = columns.iter().flat_map(|col| col.iter().copied()).collect();
        with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_set_weights(c, self.0, flat.as_ptr(), columns.len()) }))?;
        self.1 = columns.len();
        Ok(())
    }
    pub fn cols(&self) -> usize { self.1 }
    /// The columns' sums over the keys that have the `valid()` bit.
    pub fn total_weight(&self) -> Vec<u64> {
        let mut out = vec![0u64; 8];
        with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_total_weight(c, self.0, out.as_mut_ptr()) })).expect("no weights set");
        out.truncate(self.1);
        out
    }
    pub fn len(&self) -> usize { unsafe { ffi::blsbn254_keyset_count(self.0) } }
    /// KeyValidate per registered key (decodes, not the identity, on the curve, in the r-torsion): for the registrar.
    pub fn valid(&self) -> Vec<bool> {
        let n = self.len();
        let mut bm = vec![0u8; (n + 7) / 8];
        with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_valid(c, self.0, bm.as_mut_ptr()) })).expect("device error");
        bits(&bm, n)
    }
}
impl Drop for KeySet {
    fn drop(&mut self) { let _g = engine().lock(); unsafe { ffi::blsbn254_keyset_destroy(self.0) } }
}

/// `impl Sum for G2Projective` (`g2.rs:579-583`) over the keys each row selects: element g = `Some(aggregate key)`, or `None`
/// when the row selects a key that does not decode or is off the curve.
pub fn keyset_sum_batch(keys: &KeySet, rows: &[&[u8]]) -> Vec<Option<[u8; 128]>> {
    let n = rows.len();
    let sel: Vec<u8> = rows.iter().flat_map(|r| r.iter().copied()).collect();
    assert_eq!(sel.len(), n * ((keys.len() + 7) / 8));
    let mut out = vec![0u8; 128 * n];
    let mut status = vec![0u8; n];
    with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_sum_batch(c, keys.0, sel.as_ptr(), n, out.as_mut_ptr(), status.as_mut_ptr()) }))
        .expect("a padding bit is set");
    (0..n).map(|g| if status[g] == 1 { Some(out[128 * g..128 * g + 128].try_into().expect("128 bytes")) } else { None }).collect()
}

/// `fast_aggregate_verify_batch` with every group's keys named by a bitmap over a registered set.
pub fn keyset_fast_aggregate_verify_batch(keys: &KeySet, rows: &[&[u8]], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(rows.len() == msgs.len() && msgs.len() == sigs.len());
    let n = rows.len();
    let sel: Vec<u8> = rows.iter().flat_map(|r| r.iter().copied()).collect();
    assert_eq!(sel.len(), n * ((keys.len() + 7) / 8));
    let (data, off) = pack(msgs);
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_keyset_fast_aggregate_verify_batch(c, keys.0, sel.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), bm.as_mut_ptr())
    }))
    .expect("a padding bit is set");
    bits(&bm, n)
}

/// The stake each row selects (`blsbn254_keyset_weight_batch`): element g = one sum per column of the set's table.
pub fn keyset_weight_batch(keys: &KeySet, rows: &[&[u8]]) -> Vec<Vec<u64>> {
    let (n, nc) = (rows.len(), keys.cols());
    let sel: Vec<u8> = rows.iter().flat_map(|r| r.iter().copied()).collect();
    assert_eq!(sel.len(), n * ((keys.len() + 7) / 8));
    let mut out = vec![0u64; n * nc];
    with_ctx(|c| check(unsafe { ffi::blsbn254_keyset_weight_batch(c, keys.0, sel.as_ptr(), n, out.as_mut_ptr()) })).expect("no weights set, or a padding bit is set");
    out.chunks(nc.max(1)).take(n).map(|w| w.to_vec()).collect()
}

/// `keyset_fast_aggregate_verify_batch` with a quorum (`blsbn254_keyset_quorum_verify_batch`): element g = (the group carries
/// at least `min_weight[q]` in every column AND its aggregate verifies, its weights).  Groups below the quorum are neither
/// summed nor paired.
pub fn keyset_quorum_verify_batch(keys: &KeySet, rows: &[&[u8]], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8], min_weight: &[u64]) -> Vec<(bool, Vec<u64>)> {
    assert!(rows.len() == msgs.len() && msgs.len() == sigs.len() && min_weight.len() == keys.cols());
    let (n, nc) = (rows.len(), keys.cols());
    let sel: Vec<u8> = rows.iter().flat_map(|r| r.iter().copied()).collect();
    assert_eq!(sel.len(), n * ((keys.len() + 7) / 8));
    let (data, off) = pack(msgs);
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    let mut w = vec![0u64; n * nc];
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_keyset_quorum_verify_batch(c, keys.0, sel.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), min_weight.as_ptr(),
                                                 w.as_mut_ptr(), bm.as_mut_ptr())
    }))
    .expect("no weights set, or a padding bit is set");
    bits(&bm, n).into_iter().zip(w.chunks(nc.max(1))).map(|(b, x)| (b, x.to_vec())).collect()
}

/// What the node that collects a committee's individual signatures hands on (`blsbn254_keyset_aggregate_checked_batch`):
/// `entries[g]` = the `(key index, signature)` pairs received for `msgs[g]`, sorted here by index (a repeated index panics).
/// Element g = `Some((aggregate signature, participation row))`, which `keyset_fast_aggregate_verify_batch` accepts for the
/// message, or `None` when nothing usable is left (`BLSBN254_ST_SHORT`).  Bad signatures are left out, never an error.
pub fn keyset_aggregate_checked_batch(keys: &KeySet, entries: &[Vec<(u32, [u8; 64])>], msgs: &[&[u8]], dst: &[u8]) -> Vec<Option<([u8; 64], Vec<u8>)>> {
    assert_eq!(entries.len(), msgs.len());
    let n = msgs.len();
    let rb = (keys.len() + 7) / 8;
    let (mut idx, mut sg, mut soff) = (Vec::<u32>::new(), Vec::<u8>::new(), vec![0u64]);
    for e in entries {
        let mut e = e.clone();
        e.sort_by_key(|p| p.0);
        assert!(e.windows(2).all(|w| w[0].0 < w[1].0), "a key index is repeated");
        for (k, s) in &e { idx.push(*k); sg.extend_from_slice(s); }
        soff.push(idx.len() as u64);
    }
    let (data, moff) = pack(msgs);
    let (mut out, mut sel, mut status) = (vec![0u8; 64 * n], vec![0u8; rb * n], vec![0u8; n]);
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_keyset_aggregate_checked_batch(c, keys.0, idx.as_ptr(), sg.as_ptr(), soff.as_ptr(), data.as_ptr(), moff.as_ptr(), n, dst.as_ptr(), dst.len(),
                                                     out.as_mut_ptr(), sel.as_mut_ptr(), status.as_mut_ptr())
    }))
    .expect("a key index names no key of the set");
    (0..n).map(|g| if status[g] == 0 { Some((out[64 * g..64 * g + 64].try_into().expect("64 bytes"), sel[rb * g..rb * g + rb].to_vec())) } else { None }).collect()
}

/// `keyset_aggregate_checked_batch` per committee of the handle's table (`blsbn254_keyset_committee_aggregate_checked_batch`):
/// `groups[g]` = `(committee, its number of members, the (position in its member list, signature) pairs received for msgs[g])`,
/// sorted here by position (a repeated position panics).  Element g = `Some((aggregate signature, participation row of
/// ceil(members / 8) bytes))`, the row and signature the committee form of the verify accepts for the message, or `None` when
/// nothing usable is left (`BLSBN254_ST_SHORT`).  Bad signatures are left out, never an error.
pub fn keyset_committee_aggregate_checked_batch(keys: &KeySet, groups: &[(u32, usize, Vec<(u32, [u8; 64])>)], msgs: &[&[u8]], dst: &[u8])
    -> Vec<Option<([u8; 64], Vec<u8>)>> {
    assert_eq!(groups.len(), msgs.len());
    let n = msgs.len();
    let (mut com, mut pos, mut sg, mut soff, mut roff) = (Vec::<u32>::new(), Vec::<u32>::new(), Vec::<u8>::new(), vec![0u64], vec![0u64]);
    for (c, size, e) in groups {
        let mut e = e.clone();
        e.sort_by_key(|p| p.0);
        assert!(e.windows(2).all(|w| w[0].0 < w[1].0), "a position is repeated");
        for (k, s) in &e { pos.push(*k); sg.extend_from_slice(s); }
        com.push(*c);
        soff.push(pos.len() as u64);
        roff.push(roff[roff.len() - 1] + ((size + 7) / 8) as u64);
    }
    let (data, moff) = pack(msgs);
    let (mut out, mut sel, mut status) = (vec![0u8; 64 * n], vec![0u8; roff[n] as usize], vec![0u8; n]);
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_keyset_committee_aggregate_checked_batch(c, keys.0, com.as_ptr(), pos.as_ptr(), sg.as_ptr(), soff.as_ptr(), data.as_ptr(), moff.as_ptr(),
                                                               roff.as_ptr(), n, dst.as_ptr(), dst.len(), out.as_mut_ptr(), sel.as_mut_ptr(), status.as_mut_ptr())
    }))
    .expect("no committee table, a committee or position out of range, or a wrong member count");
    (0..n).map(|g| if status[g] == 0 {
        Some((out[64 * g..64 * g + 64].try_into().expect("64 bytes"), sel[roff[g] as usize..roff[g + 1] as usize].to_vec()))
    } else { None }).collect()
}

/// What an intermediate node of an aggregation tree hands on (`blsbn254_keyset_merge_checked_batch`): `contributions[g]` =
/// the partial aggregates received for `msgs[g]`, each a `(row, signature)` pair with a row of `ceil(keys.len() / 8)` bytes,
/// in the order of their priority (kept).  Element g = `Some((merged signature, merged row, used flag per contribution))`,
/// which `keyset_fast_aggregate_verify_batch` accepts for the message, or `None` when nothing usable is left
/// (`BLSBN254_ST_SHORT`).  Selection is greedy over disjoint rows; bad contributions are left out, never an error.
pub fn keyset_merge_checked_batch(keys: &KeySet, contributions: &[Vec<(Vec<u8>, [u8; 64])>], msgs: &[&[u8]], dst: &[u8]) -> Vec<Option<([u8; 64], Vec<u8>, Vec<bool>)>> {
    assert_eq!(contributions.len(), msgs.len());
    let n = msgs.len();
    let rb = (keys.len() + 7) / 8;
    let (mut rows, mut sg, mut coff) = (Vec::<u8>::new(), Vec::<u8>::new(), vec![0u64]);
    for cs in contributions {
        for (r, s) in cs {
            assert_eq!(r.len(), rb, "a row is ceil(n_keys / 8) bytes");
            rows.extend_from_slice(r); sg.extend_from_slice(s);
        }
        coff.push((sg.len() / 64) as u64);
    }
    let total = sg.len() / 64;
    let (data, moff) = pack(msgs);
    let (mut out, mut sel, mut used, mut status) = (vec![0u8; 64 * n], vec![0u8; rb * n], vec![0u8; (total + 7) / 8], vec![0u8; n]);
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_keyset_merge_checked_batch(c, keys.0, rows.as_ptr(), sg.as_ptr(), coff.as_ptr(), data.as_ptr(), moff.as_ptr(), n, dst.as_ptr(), dst.len(),
                                                 out.as_mut_ptr(), sel.as_mut_ptr(), used.as_mut_ptr(), status.as_mut_ptr())
    }))
    .expect("a padding bit is set");
    (0..n).map(|g| if status[g] == 0 {
        let flags = (coff[g] as usize..coff[g + 1] as usize).map(|s| (used[s >> 3] >> (s & 7)) & 1 == 1).collect();
        Some((out[64 * g..64 * g + 64].try_into().expect("64 bytes"), sel[rb * g..rb * g + rb].to_vec(), flags))
    } else { None }).collect()
}

/// `keyset_merge_checked_batch` per committee of the handle's table (`blsbn254_keyset_committee_merge_checked_batch`):
/// `groups[g]` = `(committee, its number of members, the (row, signature) pairs received for msgs[g])`, a row being
/// `ceil(members / 8)` bytes with bit j = member j of the committee, in the order of their priority (kept).  The pairs
/// `keyset_committee_aggregate_checked_batch` hands out are contributions of this call as they are.  Element g =
/// `Some((merged signature, merged row of ceil(members / 8) bytes, used flag per contribution))`, the row and signature the
/// committee form of the verify accepts for the message, or `None` when nothing usable is left (`BLSBN254_ST_SHORT`).
/// Selection is greedy over disjoint rows; bad contributions are left out, never an error.
pub fn keyset_committee_merge_checked_batch(keys: &KeySet, groups: &[(u32, usize, Vec<(Vec<u8>, [u8; 64])>)], msgs: &[&[u8]], dst: &[u8])
    -> Vec<Option<([u8; 64], Vec<u8>, Vec<bool>)>> {
    assert_eq!(groups.len(), msgs.len());
    let n = msgs.len();
    let (mut com, mut rows, mut sg) = (Vec::<u32>::new(), Vec::<u8>::new(), Vec::<u8>::new());
    let (mut coff, mut roff, mut soff) = (vec![0u64], vec![0u64], vec![0u64]);
    for (c, size, cs) in groups {
        let rb = (size + 7) / 8;
        for (r, s) in cs {
            assert_eq!(r.len(), rb, "a row is ceil(members / 8) bytes");
            rows.extend_from_slice(r); sg.extend_from_slice(s);
        }
        com.push(*c);
        coff.push((sg.len() / 64) as u64);
        roff.push(rows.len() as u64);
        soff.push(soff[soff.len() - 1] + rb as u64);
    }
    let total = sg.len() / 64;
    let (data, moff) = pack(msgs);
    let (mut out, mut sel, mut used, mut status) = (vec![0u8; 64 * n], vec![0u8; soff[n] as usize], vec![0u8; (total + 7) / 8], vec![0u8; n]);
    with_ctx(|c| check(unsafe {
        ffi::blsbn254_keyset_committee_merge_checked_batch(c, keys.0, com.as_ptr(), rows.as_ptr(), roff.as_ptr(), sg.as_ptr(), coff.as_ptr(), data.as_ptr(),
                                                           moff.as_ptr(), soff.as_ptr(), n, dst.as_ptr(), dst.len(), out.as_mut_ptr(), sel.as_mut_ptr(),
                                                           used.as_mut_ptr(), status.as_mut_ptr())
    }))
    .expect("no committee table, a committee out of range, a wrong member count, or a padding bit is set");
    (0..n).map(|g| if status[g] == 0 {
        let flags = (coff[g] as usize..coff[g + 1] as usize).map(|s| (used[s >> 3] >> (s & 7)) & 1 == 1).collect();
        Some((out[64 * g..64 * g + 64].try_into().expect("64 bytes"), sel[soff[g] as usize..soff[g + 1] as usize].to_vec(), flags))
    } else { None }).collect()
}

// ---------------------------------------------------------------- N GPUs of one node

/// All GPUs named in `BLSBN254_DEVICES` (comma-separated HIP ordinals, default "0"): one context and one host thread per
/// GPU inside the library, contiguous shards, no data-path collective (`blsbn254_multi`).
struct MultiEngine(*mut ffi::Multi);
unsafe impl Send for MultiEngine {}

fn multi_engine() -> &'static Mutex<MultiEngine> {
    static ENGINE: OnceLock<Mutex<MultiEngine>> = OnceLock::new();
    ENGINE.get_or_init(|| {
        let devs: Vec<c_int> = std::env::var("BLSBN254_DEVICES").unwrap_or_else(|_| "0".into())
            .split(',').filter_map(|s| s.trim().parse::<c_int>().ok()).collect();
        let mut m: *mut ffi::Multi = core::ptr::null_mut();
        let rc = unsafe { ffi::blsbn254_multi_create(devs.as_ptr(), devs.len() as c_int, &mut m) };
        assert!(rc == 0 && !m.is_null(), "blsbn254_multi_create failed with code {rc}");
        Mutex::new(MultiEngine(m))
    })
}

/// `verify_batch` sharded over every configured GPU; same result as the single-GPU call.
pub fn verify_batch_multi(pks: &[[u8; 128]], msgs: &[&[u8]], sigs: &[[u8; 64]], dst: &[u8]) -> Vec<bool> {
    assert!(pks.len() == msgs.len() && msgs.len() == sigs.len());
    let n = pks.len();
    let (data, off) = pack(msgs);
    let pk: Vec<u8> = pks.iter().flatten().copied().collect();
    let sg: Vec<u8> = sigs.iter().flatten().copied().collect();
    let mut bm = vec![0u8; (n + 7) / 8];
    let guard = multi_engine().lock().expect("engine mutex poisoned");
    check(unsafe {
        ffi::blsbn254_verify_batch_multi(guard.0, pk.as_ptr(), data.as_ptr(), off.as_ptr(), sg.as_ptr(), n, dst.as_ptr(), dst.len(), bm.as_mut_ptr())
    })
    .expect("per-tuple failures are reported in the bitmap");
    bits(&bm, n)
}

/// `aggregate_verify` sharded over every configured GPU (per-GPU Fp12 partial products, one final exponentiation).
pub fn aggregate_verify_multi(pks: &[[u8; 128]], msgs: &[&[u8]], agg_sig: &[u8; 64], dst: &[u8]) -> bool {
    assert_eq!(pks.len(), msgs.len());
    let (data, off) = pack(msgs);
    let pk: Vec<u8> = pks.iter().flatten().copied().collect();
    let mut valid: c_int = 0;
    let guard = multi_engine().lock().expect("engine mutex poisoned");
    check(unsafe {
        ffi::blsbn254_aggregate_verify_multi(guard.0, pk.as_ptr(), data.as_ptr(), off.as_ptr(), pks.len(), agg_sig.as_ptr(), dst.as_ptr(), dst.len(), &mut valid)
    })
    .expect("invalid inputs yield valid = 0");
    valid == 1
}

#[cfg(test)]
mod tests {
    use super::*;
    use elliptic_curve::Group;

    /// The crate's own `pairing_test` (`pairings.rs:971-980`), which fails on the CPU path today.
    #[test]
    fn pairing_of_generators_is_gt_generator() {
        let gt = pairing(&G1Affine::generator(), &G2Affine::generator());
        assert_eq!(gt, Gt::generator());
        let r_gt = final_exponentiation(&multi_miller_loop(&[(&G1Affine::generator(), &G2Prepared(G2Affine::generator()))]));
        assert_eq!(r_gt, gt);
    }
}
