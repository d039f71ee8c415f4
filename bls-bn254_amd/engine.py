"""ctypes binding of the C ABI (include/blsbn254.h) with the reference crate's operator names.

Mirrors, for the hot path, the interface a user of mikelodder7/bls-bn254 sees:
pairing / multi_miller_loop / final_exponentiation (pairings.rs:760-857, :50-178),
G1Projective::hash / encode, G2Projective::hash / encode (g1.rs:910-928, g2.rs:919-936),
is_on_curve / is_torsion_free (g1.rs:383-391, g2.rs:409-414, :733-736), Sum (g1.rs:561-565), and the
Bn254Error variants (error.rs:4-10) as exceptions.  Everything runs on the GPU through
libblsbn254_hip.so; if the library or a gfx950 device is missing the calls raise -- there is no CPU
path in this package.
"""
import ctypes
import threading
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_DST = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"
ST_SHORT = 5           # BLSBN254_ST_SHORT: a per-group status of threshold_combine_checked_batch, never an exception
POP_DST = b"BLS_POP_BN254G1_XMD:SHA-256_SVDW_RO_POP_"
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_lib = None


class Bn254Error(Exception):
    """Mirror of the reference's error enum (error.rs:4-10) plus device errors (negative codes)."""
    code = None

    def __init__(self, code, detail=""):
        self.code = code
        msg = load_library().blsbn254_strerror(code).decode()
        super().__init__("%s (code %d)%s" % (msg, code, (": " + detail) if detail else ""))


class InvalidScalarBytes(Bn254Error):
    pass


class InvalidG1Bytes(Bn254Error):
    pass


class InvalidG2Bytes(Bn254Error):
    pass


class InvalidGtBytes(Bn254Error):
    pass


_ERR = {1: InvalidScalarBytes, 2: InvalidG1Bytes, 3: InvalidG2Bytes, 4: InvalidGtBytes}


def library_path():
    # BLSBN254_LIB selects another build of the SAME HIP library (A/B of compile options); never a fallback
    return os.environ.get("BLSBN254_LIB") or os.path.join(HERE, "libblsbn254_hip.so")


def load_library():
    """Loads the HIP extension.  Fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError("HIP extension %s is missing: run `python -m bls_bn254_amd.build` "
                               "(or __graft_entry__.build()); there is no CPU fallback" % path)
        # torch ships its own HIP runtime with the same SONAME as /opt/rocm's: whichever is loaded first
        # serves the whole process, and torch only finds its GPUs through its own copy.  Load torch's
        # first when it is installed so that the extension and torch share one runtime (plumbing only).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = ctypes.CDLL(path)
        lib.blsbn254_strerror.restype = ctypes.c_char_p
        lib.blsbn254_last_error.restype = ctypes.c_char_p
        lib.blsbn254_ctx_stream.restype = ctypes.c_void_p
        _lib = lib
    return _lib


def _inbuf(b, expect=None):
    if isinstance(b, np.ndarray):
        a = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    else:
        a = np.frombuffer(bytes(b), dtype=np.uint8)
    if expect is not None and a.size != expect:
        raise ValueError("expected %d bytes, got %d" % (expect, a.size))
    if a.size == 0:
        a = np.zeros(1, dtype=np.uint8)
    return a, a.ctypes.data_as(_u8p)


_BIG_OUT = threading.local()


def _outbuf(n):
    """Host buffer for a call's output.  Every caller copies its result out (tobytes) before returning, so large outputs share
    one grow-only buffer per thread: a fresh multi-megabyte allocation per call is untouched mmap'ed memory, and the device-to-host
    copy into it then pays the page faults and the pinning (measured: pairing_batch(8192) 5 ms -> 24 ms depending on the
    allocator's history)."""
    if n >= (1 << 18):
        a = getattr(_BIG_OUT, "buf", None)
        if a is None or a.size < n:
            a = np.zeros(n + n // 4, dtype=np.uint8)
            _BIG_OUT.buf = a
        return a, a.ctypes.data_as(_u8p)
    a = np.zeros(max(n, 1), dtype=np.uint8)
    return a, a.ctypes.data_as(_u8p)


def pack_messages(msgs):
    """list of bytes -> (concatenated bytes, n+1 uint64 offsets)"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return b"".join(msgs), off


class Engine:
    """One context = one GPU (blsbn254_ctx): stream, workspace, resident -G2gen line table."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.blsbn254_ctx_create(ctypes.c_int(device), ctypes.byref(self._ctx))
        if rc != 0:
            self._ctx = None
            raise Bn254Error(rc)
        self.device = device

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.blsbn254_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            detail = self._lib.blsbn254_last_error(self._ctx).decode() if rc == -2 else ""
            raise _ERR.get(rc, Bn254Error)(rc, detail)

    # ---- primitives (reference operator API)
    def pairing_batch(self, g1, g2, n):
        a, pa = _inbuf(g1, 64 * n); b, pb = _inbuf(g2, 128 * n); o, po = _outbuf(384 * n)
        self._chk(self._lib.blsbn254_pairing_batch(self._ctx, pa, pb, ctypes.c_size_t(n), po))
        return o[:384 * n].tobytes()

    def pairing(self, g1, g2):
        return self.pairing_batch(g1, g2, 1)

    def miller_loop_batch(self, g1, g2, n):
        a, pa = _inbuf(g1, 64 * n); b, pb = _inbuf(g2, 128 * n); o, po = _outbuf(384 * n)
        self._chk(self._lib.blsbn254_miller_loop_batch(self._ctx, pa, pb, ctypes.c_size_t(n), po))
        return o[:384 * n].tobytes()

    def multi_miller_loop(self, g1, g2, n):
        a, pa = _inbuf(g1, 64 * n); b, pb = _inbuf(g2, 128 * n); o, po = _outbuf(384)
        self._chk(self._lib.blsbn254_multi_miller_loop(self._ctx, pa, pb, ctypes.c_size_t(n), po))
        return o.tobytes()

    @staticmethod
    def _eq_offsets(off):
        o = np.ascontiguousarray(np.asarray(off, dtype=np.uint64).reshape(-1))
        if o.size == 0:
            raise ValueError("equation offsets need n_eq + 1 entries")
        return o, o.size - 1, int(o.max())

    def multi_miller_loop_batch(self, g1, g2, off):
        """n_eq multi_miller_loop products (pairings.rs:808-857): equation g owns the pairs off[g] .. off[g + 1] of the
        concatenated points g1 (64 B each) / g2 (128 B each).  Returns n_eq x 384 bytes."""
        o, n_eq, npairs = self._eq_offsets(off)
        a, pa = _inbuf(g1, 64 * npairs); b, pb = _inbuf(g2, 128 * npairs); r, pr = _outbuf(384 * n_eq)
        self._chk(self._lib.blsbn254_multi_miller_loop_batch(self._ctx, pa, pb, o.ctypes.data_as(_u64p), ctypes.c_size_t(n_eq), pr))
        return r[:384 * n_eq].tobytes()

    def pairing_check_batch(self, g1, g2, off):
        """Bit g (LSB-first) = prod_{j in equation g} e(P_j, Q_j) == 1 with every member a valid point (P on the curve, Q on the
        curve and in the r-torsion; identities allowed).  Same arguments as multi_miller_loop_batch; returns the bitmap bytes."""
        o, n_eq, npairs = self._eq_offsets(off)
        a, pa = _inbuf(g1, 64 * npairs); b, pb = _inbuf(g2, 128 * npairs); r, pr = _outbuf((n_eq + 7) // 8)
        self._chk(self._lib.blsbn254_pairing_check_batch(self._ctx, pa, pb, o.ctypes.data_as(_u64p), ctypes.c_size_t(n_eq), pr))
        return r[:(n_eq + 7) // 8].tobytes()

    def final_exponentiation(self, ml, n=1):
        a, pa = _inbuf(ml, 384 * n); o, po = _outbuf(384 * n)
        self._chk(self._lib.blsbn254_final_exponentiation(self._ctx, pa, ctypes.c_size_t(n), po))
        return o[:384 * n].tobytes()

    def _h2c(self, fn, msgs, dst, size):
        data, off = pack_messages(msgs)
        a, pa = _inbuf(data); d, pd = _inbuf(dst); o, po = _outbuf(size * len(msgs))
        self._chk(fn(self._ctx, pa, off.ctypes.data_as(_u64p), ctypes.c_size_t(len(msgs)), pd, ctypes.c_size_t(len(dst)), po))
        return o[:size * len(msgs)].tobytes()

    def hash_to_g1_batch(self, msgs, dst): return self._h2c(self._lib.blsbn254_hash_to_g1_batch, msgs, dst, 64)
    def encode_to_g1_batch(self, msgs, dst): return self._h2c(self._lib.blsbn254_encode_to_g1_batch, msgs, dst, 64)
    def hash_to_g2_batch(self, msgs, dst): return self._h2c(self._lib.blsbn254_hash_to_g2_batch, msgs, dst, 128)
    def encode_to_g2_batch(self, msgs, dst): return self._h2c(self._lib.blsbn254_encode_to_g2_batch, msgs, dst, 128)

    def g1_check_batch(self, g1, n):
        a, pa = _inbuf(g1, 64 * n); o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_g1_check_batch(self._ctx, pa, ctypes.c_size_t(n), po))
        return o[:(n + 7) // 8].tobytes()

    def g2_check_batch(self, g2, n):
        a, pa = _inbuf(g2, 128 * n); o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_g2_check_batch(self._ctx, pa, ctypes.c_size_t(n), po))
        return o[:(n + 7) // 8].tobytes()

    # ---- BLS layer
    def verify_batch(self, pks, msgs, sigs, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * n); d, pd = _inbuf(dst)
        o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd,
                                                  ctypes.c_size_t(len(dst)), po))
        return o[:(n + 7) // 8].tobytes()

    def verify_batch_compressed(self, pks, msgs, sigs, dst=DEFAULT_DST):
        """verify_batch on compressed operands (64 bytes per key, 32 per signature): the bitmap verify_batch gives on the outputs
        of g2_inflate_batch / g1_inflate_batch, inflated on the device; a key or signature that does not inflate clears its bit."""
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 64 * n); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 32 * n); d, pd = _inbuf(dst)
        o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch_compressed(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd,
                                                             ctypes.c_size_t(len(dst)), po))
        return o[:(n + 7) // 8].tobytes()

    def set_async_verify(self, on):
        """verify_batch_dev enqueues on the previous call's key count without reading the new one back first (default on)"""
        self._chk(self._lib.blsbn254_set_async_verify(self._ctx, ctypes.c_int(1 if on else 0)))

    def async_stats(self):
        """(chunks enqueued on the assumption that the key set repeats, how many of them had to be re-run)"""
        o = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.blsbn254_async_stats(self._ctx, o))
        return int(o[0]), int(o[1])

    def set_auto_prepare(self, on):
        """verify_batch's automatic key de-duplication + per-key preparation (default on); off = exact per-tuple path."""
        self._chk(self._lib.blsbn254_set_auto_prepare(self._ctx, ctypes.c_int(1 if on else 0)))

    def set_key_cache(self, max_keys):
        """size (in keys) of the context's store of prepared keys; 0 = off: every call prepares its keys.  Empties the store."""
        self._chk(self._lib.blsbn254_set_key_cache(self._ctx, ctypes.c_size_t(max_keys)))

    def key_cache_stats(self):
        """(keys found resident, keys prepared, times the store was emptied for a batch that did not fit, keys resident now)"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_key_cache_stats(self._ctx, o))
        return int(o[0]), int(o[1]), int(o[2]), int(o[3])

    def path_stats(self):
        """(chunks served by the prepared-key path, chunks served by the exact per-tuple path)"""
        o = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.blsbn254_path_stats(self._ctx, o))
        return int(o[0]), int(o[1])

    def g2_prepare_batch(self, pks, u):
        """G2Prepared::from (pairings.rs:609-660) for u keys: a device-resident table handle (PreparedKeys)."""
        return PreparedKeys(self, pks, u)

    def verify_batch_prepared(self, keys, key_idx, msgs, sigs, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        idx = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32))
        if idx.size != n:
            raise ValueError("one key index per tuple")
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * n); d, pd = _inbuf(dst); o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch_prepared(self._ctx, keys._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), pm,
                                                           off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd, ctypes.c_size_t(len(dst)), po))
        return o[:(n + 7) // 8].tobytes()

    def multi_miller_loop_prepared(self, keys, key_idx, g1, n):
        """multi_miller_loop over (G1 point, prepared key) terms (pairings.rs:808-857): 384-byte Miller product."""
        idx = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32))
        if idx.size != n:
            raise ValueError("one key index per pair")
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        a, pa = _inbuf(g1, 64 * n); o, po = _outbuf(384)
        self._chk(self._lib.blsbn254_multi_miller_loop_prepared(self._ctx, keys._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), pa,
                                                                ctypes.c_size_t(n), po))
        return o.tobytes()

    def aggregate_verify_prepared(self, keys, key_idx, msgs, agg_sig, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        idx = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32))
        if idx.size != n:
            raise ValueError("one key index per pair")
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        m, pm = _inbuf(data); s, ps = _inbuf(agg_sig, 64); d, pd = _inbuf(dst)
        valid = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_aggregate_verify_prepared(self._ctx, keys._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), pm,
                                                               off.ctypes.data_as(_u64p), ctypes.c_size_t(n), ps, pd, ctypes.c_size_t(len(dst)),
                                                               ctypes.byref(valid)))
        return bool(valid.value)

    def verify_batch_rlc(self, pks, msgs, sigs, dst=DEFAULT_DST, seed=None):
        """Same bitmap as verify_batch, via random linear combinations (one final exponentiation per 16 tuples,
        exact re-verification of failing groups).  seed = None: the library draws it from the OS inside the call
        (production); a caller seed is for reproducible tests only."""
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * n); d, pd = _inbuf(dst)
        if seed is None:
            sd, psd = None, ctypes.cast(None, _u8p)
        else:
            sd, psd = _inbuf(seed, 32)
        o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch_rlc(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd,
                                                      ctypes.c_size_t(len(dst)), psd, po))
        return o[:(n + 7) // 8].tobytes()

    def verify_batch_rlc_compressed(self, pks, msgs, sigs, dst=DEFAULT_DST, seed=None):
        """verify_batch_rlc on compressed operands (64 bytes per key, 32 per signature); seed as there."""
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 64 * n); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 32 * n); d, pd = _inbuf(dst)
        sd, psd = self._seed_arg(seed)
        o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch_rlc_compressed(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd,
                                                                 ctypes.c_size_t(len(dst)), psd, po))
        return o[:(n + 7) // 8].tobytes()

    def aggregate_path_stats(self):
        """(aggregate_verify calls served by per-key sums, calls served pair by pair)"""
        o = (ctypes.c_uint64 * 2)()
        self._chk(self._lib.blsbn254_aggregate_path_stats(self._ctx, o))
        return int(o[0]), int(o[1])

    def set_rlc_group(self, group):
        """tuples per chunk of the repeated-key RLC path; 0 = automatic (16, raised when that saves a round of waves)"""
        self._chk(self._lib.blsbn254_set_rlc_group(self._ctx, ctypes.c_size_t(group)))

    def rlc_stats(self):
        """dict: tuples verified through chunks, chunks checked, tuples re-verified exactly, tuples of distinct-key batches"""
        o = (ctypes.c_uint64 * 6)()
        self._chk(self._lib.blsbn254_rlc_stats(self._ctx, o))
        return {"chunked_tuples": int(o[0]), "chunks": int(o[1]), "fallback_tuples": int(o[2]), "distinct_key_tuples": int(o[3]),
                "key_rounds": int(o[4]), "key_rounds_passed": int(o[5])}

    def set_rlc_key_round(self, on):
        """RLC: check every key's whole run as one virtual tuple first (default on)"""
        self._chk(self._lib.blsbn254_set_rlc_key_round(self._ctx, ctypes.c_int(1 if on else 0)))

    def aggregate_verify(self, pks, msgs, agg_sig, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); s, ps = _inbuf(agg_sig, 64); d, pd = _inbuf(dst)
        valid = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_aggregate_verify(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ctypes.c_size_t(n), ps, pd,
                                                      ctypes.c_size_t(len(dst)), ctypes.byref(valid)))
        return bool(valid.value)

    def aggregate_partial(self, pks, msgs, dst=DEFAULT_DST):
        """(384-byte Fp12 partial product of ML(H(msg_i), pk_i), all public keys valid?) for one shard."""
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); d, pd = _inbuf(dst); o, po = _outbuf(384)
        ok = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_aggregate_partial(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ctypes.c_size_t(n), pd,
                                                       ctypes.c_size_t(len(dst)), po, ctypes.byref(ok)))
        return o.tobytes(), bool(ok.value)

    def aggregate_partial_with_sig(self, pks, msgs, agg_sig, dst=DEFAULT_DST):
        """(partial product times ML(agg_sig, -G2gen), all public keys valid?, signature valid?): the shard that carries
        the aggregate signature's pair; finish with aggregate_finish(partials, k, None)."""
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); d, pd = _inbuf(dst); s, ps = _inbuf(agg_sig, 64); o, po = _outbuf(384)
        ok = ctypes.c_int(0); sok = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_aggregate_partial_with_sig(self._ctx, pa, pm, off.ctypes.data_as(_u64p), ctypes.c_size_t(n), pd,
                                                                ctypes.c_size_t(len(dst)), ps, po, ctypes.byref(ok), ctypes.byref(sok)))
        return o.tobytes(), bool(ok.value), bool(sok.value)

    def aggregate_finish(self, partials, k, agg_sig):
        a, pa = _inbuf(partials, 384 * k)
        if agg_sig is None:
            s, ps = None, ctypes.cast(None, _u8p)
        else:
            s, ps = _inbuf(agg_sig, 64)
        valid = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_aggregate_finish(self._ctx, pa, ctypes.c_size_t(k), ps, ctypes.byref(valid)))
        return bool(valid.value)

    def aggregate_sigs(self, sigs, n):
        a, pa = _inbuf(sigs, 64 * n); o, po = _outbuf(64)
        self._chk(self._lib.blsbn254_aggregate_sigs(self._ctx, pa, ctypes.c_size_t(n), po))
        return o.tobytes()

    def aggregate_pks(self, pks, n):
        """impl Sum for G2Projective (g2.rs:579-583): the sum of n public keys, 128 bytes."""
        a, pa = _inbuf(pks, 128 * n); o, po = _outbuf(128)
        self._chk(self._lib.blsbn254_aggregate_pks(self._ctx, pa, ctypes.c_size_t(n), po))
        return o[:128].tobytes()

    def fast_aggregate_verify(self, pks, n, msg, sig, dst=DEFAULT_DST):
        """One message signed by n keys: e(sig, -G2gen) * e(H(msg), sum pk_i) == 1."""
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(msg); s, ps = _inbuf(sig, 64); d, pd = _inbuf(dst)
        valid = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_fast_aggregate_verify(self._ctx, pa, ctypes.c_size_t(n), pm, ctypes.c_size_t(len(msg)), ps, pd,
                                                           ctypes.c_size_t(len(dst)), ctypes.byref(valid)))
        return bool(valid.value)

    def fast_aggregate_verify_batch(self, key_sets, msgs, sigs, dst=DEFAULT_DST):
        """key_sets: list of byte strings (each a multiple of 128 bytes: the keys of one group); msgs: one message per group;
        sigs: 64 bytes per group.  Returns the LSB-first bitmap over the groups."""
        g = len(msgs)
        if len(key_sets) != g:
            raise ValueError("one key set per message")
        koff = np.zeros(g + 1, dtype=np.uint64)
        for i, ks in enumerate(key_sets):
            if len(ks) % 128:
                raise ValueError("a key set must be a multiple of 128 bytes")
            koff[i + 1] = koff[i] + len(ks) // 128
        allk = b"".join(key_sets)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(allk); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        self._chk(self._lib.blsbn254_fast_aggregate_verify_batch(self._ctx, pa, koff.ctypes.data_as(_u64p), pm, off.ctypes.data_as(_u64p), ps,
                                                                 ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po))
        return o[:(g + 7) // 8].tobytes()

    def _keyset_rows(self, ks, sel_rows):
        """sel_rows: bytes (n_groups rows of ceil(n_keys / 8) bytes), or a list of per-group rows -> (flat bytes, n_groups)"""
        rb = (ks.count() + 7) // 8
        if not isinstance(sel_rows, (bytes, bytearray, memoryview, np.ndarray)):
            rows = [bytes(r) for r in sel_rows]
            if any(len(r) != rb for r in rows):
                raise ValueError("a row must be %d bytes" % rb)
            sel_rows = b"".join(rows)
        sel = bytes(sel_rows)
        if len(sel) % rb:
            raise ValueError("the rows must be a multiple of %d bytes" % rb)
        return sel, len(sel) // rb

    def keyset_sum_batch(self, ks, sel_rows):
        """impl Sum for G2Projective over the keys each row of bitmaps selects from a registered KeySet: (n_groups x 128 bytes,
        n_groups status bytes).  status 1: the row's sum, as aggregate_pks gives it on the selected keys; status 0: the row selects
        a key that does not decode or is off the curve, and its output is the identity encoding."""
        sel, g = self._keyset_rows(ks, sel_rows)
        a, pa = _inbuf(sel); o, po = _outbuf(128 * g); st, pst = _outbuf(g)
        self._chk(self._lib.blsbn254_keyset_sum_batch(self._ctx, ks._h, pa, ctypes.c_size_t(g), po, pst))
        return o[:128 * g].tobytes(), st[:g].tobytes()

    def keyset_fast_aggregate_verify_batch(self, ks, sel_rows, msgs, sigs, dst=DEFAULT_DST):
        """fast_aggregate_verify_batch with every group's keys named by a bitmap over a registered KeySet: one message and 64
        signature bytes per group.  Returns the LSB-first bitmap over the groups."""
        sel, g = self._keyset_rows(ks, sel_rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        data, off = pack_messages(msgs)
        a, pa = _inbuf(sel); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        self._chk(self._lib.blsbn254_keyset_fast_aggregate_verify_batch(self._ctx, ks._h, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(g), pd,
                                                                        ctypes.c_size_t(len(dst)), po))
        return o[:(g + 7) // 8].tobytes()

    def keyset_fast_aggregate_verify_batch_compressed(self, ks, sel_rows, msgs, sigs, dst=DEFAULT_DST):
        """keyset_fast_aggregate_verify_batch on compressed signatures (32 bytes per group); a signature that does not inflate
        clears its group's bit.  ks: a KeySet of any registration."""
        sel, g = self._keyset_rows(ks, sel_rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        data, off = pack_messages(msgs)
        a, pa = _inbuf(sel); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 32 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        self._chk(self._lib.blsbn254_keyset_fast_aggregate_verify_batch_compressed(self._ctx, ks._h, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(g),
                                                                                   pd, ctypes.c_size_t(len(dst)), po))
        return o[:(g + 7) // 8].tobytes()

    def keyset_stats(self):
        """dict: groups served by the keyset calls, groups summed through the complement, launches of the word kernel, key sets created"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_keyset_stats(self._ctx, o))
        return {"groups": int(o[0]), "complement_groups": int(o[1]), "launches": int(o[2]), "key_sets": int(o[3])}

    def keyset_weight_batch(self, ks, sel_rows):
        """The stake each row of bitmaps selects from a KeySet with weights (KeySet.set_weights): an (n_groups, n_cols) uint64
        array, entry (g, q) = the sum of column q over the selected keys that have the KeyValidate bit.  Exact."""
        sel, g = self._keyset_rows(ks, sel_rows)
        nc = ks.n_cols
        a, pa = _inbuf(sel); out = np.zeros(max(g * nc, 1), dtype=np.uint64)
        self._chk(self._lib.blsbn254_keyset_weight_batch(self._ctx, ks._h, pa, ctypes.c_size_t(g), out.ctypes.data_as(_u64p)))
        return out[:g * nc].reshape(g, nc)

    def keyset_quorum_verify_batch(self, ks, sel_rows, msgs, sigs, min_weight, dst=DEFAULT_DST):
        """keyset_fast_aggregate_verify_batch with a quorum: min_weight holds one minimum per stake column of the KeySet (0
        switches a column off).  Returns (bitmap, weights): bit g is set when row g carries at least the minimum in every column
        AND its aggregate verifies; weights is what keyset_weight_batch gives, for every group.  The groups are weighed first,
        and only those that reach the quorum are summed and paired."""
        sel, g = self._keyset_rows(ks, sel_rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        nc = ks.n_cols
        mw = np.ascontiguousarray(min_weight, dtype=np.uint64).reshape(-1)
        if mw.size != nc:
            raise ValueError("one minimum per weight column")
        data, off = pack_messages(msgs)
        a, pa = _inbuf(sel); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        wout = np.zeros(max(g * nc, 1), dtype=np.uint64)
        self._chk(self._lib.blsbn254_keyset_quorum_verify_batch(self._ctx, ks._h, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(g), pd,
                                                                ctypes.c_size_t(len(dst)), mw.ctypes.data_as(_u64p), wout.ctypes.data_as(_u64p), po))
        return o[:(g + 7) // 8].tobytes(), wout[:g * nc].reshape(g, nc)

    def keyset_weight_stats(self):
        """dict: groups weighed, groups below quorum (neither summed nor paired), launches of the weight kernel, weight tables set"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_keyset_weight_stats(self._ctx, o))
        return {"groups": int(o[0]), "below_quorum": int(o[1]), "launches": int(o[2]), "tables": int(o[3])}

    def _committee_rows(self, com, rows):
        """com: one committee index per group; rows: one row of ceil(size(com[g]) / 8) bytes per group -> the arguments of the C
        calls (the arrays are kept alive by the caller's reference to the tuple)"""
        rows = [bytes(r) for r in rows]
        g = len(rows)
        if len(com) != g:
            raise ValueError("one committee index per row")
        ca = np.zeros(max(g, 1), dtype=np.uint32)
        ca[:g] = np.asarray(list(com), dtype=np.uint32) if g else []
        so = np.zeros(g + 1, dtype=np.uint64)
        if g:
            so[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
        a, pa = _inbuf(b"".join(rows))
        return g, ca, ca.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), a, pa, so, so.ctypes.data_as(_u64p)

    def keyset_committee_sum_batch(self, ks, com, rows):
        """keyset_sum_batch over the committees of a KeySet (KeySet.set_committees): group g names committee com[g], rows[g] has one
        bit per MEMBER of that committee.  Returns (n_groups x 128 bytes, n_groups status bytes): what keyset_sum_batch gives on
        the rows scattered over the registry."""
        g, ca, pc, a, pa, so, pso = self._committee_rows(com, rows)
        o, po = _outbuf(128 * g); st, pst = _outbuf(g)
        self._chk(self._lib.blsbn254_keyset_committee_sum_batch(self._ctx, ks._h, pc, pa, pso, ctypes.c_size_t(g), po, pst))
        return o[:128 * g].tobytes(), st[:g].tobytes()

    def keyset_committee_fast_aggregate_verify_batch(self, ks, com, rows, msgs, sigs, dst=DEFAULT_DST):
        """keyset_fast_aggregate_verify_batch over the committees of a KeySet: one committee index, one row over that committee's
        members, one message and 64 signature bytes per group.  Returns the LSB-first bitmap over the groups."""
        g, ca, pc, a, pa, so, pso = self._committee_rows(com, rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        data, off = pack_messages(msgs)
        m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        self._chk(self._lib.blsbn254_keyset_committee_fast_aggregate_verify_batch(self._ctx, ks._h, pc, pa, pso, pm, off.ctypes.data_as(_u64p), ps,
                                                                                  ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po))
        return o[:(g + 7) // 8].tobytes()

    def keyset_committee_fast_aggregate_verify_batch_compressed(self, ks, com, rows, msgs, sigs, dst=DEFAULT_DST):
        """keyset_committee_fast_aggregate_verify_batch on compressed signatures (32 bytes per group); a signature that does not
        inflate clears its group's bit."""
        g, ca, pc, a, pa, so, pso = self._committee_rows(com, rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        data, off = pack_messages(msgs)
        m, pm = _inbuf(data); s, ps = _inbuf(sigs, 32 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        self._chk(self._lib.blsbn254_keyset_committee_fast_aggregate_verify_batch_compressed(self._ctx, ks._h, pc, pa, pso, pm, off.ctypes.data_as(_u64p), ps,
                                                                                             ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po))
        return o[:(g + 7) // 8].tobytes()

    def keyset_committee_weight_batch(self, ks, com, rows):
        """keyset_weight_batch over the committees of a KeySet: an (n_groups, n_cols) uint64 array, entry (g, q) = the sum of
        stake column q over the selected members of committee com[g] that have the KeyValidate bit."""
        g, ca, pc, a, pa, so, pso = self._committee_rows(com, rows)
        nc = ks.n_cols
        out = np.zeros(max(g * nc, 1), dtype=np.uint64)
        self._chk(self._lib.blsbn254_keyset_committee_weight_batch(self._ctx, ks._h, pc, pa, pso, ctypes.c_size_t(g), out.ctypes.data_as(_u64p)))
        return out[:g * nc].reshape(g, nc)

    def keyset_committee_stats(self):
        """dict: groups served by the committee calls, groups summed through the complement, launches of the word kernel,
        committee tables set"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_keyset_committee_stats(self._ctx, o))
        return {"groups": int(o[0]), "complement_groups": int(o[1]), "launches": int(o[2]), "tables": int(o[3])}

    @staticmethod
    def _seed_arg(seed):
        if seed is None:
            return None, ctypes.cast(None, _u8p)
        return _inbuf(seed, 32)

    def keyset_fast_aggregate_verify_batch_rlc(self, ks, sel_rows, msgs, sigs, dst=DEFAULT_DST, seed=None):
        """Same bitmap as keyset_fast_aggregate_verify_batch, via random linear combinations per message: the groups that sign the
        same message are checked a chunk (64 groups unless set_keyset_rlc_group says otherwise) at a time with ONE pairing
        equation, and whatever a chunk does not decide takes the exact path.  seed = None: the library draws it from the OS
        inside the call (production); a caller seed is for reproducible tests only."""
        sel, g = self._keyset_rows(ks, sel_rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        data, off = pack_messages(msgs)
        a, pa = _inbuf(sel); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        sd, psd = self._seed_arg(seed)
        self._chk(self._lib.blsbn254_keyset_fast_aggregate_verify_batch_rlc(self._ctx, ks._h, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(g), pd,
                                                                            ctypes.c_size_t(len(dst)), psd, po))
        return o[:(g + 7) // 8].tobytes()

    def keyset_committee_fast_aggregate_verify_batch_rlc(self, ks, com, rows, msgs, sigs, dst=DEFAULT_DST, seed=None):
        """Same bitmap as keyset_committee_fast_aggregate_verify_batch, via random linear combinations per message (see
        keyset_fast_aggregate_verify_batch_rlc)."""
        g, ca, pc, a, pa, so, pso = self._committee_rows(com, rows)
        if len(msgs) != g:
            raise ValueError("one row per message")
        data, off = pack_messages(msgs)
        m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        sd, psd = self._seed_arg(seed)
        self._chk(self._lib.blsbn254_keyset_committee_fast_aggregate_verify_batch_rlc(self._ctx, ks._h, pc, pa, pso, pm, off.ctypes.data_as(_u64p), ps,
                                                                                      ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), psd, po))
        return o[:(g + 7) // 8].tobytes()

    def set_keyset_rlc_group(self, group):
        """groups per chunk of the key-set RLC calls: 2 .. 4096; 0 = the default, 64"""
        self._chk(self._lib.blsbn254_set_keyset_rlc_group(self._ctx, ctypes.c_size_t(group)))

    def keyset_rlc_stats(self):
        """dict: groups decided by a chunk that passed, chunks checked, groups sent to the exact path after their chunk failed,
        groups sent there directly, message classes seen, calls"""
        o = (ctypes.c_uint64 * 6)()
        self._chk(self._lib.blsbn254_keyset_rlc_stats(self._ctx, o))
        return {"decided_groups": int(o[0]), "chunks": int(o[1]), "failed_chunk_groups": int(o[2]), "direct_groups": int(o[3]), "classes": int(o[4]),
                "calls": int(o[5])}

    def _stats4(self, fn, names):
        """the four counts of a stats call as a dict"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(fn(self._ctx, o))
        return {name: int(o[i]) for i, name in enumerate(names)}

    @staticmethod
    def _entry_sets(entry_sets, sb, noun):
        """entry_sets[g]: (key index or position, signature) pairs or a dict, sorted here -> (uint32 array, signature bytes, offsets);
        noun: what the first element of an entry is called in the errors"""
        ids, sigs, soff = [], [], np.zeros(len(entry_sets) + 1, dtype=np.uint64)
        for i, es in enumerate(entry_sets):
            es = sorted(es.items() if isinstance(es, dict) else ((int(k), s) for k, s in es))
            if any(a[0] == b[0] for a, b in zip(es, es[1:])):
                raise ValueError("entry set %d names a %s twice" % (i, noun.split()[0]))
            if any(k < 0 or k >= 1 << 32 for k, _ in es) or any(len(s) != sb for _, s in es):
                raise ValueError("an entry is (%s, %d signature bytes)" % (noun, sb))
            ids += [k for k, _ in es]; sigs += [bytes(s) for _, s in es]
            soff[i + 1] = len(ids)
        return np.asarray(ids if ids else [0], dtype=np.uint32), b"".join(sigs), soff

    @staticmethod
    def _bit_row(row, n, err):
        """a row of ceil(n / 8) bytes: as it is when given as bytes, else from an iterable of the indices below n it sets"""
        if isinstance(row, (bytes, bytearray, memoryview)):
            return row
        r = bytearray((n + 7) // 8)
        for k in row:
            k = int(k)
            if k < 0 or k >= n:
                raise ValueError(err)
            r[k >> 3] |= 1 << (k & 7)
        return r

    def keyset_aggregate_checked_batch(self, ks, entry_sets, msgs, dst=DEFAULT_DST):
        """The collecting node's call: entry_sets[g] = the signatures received for msgs[g], a list of (key index, 64-byte
        signature) pairs or a dict {index: signature} over the registered KeySet (sorted by index here; a repeated index raises
        ValueError).  Returns (out_sigs, rows, status): 64 bytes, one participation row of ceil(n_keys / 8) bytes and one status
        byte per group.  status 0: the aggregate of the entries the row names, which keyset_fast_aggregate_verify_batch accepts
        for (row, message); ST_SHORT = 5: nothing usable, the identity encoding and a zero row.  Entries on a key that fails
        KeyValidate or with a signature that is no curve point are left out; all candidates are checked with one pairing
        equation per group, and only a group that fails it has every signature verified.  No exception for a bad group."""
        return self._keyset_aggregate_checked(ks, entry_sets, msgs, dst, 64)

    def keyset_aggregate_checked_batch_compressed(self, ks, entry_sets, msgs, dst=DEFAULT_DST):
        """keyset_aggregate_checked_batch in wire format: 32-byte compressed signatures in the entries, 32 bytes per group in
        out_sigs.  Rows and statuses are those of keyset_aggregate_checked_batch on g1_inflate_batch of the signatures, out_sigs
        is g1_compress_batch of its out_sigs; a signature that does not inflate is left out like any undecodable one."""
        return self._keyset_aggregate_checked(ks, entry_sets, msgs, dst, 32)

    def _keyset_aggregate_checked(self, ks, entry_sets, msgs, dst, sb):
        fn = self._lib.blsbn254_keyset_aggregate_checked_batch if sb == 64 else self._lib.blsbn254_keyset_aggregate_checked_batch_compressed
        g = len(msgs)
        if len(entry_sets) != g:
            raise ValueError("one set of entries per message")
        ia, sigs, soff = self._entry_sets(entry_sets, sb, "key index")
        rb = (ks.count() + 7) // 8
        data, moff = pack_messages(msgs)
        s, ps = _inbuf(sigs); m, pm = _inbuf(data); d, pd = _inbuf(dst)
        o, po = _outbuf(sb * g)                                 # (large outputs of _outbuf share one buffer: only one per call)
        r = np.zeros(max(rb * g, 1), dtype=np.uint8); pr = r.ctypes.data_as(_u8p)
        st = np.zeros(g + 1, dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(fn(self._ctx, ks._h, ia.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ps, soff.ctypes.data_as(_u64p), pm, moff.ctypes.data_as(_u64p),
                     ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po, pr, pst))
        return o[:sb * g].tobytes(), r[:rb * g].tobytes(), st[:g].tobytes()

    def keyset_aggregate_stats(self):
        """dict: groups settled by the optimistic attempt, groups sent to the per-signature fallback, signatures verified
        individually, groups that ended in ST_SHORT"""
        return self._stats4(self._lib.blsbn254_keyset_aggregate_stats, ("optimistic_groups", "fallback_groups", "verified_signatures", "short_groups"))

    def keyset_committee_aggregate_checked_batch(self, ks, com, entry_sets, msgs, dst=DEFAULT_DST):
        """keyset_aggregate_checked_batch per committee of a KeySet (KeySet.set_committees): group g names committee com[g], and
        entry_sets[g] = the signatures received for msgs[g], a list of (position, 64-byte signature) pairs or a dict {position:
        signature}, a position counting in the committee's member list (sorted by position here; a repeated position raises
        ValueError).  Returns (out_sigs, rows, status): 64 bytes and one status byte per group, and rows as a list of per-group
        byte strings of ceil(size(com[g]) / 8) bytes each, bit j = member j is in the aggregate -- ready for
        keyset_committee_fast_aggregate_verify_batch(ks, com, rows, msgs, out_sigs).  Signatures and statuses are those of
        keyset_aggregate_checked_batch on the entries translated to registry indices; no exception for a bad group."""
        return self._keyset_committee_aggregate_checked(ks, com, entry_sets, msgs, dst, 64)

    def keyset_committee_aggregate_checked_batch_compressed(self, ks, com, entry_sets, msgs, dst=DEFAULT_DST):
        """keyset_committee_aggregate_checked_batch in wire format: 32-byte compressed signatures in the entries, 32 bytes per
        group in out_sigs -- ready for keyset_committee_fast_aggregate_verify_batch_compressed(ks, com, rows, msgs, out_sigs).
        Rows and statuses are those of the uncompressed call on g1_inflate_batch of the signatures, out_sigs is g1_compress_batch
        of its out_sigs."""
        return self._keyset_committee_aggregate_checked(ks, com, entry_sets, msgs, dst, 32)

    def _keyset_committee_aggregate_checked(self, ks, com, entry_sets, msgs, dst, sb):
        fn = (self._lib.blsbn254_keyset_committee_aggregate_checked_batch if sb == 64
              else self._lib.blsbn254_keyset_committee_aggregate_checked_batch_compressed)
        g = len(msgs)
        if len(entry_sets) != g or len(com) != g:
            raise ValueError("one committee index and one set of entries per message")
        sizes = getattr(ks, "_com_sizes", [])
        com = [int(x) for x in com]
        if any(x < 0 or x >= len(sizes) for x in com):
            raise ValueError("a group names a committee the key set does not have")
        pa, sigs, soff = self._entry_sets(entry_sets, sb, "position")
        rbs = [(sizes[x] + 7) // 8 for x in com]
        sel_off = np.zeros(g + 1, dtype=np.uint64)
        if g:
            sel_off[1:] = np.cumsum(rbs, dtype=np.uint64)
        total = int(sel_off[g])
        ca = np.asarray(com if com else [0], dtype=np.uint32)
        data, moff = pack_messages(msgs)
        s, ps = _inbuf(sigs); m, pm = _inbuf(data); d, pd = _inbuf(dst)
        o, po = _outbuf(sb * g)                                 # (large outputs of _outbuf share one buffer: only one per call)
        r = np.zeros(max(total, 1), dtype=np.uint8); pr = r.ctypes.data_as(_u8p)
        st = np.zeros(g + 1, dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._chk(fn(self._ctx, ks._h, ca.ctypes.data_as(u32p), pa.ctypes.data_as(u32p), ps, soff.ctypes.data_as(_u64p), pm, moff.ctypes.data_as(_u64p),
                     sel_off.ctypes.data_as(_u64p), ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po, pr, pst))
        raw = r[:total].tobytes()
        return o[:sb * g].tobytes(), [raw[int(sel_off[i]):int(sel_off[i + 1])] for i in range(g)], st[:g].tobytes()

    def keyset_committee_aggregate_stats(self):
        """the counts of keyset_aggregate_stats for keyset_committee_aggregate_checked_batch"""
        return self._stats4(self._lib.blsbn254_keyset_committee_aggregate_stats, ("optimistic_groups", "fallback_groups", "verified_signatures", "short_groups"))

    def keyset_merge_checked_batch(self, ks, contributions, msgs, dst=DEFAULT_DST):
        """The call of an intermediate node of an aggregation tree: contributions[g] = the partial aggregates received for
        msgs[g], a list of (row, 64-byte signature) pairs in the order of their priority, a row being ceil(n_keys / 8) bytes
        or an iterable of key indices of the registered KeySet.  The order is kept.  Returns (out_sigs, rows, used, status):
        64 bytes, one merged row and one status byte per group, and per group the list of its contributions' used flags.
        status 0: the sum of the used signatures, which keyset_fast_aggregate_verify_batch accepts for (row, message), the row
        being the OR of the used rows; ST_SHORT = 5: nothing usable, the identity encoding, a zero row and no flag.  Selection
        is greedy: a contribution is used when its signature is a curve point, its row is not empty, selects keys that pass
        KeyValidate only and is disjoint from the rows used before it.  One pairing equation per group checks the merged sum;
        only a group that fails it has every candidate verified on its own and is selected again.  No exception for a bad
        contribution or group."""
        return self._keyset_merge_checked(ks, contributions, msgs, dst, 64)

    def keyset_merge_checked_batch_compressed(self, ks, contributions, msgs, dst=DEFAULT_DST):
        """keyset_merge_checked_batch in wire format: 32-byte compressed signatures in the contributions, 32 bytes per group in
        out_sigs.  Rows, used flags and statuses are those of keyset_merge_checked_batch on g1_inflate_batch of the signatures,
        out_sigs is g1_compress_batch of its out_sigs; a contribution whose signature does not inflate is never used."""
        return self._keyset_merge_checked(ks, contributions, msgs, dst, 32)

    def _keyset_merge_checked(self, ks, contributions, msgs, dst, sb):
        fn = self._lib.blsbn254_keyset_merge_checked_batch if sb == 64 else self._lib.blsbn254_keyset_merge_checked_batch_compressed
        g = len(msgs)
        if len(contributions) != g:
            raise ValueError("one list of contributions per message")
        n, rb = ks.count(), (ks.count() + 7) // 8
        rows, sigs, coff = [], [], np.zeros(g + 1, dtype=np.uint64)
        for i, cs in enumerate(contributions):
            for row, sig in cs:
                row = self._bit_row(row, n, "a row names no key of the set")
                if len(row) != rb or len(sig) != sb:
                    raise ValueError("a contribution is (row of %d bytes or key indices, %d signature bytes)" % (rb, sb))
                rows.append(bytes(row)); sigs.append(bytes(sig))
            coff[i + 1] = len(rows)
        nc = len(rows)
        data, moff = pack_messages(msgs)
        a, pa = _inbuf(b"".join(rows)); s, ps = _inbuf(b"".join(sigs)); m, pm = _inbuf(data); d, pd = _inbuf(dst)
        o, po = _outbuf(sb * g)                                 # (large outputs of _outbuf share one buffer: only one per call)
        r = np.zeros(max(rb * g, 1), dtype=np.uint8); pr = r.ctypes.data_as(_u8p)
        u = np.zeros((nc + 7) // 8 + 1, dtype=np.uint8); pu = u.ctypes.data_as(_u8p)
        st = np.zeros(g + 1, dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(fn(self._ctx, ks._h, pa, ps, coff.ctypes.data_as(_u64p), pm, moff.ctypes.data_as(_u64p), ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)),
                     po, pr, pu, pst))
        used = [[bool((u[t >> 3] >> (t & 7)) & 1) for t in range(int(coff[i]), int(coff[i + 1]))] for i in range(g)]
        return o[:sb * g].tobytes(), r[:rb * g].tobytes(), used, st[:g].tobytes()

    def keyset_merge_stats(self):
        """dict: groups settled by the optimistic attempt, groups sent to the per-contribution fallback, contributions verified
        individually, groups that ended in ST_SHORT"""
        return self._stats4(self._lib.blsbn254_keyset_merge_stats, ("optimistic_groups", "fallback_groups", "verified_contributions", "short_groups"))

    def keyset_committee_merge_checked_batch(self, ks, com, groups, msgs, dst=DEFAULT_DST):
        """keyset_merge_checked_batch per committee of a KeySet (KeySet.set_committees): group g names committee com[g], and
        groups[g] = the partial aggregates received for msgs[g], a list of (row, 64-byte signature) pairs in the order of their
        priority, a row being ceil(size(com[g]) / 8) bytes, bit j = member j of the committee is in it, or an iterable of
        positions in the committee's member list.  The order is kept.  Returns (out_sigs, rows, used, status): 64 bytes and one
        status byte per group, per group the list of its contributions' used flags, and rows as a list of per-group byte strings
        of ceil(size(com[g]) / 8) bytes each -- ready for keyset_committee_fast_aggregate_verify_batch(ks, com, rows, msgs,
        out_sigs), and the (rows, out_sigs) of keyset_committee_aggregate_checked_batch are contributions of this call as they
        are.  Signatures, statuses and used flags are those of keyset_merge_checked_batch on the rows scattered over the
        registry; no exception for a bad contribution or group."""
        return self._keyset_committee_merge_checked(ks, com, groups, msgs, dst, 64)

    def keyset_committee_merge_checked_batch_compressed(self, ks, com, groups, msgs, dst=DEFAULT_DST):
        """keyset_committee_merge_checked_batch in wire format: 32-byte compressed signatures in the contributions, 32 bytes per
        group in out_sigs; the (rows, out_sigs) of keyset_committee_aggregate_checked_batch_compressed are contributions of this
        call as they are, and its own go to keyset_committee_fast_aggregate_verify_batch_compressed.  Rows, used flags and
        statuses are those of the uncompressed call on g1_inflate_batch of the signatures, out_sigs is g1_compress_batch of its
        out_sigs."""
        return self._keyset_committee_merge_checked(ks, com, groups, msgs, dst, 32)

    def _keyset_committee_merge_checked(self, ks, com, groups, msgs, dst, sb):
        fn = (self._lib.blsbn254_keyset_committee_merge_checked_batch if sb == 64
              else self._lib.blsbn254_keyset_committee_merge_checked_batch_compressed)
        g = len(msgs)
        if len(groups) != g or len(com) != g:
            raise ValueError("one committee index and one list of contributions per message")
        sizes = getattr(ks, "_com_sizes", [])
        com = [int(x) for x in com]
        if any(x < 0 or x >= len(sizes) for x in com):
            raise ValueError("a group names a committee the key set does not have")
        rows, sigs = [], []
        coff, roff, sel_off = (np.zeros(g + 1, dtype=np.uint64) for _ in range(3))
        for i, cs in enumerate(groups):
            n, rb = sizes[com[i]], (sizes[com[i]] + 7) // 8
            for row, sig in cs:
                row = self._bit_row(row, n, "a row names no member of the committee")
                if len(row) != rb or len(sig) != sb:
                    raise ValueError("a contribution is (row of %d bytes or positions, %d signature bytes)" % (rb, sb))
                rows.append(bytes(row)); sigs.append(bytes(sig))
            coff[i + 1] = len(rows)
            roff[i + 1] = int(roff[i]) + rb * (len(rows) - int(coff[i]))
            sel_off[i + 1] = int(sel_off[i]) + rb
        nc, total = len(rows), int(sel_off[g])
        ca = np.asarray(com if com else [0], dtype=np.uint32)
        data, moff = pack_messages(msgs)
        a, pa = _inbuf(b"".join(rows)); s, ps = _inbuf(b"".join(sigs)); m, pm = _inbuf(data); d, pd = _inbuf(dst)
        o, po = _outbuf(sb * g)                                 # (large outputs of _outbuf share one buffer: only one per call)
        r = np.zeros(max(total, 1), dtype=np.uint8); pr = r.ctypes.data_as(_u8p)
        u = np.zeros((nc + 7) // 8 + 1, dtype=np.uint8); pu = u.ctypes.data_as(_u8p)
        st = np.zeros(g + 1, dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(fn(self._ctx, ks._h, ca.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), pa, roff.ctypes.data_as(_u64p), ps, coff.ctypes.data_as(_u64p), pm,
                     moff.ctypes.data_as(_u64p), sel_off.ctypes.data_as(_u64p), ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po, pr, pu, pst))
        used = [[bool((u[t >> 3] >> (t & 7)) & 1) for t in range(int(coff[i]), int(coff[i + 1]))] for i in range(g)]
        raw = r[:total].tobytes()
        return o[:sb * g].tobytes(), [raw[int(sel_off[i]):int(sel_off[i + 1])] for i in range(g)], used, st[:g].tobytes()

    def keyset_committee_merge_stats(self):
        """the counts of keyset_merge_stats for keyset_committee_merge_checked_batch"""
        return self._stats4(self._lib.blsbn254_keyset_committee_merge_stats, ("optimistic_groups", "fallback_groups", "verified_contributions", "short_groups"))

    def aggregate_verify_batch(self, key_sets, msg_sets, agg_sigs, dst=DEFAULT_DST):
        """Many independent aggregate signatures in one call.  key_sets: list of byte strings (each a multiple of 128 bytes: the
        keys of one group); msg_sets: one list of messages per group, as many as the group has keys; agg_sigs: 64 bytes per group.
        Returns the LSB-first bitmap over the groups: bit g = aggregate_verify(key_sets[g], msg_sets[g], agg_sigs[64 g ..]).  An
        empty group is invalid."""
        g = len(key_sets)
        if len(msg_sets) != g:
            raise ValueError("one list of messages per key set")
        goff = self._group_offsets(key_sets, 128, "a key set")
        if any(int(goff[i + 1] - goff[i]) != len(ms) for i, ms in enumerate(msg_sets)):
            raise ValueError("a group needs as many messages as keys")
        return self.aggregate_verify_batch_flat(b"".join(key_sets), [m for ms in msg_sets for m in ms], goff, agg_sigs, dst)

    def aggregate_verify_batch_flat(self, pks, msgs, grp_off, agg_sigs, dst=DEFAULT_DST):
        """The same over flat arrays, as the C ABI takes them: group g owns the pairs grp_off[g] .. grp_off[g + 1] of pks (128 B each)
        and msgs (a list); the offsets need not start at 0 (pairs in front of grp_off[0] belong to no group)."""
        goff = np.ascontiguousarray(np.asarray(grp_off, dtype=np.uint64))
        if goff.ndim != 1 or goff.size < 1:
            raise ValueError("grp_off needs n_groups + 1 entries")
        g = goff.size - 1
        if g and int(goff[-1]) > len(msgs):
            raise ValueError("grp_off names more pairs than there are messages")
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * len(msgs)); m, pm = _inbuf(data); s, ps = _inbuf(agg_sigs, 64 * g); d, pd = _inbuf(dst); o, po = _outbuf((g + 7) // 8)
        self._chk(self._lib.blsbn254_aggregate_verify_batch(self._ctx, pa, pm, off.ctypes.data_as(_u64p), goff.ctypes.data_as(_u64p), ps,
                                                            ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po))
        return o[:(g + 7) // 8].tobytes()

    def aggregate_batch_stats(self):
        """dict: groups served by aggregate_verify_batch, lanes run by its two-pairs-per-lane Miller kernel, calls served by the
        small forms, launches"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_aggregate_batch_stats(self._ctx, o))
        return {"groups": int(o[0]), "lanes": int(o[1]), "small_calls": int(o[2]), "launches": int(o[3])}

    def g1_mul_batch(self, g1, scalars, n):
        """Mul<Scalar> for G1Projective (g1.rs:518-534), element-wise: [k_i] P_i."""
        a, pa = _inbuf(g1, 64 * n); k, pk = _inbuf(scalars, 32 * n); o, po = _outbuf(64 * n)
        self._chk(self._lib.blsbn254_g1_mul_batch(self._ctx, pa, pk, ctypes.c_size_t(n), po))
        return o[:64 * n].tobytes()

    def g2_mul_batch(self, g2, scalars, n):
        """Mul<Scalar> for G2Projective (g2.rs:866-886), element-wise: [k_i] Q_i."""
        a, pa = _inbuf(g2, 128 * n); k, pk = _inbuf(scalars, 32 * n); o, po = _outbuf(128 * n)
        self._chk(self._lib.blsbn254_g2_mul_batch(self._ctx, pa, pk, ctypes.c_size_t(n), po))
        return o[:128 * n].tobytes()

    def g1_msm(self, points, scalars, n):
        """LinearCombination for G1Projective (g1.rs:559), n-term form: sum_i [k_i] P_i as 64 uncompressed bytes (bucket method)."""
        a, pa = _inbuf(points, 64 * n); k, pk = _inbuf(scalars, 32 * n); o, po = _outbuf(64)
        self._chk(self._lib.blsbn254_g1_msm(self._ctx, pa, pk, ctypes.c_size_t(n), po))
        return o[:64].tobytes()

    def g2_msm(self, points, scalars, n):
        """LinearCombination for G2Projective (g2.rs:577), n-term form: sum_i [k_i] Q_i as 128 uncompressed bytes."""
        a, pa = _inbuf(points, 128 * n); k, pk = _inbuf(scalars, 32 * n); o, po = _outbuf(128)
        self._chk(self._lib.blsbn254_g2_msm(self._ctx, pa, pk, ctypes.c_size_t(n), po))
        return o[:128].tobytes()

    def set_msm_window(self, c):
        """window width of the bucket method: 0 = chosen from n, 2..16 = forced"""
        self._chk(self._lib.blsbn254_set_msm_window(self._ctx, ctypes.c_int(c)))

    def msm_stats(self):
        """dict: calls on the bucket path, calls on the small-n path, bucket entries accumulated, level-0 chunks summed"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_msm_stats(self._ctx, o))
        return {"bucket_calls": int(o[0]), "small_calls": int(o[1]), "entries": int(o[2]), "chunks": int(o[3])}

    def threshold_combine(self, ids, partial_sigs, t):
        a, pa = _inbuf(ids, 32 * t); s, ps = _inbuf(partial_sigs, 64 * t); o, po = _outbuf(64)
        self._chk(self._lib.blsbn254_threshold_combine(self._ctx, pa, ps, ctypes.c_size_t(t), po))
        return o.tobytes()

    def lagrange_at_zero(self, ids, t):
        """t x 32 bytes: lambda_i = prod_{j != i} x_j / (x_j - x_i) (big-endian Fr)."""
        a, pa = _inbuf(ids, 32 * t); o, po = _outbuf(32 * t)
        self._chk(self._lib.blsbn254_lagrange_at_zero(self._ctx, pa, ctypes.c_size_t(t), po))
        return o[:32 * t].tobytes()

    @staticmethod
    def _group_offsets(sets, width, what):
        lens = np.fromiter(map(len, sets), dtype=np.uint64, count=len(sets))
        if (lens % width).any():
            raise ValueError("%s must be a multiple of %d bytes" % (what, width))
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        np.cumsum(lens // width, out=off[1:])
        return off

    def threshold_combine_batch(self, id_sets, sig_sets):
        """id_sets / sig_sets: lists of byte strings, one per group (32 bytes per id, 64 per partial signature).  Returns
        (sigs, status): 64 bytes and one status byte per group (0, ERR_SCALAR = 1, ERR_G1 = 2); a bad group's signature is the
        identity encoding.  No exception for a bad group."""
        g = len(id_sets)
        if len(sig_sets) != g:
            raise ValueError("one set of partial signatures per set of ids")
        off = self._group_offsets(id_sets, 32, "a set of ids")
        if not np.array_equal(off, self._group_offsets(sig_sets, 64, "a set of partial signatures")):
            raise ValueError("a group needs as many partial signatures as ids")
        a, pa = _inbuf(b"".join(id_sets)); s, ps = _inbuf(b"".join(sig_sets)); o, po = _outbuf(64 * g)
        st = np.zeros(max(g, 1), dtype=np.uint8); pst = st.ctypes.data_as(_u8p)      # (large outputs share ONE buffer per thread: not for two)
        self._chk(self._lib.blsbn254_threshold_combine_batch(self._ctx, pa, ps, off.ctypes.data_as(_u64p), ctypes.c_size_t(g), po, pst))
        return o[:64 * g].tobytes(), st[:g].tobytes()

    def lagrange_at_zero_batch(self, id_sets):
        """(coefficients, status): 32 bytes per id in the order given, one status byte per group; the coefficients of a bad
        group are zero bytes."""
        g = len(id_sets)
        off = self._group_offsets(id_sets, 32, "a set of ids")
        n = int(off[-1])
        a, pa = _inbuf(b"".join(id_sets)); o, po = _outbuf(32 * n)
        st = np.zeros(max(g, 1), dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(self._lib.blsbn254_lagrange_at_zero_batch(self._ctx, pa, off.ctypes.data_as(_u64p), ctypes.c_size_t(g), po, pst))
        return o[:32 * n].tobytes(), st[:g].tobytes()

    def threshold_batch_stats(self):
        """dict: groups served by the lane-per-share kernels, groups handed to the single-group pipeline, launches, and the
        hand-over size t_big of this build"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_threshold_batch_stats(self._ctx, o))
        return {"batched_groups": int(o[0]), "single_groups": int(o[1]), "launches": int(o[2]), "t_big": int(o[3])}

    def _deal_args(self, coef_sets, coef_width, id_sets):
        if len(coef_sets) != len(id_sets):
            raise ValueError("one set of ids per set of coefficients")
        coff = self._group_offsets(coef_sets, coef_width, "a set of coefficients")
        goff = self._group_offsets(id_sets, 32, "a set of ids")
        return coff, goff, int(goff[-1])

    def fr_poly_eval_batch(self, coef_sets, id_sets):
        """Key shares: group g's polynomial (coef_sets[g]: 32 bytes per coefficient, low order first) evaluated at each id of
        id_sets[g] (32 bytes each).  Returns (shares, status): 32 bytes per id in the order given and one status byte per group
        (0, ERR_SCALAR = 1: a coefficient or an id >= r, or an id 0); a bad group's shares are zero bytes.  Signing side: not
        constant time."""
        coff, goff, n = self._deal_args(coef_sets, 32, id_sets)
        g = len(id_sets)
        a, pa = _inbuf(b"".join(coef_sets)); x, px = _inbuf(b"".join(id_sets)); o, po = _outbuf(32 * n)
        st = np.zeros(max(g, 1), dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(self._lib.blsbn254_fr_poly_eval_batch(self._ctx, pa, coff.ctypes.data_as(_u64p), px, goff.ctypes.data_as(_u64p), ctypes.c_size_t(g), po, pst))
        return o[:32 * n].tobytes(), st[:g].tobytes()

    def g2_poly_eval_batch(self, commit_sets, id_sets):
        """Public key shares: sum_j [id^j] C_j for group g's Feldman commitments (commit_sets[g]: 128 bytes each, low order
        first) at each id of id_sets[g].  Returns (pks, status): 128 bytes per id and one status byte per group (0,
        ERR_SCALAR = 1: an id >= r or 0, ERR_G2 = 3: a commitment that is not a valid subgroup point); a bad group's keys are
        the identity encoding."""
        coff, goff, n = self._deal_args(commit_sets, 128, id_sets)
        g = len(id_sets)
        a, pa = _inbuf(b"".join(commit_sets)); x, px = _inbuf(b"".join(id_sets)); o, po = _outbuf(128 * n)
        st = np.zeros(max(g, 1), dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(self._lib.blsbn254_g2_poly_eval_batch(self._ctx, pa, coff.ctypes.data_as(_u64p), px, goff.ctypes.data_as(_u64p), ctypes.c_size_t(g), po, pst))
        return o[:128 * n].tobytes(), st[:g].tobytes()

    def threshold_verify_shares_batch(self, commit_sets, id_sets, sig_sets, msgs, dst=DEFAULT_DST):
        """Partial signatures checked against the key shares of g2_poly_eval_batch, which stay on the device: sig_sets[g] holds
        64 bytes per id of id_sets[g], msgs[g] is the group's message.  Returns (bitmap, status): bit i (LSB-first, in the order
        given) = partial signature i verifies under its key share; status as g2_poly_eval_batch, every bit of a bad group 0."""
        coff, goff, n = self._deal_args(commit_sets, 128, id_sets)
        g = len(id_sets)
        if len(sig_sets) != g or len(msgs) != g:
            raise ValueError("one set of partial signatures and one message per set of ids")
        if not np.array_equal(goff, self._group_offsets(sig_sets, 64, "a set of partial signatures")):
            raise ValueError("a group needs as many partial signatures as ids")
        data, moff = pack_messages(list(msgs))
        a, pa = _inbuf(b"".join(commit_sets)); x, px = _inbuf(b"".join(id_sets)); s, ps = _inbuf(b"".join(sig_sets))
        m, pm = _inbuf(data); d, pd = _inbuf(dst); o, po = _outbuf((n + 7) // 8)
        st = np.zeros(max(g, 1), dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(self._lib.blsbn254_threshold_verify_shares_batch(self._ctx, pa, coff.ctypes.data_as(_u64p), px, ps, goff.ctypes.data_as(_u64p), pm,
                                                                   moff.ctypes.data_as(_u64p), ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po, pst))
        return o[:(n + 7) // 8].tobytes(), st[:g].tobytes()

    def threshold_deal_stats(self):
        """dict: launches of the G2 evaluation kernel, shares evaluated in G2, shares evaluated in Fr, and the bit count the last
        G2 launch looped over"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_threshold_deal_stats(self._ctx, o))
        return {"g2_launches": int(o[0]), "g2_shares": int(o[1]), "fr_shares": int(o[2]), "id_bits": int(o[3])}

    def threshold_verify_key_shares_batch(self, commit_sets, id_sets, share_sets):
        """Dealt key shares checked against their group's Feldman commitments: share_sets[g] holds 32 bytes per id of id_sets[g].
        Returns (bitmap, status): bit i (LSB-first, in the order given) = [share_i] G2gen equals sum_j [id_i^j] C_j, share_i is
        below r and its group's status is 0; status as g2_poly_eval_batch, every bit of a bad group 0.  A zero share is valid
        exactly where the polynomial is zero.  Not constant time: the generator table is indexed by the share's digits."""
        coff, goff, n = self._deal_args(commit_sets, 128, id_sets)
        g = len(id_sets)
        if len(share_sets) != g:
            raise ValueError("one set of shares per set of ids")
        if not np.array_equal(goff, self._group_offsets(share_sets, 32, "a set of shares")):
            raise ValueError("a group needs as many shares as ids")
        a, pa = _inbuf(b"".join(commit_sets)); x, px = _inbuf(b"".join(id_sets)); s, ps = _inbuf(b"".join(share_sets))
        o, po = _outbuf((n + 7) // 8)
        st = np.zeros(max(g, 1), dtype=np.uint8); pst = st.ctypes.data_as(_u8p)
        self._chk(self._lib.blsbn254_threshold_verify_key_shares_batch(self._ctx, pa, coff.ctypes.data_as(_u64p), px, ps, goff.ctypes.data_as(_u64p),
                                                                       ctypes.c_size_t(g), po, pst))
        return o[:(n + 7) // 8].tobytes(), st[:g].tobytes()

    def threshold_key_check_stats(self):
        """dict: launches of the key-share check kernel, shares checked, times this context built the generator table (1 after the
        first call with a share), and the window width of the table in bits"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_threshold_key_check_stats(self._ctx, o))
        return {"launches": int(o[0]), "shares": int(o[1]), "table_builds": int(o[2]), "window_bits": int(o[3])}

    def threshold_combine_checked_batch(self, commit_sets, id_sets, sig_sets, msgs, dst=DEFAULT_DST):
        """The combiner's call: from group g's Feldman commitments (commit_sets[g], 128 bytes each; their number is the threshold
        t_g), the ids and partial signatures it received (id_sets[g], sig_sets[g]) and its message msgs[g], the group signature
        over t_g good partials.  Returns (sigs, used_bitmap, status): 64 bytes per group, bit i (LSB-first, in the order given) =
        share i was interpolated, one status byte per group (0, ERR_SCALAR = 1: an id >= r, 0 or repeated, ERR_G2 = 3: a bad
        commitment, ST_SHORT = 5: no t_g shares whose combination verifies).  The first t_g decodable partials are tried first
        and checked with one pairing equation under C_0; only a group that fails it has every partial verified.  A bad group's
        signature is the identity encoding and its used bits are 0.  No exception for a bad group."""
        coff, goff, n = self._deal_args(commit_sets, 128, id_sets)
        g = len(id_sets)
        if len(sig_sets) != g or len(msgs) != g:
            raise ValueError("one set of partial signatures and one message per set of ids")
        if not np.array_equal(goff, self._group_offsets(sig_sets, 64, "a set of partial signatures")):
            raise ValueError("a group needs as many partial signatures as ids")
        data, moff = pack_messages(list(msgs))
        a, pa = _inbuf(b"".join(commit_sets)); x, px = _inbuf(b"".join(id_sets)); s, ps = _inbuf(b"".join(sig_sets))
        m, pm = _inbuf(data); d, pd = _inbuf(dst); o, po = _outbuf(64 * g)
        nb = (n + 7) // 8
        used = np.zeros(max(nb, 1), dtype=np.uint8); st = np.zeros(max(g, 1), dtype=np.uint8)
        self._chk(self._lib.blsbn254_threshold_combine_checked_batch(self._ctx, pa, coff.ctypes.data_as(_u64p), px, ps, goff.ctypes.data_as(_u64p), pm,
                                                                     moff.ctypes.data_as(_u64p), ctypes.c_size_t(g), pd, ctypes.c_size_t(len(dst)), po,
                                                                     used.ctypes.data_as(_u8p), st.ctypes.data_as(_u8p)))
        return o[:64 * g].tobytes(), used[:nb].tobytes(), st[:g].tobytes()

    def threshold_checked_stats(self):
        """dict: groups settled by the optimistic attempt, groups sent to the per-share fallback, shares verified individually,
        groups that ended in ST_SHORT"""
        o = (ctypes.c_uint64 * 4)()
        self._chk(self._lib.blsbn254_threshold_checked_stats(self._ctx, o))
        return {"optimistic_groups": int(o[0]), "fallback_groups": int(o[1]), "verified_shares": int(o[2]), "short_groups": int(o[3])}

    # ---- Gt group operations and the field-primitive debug ABI
    FIELD_OP_WIDTH = {**{k: 32 for k in range(0, 9)}, **{k: 64 for k in range(16, 22)}, **{k: 192 for k in range(32, 36)},
                      **{k: 384 for k in range(48, 57)}, **{k: 32 for k in range(64, 70)}}
    FIELD_OP_BINARY = (0, 3, 4, 16, 32, 48, 56, 64, 67, 68)

    def field_op_batch(self, op, a, b, n):
        """One field / tower primitive element-wise (op = BLSBN254_OP_* of the header); n * width bytes back."""
        w = self.FIELD_OP_WIDTH[op]
        x, px = _inbuf(a, w * n); o, po = _outbuf(w * n)
        if op in self.FIELD_OP_BINARY:
            y, py = _inbuf(b, w * n)
        else:
            y, py = None, ctypes.cast(None, _u8p)
        self._chk(self._lib.blsbn254_field_op_batch(self._ctx, ctypes.c_int(op), px, py, ctypes.c_size_t(n), po))
        return o[:w * n].tobytes()

    def gt_mul_batch(self, a, b, n):
        x, px = _inbuf(a, 384 * n); y, py = _inbuf(b, 384 * n); o, po = _outbuf(384 * n)
        self._chk(self._lib.blsbn254_gt_mul_batch(self._ctx, px, py, ctypes.c_size_t(n), po))
        return o[:384 * n].tobytes()

    def gt_pow_batch(self, gt, scalars, n):
        """Gt::mul_by_scalar (pairings.rs:585-600): gt_i ^ k_i, k_i = 32 bytes big-endian."""
        x, px = _inbuf(gt, 384 * n); k, pk = _inbuf(scalars, 32 * n); o, po = _outbuf(384 * n)
        self._chk(self._lib.blsbn254_gt_pow_batch(self._ctx, px, pk, ctypes.c_size_t(n), po))
        return o[:384 * n].tobytes()

    # ---- compressed codecs
    def _codec(self, fn, data, n, isz, osz):
        a, pa = _inbuf(data, isz * n); o, po = _outbuf(osz * n)
        self._chk(fn(self._ctx, pa, ctypes.c_size_t(n), po))
        return o[:osz * n].tobytes()

    def g1_compress_batch(self, g1, n): return self._codec(self._lib.blsbn254_g1_compress_batch, g1, n, 64, 32)
    def g1_decompress_batch(self, c, n): return self._codec(self._lib.blsbn254_g1_decompress_batch, c, n, 32, 64)
    def g2_compress_batch(self, g2, n): return self._codec(self._lib.blsbn254_g2_compress_batch, g2, n, 128, 64)
    def g2_decompress_batch(self, c, n): return self._codec(self._lib.blsbn254_g2_decompress_batch, c, n, 64, 128)

    def _inflate(self, fn, data, n, isz):
        a, pa = _inbuf(data, isz * n); o, po = _outbuf(2 * isz * n); st, pst = _outbuf(n)
        self._chk(fn(self._ctx, pa, ctypes.c_size_t(n), po, pst))
        return o[:2 * isz * n].tobytes(), st[:n].tobytes()

    def g1_inflate_batch(self, c, n):
        """The per-element form of g1_decompress_batch: (n x 64 bytes, n status bytes).  status 1: the element's uncompressed
        bytes; status 0: it does not decode and its output is the marker, 64 bytes of 0xFF, which no entry point decodes."""
        return self._inflate(self._lib.blsbn254_g1_inflate_batch, c, n, 32)

    def g2_inflate_batch(self, c, n):
        """As g1_inflate_batch for 64-byte compressed G2 elements: (n x 128 bytes, n status bytes)."""
        return self._inflate(self._lib.blsbn254_g2_inflate_batch, c, n, 64)

    # ---- signing side (also used to generate large synthetic batches)
    def sign_batch(self, sks, msgs, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        k, pk = _inbuf(sks, 32 * n); m, pm = _inbuf(data); d, pd = _inbuf(dst); o, po = _outbuf(64 * n)
        self._chk(self._lib.blsbn254_sign_batch(self._ctx, pk, pm, off.ctypes.data_as(_u64p), ctypes.c_size_t(n), pd,
                                                ctypes.c_size_t(len(dst)), po))
        return o[:64 * n].tobytes()

    def sk_to_pk_batch(self, sks, n):
        k, pk = _inbuf(sks, 32 * n); o, po = _outbuf(128 * n)
        self._chk(self._lib.blsbn254_sk_to_pk_batch(self._ctx, pk, ctypes.c_size_t(n), po))
        return o[:128 * n].tobytes()

    def keygen_batch(self, ikm, n, key_info=b""):
        """IETF KeyGen over HKDF-SHA-256 (salt KEYGEN_SALT, helpers.rs:3); ikm = n equal-length seeds >= 32 B."""
        if n == 0:
            return b""
        if len(ikm) % n:
            raise ValueError("ikm must hold n equal-length seeds")
        k, pk = _inbuf(ikm); ki, pki = _inbuf(key_info); o, po = _outbuf(32 * n)
        self._chk(self._lib.blsbn254_keygen_batch(self._ctx, pk, ctypes.c_size_t(len(ikm) // n), ctypes.c_size_t(n), pki,
                                                  ctypes.c_size_t(len(key_info)), po))
        return o[:32 * n].tobytes()

    def hash_to_scalar_batch(self, msgs, dst): return self._h2c(self._lib.blsbn254_hash_to_scalar_batch, msgs, dst, 32)

    def pop_prove_batch(self, sks, n, dst=POP_DST):
        k, pk = _inbuf(sks, 32 * n); d, pd = _inbuf(dst); o, po = _outbuf(64 * n)
        self._chk(self._lib.blsbn254_pop_prove_batch(self._ctx, pk, ctypes.c_size_t(n), pd, ctypes.c_size_t(len(dst)), po))
        return o[:64 * n].tobytes()

    def pop_verify_batch(self, pks, proofs, n, dst=POP_DST):
        a, pa = _inbuf(pks, 128 * n); b, pb = _inbuf(proofs, 64 * n); d, pd = _inbuf(dst); o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_pop_verify_batch(self._ctx, pa, pb, ctypes.c_size_t(n), pd, ctypes.c_size_t(len(dst)), po))
        return o[:(n + 7) // 8].tobytes()

    # ---- device-resident variants (raw device pointers, e.g. torch tensor .data_ptr())
    def verify_batch_dev(self, d_pks, d_msgs, d_off, d_sigs, n, d_bitmap, dst=DEFAULT_DST):
        d, pd = _inbuf(dst)
        self._chk(self._lib.blsbn254_verify_batch_dev(self._ctx, ctypes.c_void_p(d_pks), ctypes.c_void_p(d_msgs), ctypes.c_void_p(d_off),
                                                      ctypes.c_void_p(d_sigs), ctypes.c_size_t(n), pd, ctypes.c_size_t(len(dst)),
                                                      ctypes.c_void_p(d_bitmap)))

    def verify_batch_rlc_dev(self, d_pks, d_msgs, d_off, d_sigs, n, d_bitmap, dst=DEFAULT_DST, seed=None):
        d, pd = _inbuf(dst)
        if seed is None:
            sd, psd = None, ctypes.cast(None, _u8p)
        else:
            sd, psd = _inbuf(seed, 32)
        self._chk(self._lib.blsbn254_verify_batch_rlc_dev(self._ctx, ctypes.c_void_p(d_pks), ctypes.c_void_p(d_msgs), ctypes.c_void_p(d_off),
                                                          ctypes.c_void_p(d_sigs), ctypes.c_size_t(n), pd, ctypes.c_size_t(len(dst)), psd,
                                                          ctypes.c_void_p(d_bitmap)))

    def pairing_batch_dev(self, d_g1, d_g2, n, d_gt, d_status=0):
        self._chk(self._lib.blsbn254_pairing_batch_dev(self._ctx, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g2), ctypes.c_size_t(n),
                                                       ctypes.c_void_p(d_gt), ctypes.c_void_p(d_status)))

    def synchronize(self):
        self._chk(self._lib.blsbn254_ctx_synchronize(self._ctx))

    @property
    def stream(self):
        return self._lib.blsbn254_ctx_stream(self._ctx)

    # ---- measurement hooks
    def profile_enable(self, on=True):
        self._chk(self._lib.blsbn254_profile_enable(self._ctx, ctypes.c_int(1 if on else 0)))

    def profile_reset(self):
        self._chk(self._lib.blsbn254_profile_reset(self._ctx))

    def valu_peak(self):
        """Measured whole-chip v_mad_u64_u32 rate (lane-MADs/s)."""
        v = ctypes.c_double(0)
        self._chk(self._lib.blsbn254_valu_peak(self._ctx, ctypes.byref(v)))
        return v.value

    def valu_probe(self):
        """The whole VALU probe (blsbn254_valu_probe): MAD and plain-VOP2 rates, the clock held under each probe
        kernel, and the 4-cycle issue ceiling at that clock."""
        o = (ctypes.c_double * 6)()
        self._chk(self._lib.blsbn254_valu_probe(self._ctx, o))
        return {"mad_per_s": o[0], "vop2_per_s": o[1], "clock_hz_mad": o[2], "clock_hz_vop2": o[3], "cus": int(o[4]),
                "issue_ceiling_per_s": o[5]}

    def profile_read(self):
        names = ctypes.create_string_buffer(32 * 64)
        launches = (ctypes.c_uint64 * 64)()
        ms = (ctypes.c_double * 64)()
        k = self._lib.blsbn254_profile_read(self._ctx, names, launches, ms, ctypes.c_int(64))
        if k < 0:
            self._chk(k)
        out = {}
        for i in range(k):
            nm = names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode()
            out[nm] = {"launches": int(launches[i]), "total_ms": float(ms[i])}
        return out


class PreparedKeys:
    """blsbn254_g2prepared: the line tables of u public keys, resident on the engine's GPU."""

    def __init__(self, engine, pks, u):
        self._eng = engine
        self._lib = engine._lib
        self._lib.blsbn254_g2prepared_count.restype = ctypes.c_size_t
        self._h = ctypes.c_void_p()
        a, pa = _inbuf(pks, 128 * u)
        engine._chk(self._lib.blsbn254_g2_prepare_batch(engine._ctx, pa, ctypes.c_size_t(u), ctypes.byref(self._h)))

    def count(self):
        return int(self._lib.blsbn254_g2prepared_count(self._h))

    def valid_bitmap(self):
        u = self.count()
        o, po = _outbuf((u + 7) // 8)
        self._eng._chk(self._lib.blsbn254_g2prepared_valid(self._eng._ctx, self._h, po))
        return o[:(u + 7) // 8].tobytes()

    def close(self):
        if getattr(self, "_h", None) and getattr(self._eng, "_ctx", None):
            self._lib.blsbn254_g2prepared_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeySet:
    """blsbn254_keyset: n_keys public keys registered once on the engine's GPU (decoded, curve-checked, with their total), to be
    summed by participation bitmaps (Engine.keyset_sum_batch, Engine.keyset_fast_aggregate_verify_batch).  With proofs (n_keys x
    64 bytes, as pop_prove_batch makes them) every key's proof of possession is verified under pop_dst at registration, and a
    key whose proof fails is a bad key of the set, as one that does not decode.  compressed=True: pks are n_keys x 64 bytes and
    proofs n_keys x 32 bytes in the compressed encodings; the set is the one their inflated bytes register (a proof still signs
    the 128-byte uncompressed key)."""

    def __init__(self, engine, pks, n_keys, proofs=None, pop_dst=POP_DST, compressed=False):
        self._eng = engine
        self._lib = engine._lib
        self._lib.blsbn254_keyset_count.restype = ctypes.c_size_t
        self._lib.blsbn254_keyset_committee_count.restype = ctypes.c_size_t
        self._h = ctypes.c_void_p()
        self.n_cols = 0
        if compressed:
            a, pa = _inbuf(pks, 64 * n_keys); d, pd = _inbuf(pop_dst)
            b, pb = (None, ctypes.cast(None, _u8p)) if proofs is None else _inbuf(proofs, 32 * n_keys)
            engine._chk(self._lib.blsbn254_keyset_create_compressed(engine._ctx, pa, pb, ctypes.c_size_t(n_keys), pd, ctypes.c_size_t(len(pop_dst)),
                                                                    ctypes.byref(self._h)))
            return
        a, pa = _inbuf(pks, 128 * n_keys)
        if proofs is None:
            engine._chk(self._lib.blsbn254_keyset_create(engine._ctx, pa, ctypes.c_size_t(n_keys), ctypes.byref(self._h)))
        else:
            b, pb = _inbuf(proofs, 64 * n_keys); d, pd = _inbuf(pop_dst)
            engine._chk(self._lib.blsbn254_keyset_create_checked(engine._ctx, pa, pb, ctypes.c_size_t(n_keys), pd, ctypes.c_size_t(len(pop_dst)),
                                                                 ctypes.byref(self._h)))

    def checked(self):
        """True for a set registered with proofs of possession"""
        return bool(self._lib.blsbn254_keyset_checked(self._h))

    def set_weights(self, columns):
        """columns: 1 to 8 stake columns of n_keys unsigned 64-bit entries each (a list of sequences, or an (n_cols, n_keys)
        array).  Replaces an earlier table.  A column whose sum does not fit 64 bits raises Bn254Error and changes nothing."""
        cols = [[int(v) for v in col] for col in columns]
        n = self.count()
        if any(len(col) != n for col in cols):
            raise ValueError("a weight column must have %d entries" % n)
        if any(v < 0 or v >> 64 for col in cols for v in col):
            raise ValueError("a weight must fit 64 bits")
        w = np.array(cols, dtype=np.uint64).reshape(-1)
        if w.size == 0:
            w = np.zeros(1, dtype=np.uint64)
        self._eng._chk(self._lib.blsbn254_keyset_set_weights(self._eng._ctx, self._h, w.ctypes.data_as(_u64p), ctypes.c_size_t(len(cols))))
        self.n_cols = len(cols)

    def total_weight(self):
        """the columns' sums over the keys that have the KeyValidate bit: a list of n_cols ints"""
        o = (ctypes.c_uint64 * 8)()
        self._eng._chk(self._lib.blsbn254_keyset_total_weight(self._eng._ctx, self._h, o))
        return [int(o[q]) for q in range(self.n_cols)]

    def set_committees(self, committees):
        """committees: a list of index lists into the key set (1 to 65536 of them, none empty, no index twice within one list;
        lists may overlap).  Replaces an earlier table.  A violation raises Bn254Error and leaves the earlier table in place."""
        lists = [[int(i) for i in com] for com in committees]
        if any(i < 0 or i >> 32 for com in lists for i in com):
            raise ValueError("a member index must fit 32 bits")
        flat = np.array([i for com in lists for i in com] or [0], dtype=np.uint32)
        off = np.zeros(len(lists) + 1, dtype=np.uint64)
        if lists:
            off[1:] = np.cumsum([len(com) for com in lists], dtype=np.uint64)
        self._eng._chk(self._lib.blsbn254_keyset_set_committees(self._eng._ctx, self._h, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                                off.ctypes.data_as(_u64p), ctypes.c_size_t(len(lists))))
        self._com_sizes = [len(com) for com in lists]

    def committee_count(self):
        return int(self._lib.blsbn254_keyset_committee_count(self._h))

    def committee_total_weight(self):
        """per committee the columns' sums over its members that have the KeyValidate bit: an (n_com, n_cols) uint64 array, the
        weights of the rows that select every member"""
        sizes = getattr(self, "_com_sizes", [])
        rows = [bytes([0xff] * (n // 8) + ([0xff >> (8 - n % 8)] if n % 8 else [])) for n in sizes]
        return self._eng.keyset_committee_weight_batch(self, list(range(len(sizes))), rows)

    def count(self):
        return int(self._lib.blsbn254_keyset_count(self._h))

    def valid_bitmap(self):
        """KeyValidate per registered key: decodes, not the identity, on the curve, in the r-torsion"""
        n = self.count()
        o, po = _outbuf((n + 7) // 8)
        self._eng._chk(self._lib.blsbn254_keyset_valid(self._eng._ctx, self._h, po))
        return o[:(n + 7) // 8].tobytes()

    def close(self):
        if getattr(self, "_h", None) and getattr(self._eng, "_ctx", None):
            self._lib.blsbn254_keyset_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiEngine:
    """blsbn254_multi: one context per listed GPU, one host thread per context per call.
    An ordinal may be listed twice (two contexts on one GPU)."""

    def __init__(self, devices):
        self._lib = load_library()
        self._lib.blsbn254_multi_last_error.restype = ctypes.c_char_p
        self._lib.blsbn254_multi_ctx.restype = ctypes.c_void_p
        self._m = ctypes.c_void_p()
        devs = (ctypes.c_int * len(devices))(*devices)
        rc = self._lib.blsbn254_multi_create(devs, ctypes.c_int(len(devices)), ctypes.byref(self._m))
        if rc != 0:
            self._m = None
            raise Bn254Error(rc)
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_m", None):
            self._lib.blsbn254_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            detail = self._lib.blsbn254_multi_last_error(self._m).decode() if rc < 0 else ""
            raise _ERR.get(rc, Bn254Error)(rc, detail)

    def device_count(self):
        return int(self._lib.blsbn254_multi_device_count(self._m))

    def verify_batch(self, pks, msgs, sigs, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * n); d, pd = _inbuf(dst)
        o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch_multi(self._m, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd,
                                                        ctypes.c_size_t(len(dst)), po))
        return o[:(n + 7) // 8].tobytes()

    def verify_batch_rlc(self, pks, msgs, sigs, dst=DEFAULT_DST, seed=None):
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); s, ps = _inbuf(sigs, 64 * n); d, pd = _inbuf(dst)
        sd, psd = (None, ctypes.cast(None, _u8p)) if seed is None else _inbuf(seed, 32)
        o, po = _outbuf((n + 7) // 8)
        self._chk(self._lib.blsbn254_verify_batch_rlc_multi(self._m, pa, pm, off.ctypes.data_as(_u64p), ps, ctypes.c_size_t(n), pd,
                                                            ctypes.c_size_t(len(dst)), psd, po))
        return o[:(n + 7) // 8].tobytes()

    def aggregate_verify(self, pks, msgs, agg_sig, dst=DEFAULT_DST):
        n = len(msgs)
        data, off = pack_messages(msgs)
        a, pa = _inbuf(pks, 128 * n); m, pm = _inbuf(data); s, ps = _inbuf(agg_sig, 64); d, pd = _inbuf(dst)
        valid = ctypes.c_int(0)
        self._chk(self._lib.blsbn254_aggregate_verify_multi(self._m, pa, pm, off.ctypes.data_as(_u64p), ctypes.c_size_t(n), ps, pd,
                                                            ctypes.c_size_t(len(dst)), ctypes.byref(valid)))
        return bool(valid.value)

    def verify_batch_dev(self, d_pks, d_msgs, d_off, d_sigs, counts, d_full_bitmaps, dst=DEFAULT_DST):
        """Device-resident shards (lists of raw device pointers, one per device) -> the full bitmap on every device
        (RCCL all-reduce of the disjoint word arrays)."""
        g = len(self.devices)
        vp = lambda xs: (ctypes.c_void_p * g)(*xs)
        cnt = (ctypes.c_size_t * g)(*counts)
        d, pd = _inbuf(dst)
        self._chk(self._lib.blsbn254_verify_batch_multi_dev(self._m, vp(d_pks), vp(d_msgs), vp(d_off), vp(d_sigs), cnt, pd,
                                                            ctypes.c_size_t(len(dst)), vp(d_full_bitmaps)))
