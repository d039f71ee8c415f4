// kernels.h -- declarations of the phase kernels (defined in k_miller.hip, k_finalexp.hip, k_misc.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifndef BN_WAVES_PER_SIMD
#define BN_WAVES_PER_SIMD 1
#endif
#define BN_KERNEL __global__ void __launch_bounds__(256, BN_WAVES_PER_SIMD)

#if defined(__HIPCC__)
// One validity bit per tuple, written as the wave's 64-bit ballot: lanes 0..7 store one byte each (LSB-first bitmap).
// Every lane of the wave must call it (lanes past n pass bit = false).
__device__ inline void write_ballot(uint8_t* bitmap, size_t n, size_t i, bool bit) {
  unsigned long long m = __ballot(bit);
  unsigned lane = threadIdx.x & 63;
  size_t base = (i - lane) >> 3;                       // first byte of this wave's 64 tuples
  size_t nbytes = (n + 7) >> 3;
  if (lane < 8 && base + lane < nbytes) bitmap[base + lane] = (uint8_t)(m >> (8 * lane));
}
#endif

BN_KERNEL k_hash_to_g1(const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                       int32_t* h_ws, size_t h_stride, uint8_t* out_bytes, int mode);
BN_KERNEL k_hash_to_g2(const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                       uint8_t* out_bytes, int ro);
// the four hashing kernels under the expander xid != 0 (k_hash_keccak.hip, keccak.h EXPAND_*): k_hash_to_g1 / k_hash_to_g2 above,
// k_sign / k_hash_to_scalar below, with xid in front of their arguments.  BN_KERNEL_1: one wave per SIMD whatever the unit's policy
#define BN_KERNEL_1 __global__ void __launch_bounds__(256, 1)
BN_KERNEL k_hash_to_g1_x(uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                         int32_t* h_ws, size_t h_stride, uint8_t* out_bytes, int mode);
BN_KERNEL_1 k_hash_to_g2_x(uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                           uint8_t* out_bytes, int ro);
BN_KERNEL_1 k_sign_x(uint32_t xid, const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                     uint8_t* sigs, uint8_t* status);
BN_KERNEL k_hash_to_scalar_x(uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len, uint8_t* out);
// the G1 hashing kernels under the try-and-increment map (k_hash_tai.hip, lane_hash_tai.h G1MAP_*): k_hash_to_g1_x / k_sign_x with
// the map id in front; dst is accepted and ignored
BN_KERNEL k_hash_to_g1_tai(uint32_t map, uint32_t xid, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                           int32_t* h_ws, size_t h_stride, uint8_t* out_bytes, int mode);
BN_KERNEL_1 k_sign_tai(uint32_t map, uint32_t xid, const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                       uint8_t* sigs, uint8_t* status);
BN_KERNEL k_g1_check(const uint8_t* g1, size_t n, uint8_t* bitmap);
BN_KERNEL k_g2_check(const uint8_t* g2, size_t n, uint8_t* ok_bytes, uint8_t* bitmap);
BN_KERNEL k_miller_1(const uint8_t* g1, const uint8_t* g2, size_t n, int32_t* f_ws, size_t f_stride, uint8_t* status);
BN_KERNEL k_miller_hpk(const int32_t* h_ws, const uint8_t* pks, size_t n, int32_t* f_ws, size_t f_stride, uint8_t* flags);
BN_KERNEL k_miller_hpk2(const int32_t* h_ws, const uint8_t* pks, size_t n, int32_t* q_ws, int32_t* f_ws, size_t f_stride, uint8_t* flags);
BN_KERNEL k_miller_hpk2p(const int32_t* h_ws, size_t h_stride, const uint32_t* kid, const int32_t* table, const uint8_t* key_ok, size_t n,
                         int32_t* f_ws, size_t f_stride, uint8_t* flags, const uint8_t* skip);
BN_KERNEL k_miller_hpk1p(const int32_t* h_ws, size_t h_stride, const uint32_t* kid, const int32_t* table, const uint8_t* key_ok, size_t n,
                         int32_t* f_ws, size_t f_stride, uint8_t* flags, const uint8_t* skip);
BN_KERNEL k_g1_to_ws_batch(const uint8_t* g1, size_t n, int32_t* h_ws, uint8_t* status);
BN_KERNEL k_g1_to_ws(const uint8_t* g1, int32_t* h_ws, size_t slot, size_t stride, uint8_t* ok);
BN_KERNEL k_miller_verify(const uint8_t* pks, const uint8_t* sigs, const int32_t* h_ws, size_t n, int32_t* f_ws, uint8_t* flags);
BN_KERNEL k_fe_easy(const int32_t* in, int32_t* out, size_t n, size_t stride);
BN_KERNEL k_fe_easy_head(const int32_t* in, size_t n, size_t stride, int32_t* head, int32_t* nu);
BN_KERNEL k_fe_inv4(int32_t* nu, size_t n, size_t stride);
BN_KERNEL k_fe_easy_tail(const int32_t* in, int32_t* out, size_t n, size_t stride, const int32_t* head, const int32_t* nu);
BN_KERNEL k_fe_expx(const int32_t* in, int32_t* out, int32_t* slots, size_t n, size_t stride);
BN_KERNEL k_fe_expx_h1(const int32_t* in, int32_t* slots, size_t n, size_t stride, int32_t* a_out, int32_t* b_out);
BN_KERNEL k_fe_expx_h2(const int32_t* in, int32_t* slots, size_t n, size_t stride, int32_t* b_in, int32_t* c_out, int32_t* b2_out, int32_t* d2_out);
BN_KERNEL k_fe_h3(const int32_t* t, const int32_t* a, const int32_t* c, const int32_t* b2, const int32_t* x0, int32_t* tmp, size_t n, size_t stride,
                  const uint8_t* flags, const uint8_t* sub_ok, uint8_t* bitmap, uint8_t* gt_bytes, int* is_one, int mode);
__global__ void __launch_bounds__(128) k_miller_wide_prepared(const uint32_t* perm, const uint32_t* kid, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride,
                                                             const int32_t* table, const uint8_t* key_ok, size_t n, int32_t* f_ws, uint8_t* flags);
__global__ void __launch_bounds__(128) k_miller_wide_1p(const int32_t* h_ws, size_t h_stride, const uint32_t* kid, const int32_t* table, const uint8_t* key_ok, size_t n,
                                                       int32_t* f_ws, size_t f_stride, uint8_t* flags, const uint8_t* skip);
__global__ void __launch_bounds__(128) k_miller_wide_1(const uint8_t* g1, const uint8_t* g2, size_t n, int32_t* f_ws, size_t f_stride, uint8_t* status);
__global__ void __launch_bounds__(128) k_fe_hard_wide(const int32_t* t_ws, size_t n, size_t stride, const uint8_t* flags, const uint8_t* sub_ok,
                                                     uint8_t* one, uint8_t* gt_bytes, int* is_one, int mode);
BN_KERNEL k_fp12_from_bytes(const uint8_t* in, size_t n, int32_t* f_ws, size_t f_stride, uint8_t* status);
BN_KERNEL k_fp12_to_bytes(const int32_t* f_ws, size_t n, size_t stride, uint8_t* out);
BN_KERNEL k_fp12_mul_pairs(const int32_t* in, size_t n_in, size_t in_stride, int32_t* out, size_t out_stride);
BN_KERNEL k_g1_load(const uint8_t* g1, size_t n, int32_t* ws, uint8_t* status);
BN_KERNEL k_g1_add_pairs(const int32_t* in, size_t n_in, size_t in_stride, int32_t* out, size_t out_stride);
BN_KERNEL k_g1_to_bytes(const int32_t* ws, size_t stride, uint8_t* out);
BN_KERNEL k_sign(const uint8_t* sks, const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len,
                 uint8_t* sigs, uint8_t* status);
BN_KERNEL k_sk_to_pk(const uint8_t* sks, size_t n, uint8_t* pks, uint8_t* status);
BN_KERNEL k_g1_mul(const uint8_t* g1, const uint8_t* scalars, size_t n, uint8_t* out, uint8_t* status);
BN_KERNEL k_g2_mul(const uint8_t* g2, const uint8_t* scalars, size_t n, uint8_t* out, uint8_t* status);
BN_KERNEL k_g2_load(const uint8_t* g2, size_t n, int32_t* ws, uint8_t* ok);
BN_KERNEL k_g2_seg_sum(const int32_t* in_ws, size_t in_stride, const uint8_t* ok_in, const uint32_t* chunk_start, const uint32_t* chunk_len, size_t m,
                       int32_t* out_ws, size_t out_stride, uint8_t* ok_out);
BN_KERNEL k_pair_ok(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* ok);
BN_KERNEL k_fp12_seg_prod(const int32_t* in_ws, size_t in_stride, const uint8_t* ok_in, const uint32_t* chunk_start, const uint32_t* chunk_len,
                          size_t m, int32_t* out_ws, size_t out_stride, uint8_t* ok_out, int carry);
// aggregate verify over groups (k_aggregate_batch.hip): the missing half of a two-slot lane descriptor
#define AGB_NO_SLOT 0xffffffffu
BN_KERNEL k_agb_place_sigs(const uint8_t* sigs, size_t n_groups, int32_t* h_ws, size_t n_pairs, size_t h_stride, uint8_t* sig_ok);
BN_KERNEL k_miller_hpk2r(const int32_t* h_ws, size_t h_stride, const uint8_t* pks, size_t n_pairs, const uint32_t* slot_a, const uint32_t* slot_b,
                         size_t m, int32_t* q_ws, int32_t* f_ws, size_t f_stride, uint8_t* flags);
__global__ void __launch_bounds__(256) k_agb_fold(const uint32_t* slot_a, const uint32_t* slot_b, size_t m, size_t n_pairs, const uint8_t* flags,
                                                  const uint8_t* sub_ok, const uint8_t* sig_ok, const uint32_t* goff, uint8_t* ok);
BN_KERNEL k_g2p_to_bytes(const int32_t* ws, size_t stride, const uint8_t* ok, size_t m, uint8_t* out, int poison);
BN_KERNEL k_keygen(const uint8_t* ikm, size_t ikm_len, size_t n, const uint8_t* key_info, size_t key_info_len,
                   uint8_t* sks, uint8_t* status);
BN_KERNEL k_hash_to_scalar(const uint8_t* msgs, const uint64_t* off, size_t n, const uint8_t* dst, uint32_t dst_len, uint8_t* out);
BN_KERNEL k_iota_off(uint64_t* off, size_t n, uint64_t step);
BN_KERNEL k_g1_codec(const uint8_t* in, size_t n, uint8_t* out, uint8_t* status, int mode);
BN_KERNEL k_g2_codec(const uint8_t* in, size_t n, uint8_t* out, uint8_t* status, int mode);
// compressed -> uncompressed per element (k_inflate.hip, inflate.h): the bytes or the marker to out, 1 / 0 to status (may be null)
BN_KERNEL k_g1_inflate(const uint8_t* in, size_t n, uint8_t* out, uint8_t* status);
BN_KERNEL k_g2_inflate(const uint8_t* in, size_t n, uint8_t* out, uint8_t* status);
BN_KERNEL k_rlc_prep(const uint8_t* pks, const uint8_t* sigs, const int32_t* h_ws, const uint8_t* sub_ok, const uint8_t* seed,
                     size_t n, size_t n_pad, int32_t* a_ws, int32_t* b_ws, uint8_t* elig);
BN_KERNEL k_fp12_mask_one(int32_t* f_ws, size_t stride, const uint8_t* elig, size_t n_pad);
BN_KERNEL k_fp12_mul_elem(int32_t* a, size_t sa, const int32_t* b, size_t sb, size_t m);
BN_KERNEL k_g1p_to_bytes(const int32_t* ws, size_t stride, size_t m, uint8_t* out);
BN_KERNEL k_rlc_gather(const uint32_t* idx, size_t m, const uint8_t* pks, const uint8_t* sigs, const int32_t* h_ws, size_t n,
                       const uint8_t* sub_ok, uint8_t* c_pks, uint8_t* c_sigs, int32_t* c_h, uint8_t* c_sub);
BN_KERNEL k_rlc2_prep(const uint32_t* perm, const uint8_t* pks, const uint8_t* sigs, const int32_t* h_ws, size_t n, const uint8_t* seed,
                      int32_t* a_ws, int32_t* b_ws, uint8_t* sig_ok);
__global__ void k_rlc2_chunk_counts(const uint32_t* hist, uint32_t u, uint32_t G, uint32_t* cnt);
__global__ void k_rlc2_mark(const uint32_t* perm, const uint32_t* kid, const uint32_t* hist, const uint32_t* run_end, const uint32_t* chunk_base,
                            uint32_t n, uint32_t G, uint32_t* tuple_chunk, uint32_t* chunk_kid, uint32_t* chunk_start, uint32_t* chunk_len);
BN_KERNEL k_rlc2_sum(const int32_t* a_ws, const int32_t* b_ws, size_t n, const uint8_t* sig_ok, const uint32_t* chunk_start, const uint32_t* chunk_len,
                     size_t m, int32_t* sa_ws, int32_t* sb_ws, uint32_t* elig_out);
__global__ void k_rlc2_key_elig(const uint32_t* chunk_kid, const uint32_t* chunk_elig, uint32_t m, uint32_t* key_elig);
BN_KERNEL k_rlc2_virtual(const int32_t* sa_ws, const int32_t* sb_ws, size_t stride, const uint32_t* elig, const uint32_t* list, size_t cnt,
                         uint8_t* c_sig, int32_t* c_h, uint8_t* c_state);
__global__ void k_rlc2_keys_pass(const uint8_t* key_ok, const uint8_t* state, const uint8_t* isone, uint32_t u, uint8_t* key_pass, int* all_pass);
__global__ void __launch_bounds__(256) k_rlc2_chunk_need(const uint32_t* chunk_kid, const uint8_t* key_pass, uint32_t m, uint8_t* need, uint32_t* block_cnt);
__global__ void k_rlc2_chunk_pass(const uint32_t* list, const uint8_t* state, const uint8_t* isone, const uint8_t* flags, uint32_t cnt, uint8_t* chunk_pass);
__global__ void k_rlc2_valid_fast(const uint32_t* perm, const uint32_t* kid, const uint8_t* sig_ok, const uint8_t* key_ok, uint32_t n, uint8_t* valid);
__global__ void k_iota_u32(uint32_t* out, uint32_t n);
__global__ void __launch_bounds__(256) k_rlc2_resolve(const uint32_t* perm, const uint32_t* kid, const uint32_t* tuple_chunk, const uint8_t* sig_ok,
                                                      const uint8_t* key_ok, const uint8_t* chunk_pass, uint32_t n, uint8_t* valid, uint8_t* need, uint32_t* block_cnt);
__global__ void __launch_bounds__(256) k_rlc2_compact(const uint8_t* need, const uint32_t* perm, uint32_t n, const uint32_t* block_base, uint32_t* list);
BN_KERNEL k_g1_seg_sum(const int32_t* in_ws, size_t in_stride, const uint32_t* perm, const uint32_t* chunk_start, const uint32_t* chunk_len, size_t m,
                       int32_t* out_ws, size_t out_stride);
BN_KERNEL k_g1p_to_h_affine(const int32_t* in_ws, size_t in_stride, size_t u, int32_t* h_ws, size_t h_stride, uint8_t* status);
BN_KERNEL k_field_op(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, uint8_t* status);
BN_KERNEL k_gt_pow(const uint8_t* gt, const uint8_t* scalars, size_t n, uint8_t* out, uint8_t* status);
BN_KERNEL k_fr_decode(const uint8_t* ids, size_t t, int32_t* x_ws, uint8_t* status);
__global__ void k_kd_insert(const uint8_t* pks, uint32_t n, uint32_t* slots, uint32_t mask, uint32_t seed, uint32_t* rep);
__global__ void k_kd_assign(const uint32_t* rep, uint32_t n, uint32_t* kid, uint32_t* counter, uint32_t* keys);
__global__ void __launch_bounds__(256) k_kd_propagate(const uint32_t* rep, uint32_t n, uint32_t u, uint32_t* kid, uint32_t* hist);
__global__ void k_kd_hist(const uint32_t* kid, uint32_t n, uint32_t u, uint32_t* hist, int* bad);
__global__ void __launch_bounds__(1024) k_scan_excl(const uint32_t* hist, uint32_t u, uint32_t* cursor);
__global__ void __launch_bounds__(256) k_kd_scatter(const uint32_t* kid, uint32_t n, uint32_t u, uint32_t* cursor, uint32_t* perm);
BN_KERNEL k_g2_prepare(const uint8_t* pks, const uint32_t* keys, uint32_t u, int32_t* table, uint8_t* key_ok, const uint32_t* d_u);
BN_KERNEL k_g2_prepare_quad(const uint8_t* pks, const uint32_t* keys, uint32_t u, int32_t* table, uint8_t* key_ok, const uint32_t* d_u);
BN_KERNEL k_g2_expand(const int32_t* raw, uint32_t u, int32_t* expanded, const uint32_t* d_u, uint8_t* key_ok);
__global__ void k_kd_decide(const uint32_t* cnt, uint32_t n, uint32_t cap, int small, uint32_t* res);
__global__ void k_prep_unsort(const uint8_t* is_one, const uint8_t* flags, const uint32_t* perm, uint32_t n, uint8_t* valid);
__global__ void __launch_bounds__(256) k_pack_bitmap(const uint8_t* valid, size_t n, uint8_t* bitmap);
BN_KERNEL k_miller_prepared(const uint32_t* perm, const uint32_t* kid, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride,
                            const int32_t* table, const uint8_t* key_ok, size_t n, int32_t* f_ws, uint8_t* flags);
BN_KERNEL k_miller_tri_prepared(const uint32_t* perm, const uint32_t* kid, const uint8_t* sigs, const int32_t* h_ws, size_t h_stride,
                                const int32_t* table, const uint8_t* key_ok, size_t n, int32_t* f_ws, uint8_t* flags);
BN_KERNEL k_miller_tri_1(const uint8_t* g1, const uint8_t* g2, size_t n, int32_t* f_ws, size_t f_stride, uint8_t* status);
BN_KERNEL k_miller_tri_1p(const int32_t* h_ws, size_t h_stride, const uint32_t* kid, const int32_t* table, const uint8_t* key_ok, size_t n,
                          int32_t* f_ws, size_t f_stride, uint8_t* flags, const uint8_t* skip);
BN_KERNEL k_fe_tri_hard(const int32_t* t_ws, size_t n, size_t stride, int32_t* vals, const uint8_t* flags, const uint8_t* sub_ok,
                        uint8_t* one, uint8_t* gt_bytes, int* is_one, int mode);
BN_KERNEL k_lagrange_partial(const int32_t* x_ws, size_t t, size_t J, int32_t* pnum, int32_t* pden, uint8_t* dup);
BN_KERNEL k_lagrange_finish(const int32_t* pnum, const int32_t* pden, size_t t, size_t S, uint8_t* scalars, uint32_t* glv_ws);
BN_KERNEL k_msm_window(const uint8_t* g1, const uint32_t* glv_ws, size_t t, int32_t* part, uint8_t* status);
__global__ void __launch_bounds__(64) k_msm_finish(const int32_t* part, size_t n_chunks, uint8_t* out);
BN_KERNEL k_msm_fold(const int32_t* in, size_t n_in, int32_t* out);
BN_KERNEL k_lagrange_seg(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, uint32_t t_big,
                         uint8_t* scalars, uint32_t* glv_ws, uint32_t* gid, uint32_t* gstat);
BN_KERNEL k_g1_smul_glv(const uint8_t* g1, const uint32_t* glv_ws, const uint32_t* gid, size_t m, int32_t* out_ws, uint32_t* gstat);
__global__ void __launch_bounds__(256) k_th_finish(const uint32_t* gstat, size_t n_groups, uint8_t* out, uint8_t* status);
BN_KERNEL k_fr_coef_decode(const uint8_t* coeffs, size_t T, int32_t* cf_ws, uint8_t* cf_ok);
BN_KERNEL k_fr_poly_eval(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, const uint32_t* coff, uint32_t ng,
                         const int32_t* cf_ws, size_t T, int32_t* r_ws, size_t N, uint32_t* gstat);
BN_KERNEL k_g2_poly_eval(const int32_t* x_ws, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, const uint32_t* coff, uint32_t ng,
                         const int32_t* c_ws, size_t T, int nbits, int32_t* r_ws, size_t N, uint32_t* gstat);
BN_KERNEL k_td_fr_encode(const int32_t* r_ws, size_t N, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, const uint32_t* gstat, uint8_t* out);
BN_KERNEL k_td_g2_encode(const int32_t* r_ws, size_t N, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, const uint32_t* gstat, uint8_t* out);
__global__ void __launch_bounds__(256) k_td_finish(uint32_t* gstat, size_t n_groups, const uint32_t* coff, const uint8_t* ok_a, const uint8_t* ok_b, uint32_t mark,
                                                  uint8_t* status);
__global__ void __launch_bounds__(64) k_g2gen_table(int32_t* tab);
BN_KERNEL k_td_key_check(const uint8_t* shares, size_t m, uint32_t lo, const int32_t* tab, const int32_t* r_ws, size_t N, uint8_t* share_ok);
__global__ void __launch_bounds__(256) k_td_key_bits(const uint8_t* share_ok, size_t N, const uint32_t* goff, uint32_t ng, const uint32_t* gstat, uint8_t* bitmap);
BN_KERNEL k_tc_scan(const uint8_t* ids, const uint8_t* sigs, const uint8_t* id_ok, size_t m, uint32_t lo, const uint32_t* goff, uint32_t ng, uint32_t* gstat,
                    uint8_t* cand);
__global__ void __launch_bounds__(256) k_tc_select(const uint8_t* bits_a, const uint8_t* bits_b, size_t m, uint32_t lo, const uint32_t* goff, const uint32_t* coff,
                                                  uint32_t ng, uint32_t* gstat, const uint32_t* ids, const uint32_t* sigs, uint32_t* c_ids, uint32_t* c_sigs,
                                                  uint8_t* used);
__global__ void __launch_bounds__(256) k_tc_gather_c0(const uint32_t* commitments, const uint32_t* coff, const uint32_t* goff, size_t n_groups, uint32_t* gstat,
                                                     uint32_t* keys);
// sums over a registered key set selected by bitmaps (k_keyset.hip)
BN_KERNEL k_ks_register(uint8_t* pks, uint32_t n_keys, const uint8_t* sub_ok, const uint8_t* mask, int32_t* aff, uint32_t* bad, uint32_t* skip, uint8_t* valid);
BN_KERNEL k_ks_count(const uint8_t* sel, size_t G, uint32_t n_keys, const uint32_t* bad, uint8_t* flip, uint8_t* ok);
BN_KERNEL k_ks_word_sum(const int32_t* aff, uint32_t n_keys, const uint32_t* skip, const uint8_t* sel, const uint8_t* flip, size_t G,
                        int32_t* out, size_t out_stride);
BN_KERNEL k_ks_group_sum(const int32_t* in, size_t in_stride, uint32_t cnt, size_t G, const uint8_t* flip, const uint8_t* ok, const int32_t* total,
                         int last, int32_t* out, size_t out_stride, uint8_t* ok_out);
// checked signature aggregation over a registered key set (k_keyset_agg.hip)
BN_KERNEL k_ka_scan(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand,
                    int32_t* pts);
__global__ void __launch_bounds__(256) k_ka_rows(const uint32_t* idx, const uint8_t* cand, const uint32_t* goff, size_t m, size_t lo, uint32_t n_keys, uint8_t* rows);
__global__ void __launch_bounds__(256) k_ka_gather_keys(const uint4* enc, const uint32_t* idx, size_t m, uint4* out);
// checked merge of partial aggregates over a registered key set (k_keyset_merge.hip)
BN_KERNEL k_km_sig(const uint8_t* sigs, size_t m, uint32_t lo, size_t N, uint8_t* sig_ok, int32_t* pts);
__global__ void __launch_bounds__(256) k_km_select(const uint8_t* rows, const uint8_t* sig_ok, const uint8_t* mask, const uint32_t* goff, const uint32_t* valid,
                                                  uint32_t n_keys, size_t g_lo, size_t m, uint8_t* flags, uint8_t* urows);
BN_KERNEL k_km_points(const uint8_t* flags, size_t m, uint32_t lo, size_t N, int32_t* pts, uint8_t* used, uint8_t* cand);
// stake weights over a registered key set selected by bitmaps (k_keyset_weight.hip)
__global__ void __launch_bounds__(256) k_ks_weight(const uint8_t* rows, const uint32_t* vwords, const uint64_t* tab, uint32_t n_keys, uint32_t n_cols, size_t g_lo,
                                                  size_t m, uint64_t* out);
// committees over a registered key set (k_keyset_committee.hip)
BN_KERNEL k_kc_words(const uint32_t* members, const uint4* coms, const uint32_t* wcom, size_t n_words, const uint32_t* bad, const uint32_t* skip,
                     const uint32_t* vwords, uint32_t* cbad, uint32_t* cskip, uint32_t* cvalid);
BN_KERNEL k_kc_count(const uint8_t* sel, const uint64_t* srow, const uint32_t* scom, const uint4* coms, const uint32_t* cbad, size_t lo, size_t m, int noflip,
                     uint8_t* flip, uint8_t* ok);
BN_KERNEL k_kc_word_sum(const int32_t* aff, uint32_t n_keys, const uint32_t* members, const uint4* coms, const uint32_t* cskip, const uint4* items, const uint8_t* sel,
              const uint64_t* srow, const uint32_t* scom, const uint32_t* spbase, const uint8_t* flip, int32_t* out, size_t out_stride);
BN_KERNEL k_kc_finish(const int32_t* u, size_t u_stride, size_t G, const uint32_t* scom, const uint32_t* order, const int32_t* totals, size_t n_com,
                      const uint8_t* flip, const uint8_t* ok, int32_t* out, size_t out_stride, uint8_t* ok_out);
__global__ void __launch_bounds__(256) k_kc_weight(const uint8_t* rows, const uint64_t* grow, const uint32_t* gcom, const uint4* coms, const uint32_t* members,
                                                  const uint32_t* cvalid, const uint64_t* tab, uint32_t n_cols, size_t g_lo, size_t m, uint64_t* out);
// checked signature aggregation per committee of a registered key set (k_keyset_committee_agg.hip)
BN_KERNEL k_kca_scan(const uint32_t* cvalid, const uint4* coms, const uint32_t* com, const uint32_t* goff, uint32_t ng, const uint32_t* pos, const uint8_t* sigs,
                     const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand, int32_t* pts);
__global__ void __launch_bounds__(256) k_kca_rows(const uint32_t* pos, const uint8_t* cand, const uint32_t* goff, const uint64_t* wpre, const uint64_t* roff,
                                                 const uint4* coms, const uint32_t* com, uint32_t ng, size_t m, uint64_t lo, uint8_t* rows);
__global__ void __launch_bounds__(256) k_kca_resolve(const uint32_t* members, const uint4* coms, const uint32_t* com, const uint32_t* goff, uint32_t ng,
                                                    const uint32_t* pos, size_t m, uint32_t lo, uint32_t* idx);
// checked merge of partial aggregates per committee of a registered key set (k_keyset_committee_merge.hip)
__global__ void __launch_bounds__(256) k_kcm_select(const uint8_t* rows, const uint8_t* sig_ok, const uint8_t* mask, const uint32_t* goff, const uint32_t* com,
                                                   const uint4* coms, const uint32_t* cvalid, const uint64_t* rbase, const uint64_t* roff, size_t g_lo, size_t m,
                                                   uint8_t* flags, uint8_t* urows);
// the checked aggregation and merge calls in wire format (k_keyset_wire.hip): the scans for 32-byte entries, a sum in both encodings
BN_KERNEL k_ka_scan_wire(const uint8_t* key_valid, const uint32_t* idx, const uint8_t* sigs, const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand,
                         int32_t* pts);
BN_KERNEL k_kca_scan_wire(const uint32_t* cvalid, const uint4* coms, const uint32_t* com, const uint32_t* goff, uint32_t ng, const uint32_t* pos, const uint8_t* sigs,
                          const uint8_t* mask, size_t m, uint32_t lo, size_t N, uint8_t* cand, int32_t* pts);
BN_KERNEL k_g1p_to_wire(const int32_t* ws, size_t stride, size_t m, uint8_t* full, uint8_t* wire);
// key-set FastAggregateVerify by random linear combination per message (k_keyset_rlc.hip)
BN_KERNEL k_ksr_elig(const uint8_t* rows, const uint64_t* row_off, uint32_t n_keys, const uint32_t* com, const uint4* coms, const uint32_t* skip,
                     const uint32_t* valid, const int32_t* sums, const uint8_t* sum_ok, size_t G, const uint8_t* sigs, const uint8_t* seed,
                     const uint8_t* multi, uint8_t* elig, uint64_t* wt);
BN_KERNEL k_ksr_weigh_g1(const uint8_t* sigs, const uint8_t* elig, const uint64_t* wt, const uint32_t* pos, size_t G, int32_t* a_ws);
BN_KERNEL k_ksr_weigh_g2(const int32_t* sums, const uint8_t* elig, const uint64_t* wt, const uint32_t* pos, size_t G, int32_t* b_ws);
BN_KERNEL k_ksr_chunks(const int32_t* sa, const int32_t* sb, size_t M, const uint32_t* cstart, const uint32_t* clen, const uint32_t* order,
                       const uint8_t* elig, uint32_t* cnt, uint8_t* state, uint8_t* sa_bytes);
__global__ void __launch_bounds__(256) k_ksr_gather(const uint32_t* list, size_t m, const int32_t* pts, size_t pts_stride, const uint8_t* ok, const uint8_t* sigs,
                                                   int32_t* c_pts, uint8_t* c_ok, uint8_t* c_sigs);
// aggregate verify over ragged groups by random linear combination (k_aggregate_rlc.hip)
BN_KERNEL k_agr_group(const uint8_t* sigs, const uint32_t* goff, const uint32_t* kid, const uint8_t* key_ok, const uint8_t* seed, size_t G, uint8_t* sig_ok,
                      uint8_t* elig, uint2* wt, int32_t* w_ws, size_t W, size_t col0);
BN_KERNEL k_agr_weigh(const int32_t* h_ws, size_t N, const uint32_t* gidx, const uint8_t* elig, const uint2* wt, int32_t* w_ws, size_t W);
__global__ void __launch_bounds__(256) k_agr_items(const uint32_t* gidx, const uint32_t* kid, const uint32_t* seg_of, size_t N, size_t G, uint32_t u, uint32_t S,
                                                  int32_t* w_ws, size_t W, uint32_t* vkid, uint32_t* mkid);
__global__ void __launch_bounds__(256) k_agr_bits(const uint8_t* elig, const uint32_t* seg_of, const uint8_t* isone, size_t G, uint8_t* valid);
// pairing-product checks over ragged groups by random linear combination (k_pairing_check_rlc.hip)
BN_KERNEL k_pcr_pairs(const uint8_t* g1, const uint8_t* g2, const uint32_t* kid, const uint8_t* key_ok, size_t N, int32_t* p_ws, uint8_t* flag);
BN_KERNEL k_pcr_eq(const uint32_t* goff, const uint8_t* flag, const uint8_t* seed, size_t G, uint8_t* elig, uint2* wt);
BN_KERNEL k_pcr_weigh(const int32_t* p_ws, size_t N, const uint32_t* gidx, const uint8_t* flag, const uint8_t* elig, const uint2* wt, int32_t* w_ws, size_t W);
__global__ void __launch_bounds__(256) k_pcr_items(const uint32_t* gidx, const uint32_t* kid, const uint32_t* seg_of, size_t N, uint32_t u, uint32_t S,
                                                  int32_t* w_ws, size_t W, uint32_t* vkid, uint32_t* mkid);
__global__ void __launch_bounds__(256) k_valu_peak(uint32_t* out, uint32_t seed, int iters, int kind, uint64_t* stamps);
__global__ void k_status_reduce(const uint8_t* status, size_t n, uint8_t want_mask, uint8_t want_val, int* first_bad);
__global__ void k_and_reduce(const uint8_t* flags, const uint8_t* sub_ok, size_t n, int* all_ok);
